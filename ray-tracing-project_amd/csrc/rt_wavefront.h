// rt_wavefront.h -- the wavefront path of rt_trace_stream_color (RT_RAYS_WAVEFRONT): traceRay's level loop
// (rt_trace_ray.h k_render_depth / trace_depth) cut into stage kernels, so that the rays of every stage can be regrouped into
// packets of their own. Included only by rt_rays.hip, which holds the host glue (enqueue_wavefront).
//
// Level d = 0 .. D-1 of a call (D = max_depth, FULL = shadow rays and at least one light):
//   closest   k_wf_closest over the live list L_d: closest hit, hit_normal; FULL: the hit goes to the state and the
//             stage ends there; otherwise the shading has no traversal and is fused in (calc_color<false>, the ks
//             update, the reflection ray as the ray of level d + 1)
//   regroup   the hits of L_d -> H_d (FULL), or straight to L_(d+1) (fused)
//   shade     FULL only: k_wf_shade over H_d: calc_color<true> -- the any-hit walks now run over packets of
//             regrouped hit points --, direct[d], the ks update, the reflection ray
//   regroup   H_d -> L_(d+1) (RT_RAYS_REORDER only: without it L_(d+1) is H_d)
// then k_wf_resolve folds direct[] with the final ks and writes rgb3 / face / t at each ray's own index.
//
// Regrouping. A list holds ray indices; a stage's packet w takes entries 64 w .. 64 w + 63 of its list and every
// lane reads and writes the state of the ray its entry names, so a ray's arithmetic is its lane's alone and any
// grouping gives the same bits. Without RT_RAYS_REORDER the hits are compacted in list order (hipcub
// DeviceSelect::Flagged on the flags the stage wrote per entry). With it the stage writes a coherence key per
// entry (rt_raykey.h: the closest stage of level d + 1 from the new ray's origin and direction, the shade stage
// from the hit point and the direction to the first light, the SHADOW key; a dead entry 0xFFFFFFFF, after every
// live key) and a stable radix sort of (key, ray) orders the next list: a pure function of the inputs.
// No count comes back to the host: every stage is launched for the upper bound n, reads its list's length from
// counts[] through a wave-uniform load, and its packets beyond that length only mark their entries dead.
// counts[0] = n, counts[d + 1] = the hits of level d = the live rays of level d + 1 (one integer atomic add per
// wave of the closest stage: a sum, so the same on every run; rt_debug_ray_levels reads these words).
//
// Scratch per ray (scene-owned, rt_scene.h RayScratch::d_wf; WfState below):
//   24 B  the current ray (origin, direction) of levels >= 1; level 0 reads the caller's list
//   32 B  the hit: point, normal, material, face
//   40 B  MatState ka, kd, ks, Ns -- carried across levels as the in-order loop carries `st`
//   12 B  first-hit face and t, the number of hit levels
//   16 B  two lists and two key (or flag) arrays of one word each
//   12 B  direct[d], per level d < D
// = 124 + 12 D bytes (172 B at D = 4, 316 B at D = 16), plus hipcub's temporary storage (a few bytes per ray) and,
// with RT_RAYS_REORDER, the 16 B of level 0's sort (rt_rays.hip ScratchView).
#pragma once
#include "rt_trace_ray.h"
#include "rt_raykey.h"

namespace rt {

constexpr uint32_t kWfDeadKey = 0xFFFFFFFFu;  // above every ray_key (bit 31 set alone marks a degenerate ray)
constexpr size_t wf_bytes_per_ray(int D) { return 124 + 12 * (size_t)D; }

struct WfState {
  float *o, *d;          // [n][3] the ray of the next level (levels >= 1 read it)
  float *hp, *hn;        // [n][3] hit point, normal
  int32_t* hmat;         // [n]
  uint32_t* hface;       // [n]
  float *ka, *kd, *ks;   // [n][3]
  float* ns;             // [n]
  int32_t* face0;        // [n] first hit (-1: miss)
  float* t0;             // [n]
  int32_t* levels;       // [n] levels with a hit
  float* direct;         // [D][n][3]
  uint32_t *list_a, *list_b, *key_a, *key_b;  // [n] each
};

struct WfParams {
  WfState s;
  const float *ro, *rd;      // the stage's rays [n][3]: the caller's list at level 0, s.o / s.d after it
  const uint32_t* list;      // the stage's list (null: entry k is ray k)
  uint32_t* mark;            // [n] per entry: flag (1 = hit) or key for the regroup after this stage; null: none
  uint32_t* counts;          // [RT_MAX_TRACE_DEPTH + 1]
  const float* bounds;       // [6] the key grid (RT_RAYS_REORDER), else null: mark holds flags
  int32_t n, level, D, origin_major;
};

__device__ __forceinline__ void st3(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }

__device__ __forceinline__ MatState wf_load_mat(const WfState& s, size_t i) {
  return MatState{ld3(s.ka + 3 * i), ld3(s.kd + 3 * i), ld3(s.ks + 3 * i), s.ns[i]};
}
__device__ __forceinline__ void wf_store_mat(const WfState& s, size_t i, const MatState& m) {
  st3(s.ka + 3 * i, m.ka);
  st3(s.kd + 3 * i, m.kd);
  st3(s.ks + 3 * i, m.ks);
  s.ns[i] = m.ns;
}

__device__ __forceinline__ uint32_t wf_key(const WfParams& W, f3 o, f3 d) {
  const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
  float b[6];
  for (int k = 0; k < 6; k++) b[k] = W.bounds[k];
  return ray_key(oo, dd, b, W.origin_major != 0);
}

// the lane's entry of the stage's list, or the packet's exit: packets past the live count mark their entries dead
// (flag 0 / the dead key) and leave. count: counts word of this stage's list.
struct WfLane {
  int base, lane, wv;
  bool active;
  uint32_t i;  // the lane's ray (inactive lanes alias the packet's first)
};
__device__ __forceinline__ bool wf_lane(const WfParams& W, uint32_t count_word, WfLane& c) {
  c.lane = threadIdx.x & 63;
  c.wv = (int)uniform(threadIdx.x >> 6);
  c.base = (int)uniform((blockIdx.x * 4 + (threadIdx.x >> 6)) * 64);
  if (c.base >= W.n) return false;
  const int count = (int)uniform(W.counts[count_word]);
  const uint32_t dead = W.bounds ? kWfDeadKey : 0u;
  if (c.base >= count) {
    if (W.mark && c.base + c.lane < W.n) W.mark[c.base + c.lane] = dead;
    return false;
  }
  c.active = c.base + c.lane < count;
  if (W.mark && !c.active && c.base + c.lane < W.n) W.mark[c.base + c.lane] = dead;
  const int e = c.active ? c.base + c.lane : c.base;
  c.i = W.list ? W.list[e] : (uint32_t)e;
  return true;
}

// the ks update and the reflection ray after level `level`'s shading of a hit lane (traceRay :355-363), written as
// the ray of the next level, with its entry's mark for the regroup that follows (1, or the ray's closest key); the
// reflection ray is counted (ST_TOTAL) by the closest stage that traces it
__device__ __forceinline__ void wf_finish_level(const FrameParams& P, const WfParams& W, const WfLane& c, const Ray& cur,
                                                const HitInfo& hi, MatState st, f3 dc) {
  const size_t i = c.i;
  st3(W.s.direct + 3 * ((size_t)W.level * (size_t)W.n + i), dc);
  W.s.levels[i] = W.level + 1;
  if (hi.mat != -1) st.ks = load_mat(P.sc.mats[hi.mat]).ks;  // traceRay :355-358
  wf_store_mat(W.s, i, st);
  if (W.level + 1 == W.D) return;
  // reflect(dir.normalized(), interpolateNormal(...)), offset 0.001 (flyscene.cpp:361-363)
  const f3 rd = reflect(normalized(cur.d), hi.n);
  const f3 ro = offset(hi.p, rd, 0.001f);
  st3(W.s.o + 3 * i, ro);
  st3(W.s.d + 3 * i, rd);
  if (W.mark) W.mark[c.base + c.lane] = W.bounds ? wf_key(W, ro, rd) : 1u;
}

// Closest stage of level W.level over the list of counts[level] entries. FIRST: level 0 (the caller's rays, the
// octant-specialised walk of the in-order loop's level 0, the first hit's outputs, the default material); an
// instantiation of its own, so that a level's kernel holds one traversal. FUSED: PRIMARY mode or no lights -- the
// shading is done here and the hits are the next level's rays.
// LSRC: LS_KERNARG, or LS_MEMORY for a light set read from device memory (rt_trace_stream_lit): the fused shading
// has no shadow packets and hence no occluder cache, the shade stage's key reads the set's first light.
template <bool FIRST, bool FUSED, bool STATS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(256) void k_wf_closest(FrameParams P, WfParams W) {
  __shared__ WaveLds<TRAV_B2_LDS, STATS> lds;
  WfLane c;
  if (!wf_lane(W, (uint32_t)W.level, c)) return;
  const size_t i = c.i;
  const int d = W.level;
  uint32_t cnt_[STATS ? ST_COUNT : 1] = {};
  uint32_t* const cnt = STATS ? cnt_ : nullptr;
  Ray cur;
  cur.o = ld3(W.ro + 3 * i);
  cur.d = ld3(W.rd + 3 * i);
  cur.o2 = affv3(P.Minv, cur.o);
  setup_cull(cur, P.sc.static_pad);
  if (STATS && c.active) {
    if (FIRST) cnt[ST_RAYS]++;
    cnt[ST_TOTAL]++;
  }
  Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  bool dummy = false;
  if (FIRST) trace_oct<false, STATS, TRAV_B2_LDS>(P.sc, cur, c.active, h, dummy, lds, c.wv, cnt);
  else trace<false, STATS, TRAV_B2_LDS>(P.sc, cur, c.active, h, dummy, lds, c.wv, cnt);
  const bool hit = c.active && h.t != INFINITY;
  if (STATS && FIRST && hit) cnt[ST_HITS]++;
  HitInfo hi;
  hi.mat = -1;
  hi.face = 0xFFFFFFFFu;
  hi.p = f3{0.0f, 0.0f, 0.0f};
  hi.n = f3{0.0f, 0.0f, 0.0f};
  if (hit) {
    const TriRec64 tr = vload_tri(P.sc.tris, h.slot);
    hi.face = tr.face;
    hi.p = f3{cur.o.x + h.t * cur.d.x, cur.o.y + h.t * cur.d.y, cur.o.z + h.t * cur.d.z};
    hi.n = hit_normal(P.sc, tr, h.slot, hi.p, hi.mat);
  }
  if (FIRST && c.active) {
    W.s.face0[i] = hit ? (int32_t)hi.face : -1;
    W.s.t0[i] = h.t;
    W.s.levels[i] = 0;
  }
  const uint32_t nh = (uint32_t)__popcll(ballot(hit));
  if (c.lane == 0 && nh) atomicAdd(W.counts + d + 1, nh);
  if (FUSED) {
    MatState st = FIRST ? load_mat(P.defmat) : wf_load_mat(W.s, i);
    const f3 dc = calc_color<false, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, hit, &lds, c.wv, cnt);
    if (hit) wf_finish_level(P, W, c, cur, hi, st, dc);
    else if (c.active && W.mark) W.mark[c.base + c.lane] = W.bounds ? kWfDeadKey : 0u;
  } else {
    if (hit) {
      st3(W.s.hp + 3 * i, hi.p);
      st3(W.s.hn + 3 * i, hi.n);
      W.s.hmat[i] = hi.mat;
      W.s.hface[i] = hi.face;
      if (FIRST) wf_store_mat(W.s, i, load_mat(P.defmat));
    }
    if (c.active) {  // the shade stage's key: the hit point and the direction to calculateColor's first light
      uint32_t m = W.bounds ? kWfDeadKey : 0u;
      if (hit) m = W.bounds ? wf_key(W, hi.p, light_dir(hi.p, LSRC == LS_KERNARG ? frame_light(0) : set_light(P, 0))) : 1u;
      W.mark[c.base + c.lane] = m;
    }
  }
  if (STATS) flush_stats(P, cnt, c.lane);
}

// Shade stage of level W.level (FULL with lights) over the hit list of counts[level + 1] entries
// LSRC: calc_color's light source (LS_MEMORY_CACHED / LS_MEMORY for a light set read from device memory)
template <bool STATS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEu)))
void k_wf_shade(FrameParams P, WfParams W) {
  __shared__ WaveLds<TRAV_B2_LDS, STATS> lds;
  WfLane c;
  if (!wf_lane(W, (uint32_t)W.level + 1u, c)) return;
  const size_t i = c.i;
  uint32_t cnt_[STATS ? ST_COUNT : 1] = {};
  uint32_t* const cnt = STATS ? cnt_ : nullptr;
  Ray cur;  // calc_color and the reflection read the level's ray: its origin and direction only
  cur.o = ld3(W.ro + 3 * i);
  cur.d = ld3(W.rd + 3 * i);
  HitInfo hi;
  hi.p = ld3(W.s.hp + 3 * i);
  hi.n = ld3(W.s.hn + 3 * i);
  hi.mat = W.s.hmat[i];
  hi.face = W.s.hface[i];
  MatState st = wf_load_mat(W.s, i);
  const f3 dc = calc_color<true, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, c.active, &lds, c.wv, cnt);
  if (c.active) wf_finish_level(P, W, c, cur, hi, st, dc);
  if (STATS) flush_stats(P, cnt, c.lane);
}

// the colour of every ray from its levels' direct colours, deepest hit level upwards with the final ks
// (k_render_depth's fold); the background for a primary miss; written at the ray's own index
__global__ __launch_bounds__(256) void k_wf_resolve(FrameParams P, WfParams W, float* __restrict__ rgb,
                                                    int32_t* __restrict__ face, float* __restrict__ t) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)W.n) return;
  const int levels = W.s.levels[i];
  f3 col{0.0f, 0.0f, 0.0f};
  if (levels > 0) {
    const f3 ks = ld3(W.s.ks + 3 * i);
    for (int d = levels - 1; d >= 0; d--) {
      const f3 dc = ld3(W.s.direct + 3 * ((size_t)d * (size_t)W.n + i));
      col = f3{clamp01(dc.x + col.x * ks.x), clamp01(dc.y + col.y * ks.y), clamp01(dc.z + col.z * ks.z)};
    }
  } else {
    col = f3{P.bg[0], P.bg[1], P.bg[2]};  // primary miss: BACKGROUND_COLOR (:327-332)
  }
  st3(rgb + 3 * i, col);
  if (face) face[i] = W.s.face0[i];
  if (t) t[i] = W.s.t0[i];
}

// counts[0] = n, the rest 0
__global__ void k_wf_counts(uint32_t* counts, uint32_t n) {
  const int k = (int)threadIdx.x;
  if (k <= RT_MAX_TRACE_DEPTH) counts[k] = k == 0 ? n : 0u;
}

}  // namespace rt
