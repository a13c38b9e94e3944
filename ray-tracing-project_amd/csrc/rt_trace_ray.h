// rt_trace_ray.h -- the reference's traceRay for one packet, in the three forms the kernels share: depth limit 1
// without shadows (shade_primary_pixel, after a closest hit), FULL at max_depth 2 (trace_full), and any depth
// (k_render_depth and trace_depth, the level loop). Each is used by more than one of the frame, ray-list and view
// kernels (rt_frame_kernels.h, rt_ray_kernels.h, rt_view_kernels.h), so it lives below all three; the launch bounds
// those kernels share are here as well. The one kernel defined here, k_render_depth, is a frame kernel (instantiated
// in rt_frame.hip): it sits beside trace_depth because the two are one loop written twice.
#pragma once
#include "rt_frame_wave.h"
#include "rt_shade.h"

namespace rt {

// launch bounds of the PRIMARY traversal kernels (k_trace_primary, k_primary_fused, k_views_primary)
constexpr int kTraceWavesPerEu = 8;  // 8 waves/SIMD: measured +2.5% over the 7 the register count allows
constexpr int kTraceWPB = 1;  // waves per block of the traversal kernel (4 or 1; 1 measured 3% faster)

// PRIMARY stage 2: traceRay at depth limit 1 without shadows: calculateColor (flyscene.cpp:603-614)
// + traceRay's ks update and clamp (:355-370), or the background on a miss (:327-332), for one pixel
// whose closest hit (t, triangle slot) is known.
// BOXCOL: RENDER_BOUNDINGBOX_COLORED_TRIANGLES (flyscene.cpp:334-348) instead of the shading: the hit
// face's summed box colours (k_face_box_colors), unclamped.
template <bool HITS, bool BOXCOL = false>
__device__ __forceinline__ void shade_primary_pixel(const FrameParams& P, const Ray& r, size_t pix, float t,
                                                    uint32_t slot) {
  const bool hit0 = t != INFINITY;
  f3 col;
  int32_t face = -1;
  if (BOXCOL && hit0) {
    face = (int32_t)P.sc.tris[slot].face;
    const float4 c = reinterpret_cast<const float4*>(P.face_boxcolor)[face];
    col = f3{c.x, c.y, c.z};
  } else if (hit0) {
    const TriRec64 tr0 = vload_tri(P.sc.tris, slot);
    HitInfo hi0;
    hi0.face = tr0.face;
    face = (int32_t)tr0.face;
    hi0.p = f3{r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z};
    hi0.n = hit_normal(P.sc, tr0, slot, hi0.p, hi0.mat);
    MatState st = load_mat(P.defmat);
    const f3 direct0 = calc_color<false, false, TRAV_B2_LDS>(P, st, hi0, r.o, true, nullptr, 0, nullptr);
    if (hi0.mat != -1) st.ks = load_mat(P.sc.mats[hi0.mat]).ks;
    col = f3{clamp01(direct0.x + 0.0f * st.ks.x), clamp01(direct0.y + 0.0f * st.ks.y),
             clamp01(direct0.z + 0.0f * st.ks.z)};
  } else {
    col = f3{P.bg[0], P.bg[1], P.bg[2]};
  }
  P.rgb[3 * pix + 0] = col.x;
  P.rgb[3 * pix + 1] = col.y;
  P.rgb[3 * pix + 2] = col.z;
  if (HITS) {
    P.face_out[pix] = face;
    P.t_out[pix] = t;
  }
}

// FULL: the reference traceRay as-is (max_depth 2): shadow any-hit per light and one reflection
// bounce, all in one kernel (flyscene.cpp:317-371, 510-566, 603-614).
// traceRay(o, d, 0) with max_depth 2 (FULL, flyscene.cpp:317-371): primary hit, per-light shadows, one
// reflection bounce with its own shadows. Shared by the frame megakernel and the ray-list colour query.
// Returns the colour; h0 / face0: the first hit (t, face id).
// SPLIT: mixed-octant secondary packets walk once per octant (trace_oct); the small-scene build only --
// measured C5 +1.5% at 4 frames in flight, +1..3% one at a time, the 1M soup in FULL -5%
// (profiles/ab/r03_full_split_oct_ab.txt)
// counting run: one phase's packet walk(s) of a wave (ST_PW ..)
struct PhaseMark {
  uint32_t n0, t0;
};
template <bool STATS>
__device__ __forceinline__ PhaseMark phase_begin(const uint32_t* cnt) {
  if (!STATS) return PhaseMark{0, 0};
  return PhaseMark{cnt[ST_WNODE], cnt[ST_WTRI]};
}
template <bool STATS>
__device__ __forceinline__ void phase_end(uint32_t* cnt, int p, const PhaseMark& m, bool act) {
  if (!STATS) return;
  const uint64_t b = ballot(act);
  if (b == 0) return;
  const uint32_t lanes = (uint32_t)__popcll(b), steps = cnt[ST_WNODE] - m.n0;
  cnt[ST_PW + p]++;
  cnt[ST_PL + p] += lanes;
  cnt[ST_PS + p] += steps;
  cnt[ST_PT + p] += cnt[ST_WTRI] - m.t0;
  if (p > 0) cnt[ST_PH + (lanes <= 8 ? 0 : lanes <= 16 ? 1 : lanes <= 32 ? 2 : lanes <= 48 ? 3 : 4)] += steps;
}

template <bool STATS, int TRAV, bool SPLIT = false>
__device__ __forceinline__ f3 trace_full(const FrameParams& P, const Ray& r, bool active, WaveLds<TRAV, STATS>& lds, int wv,
                                         uint32_t* cnt, Hit& h, uint32_t& face0, float* tprim = nullptr) {
  h = Hit{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  bool dummy = false;
  // the primary packet is coherent: octant-specialised loops
  PhaseMark pm = phase_begin<STATS>(cnt);
  trace_oct<false, STATS, TRAV>(P.sc, r, active, h, dummy, lds, wv, cnt);
  phase_end<STATS>(cnt, 0, pm, active);
  const bool hit0 = active && h.t != INFINITY;
  if (STATS && hit0) cnt[ST_HITS]++;
  if (tprim) tprim[lane_id()] = hit0 ? h.t : INFINITY;

  MatState st = load_mat(P.defmat);
  HitInfo hi0;
  hi0.mat = -1;
  hi0.face = 0xFFFFFFFFu;
  hi0.p = f3{0.0f, 0.0f, 0.0f};
  hi0.n = f3{0.0f, 0.0f, 0.0f};
  if (hit0) {
    const TriRec64 tr0 = vload_tri(P.sc.tris, h.slot);
    hi0.face = tr0.face;
    hi0.p = f3{r.o.x + h.t * r.d.x, r.o.y + h.t * r.d.y, r.o.z + h.t * r.d.z};
    hi0.n = hit_normal(P.sc, tr0, h.slot, hi0.p, hi0.mat);
  }
  // the primary hits' shadow packets head for the same light from neighbouring points: octant loops for
  // them too (A/B knob RT_FULL_OCT_SHADOW); the reflection hits' shadows keep the generic loop
  pm = phase_begin<STATS>(cnt);
  const f3 direct0 = calc_color<true, STATS, TRAV, true, SPLIT>(P, st, hi0, r.o, hit0, &lds, wv, cnt);
  phase_end<STATS>(cnt, 1, pm, hit0);
  if (hit0 && hi0.mat != -1) st.ks = load_mat(P.sc.mats[hi0.mat]).ks;  // traceRay :355-358

  // reflect(dir.normalized(), interpolateNormal(...)), offset 0.001 (flyscene.cpp:361-363)
  f3 refl{0.0f, 0.0f, 0.0f};
  Ray rr;
  rr.d = reflect(normalized(r.d), hi0.n);
  rr.o = offset(hi0.p, rr.d, 0.001f);
  rr.o2 = affv3(P.Minv, rr.o);
  setup_cull(rr, P.sc.static_pad);
  if (STATS && hit0) cnt[ST_TOTAL]++;
  Hit h1{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  pm = phase_begin<STATS>(cnt);
  trace_oct<false, STATS, TRAV, false, SPLIT>(P.sc, rr, hit0, h1, dummy, lds, wv, cnt);
  phase_end<STATS>(cnt, 2, pm, hit0);
  const bool hit1 = hit0 && h1.t != INFINITY;
  HitInfo hi1;
  hi1.mat = -1;
  hi1.p = f3{0.0f, 0.0f, 0.0f};
  hi1.n = f3{0.0f, 0.0f, 0.0f};
  if (hit1) {
    const TriRec64 tr1 = vload_tri(P.sc.tris, h1.slot);
    hi1.face = tr1.face;
    hi1.p = f3{rr.o.x + h1.t * rr.d.x, rr.o.y + h1.t * rr.d.y, rr.o.z + h1.t * rr.d.z};
    hi1.n = hit_normal(P.sc, tr1, h1.slot, hi1.p, hi1.mat);
  }
  pm = phase_begin<STATS>(cnt);
  const f3 direct1 = calc_color<true, STATS, TRAV, true, SPLIT>(P, st, hi1, rr.o, hit1, &lds, wv, cnt);
  phase_end<STATS>(cnt, 3, pm, hit1);
  if (hit1) {
    if (hi1.mat != -1) st.ks = load_mat(P.sc.mats[hi1.mat]).ks;
    // depth 1: direct1 + traceRay(depth 2)=0 * ks, clamped
    refl = f3{clamp01(direct1.x + 0.0f * st.ks.x), clamp01(direct1.y + 0.0f * st.ks.y),
              clamp01(direct1.z + 0.0f * st.ks.z)};
  }
  f3 col;
  if (hit0) {
    col = f3{clamp01(direct0.x + refl.x * st.ks.x), clamp01(direct0.y + refl.y * st.ks.y),
             clamp01(direct0.z + refl.z * st.ks.z)};
  } else {
    col = f3{P.bg[0], P.bg[1], P.bg[2]};
  }
  face0 = hit0 ? hi0.face : 0xFFFFFFFFu;
  return col;
}

// Occupancy of the FULL megakernel, by scene: 8 waves per SIMD for scenes whose node + triangle records
// exceed the chip's aggregate L2 (the 1M soup: 8 waves beat 5 by 18% and 3 by 24% -- the traversal waits
// on L2 misses and needs the waves), a 6-wave bound for smaller ones (bunny, C5: +14% over 8 -- their
// records are L2-resident). Resources of the shipped instantiations (make asm, round 5, after the pixel
// coordinates moved to LDS): k_render_full<false, false, 1, 6> 80 VGPR, 104 SGPR, no scratch (round 4: 80
// VGPR + 32 B of scratch -- the spill of the thread id and px / py); <false, false, 1, 8> 64 VGPR + 96 B
// scratch. Re-swept in round 5 without the spill: 5 waves (85 VGPR, no scratch) -1..-6%, 7 waves (72 VGPR +
// 48 B scratch) -3..-8% against 6 (profiles/ab/r05_full_waves_ab.txt).
#ifndef RT_FULL_WPE_SMALL  // A/B builds only (make ablib EXTRA=-DRT_FULL_WPE_SMALL=n)
#define RT_FULL_WPE_SMALL 6
#endif
constexpr int kFullWavesPerEu = 8, kFullWavesPerEuSmall = RT_FULL_WPE_SMALL;
// waves per block of the FULL megakernel (1: one 8x8 wave per block, measured +6.5% on bunny FULL and +8%
// on the soup over 4 = one 16x16 tile per block)
constexpr int kFullWPB = 1;

// The level loop of traceRay at any depth exists three times: in k_render_depth (the frame kernel), in trace_depth
// right below it (the ray-list and view kernels), and cut into stages in rt_wavefront.h (k_wf_closest / k_wf_shade /
// k_wf_resolve). A change to one is a change to all three.
// traceRay(o, d, 0) for any recursion limit D = P.max_depth (flyscene.cpp:317-371; the reference fixes
// max_depth = 2 at flyscene.hpp:142, SURVEY 8(b) b2 exposes it): level d traces the closest hit of
// the ray from level d-1's reflection, shades it (calculateColor, shadows per P.shadows) and updates
// the sticky ks (traceRay :355-358). The reference combines on the way back up,
//   colour_d = clamp01(direct_d + colour_{d+1} (*) ks),
// reading the ks member AFTER the deeper levels returned, i.e. the last value any level wrote; so the
// kernel keeps each level's direct colour (lane-private array, D <= RT_MAX_TRACE_DEPTH) and folds them
// from the deepest hit level upwards with that final ks. The deepest hit level adds 0 (*) ks (its own
// reflection returned black: a miss below depth 0, or depth == max_depth). D = 0 returns black for
// every pixel without tracing (traceRay :318-320). Same expressions and order as k_render_full for
// D = 2, hence the same bits (tested); this kernel serves the other depths.
// LSRC (calc_color): LS_KERNARG for rt_render's frames; the light-set frames beyond 32 lights instantiate
// LS_MEMORY_CACHED (LS_MEMORY: the same without the occluder cache, VB_NO_OCCLUDER_CACHE).
template <bool STATS, bool HITS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEuSmall)))
void k_render_depth(FrameParams P) {
  __shared__ WaveLds<TRAV_B2_LDS, STATS> lds;
  wave_clock_start(P, lds.clk);
  const PixelCoord c = pixel_coord<1>(P);
  const bool active = c.active;
  uint32_t cnt[ST_COUNT] = {};
  Ray cur = primary_ray(P, c.px, c.py);
  const Ray r0 = cur;
  if (STATS && active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }
  MatState st = load_mat(P.defmat);
  f3 direct[RT_MAX_TRACE_DEPTH];
  int levels = 0;  // levels whose closest hit exists (the chain stops at the first miss)
  bool act = active;
  Hit h0{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t face0 = 0xFFFFFFFFu;
  const int D = P.max_depth;
#pragma clang loop unroll(disable)
  for (int d = 0; d < D; d++) {
    Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
    bool dummy = false;
    if (d == 0) trace_oct<false, STATS, TRAV_B2_LDS>(P.sc, cur, act, h, dummy, lds, c.slot, cnt);
    else trace<false, STATS, TRAV_B2_LDS>(P.sc, cur, act, h, dummy, lds, c.slot, cnt);
    const bool hit = act && h.t != INFINITY;
    if (STATS && d == 0 && hit) cnt[ST_HITS]++;
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
    if (d == 0) {
      h0 = h;
      face0 = hit ? hi.face : 0xFFFFFFFFu;
    }
    const f3 dc = P.shadows ? calc_color<true, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, hit, &lds, c.slot, cnt)
                            : calc_color<false, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, hit, &lds, c.slot, cnt);
    if (hit) {
      direct[d] = dc;
      levels = d + 1;
      if (hi.mat != -1) st.ks = load_mat(P.sc.mats[hi.mat]).ks;  // traceRay :355-358
    }
    if (d + 1 == D) break;  // traceRay(depth + 1) returns black without tracing (:318-320)
    // reflect(dir.normalized(), interpolateNormal(...)), offset 0.001 (flyscene.cpp:361-363)
    Ray rr;
    rr.d = reflect(normalized(cur.d), hi.n);
    rr.o = offset(hi.p, rr.d, 0.001f);
    rr.o2 = affv3(P.Minv, rr.o);
    setup_cull(rr, P.sc.static_pad);
    if (STATS && hit) cnt[ST_TOTAL]++;
    cur = rr;
    act = hit;
    if (ballot(act) == 0) break;  // no lane of the wave continues
  }
  f3 col{0.0f, 0.0f, 0.0f};
  for (int d = levels - 1; d >= 0; d--)
    col = f3{clamp01(direct[d].x + col.x * st.ks.x), clamp01(direct[d].y + col.y * st.ks.y),
             clamp01(direct[d].z + col.z * st.ks.z)};
  if (D > 0 && levels == 0) col = f3{P.bg[0], P.bg[1], P.bg[2]};  // primary miss: BACKGROUND_COLOR (:327-332)
  (void)r0;
  if (active) {
    const size_t pix = (size_t)c.py * P.W + c.px;
    P.rgb[3 * pix + 0] = col.x;
    P.rgb[3 * pix + 1] = col.y;
    P.rgb[3 * pix + 2] = col.z;
    if (HITS) {
      P.face_out[pix] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
      P.t_out[pix] = h0.t;
    }
  }
  if (STATS) flush_stats(P, cnt, c.lane);
  wave_clock_end(P, lds.clk, c.lane, c.qw);
}

// k_render_depth's level loop for the list kernel below: cur is level 0's ray, the return value traceRay's colour,
// h0 / face0 the first hit (face0 = ~0: a miss). A copy, statement for statement, and not a function both kernels
// share: with the loop moved into a function k_render_depth's scratch size and spill counts changed (make asm), and
// the frame kernels stay as they are. Keep the two in step.
template <bool STATS, int LSRC = LS_KERNARG>
__device__ __forceinline__ f3 trace_depth(const FrameParams& P, Ray cur, bool active, WaveLds<TRAV_B2_LDS, STATS>& lds,
                                          int slot, uint32_t* cnt, Hit& h0, uint32_t& face0) {
  MatState st = load_mat(P.defmat);
  f3 direct[RT_MAX_TRACE_DEPTH];
  int levels = 0;  // levels whose closest hit exists (the chain stops at the first miss)
  bool act = active;
  h0 = Hit{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  face0 = 0xFFFFFFFFu;
  const int D = P.max_depth;
#pragma clang loop unroll(disable)
  for (int d = 0; d < D; d++) {
    Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
    bool dummy = false;
    if (d == 0) trace_oct<false, STATS, TRAV_B2_LDS>(P.sc, cur, act, h, dummy, lds, slot, cnt);
    else trace<false, STATS, TRAV_B2_LDS>(P.sc, cur, act, h, dummy, lds, slot, cnt);
    const bool hit = act && h.t != INFINITY;
    if (STATS && d == 0 && hit) cnt[ST_HITS]++;
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
    if (d == 0) {
      h0 = h;
      face0 = hit ? hi.face : 0xFFFFFFFFu;
    }
    const f3 dc = P.shadows ? calc_color<true, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, hit, &lds, slot, cnt)
                            : calc_color<false, STATS, TRAV_B2_LDS, false, false, LSRC>(P, st, hi, cur.o, hit, &lds, slot, cnt);
    if (hit) {
      direct[d] = dc;
      levels = d + 1;
      if (hi.mat != -1) st.ks = load_mat(P.sc.mats[hi.mat]).ks;  // traceRay :355-358
    }
    if (d + 1 == D) break;  // traceRay(depth + 1) returns black without tracing (:318-320)
    // reflect(dir.normalized(), interpolateNormal(...)), offset 0.001 (flyscene.cpp:361-363)
    Ray rr;
    rr.d = reflect(normalized(cur.d), hi.n);
    rr.o = offset(hi.p, rr.d, 0.001f);
    rr.o2 = affv3(P.Minv, rr.o);
    setup_cull(rr, P.sc.static_pad);
    if (STATS && hit) cnt[ST_TOTAL]++;
    cur = rr;
    act = hit;
    if (ballot(act) == 0) break;  // no lane of the wave continues
  }
  f3 col{0.0f, 0.0f, 0.0f};
  for (int d = levels - 1; d >= 0; d--)
    col = f3{clamp01(direct[d].x + col.x * st.ks.x), clamp01(direct[d].y + col.y * st.ks.y),
             clamp01(direct[d].z + col.z * st.ks.z)};
  if (D > 0 && levels == 0) col = f3{P.bg[0], P.bg[1], P.bg[2]};  // primary miss: BACKGROUND_COLOR (:327-332)
  return col;
}

}  // namespace rt
