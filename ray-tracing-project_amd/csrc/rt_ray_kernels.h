// rt_ray_kernels.h -- the ray-list packet kernels of rt_trace_* / rt_trace_stream: k_rays (closest hit or shadow),
// k_rays_color (trace_full per ray) and k_rays_depth (trace_depth per ray). Instantiated in rt_rays.hip and nowhere
// else among the product objects; the variants library instantiates k_rays and k_rays_color with other traversal
// flavours in rt_variants.hip.
#pragma once
#include "rt_trace_ray.h"

namespace rt {

// Ray-list packets (rt_trace_* / rt_trace_stream): wave w of the list traces entries 64 w .. 64 w + 63 -- of the
// list itself, or of its coherence order R.perm (RT_RAYS_REORDER), each lane then loading the ray perm names and
// writing that ray's results at its own index. A ray's result is its lane's (t, rank) argmin and never depends
// on the rays beside it, so any grouping gives the same bits. Inactive tail lanes alias the packet's first ray
// and write nothing. STATS (RT_RAYS_STATS): the counting loops, flushed into P.stats.
__device__ __forceinline__ int ray_index(const RayParams& R, int entry) {
  return R.perm ? (int)R.perm[entry] : entry;
}

template <bool ANY, int TRAV, bool STATS = false>
__global__ __launch_bounds__(256) void k_rays(FrameParams P, RayParams R) {
  __shared__ WaveLds<TRAV, STATS> lds;
  const int lane = threadIdx.x & 63;
  const int base = (int)uniform((blockIdx.x * 4 + (threadIdx.x >> 6)) * 64);
  if (base >= R.n) return;
  const bool active = base + lane < R.n;
  const int i = ray_index(R, active ? base + lane : base);  // the lane's ray: loaded from and written at i
  uint32_t cnt_[STATS ? ST_COUNT : 1] = {};
  uint32_t* const cnt = STATS ? cnt_ : nullptr;
  Ray r;
  if (ANY) {  // shadow(P, L): triangle tests from P + 0.003 L, box tests from P (flyscene.cpp:512-519)
    const f3 p = ld3(R.o + 3 * (size_t)i), L = ld3(R.d + 3 * (size_t)i);
    r.o = offset(p, L, 0.003f);
    r.d = L;
    r.o2 = affv3(P.Minv, p);
  } else {
    r.o = ld3(R.o + 3 * (size_t)i);
    r.d = ld3(R.d + 3 * (size_t)i);
    r.o2 = affv3(P.Minv, r.o);
  }
  setup_cull(r, P.sc.static_pad);
  Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  bool found = false;
  if (STATS && active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }
  trace<ANY, STATS, TRAV>(P.sc, r, active, h, found, lds, (int)uniform(threadIdx.x >> 6), cnt);
  if (STATS) {
    if (active && (ANY ? found : h.t != INFINITY)) cnt[ST_HITS]++;
    flush_stats(P, cnt, lane);
  }
  if (!active) return;
  if (ANY) {
    R.blocked[i] = found ? 1 : 0;
  } else if (h.t != INFINITY) {
    const TriRec64 tr = vload_tri(P.sc.tris, h.slot);
    R.face[i] = (int32_t)tr.face;
    R.t[i] = h.t;
    const f3 p{r.o.x + h.t * r.d.x, r.o.y + h.t * r.d.y, r.o.z + h.t * r.d.z};
    if (R.P) {
      R.P[3 * (size_t)i + 0] = p.x;
      R.P[3 * (size_t)i + 1] = p.y;
      R.P[3 * (size_t)i + 2] = p.z;
    }
    if (R.N) {  // interpolateNormal(face, P) (flyscene.cpp:572-600)
      int32_t mat;
      const f3 nn = hit_normal(P.sc, tr, h.slot, p, mat);
      R.N[3 * (size_t)i + 0] = nn.x;
      R.N[3 * (size_t)i + 1] = nn.y;
      R.N[3 * (size_t)i + 2] = nn.z;
    }
  } else {
    R.face[i] = -1;
    R.t[i] = INFINITY;
    if (R.P) R.P[3 * (size_t)i] = R.P[3 * (size_t)i + 1] = R.P[3 * (size_t)i + 2] = 0.0f;
    if (R.N) R.N[3 * (size_t)i] = R.N[3 * (size_t)i + 1] = R.N[3 * (size_t)i + 2] = 0.0f;
  }
}

// traceRay(o, d, 0) (FULL, max_depth 2) for a list of rays (rt_trace_color): colour, first-hit face and t
template <int TRAV, bool STATS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEu)))
void k_rays_color(FrameParams P, RayParams R) {
  __shared__ WaveLds<TRAV, STATS> lds;
  const int lane = threadIdx.x & 63, wv = (int)uniform(threadIdx.x >> 6);
  const int base = (int)uniform((blockIdx.x * 4 + (threadIdx.x >> 6)) * 64);
  if (base >= R.n) return;
  const bool active = base + lane < R.n;
  const int i = ray_index(R, active ? base + lane : base);
  uint32_t cnt_[STATS ? ST_COUNT : 1] = {};
  uint32_t* const cnt = STATS ? cnt_ : nullptr;
  Ray r;
  r.o = ld3(R.o + 3 * (size_t)i);
  r.d = ld3(R.d + 3 * (size_t)i);
  r.o2 = affv3(P.Minv, r.o);
  setup_cull(r, P.sc.static_pad);
  if (STATS && active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }
  Hit h;
  uint32_t face0;
  const f3 col = trace_full<STATS, TRAV>(P, r, active, lds, wv, cnt, h, face0);
  if (STATS) flush_stats(P, cnt, lane);
  if (!active) return;
  R.rgb[3 * (size_t)i + 0] = col.x;
  R.rgb[3 * (size_t)i + 1] = col.y;
  R.rgb[3 * (size_t)i + 2] = col.z;
  if (R.face) R.face[i] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
  if (R.t) R.t[i] = h.t;
}

// traceRay(o, d, 0) at any recursion limit, with or without shadow rays (P.max_depth, P.shadows), for a list of
// rays (rt_trace_stream_color): the level loop (trace_depth) under the list packets' addressing
template <bool STATS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEu)))
void k_rays_depth(FrameParams P, RayParams R) {
  __shared__ WaveLds<TRAV_B2_LDS, STATS> lds;
  const int lane = threadIdx.x & 63, wv = (int)uniform(threadIdx.x >> 6);
  const int base = (int)uniform((blockIdx.x * 4 + (threadIdx.x >> 6)) * 64);
  if (base >= R.n) return;
  const bool active = base + lane < R.n;
  const int i = ray_index(R, active ? base + lane : base);
  uint32_t cnt_[STATS ? ST_COUNT : 1] = {};
  uint32_t* const cnt = STATS ? cnt_ : nullptr;
  Ray r;
  r.o = ld3(R.o + 3 * (size_t)i);
  r.d = ld3(R.d + 3 * (size_t)i);
  r.o2 = affv3(P.Minv, r.o);
  setup_cull(r, P.sc.static_pad);
  if (STATS && active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }
  Hit h;
  uint32_t face0;
  const f3 col = trace_depth<STATS, LSRC>(P, r, active, lds, wv, cnt, h, face0);
  if (STATS) flush_stats(P, cnt, lane);
  if (!active) return;
  R.rgb[3 * (size_t)i + 0] = col.x;
  R.rgb[3 * (size_t)i + 1] = col.y;
  R.rgb[3 * (size_t)i + 2] = col.z;
  if (R.face) R.face[i] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
  if (R.t) R.t[i] = h.t;
}

}  // namespace rt
