// rt_shade.h -- shading of a hit: the material state, interpolateNormal, Phong, and calculateColor with its shadow
// any-hit walks per light (lights from the kernel arguments or from device memory). Used by every kernel that
// colours a hit: the frame, ray-list and view kernels through rt_trace_ray.h, the wavefront stages and the variants.
#pragma once
#include "rt_traverse.h"

namespace rt {

// ------------------------------------------------------------------------------------------------
// Shading
// ------------------------------------------------------------------------------------------------
struct MatState {  // Flyscene members ka/kd/ks/shininess (flyscene.hpp:179-182)
  f3 ka, kd, ks;
  float ns;
};

__device__ __forceinline__ MatState load_mat(const DevMat& m) {
  return MatState{f3{m.ka[0], m.ka[1], m.ka[2]}, f3{m.kd[0], m.kd[1], m.kd[2]}, f3{m.ks[0], m.ks[1], m.ks[2]}, m.ns};
}

// interpolateNormal (flyscene.cpp:572-600) for the hit triangle of this lane: one contiguous 48-B
// gather of the face's shading record (its three unit vertex normals + material)
// the shading record is indexed by the triangle slot (like the record itself), so its gather does not wait
// for the record's face id: both loads of a hit are issued together
__device__ __forceinline__ f3 hit_normal(const DevScene& P, const TriRec64& tr, uint32_t slot, f3 p, int32_t& mat) {
  const f3 n{tr.nx, tr.ny, tr.nz};
  const f3 w0{tr.w0x, tr.w0y, tr.w0z}, w1{tr.w1x, tr.w1y, tr.w1z}, w2{tr.w2x, tr.w2y, tr.w2z};
  const f3 e0 = sub(w1, w0), e1 = sub(w2, w1), e2 = sub(w0, w2);
  const f3 a0 = cross(e0, sub(p, w0)), a1 = cross(e1, sub(p, w1)), a2 = cross(e2, sub(p, w2));
  const float4* fs = reinterpret_cast<const float4*>(P.fshade + 12 * (size_t)slot);
  const float4 n0 = fs[0];
  mat = __float_as_int(n0.w);
  if (dot(n, a0) < 0 || dot(n, a1) < 0 || dot(n, a2) < 0) return f3{0.0f, 0.0f, 0.0f};
  const float area0 = norm(a0) / 2, area1 = norm(a1) / 2, area2 = norm(a2) / 2;
  const float area = norm(cross(e0, neg(e2))) / 2;
  const float4 n1 = fs[1], n2 = fs[2];
  return blend_normal(f3{n0.x, n0.y, n0.z}, f3{n1.x, n1.y, n1.z}, f3{n2.x, n2.y, n2.z}, area0, area1, area2, area);
}

__device__ __forceinline__ TriRec64 vload_tri(const TriRec64* base, uint32_t i) {
  const float4* p = reinterpret_cast<const float4*>(base + i);
  TriRec64 r;
  float4* q = reinterpret_cast<float4*>(&r);
  q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; q[3] = p[3];
  return r;
}


// Light l of the frame, read from the kernel-argument segment. Every kernel takes FrameParams as its
// first argument, so the lights sit at offsetof(FrameParams, lights) of that segment; indexing them
// there (scalar loads, l is wave-uniform) means a light loop never makes the compiler copy the whole
// FrameParams into private memory for a dynamic index -- which it did in the FULL megakernel once the
// kernel grew (1.7 KB of scratch per lane, 3x slower).
__device__ __forceinline__ Light frame_light(int l) {
  typedef const __attribute__((address_space(4))) char* KArg;
  typedef const __attribute__((address_space(4))) Light* KLight;
  const KArg base = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
  const KLight q = (KLight)(base + offsetof(FrameParams, lights) + (size_t)l * sizeof(Light));
  Light r;
  for (int k = 0; k < 3; k++) {
    r.p[k] = q->p[k];
    r.c[k] = q->c[k];
  }
  r.kind = q->kind;
  return r;
}

// Light l of a light set (rt_light_set, FrameParams::light_set): the set's device array, in calculateColor's
// order, read through the constant address space -- base and l are wave-uniform, so these are scalar loads
// (one fetch per wave into SGPRs, as frame_light's) and nothing is ever written there
__device__ __forceinline__ Light set_light(const FrameParams& P, int l) {
  typedef const __attribute__((address_space(4))) Light* CLight;
  const uint64_t b = (uint64_t)P.light_set;
  const uint64_t bs = ((uint64_t)uniform((uint32_t)(b >> 32)) << 32) | (uint32_t)uniform((uint32_t)b);
  const CLight q = (CLight)bs + uniform((uint32_t)l);
  Light r;
  for (int k = 0; k < 3; k++) {
    r.p[k] = q->p[k];
    r.c[k] = q->c[k];
  }
  r.kind = q->kind;
  return r;
}

// calculateColor's light direction (flyscene.cpp:607-611): point light -(P - pos).normalized(), or a
// directional light's stored vector as is
__device__ __forceinline__ f3 light_dir(f3 p, const Light& l) {
  if (l.kind == RT_LIGHT_DIRECTIONAL) return f3{l.p[0], l.p[1], l.p[2]};
  return neg(normalized(sub(p, f3{l.p[0], l.p[1], l.p[2]})));
}

// Hit information of one lane, gathered once and reused by every light of calculateColor
struct HitInfo {
  f3 p, n;
  int32_t mat;
  uint32_t face;
};

// calcSingleColor body after the shadow test (flyscene.cpp:546-565)
__device__ __forceinline__ f3 phong(const FrameParams& P, MatState& st, const HitInfo& hi, f3 o, f3 L, const float* I) {
  if (hi.mat != -1) st = load_mat(P.sc.mats[hi.mat]);
  const f3 R = phong_r(L, hi.n);
  const f3 E = normalized(sub(o, hi.p));
  const float dif = smax(dot(L, hi.n), 0.0f);
  const float spe = smax(pow_ref(dot(R, E), st.ns), 0.0f);
  return f3{(I[0] * st.ka.x + (I[0] * st.kd.x) * dif) + (I[0] * st.ks.x) * spe,
            (I[1] * st.ka.y + (I[1] * st.kd.y) * dif) + (I[1] * st.ks.y) * spe,
            (I[2] * st.ka.z + (I[2] * st.kd.z) * dif) + (I[2] * st.ks.z) * spe};
}

__device__ __forceinline__ float clamp01(float x) { return smax(smin(x, 1.0f), 0.0f); }

// calculateColor (flyscene.cpp:603-614). SHADOWS: per light, a wave-packet any-hit traversal from
// P + 0.003 L (box predicate from P) decides whether the light contributes (calcSingleColor :543).
// LSRC: where light l comes from -- LS_KERNARG: frame_light(l), every kernel of rt_render's path; LS_MEMORY /
// LS_MEMORY_CACHED: set_light(P, l), the light-set instantiations of the generic kernels. Same arithmetic and
// summation order either way, hence the same bits for the same lights.
// LS_MEMORY_CACHED adds the wave-level occluder cache to the shadow packets. shadow(P, L) is true iff any triangle
// passes test_tri<true>; which one is found first never matters. The lights of a soft (spherical) light lie close
// together, so the triangle that blocked light l for some lanes very often blocks light l + 1 for the same lanes.
// The walk reports the slots at which lanes first became blocked (test_tri's occ); before the walk of the next
// light the wave runs test_tri<true> -- the leaves' own test: plane, edges, normal check, box predicate and
// certificates -- on those kOccK records for the lanes not yet blocked, walks only for the lanes that remain, and
// skips the walk when none do. A lane the pre-test blocks is one a leaf visit would have blocked: bit-identical.
// The cache lives in this call, so it starts empty at each hit level.
template <bool SHADOWS, bool STATS, int TRAV, bool OCTSH = false, bool SPLIT = false, int LSRC = LS_KERNARG>
__device__ __forceinline__ f3 calc_color(const FrameParams& P, MatState& st, const HitInfo& hi, f3 o, bool lane_hit,
                                         WaveLds<TRAV, STATS>* lds, int wv, uint32_t* cnt) {
  f3 sum{0.0f, 0.0f, 0.0f};
  uint32_t occ[kOccK];
#pragma unroll
  for (int k = 0; k < kOccK; k++) occ[k] = kOccNone;
  for (int l = 0; l < P.n_lights; l++) {
    const Light lt = LSRC == LS_KERNARG ? frame_light(l) : set_light(P, l);
    const f3 L = light_dir(hi.p, lt);
    bool blocked = false;
    if (SHADOWS) {
      Ray sr;
      sr.o = offset(hi.p, L, 0.003f);
      sr.d = L;
      sr.o2 = affv3(P.Minv, hi.p);
      setup_cull(sr, P.sc.static_pad);
      Hit hh{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
      if (STATS && lane_hit) cnt[ST_TOTAL]++;
      if constexpr (LSRC == LS_MEMORY_CACHED) {
#pragma unroll
        for (int k = 0; k < kOccK; k++) {
          const uint32_t slot = uniform(occ[k]);
          const uint64_t rem = ballot(lane_hit && !blocked);
          if (slot == kOccNone || rem == 0) continue;
          const TriRec64 tr = sload_tri(P.sc.tris, slot);
          if (STATS) {  // a record fetched once per wave and tested by the remaining lanes, as in a leaf
            cnt[ST_WTRI]++;
            if (lane_hit && !blocked) cnt[ST_TRI]++;
          }
          test_tri<true>(P.sc, tr, slot, sr, rem, hh, blocked);
        }
        const bool remain = lane_hit && !blocked;
        if (ballot(remain) != 0) trace_full_ray<true, STATS, TRAV>(P.sc, sr, remain, hh, blocked, *lds, wv, cnt, occ);
      } else if (OCTSH)
        trace_oct<true, STATS, TRAV, false, SPLIT>(P.sc, sr, lane_hit, hh, blocked, *lds, wv, cnt);
      else trace_full_ray<true, STATS, TRAV>(P.sc, sr, lane_hit, hh, blocked, *lds, wv, cnt);
    }
    f3 c{0.0f, 0.0f, 0.0f};
    if (lane_hit && !blocked) c = phong(P, st, hi, o, L, lt.c);
    sum = f3{sum.x + c.x, sum.y + c.y, sum.z + c.z};
  }
  return f3{clamp01(sum.x), clamp01(sum.y), clamp01(sum.z)};
}

}  // namespace rt
