// rt_update_kernels.h -- the kernels of rt_scene_update_device (rt_update_device.hip): the host stages of an update
// re-stated one lane per vertex, face, slot or position, from the same RT_HD functions the host stages call
// (rt_math.h, rt_faceflags.h), so every word they write is the host's. 256-thread blocks, every index bounds
// checked, plain vector stores; the reductions go through wave shuffles and one atomic per wave and value.
//   k_upd_vertices    scene_invariants' first loop: raw xyz, world vertex, unit vertex normal
//   k_upd_faces       its second loop and accept_region: unit face normal, plane distance, accept-region triangle
//   k_upd_slot_bounds scene_static_pad's bounds over the slots' faces (of the world and of the accept-region vertices)
//   k_upd_ranks       assign_box_ranks: rank and box of the face at every position of the partition's face order
//   k_upd_face_words  face_records' flags: safe_normal and box_certified into the face's box word
#pragma once
#include <hip/hip_runtime.h>

#include "rt_faceflags.h"
#include "rt_scene.h"

namespace rt {

// The reduction words of one update (uint32 each): flags, the largest |object coordinate| (bits of a non-negative
// float order as integers), and two sets of bounds as ordered keys (key_of: monotone in the float).
enum UpdRed { UR_NONFINITE = 0, UR_TILTED = 1, UR_MAXABS = 2, UR_WLO = 4, UR_WHI = 7, UR_ALO = 10, UR_AHI = 13, UR_WORDS = 16 };

struct Mat16 {
  float m[16];
};

__host__ __device__ __forceinline__ uint32_t key_of(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return (u >> 31) ? ~u : (u | 0x80000000u);
}
__host__ __device__ __forceinline__ float float_of_key(uint32_t k) {
  const uint32_t u = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
  float x;
  memcpy(&x, &u, 4);
  return x;
}

__device__ __forceinline__ bool in_range(float x) { return fabsf(x) <= 1e30f; }  // NaN fails too
__device__ __forceinline__ bool in_range3(f3 p) { return in_range(p.x) && in_range(p.y) && in_range(p.z); }

__device__ __forceinline__ float wave_min(float x) {
  for (int m = 32; m >= 1; m >>= 1) x = fminf(x, __shfl_xor(x, m));
  return x;
}
__device__ __forceinline__ float wave_max(float x) {
  for (int m = 32; m >= 1; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
  return x;
}

__global__ void __launch_bounds__(64) k_upd_init(uint32_t* red) {
  const uint32_t k = threadIdx.x;
  if (k >= UR_WORDS) return;
  const bool is_min = (k >= UR_WLO && k < UR_WHI) || (k >= UR_ALO && k < UR_AHI);
  red[k] = is_min ? 0xFFFFFFFFu : 0u;
}

// One lane per vertex. A coordinate that is not finite or beyond 1e30 in magnitude (object or world space) raises
// UR_NONFINITE: the caller then takes the host path, which decides for itself.
__global__ void __launch_bounds__(256) k_upd_vertices(uint32_t nv, const float* v4, const float* vn3, Mat16 M, float* ov3, float* wv,
                                                      float* vnn, uint32_t* red) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  float mag = 0.0f;
  if (i < nv) {
    const float* v = v4 + 4 * (size_t)i;
    const float x = v[0], y = v[1], z = v[2], w = v[3];
    const f3 p = affv3(M.m, f3{x / w, y / w, z / w});
    const float* n = vn3 + 3 * (size_t)i;
    const f3 un = normalized(f3{n[0], n[1], n[2]});
    float* o = ov3 + 3 * (size_t)i;
    o[0] = x, o[1] = y, o[2] = z;
    float* pw = wv + 3 * (size_t)i;
    pw[0] = p.x, pw[1] = p.y, pw[2] = p.z;
    float* pn = vnn + 3 * (size_t)i;
    pn[0] = un.x, pn[1] = un.y, pn[2] = un.z;
    bad = !in_range(x) || !in_range(y) || !in_range(z) || !in_range3(p);
    mag = fmaxf(fmaxf(fabsf(x), fabsf(y)), fabsf(z));
  }
  const bool any_bad = __any(bad);
  mag = wave_max(mag);
  if ((threadIdx.x & 63u) == 0) {
    if (any_bad) atomicOr(red + UR_NONFINITE, 1u);
    else atomicMax(red + UR_MAXABS, __float_as_uint(mag));  // (finite, non-negative)
  }
}

// One lane per face: the first four words of its FaceWords (rank and box follow from the partition), its
// accept-region triangle (the world triangle unless the face is tilted), UR_TILTED when it is.
__global__ void __launch_bounds__(256) k_upd_faces(uint32_t nf, uint32_t nv, const uint32_t* fidx, const float* fn3, const float* wv,
                                                   FaceWords* face, float* av, uint32_t* red) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  bool bad = false, tilted = false;
  if (f < nf) {
    const uint32_t v0 = fidx[3 * (size_t)f], v1 = fidx[3 * (size_t)f + 1], v2 = fidx[3 * (size_t)f + 2];
    if (v0 < nv && v1 < nv && v2 < nv) {  // (always: the scene's own indices)
      const float* n = fn3 + 3 * (size_t)f;
      const f3 un = normalized(f3{n[0], n[1], n[2]});
      const f3 w[3] = {ld3(wv + 3 * (size_t)v0), ld3(wv + 3 * (size_t)v1), ld3(wv + 3 * (size_t)v2)};
      const float dist = dot(un, w[0]);
      face[f].nx = un.x, face[f].ny = un.y, face[f].nz = un.z, face[f].dist = dist;
      tilted = !(face_tilt_of(w[0], w[1], w[2], un) <= kBoundTilt);
      float* a = av + 9 * (size_t)f;
      for (int j = 0; j < 3; j++) {
        const f3 p = accept_vertex_of(w[j], un, dist, tilted);
        a[3 * j] = p.x, a[3 * j + 1] = p.y, a[3 * j + 2] = p.z;
        bad = bad || !in_range3(p);
      }
    }
  }
  const bool any_bad = __any(bad), any_tilted = __any(tilted);
  if ((threadIdx.x & 63u) == 0) {
    if (any_bad) atomicOr(red + UR_NONFINITE, 1u);
    if (any_tilted) atomicOr(red + UR_TILTED, 1u);
  }
}

// One lane per triangle slot: the bounds of its face's world vertices and of its accept-region vertices, reduced
// over the scene (finite data: min / max in any order give the host's bounds).
__global__ void __launch_bounds__(256) k_upd_slot_bounds(uint32_t n_slots, uint32_t nf, uint32_t nv, const TriRec64* tris,
                                                         const uint32_t* fidx, const float* wv, const float* av, uint32_t* red) {
  const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
  float lo[6] = {INFINITY, INFINITY, INFINITY, INFINITY, INFINITY, INFINITY};
  float hi[6] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY, -INFINITY};
  if (sl < n_slots) {
    const uint32_t f = tris[sl].face;
    if (f < nf) {
      for (int j = 0; j < 3; j++) {
        const uint32_t v = fidx[3 * (size_t)f + j];
        if (v >= nv) continue;  // (never)
        const float* w = wv + 3 * (size_t)v;
        const float* a = av + 9 * (size_t)f + 3 * j;
        for (int k = 0; k < 3; k++) {
          lo[k] = fminf(lo[k], w[k]), hi[k] = fmaxf(hi[k], w[k]);
          lo[3 + k] = fminf(lo[3 + k], a[k]), hi[3 + k] = fmaxf(hi[3 + k], a[k]);
        }
      }
    }
  }
  for (int k = 0; k < 6; k++) { lo[k] = wave_min(lo[k]); hi[k] = wave_max(hi[k]); }
  if ((threadIdx.x & 63u) == 0)
    for (int k = 0; k < 3; k++) {
      atomicMin(red + UR_WLO + k, key_of(lo[k]));
      atomicMax(red + UR_WHI + k, key_of(hi[k]));
      atomicMin(red + UR_ALO + k, key_of(lo[3 + k]));
      atomicMax(red + UR_AHI + k, key_of(hi[3 + k]));
    }
}

// One lane per position of the partition's face order. The boxes' segments tile [0, nf); seg_start lists them by
// position, seg_box their boxes (creation order index), seg_first the rank of a box's first face (the counts of
// the boxes created before it, summed).
__global__ void __launch_bounds__(256) k_upd_ranks(uint32_t nf, uint32_t n_boxes, const int32_t* seg_start, const uint32_t* seg_box,
                                                   const uint32_t* seg_first, const int32_t* ids, FaceWords* face) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  if (p >= nf || n_boxes == 0) return;
  uint32_t a = 0, b = n_boxes;  // the last segment starting at or before p
  while (b - a > 1) {
    const uint32_t m = (a + b) >> 1;
    if ((uint32_t)seg_start[m] <= p) a = m; else b = m;
  }
  const int32_t f = ids[p];
  if (f < 0 || (uint32_t)f >= nf) return;  // (never: a permutation of the face ids)
  face[f].rank = seg_first[a] + (p - (uint32_t)seg_start[a]);
  face[f].box = seg_box[a];
}

// One lane per face: the flag bits of tri_flags into the box word k_upd_ranks wrote. bounds6: the boxes' low xyz,
// high xyz by box index.
__global__ void __launch_bounds__(256) k_upd_face_words(uint32_t nf, uint32_t nv, uint32_t n_boxes, const uint32_t* fidx, const float* ov3,
                                                        const float* wv, const float* vnn, const float* bounds6, float Ro,
                                                        FaceWords* face) {
  const uint32_t f = blockIdx.x * 256u + threadIdx.x;
  if (f >= nf) return;
  const uint32_t v0 = fidx[3 * (size_t)f], v1 = fidx[3 * (size_t)f + 1], v2 = fidx[3 * (size_t)f + 2];
  if (v0 >= nv || v1 >= nv || v2 >= nv) return;  // (never)
  const FaceWords fw = face[f];
  const uint32_t box = fw.box & kBoxIndexMask;
  if (box >= n_boxes) return;  // (never)
  const f3 n{fw.nx, fw.ny, fw.nz};
  const f3 w0 = ld3(wv + 3 * (size_t)v0), w1 = ld3(wv + 3 * (size_t)v1), w2 = ld3(wv + 3 * (size_t)v2);
  uint32_t flags = 0;
  if (safe_normal_of(w0, w1, w2, n, ld3(vnn + 3 * (size_t)v0), ld3(vnn + 3 * (size_t)v1), ld3(vnn + 3 * (size_t)v2)))
    flags |= kSafeNormalBit;
  if (Ro > 0.0f) {
    const double tilt = face_tilt_of(w0, w1, w2, n);
    const float* b = bounds6 + 6 * (size_t)box;
    if (tilt <= kCertNormalSin &&
        box_certified_of(ov3 + 3 * (size_t)v0, ov3 + 3 * (size_t)v1, ov3 + 3 * (size_t)v2, b, b + 3, Ro, tilt))
      flags |= kBoxCertBit;
  }
  face[f].box = box | flags;
}

}  // namespace rt
