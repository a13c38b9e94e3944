// rt_traverse.h -- the gfx950 wave-packet traversal of the MI355X ray-tracing hot path: scalar record loads and lane
// primitives, the counting run's slots, the ray and its culling set-up, the slab and triangle tests, the traversal
// loops and their octant dispatch. The lowest device header: rt_shade.h, the kernel headers (rt_frame_kernels.h,
// rt_ray_kernels.h, rt_view_kernels.h), rt_wavefront.h and the A/B variants (rt_variants.hip) build on it.
//
// Hot path (reference: src/flyscene.cpp:299-614):
//   one wave = one 8x8 pixel tile, one ray per lane; rays generated in registers (traceRayThread +
//   Camera::screenToWorld, fp64 NDC as camera.hpp:159-162);
//   wave-packet BVH traversal: every node record is fetched once per wave with a scalar load
//   (s_load_dwordx16 of the 64-B node), each lane slab-tests both children, the wave descends by
//   ballot (near child from the node's order bit for the wave's direction octant) and keeps ONE
//   traversal stack for the wave in LDS; lanes that cannot improve their hit simply vote "no", so the
//   wave stays converged and only visits nodes some lane still needs;
//   triangle test = the reference's calculateDistance/interpolateNormal arithmetic bit for bit
//   (flyscene.cpp:444-478,572-600), tie-break by reference iteration rank (calculateMinimumFace
//   keeps the first minimum, flyscene.cpp:381-391), plus the reference's own object-space box test
//   (intersectBox, flyscene.cpp:484-507) for the candidate's reference box;
//   shading (rt_shade.h) = calculateColor/calcSingleColor (flyscene.cpp:542-614); FULL mode adds the shadow any-hit
//   per light (flyscene.cpp:510-526) and the one reflection bounce of traceRay (flyscene.cpp:317-371).
// No MFMA: there is no dense contraction in this path.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rt_kat.h"
#include "rt_scene.h"

using rt::f3;

namespace rt {

// ------------------------------------------------------------------------------------------------
// uniform (scalar) loads: a generic pointer re-typed into the constant address space makes hipcc
// emit s_load_dwordx16 for wave-uniform indices (one fetch per wave, data in SGPRs)
// ------------------------------------------------------------------------------------------------
typedef int i16v __attribute__((ext_vector_type(16)));

// One s_load_dwordx16 per 64-B record (hipcc otherwise splits the record into x4/x8 pieces, one
// scalar-cache request each, and sinks parts below the first use). The wait is inside the asm
// because the compiler does not track the counter of an inline-asm load.
template <typename T>
__device__ __forceinline__ T sload64(const T* base, uint32_t i) {
  static_assert(sizeof(T) == 64, "64-byte records");
  const uint32_t off = __builtin_amdgcn_readfirstlane(i) * 64u;  // byte offset in an SGPR (< 4 GiB)
  // the base is uniform, but inside divergent regions (FULL mode's secondary packets) the compiler
  // may keep it in VGPRs; readfirstlane folds away when it is already scalar
  const uint64_t b = (uint64_t)base;
  const uint64_t bs = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  i16v v;
  asm volatile("s_load_dwordx16 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(bs), "s"(off) : "memory");
  T r;
  __builtin_memcpy(&r, &v, 64);
  return r;
}
// Interior node handles on the device are byte offsets of the node record (RT_BYTE_HANDLES, set by
// device_upload: index * 64, < 2^31 below kMaxFaces), so a node fetch needs no shift per step; leaf
// handles keep the (first triangle, count) form.
__device__ __forceinline__ uint32_t node_index(uint32_t h) { return h >> 6; }
__device__ __forceinline__ uint32_t node_offset(uint32_t h) { return h; }
__device__ __forceinline__ Node64 sload_node(const Node64* base, uint32_t h) { return sload64(base, node_index(h)); }
// The node fetch of the production loop, then a prefetch of both children's records into the scalar
// cache, issued the moment the node has arrived so that it overlaps this node's box tests (one dword
// each pulls in the 64-B line). The child offsets come from the record's own registers (Node64::pad0 /
// pad1, words 14 / 15 of the x16 load: the children's node records or, for a leaf child, its first
// triangle record, device_upload). The prefetch sinks pf0 / pf1 are carried from the previous node step
// ("+s"): this load's own s_waitcnt retires the previous step's prefetches, so a step needs no wait of
// its own (the caller waits once at the end of the traversal). The ray's reciprocal direction, passed
// through the prefetch asm as a read-write operand (a loop-carried copy, no move), keeps the box tests
// below it.
// Prefetch-offset check of the RT_CHECK_PREFETCH debug build (`make pfcheck`, DESIGN.md section 5 "scalar
// prefetch offsets"): an offset at or above its limit is recorded in bit `site` of *check and replaced by 0
// (a valid record), so a GPU run of the test suite with that build shows that no product loop issues an
// out-of-range scalar load -- without faulting the GPU. The product build compiles this to the offset.
__device__ __forceinline__ uint32_t pf_off(uint32_t off, uint32_t limit, uint32_t* check, int site) {
#ifdef RT_CHECK_PREFETCH
  if (off >= limit) {
    atomicOr(check, 1u << site);  // (a vector atomic from every active lane)
    return 0u;
  }
#endif
  (void)limit, (void)check, (void)site;
  return off;
}
__device__ __forceinline__ Node64 sload_node_pf_inreg(const DevScene& P, uint32_t h, uint32_t& pf0, uint32_t& pf1,
                                                      f3& id) {
  const uint32_t off = pf_off(node_offset(__builtin_amdgcn_readfirstlane(h)), P.rec_bytes, P.pf_check, 0);
  const uint64_t b = (uint64_t)P.nodes;
  const uint64_t bs = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  i16v v;
  asm volatile("s_load_dwordx16 %0, %3, %4\n\ts_waitcnt lgkmcnt(0)" : "=&s"(v), "+s"(pf0), "+s"(pf1) : "s"(bs), "s"(off) : "memory");
  Node64 r;
  __builtin_memcpy(&r, &v, 64);
  asm volatile("s_load_dword %0, %5, %6\n\ts_load_dword %1, %5, %7"
               : "+s"(pf0), "+s"(pf1), "+v"(id.x), "+v"(id.y), "+v"(id.z)
               : "s"(bs), "s"(pf_off(r.pad0, P.rec_bytes, P.pf_check, 1)), "s"(pf_off(r.pad1, P.rec_bytes, P.pf_check, 2))
               : "memory");
  return r;
}
__device__ __forceinline__ TriRec64 sload_tri(const TriRec64* base, uint32_t i) { return sload64(base, i); }
__device__ __forceinline__ uint32_t uniform(uint32_t x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ int lane_id() { return (int)__lane_id(); }
// The lane id recomputed where it is needed (v_mbcnt; volatile, so the compiler cannot reuse the entry's
// thread id and keep it live across the traversal -- in the FULL megakernel that value was spilled).
__device__ __forceinline__ uint32_t lane_id_fresh() {
  uint32_t l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}

// counters of the RT_FRAME_STATS counting run
// ST_WPOP / ST_WCULL (counting run, closest hit): stack pops per wave, and those pops at which no lane
// that wanted the entry still could (every such lane's entry distance into it, recorded at the push,
// now beyond its closest hit) -- what culling at the pop would save (rt_debug_counters)
// ST_WWIDE: 128-B fp32 4-wide node records fetched per wave (ST_WNODE: 64-B binary / quantised records)
// ST_WCAND / ST_WPRE / ST_WINS (counting run, per wave-level triangle test): some lane passed the plane-
// distance stage; some candidate lane's hit point lies inside the triangle's bounding box grown by 1e-3 of
// its extent (what a box prefilter would keep); some lane passed the reference's edge tests. ST_WE1 / ST_WE2:
// the staged edge tests left no candidate after the first / the second edge
enum { ST_NODE = 0, ST_TRI, ST_WNODE, ST_WTRI, ST_RAYS, ST_HITS, ST_TOTAL, ST_WPOP, ST_WCULL, ST_WWIDE,
       ST_WCAND, ST_WPRE, ST_WINS, ST_WE1, ST_WE2,
       // round 4: the same triangle-stage counts with the candidates restricted to the lanes whose ray entered
       // the leaf's box (ST_WCANDM .. ST_WINSM), the triangle tests of leaves reached by descent (ST_WTRID) and
       // their entry-masked candidate count (ST_WCANDD: popped leaves unmasked), and wave-level tests where a
       // lane that never entered the leaf accepted (ST_WACCX: 0 if leaf-entry masking is exact)
       ST_WCANDM, ST_WE1M, ST_WE2M, ST_WINSM, ST_WTRID, ST_WCANDD, ST_WACCX,
       // round 5: the packet -> per-lane hybrid model. ST_HN0 .. ST_HN0 + 6: node steps
       // by the number of lanes whose ray entered the node (bins 0, 1, 2-3, 4-7, 8-15, 16-31, 32-64);
       // ST_HL0 .. + 6: the same for leaf visits. Per threshold k of kHybridK (3 thresholds): once the lanes
       // entering a node fall below k, that node's subtree is a "switched region" (it ends at the first
       // pop below the depth where it began); ST_HPN/ST_HPT + i: the packet's node steps / triangle tests
       // inside such regions, ST_HLN/ST_HLT + i: the per-lane cost of the same regions (the maximum over the
       // wave's lanes of the steps / tests whose node the lane entered, summed over regions) -- what a wave
       // walking those regions one ray per lane would spend
       ST_HN0, ST_HL0 = ST_HN0 + 7, ST_HPN = ST_HL0 + 7, ST_HPT = ST_HPN + 3, ST_HLN = ST_HPT + 3, ST_HLT = ST_HLN + 3,
       // round 6: the FULL megakernel's packet walks by phase p (0 primary, 1 shadows of the
       // primary hits, 2 reflection, 3 shadows of the reflection hits): walks with some active lane (ST_PW + p), the
       // active lanes at their entry summed (ST_PL + p), their node steps (ST_PS + p) and triangle tests (ST_PT + p);
       // ST_PH + b: the secondary phases' node steps by the walk's active lanes at entry (1-8, 9-16, 17-32, 33-48,
       // 49-64)
       ST_PW = ST_HLT + 3, ST_PL = ST_PW + 4, ST_PS = ST_PL + 4, ST_PT = ST_PS + 4, ST_PH = ST_PT + 4,
       ST_COUNT = ST_PH + 5 };
constexpr int kStatSlots = 80;
static_assert(ST_COUNT <= kStatSlots, "stat slots");
constexpr int kHybridK[3] = {4, 8, 16};
__device__ __forceinline__ int lane_bin(uint32_t n) { return n == 0 ? 0 : n == 1 ? 1 : n < 4 ? 2 : n < 8 ? 3 : n < 16 ? 4 : n < 32 ? 5 : 6; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
  for (int off = 32; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}

struct Hit {
  float t;
  uint32_t rank;
  uint32_t slot;
};

struct Ray {
  f3 o, d;      // world space (triangle tests)
  f3 id;        // culling: 1/d (zeros nudged)
  f3 oa, ob;    // culling: -(o + p)/d and -(o - p)/d, the lo / hi plane offsets of boxes grown by p
  f3 o2;        // object space (reference intersectBox): Minv*o_box; its direction normalized(MS*d) is
                // formed where the exact box test needs it (ref_box_test), off the traversal's registers
};

__device__ __forceinline__ float nudge(float x) { return fabsf(x) < 1e-20f ? copysignf(1e-20f, x) : x; }

// Culling set-up of a ray, once per ray.
// The BVH boxes carry a static pad for the scene-scale rounding of the reference's arithmetic (bvh_pad,
// rt_layout.cpp). The rounding of the reference's hit point P = o + t d, and of this slab test, also grows
// with the ray origin's magnitude: both are a few ulp of |o| + |t d| <= 2|o| + R per axis (R: the scene's
// magnitude). So every ray grows the boxes it tests by its own pad p = kCullPadRel * |o|_inf, folded into
// two per-axis offsets: with box [lo - p, hi + p] the plane distances are fma(lo, 1/d, -(o + p)/d) and
// fma(hi, 1/d, -(o - p)/d). That costs no instruction per node (the octant loops pick the offset of each
// plane at compile time). kCullPadRel = 4e-5 is ~100x the worst-case rounding (<= 6 ulp of |o|, each
// 2^-24 |o|), so for every origin the culling never drops a face the reference accepts.
// Outside the range where these products stay finite (|o|_inf > 1e18, |d|_inf outside [1e-12, 1e18], or
// non-finite input) the ray's boxes grow without bound instead: p = inf, every box is entered, and the
// packet tests every triangle with the exact test -- still the reference's result, by brute force.
constexpr float kCullPadRel = 4e-5f, kCullOriginMax = 1e18f, kCullDirMin = 1e-12f, kCullDirMax = 1e18f;
// The ray's own pad is needed only once it exceeds the static one (every box already carries
// static_pad >= the ray's pad, so the same ~100x margin holds): for origins near the scene -- every
// secondary ray, and primary rays of an eye near it -- the boxes keep exactly their static size.
__device__ __forceinline__ void setup_cull(Ray& r, float static_pad) {
  const float om = fmaxf(fmaxf(fabsf(r.o.x), fabsf(r.o.y)), fabsf(r.o.z));
  const float dm = fmaxf(fmaxf(fabsf(r.d.x), fabsf(r.d.y)), fabsf(r.d.z));
  const bool certified = om <= kCullOriginMax && dm >= kCullDirMin && dm <= kCullDirMax;  // false for NaN
  if (certified) {
    r.id = f3{__builtin_amdgcn_rcpf(nudge(r.d.x)), __builtin_amdgcn_rcpf(nudge(r.d.y)),
              __builtin_amdgcn_rcpf(nudge(r.d.z))};
    const float pr = kCullPadRel * om;
    const float p = pr > static_pad ? pr : 0.0f;
    r.oa = f3{-(r.o.x + p) * r.id.x, -(r.o.y + p) * r.id.y, -(r.o.z + p) * r.id.z};
    r.ob = f3{-(r.o.x - p) * r.id.x, -(r.o.y - p) * r.id.y, -(r.o.z - p) * r.id.z};
  } else {
    // unbounded boxes: lo planes at -inf, hi planes at +inf along the (kept) direction signs
    r.id = f3{copysignf(1.0f, nudge(r.d.x)), copysignf(1.0f, nudge(r.d.y)), copysignf(1.0f, nudge(r.d.z))};
    r.oa = f3{-r.id.x * INFINITY, -r.id.y * INFINITY, -r.id.z * INFINITY};
    r.ob = f3{r.id.x * INFINITY, r.id.y * INFINITY, r.id.z * INFINITY};
  }
}

// Conservative slab test for one padded child box (culling only; exactness comes from padding):
// returns the entry distance tmin and the exit distance clipped to [0, tmax_ray] (hit iff tmin <= tmax)
struct Span {
  float tmin, tmax;
};
__device__ __forceinline__ Span slab(float lx, float hx, float ly, float hy, float lz, float hz, const Ray& r,
                                     float tmax_ray) {
  const float tx0 = __builtin_fmaf(lx, r.id.x, r.oa.x), tx1 = __builtin_fmaf(hx, r.id.x, r.ob.x);
  const float ty0 = __builtin_fmaf(ly, r.id.y, r.oa.y), ty1 = __builtin_fmaf(hy, r.id.y, r.ob.y);
  const float tz0 = __builtin_fmaf(lz, r.id.z, r.oa.z), tz1 = __builtin_fmaf(hz, r.id.z, r.ob.z);
  Span s;
  s.tmin = fmaxf(fmaxf(fminf(tx0, tx1), fminf(ty0, ty1)), fmaxf(fminf(tz0, tz1), 0.0f));
  s.tmax = fminf(fminf(fmaxf(tx0, tx1), fmaxf(ty0, ty1)), fminf(fmaxf(tz0, tz1), tmax_ray));
  return s;
}
// The same span when the wave's active rays share one direction octant (OCT bit k: axis k negative,
// by the sign of the nudged reciprocal): fma(., id, offset) is monotone in the box coordinate, so the
// near / far plane of each axis is known and min(t0, t1) / max(t0, t1) are exactly the near / far
// values -- identical results with 8 fewer min/max per child. OCT < 0: the generic test. (An unclipped
// entry distance for packets starting in front of the scene measured within noise, r03_micro_ab.txt.)
template <int OCT>
__device__ __forceinline__ Span slab_o(float lx, float hx, float ly, float hy, float lz, float hz, const Ray& r,
                                       float tmax_ray) {
  if (OCT < 0) return slab(lx, hx, ly, hy, lz, hz, r, tmax_ray);
  // near plane of a positive axis: lo (offset oa); of a negative axis: hi (offset ob); far the other
  const float nx = (OCT & 1) ? hx : lx, fx = (OCT & 1) ? lx : hx;
  const float ny = (OCT & 2) ? hy : ly, fy = (OCT & 2) ? ly : hy;
  const float nz = (OCT & 4) ? hz : lz, fz = (OCT & 4) ? lz : hz;
  const float nox = (OCT & 1) ? r.ob.x : r.oa.x, fox = (OCT & 1) ? r.oa.x : r.ob.x;
  const float noy = (OCT & 2) ? r.ob.y : r.oa.y, foy = (OCT & 2) ? r.oa.y : r.ob.y;
  const float noz = (OCT & 4) ? r.ob.z : r.oa.z, foz = (OCT & 4) ? r.oa.z : r.ob.z;
  Span s;
  s.tmin = fmaxf(fmaxf(__builtin_fmaf(nx, r.id.x, nox), __builtin_fmaf(ny, r.id.y, noy)),
                 fmaxf(__builtin_fmaf(nz, r.id.z, noz), 0.0f));
  // min of the three far planes and tmax_ray in two instructions (the compiler's fminf would first
  // canonicalise tmax_ray, a loop-carried value, with an extra v_max per node)
  asm("v_min3_f32 %0, %1, %2, %3\n\tv_min_f32 %0, %0, %4"
      : "=&v"(s.tmax)
      : "v"(__builtin_fmaf(fx, r.id.x, fox)), "v"(__builtin_fmaf(fy, r.id.y, foy)),
        "v"(__builtin_fmaf(fz, r.id.z, foz)), "v"(tmax_ray));
  return s;
}
// lane masks straight from v_cmp (no bool materialisation): llvm.amdgcn.fcmp predicates
constexpr int kFcmpOLE = 5;
__device__ __forceinline__ uint64_t mask_le(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, kFcmpOLE); }

// The reference's object-space box test, exact (flyscene.cpp:484-507): origin Minv*o (Ray::o2), direction
// (MS*d).normalized() with MS the linear block of Minv (flyscene.cpp:486-487; m3v3's Matrix3f order)
__device__ __forceinline__ bool ref_box_test(const DevScene& S, const Ray& r, const float* bx) {
  const float MS[9] = {S.Minv[0], S.Minv[1], S.Minv[2], S.Minv[4], S.Minv[5], S.Minv[6], S.Minv[8], S.Minv[9], S.Minv[10]};
  const f3 dd = normalized(m3v3(MS, r.d));
  const float lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[4], bx[5], bx[6]};
  const float o2[3] = {r.o2.x, r.o2.y, r.o2.z}, d2[3] = {dd.x, dd.y, dd.z};
  float tin3[3], tout3[3];
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float a = (lo[k] - o2[k]) / d2[k];
    const float b = (hi[k] - o2[k]) / d2[k];
    tin3[k] = smin(a, b);
    tout3[k] = smax(a, b);
  }
  const float tin = smax(tin3[0], smax(tin3[1], tin3[2]));
  const float tout = smin(tout3[0], smin(tout3[1], tout3[2]));
  return !(tin > tout || tout < 0);
}

__device__ __forceinline__ f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }

// Lane masks straight from the compares (llvm.amdgcn.fcmp / icmp predicates): candidate sets stay in
// SGPR pairs and wave-level decisions are one s_cmp, with no bool materialisation in VGPRs
constexpr int kFcmpOEQ = 1, kFcmpOGE = 3, kFcmpOLT = 4, kFcmpUNE = 14, kIcmpULT = 36;
template <int PRED>
__device__ __forceinline__ uint64_t fmask(float a, float b) { return __builtin_amdgcn_fcmpf(a, b, PRED); }
__device__ __forceinline__ bool lane_in(uint64_t m) { return __builtin_amdgcn_inverse_ballot_w64(m); }

// LATE (the octant loops of the binary-only fused PRIMARY kernel, whose slot is an SGPR): the shading record's
// address is formed inside the uncertified-normal branch from an opaque copy of the slot. Left to itself the
// compiler makes 48 * slot a 64-bit induction variable of every leaf loop -- 8 SALU per leaf and 2 per record on
// the scalar chain -- for a branch that certified faces never take (SALU per wave 1,998 -> 1,875 on the 1M
// soup, profiles/ab/leaf_records_ab.txt). Other kernels keep the plain form: applied to every kernel the same
// edit changed the low bits of one colour in the wavefront counting kernel.
template <bool LATE = false>
__device__ __forceinline__ uint64_t accept_candidate(const DevScene& P, const TriRec64& tr, uint32_t slot, f3 e0, f3 e2,
                                                    f3 a0, f3 a1, f3 a2, f3 p, const Ray& r, uint64_t cand) {
  if (!(tr.box & kSafeNormalBit)) {  // uniform branch: only faces the host could not certify
    const float area0 = norm(a0) / 2, area1 = norm(a1) / 2, area2 = norm(a2) / 2;
    const float area = norm(cross(e0, neg(e2))) / 2;
    uint32_t us = slot;
    if constexpr (LATE) asm volatile("" : "+s"(us));
    const float* fs = P.fshade + 12 * (size_t)us;
    const f3 n0 = ld3(fs), n1 = ld3(fs + 4), n2 = ld3(fs + 8);
    const f3 nn = blend_normal(n0, n1, n2, area0, area1, area2, area);
    cand &= fmask<kFcmpUNE>(norm(nn), 0.0f);
  }
  if (tr.box & kBoxCertBit) {
    // certified face (kBoxCertBit): the predicate holds for every candidate lane whose object-space
    // origin is within the certified range (NaN fails the compare and takes the path below)
    const float om = fmaxf(fmaxf(fabsf(r.o2.x), fabsf(r.o2.y)), fabsf(r.o2.z));
    if ((cand & ~ballot(om <= P.cert_origin_max)) == 0) return cand;
  }
  // reference box predicate. Fast path: the object-space hit point lies inside the reference box
  // with a margin (1e-5 relative) far above the reference slab test's rounding, so the exact ray
  // crosses the box interior at t >= 0 and intersectBox accepts. Otherwise run the exact test.
  const float* bx = P.refbox + 8 * (size_t)(tr.box & kBoxIndexMask);
  const f3 X = affv3(P.Minv, p);
  const float lo[3] = {bx[0], bx[1], bx[2]}, hi[3] = {bx[4], bx[5], bx[6]};
  const float xs[3] = {X.x, X.y, X.z}, os[3] = {r.o2.x, r.o2.y, r.o2.z};
  bool inside = true;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float m = 1e-5f * ((hi[k] - lo[k]) + fabsf(lo[k]) + fabsf(hi[k]) + fabsf(os[k])) + 1e-30f;
    inside = inside & (xs[k] > lo[k] + m) & (xs[k] < hi[k] - m);
  }
  const uint64_t ins = ballot(inside);
  if ((cand & ~ins) == 0) return cand;
  return cand & (ins | ballot(ref_box_test(P, r, bx)));
}

// The wave-level occluder cache of the memory-lights kernels (calc_color): the triangle slots at which lanes of
// this wave last became blocked, most recent first; kOccNone = empty
constexpr int kOccK = 2;
constexpr uint32_t kOccNone = 0xFFFFFFFFu;
__device__ __forceinline__ void occ_push(uint32_t* occ, uint32_t slot) {
#pragma unroll
  for (int k = kOccK - 1; k > 0; k--) occ[k] = occ[k - 1];
  occ[0] = slot;
}

// calculateDistance (flyscene.cpp:444-478) against a wave-uniform triangle record, for the lanes of
// `act`. CLOSEST: update (t, rank, slot) if 0 <= t < best (rank breaks ties as the reference's order
// does). ANY: any valid t >= 0 (shadow(), flyscene.cpp:519).
template <bool ANY, bool STATS = false, bool LATE = false>
__device__ __forceinline__ void test_tri(const DevScene& P, const TriRec64& tr, uint32_t slot, const Ray& r,
                                         uint64_t act, Hit& h, bool& found, uint32_t* cnt = nullptr,
                                         uint64_t entry = ~0ull, bool desc = false, uint32_t* occ = nullptr) {
  const f3 n{tr.nx, tr.ny, tr.nz};
  const float dn = dot(n, r.d);                 // facenormal.dot(dir)
  const float orth = tr.dist - dot(r.o, n);     // distancePlane - origin.dot(facenormal)
  const float t = orth / dn;                    // / dir.dot(facenormal)  (same bits as dn)
  uint64_t cand;
  if (!ANY) {
    // dn != 0 && 0 <= t < inf in one class test: t is -0, +0, +denormal or +normal (dn == 0 makes t
    // +-inf or NaN, which the class excludes as the separate tests did)
    uint64_t cls;
    asm("v_cmp_class_f32_e64 %0, %1, %2" : "=s"(cls) : "v"(t), "v"(0x1E0u));
    cand = act & cls &
           (fmask<kFcmpOLT>(t, h.t) | (fmask<kFcmpOEQ>(t, h.t) & __builtin_amdgcn_uicmp(tr.rank, h.rank, kIcmpULT)));
  } else {
    cand = act & fmask<kFcmpUNE>(dn, 0.0f) & fmask<kFcmpOGE>(t, 0.0f);
  }
  if (STATS) cnt[ST_WCAND] += cand != 0;
  const f3 p{r.o.x + t * r.d.x, r.o.y + t * r.d.y, r.o.z + t * r.d.z};
  const f3 w0{tr.w0x, tr.w0y, tr.w0z}, w1{tr.w1x, tr.w1y, tr.w1z}, w2{tr.w2x, tr.w2y, tr.w2z};
  if (STATS) {
    // entry-masked stage counts: all three edge masks evaluated for every lane, the stages derived
    const uint64_t cm = cand & entry;
    const uint64_t b0 = ballot(dot(n, cross(sub(w1, w0), sub(p, w0))) < 0);
    const uint64_t b1 = ballot(dot(n, cross(sub(w2, w1), sub(p, w1))) < 0);
    const uint64_t b2 = ballot(dot(n, cross(sub(w0, w2), sub(p, w2))) < 0);
    cnt[ST_WCANDM] += cm != 0;
    cnt[ST_WE1M] += cm != 0 && (cm & ~b0) == 0;
    cnt[ST_WE2M] += (cm & ~b0) != 0 && (cm & ~b0 & ~b1) == 0;
    cnt[ST_WINSM] += (cm & ~b0 & ~b1 & ~b2) != 0;
    if (desc) cnt[ST_WTRID]++;
    cnt[ST_WCANDD] += (cand & (desc ? entry : ~0ull)) != 0;
  }
  if (cand == 0) return;
  if (STATS) {
    const f3 lo{fminf(fminf(w0.x, w1.x), w2.x), fminf(fminf(w0.y, w1.y), w2.y), fminf(fminf(w0.z, w1.z), w2.z)};
    const f3 hi{fmaxf(fmaxf(w0.x, w1.x), w2.x), fmaxf(fmaxf(w0.y, w1.y), w2.y), fmaxf(fmaxf(w0.z, w1.z), w2.z)};
    const float m = 1e-3f * fmaxf(fmaxf(hi.x - lo.x, hi.y - lo.y), hi.z - lo.z);
    const bool in = p.x >= lo.x - m && p.x <= hi.x + m && p.y >= lo.y - m && p.y <= hi.y + m &&
                    p.z >= lo.z - m && p.z <= hi.z + m;
    cnt[ST_WPRE] += (cand & ballot(in)) != 0;
  }
  // the record is wave-uniform (SGPRs) and a VALU op reads at most one SGPR: w0 and w1 copied into
  // VGPRs once serve all three edge differences (6 moves instead of 9; same float operations)
  f3 v0 = w0, v1 = w1;
  asm("" : "+v"(v0.x), "+v"(v0.y), "+v"(v0.z), "+v"(v1.x), "+v"(v1.y), "+v"(v1.z));
  const f3 e0 = sub(w1, v0), e1 = sub(w2, v1), e2 = sub(v0, w2);
  // the reference's three edge tests are independent (interpolateNormal, flyscene.cpp:591: rejected if any is
  // negative), so they run one at a time and the wave stops as soon as no candidate lane is left --
  // the same values, the same set; a packet wholly beyond one edge line skips the other edges' work
  const f3 a0 = cross(e0, sub(p, w0));
  cand &= ~ballot(dot(n, a0) < 0);
  if (STATS) cnt[ST_WE1] += cand == 0;
  if (cand == 0) return;
  const f3 a1 = cross(e1, sub(p, w1));
  cand &= ~ballot(dot(n, a1) < 0);
  if (STATS) cnt[ST_WE2] += cand == 0;
  if (cand == 0) return;
  const f3 a2 = cross(e2, sub(p, w2));
  cand &= ~ballot(dot(n, a2) < 0);
  if (STATS) cnt[ST_WINS] += cand != 0;
  if (cand == 0) return;
  const bool acc = lane_in(accept_candidate<LATE>(P, tr, slot, e0, e2, a0, a1, a2, p, r, cand));
  if (STATS) cnt[ST_WACCX] += (ballot(acc) & ~entry) != 0;
  if (ANY) {
    // occluder cache (calc_color, memory-lights kernels only; null everywhere else): the slot at which some
    // lane first became blocked goes to the front of the wave's last kOccK occluders
    if (occ != nullptr && ballot(acc && !found) != 0) occ_push(occ, slot);
    found = found | acc;
  } else {
    h.t = acc ? t : h.t;
    h.rank = acc ? tr.rank : h.rank;
    h.slot = acc ? slot : h.slot;
  }
}

// ------------------------------------------------------------------------------------------------
// Wave-packet traversal. STACK_LDS selects the wave stack home: LDS (one uint32 row per wave) or the
// 64 lanes of one VGPR (v_writelane / v_readlane with an SGPR lane index).
// ------------------------------------------------------------------------------------------------
// Wave-packet loop with every option: VGPR or LDS stack and the counting run (RT_FRAME_STATS). The
// production closest-hit / any-hit path is traverse_fast() below (same visit order, leaner per-node
// code); this loop serves the counting run and the VGPR-stack A/B variant (rt_variants.hip). Octant-
// specialised loops take the near child from the node's precomputed order bit for the wave's octant
// (split-axis rule, octant_order() in rt_layout.cpp) instead of a lane-majority vote: 3 fewer SALU and one
// fewer v_cmp per node step (C3 +3.7% at 4 frames in flight, bunny +2.6%).
// Node64::pad0 / pad1 hold the children's record offsets (multiples of 64, the prefetch targets), so the
// eight octant order bits travel in their low bits: octants 0-5 in pad0 bits 0-5, octants 6-7 in pad1
// bits 0-1. A scalar load ignores the two low offset bits and the rest stays inside the 64-B record,
// so the prefetch still touches the child's cache line.
template <int OCT>
__device__ __forceinline__ uint32_t order_word(const Node64& nd) {
  return OCT < 6 ? nd.pad0 : nd.pad1;
}
template <int OCT>
constexpr int order_bit() {
  return OCT < 6 ? OCT : OCT - 6;
}
template <bool ANY, bool STATS, bool STACK_LDS, int OCT = -1>
__device__ __forceinline__ void traverse(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                         uint32_t* lds_stack, uint32_t* cnt, uint32_t* occ = nullptr) {
  if (P.n_nodes == 0) return;
  uint32_t stackv = 0;     // lane k holds stack entry k (VGPR stack)
  int sp = 0;              // wave-uniform stack depth (SGPR)
  uint64_t flagstack = 0;  // STATS: per-lane "my ray wanted this entry" bit per stack level
  float tstack[STATS ? 64 : 1];  // STATS: per-lane entry distance into each stack entry
  bool want = active;      // STATS: this lane's ray intersects the current node
  bool desc = false;       // STATS: the current node was reached by descent (not popped)
  uint32_t node = P.root;
  const float tmax_any = INFINITY;
  uint64_t act = ballot(active);  // lanes still tracing (wave-uniform mask)
  // STATS, hybrid model (ST_HPN ..): per threshold, the stack depth where the current switched region began
  // (-1: none) and this lane's node steps / triangle tests inside it
  int hr[3] = {-1, -1, -1};
  uint32_t hln[3] = {0, 0, 0}, hlt[3] = {0, 0, 0};
  auto hybrid_close = [&](int depth) {  // regions that began deeper than `depth` end here
#pragma unroll
    for (int i = 0; i < 3; i++)
      if (hr[i] >= 0 && depth < hr[i]) {
        cnt[ST_HLN + i] += wave_max_u32(hln[i]);
        cnt[ST_HLT + i] += wave_max_u32(hlt[i]);
        hln[i] = hlt[i] = 0;
        hr[i] = -1;
      }
  };
  // one pop site and branch-free pushes keep the per-node control flow to the two uniform branches
  // (interior vs leaf, pop vs descend)
  for (;;) {
    bool pop = true;
    if (STATS) {
      const uint32_t nw = (uint32_t)__popcll(ballot(want) & act);
      cnt[(is_leaf(node) ? ST_HL0 : ST_HN0) + lane_bin(nw)]++;
#pragma unroll
      for (int i = 0; i < 3; i++) {
        if (hr[i] < 0 && nw < (uint32_t)kHybridK[i]) hr[i] = sp;
        if (hr[i] >= 0) {
          if (!is_leaf(node)) {
            cnt[ST_HPN + i]++;
            hln[i] += want ? 1u : 0u;
          } else {
            cnt[ST_HPT + i] += leaf_count(node);
            hlt[i] += want ? leaf_count(node) : 0u;
          }
        }
      }
    }
    if (!is_leaf(node)) {
      const Node64 nd = sload_node(P.nodes, node);  // one scalar 64-B fetch per wave
      if (STATS) {
        if (want) cnt[ST_NODE]++;
        cnt[ST_WNODE]++;
      }
      const float tcut = ANY ? tmax_any : h.t;
      const Span s0 = slab_o<OCT>(nd.c0lx, nd.c0hx, nd.c0ly, nd.c0hy, nd.c0lz, nd.c0hz, r, tcut);
      const Span s1 = slab_o<OCT>(nd.c1lx, nd.c1hx, nd.c1ly, nd.c1hy, nd.c1lz, nd.c1hz, r, tcut);
      const uint64_t m0 = mask_le(s0.tmin, s0.tmax) & act, m1 = mask_le(s1.tmin, s1.tmax) & act;
      bool first0;
      if (OCT >= 0) {
        // the node's order bit for this octant, overridden when only one child is needed
        const bool pref1 = (order_word<OCT>(nd) >> order_bit<OCT>()) & 1u;
        first0 = m1 == 0 || (m0 != 0 && !pref1);
      } else {
        // near child first by lane majority: each lane that needs a child votes for the one it enters
        // first (covers m0 == 0 -> child 1 and m1 == 0 -> child 0)
        const uint64_t v0 = m0 & (~m1 | mask_le(s0.tmin, s1.tmin));
        first0 = 2 * __popcll(v0) >= __popcll(m0 | m1);
      }
      const uint32_t far = first0 ? nd.child1 : nd.child0;
      // the far child is written above the top unconditionally and kept only when both are needed
      if (STACK_LDS) lds_stack[sp] = far;
      else asm volatile("s_mov_b32 m0, %2\n\tv_writelane_b32 %0, %1, m0"
                        : "+v"(stackv)
                        : "s"(uniform(far)), "s"(uniform((uint32_t)sp))
                        : "m0");
      if (STATS) {
        const bool h0 = (m0 >> lane_id()) & 1, h1 = (m1 >> lane_id()) & 1;
        const bool wf = first0 ? h1 : h0;
        flagstack = (flagstack & ~(1ull << sp)) | ((uint64_t)wf << sp);
        want = first0 ? h0 : h1;
        desc = true;
        tstack[sp] = first0 ? s1.tmin : s0.tmin;
      }
      sp += ((m0 != 0) & (m1 != 0)) ? 1 : 0;
      node = first0 ? nd.child0 : nd.child1;
      pop = (m0 | m1) == 0;
    } else {
      // leaf: its triangles are fetched once per wave and tested by every lane
      const uint32_t first = leaf_first(node), count = leaf_count(node);
      if (STATS) {
        if (want) cnt[ST_TRI] += count;
        cnt[ST_WTRI] += count;
      }
      for (uint32_t k = 0; k < count; k++) {
        const TriRec64 tr = sload_tri(P.tris, first + k);
        test_tri<ANY, STATS>(P, tr, first + k, r, act, h, found, cnt, STATS ? ballot(want) : ~0ull, desc, occ);
      }
      if (ANY) {
        active = active & !found;
        act = ballot(active);
        if (!act) break;
      }
    }
    if (pop) {
      if (sp == 0) break;
      sp--;
      node = STACK_LDS ? uniform(lds_stack[sp]) : (uint32_t)__builtin_amdgcn_readlane(stackv, sp);
      if (STATS) {
        want = (flagstack >> sp) & 1;
        desc = false;
        cnt[ST_WPOP]++;
        if (!ANY && ballot(want && tstack[sp] <= h.t) == 0) cnt[ST_WCULL]++;
        hybrid_close(sp);  // the popped entry lies outside regions that began deeper than it
      }
    }
  }
  if (STATS) hybrid_close(-1);
}

// ------------------------------------------------------------------------------------------------
// The production packet loop (LDS wave stack, no counting): the same visit order as traverse(), with
// the per-node work arranged for the scalar unit, which is this kernel's tightest resource (measured:
// one extra SALU per node step costs ~0.9% of the trace time, one extra VALU ~0.2%):
//  * the descend / push / pop decision is one straight-line SALU block; a pop is signalled by the
//    marker handle kPopMarker (leaf bit set, never a real leaf), so the interior loop needs one
//    compare-and-branch per step and there is a single pop site;
//  * lanes without a ray (closest hit) carry t_best = -1 and lanes whose shadow ray is blocked (any
//    hit) carry a box-test limit of -1, so every box test fails for them and the masks need no
//    "& active lanes" step.
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kPopMarker = 0xFFFFFFFFu;

// Leaf entry of the binary loops: touch the leaf's triangle records [from, count) (one s_load_dword per 64-B
// record into a prefetch sink; the parent's prefetch already brought record 0), so that their scalar-cache
// misses overlap one another and the first record's instead of following each test (C5 +4%, C3 unchanged:
// profiles/ab/r04_leaf_prefetch_ab.txt). The wide loop's parent prefetch covers records 0 and 1 already.
__device__ __forceinline__ void leaf_prefetch(const DevScene& P, uint64_t bs, uint32_t first, uint32_t from, uint32_t count,
                                              uint32_t& sink) {
  for (uint32_t k = from; k < count; k++)
    asm volatile("s_load_dword %0, %1, %2" : "+s"(sink) : "s"(bs), "s"(pf_off((first + k) * 64u, P.tri_bytes, P.pf_check, 3))
                 : "memory");
}

// the fast loop's wave-stack push as inline asm: a ds_write issued where it stands (the compiler would
// otherwise schedule the store with the decision block at the end of the step)
__device__ __forceinline__ void lds_push(uint32_t* slot, uint32_t v) {
  const uint32_t a = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)slot;
  asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory");
}
// traverse_fast from a given state (node handle, stack depth): the whole traversal starts at the root
// with an empty stack. Per node step (octant loops): the node record arrives with one s_load_dwordx16;
// the same asm then prefetches both children's records into the scalar cache (offsets in the record's
// pad0 / pad1), the sinks carried to the next step, whose own wait retires them; the far child (fixed
// by the node's order bit for this octant) is pushed at once; both slab tests give the lane masks; an
// 8-SALU block picks the next node (near child, the one child needed, or the pop marker) and keeps the
// push only when both children are needed.
// LATE: accept_candidate's form for the octant loops of the fused PRIMARY kernel.
template <bool ANY, int OCT, bool LATE = false>
__device__ __forceinline__ void traverse_fast_from(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                                   uint32_t* lds_stack, uint32_t node, int sp, uint32_t* occ = nullptr) {
  // lanes still tracing: used by the any-hit triangle tests only (a closest-hit lane without a ray
  // carries t_best = -1, which no candidate t >= -0 passes, so its triangle tests need no mask)
  uint64_t act = ANY ? ballot(active) : ~0ull;
  float tlim = active ? INFINITY : -1.0f;  // ANY: box-test limit (-1 once the lane is blocked)
  if (!ANY && !active) h.t = -1.0f;
  uint32_t cpf0 = 0, cpf1 = 0;  // prefetch sinks, live across the traversal
  f3 rid = r.id;  // loop-carried copy threaded through the prefetch asm
  for (;;) {
    while (!is_leaf(node)) {
      const Node64 nd = sload_node_pf_inreg(P, node, cpf0, cpf1, rid);
      // octant loops: when both children are needed the far one is fixed by the node's order bit for
      // this octant alone, so it is chosen and pushed the moment the node has arrived -- the LDS write
      // completes under the box tests instead of delaying the next node fetch
      uint32_t nearb = 0, farb = 0;
      if (OCT >= 0) {
        sp = (int)uniform((uint32_t)sp);
        asm("s_bitcmp1_b32 %[bits], %[oct]\n\t"
            "s_cselect_b32 %[nb], %[c1], %[c0]\n\t"
            "s_cselect_b32 %[fb], %[c0], %[c1]"
            : [nb] "=&s"(nearb), [fb] "=&s"(farb)
            : [bits] "s"(uniform(order_word<OCT>(nd))), [oct] "i"(order_bit<OCT>()), [c0] "s"(uniform(nd.child0)),
              [c1] "s"(uniform(nd.child1))
            : "scc");
        lds_push(lds_stack + sp, farb);
      }
      const float tcut = ANY ? tlim : h.t;
      Ray rb = r;
      rb.id = rid;
      const Span s0 = slab_o<OCT>(nd.c0lx, nd.c0hx, nd.c0ly, nd.c0hy, nd.c0lz, nd.c0hz, rb, tcut);
      const Span s1 = slab_o<OCT>(nd.c1lx, nd.c1hx, nd.c1ly, nd.c1hy, nd.c1lz, nd.c1hz, rb, tcut);
      const uint64_t m0 = mask_le(s0.tmin, s0.tmax), m1 = mask_le(s1.tmin, s1.tmax);
      uint32_t nxt, far, ta, tb;
      uint64_t tt;
      // (uniform(): inside FULL mode's divergent regions the compiler may otherwise hand the scalar
      // decision block values it keeps in VGPRs; readfirstlane folds away on SGPR values)
      sp = (int)uniform((uint32_t)sp);
      const uint32_t c0 = uniform(nd.child0), c1 = uniform(nd.child1);
      uint32_t* const slot = lds_stack + sp;
      if (OCT >= 0) {
        // both needed: the near child chosen above; one needed: that one; none: the pop marker.
        // 8 SALU: any1 picks (c1 | pop) and (near | c0), any0 then chooses between them; both -> push
        asm("s_cmp_lg_u64 %[m1], 0\n\t"
            "s_cselect_b32 %[nxt], %[c1], -1\n\t"
            "s_cselect_b32 %[ta], %[nb], %[c0]\n\t"
            "s_cselect_b64 %[tt], %[m0], 0\n\t"
            "s_cmp_lg_u64 %[m0], 0\n\t"
            "s_cselect_b32 %[nxt], %[ta], %[nxt]\n\t"
            "s_cmp_lg_u64 %[tt], 0\n\t"
            "s_addc_u32 %[sp], %[sp], 0"
            : [nxt] "=&s"(nxt), [sp] "+s"(sp), [tt] "=&s"(tt), [ta] "=&s"(ta)
            : [m0] "s"(m0), [m1] "s"(m1), [c0] "s"(c0), [c1] "s"(c1), [nb] "s"(nearb)
            : "scc");
        far = farb;
        (void)ta;
        (void)tb;
      } else {
        // mixed-octant packets: near child by lane majority -- each lane that needs a child votes for
        // the one it enters first (v0: lanes voting child 0; 2 * |v0| >= |m0 | m1| picks child 0, which
        // also covers m1 == 0); the far child is written above the top unconditionally and kept only
        // when both are needed
        const uint64_t le = mask_le(s0.tmin, s1.tmin);
        asm("s_orn2_b64 %[tt], %[le], %[m1]\n\t"
            "s_and_b64 %[tt], %[tt], %[m0]\n\t"
            "s_bcnt1_i32_b64 %[ta], %[tt]\n\t"
            "s_or_b64 %[tt], %[m0], %[m1]\n\t"
            "s_bcnt1_i32_b64 %[tb], %[tt]\n\t"
            "s_lshl_b32 %[ta], %[ta], 1\n\t"
            "s_cmp_ge_u32 %[ta], %[tb]\n\t"
            "s_cselect_b32 %[nxt], %[c0], %[c1]\n\t"
            "s_cselect_b32 %[far], %[c1], %[c0]\n\t"
            "s_cmp_lg_u64 %[m0], 0\n\t"
            "s_cselect_b64 %[tt], %[m1], 0\n\t"
            "s_cmp_lg_u64 %[tt], 0\n\t"
            "s_addc_u32 %[sp], %[sp], 0\n\t"
            "s_cmp_eq_u32 %[tb], 0\n\t"
            "s_cselect_b32 %[nxt], -1, %[nxt]"
            : [nxt] "=&s"(nxt), [far] "=&s"(far), [sp] "+s"(sp), [ta] "=&s"(ta), [tb] "=&s"(tb),
              [tt] "=&s"(tt)
            : [m0] "s"(m0), [m1] "s"(m1), [le] "s"(le), [c0] "s"(c0), [c1] "s"(c1)
            : "scc");
        *slot = far;
      }
      node = nxt;
    }
    if (node != kPopMarker) {
      // leaf: its triangles are fetched once per wave and tested by every lane
      const uint32_t first = leaf_first(node), count = leaf_count(node);
      {
        const uint64_t b = (uint64_t)P.tris;
        const uint64_t bs = ((uint64_t)uniform((uint32_t)(b >> 32)) << 32) | (uint32_t)uniform((uint32_t)b);
        leaf_prefetch(P, bs, first, 1, count, cpf0);
      }
      for (uint32_t k = 0; k < count; k++) {
        const TriRec64 tr = sload_tri(P.tris, first + k);
        test_tri<ANY, false, LATE>(P, tr, first + k, r, act, h, found, nullptr, ~0ull, false, occ);
      }
      if (ANY) {
        active = active & !found;
        act = ballot(active);
        if (!act) break;
        tlim = active ? INFINITY : -1.0f;
      }
    }
    if (sp == 0) break;
    sp--;
    node = uniform(lds_stack[sp]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(cpf0), "s"(cpf1) : "memory");  // the last prefetches landed
  if (!ANY && !active) h.t = INFINITY;
}

template <bool ANY, int OCT, bool LATE = false>
__device__ __forceinline__ void traverse_fast(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                              uint32_t* lds_stack, uint32_t* occ = nullptr) {
  if (P.n_nodes == 0) return;
  traverse_fast_from<ANY, OCT, LATE>(P, r, active, h, found, lds_stack, P.root, 0, occ);
}

// ------------------------------------------------------------------------------------------------
// fp32 4-wide packet traversal (Node128, the default PRIMARY tree). A node step fetches the 128-B record
// with two s_load_dwordx16 under one wait, slab-tests the four children per lane (exact fp32 boxes, no
// dequantisation), and -- the children being stored in this octant's near-to-far order -- writes every
// hit child to the wave stack farthest first with a conditional increment, takes the nearest hit child
// as the next node and drops it from the top again: no sort, no lane vote, 14 SALU. Same exact triangle
// tests and (t, rank) argmin as the binary loops, so every result is identical; only the visit order
// differs. Half the dependent node fetches of the binary tree per wave (SBVH soup: 52 vs 100 per wave).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ Node128 sload128(const void* base, uint32_t off) {
  const uint64_t b = (uint64_t)base;
  const uint64_t bs = ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(b >> 32)) << 32) |
                      (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)b);
  const uint32_t o = __builtin_amdgcn_readfirstlane(off);
  i16v lo, hi;
  asm volatile("s_load_dwordx16 %0, %2, %3\n\ts_load_dwordx16 %1, %2, %3 offset:0x40\n\ts_waitcnt lgkmcnt(0)"
               : "=&s"(lo), "=&s"(hi)
               : "s"(bs), "s"(o)
               : "memory");
  Node128 r;
  __builtin_memcpy(&r, &lo, 64);
  __builtin_memcpy(reinterpret_cast<char*>(&r) + 64, &hi, 64);
  return r;
}

// Reference form with the counting run's statistics (RT_FRAME_STATS): the same visit order as
// traverse_wide_fast. OCT < 0 (mixed-octant packets): the generic slab test, copy 0's child order.
template <bool ANY, bool STATS, int OCT>
__device__ __forceinline__ void traverse_wide(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                              uint32_t* lds_stack, uint64_t* lds_mask, uint32_t* cnt) {
  uint64_t act = ballot(active);
  float tlim = active ? INFINITY : -1.0f;
  if (!ANY && !active) h.t = -1.0f;
  bool want = active;
  int sp = 0;
  uint32_t node = P.wide_base + (uint32_t)(OCT < 0 ? 0 : OCT) * P.wide_copy_bytes;
  for (;;) {
    while (!is_leaf(node)) {
      const Node128 nd = sload128(P.nodes, node);
      if (STATS) {
        if (want) cnt[ST_NODE]++;
        cnt[ST_WWIDE]++;
      }
      const float tcut = ANY ? tlim : h.t;
      uint64_t m[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float* b = nd.box[c];
        const Span s = slab_o<OCT>(b[0], b[1], b[2], b[3], b[4], b[5], r, tcut);
        m[c] = mask_le(s.tmin, s.tmax);
      }
      uint32_t nxt = kPopMarker;
      uint64_t wm = 0;
#pragma unroll
      for (int c = 3; c >= 0; c--) {  // farthest first; the nearest hit ends on top and is taken next
        lds_stack[sp] = nd.child[c];
        if (STATS) lds_mask[sp] = m[c];
        if (m[c] != 0) {
          nxt = nd.child[c];
          wm = m[c];
          sp++;
        }
      }
      sp = (int)uniform((uint32_t)sp);
      if (nxt != kPopMarker) sp--;
      if (STATS) want = (wm >> lane_id()) & 1;
      node = uniform(nxt);
    }
    if (node != kPopMarker) {
      const uint32_t first = leaf_first(node), count = leaf_count(node);
      if (STATS) {
        if (want) cnt[ST_TRI] += count;
        cnt[ST_WTRI] += count;
      }
      for (uint32_t k = 0; k < count; k++) {
        const TriRec64 tr = sload_tri(P.tris, first + k);
        test_tri<ANY>(P, tr, first + k, r, act, h, found);
      }
      if (ANY) {
        active = active & !found;
        act = ballot(active);
        if (!act) break;
        tlim = active ? INFINITY : -1.0f;
      }
    }
    if (sp == 0) break;
    sp--;
    node = uniform(lds_stack[sp]);
    if (STATS) {
      want = (lds_mask[sp] >> lane_id()) & 1;
      cnt[ST_WPOP]++;
    }
  }
  if (!ANY && !active) h.t = INFINITY;
}

// The production form (octant loops, no counting): node fetch + the prefetch of the nearest child's
// record (both 64-B halves; the measured best of five prefetch forms, profiles/ab/r03_wide_tree_ab.txt),
// the four slab tests, and the decision as one SALU block interleaved with the four stack writes.
template <bool ANY, int OCT>
__device__ __forceinline__ void traverse_wide_fast(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                                   uint32_t* lds_stack) {
  uint64_t act = ballot(active);
  float tlim = active ? INFINITY : -1.0f;
  if (!ANY && !active) h.t = -1.0f;
  int sp = 0;
  const uint32_t vbase = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)lds_stack;
  const uint64_t bb = (uint64_t)P.nodes;
  const uint64_t bs = ((uint64_t)uniform((uint32_t)(bb >> 32)) << 32) | (uint32_t)uniform((uint32_t)bb);
  uint32_t sink = 0;  // the prefetches' destination (values unused): retired by the next node load's wait
  uint32_t node = uniform(P.wide_base + (uint32_t)OCT * P.wide_copy_bytes);
  Ray rr = r;
  // the node loop is rotated: the record load that follows a descent sits at the end of the loop body
  // and a separate copy serves the entry after a pop, so a wait the compiler needs after the leaf path
  // (its kernel-argument reloads) stays on that path instead of heading every node step
  auto load = [&](uint32_t off, i16v& lo, i16v& hi) {
    off = pf_off(off, P.all_bytes - 127u, P.pf_check, 5);
    asm volatile("s_load_dwordx16 %0, %3, %4\n\ts_load_dwordx16 %1, %3, %4 offset:0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(lo), "=&s"(hi), "+&s"(sink)
                 : "s"(bs), "s"(off)
                 : "memory");
  };
  for (;;) {
    if (!is_leaf(node)) {
      i16v lo, hi;
      load(node, lo, hi);
      for (;;) {
      Node128 nd;
      __builtin_memcpy(&nd, &lo, 64);
      __builtin_memcpy(reinterpret_cast<char*>(&nd) + 64, &hi, 64);
      // the ray's reciprocal direction passes through the prefetch asm ("+v", carried across steps: no
      // copies), so the slab tests that read it cannot be scheduled above the prefetches: those are issued
      // the moment the node has arrived
      asm volatile("s_load_dword %[k], %[b], %[p0]\n\ts_load_dword %[k], %[b], %[p0] offset:0x40"
                   : [k] "+&s"(sink), "+v"(rr.id.x), "+v"(rr.id.y), "+v"(rr.id.z)
                   : [b] "s"(bs), [p0] "s"(pf_off(uniform(nd.pf[0]), P.all_bytes - 64u, P.pf_check, 4))
                   : "memory");
      // the handles into VGPRs for the stack writes (off the masks' critical path)
      uint32_t v0 = nd.child[0], v1 = nd.child[1], v2 = nd.child[2], v3 = nd.child[3];
      asm("" : "+v"(v0), "+v"(v1), "+v"(v2), "+v"(v3));
      const float tcut = ANY ? tlim : h.t;
      uint64_t m[4];
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float* b = nd.box[c];
        const Span s = slab_o<OCT>(b[0], b[1], b[2], b[3], b[4], b[5], rr, tcut);
        m[c] = mask_le(s.tmin, s.tmax);
      }
      sp = (int)uniform((uint32_t)sp);
      uint32_t nxt, a0, a1, a2, a3;
      asm volatile(
          "v_lshl_add_u32 %[a3], %[sp], 2, %[vb]\n\t"
          "s_cmp_lg_u64 %[m3], 0\n\t"
          "s_cselect_b32 %[nxt], %[h3], -1\n\t"
          "s_addc_u32 %[sp], %[sp], 0\n\t"
          "ds_write_b32 %[a3], %[v3]\n\t"
          "v_lshl_add_u32 %[a2], %[sp], 2, %[vb]\n\t"
          "s_cmp_lg_u64 %[m2], 0\n\t"
          "s_cselect_b32 %[nxt], %[h2], %[nxt]\n\t"
          "s_addc_u32 %[sp], %[sp], 0\n\t"
          "ds_write_b32 %[a2], %[v2]\n\t"
          "v_lshl_add_u32 %[a1], %[sp], 2, %[vb]\n\t"
          "s_cmp_lg_u64 %[m1], 0\n\t"
          "s_cselect_b32 %[nxt], %[h1], %[nxt]\n\t"
          "s_addc_u32 %[sp], %[sp], 0\n\t"
          "ds_write_b32 %[a1], %[v1]\n\t"
          "v_lshl_add_u32 %[a0], %[sp], 2, %[vb]\n\t"
          "s_cmp_lg_u64 %[m0], 0\n\t"
          "s_cselect_b32 %[nxt], %[h0], %[nxt]\n\t"
          "s_addc_u32 %[sp], %[sp], 0\n\t"
          "ds_write_b32 %[a0], %[v0]\n\t"
          "s_cmp_lg_u32 %[nxt], -1\n\t"
          "s_subb_u32 %[sp], %[sp], 0"
          : [nxt] "=&s"(nxt), [sp] "+&s"(sp), [a0] "=&v"(a0), [a1] "=&v"(a1), [a2] "=&v"(a2), [a3] "=&v"(a3)
          : [m0] "s"(m[0]), [m1] "s"(m[1]), [m2] "s"(m[2]), [m3] "s"(m[3]), [h0] "s"(uniform(nd.child[0])),
            [h1] "s"(uniform(nd.child[1])), [h2] "s"(uniform(nd.child[2])), [h3] "s"(uniform(nd.child[3])),
            [v0] "v"(v0), [v1] "v"(v1), [v2] "v"(v2), [v3] "v"(v3), [vb] "v"(vbase)
          : "scc", "memory");
      node = nxt;
      if (is_leaf(node)) break;
      load(node, lo, hi);
      }
    }
    if (node != kPopMarker) {
      const uint32_t first = leaf_first(node), count = leaf_count(node);
      for (uint32_t k = 0; k < count; k++) {
        const TriRec64 tr = sload_tri(P.tris, first + k);
        test_tri<ANY>(P, tr, first + k, r, act, h, found);
      }
      if (ANY) {
        active = active & !found;
        act = ballot(active);
        if (!act) break;
        tlim = active ? INFINITY : -1.0f;
      }
    }
    if (sp == 0) break;
    sp--;
    node = uniform(lds_stack[sp]);
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::"s"(sink) : "memory");  // the last prefetches have landed
  if (!ANY && !active) h.t = INFINITY;
}

template <int TRAV, bool STATS>
struct WaveLds {
  // binary LDS-stack kernels also run the fp32 4-wide loops (traverse_wide*): kStackW entries
  static constexpr int kEntries = TRAV == TRAV_W4 ? kStack4 : (TRAV == TRAV_LANE ? 1 : (TRAV == TRAV_B2_LDS ? kStackW : 64));
  uint32_t stack[4][kEntries];
  uint64_t mask[4][(STATS && (TRAV == TRAV_W4 || TRAV == TRAV_B2_LDS)) ? kEntries : 1];
  uint32_t clk[4];  // one-wave kernels: the wave's start clocks (wave_clock_start), kept out of registers
};

// the A/B traversal flavours, defined in rt_variants.hip (instantiated only there)
template <bool ANY, bool STATS>
__device__ __forceinline__ void traverse4(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                          uint32_t* lds_stack, uint64_t* lds_mask, uint32_t* cnt);
template <bool ANY, bool STATS>
__device__ __forceinline__ void traverse_lane(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                              uint32_t* cnt);

template <bool ANY, bool STATS, int TRAV>
__device__ __forceinline__ void trace(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                      WaveLds<TRAV, STATS>& L, int wv, uint32_t* cnt, uint32_t* occ = nullptr) {
  if constexpr (TRAV == TRAV_W4) traverse4<ANY, STATS>(P, r, active, h, found, L.stack[wv], L.mask[STATS ? wv : 0], cnt);
  else if constexpr (TRAV == TRAV_LANE) traverse_lane<ANY, STATS>(P, r, active, h, found, cnt);
  else if constexpr (!STATS && TRAV == TRAV_B2_LDS) traverse_fast<ANY, -1>(P, r, active, h, found, L.stack[wv], occ);
  else traverse<ANY, STATS, TRAV == TRAV_B2_LDS>(P, r, active, h, found, L.stack[wv], cnt, occ);
}

// Packet traversal specialised by the wave's direction octant when every active ray shares it (coherent
// camera / reflection packets): loops compiled for that octant (known near / far planes, order bits);
// mixed-octant waves take the generic loop.
// WIDE: packets whose rays share an octant walk the fp32 4-wide tree when the scene has one
// (traverse_wide_fast; the counting run traverse_wide); mixed-octant packets keep the binary loop.
// SPLIT (FULL mode's secondary packets, small-scene build): a packet whose rays span several direction
// octants is walked once per octant present, each walk with that octant's lanes only (ballot masks) and
// the octant loop's cheaper slab test, instead of one generic walk of the union; a one-octant packet is
// the loop's single iteration. Each lane is traced by exactly one walk, so results are unchanged.
// LATE: the octant loops' accept_candidate form (the fused PRIMARY kernel).
template <bool ANY, bool STATS, int TRAV, bool WIDE = false, bool SPLIT = false, bool LATE = false>
__device__ __forceinline__ void trace_oct(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                          WaveLds<TRAV, STATS>& L, int wv, uint32_t* cnt) {
  if (SPLIT && !STATS && TRAV == TRAV_B2_LDS) {
    const uint32_t loct = (__float_as_uint(r.id.x) >> 31) | ((__float_as_uint(r.id.y) >> 31) << 1) |
                          ((__float_as_uint(r.id.z) >> 31) << 2);
    uint64_t rem = ballot(active);
    Hit hres = h;
    bool fres = found;
    while (rem != 0) {
      const uint32_t oct = uniform((uint32_t)__builtin_amdgcn_readlane((int)loct, (int)__builtin_ctzll(rem)));
      const uint64_t sub = ballot(loct == oct) & rem;
      rem &= ~sub;
      const bool a = lane_in(sub);
      Hit hs = h;
      bool fs = false;
      switch (oct) {
        case 0: traverse_fast<ANY, 0>(P, r, a, hs, fs, L.stack[wv]); break;
        case 1: traverse_fast<ANY, 1>(P, r, a, hs, fs, L.stack[wv]); break;
        case 2: traverse_fast<ANY, 2>(P, r, a, hs, fs, L.stack[wv]); break;
        case 3: traverse_fast<ANY, 3>(P, r, a, hs, fs, L.stack[wv]); break;
        case 4: traverse_fast<ANY, 4>(P, r, a, hs, fs, L.stack[wv]); break;
        case 5: traverse_fast<ANY, 5>(P, r, a, hs, fs, L.stack[wv]); break;
        case 6: traverse_fast<ANY, 6>(P, r, a, hs, fs, L.stack[wv]); break;
        default: traverse_fast<ANY, 7>(P, r, a, hs, fs, L.stack[wv]); break;
      }
      hres.t = a ? hs.t : hres.t;
      hres.rank = a ? hs.rank : hres.rank;
      hres.slot = a ? hs.slot : hres.slot;
      fres = fres | (a & fs);
    }
    h = hres;
    found = fres;
    return;
  }
  if (TRAV == TRAV_B2_LDS || TRAV == TRAV_B2_VGPR) {
    constexpr bool SL = TRAV == TRAV_B2_LDS;
    const uint64_t act = ballot(active);
    const uint64_t sx = ballot(__float_as_uint(r.id.x) >> 31) & act, sy = ballot(__float_as_uint(r.id.y) >> 31) & act,
                   sz = ballot(__float_as_uint(r.id.z) >> 31) & act;
    if ((sx == 0 || sx == act) && (sy == 0 || sy == act) && (sz == 0 || sz == act)) {
      const int oct = (sx ? 1 : 0) | (sy ? 2 : 0) | (sz ? 4 : 0);
      if (WIDE && SL && P.wide_copy_bytes != 0) {
        uint32_t* st = L.stack[wv];
        uint64_t* mk = L.mask[STATS ? wv : 0];
#define RT_WIDE_CASE(o)                                                              \
  case o:                                                                           \
    if (STATS) traverse_wide<ANY, STATS, o>(P, r, active, h, found, st, mk, cnt);   \
    else traverse_wide_fast<ANY, o>(P, r, active, h, found, st);                    \
    return;
        switch (oct) {
          RT_WIDE_CASE(0) RT_WIDE_CASE(1) RT_WIDE_CASE(2) RT_WIDE_CASE(3)
          RT_WIDE_CASE(4) RT_WIDE_CASE(5) RT_WIDE_CASE(6) default: RT_WIDE_CASE(7)
        }
#undef RT_WIDE_CASE
      }
      if (!STATS && SL) {
        switch (oct) {
          case 0: traverse_fast<ANY, 0, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 1: traverse_fast<ANY, 1, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 2: traverse_fast<ANY, 2, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 3: traverse_fast<ANY, 3, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 4: traverse_fast<ANY, 4, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 5: traverse_fast<ANY, 5, LATE>(P, r, active, h, found, L.stack[wv]); return;
          case 6: traverse_fast<ANY, 6, LATE>(P, r, active, h, found, L.stack[wv]); return;
          default: traverse_fast<ANY, 7, LATE>(P, r, active, h, found, L.stack[wv]); return;
        }
      }
      switch (oct) {
        case 0: traverse<ANY, STATS, SL, 0>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 1: traverse<ANY, STATS, SL, 1>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 2: traverse<ANY, STATS, SL, 2>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 3: traverse<ANY, STATS, SL, 3>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 4: traverse<ANY, STATS, SL, 4>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 5: traverse<ANY, STATS, SL, 5>(P, r, active, h, found, L.stack[wv], cnt); return;
        case 6: traverse<ANY, STATS, SL, 6>(P, r, active, h, found, L.stack[wv], cnt); return;
        default: traverse<ANY, STATS, SL, 7>(P, r, active, h, found, L.stack[wv], cnt); return;
      }
    }
  }
  trace<ANY, STATS, TRAV>(P, r, active, h, found, L, wv, cnt);
}
template <bool STATS, int TRAV, bool WIDE = false, bool LATE = false>
__device__ __forceinline__ void trace_closest_oct(const DevScene& P, const Ray& r, bool active, Hit& h,
                                                  WaveLds<TRAV, STATS>& L, int wv, uint32_t* cnt) {
  bool found = false;
  trace_oct<false, STATS, TRAV, WIDE, false, LATE>(P, r, active, h, found, L, wv, cnt);
}
// incoherent FULL-mode packets (the generic loop)
template <bool ANY, bool STATS, int TRAV>
__device__ __forceinline__ void trace_full_ray(const DevScene& P, const Ray& r, bool active, Hit& h, bool& found,
                                               WaveLds<TRAV, STATS>& L, int wv, uint32_t* cnt, uint32_t* occ = nullptr) {
  trace<ANY, STATS, TRAV>(P, r, active, h, found, L, wv, cnt, occ);
}

}  // namespace rt
