// rt_view_kernels.h -- the view-batch kernels of rt_render_views / rt_render_views_ss: k_views_primary,
// k_views_depth, k_views_ss_loop and k_views_ss_packed. Instantiated in rt_views.hip and nowhere else.
#pragma once
#include "rt_trace_ray.h"

namespace rt {

// ------------------------------------------------------------------------------------------------
// View batches (rt_views.hip rt_render_views): n cameras of one scene in one launch of one-wave blocks, in plain
// order -- no cost map, no wave split, no timeline. Block b renders view b / units_per_view; within the view its
// logical wave b % units_per_view is tile * 4 + quarter in the frame kernels' layout (pixel_coord<1> at its
// defaults: tiles row-major, quarters 2 x 2 waves of 8 x 8 pixels). FrameParams carries the scene, the lights, the
// frame shape and the bases of the batch's output arrays; the camera is the view's record.
// ------------------------------------------------------------------------------------------------
struct ViewCoord {
  uint32_t view;
  int px, py, lane;
  bool active;
};
__device__ __forceinline__ ViewCoord view_coord(const FrameParams& P, const ViewParams& V) {
  ViewCoord c;
  c.lane = threadIdx.x & 63;
  c.view = uniform(blockIdx.x / V.units_per_view);
  const uint32_t w = uniform(blockIdx.x - c.view * V.units_per_view);
  const int tile = (int)(w >> 2), wv = (int)(w & 3u);
  const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
  c.px = tx * 16 + (wv & 1) * 8 + (c.lane & 7);
  c.py = ty * 16 + (wv >> 1) * 8 + (c.lane >> 3);
  c.active = c.px < P.W && c.py < P.H;
  return c;
}

// View `view`'s camera record, read through the constant address space: base and view are wave-uniform, so these are
// scalar loads (one fetch per wave into SGPRs, as the frame kernels read the camera from their kernel arguments)
__device__ __forceinline__ ViewCam load_view_cam(const ViewParams& V, uint32_t view) {
  typedef const __attribute__((address_space(4))) ViewCam* CCam;
  const uint64_t b = (uint64_t)V.cams;
  const uint64_t bs = ((uint64_t)uniform((uint32_t)(b >> 32)) << 32) | (uint32_t)uniform((uint32_t)b);
  const CCam q = (CCam)bs + view;
  ViewCam c;
  for (int k = 0; k < 16; k++) c.vinv[k] = q->vinv[k];
  for (int k = 0; k < 3; k++) {
    c.eye[k] = q->eye[k];
    c.eye_obj[k] = q->eye_obj[k];
  }
  for (int k = 0; k < 4; k++) c.vp[k] = q->vp[k];
  c.xscale = q->xscale;
  c.yscale = q->yscale;
  return c;
}

// primary_ray(P, px, py) with the camera taken from a view's record instead of P: the same expressions in the same
// order, hence the same ray
__device__ __forceinline__ Ray primary_ray(const DevScene& S, const ViewCam& C, int px, int py) {
  Ray r;
  const float nx = (float)(2.0 * (double)((float)px - C.vp[0]) / (double)C.vp[2] - 1.0);
  const float ny = (float)(1.0 - 2.0 * (double)((float)py - C.vp[1]) / (double)C.vp[3]);
  const f3 w = affv3(C.vinv, f3{nx * C.xscale, ny * C.yscale, -1.0f});
  r.o = f3{C.eye[0], C.eye[1], C.eye[2]};
  r.d = normalized(sub(w, r.o));
  r.o2 = f3{C.eye_obj[0], C.eye_obj[1], C.eye_obj[2]};
  setup_cull(r, S.static_pad);
  return r;
}

// the pixel's index in the batch's output arrays ([n_views][H][W]); size_t throughout
__device__ __forceinline__ size_t view_pixel(const FrameParams& P, const ViewCoord& c) {
  return ((size_t)c.view * (size_t)P.H + (size_t)c.py) * (size_t)P.W + (size_t)c.px;
}

// PRIMARY at depth 1: k_primary_fused's body -- the closest hit on the tree rt_render walks (the fp32 4-wide tree
// when the scene has one), then shade_primary_pixel -- without the wave clock and the prediction words.
// HITS: the batch has a face or a t array (either may be null); the colour never depends on it.
template <bool HITS>
__global__ __launch_bounds__(64 * kTraceWPB) __attribute__((amdgpu_waves_per_eu(kTraceWavesPerEu)))
void k_views_primary(FrameParams P, ViewParams V) {
  __shared__ WaveLds<TRAV_B2_LDS, false> lds;
  const ViewCoord c = view_coord(P, V);
  const ViewCam cam = load_view_cam(V, c.view);
  Ray r = primary_ray(P.sc, cam, c.px, c.py);
  asm("" : "+v"(r.o.x), "+v"(r.o.y), "+v"(r.o.z));  // the eye in VGPRs, as in k_primary_fused
  Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  trace_closest_oct<false, TRAV_B2_LDS, true>(P.sc, r, c.active, h, lds, 0, nullptr);
  if (!c.active) return;
  const size_t pix = view_pixel(P, c);
  if (HITS) {  // shade_primary_pixel<true>'s face and t, each behind its own pointer; written first, so that neither
               // pointer stays live through the shading
    if (P.face_out) {
      // (the record's face word alone, as a plain word load: read as a member, the load merged with vload_tri's
      // in the shading and left part of that record in scratch)
      int32_t face = -1;
      if (h.t != INFINITY) face = (int32_t)reinterpret_cast<const uint32_t*>(P.sc.tris + h.slot)[offsetof(TriRec64, face) / 4];
      P.face_out[pix] = face;
    }
    if (P.t_out) P.t_out[pix] = h.t;
  }
  shade_primary_pixel<false>(P, r, pix, h.t, h.slot);
}

// Everything else -- PRIMARY at depth >= 2, FULL at every depth, every batch lit from device memory: k_render_depth's
// level loop (trace_depth, its statement-for-statement copy) under the view's camera. LSRC as in k_render_depth.
template <bool HITS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEuSmall)))
void k_views_depth(FrameParams P, ViewParams V) {
  __shared__ WaveLds<TRAV_B2_LDS, false> lds;
  const ViewCoord c = view_coord(P, V);
  const ViewCam cam = load_view_cam(V, c.view);
  const Ray r = primary_ray(P.sc, cam, c.px, c.py);
  Hit h;
  uint32_t face0;
  const f3 col = trace_depth<false, LSRC>(P, r, c.active, lds, 0, nullptr, h, face0);
  if (!c.active) return;
  const size_t pix = view_pixel(P, c);
  P.rgb[3 * pix + 0] = col.x;
  P.rgb[3 * pix + 1] = col.y;
  P.rgb[3 * pix + 2] = col.z;
  if (HITS) {
    if (P.face_out) P.face_out[pix] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
    if (P.t_out) P.t_out[pix] = h.t;
  }
}

// ------------------------------------------------------------------------------------------------
// Supersampled view batches (rt_views.hip rt_render_views_ss): S rays per pixel, averaged in the launch. Sample k of
// a pixel is the view's camera with viewport[0..1] - offset k (float subtractions), traced by trace_depth exactly as
// k_views_depth traces the unshifted one; the pixel is ((c_0 + c_1) + ... + c_{S-1}) / (float)S per channel, float
// additions in that order and one correctly rounded division. face and t are sample 0's. Two layouts (rt_dispatch.h
// SampleLayout), both bit-equal to S rt_render frames summed in order.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ ViewCam sample_cam(const ViewCam& cam, float ox, float oy) {
  ViewCam c = cam;
  c.vp[0] = cam.vp[0] - ox;
  c.vp[1] = cam.vp[1] - oy;
  return c;
}

// Loop layout: k_views_depth's blocks; the sample index is wave-uniform, so the offsets are scalar loads.
template <bool HITS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEuSmall)))
void k_views_ss_loop(FrameParams P, ViewParams V, SampleParams SP) {
  __shared__ WaveLds<TRAV_B2_LDS, false> lds;
  typedef const __attribute__((address_space(4))) float* CFloat;
  const ViewCoord c = view_coord(P, V);
  const ViewCam cam = load_view_cam(V, c.view);
  const uint64_t ob = (uint64_t)SP.offsets;
  const CFloat offs = (CFloat)(((uint64_t)uniform((uint32_t)(ob >> 32)) << 32) | (uint32_t)uniform((uint32_t)ob));
  const int S = (int)uniform((uint32_t)SP.n_samples);
  f3 acc{0.0f, 0.0f, 0.0f};
  Hit h0{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  uint32_t face0 = 0xFFFFFFFFu;
#pragma clang loop unroll(disable)
  for (int k = 0; k < S; k++) {
    const ViewCam ck = sample_cam(cam, offs[2 * k], offs[2 * k + 1]);
    const Ray r = primary_ray(P.sc, ck, c.px, c.py);
    Hit h;
    uint32_t face;
    const f3 col = trace_depth<false, LSRC>(P, r, c.active, lds, 0, nullptr, h, face);
    if (k == 0) {
      acc = col;
      h0 = h;
      face0 = face;
    } else {
      acc = f3{acc.x + col.x, acc.y + col.y, acc.z + col.z};
    }
  }
  if (!c.active) return;
  const float fs = (float)S;
  const size_t pix = view_pixel(P, c);
  P.rgb[3 * pix + 0] = acc.x / fs;
  P.rgb[3 * pix + 1] = acc.y / fs;
  P.rgb[3 * pix + 2] = acc.z / fs;
  if (HITS) {
    if (P.face_out) P.face_out[pix] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
    if (P.t_out) P.t_out[pix] = h0.t;
  }
}

// Packed layout (S = 2^SP.lg_samples, 2..64): block b of a view is tile b / (4 S), pixel block b % (4 S) of it,
// row-major over the tile's (16 >> lg_block_w) x (16 >> lg_block_h) blocks of (1 << lg_block_w) x (1 << lg_block_h)
// pixels; lane = pixel_in_block * S + k, pixels row-major within the block. Every lane traces one sample, with its
// offset read per lane (a vector load). The S colours of a pixel are then summed by every lane of the pixel's group
// as the chain c_0 + c_1 + ... + c_{S-1}, each term read from its lane (ds_bpermute) in that order -- never a
// butterfly -- and lane k = 0 writes. Lanes of pixels outside the frame trace nothing and write nothing, but stay in
// the wave to the end: the cross-lane reads need every lane executing.
template <bool HITS, int LSRC = LS_KERNARG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(kFullWavesPerEuSmall)))
void k_views_ss_packed(FrameParams P, ViewParams V, SampleParams SP) {
  __shared__ WaveLds<TRAV_B2_LDS, false> lds;
  const int lane = threadIdx.x & 63;
  const uint32_t view = uniform(blockIdx.x / V.units_per_view);
  const uint32_t w = uniform(blockIdx.x - view * V.units_per_view);
  const int lgS = (int)uniform((uint32_t)SP.lg_samples), lgW = (int)uniform((uint32_t)SP.lg_block_w),
            lgH = (int)uniform((uint32_t)SP.lg_block_h);
  const int tile = (int)(w >> (2 + lgS)), sub = (int)(w & ((4u << lgS) - 1u));
  const int tx = tile % P.tiles_x, ty = tile / P.tiles_x;
  const int bx = sub & ((16 >> lgW) - 1), by = sub >> (4 - lgW);
  const int pib = lane >> lgS, k = lane & ((1 << lgS) - 1);
  ViewCoord c;
  c.view = view;
  c.lane = lane;
  c.px = tx * 16 + (bx << lgW) + (pib & ((1 << lgW) - 1));
  c.py = ty * 16 + (by << lgH) + (pib >> lgW);
  c.active = c.px < P.W && c.py < P.H;
  const ViewCam cam = load_view_cam(V, view);
  const ViewCam ck = sample_cam(cam, SP.offsets[2 * k], SP.offsets[2 * k + 1]);
  const Ray r = primary_ray(P.sc, ck, c.px, c.py);
  Hit h;
  uint32_t face0;
  const f3 col = trace_depth<false, LSRC>(P, r, c.active, lds, 0, nullptr, h, face0);
  const int first = lane - k;  // the pixel's sample 0
  f3 acc{__shfl(col.x, first), __shfl(col.y, first), __shfl(col.z, first)};
  const int S = 1 << lgS;
#pragma clang loop unroll(disable)
  for (int j = 1; j < S; j++)
    acc = f3{acc.x + __shfl(col.x, first + j), acc.y + __shfl(col.y, first + j), acc.z + __shfl(col.z, first + j)};
  if (!c.active || k != 0) return;
  const float fs = (float)S;
  const size_t pix = view_pixel(P, c);
  P.rgb[3 * pix + 0] = acc.x / fs;
  P.rgb[3 * pix + 1] = acc.y / fs;
  P.rgb[3 * pix + 2] = acc.z / fs;
  if (HITS) {
    if (P.face_out) P.face_out[pix] = face0 != 0xFFFFFFFFu ? (int32_t)face0 : -1;
    if (P.t_out) P.t_out[pix] = h.t;
  }
}

}  // namespace rt
