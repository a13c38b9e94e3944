// rt_frame_kernels.h -- the frame kernels of rt_render: PRIMARY in two stages (k_trace_primary, k_shade_primary) and
// as one kernel (k_primary_fused, the default), and the FULL megakernel (k_render_full). With k_render_depth
// (rt_trace_ray.h, beside its twin trace_depth) these are instantiated in rt_frame.hip and nowhere else among the
// product objects; the variants library instantiates k_trace_primary and k_render_full with other traversal
// flavours in rt_variants.hip.
#pragma once
#include "rt_trace_ray.h"

namespace rt {

// PRIMARY stage 1: closest hit per pixel (calculateMinimumFace, flyscene.cpp:373-396) -> 8-B hit record.
// Only traversal state is live here, so the kernel fits 8 waves per SIMD.
template <bool STATS, int TRAV>
__global__ __launch_bounds__(64 * kTraceWPB) __attribute__((amdgpu_waves_per_eu(kTraceWavesPerEu)))
void k_trace_primary(FrameParams P) {
  __shared__ WaveLds<TRAV, STATS> lds;
  const PixelCoord c = pixel_coord<kTraceWPB>(P);
  uint32_t cnt[ST_COUNT] = {};
  const Ray r = primary_ray(P, c.px, c.py);
  if (STATS && c.active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }
  Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  trace_closest_oct<STATS, TRAV, true>(P.sc, r, c.active, h, lds, c.slot, cnt);
  if (STATS && c.active && h.t != INFINITY) cnt[ST_HITS]++;
  if (c.active) P.hits[(size_t)c.py * P.W + c.px] = make_uint2(__float_as_uint(h.t), h.slot);
  if (P.wcount0 != nullptr) {  // FULL pipeline: per-wave hit count for the list0 compaction
    const uint32_t nh = (uint32_t)__popcll(ballot(c.active && h.t != INFINITY));
    if (c.lane == 0) P.wcount0[c.qw] = nh;
  }
  if (STATS) {
    if (P.wave_stats) {  // the wave's hit lanes (ST_HITS counts per lane)
      uint32_t w[ST_COUNT];
      for (int k = 0; k < ST_COUNT; k++) w[k] = cnt[k];
      w[ST_HITS] = (uint32_t)__popcll(ballot(c.active && h.t != INFINITY));
      wave_stats_out(P, w, c.lane, c.qw, false);
    }
    flush_stats(P, cnt, c.lane);
  }
}

// PRIMARY stage 2: shade_primary_pixel (rt_trace_ray.h) for every pixel of the stage-1 hit records
template <bool HITS, bool BOXCOL>
__global__ __launch_bounds__(256) void k_shade_primary(FrameParams P) {
  const PixelCoord c = pixel_coord(P);
  if (!c.active) return;
  const size_t pix = (size_t)c.py * P.W + c.px;
  const uint2 hb = P.hits[pix];
  const float t = __uint_as_float(hb.x);
  Ray r;
  if (t != INFINITY) r = primary_ray(P, c.px, c.py);
  shade_primary_pixel<HITS, BOXCOL>(P, r, pix, t, hb.y);
}


// PRIMARY as one kernel (default; variant VB_SPLIT_PRIMARY selects the two-kernel form k_trace_primary +
// k_shade_primary): the traversal, then the shading of the same lane -- the hit record stays in
// registers instead of a round trip through HBM, and the traversal state is dead by then, so the
// shading's registers do not add to the traversal's. Measured: C3 +2.7% at 4 frames in flight, bunny +4%.
// WIDE: the instantiation for scenes built with the fp32 4-wide tree (eight traverse_wide_fast copies beside
// the binary loops); it is the kernel as it was. A frame without a wide tree -- the default scene, or
// VB_PRIMARY_BINARY_TREE -- runs the binary-only instantiation (launch_frame chooses by the frame's
// DevScene::wide_copy_bytes), which drops the wide copies and takes accept_candidate's LATE form. Resources
// (make asm -> build/asm/rt_frame.resource.txt), both 8 waves/SIMD without scratch: binary-only 60 VGPR, 78 SGPR, 26
// SGPR spill lanes, 51,756 B of code; wide 60 VGPR, 78 SGPR, 20 spill lanes, 93,868 B.
template <bool HITS, bool BOXCOL = false, bool WIDE = true>
__global__ __launch_bounds__(64 * kTraceWPB) __attribute__((amdgpu_waves_per_eu(kTraceWavesPerEu)))
void k_primary_fused(FrameParams P) {
  __shared__ WaveLds<TRAV_B2_LDS, false> lds;
  __shared__ float tprim[64];  // the lanes' primary hit distances (wave_clock_end's prediction)
  wave_clock_start(P, lds.clk);
  const PixelCoord c = pixel_coord<kTraceWPB>(P);
  // the eye (every primary ray's origin) held in VGPRs: origin.dot(facenormal) in each triangle test
  // then reads one SGPR per op and needs no moves
  Ray r = primary_ray(P, c.px, c.py);
  asm("" : "+v"(r.o.x), "+v"(r.o.y), "+v"(r.o.z));
  Hit h{INFINITY, 0xFFFFFFFFu, 0xFFFFFFFFu};
  trace_closest_oct<false, TRAV_B2_LDS, WIDE, !WIDE>(P.sc, r, c.active, h, lds, c.slot, nullptr);
  tprim[c.lane] = h.t;  // (INFINITY for a miss or an inactive lane)
  if (c.active) shade_primary_pixel<HITS, BOXCOL>(P, r, (size_t)c.py * P.W + c.px, h.t, h.slot);
  wave_clock_end(P, lds.clk, c.lane, c.qw, c.sub >= 0, tprim);
}

// FULL: the reference traceRay as-is (max_depth 2) for a frame, all in one kernel: trace_full (rt_trace_ray.h, with
// the occupancy bounds kFullWavesPerEu / kFullWavesPerEuSmall and kFullWPB) under the frame's pixel addressing.
template <bool STATS, bool HITS, int TRAV, int WPE = kFullWavesPerEu>
__global__ __launch_bounds__(64 * kFullWPB) __attribute__((amdgpu_waves_per_eu(WPE)))
void k_render_full(FrameParams P) {
  static_assert(kFullWPB == 1, "the pixel words below are per one-wave block");
  __shared__ WaveLds<TRAV, STATS> lds;
  // the lane's pixel (x, y; x = ~0 when inactive), parked in LDS across the traversal and re-read by a
  // freshly computed lane id at the end: held in registers, the thread id and the pixel coordinates were
  // spilled to scratch (16 B per lane written at every pixel: ~33 MB of HBM writes per 1080p frame
  // against the 24.9 MB frame itself)
  __shared__ uint32_t pix_xy[2][64];
  __shared__ float tprim[64];  // the lanes' primary hit distances (wave_clock_end's prediction)
  wave_clock_start(P, lds.clk);
  const PixelCoord c = pixel_coord<kFullWPB>(P);
  const bool active = c.active;
  pix_xy[0][c.lane] = active ? (uint32_t)c.px : 0xFFFFFFFFu;
  pix_xy[1][c.lane] = (uint32_t)c.py;
  uint32_t cnt[ST_COUNT] = {};
  const Ray r = primary_ray(P, c.px, c.py);
  if (STATS && active) { cnt[ST_RAYS]++; cnt[ST_TOTAL]++; }

  Hit h;
  uint32_t face0;
  const f3 col = trace_full<STATS, TRAV, WPE == kFullWavesPerEuSmall>(P, r, active, lds, c.slot, cnt, h, face0, tprim);
  const bool hit0 = face0 != 0xFFFFFFFFu;
  const uint32_t lane = lane_id_fresh();
  const uint32_t px = reinterpret_cast<volatile uint32_t*>(pix_xy[0])[lane];
  const uint32_t py = reinterpret_cast<volatile uint32_t*>(pix_xy[1])[lane];
  if (px != 0xFFFFFFFFu) {
    const size_t pix = (size_t)py * P.W + px;
    P.rgb[3 * pix + 0] = col.x;
    P.rgb[3 * pix + 1] = col.y;
    P.rgb[3 * pix + 2] = col.z;
    if (HITS) {
      P.face_out[pix] = hit0 ? (int32_t)face0 : -1;
      P.t_out[pix] = h.t;
    }
  }
  if (STATS) {
    wave_stats_out(P, cnt, (int)lane, c.qw, true);
    flush_stats(P, cnt, (int)lane);
  }
  wave_clock_end(P, lds.clk, (int)lane, c.qw, c.sub >= 0, tprim);
}

}  // namespace rt
