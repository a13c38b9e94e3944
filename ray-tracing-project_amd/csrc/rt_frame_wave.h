// rt_frame_wave.h -- what one wave of a frame kernel does around its traversal: its pixel (pixel_coord), its primary
// ray, the wave clocks of the cost map and the timeline, and the counting run's output (flush_stats, which the
// ray-list kernels use too). No kernel is defined here.
// Frame kernels: one block = one 16x16 pixel tile (2x2 waves of 8x8, one ray per lane).
// XCD-aware order: blocks b and b+8 share an XCD under round-robin dispatch, so each XCD gets a
// contiguous run of tiles (L2 reuse; speed only, any placement is correct).
#pragma once
#include "rt_traverse.h"

namespace rt {

struct PixelCoord {
  int px, py, wv, lane;
  int slot;   // this wave's LDS slot within its block
  int qw;     // global wave number (tile-block * 4 + wave): the same for every block shape
  int sub;    // FrameParams::split_k: this block's 16-lane part (rows 2 sub, 2 sub + 1) of its wave, else -1
  bool active;
};

// WPB = waves per block: 4 (one 256-thread block per 16x16 tile) or 1 (one 64-thread block per 8x8
// quarter, blocks 4t..4t+3 cover tile t; finer-grained dispatch, same pixels and shard assignment)
template <int WPB = 4>
__device__ __forceinline__ PixelCoord pixel_coord(const FrameParams& P) {
  PixelCoord c;
  c.lane = threadIdx.x & 63;
  int nb, b;
  int bid = (int)blockIdx.x;
  c.sub = -1;
  if (WPB == 1 && P.order != nullptr) {
    // longest-first order from an earlier frame's wave costs (k_order_lpt): a permutation of the
    // logical waves that keeps each XCD on its own chunked bands; an out-of-range entry (never
    // produced) falls back to the block's own position, so a wave never leaves the grid.
    // split_k > 0: order positions 0 .. split_k - 1 (the costliest waves) are traced by four blocks
    // each, every one with 16 of the wave's lanes, so the frame's slowest packets shrink to 16 rays
    const uint32_t k = (uint32_t)P.split_k, nlog = gridDim.x - 3u * k;
    uint32_t pos = blockIdx.x;
    if (k > 0) {
      if (pos < 4u * k) {
        c.sub = (int)(pos & 3u);
        pos >>= 2;
      } else {
        pos -= 3u * k;
      }
    }
    const uint32_t o = uniform(P.order[pos]);
    bid = o < nlog ? (int)o : (int)pos;
  } else if (P.xcd_remap >= 2) {
    // chunked XCD order: blocks b and b + 8 share an XCD, so the k-th block of XCD x takes position
    // (k / C) * 8C + x C + k % C -- each XCD receives runs of C consecutive blocks (for one-wave
    // blocks, the four quarters of a tile and its row neighbours) while the runs still interleave
    // over the frame (load balance). The trailing partial group keeps the identity order.
    const int C = P.xcd_remap, G = 8 * C, full = ((int)gridDim.x / G) * G;
    if (bid < full) {
      const int x = ((bid & 7) + P.xcd_rot) & 7, k = bid >> 3;
      bid = (k / C) * G + x * C + (k % C);
    }
  }
  if (WPB == 4) {
    c.wv = (int)uniform(threadIdx.x >> 6);
    c.slot = c.wv;
    nb = (int)gridDim.x;
    b = bid;
  } else {
    c.wv = bid & 3;
    c.slot = 0;
    nb = (int)((gridDim.x - 3u * (uint32_t)P.split_k) >> 2);
    b = bid >> 2;
  }
  c.qw = b * 4 + c.wv;
  int L = b;
  if (P.xcd_remap == 1) {
    const int q = nb >> 3, rr = nb & 7, x = b & 7, k = b >> 3;
    L = x < rr ? x * (q + 1) + k : rr * (q + 1) + (x - rr) * q + k;
  }
  int tx, ty;
  shard_tile_xy(P.tiles_x, P.super_tile, P.shard_index, P.shard_count, L, tx, ty);
  c.px = tx * 16 + (c.wv & 1) * 8 + (c.lane & 7);
  c.py = ty * 16 + (c.wv >> 1) * 8 + (c.lane >> 3);
  c.active = c.px < P.W && c.py < P.H && (c.sub < 0 || (c.lane >> 4) == c.sub);
  return c;
}

// traceRayThread: o = getCenter(), d = normalize(screenToWorld(i, j) - o)   (flyscene.cpp:301-308;
// Camera::screenToWorld camera.hpp:155-173 with its fp64 NDC)
__device__ __forceinline__ Ray primary_ray(const FrameParams& P, int px, int py) {
  Ray r;
  const float nx = (float)(2.0 * (double)((float)px - P.vp[0]) / (double)P.vp[2] - 1.0);
  const float ny = (float)(1.0 - 2.0 * (double)((float)py - P.vp[1]) / (double)P.vp[3]);
  const f3 w = affv3(P.vinv, f3{nx * P.xscale, ny * P.yscale, -1.0f});
  r.o = f3{P.eye[0], P.eye[1], P.eye[2]};
  r.d = normalized(sub(w, r.o));
  r.o2 = f3{P.eye_obj[0], P.eye_obj[1], P.eye_obj[2]};
  setup_cull(r, P.sc.static_pad);
  return r;
}

// RT_FRAME_TIMELINE: the wave's start / end clocks and where it ran (diagnostics; one uniform branch
// when off). HW_ID / XCC_ID via s_getreg (hwreg ids 4 and 20, all 32 bits).
// The start clocks go to the wave's LDS words rather than staying live in registers for the whole
// kernel (the FULL megakernel's allocation tips into heavy spilling otherwise).
// A kernel argument read at this point of the kernel: the offset passes through an empty asm, so the load
// cannot be hoisted to the kernel's start and its value is not held in registers before it is needed
template <typename T>
__device__ __forceinline__ T late_kernarg(size_t off) {
  uint32_t o = (uint32_t)off;
  asm volatile("" : "+s"(o));
  typedef const __attribute__((address_space(4))) char* KArg;
  const KArg base = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
  return *reinterpret_cast<const __attribute__((address_space(4))) T*>(base + o);
}

__device__ __forceinline__ void wave_clock_start(const FrameParams& P, uint32_t* clk) {
  if (P.timeline || P.cost) {
    const uint64_t t0 = __builtin_amdgcn_s_memtime();
    const uint32_t r0 = (uint32_t)__builtin_amdgcn_s_memrealtime();
    if ((threadIdx.x & 63) == 0) {
      clk[0] = (uint32_t)t0;
      clk[1] = (uint32_t)(t0 >> 32);
      clk[2] = r0;
    }
  }
}
// tprim (PRIMARY / FULL frame kernels): each lane's primary hit distance (INFINITY: missed or inactive), stored to
// LDS right after the primary hit -- one ds_write per lane, no branch, nothing held in registers -- for a moving
// camera's prediction below (FrameParams::pred)
__device__ __forceinline__ void wave_clock_end(const FrameParams& P, const uint32_t* clk, int lane, int qw,
                                               bool sub_wave = false, const float* tprim = nullptr) {
  if (!P.timeline && !P.cost) return;
  const uint64_t t1 = __builtin_amdgcn_s_memtime();
  struct { uint64_t t0; uint32_t r0; } w;
  w.t0 = (uint64_t)uniform(clk[0]) | ((uint64_t)uniform(clk[1]) << 32);
  w.r0 = uniform(clk[2]);
  // this wave's cost for the next frame's dispatch order. The four 16-lane sub-waves of a split wave
  // (sub_wave) write the maximum of their times into the wave's slot, which the host cleared before such
  // a frame: a split wave's cost is re-measured like every other wave's, so one whose
  // work has become cheap leaves the split range (profiles/ab/r03_subwave_cost_ab.txt: the sum ranks the
  // split waves far above the rest and coarsens the order's buckets, -20% on C5 lone frames; keeping the
  // stale cost is within 1% of the maximum but never refreshes it; running cost-recording frames unsplit
  // costs 6%)
  if (P.cost && lane == 0) {
    const uint64_t dt = t1 - w.t0;
    const uint32_t c = dt > 0x3FFFFFFFull ? 0x3FFFFFFFu : (uint32_t)dt;
    if (!sub_wave) P.cost[qw] = c;
    else atomicMax(P.cost + qw, c);
  }
  // a moving camera: lane i raises the map at the i-th wave around the wave's footprint (whole frames: tile qw / 4
  // sits at (tile % tiles_x, tile / tiles_x), its quarters 2 x 2 waves). The fields are read here, from the
  // kernel arguments (late_kernarg), so nothing of this stays live through the traversal: read through P, the
  // compiler loaded them at the kernel's start and held them in SGPRs, spilling more of the kernel's SGPRs to
  // VGPR lanes (C2 with frames in flight -4..-8%, round 6)
  uint32_t* const dil = late_kernarg<uint32_t*>(offsetof(FrameParams, cost_dil));
  if (dil) {
    const uint64_t dt = t1 - w.t0;
    const uint32_t c = dt > 0x3FFFFFFFull ? 0x3FFFFFFFu : (uint32_t)dt;
    const int r = late_kernarg<int32_t>(offsetof(FrameParams, dil_r));
    const int tx = late_kernarg<int32_t>(offsetof(FrameParams, tiles_x)), ty = late_kernarg<int32_t>(offsetof(FrameParams, tiles_y));
    const int t = qw >> 2, q = qw & 3;
    // the wave's pixel origin: its own, or where a moving camera's prediction (FrameParams::pred) expects its
    // content in the next frame -- one hit lane's primary hit (lane 36, the wave's centre, when it hit, else the
    // first hit lane): t along its view-space direction (a px + b, c py + e, -1) (the camera is rigid, so t is a
    // view-space distance), moved by the camera's last step (pred_step: a translation in view space, as the
    // reference's WASD keys make it) and projected back to a pixel; its own when no lane hit
    float ox = (float)(((t % tx) * 2 + (q & 1)) * 8), oy = (float)(((t / tx) * 2 + (q >> 1)) * 8);
    const uint64_t hb = (tprim && late_kernarg<int32_t>(offsetof(FrameParams, pred)))
                            ? ballot(reinterpret_cast<const volatile float*>(tprim)[lane] != INFINITY) : 0;
    if (hb != 0) {
      const int rep = ((hb >> 36) & 1) ? 36 : (int)__builtin_ctzll(hb);
      const float th = reinterpret_cast<const volatile float*>(tprim)[rep];
      const size_t po = offsetof(FrameParams, pred_proj), so = offsetof(FrameParams, pred_step);
      const float a = late_kernarg<float>(po), b = late_kernarg<float>(po + 4), cc = late_kernarg<float>(po + 8),
                  e = late_kernarg<float>(po + 12);
      const float dx = a * (ox + (float)(rep & 7)) + b, dy = cc * (oy + (float)(rep >> 3)) + e;
      const float k = th / sqrtf(dx * dx + dy * dy + 1.0f);
      const float qx = dx * k + late_kernarg<float>(so), qy = dy * k + late_kernarg<float>(so + 4),
                  qz = late_kernarg<float>(so + 8) - k;
      if (qz < 0.0f) {
        const float sx = (qx / -qz - b) / a - (float)(rep & 7), sy = (qy / -qz - e) / cc - (float)(rep >> 3);
        if (sx > -8.0f && sy > -8.0f && sx < 16.0f * (float)tx && sy < 16.0f * (float)ty) {
          ox = sx;
          oy = sy;
        }
      }
    }
    // the waves the 8 x 8 footprint at (ox, oy) overlaps (1 x 1 at the wave's own position, up to 2 x 2 when
    // predicted) take its full cost, a ring of r waves around them 3/4 of it: where the camera stands still the
    // costliest waves still rank first (and take the split), where it moves their neighbours rank next
    const int x0 = (int)floorf(ox * 0.125f), y0 = (int)floorf(oy * 0.125f);
    const int fw = ox * 0.125f != (float)x0 ? 2 : 1, fh = oy * 0.125f != (float)y0 ? 2 : 1;
    const int dw = fw + 2 * r, dh = fh + 2 * r;
    if (lane < dw * dh) {
      const int i = lane % dw, j = lane / dw, x = x0 - r + i, y = y0 - r + j;
      const bool inner = i >= r && i < r + fw && j >= r && j < r + fh;
      const uint32_t v = inner ? c : c - (c >> 2);
      if (x >= 0 && y >= 0 && x < 2 * tx && y < 2 * ty)
        atomicMax(dil + 4 * ((y >> 1) * tx + (x >> 1)) + (y & 1) * 2 + (x & 1), v);
    }
  }
  if (!P.timeline) return;
  const uint32_t r1 = (uint32_t)__builtin_amdgcn_s_memrealtime();
  const uint32_t hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
  if (lane == 0) {
    uint4* o = reinterpret_cast<uint4*>(P.timeline + 8 * (size_t)blockIdx.x);
    o[0] = make_uint4((uint32_t)w.t0, (uint32_t)(w.t0 >> 32), (uint32_t)t1, (uint32_t)(t1 >> 32));
    o[1] = make_uint4(w.r0, r1, hw, (xcc << 28) | ((uint32_t)qw & 0x0FFFFFFFu));
  }
}

// RT_FRAME_WAVE_STATS: this wave's own counts (PRIMARY: node steps, triangle tests, hit lanes; FULL: node steps of
// the four phases, then their triangle tests), for the per-wave time breakdown (tools/wave_breakdown.py)
__device__ __forceinline__ void wave_stats_out(const FrameParams& P, const uint32_t* cnt, int lane, int qw, bool full) {
  if (!P.wave_stats || lane != 0) return;
  uint32_t* o = P.wave_stats + 8 * (size_t)qw;
  if (full) {
    for (int p = 0; p < 4; p++) { o[p] = cnt[ST_PS + p]; o[4 + p] = cnt[ST_PT + p]; }
  } else {
    o[0] = cnt[ST_WNODE]; o[1] = cnt[ST_WTRI]; o[2] = cnt[ST_HITS]; o[3] = 0;
    o[4] = o[5] = o[6] = o[7] = 0;
  }
}

__device__ __forceinline__ void flush_stats(const FrameParams& P, const uint32_t* cnt, int lane) {
#pragma unroll
  for (int c = 0; c < ST_COUNT; c++) {
    unsigned long long v = cnt[c];
    if (c == ST_WNODE || c == ST_WTRI || c == ST_WPOP || c == ST_WCULL || c == ST_WWIDE || c == ST_WCAND || c == ST_WPRE ||
        c == ST_WINS || c == ST_WE1 || c == ST_WE2 || c >= ST_WCANDM)
      v = (lane == 0) ? v : 0;  // wave counts once
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0 && v) atomicAdd(P.stats + c, v);
  }
}

}  // namespace rt
