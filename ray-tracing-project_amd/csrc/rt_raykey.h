// rt_raykey.h -- the coherence key of a ray (RT_RAYS_REORDER). One function for the device kernel (k_ray_keys,
// rt_rays.hip) and the host (rt_debug_ray_keys, rt_host.cpp): only comparisons, subtractions, one multiplication
// and correctly rounded divisions, everything compiled with -ffp-contract=off, so both give the same bits.
//
// The key orders rays so that 64 consecutive ones walk nearly the same root-to-leaf paths; it never decides a
// result (rt_ray_kernels.h k_rays). 32 bits:
//   bit 31     the ray is degenerate: a NaN or infinite component of its origin or direction, or a direction of
//              all zeros. Such rays sort last, among themselves by index (the other bits are 0), and are
//              traced as they are.
//   bits 0..30 octant-major (the default): direction octant (3) | origin cell (12) | direction (16)
//              origin-major (VB_RAYKEY_ORIGIN_MAJOR): origin cell (12) | direction octant (3) | direction (16)
//              ("Ray streams", has the counted node fetches that chose the layout and the split)
//   octant     the sign bits of d (x | y << 1 | z << 2), so -0 counts as negative: the octant the traversal's
//              octant test (trace_oct) sees
//   origin     Morton code of the origin on a 16^3 grid over the scene's world bounds, origins outside clamped
//              to the border cells; an axis without extent (lo == hi) is one cell
//   direction  the octahedral map inside the octant: (|dx|, |dy|) / (|dx| + |dy| + |dz|) on a 256 x 256 grid,
//              Morton-interleaved: fine enough that a 1080p frame's camera rays, which share one origin, fall
//              into cells of a few pixels
// A shadow ray's key takes P as the origin and L as the direction (its 0.003 L offset does not matter here).
#pragma once
#include <cstdint>

#include "rt_math.h"

namespace rt {

constexpr uint32_t kRayKeyDegenerate = 0x80000000u;
constexpr int kRayKeyOriginCells = 16, kRayKeyDirCells = 256;  // per axis: 4 and 8 bits

RT_HD uint32_t raykey_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
// bits 0..5 of v to bits 0, 3, .., 15
RT_HD uint32_t raykey_spread3(uint32_t v) {
  v &= 63u;
  v = (v | (v << 8)) & 0x0000F00Fu;   // ....5432 ........ ....10 -> two groups
  v = (v | (v << 4)) & 0x000C30C3u;
  v = (v | (v << 2)) & 0x00249249u;
  return v;
}
// bits 0..7 of v to bits 0, 2, .., 14
RT_HD uint32_t raykey_spread2(uint32_t v) {
  v &= 255u;
  v = (v | (v << 4)) & 0x0F0Fu;
  v = (v | (v << 2)) & 0x3333u;
  v = (v | (v << 1)) & 0x5555u;
  return v;
}
// the cell of x among `cells` equal cells of [lo, hi]; outside (and NaN) clamps; lo >= hi: cell 0
RT_HD uint32_t raykey_cell(float x, float lo, float hi, int cells) {
  const float e = hi - lo;
  if (!(e > 0.0f)) return 0u;
  const float f = (x - lo) / e;
  if (!(f > 0.0f)) return 0u;
  if (f >= 1.0f) return (uint32_t)(cells - 1);
  const int q = (int)(f * (float)cells);
  return (uint32_t)(q < cells - 1 ? q : cells - 1);
}

RT_HD uint32_t ray_key(const float* o, const float* d, const float* bounds6, bool origin_major) {
  const uint32_t ox = raykey_bits(o[0]), oy = raykey_bits(o[1]), oz = raykey_bits(o[2]);
  const uint32_t dx = raykey_bits(d[0]), dy = raykey_bits(d[1]), dz = raykey_bits(d[2]);
  const uint32_t kExp = 0x7F800000u;
  const bool nonfinite = (ox & kExp) == kExp || (oy & kExp) == kExp || (oz & kExp) == kExp || (dx & kExp) == kExp ||
                         (dy & kExp) == kExp || (dz & kExp) == kExp;
  const bool zero_dir = ((dx | dy | dz) & 0x7FFFFFFFu) == 0u;
  if (nonfinite || zero_dir) return kRayKeyDegenerate;
  const uint32_t oct = (dx >> 31) | ((dy >> 31) << 1) | ((dz >> 31) << 2);
  const uint32_t cell = raykey_spread3(raykey_cell(o[0], bounds6[0], bounds6[3], kRayKeyOriginCells)) |
                        (raykey_spread3(raykey_cell(o[1], bounds6[1], bounds6[4], kRayKeyOriginCells)) << 1) |
                        (raykey_spread3(raykey_cell(o[2], bounds6[2], bounds6[5], kRayKeyOriginCells)) << 2);
  const float ax = d[0] < 0.0f ? -d[0] : d[0], ay = d[1] < 0.0f ? -d[1] : d[1], az = d[2] < 0.0f ? -d[2] : d[2];
  const float sum = (ax + ay) + az;  // > 0; +inf for huge components: the map then lands in cell (0, 0)
  const uint32_t dir = raykey_spread2(raykey_cell(ax / sum, 0.0f, 1.0f, kRayKeyDirCells)) |
                       (raykey_spread2(raykey_cell(ay / sum, 0.0f, 1.0f, kRayKeyDirCells)) << 1);
  return origin_major ? (cell << 19) | (oct << 16) | dir : (oct << 28) | (cell << 16) | dir;
}

}  // namespace rt
