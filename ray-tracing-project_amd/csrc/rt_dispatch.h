// rt_dispatch.h -- which kernel renders a frame, and in which block order: one pure host function (plan_frame)
// that rt_frame.hip's render_one reads for every such decision, and that rt_debug_frame_plan shows the tests
// without a device; and the same for a view batch (plan_views, read by rt_views.hip, shown by rt_debug_view_plan).
// Host-only: no HIP, no globals, no environment -- a knob that changes the plan is an input.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/rt/rt_api.h"
#include "rt_internal.h"

namespace rt {

constexpr size_t kFullSmallSceneBytes = 32u << 20;  // 8 XCDs x 4 MiB L2
constexpr int kSplitK = 1536;  // FULL lone frames: waves split into 16-lane sub-waves (FrameParams::split_k); round 5
                               // re-sweep without the spill: 1536 +2.5..6% over 2048 (profiles/ab/r05_c5_split_ab.txt)
constexpr int kSplitKPrimary = 256;   // the same for k_primary_fused (small scenes); round 6 re-sweep after the
                                      // scene-level map: 256 against 1024 -2.5% static, -7% moving, -8% at a stopped
                                      // pose (C2 lone frames, profiles/ab/r06_split_size_ab.txt)

// Super-tile width of a shard_count-way split (shard_tile_xy, rt_api.h rt_frame): 4x4 tiles (64x64
// pixels) per super-tile when the frame is split, so that the waves an XCD runs together trace
// neighbouring pixels (the rank's L2 working set stays compact): C4 over 8 / 4 GPUs +10% / +7% per GPU
// against single tiles interleaved (profiles/ab/r02_super_tiles_ab.txt); an unsplit frame keeps its tile
// order (super-tiles there: C3 +-1%, C4 -3%). A pure function of the shard count: the render,
// rt_frame_shard_tiles, the pack on every rank and the unpack on rank 0 derive the same layout, whatever
// the process environment or the kernel variant.
inline int frame_super_tile(int shard_count) { return shard_count > 1 ? kShardSuperTile : 1; }

// The product's traversal flavour is the binary tree with the LDS wave stack (TRAV_B2_LDS); the other
// flavours are A/B variants built only into the variants library (variant_launch).
inline int pick_trav(int variant, bool has_wide4) {
  if (variant & VB_VGPR_STACK) return TRAV_B2_VGPR;
  if ((variant & VB_WIDE4) && has_wide4) return TRAV_W4;
  return TRAV_B2_LDS;
}

enum FrameKernel {
  FK_NONE = 0,            // an empty shard: nothing to launch
  FK_GENERIC_DEPTH,       // k_render_depth: any recursion limit but the mode's own, or VB_GENERIC_DEPTH
  FK_PRIMARY_FUSED,       // k_primary_fused (the default PRIMARY / box-colours kernel)
  FK_PRIMARY_TRACE_SHADE, // k_trace_primary + k_shade_primary (every counting frame; VB_SPLIT_PRIMARY; A/B flavours)
  FK_PRIMARY_DUAL,        // k_primary_dual (VB_DUAL_CHAIN)
  FK_PRIMARY_TWO_RAYS,    // k_trace_primary_x2 + k_shade_primary (VB_TWO_RAYS_PER_LANE)
  FK_PRIMARY_PERSISTENT,  // k_trace_primary_persistent + k_shade_primary (VB_PERSISTENT)
  FK_FULL_MEGAKERNEL,     // k_render_full (the default FULL kernel)
  FK_FULL_PIPELINE,       // the k_full_* stage pipeline (VB_FULL_PIPELINE)
};

struct FrameInputs {
  int mode = RT_MODE_PRIMARY, max_depth = 0, flags = 0;  // rt_frame's, validated
  int tiles_x = 0, tiles_y = 0;                          // 16x16-pixel tiles of the frame
  int shard_index = 0, shard_count = 1;
  int variant = 0;
  uint64_t record_bytes = 0;  // the scene's binary node + triangle records
  bool has_wide4 = false;     // the scene has the quantised 4-wide tree (DevScene::n_nodes4 > 0)
  bool alone = true;          // no other frame of this scene in flight
  int mem_lights = 0;         // lights the frame reads from a light set in device memory (0 = none: kernel arguments)
  bool occluder_cache = true; // ... with the wave-level occluder cache of its shadow packets (VB_NO_OCCLUDER_CACHE: off)
  // debug-environment knobs (RT_SPLIT_K, RT_SPLIT_KP, RT_TIMELINE_SPLIT), at their defaults unless set
  int split_k = kSplitK, split_kp = kSplitKPrimary;
  bool timeline_split = false;
};

struct FramePlan {
  FrameKernel kernel = FK_NONE;
  int trav = TRAV_B2_LDS;
  bool needs_variants = false;   // only the variants library can render this frame
  int grid = 0;                  // this shard's tile slots (shard_tile_slots)
  size_t units = 0;              // one-wave blocks of the render kernel
  int depth = 1;                 // the frame's recursion limit (max_depth, or the mode's own)
  bool l2_resident = false;      // the scene's records fit the chip's 32 MiB of L2
  bool full_small_build = false; // k_render_full at the small scenes' occupancy (VB_FULL_8_WAVES / _SMALL_BUILD force it)
  int xcd_remap = 0;             // FrameParams::xcd_remap
  bool rotate_bands = false;     // this frame takes the next FrameParams::xcd_rot
  bool writes_wave_stats = true; // false: the kernel keeps no per-wave counts, an RT_FRAME_WAVE_STATS frame is refused
  bool pipeline_buffers = false; // FULL under VB_FULL_PIPELINE: binds the stage pipeline's hand-off buffers (whole frames only)
  bool lpt = false;              // dispatched longest-first (k_order_lpt)
  int split_ceiling = 0;         // FrameParams::split_k once the frame has an order (0: the kernel never splits)
  bool primary_binary_tree = false, lpt_coarse = false;  // VB_PRIMARY_BINARY_TREE, VB_COARSE_COST_BUCKETS
  int light_source = LS_KERNARG; // k_render_depth's LSRC: LS_MEMORY_CACHED / LS_MEMORY for a light set in device memory
  int variant = 0;               // handed on to variant_launch: rt_variants.hip reads the pipeline's and persistent's sub-bits
};

inline FramePlan plan_frame(const FrameInputs& in) {
  FramePlan p;
  const int v = p.variant = in.variant;
  const bool boxcol = in.mode == RT_MODE_BOX_COLORS, full = in.mode == RT_MODE_FULL, prim = !full;
  const bool stats = (in.flags & RT_FRAME_STATS) != 0;
  // box-colour frames return before any reflection: one depth, the PRIMARY kernels' dispatch
  const int own_depth = full ? 2 : 1;
  p.depth = (in.max_depth > 0 && !boxcol) ? in.max_depth : own_depth;
  p.trav = pick_trav(v, in.has_wide4);
  p.grid = shard_tile_slots(in.tiles_x, in.tiles_y, frame_super_tile(in.shard_count), in.shard_index, in.shard_count);
  p.l2_resident = in.record_bytes <= kFullSmallSceneBytes;
  p.full_small_build = (v & VB_FULL_SMALL_BUILD) || (!(v & VB_FULL_8_WAVES) && p.l2_resident);
  p.primary_binary_tree = (v & VB_PRIMARY_BINARY_TREE) != 0;
  p.lpt_coarse = (v & VB_COARSE_COST_BUCKETS) != 0;
  // a light set in device memory is read by the generic kernel's memory-lights instantiations alone: PRIMARY and
  // FULL at every depth (a box-colours frame has no lights and keeps its kernel)
  const bool mem_lights = !boxcol && in.mem_lights > 0;
  p.light_source = !mem_lights ? LS_KERNARG : in.occluder_cache ? LS_MEMORY_CACHED : LS_MEMORY;
  const bool generic = !boxcol && (p.depth != own_depth || (v & VB_GENERIC_DEPTH) || mem_lights);
  const bool dual = prim && !stats && (in.max_depth <= 1 || boxcol) && !(v & VB_DUAL_EXCLUDED) && (v & VB_DUAL_CHAIN) && !mem_lights;
  const bool lds = p.trav == TRAV_B2_LDS;
  FrameKernel k;
  if (generic) k = FK_GENERIC_DEPTH;
  else if (dual) k = FK_PRIMARY_DUAL;
  else if (prim && !stats && !(v & VB_PRIMARY_UNFUSED) && lds) k = FK_PRIMARY_FUSED;
  else if (prim && !stats && (v & VB_TWO_RAYS_PER_LANE) && lds) k = FK_PRIMARY_TWO_RAYS;
  else if (prim && !stats && (v & VB_PERSISTENT) && lds) k = FK_PRIMARY_PERSISTENT;
  else if (prim) k = FK_PRIMARY_TRACE_SHADE;
  else k = (v & VB_FULL_PIPELINE) ? FK_FULL_PIPELINE : FK_FULL_MEGAKERNEL;
  p.kernel = p.grid > 0 ? k : FK_NONE;
  p.units = (size_t)p.grid * (dual ? 2 : 4);
  p.writes_wave_stats = !generic;
  // The refusals look at the frame's mode and variant bits, not at the kernel chosen above, so a frame the
  // generic-depth kernel renders is still refused for a bit it never uses (VB_FULL_PIPELINE's buffers and
  // whole-frame rule, VB_TWO_RAYS_PER_LANE / VB_PERSISTENT, a non-LDS flavour).
  p.pipeline_buffers = full && (v & VB_FULL_PIPELINE);
  p.needs_variants = !lds || dual || p.pipeline_buffers || (prim && !stats && (v & (VB_TWO_RAYS_PER_LANE | VB_PERSISTENT)));
  // block order: chunked XCD order -- block b runs on XCD b % 8, and the XCD's k-th block takes the k-th
  // position of its runs of C consecutive blocks. Scenes whose records exceed the chip's 32 MiB of L2 take
  // one contiguous band of the frame per XCD (C = units / 8), so that each XCD's 4 MiB L2 holds the part
  // of the scene its band sees (L2 hit 0.90 -> 0.94 on C3): a frame alone on the GPU +4.3% on C3, +8.7%
  // on C4. With frames in flight the XCDs' bands rotate frame by frame (xcd_rot), so that no XCD keeps
  // the costliest band of every frame: +1.5% on C3 at 100 frames (fixed bands lost 1-3% there); all in
  // profiles/ab/r05_xcd_bands_ab.txt. L2-resident scenes keep runs of C = 64 (bunny one frame alone with
  // bands: PRIMARY -9%, FULL -6..-12% -- no locality to gain, and the bands differ in cost; runs of
  // 32 .. 256 within noise, profiles/ab/r05_xcd_run_ab.txt; 64 against the plain order -4% trace time on
  // C3 before the bands). VB_XCD_RUNS_4 / _16 select runs of 4 / 16 blocks, VB_DISPATCH_ORDER the plain
  // dispatch order, VB_XCD_ORDER one contiguous tile range per XCD (256-thread blocks)
  const int sel = v & VB_DISPATCH_ORDER;
  const int run = p.l2_resident ? 64 : std::max<int>(2, (int)(p.units / 8));
  p.xcd_remap = (v & VB_XCD_ORDER) ? 1 : sel == 0 ? run : sel == VB_XCD_RUNS_4 ? 4 : sel == VB_XCD_RUNS_16 ? 16 : 0;
  p.rotate_bands = !in.alone && !p.l2_resident && p.xcd_remap >= 2;
  // longest-first dispatch (k_order_lpt) for the one-wave render kernels of the default build. (A box-colours
  // frame under VB_GENERIC_DEPTH keeps the fused kernel but not the longest-first order.)
  const bool one_wave_kernel = !stats && lds && (generic || dual || k == FK_FULL_MEGAKERNEL ||
                                                 (k == FK_PRIMARY_FUSED && !(v & VB_GENERIC_DEPTH)));
  // Only for a frame that has the GPU to itself (no other frame of this scene in flight): then the
  // tail of the frame would leave the GPU idle and longest-first fills it (one frame at a time: C3
  // +18%, C5 +28%); with frames in flight the next frame fills the tail and the default order's tile
  // locality is worth more (LPT measured -3..-7% there). VB_LPT_IN_FLIGHT forces it, VB_NO_LPT disables it.
  // (VB_LPT_IN_FLIGHT is A/B only and the product path never takes it: with frames in flight the one map is
  // shared by frames that overlap, so a frame can read an order that a sort is rewriting and skip or repeat waves)
  p.lpt = one_wave_kernel && !(v & VB_NO_LPT) && p.xcd_remap >= 2 && p.grid > 0 && (in.alone || (v & VB_LPT_IN_FLIGHT));
  // lone frames of small scenes run their costliest waves as 16-lane sub-waves (launch_frame); a timeline frame
  // only under RT_TIMELINE_SPLIT. Rounded down to a multiple of 8 and at most a quarter of the frame's waves.
  // k_render_full splits by the build it runs, so VB_FULL_SMALL_BUILD also splits a large scene's frames.
  const bool may_split = !(in.flags & RT_FRAME_TIMELINE) || in.timeline_split;
  const int quarter = (int)(p.units / 4);
  if (p.kernel == FK_PRIMARY_FUSED && p.l2_resident && may_split)
    p.split_ceiling = std::max(0, std::min(in.split_kp, quarter)) & ~7;
  if (p.kernel == FK_FULL_MEGAKERNEL && p.full_small_build && may_split && !stats && lds)
    p.split_ceiling = std::max(0, std::min(in.split_k, quarter)) & ~7;
  return p;
}

// ---- view batches (rt_views.hip rt_render_views; shown to the tests by rt_debug_view_plan) ----
// One launch of one-wave blocks in plain order: block b renders view b / units_per_view, logical wave
// b % units_per_view of it (tile * 4 + quarter). The limit on the blocks is the launch's: a grid holds fewer than
// 2^32 work-items, 64 per block, so 2^26 blocks and more are refused (which keeps the count below 2^31 as well).
constexpr int64_t kMaxViewBlocks = ((int64_t)1 << 26) - 1;

enum ViewKernel {
  VK_NONE = 0,  // an empty batch (or a refused one): nothing to launch
  VK_PRIMARY,   // k_views_primary: PRIMARY at depth 1 with the lights in the kernel arguments
  VK_DEPTH,     // k_views_depth: every other depth, FULL, lights read from device memory, VB_GENERIC_DEPTH
};

struct ViewInputs {
  int mode = RT_MODE_PRIMARY, max_depth = 0, flags = 0, shard_count = 0;  // rt_frame's, as given
  int tiles_x = 0, tiles_y = 0;                                           // 16x16-pixel tiles of one view
  int64_t n_views = 0;
  int variant = 0;
  int mem_lights = 0;  // lights the batch reads from a light set in device memory (0 = none: kernel arguments)
  int samples = 1;     // rays per pixel (rt_render_views_ss); 1: rt_render_views' plan, unchanged
};

// Supersampled batches (rt_render_views_ss): where the S samples of a pixel sit.
//   SL_LOOP:   a wave is an 8x8-pixel block as in k_views_depth; each lane traces its pixel's S samples one after
//              the other (any S).
//   SL_PACKED: a wave is 64 / S neighbouring pixels times S samples, lane = pixel_in_block * S + k (S a power of
//              two from 2 to 64). The pixel block is block_w x block_h (sample_block below); a 16x16 tile is 4 S waves.
enum SampleLayout { SL_LOOP = 0, SL_PACKED = 1 };
// the layout a power-of-two sample count takes by default; VB_SAMPLE_LAYOUT selects the other one. Measured
// (tools/supersample_ab.py, profiles/ab/supersample_ab.txt; DESIGN.md "Supersampled views"): at every count from 2
// to 64 the packed waves were faster than the loop beyond the run-to-run spread in every case on both scenes (device
// time about 1.3x at S = 2 up to about 7x at S = 64), so every count takes them.
inline SampleLayout default_sample_layout(int /*samples*/) { return SL_PACKED; }
// the packed layout's pixel block, as base-2 logarithms: S = 2: 8x4, 4: 4x4, 8: 4x2, 16: 2x2, 32: 2x1, 64: 1x1
inline void sample_block(int samples, int& lg_samples, int& lg_w, int& lg_h) {
  lg_samples = 0;
  while ((1 << lg_samples) < samples) lg_samples++;
  const int lg_pixels = 6 - lg_samples;
  lg_w = (lg_pixels + 1) / 2, lg_h = lg_pixels / 2;
}

struct ViewPlan {
  ViewKernel kernel = VK_NONE;
  int depth = 1;                 // the recursion limit (max_depth, or the mode's own)
  int64_t units_per_view = 0;    // one-wave blocks of a view
  int64_t total_blocks = 0;
  int light_source = LS_KERNARG; // k_views_depth's LSRC
  bool primary_binary_tree = false;  // VB_PRIMARY_BINARY_TREE, as for frames
  // supersampled batches (samples = 1: the loop's numbers, which are rt_render_views')
  SampleLayout layout = SL_LOOP;
  int pixels_per_wave = 64;      // 64 (loop) or 64 / samples (packed)
  int waves_per_tile = 4;        // one-wave blocks of a 16x16 tile: 4 (loop) or 4 * samples (packed)
  int status = RT_OK;            // not RT_OK: the batch is refused with this status, because of `why`
  const char* why = "";
};

inline ViewPlan plan_views(const ViewInputs& in) {
  ViewPlan p;
  auto refuse = [&](int status, const char* why) {
    p.kernel = VK_NONE, p.status = status, p.why = why;
    return p;
  };
  const bool full = in.mode == RT_MODE_FULL;
  p.depth = in.max_depth > 0 ? in.max_depth : (full ? 2 : 1);
  if (in.samples < 1 || in.samples > RT_MAX_SAMPLES) return refuse(RT_ERR_INVALID, "n_samples outside 1..RT_MAX_SAMPLES");
  const bool pow2 = in.samples >= 2 && (in.samples & (in.samples - 1)) == 0;  // others always take the loop
  if (pow2) p.layout = (SampleLayout)(default_sample_layout(in.samples) ^ ((in.variant & VB_SAMPLE_LAYOUT) ? 1 : 0));
  if (p.layout == SL_PACKED) p.pixels_per_wave = 64 / in.samples, p.waves_per_tile = 4 * in.samples;
  p.units_per_view = (int64_t)p.waves_per_tile * in.tiles_x * in.tiles_y;
  p.light_source = in.mem_lights <= 0 ? LS_KERNARG : (in.variant & VB_NO_OCCLUDER_CACHE) ? LS_MEMORY : LS_MEMORY_CACHED;
  p.primary_binary_tree = (in.variant & VB_PRIMARY_BINARY_TREE) != 0;
  if (in.mode == RT_MODE_BOX_COLORS) return refuse(RT_ERR_UNSUPPORTED, "box colours need the scene's per-face colour pass, which a batch leaves out");
  if (in.mode != RT_MODE_PRIMARY && !full) return refuse(RT_ERR_INVALID, "bad mode");
  if (in.max_depth < 0 || in.max_depth > RT_MAX_TRACE_DEPTH) return refuse(RT_ERR_INVALID, "max_depth outside 0..RT_MAX_TRACE_DEPTH");
  if (in.shard_count != 0 && in.shard_count != 1) return refuse(RT_ERR_UNSUPPORTED, "a batch renders whole frames (shard_count must be 0 or 1)");
  if (in.flags & (RT_FRAME_STATS | RT_FRAME_TIMELINE | RT_FRAME_WAVE_STATS)) return refuse(RT_ERR_UNSUPPORTED, "a batch keeps no counters, timeline or per-wave counts");
  if (in.flags & ~RT_FRAME_WRITE_HITS) return refuse(RT_ERR_INVALID, "bad flags");
  if (in.tiles_x <= 0 || in.tiles_y <= 0) return refuse(RT_ERR_INVALID, "empty frame");
  if (in.n_views < 0 || in.n_views > RT_MAX_VIEWS) return refuse(RT_ERR_INVALID, "n_views outside 0..RT_MAX_VIEWS");
  // (tiles up to 2^27 a side give 2^56 units, times 2^16 views: saturated so the product stays within 64 bits)
  p.total_blocks = p.units_per_view > ((int64_t)1 << 40) ? INT64_MAX : p.units_per_view * in.n_views;
  if (p.total_blocks > kMaxViewBlocks)
    return refuse(RT_ERR_INVALID, p.layout == SL_PACKED ? "2^26 or more one-wave blocks in one batch (packed samples)" : "2^26 or more 8x8-pixel blocks in one batch");
  if (in.n_views == 0) return p;
  const bool generic = full || p.depth != 1 || in.mem_lights > 0 || (in.variant & VB_GENERIC_DEPTH);
  p.kernel = generic ? VK_DEPTH : VK_PRIMARY;
  return p;
}

}  // namespace rt
