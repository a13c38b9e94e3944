// rt_variant_api.h -- the call interface between the product's launch sites (rt_frame.hip, rt_rays.hip) and the
// A/B kernel variants (rt_variants.hip). Host declarations only.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_scene.h"

namespace rt {

// ------------------------------------------------------------------------------------------------
// The A/B kernel variants (RT_KERNEL_VARIANT bits, rt_debug_set_variant) live in rt_variants.hip and are
// linked only into the variants library (`make variants` -> lib/librtamd_variants.so): the product
// library's weak default of variant_launch() refuses them with RT_ERR_UNSUPPORTED.
// ------------------------------------------------------------------------------------------------
enum RayQuery { Q_CLOSEST = 0, Q_SHADOW = 1, Q_COLOR = 2 };  // rt_trace_closest / _shadow / _color
enum VariantOp {
  VOP_TRACE_PRIMARY = 0,  // k_trace_primary with a non-default traversal flavour (c.trav)
  VOP_RENDER_FULL,        // k_render_full with a non-default traversal flavour
  VOP_FULL_PIPELINE,      // the FULL stage pipeline (VB_FULL_PIPELINE; VB_PIPE_LANE_* per-lane stages)
  VOP_PRIMARY_DUAL,       // two 8x8 packets per wave (VB_DUAL_CHAIN)
  VOP_PRIMARY_X2,         // two rays per lane (VB_TWO_RAYS_PER_LANE)
  VOP_PRIMARY_PERSISTENT, // persistent threads (VB_PERSISTENT; VB_PERSISTENT_NO_STEAL)
  VOP_RAYS,               // ray-list queries with a non-default traversal flavour
};
struct VariantCall {
  FrameParams P;
  RayParams R;
  int grid = 0, trav = 0, variant = 0, query = 0, device = 0;
  size_t units = 0;
  bool stats = false, hits = false, boxcol = false, small = false;
  hipStream_t st = nullptr;
  hipEvent_t ev_m = nullptr;
  uint32_t* queue = nullptr;  // persistent threads' work counters (8 words)
};
int variant_launch(int op, const VariantCall& c);
bool variants_linked();

}  // namespace rt
