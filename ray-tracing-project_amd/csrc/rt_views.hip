// rt_views.hip -- view batches of the MI355X ray-traversal library: rt_render_views / rt_render_views_lit render n
// cameras of one scene, one frame shape and one set of lights in a single launch, straight into the caller's
// device buffers on the caller's stream. The kernels are rt_view_kernels.h k_views_primary / k_views_depth (the frame
// kernels' arithmetic under a per-view camera record); which of them runs, and every refusal, is rt_dispatch.h
// plan_views. The camera records live in a scene-owned device array (rt_scene::ViewScratch).
// rt_render_views_ss / _ss_lit are the same batches with a sample pattern: S rays per pixel averaged in the launch
// (k_views_ss_loop / k_views_ss_packed), the pattern's offsets uploaded behind the camera records by the same copy.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "rt_device.h"
#include "rt_view_kernels.h"

namespace rt {

// the instantiations a batch can launch: <HITS> x the light sources of k_views_depth
template <bool HITS>
static void launch_views(const ViewPlan& plan, const FrameParams& P, const ViewParams& V, hipStream_t st) {
  const dim3 grid((unsigned)plan.total_blocks), block(64);
  if (plan.kernel == VK_PRIMARY) hipLaunchKernelGGL((k_views_primary<HITS>), grid, block, 0, st, P, V);
  else with_light_source(plan.light_source, [&](auto LS) { hipLaunchKernelGGL((k_views_depth<HITS, LS.value>), grid, block, 0, st, P, V); });
}

// the sample kernels: <HITS> x the light sources, in the layout the plan chose
template <bool HITS>
static void launch_views_ss(const ViewPlan& plan, const FrameParams& P, const ViewParams& V, const SampleParams& SP, hipStream_t st) {
  const dim3 grid((unsigned)plan.total_blocks), block(64);
  with_light_source(plan.light_source, [&](auto LS) {
    if (plan.layout == SL_PACKED) hipLaunchKernelGGL((k_views_ss_packed<HITS, LS.value>), grid, block, 0, st, P, V, SP);
    else hipLaunchKernelGGL((k_views_ss_loop<HITS, LS.value>), grid, block, 0, st, P, V, SP);
  });
}

void view_batch_release(rt_scene* s) {
  rt_scene::ViewScratch& v = s->views;
  for (void* e : {v.ev_upload, v.ev_use})
    if (e) {
      (void)hipEventSynchronize((hipEvent_t)e);
      (void)hipEventDestroy((hipEvent_t)e);
    }
  if (v.d_cams) (void)hipFree(v.d_cams);
  if (v.h_cams) (void)hipHostFree(v.h_cams);
  if (v.d_frame) (void)hipFree(v.d_frame);
  for (void* p : v.retired_device) (void)hipFree(p);
  for (void* p : v.retired_host) (void)hipHostFree(p);
  v = rt_scene::ViewScratch{};
}

namespace {

// the derived camera of one view: fill_camera_lights' fields, computed by that function
void fill_view_cam(const FrameParams& scene_params, const rt_camera* cam, ViewCam& c) {
  FrameParams P = scene_params;  // (P.Minv: eye_obj is in object space)
  fill_camera_lights(P, cam, nullptr, 0);
  memset(&c, 0, sizeof c);
  memcpy(c.vinv, P.vinv, sizeof c.vinv);
  memcpy(c.eye, P.eye, sizeof c.eye);
  memcpy(c.eye_obj, P.eye_obj, sizeof c.eye_obj);
  memcpy(c.vp, P.vp, sizeof c.vp);
  c.xscale = P.xscale;
  c.yscale = P.yscale;
}

// a usable pattern: 1..RT_MAX_SAMPLES offsets, each finite and within [-1, 1]
int check_sample_pattern(const char* who, const rt_sample_pattern* pattern) {
  if (!pattern) { set_error("%s: null sample pattern", who); return RT_ERR_INVALID; }
  if (pattern->n_samples < 1 || pattern->n_samples > RT_MAX_SAMPLES) {
    set_error("%s: %d samples (1..%d)", who, pattern->n_samples, RT_MAX_SAMPLES);
    return RT_ERR_INVALID;
  }
  for (int32_t k = 0; k < pattern->n_samples; k++)
    for (int a = 0; a < 2; a++)
      if (!(pattern->offsets[k][a] >= -1.0f && pattern->offsets[k][a] <= 1.0f)) {  // (NaN fails both comparisons)
        set_error("%s: sample offset %d is not finite or lies outside [-1, 1]", who, k);
        return RT_ERR_INVALID;
      }
  return RT_OK;
}

// Room for n camera records on the device and in the pinned staging buffer. A growth retires the old pair instead
// of freeing it (hipFree / hipHostFree wait for the device, hence for renders that still read the old array); the
// capacity doubles, so the retired buffers together stay below the live one, and all go with the scene.
int ensure_view_cams(rt_scene* s, size_t n) {
  rt_scene::ViewScratch& v = s->views;
  int rc;
  if ((rc = ensure_event(v.ev_upload)) || (rc = ensure_event(v.ev_use))) return rc;
  if (n <= v.capacity) return RT_OK;
  const size_t cap = std::max<size_t>(std::max(n, 2 * v.capacity), 64);
  void *d = nullptr, *h = nullptr;
  if (hipMalloc(&d, cap * sizeof(ViewCam)) != hipSuccess || hipHostMalloc(&h, cap * sizeof(ViewCam), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    set_error("rt_render_views: allocation of %zu camera records failed", cap);
    return RT_ERR_NOMEM;
  }
  if (v.d_cams) v.retired_device.push_back(v.d_cams);
  if (v.h_cams) v.retired_host.push_back(v.h_cams);
  v.d_cams = (ViewCam*)d;
  v.h_cams = (ViewCam*)h;
  v.capacity = cap;
  v.fresh = true;  // nothing reads or writes the new pair yet
  return RT_OK;
}

// The cameras of a batch into the scene's array, on st. The host fills the pinned buffer once the previous call's
// upload has left it (the one host-side wait of a batch: for an earlier call's copy, never for its render); the copy
// itself overwrites the device array, so on another stream than the last batch's it first waits -- on the device --
// for that batch's kernel (ev_use). Two batches on two streams therefore run one after the other.
// A sample pattern rides behind the n records (kPatternRecords more, the offsets at their start), in the same copy.
constexpr size_t kPatternRecords = sizeof(((rt_sample_pattern*)nullptr)->offsets) / sizeof(ViewCam);
static_assert(kPatternRecords * sizeof(ViewCam) == sizeof(float) * 2 * RT_MAX_SAMPLES, "the pattern fills whole records");

int upload_view_cams(rt_scene* s, const FrameParams& P, const rt_camera* cams, int32_t n, const rt_sample_pattern* pattern,
                     hipStream_t st) {
  const size_t records = (size_t)n + (pattern ? kPatternRecords : 0);
  int rc = ensure_view_cams(s, records);
  if (rc) return rc;
  rt_scene::ViewScratch& v = s->views;
  if (!v.fresh) {
    HIPCHECK(hipEventSynchronize((hipEvent_t)v.ev_upload));
    if (v.last_stream != (void*)st) HIPCHECK(hipStreamWaitEvent(st, (hipEvent_t)v.ev_use, 0));
  }
  for (int32_t i = 0; i < n; i++) fill_view_cam(P, cams + i, v.h_cams[i]);
  if (pattern) memcpy(v.h_cams + n, pattern->offsets, sizeof pattern->offsets);
  HIPCHECK(hipMemcpyAsync(v.d_cams, v.h_cams, records * sizeof(ViewCam), hipMemcpyHostToDevice, st));
  HIPCHECK(hipEventRecord((hipEvent_t)v.ev_upload, st));
  v.fresh = false;
  v.last_stream = (void*)st;
  return RT_OK;
}

// sampled: the call is rt_render_views_ss / _ss_lit (pattern may then still be null, which is refused)
int render_views(const char* who, rt_scene* s, const rt_view_batch* views, const rt_light* lights, int32_t n_lights,
                 const rt_light_set* ls, const rt_frame* fr, void* hip_stream, bool sampled = false,
                 const rt_sample_pattern* pattern = nullptr) {
  int rc = check_device_scene(s);  // null scene: RT_ERR_INVALID; host-only scene: RT_ERR_NO_DEVICE
  if (rc) return rc;
  if (!views || !fr || fr->width <= 0 || fr->height <= 0) { set_error("%s: invalid arguments", who); return RT_ERR_INVALID; }
  if (sampled && (rc = check_sample_pattern(who, pattern))) return rc;
  if (ls && ls->scene != s) { set_error("%s: the light set belongs to another scene", who); return RT_ERR_INVALID; }
  if (!ls && (n_lights < 0 || n_lights > RT_MAX_LIGHTS || (n_lights && !lights))) {
    set_error("%s: %d lights (at most %d in the array call)", who, n_lights, RT_MAX_LIGHTS);
    return RT_ERR_INVALID;
  }
  if (fr->shard_index != 0) { set_error("%s: a batch renders whole frames (shard_index %d)", who, fr->shard_index); return RT_ERR_UNSUPPORTED; }
  FrameParams P;
  fill_scene_params(s, P);
  int lsrc = LS_KERNARG;
  if (ls) lsrc = fill_light_set(P, ls, 0);  // devices[0]'s copy
  else fill_lights(P, lights, n_lights);
  ViewInputs in;
  in.mode = fr->mode, in.max_depth = fr->max_depth, in.flags = fr->flags, in.shard_count = fr->shard_count;
  in.tiles_x = (fr->width + 15) / 16, in.tiles_y = (fr->height + 15) / 16;
  in.n_views = views->n_views;
  in.variant = kernel_variant();
  in.mem_lights = lsrc == LS_KERNARG ? 0 : P.n_lights;
  if (sampled) in.samples = pattern->n_samples;
  const ViewPlan plan = plan_views(in);
  if (plan.status != RT_OK) { set_error("%s: %s", who, plan.why); return plan.status; }
  if (plan.kernel == VK_NONE) return RT_OK;  // n_views == 0
  if (!views->cameras || !views->rgb) { set_error("%s: cameras and rgb are required", who); return RT_ERR_INVALID; }
  const struct { const void* p; const char* what; } ptrs[] = {{views->rgb, "rgb"}, {views->face, "face"}, {views->t, "t"}};
  for (const auto& q : ptrs)
    if ((rc = check_device_pointer(s, q.p, who, q.what))) return rc;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  P.W = fr->width, P.H = fr->height, P.tiles_x = in.tiles_x, P.tiles_y = in.tiles_y;
  P.shard_count = 1, P.super_tile = 1;
  P.mode = fr->mode, P.max_depth = plan.depth, P.shadows = fr->mode == RT_MODE_FULL ? 1 : 0;
  P.rgb = views->rgb, P.face_out = views->face, P.t_out = views->t;
  if (plan.primary_binary_tree) P.sc.wide_copy_bytes = 0;  // as rt_render under that variant
  if ((rc = upload_view_cams(s, P, views->cameras, views->n_views, pattern, st))) return rc;
  ViewParams V;
  V.cams = s->views.d_cams;
  V.units_per_view = (uint32_t)plan.units_per_view;
  if (sampled) {
    SampleParams SP;
    SP.offsets = reinterpret_cast<const float*>(s->views.d_cams + views->n_views);
    SP.n_samples = pattern->n_samples;
    sample_block(pattern->n_samples, SP.lg_samples, SP.lg_block_w, SP.lg_block_h);
    if (views->face || views->t) launch_views_ss<true>(plan, P, V, SP, st);
    else launch_views_ss<false>(plan, P, V, SP, st);
  } else if (views->face || views->t) launch_views<true>(plan, P, V, st);
  else launch_views<false>(plan, P, V, st);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord((hipEvent_t)s->views.ev_use, st));
  if (hip_stream) return RT_OK;
  HIPCHECK(hipStreamSynchronize(st));
  return check_prefetch_word(s);
}

}  // namespace
}  // namespace rt

using namespace rt;

extern "C" int rt_render_views(rt_scene* s, const rt_view_batch* views, const rt_light* lights, int32_t n_lights,
                               const rt_frame* frame, void* hip_stream) {
  return render_views("rt_render_views", s, views, lights, n_lights, nullptr, frame, hip_stream);
}

extern "C" int rt_render_views_lit(rt_scene* s, const rt_view_batch* views, const rt_light_set* ls, const rt_frame* frame,
                                   void* hip_stream) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!ls) { set_error("rt_render_views_lit: null light set"); return RT_ERR_INVALID; }
  return render_views("rt_render_views_lit", s, views, nullptr, 0, ls, frame, hip_stream);
}

extern "C" int rt_render_views_ss(rt_scene* s, const rt_view_batch* views, const rt_light* lights, int32_t n_lights,
                                  const rt_frame* frame, const rt_sample_pattern* pattern, void* hip_stream) {
  return render_views("rt_render_views_ss", s, views, lights, n_lights, nullptr, frame, hip_stream, true, pattern);
}

extern "C" int rt_render_views_ss_lit(rt_scene* s, const rt_view_batch* views, const rt_light_set* ls, const rt_frame* frame,
                                      const rt_sample_pattern* pattern, void* hip_stream) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!ls) { set_error("rt_render_views_ss_lit: null light set"); return RT_ERR_INVALID; }
  return render_views("rt_render_views_ss_lit", s, views, nullptr, 0, ls, frame, hip_stream, true, pattern);
}

// One supersampled frame into host memory: a one-view batch on the scene's stream into a scene-owned device buffer
// (grown geometrically, freed with the scene), then the copy to the caller. The buffer is only ever used between
// this function's launch and its own wait, so a growth frees the old one at once.
extern "C" int rt_render_ss(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* frame,
                            const rt_sample_pattern* pattern, float* out_rgb) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!cam || !frame || !out_rgb || frame->width <= 0 || frame->height <= 0) { set_error("rt_render_ss: invalid arguments"); return RT_ERR_INVALID; }
  const size_t need = (size_t)frame->width * (size_t)frame->height * 3;
  rt_scene::ViewScratch& v = s->views;
  if (need > v.frame_capacity) {
    const size_t cap = std::max(need, 2 * v.frame_capacity);
    void* d = nullptr;
    if (hipMalloc(&d, cap * sizeof(float)) != hipSuccess) {
      (void)hipGetLastError();
      set_error("rt_render_ss: allocation of a %d x %d frame failed", frame->width, frame->height);
      return RT_ERR_NOMEM;
    }
    if (v.d_frame) (void)hipFree(v.d_frame);
    v.d_frame = (float*)d;
    v.frame_capacity = cap;
  }
  rt_view_batch vb;
  vb.n_views = 1, vb.cameras = cam, vb.rgb = v.d_frame, vb.face = nullptr, vb.t = nullptr;
  if ((rc = render_views("rt_render_ss", s, &vb, lights, n_lights, nullptr, frame, s->stream, true, pattern))) return rc;
  HIPCHECK(hipMemcpyAsync(out_rgb, v.d_frame, need * sizeof(float), hipMemcpyDeviceToHost, (hipStream_t)s->stream));
  HIPCHECK(hipStreamSynchronize((hipStream_t)s->stream));
  return check_prefetch_word(s);
}
