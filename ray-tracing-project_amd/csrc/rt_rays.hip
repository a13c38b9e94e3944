// rt_rays.hip -- ray-list queries of the MI355X ray-traversal library: the device-resident, stream-ordered
// path (rt_trace_stream, rt_rays_camera), its coherence reorder (key kernel + radix sort + indexed packets),
// and the host-pointer entry points (rt_trace_closest and its siblings), which are "upload, stream path,
// download". The packet kernels themselves are rt_ray_kernels.h k_rays / k_rays_color / k_rays_depth; the stage kernels
// of RT_RAYS_WAVEFRONT are rt_wavefront.h, their host glue (enqueue_wavefront) is here.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "rt_device.h"
#include "rt_ray_kernels.h"
#include "rt_raykey.h"
#include "rt_variant_api.h"
#include "rt_wavefront.h"

namespace rt {

// one thread per ray: its coherence key and its index, the radix sort's (key, value) pair
__global__ __launch_bounds__(256) void k_ray_keys(const float* __restrict__ a3, const float* __restrict__ b3, int n,
                                                  const float* __restrict__ bounds6, int origin_major,
                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ index) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  float o[3], d[3], b[6];
  for (int k = 0; k < 3; k++) { o[k] = a3[3 * (size_t)i + k]; d[k] = b3[3 * (size_t)i + k]; }
  for (int k = 0; k < 6; k++) b[k] = bounds6[k];
  keys[i] = ray_key(o, d, b, origin_major != 0);
  index[i] = (uint32_t)i;
}

// rt_rays_camera: the primary rays of a W x H frame as a list, pixel (px, py) at index py * W + px -- the o and d
// of primary_ray(), the frame kernels' own generator
__global__ __launch_bounds__(256) void k_camera_rays(FrameParams P, float* __restrict__ o3, float* __restrict__ d3) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)P.W * P.H) return;
  const Ray r = primary_ray(P, (int)(i % (size_t)P.W), (int)(i / (size_t)P.W));
  o3[3 * i + 0] = r.o.x; o3[3 * i + 1] = r.o.y; o3[3 * i + 2] = r.o.z;
  d3[3 * i + 0] = r.d.x; d3[3 * i + 1] = r.d.y; d3[3 * i + 2] = r.d.z;
}

void ray_stream_release(rt_scene* s) {
  rt_scene::RayScratch& r = s->rays;
  if (r.ev) {
    (void)hipEventSynchronize((hipEvent_t)r.ev);
    (void)hipEventDestroy((hipEvent_t)r.ev);
  }
  if (r.d_buf) (void)hipFree(r.d_buf);
  if (r.d_tmp) (void)hipFree(r.d_tmp);
  if (r.d_wf) (void)hipFree(r.d_wf);
  if (r.d_counts) (void)hipFree(r.d_counts);
  r = rt_scene::RayScratch{};
  for (auto& u : s->list_use) {
    (void)hipEventSynchronize((hipEvent_t)u.second);
    (void)hipEventDestroy((hipEvent_t)u.second);
  }
  s->list_use.clear();
}

// A list call enqueued on a caller's stream reads the scene's records until its kernels end, whatever its flags
// (an in-order list uses no scratch and records no scratch event): one event per caller stream, recorded after
// each such call, for rt_scene_update to wait for (rt_refit.hip update_quiesce). Callers use a handful of streams;
// beyond kListStreams the oldest entry's work is waited for and its event reused.
constexpr size_t kListStreams = 64;
static int note_list_use(rt_scene* s, hipStream_t st) {
  void* ev = nullptr;
  for (auto& u : s->list_use)
    if (u.first == (void*)st) ev = u.second;
  if (!ev && s->list_use.size() >= kListStreams) {
    ev = s->list_use.front().second;
    HIPCHECK(hipEventSynchronize((hipEvent_t)ev));
    s->list_use.erase(s->list_use.begin());
    s->list_use.emplace_back((void*)st, ev);
  } else if (!ev) {
    if (const int rc = rt::ensure_event(ev)) return rc;
    s->list_use.emplace_back((void*)st, ev);
  }
  HIPCHECK(hipEventRecord((hipEvent_t)ev, st));
  return RT_OK;
}

namespace {

// the reorder scratch's layout: four arrays of `capacity` words, then the six floats of the key grid
struct ScratchView {
  uint32_t *keys_in, *keys_out, *index_in, *perm;
  float* bounds;
};
ScratchView scratch_view(const rt_scene::RayScratch& r) {
  return ScratchView{r.d_buf, r.d_buf + r.capacity, r.d_buf + 2 * r.capacity, r.d_buf + 3 * r.capacity,
                     reinterpret_cast<float*>(r.d_buf + 4 * r.capacity)};
}

// room for n rays and the sort's temporary storage. A growth waits for the previous use, then reallocates
// (hipFree / hipMalloc: the one place a stream call may stall).
int ensure_scratch(rt_scene* s, size_t n, size_t tmp_bytes) {
  rt_scene::RayScratch& r = s->rays;
  if (const int rc = ensure_event(r.ev)) return rc;
  if (n > r.capacity || tmp_bytes > r.tmp_bytes) HIPCHECK(hipEventSynchronize((hipEvent_t)r.ev));
  if (n > r.capacity) {
    const size_t cap = std::max<size_t>(std::max(n, 2 * r.capacity), 4096);
    if (r.d_buf) (void)hipFree(r.d_buf);
    r.d_buf = nullptr;
    r.capacity = 0;
    if (hipMalloc((void**)&r.d_buf, cap * 16 + 32) != hipSuccess) {
      (void)hipGetLastError();
      set_error("trace: device allocation failed");
      return RT_ERR_NOMEM;
    }
    r.capacity = cap;
    if (const int rc = host_mirror_geometry(s)) return rc;  // (hs.wv after a device update)
    HIPCHECK(hipMemcpy(scratch_view(r).bounds, scene_ray_bounds(s), 24, hipMemcpyHostToDevice));
  }
  if (tmp_bytes > r.tmp_bytes) {
    const size_t want = std::max(tmp_bytes, 2 * r.tmp_bytes);
    if (r.d_tmp) (void)hipFree(r.d_tmp);
    r.d_tmp = nullptr;
    r.tmp_bytes = 0;
    if (hipMalloc(&r.d_tmp, want) != hipSuccess) {
      (void)hipGetLastError();
      set_error("trace: device allocation failed");
      return RT_ERR_NOMEM;
    }
    r.tmp_bytes = want;
  }
  return RT_OK;
}

// keys, sort: the permutation of R's rays on st. The scratch is the scene's: a call on another stream than the
// last one first waits for that call's use.
int enqueue_reorder(rt_scene* s, const RayParams& R, hipStream_t st, const uint32_t** perm) {
  const int n = R.n;
  size_t tmp = 0;
  HIPCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32, st));
  int rc = ensure_scratch(s, (size_t)n, tmp);
  if (rc) return rc;
  rt_scene::RayScratch& r = s->rays;
  if (r.last_stream && r.last_stream != (void*)st) HIPCHECK(hipStreamWaitEvent(st, (hipEvent_t)r.ev, 0));
  const ScratchView v = scratch_view(r);
  const int origin_major = (kernel_variant() & VB_RAYKEY_ORIGIN_MAJOR) ? 1 : 0;
  hipLaunchKernelGGL(k_ray_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, R.o, R.d, n, (const float*)v.bounds,
                     origin_major, v.keys_in, v.index_in);
  HIPCHECK(hipGetLastError());
  // a stable sort of the keys' 32 bits with the indices as values: equal keys keep index order, so the order is
  // total and the same on every run (= a stable argsort of the keys)
  size_t tb = r.tmp_bytes;
  HIPCHECK(hipcub::DeviceRadixSort::SortPairs(r.d_tmp, tb, (const uint32_t*)v.keys_in, v.keys_out, (const uint32_t*)v.index_in,
                                              v.perm, n, 0, 32, st));
  *perm = v.perm;
  return RT_OK;
}

// RT_RAYS_REORDER of a list call on st: R.perm for a list beyond one packet, and the record rt_debug_ray_order reads
int begin_reorder(rt_scene* s, RayParams& R, hipStream_t st) {
  const bool sorted = R.n > 64;  // up to 64 rays are one packet in any order
  int rc;
  if (sorted && (rc = enqueue_reorder(s, R, st, &R.perm))) return rc;
  s->rays.last_n = R.n;
  s->rays.last_sorted = sorted;
  return RT_OK;
}

// RT_RAYS_STATS of a list call on st: the scene's counters, cleared, as the kernels' P.stats
int begin_stats(rt_scene* s, FrameParams& P, hipStream_t st) {
  P.stats = s->d_stats;
  HIPCHECK(hipMemsetAsync(s->d_stats, 0, kStatSlots * sizeof(unsigned long long), st));
  s->last_flags = RT_FRAME_STATS;  // rt_debug_counters reads these counters
  return RT_OK;
}

// the packet kernels of one query on st (R's pointers are device memory); flags: RT_RAYS_*
int enqueue_rays(rt_scene* s, int query, int flags, RayParams R, const rt_light* lights, int32_t n_lights, hipStream_t st) {
  FrameParams P;
  fill_scene_params(s, P);
  if (query == Q_COLOR) fill_lights(P, lights, n_lights);
  const bool stats = (flags & RT_RAYS_STATS) != 0, reorder = (flags & RT_RAYS_REORDER) != 0;
  const bool w4 = pick_trav(kernel_variant(), P.sc.n_nodes4 > 0) == TRAV_W4;
  if (w4 && !variants_linked()) {
    set_error("trace: kernel variant %d is an A/B build option, not in this library (make variants)", kernel_variant());
    return RT_ERR_UNSUPPORTED;
  }
  if (w4 && stats) {
    set_error("rt_trace_stream: RT_RAYS_STATS counts the binary-tree packets only, not kernel variant %d", kernel_variant());
    return RT_ERR_UNSUPPORTED;
  }
  int rc;
  if (reorder && (rc = begin_reorder(s, R, st))) return rc;
  if (stats && (rc = begin_stats(s, P, st))) return rc;
  const int grid = (R.n + 255) / 256;
  if (w4) {
    VariantCall vc;
    vc.P = P, vc.R = R, vc.grid = grid, vc.st = st, vc.query = query;
    variant_launch(VOP_RAYS, vc);
  } else if (query == Q_COLOR) {
    with_bools([&](auto ST) { hipLaunchKernelGGL((k_rays_color<TRAV_B2_LDS, ST.value>), dim3(grid), dim3(256), 0, st, P, R); }, stats);
  } else {
    with_bools([&](auto ANY, auto ST) { hipLaunchKernelGGL((k_rays<ANY.value, TRAV_B2_LDS, ST.value>), dim3(grid), dim3(256), 0, st, P, R); },
               query == Q_SHADOW, stats);
  }
  HIPCHECK(hipGetLastError());
  if (R.perm) {  // the scratch is in use until here
    HIPCHECK(hipEventRecord((hipEvent_t)s->rays.ev, st));
    s->rays.last_stream = (void*)st;
  }
  return RT_OK;
}

// ---- rt_trace_stream_color: traceRay at any depth and mode ----

// the in-order (or level-0 reordered) list kernel k_rays_depth; P carries mode, depth and lights
int enqueue_rays_depth(rt_scene* s, int flags, RayParams R, FrameParams& P, hipStream_t st, int lsrc) {
  const bool stats = (flags & RT_RAYS_STATS) != 0, reorder = (flags & RT_RAYS_REORDER) != 0;
  int rc;
  if (reorder && (rc = begin_reorder(s, R, st))) return rc;
  if (stats && (rc = begin_stats(s, P, st))) return rc;
  const int grid = (R.n + 255) / 256;
  with_light_source(lsrc, [&](auto LS) {
    with_bools([&](auto ST) { hipLaunchKernelGGL((k_rays_depth<ST.value, decltype(LS)::value>), dim3(grid), dim3(256), 0, st, P, R); }, stats);
  });
  HIPCHECK(hipGetLastError());
  if (R.perm) {
    HIPCHECK(hipEventRecord((hipEvent_t)s->rays.ev, st));
    s->rays.last_stream = (void*)st;
  }
  return RT_OK;
}

// the wavefront state of n rays at D levels, carved from one allocation (rt_wavefront.h has the sizes)
WfState wf_view(void* base, size_t n, int D) {
  float* f = (float*)base;
  auto take = [&](size_t words) { float* q = f; f += words; return q; };
  WfState w;
  w.o = take(3 * n), w.d = take(3 * n), w.hp = take(3 * n), w.hn = take(3 * n);
  w.hmat = (int32_t*)take(n), w.hface = (uint32_t*)take(n);
  w.ka = take(3 * n), w.kd = take(3 * n), w.ks = take(3 * n), w.ns = take(n);
  w.face0 = (int32_t*)take(n), w.t0 = take(n), w.levels = (int32_t*)take(n);
  w.direct = take(3 * n * (size_t)D);
  w.list_a = (uint32_t*)take(n), w.list_b = (uint32_t*)take(n), w.key_a = (uint32_t*)take(n), w.key_b = (uint32_t*)take(n);
  return w;
}

// room for the state of n rays at D levels; a growth waits for the previous use (as ensure_scratch)
int ensure_wavefront(rt_scene* s, size_t n, int D) {
  rt_scene::RayScratch& r = s->rays;
  if (const int rc = ensure_event(r.ev)) return rc;
  if (!r.d_counts && hipMalloc((void**)&r.d_counts, (RT_MAX_TRACE_DEPTH + 2) * sizeof(uint32_t)) != hipSuccess) {
    (void)hipGetLastError();
    r.d_counts = nullptr;
    set_error("trace: device allocation failed");
    return RT_ERR_NOMEM;
  }
  const size_t need = n * wf_bytes_per_ray(D);
  if (need <= r.wf_bytes) return RT_OK;
  HIPCHECK(hipEventSynchronize((hipEvent_t)r.ev));
  const size_t want = std::max(std::max(need, 2 * r.wf_bytes), (size_t)4096 * wf_bytes_per_ray(2));
  if (r.d_wf) (void)hipFree(r.d_wf);
  r.d_wf = nullptr;
  r.wf_bytes = 0;
  if (hipMalloc(&r.d_wf, want) != hipSuccess) {
    (void)hipGetLastError();
    set_error("trace: device allocation failed");
    return RT_ERR_NOMEM;
  }
  r.wf_bytes = want;
  return RT_OK;
}

// RT_RAYS_WAVEFRONT: the stage kernels of every level, the regroups between them, the resolve pass -- all on st,
// launched for the upper bound n (the live counts stay on the device)
int enqueue_wavefront(rt_scene* s, int flags, RayParams R, FrameParams& P, hipStream_t st, int lsrc) {
  const int n = R.n, D = P.max_depth;
  const bool stats = (flags & RT_RAYS_STATS) != 0, reorder = (flags & RT_RAYS_REORDER) != 0;
  const bool sorting = reorder && n > 64;  // up to 64 rays are one packet in any order
  const bool fused = !(P.shadows && P.n_lights > 0);  // no traversal in the shading
  size_t tmp_sel = 0, tmp_sort = 0;
  HIPCHECK(hipcub::DeviceSelect::Flagged(nullptr, tmp_sel, (const uint32_t*)nullptr, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         (uint32_t*)nullptr, n, st));
  HIPCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_sort, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                              (const uint32_t*)nullptr, (uint32_t*)nullptr, n, 0, 32, st));
  // every growth first, so that nothing is freed under work this call has enqueued
  int rc = ensure_scratch(s, sorting ? (size_t)n : 0, std::max(tmp_sel, tmp_sort));
  if (rc) return rc;
  if ((rc = ensure_wavefront(s, (size_t)n, D))) return rc;
  rt_scene::RayScratch& r = s->rays;
  if (r.last_stream && r.last_stream != (void*)st) HIPCHECK(hipStreamWaitEvent(st, (hipEvent_t)r.ev, 0));
  // level 0's order is the plain RT_RAYS_REORDER call's, kept for rt_debug_ray_order
  if (reorder && (rc = begin_reorder(s, R, st))) return rc;
  if (stats && (rc = begin_stats(s, P, st))) return rc;
  hipLaunchKernelGGL(k_wf_counts, dim3(1), dim3(64), 0, st, r.d_counts, (uint32_t)n);
  HIPCHECK(hipGetLastError());
  r.last_levels = D;
  WfParams W{};
  W.s = wf_view(r.d_wf, (size_t)n, D);
  W.counts = r.d_counts;
  W.bounds = sorting ? (const float*)scratch_view(r).bounds : nullptr;
  W.n = n, W.D = D;
  W.origin_major = (kernel_variant() & VB_RAYKEY_ORIGIN_MAJOR) ? 1 : 0;
  const dim3 grid((unsigned)((n + 255) / 256)), block(256);
  // the entries `in` marked by the last stage (W.s.key_a: keys or flags) -> the other list
  auto regroup = [&](const uint32_t*& in) -> int {
    uint32_t* out = in == W.s.list_b ? W.s.list_a : W.s.list_b;
    size_t tb = r.tmp_bytes;
    if (sorting) {  // stable: equal keys keep the order of `in`
      HIPCHECK(hipcub::DeviceRadixSort::SortPairs(r.d_tmp, tb, (const uint32_t*)W.s.key_a, W.s.key_b, in, out, n, 0, 32, st));
    } else if (in) {
      HIPCHECK(hipcub::DeviceSelect::Flagged(r.d_tmp, tb, in, (const uint32_t*)W.s.key_a, out, r.d_counts + RT_MAX_TRACE_DEPTH + 1, n, st));
    } else {
      HIPCHECK(hipcub::DeviceSelect::Flagged(r.d_tmp, tb, hipcub::CountingInputIterator<uint32_t>(0u), (const uint32_t*)W.s.key_a, out,
                                             r.d_counts + RT_MAX_TRACE_DEPTH + 1, n, st));
    }
    in = out;
    return RT_OK;
  };
  const uint32_t* in = R.perm;  // level 0: the list as given, or its coherence order
  for (int d = 0; d < D; d++) {
    const bool last = d + 1 == D;
    W.level = d;
    W.ro = d ? W.s.o : R.o;
    W.rd = d ? W.s.d : R.d;
    W.list = in;
    if (fused) {
      W.mark = last ? nullptr : W.s.key_a;
      if (lsrc != LS_KERNARG)
        with_bools([&](auto FI, auto ST) { hipLaunchKernelGGL((k_wf_closest<FI.value, true, ST.value, LS_MEMORY>), grid, block, 0, st, P, W); }, d == 0, stats);
      else
        with_bools([&](auto FI, auto ST) { hipLaunchKernelGGL((k_wf_closest<FI.value, true, ST.value>), grid, block, 0, st, P, W); }, d == 0, stats);
      HIPCHECK(hipGetLastError());
      if (!last && (rc = regroup(in))) return rc;
      continue;
    }
    W.mark = W.s.key_a;
    if (lsrc != LS_KERNARG)
      with_bools([&](auto FI, auto ST) { hipLaunchKernelGGL((k_wf_closest<FI.value, false, ST.value, LS_MEMORY>), grid, block, 0, st, P, W); }, d == 0, stats);
    else
      with_bools([&](auto FI, auto ST) { hipLaunchKernelGGL((k_wf_closest<FI.value, false, ST.value>), grid, block, 0, st, P, W); }, d == 0, stats);
    HIPCHECK(hipGetLastError());
    if ((rc = regroup(in))) return rc;  // the hits, for the shade stage
    W.list = in;
    W.mark = (sorting && !last) ? W.s.key_a : nullptr;  // without a sort the hit list is the next level's list
    with_light_source(lsrc, [&](auto LS) {
      with_bools([&](auto ST) { hipLaunchKernelGGL((k_wf_shade<ST.value, decltype(LS)::value>), grid, block, 0, st, P, W); }, stats);
    });
    HIPCHECK(hipGetLastError());
    if (W.mark && (rc = regroup(in))) return rc;
  }
  hipLaunchKernelGGL(k_wf_resolve, grid, block, 0, st, P, W, R.rgb, R.face, R.t);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipEventRecord((hipEvent_t)r.ev, st));
  r.last_stream = (void*)st;
  return RT_OK;
}

}  // namespace

// A pointer the kernels may dereference: device or managed memory of the scene's device (shared with rt_views.hip)
int check_device_pointer(const rt_scene* s, const void* p, const char* who, const char* what) {
  if (!p) return RT_OK;
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    set_error("%s: %s is not device memory", who, what);
    return RT_ERR_INVALID;
  }
  if (a.type != hipMemoryTypeDevice && a.type != hipMemoryTypeManaged) {
    set_error("%s: %s is not device memory", who, what);
    return RT_ERR_INVALID;
  }
  if (a.type == hipMemoryTypeDevice && a.device != s->device) {
    set_error("%s: %s is memory of device %d, the scene is on device %d", who, what, a.device, s->device);
    return RT_ERR_INVALID;
  }
  return RT_OK;
}

namespace {

int check_lights(const rt_light* lights, int32_t n_lights) {
  return (n_lights < 0 || n_lights > RT_MAX_LIGHTS || (n_lights && !lights)) ? RT_ERR_INVALID : RT_OK;
}

// ray-list queries from host memory: closest (face, t, P, optional interpolated normal), any-hit (blocked) or
// colour -- upload, the stream path on the scene's stream, download
int trace_rays(rt_scene* s, int query, int32_t n, const float* o, const float* d, int32_t* face, float* t, float* P3,
               float* N3, int32_t* blocked, float* rgb, const rt_light* lights, int32_t n_lights) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (n < 0 || (n && (!o || !d)) || check_lights(lights, n_lights)) {
    set_error("trace: invalid arguments");
    return RT_ERR_INVALID;
  }
  if (n == 0) return RT_OK;
  const size_t n3 = (size_t)n * 12;
  hipStream_t st = (hipStream_t)s->stream;
  std::vector<void*> bufs;
  struct Free {
    std::vector<void*>& b;
    ~Free() { for (void* p : b) (void)hipFree(p); }
  } free_{bufs};
  auto dalloc = [&](size_t bytes) -> void* {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    bufs.push_back(p);
    return p;
  };
  RayParams R{};
  R.n = n;
  float* d_o = (float*)dalloc(n3);
  float* d_d = (float*)dalloc(n3);
  if (!d_o || !d_d) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
  HIPCHECK(hipMemcpy(d_o, o, n3, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_d, d, n3, hipMemcpyHostToDevice));
  R.o = d_o;
  R.d = d_d;
  if (query == Q_SHADOW) {
    if (!(R.blocked = (int32_t*)dalloc((size_t)n * 4))) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
  } else {
    R.face = (int32_t*)dalloc((size_t)n * 4);
    R.t = (float*)dalloc((size_t)n * 4);
    if (!R.face || !R.t) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
    if (query == Q_CLOSEST && P3 && !(R.P = (float*)dalloc(n3))) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
    if (query == Q_CLOSEST && N3 && !(R.N = (float*)dalloc(n3))) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
    if (query == Q_COLOR && !(R.rgb = (float*)dalloc(n3))) { set_error("trace: device allocation failed"); return RT_ERR_NOMEM; }
  }
  if ((rc = enqueue_rays(s, query, 0, R, lights, n_lights, st))) return rc;
  HIPCHECK(hipStreamSynchronize(st));
  if ((rc = check_prefetch_word(s))) return rc;
  if (query == Q_SHADOW) {
    HIPCHECK(hipMemcpy(blocked, R.blocked, (size_t)n * 4, hipMemcpyDeviceToHost));
  } else {
    if (face) HIPCHECK(hipMemcpy(face, R.face, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (t) HIPCHECK(hipMemcpy(t, R.t, (size_t)n * 4, hipMemcpyDeviceToHost));
    if (R.P) HIPCHECK(hipMemcpy(P3, R.P, n3, hipMemcpyDeviceToHost));
    if (R.N) HIPCHECK(hipMemcpy(N3, R.N, n3, hipMemcpyDeviceToHost));
    if (R.rgb) HIPCHECK(hipMemcpy(rgb, R.rgb, n3, hipMemcpyDeviceToHost));
  }
  return RT_OK;
}

}  // namespace
}  // namespace rt

using namespace rt;

extern "C" int rt_trace_closest(rt_scene* s, int32_t n, const float* o, const float* d, int32_t* face, float* t,
                                float* P3) {
  return trace_rays(s, Q_CLOSEST, n, o, d, face, t, P3, nullptr, nullptr, nullptr, nullptr, 0);
}

extern "C" int rt_trace_closest_normal(rt_scene* s, int32_t n, const float* o, const float* d, int32_t* face, float* t,
                                       float* P3, float* N3) {
  return trace_rays(s, Q_CLOSEST, n, o, d, face, t, P3, N3, nullptr, nullptr, nullptr, 0);
}

extern "C" int rt_trace_shadow(rt_scene* s, int32_t n, const float* P3, const float* L3, int32_t* blocked) {
  if (!blocked && n > 0) { set_error("rt_trace_shadow: null output"); return RT_ERR_INVALID; }
  return trace_rays(s, Q_SHADOW, n, P3, L3, nullptr, nullptr, nullptr, nullptr, blocked, nullptr, nullptr, 0);
}

extern "C" int rt_trace_color(rt_scene* s, int32_t n, const float* o, const float* d, const rt_light* lights,
                              int32_t n_lights, float* rgb, int32_t* face, float* t) {
  if (!rgb && n > 0) { set_error("rt_trace_color: null output"); return RT_ERR_INVALID; }
  return trace_rays(s, Q_COLOR, n, o, d, face, t, nullptr, nullptr, nullptr, rgb, lights, n_lights);
}

extern "C" int rt_trace_stream(rt_scene* s, int32_t query, int32_t flags, const rt_ray_stream* rays, const rt_light* lights,
                               int32_t n_lights, void* hip_stream) {
  // argument checks that need no device come first, so they read the same on every machine
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  if (query != RT_RAYS_CLOSEST && query != RT_RAYS_SHADOW && query != RT_RAYS_COLOR) {
    set_error("rt_trace_stream: bad query %d", query);
    return RT_ERR_INVALID;
  }
  if (flags & ~(RT_RAYS_REORDER | RT_RAYS_STATS)) { set_error("rt_trace_stream: bad flags %d", flags); return RT_ERR_INVALID; }
  if (!rays || rays->n < 0) { set_error("rt_trace_stream: invalid arguments"); return RT_ERR_INVALID; }
  const int32_t n = rays->n;
  if (n > 0) {
    if (!rays->a3 || !rays->b3 || (query == RT_RAYS_COLOR && check_lights(lights, n_lights))) {
      set_error("rt_trace_stream: invalid arguments");
      return RT_ERR_INVALID;
    }
    if (query == RT_RAYS_CLOSEST && (!rays->face || !rays->t)) { set_error("rt_trace_stream: RT_RAYS_CLOSEST needs face and t"); return RT_ERR_INVALID; }
    if (query == RT_RAYS_SHADOW && !rays->blocked) { set_error("rt_trace_stream: RT_RAYS_SHADOW needs blocked"); return RT_ERR_INVALID; }
    if (query == RT_RAYS_COLOR && !rays->rgb3) { set_error("rt_trace_stream: RT_RAYS_COLOR needs rgb3"); return RT_ERR_INVALID; }
  }
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (n == 0) return RT_OK;
  RayParams R{};
  R.n = n;
  R.o = rays->a3;
  R.d = rays->b3;
  if (query == RT_RAYS_SHADOW) {
    R.blocked = rays->blocked;
  } else {
    R.face = rays->face;
    R.t = rays->t;
    if (query == RT_RAYS_CLOSEST) R.P = rays->P3, R.N = rays->N3;
    else R.rgb = rays->rgb3;
  }
  const struct { const void* p; const char* what; } ptrs[] = {
      {R.o, "a3"}, {R.d, "b3"}, {R.face, "face"}, {R.t, "t"}, {R.P, "P3"}, {R.N, "N3"}, {R.blocked, "blocked"}, {R.rgb, "rgb3"}};
  for (const auto& q : ptrs)
    if ((rc = check_device_pointer(s, q.p, "rt_trace_stream", q.what))) return rc;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  if ((rc = enqueue_rays(s, query, flags, R, lights, query == RT_RAYS_COLOR ? n_lights : 0, st))) return rc;
  if (hip_stream) return note_list_use(s, st);
  HIPCHECK(hipStreamSynchronize(st));
  return check_prefetch_word(s);
}

// rt_trace_stream_color (lights / n_lights from host memory, ls null) and rt_trace_stream_lit (the light set ls)
static int trace_stream_color(const char* who, rt_scene* s, int32_t flags, const rt_ray_stream* rays, const rt_light* lights,
                              int32_t n_lights, const rt_light_set* ls, int32_t mode, int32_t max_depth, void* hip_stream) {
  // argument checks that need no device come first
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  if (mode != RT_MODE_PRIMARY && mode != RT_MODE_FULL) { set_error("%s: bad mode %d", who, mode); return RT_ERR_INVALID; }
  if (max_depth < 0 || max_depth > RT_MAX_TRACE_DEPTH) {
    set_error("%s: max_depth %d outside 0..%d", who, max_depth, RT_MAX_TRACE_DEPTH);
    return RT_ERR_INVALID;
  }
  if (flags & ~(RT_RAYS_REORDER | RT_RAYS_STATS | RT_RAYS_WAVEFRONT)) {
    set_error("%s: bad flags %d", who, flags);
    return RT_ERR_INVALID;
  }
  if (!rays || rays->n < 0) { set_error("%s: invalid arguments", who); return RT_ERR_INVALID; }
  const int32_t n = rays->n;
  if (n > 0) {
    if (!rays->a3 || !rays->b3 || check_lights(lights, n_lights)) { set_error("%s: invalid arguments", who); return RT_ERR_INVALID; }
    if (!rays->rgb3) { set_error("%s: needs rgb3", who); return RT_ERR_INVALID; }
  }
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (n == 0) return RT_OK;
  RayParams R{};
  R.n = n;
  R.o = rays->a3, R.d = rays->b3;
  R.face = rays->face, R.t = rays->t, R.rgb = rays->rgb3;
  const struct { const void* p; const char* what; } ptrs[] = {{R.o, "a3"}, {R.d, "b3"}, {R.face, "face"}, {R.t, "t"}, {R.rgb, "rgb3"}};
  for (const auto& q : ptrs)
    if ((rc = check_device_pointer(s, q.p, who, q.what))) return rc;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  const int depth = max_depth > 0 ? max_depth : (mode == RT_MODE_FULL ? 2 : 1);
  const bool wavefront = (flags & RT_RAYS_WAVEFRONT) != 0;
  // a light set: in the kernel arguments when it fits (then exactly the lights / n_lights call), else devices[0]'s
  // copy in device memory, which only the generic list kernels read
  FrameParams P;
  fill_scene_params(s, P);
  int lsrc = LS_KERNARG;
  if (ls) lsrc = fill_light_set(P, ls, 0);
  else fill_lights(P, lights, n_lights);
  if (mode == RT_MODE_FULL && depth == 2 && !wavefront && lsrc == LS_KERNARG) {  // the existing RT_RAYS_COLOR path, same kernel
    rc = ls ? enqueue_rays(s, Q_COLOR, flags, R, ls->host.data(), (int32_t)ls->host.size(), st)
            : enqueue_rays(s, Q_COLOR, flags, R, lights, n_lights, st);
  } else {
    P.mode = mode, P.max_depth = depth, P.shadows = mode == RT_MODE_FULL ? 1 : 0;
    if (pick_trav(kernel_variant(), P.sc.n_nodes4 > 0) == TRAV_W4) {
      set_error("%s: only the binary-tree kernels trace this mode / depth / flag, not kernel variant %d", who, kernel_variant());
      return RT_ERR_UNSUPPORTED;
    }
    rc = wavefront ? enqueue_wavefront(s, flags, R, P, st, lsrc) : enqueue_rays_depth(s, flags, R, P, st, lsrc);
  }
  if (rc) return rc;
  if (hip_stream) return note_list_use(s, st);
  HIPCHECK(hipStreamSynchronize(st));
  return check_prefetch_word(s);
}

extern "C" int rt_trace_stream_color(rt_scene* s, int32_t flags, const rt_ray_stream* rays, const rt_light* lights,
                                     int32_t n_lights, int32_t mode, int32_t max_depth, void* hip_stream) {
  return trace_stream_color("rt_trace_stream_color", s, flags, rays, lights, n_lights, nullptr, mode, max_depth, hip_stream);
}

extern "C" int rt_trace_stream_lit(rt_scene* s, int32_t flags, const rt_ray_stream* rays, const rt_light_set* ls, int32_t mode,
                                   int32_t max_depth, void* hip_stream) {
  if (s && !ls) { set_error("rt_trace_stream_lit: null light set"); return RT_ERR_INVALID; }
  if (s && ls->scene != s) { set_error("rt_trace_stream_lit: the light set belongs to another scene"); return RT_ERR_INVALID; }
  return trace_stream_color("rt_trace_stream_lit", s, flags, rays, nullptr, 0, ls, mode, max_depth, hip_stream);
}

extern "C" int rt_debug_ray_levels(rt_scene* s, int32_t capacity, int64_t* out2, int32_t* n_levels) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  const rt_scene::RayScratch& r = s->rays;
  if (r.last_levels < 0) { set_error("rt_debug_ray_levels: no RT_RAYS_WAVEFRONT call yet"); return RT_ERR_INVALID; }
  if (n_levels) *n_levels = r.last_levels;
  if (!out2) return RT_OK;
  if (capacity < r.last_levels) { set_error("rt_debug_ray_levels: buffer too small"); return RT_ERR_INVALID; }
  HIPCHECK(hipEventSynchronize((hipEvent_t)r.ev));
  uint32_t c[RT_MAX_TRACE_DEPTH + 1];
  HIPCHECK(hipMemcpy(c, r.d_counts, sizeof(c), hipMemcpyDeviceToHost));
  for (int d = 0; d < r.last_levels; d++) out2[2 * d] = c[d], out2[2 * d + 1] = c[d + 1];
  return RT_OK;
}

extern "C" int rt_rays_camera(rt_scene* s, const rt_camera* cam, int32_t width, int32_t height, float* origins3_device,
                              float* dirs3_device, void* hip_stream) {
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  if (!cam || width <= 0 || height <= 0 || (int64_t)width * height > INT32_MAX || !origins3_device || !dirs3_device) {
    set_error("rt_rays_camera: invalid arguments");
    return RT_ERR_INVALID;
  }
  int rc = check_device_scene(s);
  if (rc) return rc;
  if ((rc = check_device_pointer(s, origins3_device, "rt_rays_camera", "origins3_device"))) return rc;
  if ((rc = check_device_pointer(s, dirs3_device, "rt_rays_camera", "dirs3_device"))) return rc;
  FrameParams P;
  fill_scene_params(s, P);
  fill_camera_lights(P, cam, nullptr, 0);  // the frame path's camera parameters
  P.W = width, P.H = height;
  hipStream_t st = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)s->stream;
  const size_t n = (size_t)width * height;
  hipLaunchKernelGGL(k_camera_rays, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, P, origins3_device, dirs3_device);
  HIPCHECK(hipGetLastError());
  if (hip_stream) return RT_OK;
  HIPCHECK(hipStreamSynchronize(st));
  return RT_OK;
}

extern "C" int rt_debug_ray_order(rt_scene* s, int64_t capacity, uint32_t* perm_out, int64_t* n_out) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  const rt_scene::RayScratch& r = s->rays;
  if (r.last_n < 0) { set_error("rt_debug_ray_order: no RT_RAYS_REORDER call yet"); return RT_ERR_INVALID; }
  if (n_out) *n_out = r.last_n;
  if (!perm_out) return RT_OK;
  if (capacity < r.last_n) { set_error("rt_debug_ray_order: buffer too small"); return RT_ERR_INVALID; }
  if (!r.last_sorted) {
    for (int64_t i = 0; i < r.last_n; i++) perm_out[i] = (uint32_t)i;
    return RT_OK;
  }
  HIPCHECK(hipEventSynchronize((hipEvent_t)r.ev));
  HIPCHECK(hipMemcpy(perm_out, r.d_buf + 3 * r.capacity, (size_t)r.last_n * 4, hipMemcpyDeviceToHost));
  return RT_OK;
}
