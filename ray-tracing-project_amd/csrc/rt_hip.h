// rt_hip.h -- the host-side HIP glue every .hip source shares: the checked call, runtime values as template
// arguments for the launch sites, and the GPU builders' scratch (rt_build.hip, rt_boxes.hip). Host code only: no
// __device__ function and no kernel lives here, so a source that launches nothing of the traversal (rt_device.hip,
// rt_multi.hip, rt_lights.hip, rt_download.hip, rt_refit.hip, the builders) includes this and none of the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "rt_scene.h"

#define HIPCHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess) {                                                              \
      rt::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return RT_ERR_HIP;                                                                 \
    }                                                                                    \
  } while (0)

namespace rt {

// Runtime bools as template arguments: with_bools(f, a, b) calls f(std::bool_constant<a>{}, std::bool_constant<b>{}),
// so one generic lambda per kernel picks its <STATS, HITS, ...> instantiation.
template <class F>
void with_bools(F&& f) { f(); }
template <class F, class... Bools>
void with_bools(F&& f, bool b, Bools... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// A runtime LightSource as a template argument: f(std::integral_constant<int, LS_...>{}), around with_bools or
// inside it, so one generic lambda picks a kernel's LSRC instantiation too.
template <class F>
void with_light_source(int ls, F&& f) {
  if (ls == LS_MEMORY_CACHED) f(std::integral_constant<int, LS_MEMORY_CACHED>{});
  else if (ls == LS_MEMORY) f(std::integral_constant<int, LS_MEMORY>{});
  else f(std::integral_constant<int, LS_KERNARG>{});
}

// The scratch of one GPU build (gpu_build_lbvh / _ploc / _sah, gpu_build_ref_boxes) on the build stream of its
// device (build_stream): the buffers it allocates and its timing event pair, released on every return path --
// the stream drained first (a kernel may still use the buffers), then the buffers, then the events.
struct BuildScratch {
  hipStream_t st;
  std::vector<void*> bufs;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  explicit BuildScratch(hipStream_t s) : st(s) {}
  BuildScratch(const BuildScratch&) = delete;
  BuildScratch& operator=(const BuildScratch&) = delete;
  ~BuildScratch() {
    (void)hipStreamSynchronize(st);
    for (void* b : bufs) (void)hipFree(b);
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
  template <class T>
  hipError_t alloc(T*& p, size_t bytes) {  // at least 16 B, so that an empty array still has an address
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(bytes, 16));
    if (e == hipSuccess) bufs.push_back((void*)p);
    return e;
  }
  // the timed span: make_timer() once, start() / stop() around the span on st, elapsed_ms() after st has drained
  hipError_t make_timer() {
    hipError_t e = hipEventCreate(&e0);
    return e != hipSuccess ? e : hipEventCreate(&e1);
  }
  hipError_t start() { return hipEventRecord(e0, st); }
  hipError_t stop() { return hipEventRecord(e1, st); }
  hipError_t elapsed_ms(double* out) {
    float ms = 0.0f;
    hipError_t e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess && out) *out = ms;
    return e;
  }
};

// Morton quantisation of the tree builders: 1024 cells per axis of the scene box [lo, hi]; 0 on a flat axis (every
// centroid then falls into cell 0 of it)
inline float3 morton_scale(const float lo[3], const float hi[3]) {
  float3 s;
  s.x = hi[0] > lo[0] ? 1024.0f / (hi[0] - lo[0]) : 0.0f;
  s.y = hi[1] > lo[1] ? 1024.0f / (hi[1] - lo[1]) : 0.0f;
  s.z = hi[2] > lo[2] ? 1024.0f / (hi[2] - lo[2]) : 0.0f;
  return s;
}

}  // namespace rt
