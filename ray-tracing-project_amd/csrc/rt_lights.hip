// rt_lights.hip -- the lights of a frame or ray list of the MI355X ray-traversal library: the kernel-argument
// lights in calculateColor's order (fill_lights), and light sets (rt_api.h RT_HAS_LIGHT_SETS): their host and
// per-device copies, and which path a set takes (fill_light_set).
#include <algorithm>
#include <memory>
#include <vector>

#include "rt_device.h"

using namespace rt;

void rt::free_light_set(rt_light_set* ls) {
  rt_scene* s = ls->scene;
  for (size_t k = 0; k < ls->dev.size(); k++) {
    if (!ls->dev[k]) continue;
    const rt_scene* r = k == 0 ? s : s->replicas[k - 1].get();
    (void)hipSetDevice(r->device);
    (void)hipFree(ls->dev[k]);
  }
  if (!ls->dev.empty() && s->device != RT_DEVICE_NONE) (void)hipSetDevice(s->device);
  delete ls;
}

// calculateColor's order: point lights first, then directional lights (each in array order)
void rt::fill_lights(FrameParams& P, const rt_light* lights, int32_t n_lights) {
  P.n_lights = n_lights;
  int k = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int l = 0; l < n_lights; l++) {
      const int kind = lights[l].kind == RT_LIGHT_DIRECTIONAL ? RT_LIGHT_DIRECTIONAL : RT_LIGHT_POINT;
      if (kind != (pass ? RT_LIGHT_DIRECTIONAL : RT_LIGHT_POINT)) continue;
      memcpy(P.lights[k].p, lights[l].position, 12);
      memcpy(P.lights[k].c, lights[l].color, 12);
      P.lights[k].kind = kind;
      k++;
    }
}

// A light set on the path the variant selects: at most RT_MAX_LIGHTS lights travel in the kernel arguments and take
// exactly rt_render's path (the host copy is already in calculateColor's order, which fill_lights keeps); more
// -- or any number but none under VB_MEM_LIGHTS -- are read from replica `rep`'s device array.
int rt::fill_light_set(FrameParams& P, const rt_light_set* ls, int rep) {
  const int32_t n = (int32_t)ls->host.size();
  const int v = kernel_variant();
  if (n <= RT_MAX_LIGHTS && !((v & VB_MEM_LIGHTS) && n > 0)) {
    fill_lights(P, ls->host.data(), n);
    return LS_KERNARG;
  }
  P.n_lights = n;
  P.light_set = ls->dev[(size_t)rep];
  return (v & VB_NO_OCCLUDER_CACHE) ? LS_MEMORY : LS_MEMORY_CACHED;
}

// ---- light sets (rt_api.h RT_HAS_LIGHT_SETS) ----

extern "C" int rt_light_set_create(rt_scene* s, const rt_light* lights, int32_t n_lights, rt_light_set** out) {
  if (out) *out = nullptr;
  if (!s || !out || n_lights < 0 || n_lights > RT_MAX_LIGHT_SET || (n_lights && !lights)) {
    set_error("rt_light_set_create: invalid arguments");
    return RT_ERR_INVALID;
  }
  std::unique_ptr<rt_light_set> ls(new rt_light_set);
  ls->scene = s;
  // calculateColor's order, as fill_lights: every point light, then every directional light
  ls->host.reserve((size_t)n_lights);
  for (int pass = 0; pass < 2; pass++)
    for (int32_t l = 0; l < n_lights; l++) {
      const int kind = lights[l].kind == RT_LIGHT_DIRECTIONAL ? RT_LIGHT_DIRECTIONAL : RT_LIGHT_POINT;
      if (kind != (pass ? RT_LIGHT_DIRECTIONAL : RT_LIGHT_POINT)) continue;
      rt_light x = lights[l];
      x.kind = kind;
      ls->host.push_back(x);
    }
  if (s->device != RT_DEVICE_NONE) {
    std::vector<Light> dl((size_t)n_lights);
    for (int32_t l = 0; l < n_lights; l++) {
      memcpy(dl[(size_t)l].p, ls->host[(size_t)l].position, 12);
      memcpy(dl[(size_t)l].c, ls->host[(size_t)l].color, 12);
      dl[(size_t)l].kind = ls->host[(size_t)l].kind;
    }
    const size_t bytes = std::max<size_t>(dl.size(), 1) * sizeof(Light);
    const int D = n_replicas(s);
    ls->dev.assign((size_t)D, nullptr);
    int rc = RT_OK;
    for (int k = 0; k < D && rc == RT_OK; k++) {
      hipError_t e = hipSetDevice(replica(s, k)->device);
      if (e == hipSuccess) e = hipMalloc((void**)&ls->dev[(size_t)k], bytes);
      if (e != hipSuccess) {
        (void)hipGetLastError();
        ls->dev[(size_t)k] = nullptr;
        set_error("rt_light_set_create: device allocation failed (%s)", hipGetErrorString(e));
        rc = RT_ERR_NOMEM;
        break;
      }
      if (!dl.empty() && (e = hipMemcpy(ls->dev[(size_t)k], dl.data(), dl.size() * sizeof(Light), hipMemcpyHostToDevice)) != hipSuccess) {
        set_error("rt_light_set_create: upload failed (%s)", hipGetErrorString(e));
        rc = RT_ERR_HIP;
      }
    }
    (void)hipSetDevice(s->device);
    if (rc) {
      free_light_set(ls.release());
      return rc;
    }
  }
  s->light_sets.push_back(ls.get());
  *out = ls.release();
  return RT_OK;
}

extern "C" void rt_light_set_destroy(rt_light_set* ls) {
  if (!ls) return;
  rt_scene* s = ls->scene;
  if (!ls->dev.empty()) drain_replicas_quiet(s);  // frames in flight on the scene's own streams may still read the set
  s->light_sets.erase(std::remove(s->light_sets.begin(), s->light_sets.end(), ls), s->light_sets.end());
  free_light_set(ls);
}

extern "C" int rt_light_set_get(const rt_light_set* ls, int32_t capacity, rt_light* out, int32_t* n_out) {
  if (!ls) { set_error("rt_light_set_get: null set"); return RT_ERR_INVALID; }
  const int32_t n = (int32_t)ls->host.size();
  if (out && capacity < n) { set_error("rt_light_set_get: buffer too small (%d lights)", n); return RT_ERR_INVALID; }
  if (n_out) *n_out = n;
  if (out && n) memcpy(out, ls->host.data(), sizeof(rt_light) * (size_t)n);
  return RT_OK;
}
