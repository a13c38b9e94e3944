// rt_device.h -- what the device-layer sources share (rt_device.hip, rt_frame.hip, rt_multi.hip, rt_lights.hip,
// rt_download.hip, rt_rays.hip, rt_views.hip): each stage's entry points, the shard layout and its tile walk, and
// the small rules every stage repeats (drain a scene's slots, create an event at first use, regrow a slot's
// buffer). Private to those files: no host .cpp includes it (rt_scene.h carries what the host side needs).
#pragma once
#include <cstring>

#include "rt_dispatch.h"
#include "rt_hip.h"

namespace rt {

// ---- rt_device.hip: bring-up and teardown ----
int check_device_scene(rt_scene* s);  // RT_ERR_NO_DEVICE for a host-only scene; makes the scene's device current
// every frame slot's stream of this scene drained (its device is current): checked, or best effort on teardown;
// the last for every replica of a scene in turn (each made current)
int drain_slots(rt_scene* s);
void drain_slots_quiet(rt_scene* s);
void drain_replicas_quiet(rt_scene* s);

inline int ensure_event(void*& ev) {  // an untimed event, created at first use
  if (!ev) HIPCHECK(hipEventCreateWithFlags((hipEvent_t*)&ev, hipEventDisableTiming));
  return RT_OK;
}
// A buffer of one frame slot regrown to exactly `bytes` (capacity counts the caller's units): the slot's earlier
// work on st may still use the old one, so st drains before the free.
template <class T>
int regrow(T*& ptr, size_t& capacity, size_t want, size_t bytes, hipStream_t st) {
  HIPCHECK(hipStreamSynchronize(st));
  if (ptr) (void)hipFree(ptr);
  ptr = nullptr, capacity = 0;
  HIPCHECK(hipMalloc((void**)&ptr, bytes));
  capacity = want;
  return RT_OK;
}

// the reference boxes and the materials in their device form (device_upload, rt_scene_update)
inline std::vector<float> refbox_image(const HostScene& hs) {
  std::vector<float> rb(8 * hs.boxes.size());
  for (size_t b = 0; b < hs.boxes.size(); b++)
    for (int k = 0; k < 3; k++) { rb[8 * b + k] = hs.boxes[b].low[k]; rb[8 * b + 4 + k] = hs.boxes[b].high[k]; }
  return rb;
}
inline std::vector<DevMat> mats_image(const HostScene& hs) {
  std::vector<DevMat> dm(hs.mats.size());
  for (size_t m = 0; m < hs.mats.size(); m++) {
    DevMat& d = dm[m];
    memset(&d, 0, sizeof d);
    for (int k = 0; k < 3; k++) { d.ka[k] = hs.mats[m].ka[k]; d.kd[k] = hs.mats[m].kd[k]; d.ks[k] = hs.mats[m].ks[k]; }
    d.ns = hs.mats[m].shininess;
  }
  return dm;
}
// device 0's buffer to a replica's, queued on the replica's stream st (its device is current): over xGMI between
// GPUs with peer access, a plain device copy when both replicas share a GPU
inline int replica_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
  if (dst_dev == src_dev) HIPCHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
  else HIPCHECK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
  return RT_OK;
}

// ---- rt_frame.hip: one device's frame ----
void fill_scene_params(const rt_scene* s, FrameParams& P);  // clears P, then the scene's part of it
// camera and lights of a frame; P.Minv is set (fill_scene_params)
void fill_camera_lights(FrameParams& P, const rt_camera* cam, const rt_light* lights, int32_t n_lights);
int check_prefetch_word(rt_scene* s);  // RT_CHECK_PREFETCH debug build; RT_OK otherwise
int render_one(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* fr,
               const rt_light_set* ls = nullptr, int rep = 0);
int sync_one(rt_scene* s, rt_stats* out);  // waits for this device's frames; their times and counters

// ---- rt_lights.hip ----
void fill_lights(FrameParams& P, const rt_light* lights, int32_t n_lights);
int fill_light_set(FrameParams& P, const rt_light_set* ls, int rep);  // returns the LightSource the set takes
// frees a light set's device copies (dev[k] lives on replica k's device) and the set; the caller has drained the
// streams that may read it
void free_light_set(rt_light_set* ls);

// ---- rt_multi.hip: a scene's replicas (k = 0: the scene itself) ----
inline rt_scene* replica(rt_scene* s, int k) { return k == 0 ? s : s->replicas[(size_t)k - 1].get(); }
inline int n_replicas(const rt_scene* s) { return 1 + (int)s->replicas.size(); }
void stop_workers(rt_scene* s);

// ---- rt_download.hip ----
enum AsmKind { ASM_RGB = 0, ASM_FACE = 1, ASM_T = 2, ASM_RGB8 = 3 };
// the last frame of a multi-device scene, assembled from its replicas' tiles in the caller's buffer
int assemble(rt_scene* s, AsmKind kind, int64_t capacity_pixels, void* out, int32_t* exact, const char* what);

// ---- rt_rays.hip ----
// a pointer the kernels may dereference (device or managed memory of the scene's device; null passes)
int check_device_pointer(const rt_scene* s, const void* p, const char* who, const char* what);

// One shard of a W x H frame (rt_internal.h shard_tile_xy): its tile slots, and its packed form at bytes_per_pixel
// (256 pixels per slot, slot order) with the 8-bit frame's exactness flag in the 16 bytes behind it
struct ShardLayout {
  int W, H, tiles_x, tiles_y, index, count, S, slots;
  size_t bytes, flag_off;
};
inline ShardLayout shard_layout(int W, int H, int index, int count, size_t bytes_per_pixel) {
  ShardLayout l;
  l.W = W, l.H = H, l.tiles_x = (W + 15) / 16, l.tiles_y = (H + 15) / 16;
  l.index = index, l.count = count, l.S = frame_super_tile(count);
  l.slots = shard_tile_slots(l.tiles_x, l.tiles_y, l.S, index, count);
  l.bytes = (size_t)l.slots * 256 * bytes_per_pixel;
  l.flag_off = (l.bytes + 15) & ~(size_t)15;
  return l;
}
// f(L, tx, ty) for the shard's slots that lie inside the frame, in slot order (a super-tile may overhang it)
template <class F>
void for_each_shard_tile(const ShardLayout& l, F&& f) {
  for (int L = 0; L < l.slots; L++) {
    int tx, ty;
    shard_tile_xy(l.tiles_x, l.S, l.index, l.count, L, tx, ty);
    if (tx < l.tiles_x && ty < l.tiles_y) f(L, tx, ty);
  }
}

}  // namespace rt
