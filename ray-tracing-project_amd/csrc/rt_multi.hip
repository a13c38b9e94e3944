// rt_multi.hip -- multi-device scenes (rt_scene_opts.n_devices > 1) of the MI355X ray-traversal library: one frame
// over the scene's replicas. rt_render_async / rt_render_lit_async hand a single-device scene's frame to
// rt_frame.hip render_one and split a multi-device scene's over the replicas' enqueue workers;
// rt_synchronize(_devices) waits for every device and sums their stats.
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "rt_device.h"

using namespace rt;

// Enqueue workers of a multi-device scene. Queueing one device's share of a frame costs ~20 us of host time
// (frame parameters, three events, the launch); done for D devices one after the other on the caller's
// thread that is D x 20 us per frame, which at 8 devices exceeds a device's share of the frame. So each
// further replica has a host thread of its own: the caller posts the frame to every worker, queues replica 0
// itself, and returns once every worker has queued its share (so errors are reported by this call and the
// frames stay in call order on every device). A worker waits for work spinning for a while, then blocks.
namespace rt {
struct EnqueueWorker {
  std::thread th;
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<uint32_t> posted{0}, done{0};  // job sequence numbers
  bool quit = false;
  rt_scene* r = nullptr;
  rt_camera cam;
  rt_light lights[RT_MAX_LIGHTS];
  int32_t n_lights = 0;
  const rt_light_set* ls = nullptr;  // rt_render_lit: the frame's light set (then n_lights = 0), replica `rep`'s copy
  int rep = 0;
  rt_frame fr;
  int rc = RT_OK;
  std::string err;
};

static void worker_loop(EnqueueWorker* w) {
  uint32_t seen = 0;
  for (;;) {
    // spin ~50 us for the next frame (frames come at sub-millisecond cadence), then block
    for (int i = 0; i < 20000 && w->posted.load(std::memory_order_acquire) == seen; i++) __builtin_ia32_pause();
    if (w->posted.load(std::memory_order_acquire) == seen) {
      std::unique_lock<std::mutex> lk(w->mu);
      w->cv.wait(lk, [&] { return w->quit || w->posted.load(std::memory_order_acquire) != seen; });
    }
    {
      std::lock_guard<std::mutex> lk(w->mu);
      if (w->quit && w->posted.load(std::memory_order_acquire) == seen) return;
    }
    seen = w->posted.load(std::memory_order_acquire);
    w->rc = render_one(w->r, &w->cam, w->n_lights ? w->lights : nullptr, w->n_lights, &w->fr, w->ls, w->rep);
    if (w->rc) w->err = rt_last_error();
    w->done.store(seen, std::memory_order_release);
    { std::lock_guard<std::mutex> lk(w->mu); }
    w->cv.notify_all();
  }
}

void stop_workers(rt_scene* s) {
  for (auto& w : s->workers) {
    {
      std::lock_guard<std::mutex> lk(w->mu);
      w->quit = true;
    }
    w->cv.notify_all();
    if (w->th.joinable()) w->th.join();
  }
  s->workers.clear();
}

static int start_workers(rt_scene* s) {
  if (s->workers.size() == s->replicas.size()) return RT_OK;
  stop_workers(s);
  for (auto& r : s->replicas) {
    auto w = std::make_shared<EnqueueWorker>();
    w->r = r.get();
    w->rep = 1 + (int)s->workers.size();
    try {
      w->th = std::thread(worker_loop, w.get());
    } catch (const std::exception&) {
      stop_workers(s);  // no threads: the caller queues every device itself
      return RT_ERR_UNSUPPORTED;
    }
    s->workers.push_back(std::move(w));
  }
  return RT_OK;
}

}  // namespace rt

// The caller's frame (shard si of sc, normally the whole frame) goes to the D replicas as shards of an
// sc*D-way split: replica k renders shard si + sc*k, so the D shards together are exactly the caller's
// shard (super-tile t: t % (sc*D) = si + sc*k  <=>  t % sc = si). Each replica renders on its own slot
// streams, its launches queued by its own worker thread (replica 0's by the caller); nothing is exchanged
// between devices.
static int render_multi(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* fr,
                        const rt_light_set* ls = nullptr) {
  if (ls) lights = nullptr, n_lights = 0;  // every replica reads its own copy of the set
  if (!fr || !cam || n_lights < 0 || n_lights > RT_MAX_LIGHTS || (n_lights && !lights)) {
    set_error("rt_render: invalid arguments");
    return RT_ERR_INVALID;
  }
  const int D = n_replicas(s);
  const int sc = fr->shard_count > 0 ? fr->shard_count : 1, si = fr->shard_index;
  if (si < 0 || si >= sc) { set_error("rt_render: shard %d of %d", si, sc); return RT_ERR_INVALID; }
  if ((int64_t)sc * D > (1 << 24)) { set_error("rt_render: %d shards x %d devices", sc, D); return RT_ERR_INVALID; }
  auto shard_of = [&](int k) {
    rt_frame f = *fr;
    f.shard_count = sc * D;
    f.shard_index = si + sc * k;
    return f;
  };
  // the reference's default box colours (setRandomColor draws) reach every replica here, on the caller's
  // thread, before any worker reads its replica's colours
  if (fr->mode == RT_MODE_BOX_COLORS)  // (the object-space vertices every replica's colour pass reads)
    if (const int rc = host_mirror_geometry(s)) return rc;
  if (fr->mode == RT_MODE_BOX_COLORS && s->box_colors.size() != 3 * s->hs.boxes.size()) {
    const int rc = rt_scene_set_box_colors(s, nullptr);
    if (rc) return rc;
  }
  if (start_workers(s) != RT_OK) {  // (no helper threads: queue every device from this thread)
    for (int k = 0; k < D; k++) {
      const rt_frame f = shard_of(k);
      const int rc = render_one(replica(s, k), cam, lights, n_lights, &f, ls, k);
      if (rc) return rc;
    }
    HIPCHECK(hipSetDevice(s->device));
    return RT_OK;
  }
  std::vector<uint32_t> seq(s->workers.size());
  for (size_t k = 0; k < s->workers.size(); k++) {
    EnqueueWorker& w = *s->workers[k];
    {
      std::lock_guard<std::mutex> lk(w.mu);
      w.cam = *cam;
      w.n_lights = n_lights;
      w.ls = ls;
      if (n_lights) memcpy(w.lights, lights, sizeof(rt_light) * (size_t)n_lights);
      w.fr = shard_of((int)k + 1);
      seq[k] = w.posted.load(std::memory_order_relaxed) + 1;
      w.posted.store(seq[k], std::memory_order_release);
    }
    w.cv.notify_all();
  }
  const rt_frame f0 = shard_of(0);
  int rc = render_one(s, cam, lights, n_lights, &f0, ls, 0);
  std::string err0 = rc ? rt_last_error() : "";
  for (size_t k = 0; k < s->workers.size(); k++) {  // every worker has queued its share before this returns
    EnqueueWorker& w = *s->workers[k];
    for (int i = 0; i < 200000 && w.done.load(std::memory_order_acquire) != seq[k]; i++) __builtin_ia32_pause();
    if (w.done.load(std::memory_order_acquire) != seq[k]) {
      std::unique_lock<std::mutex> lk(w.mu);
      w.cv.wait(lk, [&] { return w.done.load(std::memory_order_acquire) == seq[k]; });
    }
    if (w.rc && rc == RT_OK) {
      rc = w.rc;
      err0 = "device " + std::to_string(w.r->device) + ": " + w.err;
    }
  }
  if (rc) {
    set_error("%s", err0.c_str());
    return rc;
  }
  HIPCHECK(hipSetDevice(s->device));
  return RT_OK;
}

extern "C" int rt_render_async(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights,
                               const rt_frame* fr) {
  if (s && !s->replicas.empty()) return render_multi(s, cam, lights, n_lights, fr);
  return render_one(s, cam, lights, n_lights, fr);
}

extern "C" int rt_render_lit_async(rt_scene* s, const rt_camera* cam, const rt_light_set* ls, const rt_frame* fr) {
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  if (!ls) { set_error("rt_render_lit: null light set"); return RT_ERR_INVALID; }
  if (ls->scene != s) { set_error("rt_render_lit: the light set belongs to another scene"); return RT_ERR_INVALID; }
  if (!s->replicas.empty()) return render_multi(s, cam, nullptr, 0, fr, ls);
  return render_one(s, cam, nullptr, 0, fr, ls, 0);
}

extern "C" int rt_synchronize_devices(rt_scene* s, rt_stats* out, int32_t capacity, rt_stats* per_device) {
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  const int D = n_replicas(s);
  rt_stats tot;
  memset(&tot, 0, sizeof tot);
  int first_rc = RT_OK;
  for (int k = 0; k < D; k++) {  // every device is drained, even after a failure on one of them
    rt_stats st;
    const int rc = sync_one(replica(s, k), &st);
    if (rc) {
      if (first_rc == RT_OK) first_rc = rc;
      continue;
    }
    if (per_device && k < capacity) per_device[k] = st;
    tot.kernel_ms = std::max(tot.kernel_ms, st.kernel_ms);
    tot.trace_kernel_ms = std::max(tot.trace_kernel_ms, st.trace_kernel_ms);
    tot.launches = std::max(tot.launches, st.launches);
    tot.primary_rays += st.primary_rays;
    tot.total_rays += st.total_rays;
    tot.hits += st.hits;
    tot.node_visits += st.node_visits;
    tot.tri_tests += st.tri_tests;
    tot.wave_node_fetches += st.wave_node_fetches;
    tot.wave_tri_fetches += st.wave_tri_fetches;
    tot.wave_node_bytes += st.wave_node_bytes;
  }
  if (D > 1 && s->device != RT_DEVICE_NONE) (void)hipSetDevice(s->device);
  if (first_rc) return first_rc;
  if (out) *out = tot;
  return D;
}

extern "C" int rt_synchronize(rt_scene* s, rt_stats* out) {
  const int rc = rt_synchronize_devices(s, out, 0, nullptr);
  return rc < 0 ? rc : RT_OK;
}
