// rt_device.hip -- device bring-up and teardown of the MI355X ray-traversal library: the per-device build stream
// and pinned staging copies, the hardware-queue registry and the frame slots' streams, scene upload, replication to
// further devices and release. The frame path is rt_frame.hip (one device) and rt_multi.hip (a scene's replicas),
// light sets rt_lights.hip, frame download and assembly rt_download.hip, ray lists rt_rays.hip, view batches
// rt_views.hip; rt_device.h declares what they share.
#include <errno.h>
#include <fcntl.h>
#include <signal.h>
#include <sys/file.h>
#include <unistd.h>

#include <cctype>
#include <chrono>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "rt_device.h"
#include "rt_traverse.h"  // kStatSlots

namespace rt {

// Host -> device copy of scene data. Large copies from pageable host memory go through two pinned 8-MiB
// staging buffers on their own stream (host memcpy of one chunk overlaps the DMA of the other): a plain
// hipMemcpy from pageable memory measured ~1 GB/s for the scene upload (263 ms for the 1M soup's ~250 MB,
// BENCH_r03 build_ms.upload).
// One stream per device for scene construction (the builders' kernels, the staged copies): created on
// first use and kept for the process, so building scenes creates no HIP streams beyond it. Each stream a
// process creates is bound to one of the device's few hardware queues; transient build streams created
// before a scene's frame-slot streams changed which queues those landed on.
void* build_stream(int device) {
  static std::mutex mu;
  static hipStream_t st[64] = {};
  if (device < 0 || device >= 64) return nullptr;
  std::lock_guard<std::mutex> lock(mu);
  if (!st[device]) {
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&st[device], hipStreamNonBlocking) != hipSuccess)
      st[device] = nullptr;
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  return (void*)st[device];
}

// First use of the device in a process (its construction stream, a first allocation), run on a helper thread
// while rt_scene_create prepares the host arrays: measured ~0.14 s before the first builder's allocations
// on a fresh process (C3, RT_TIMING), which otherwise adds to the scene setup after the host preparation.
void device_warmup(int device) {
  PhaseTimer pt("warmup");
  if (device < 0 || hipSetDevice(device) != hipSuccess) return;
  pt.mark("set_device");
  (void)build_stream(device);
  pt.mark("stream");
  void* p = nullptr;
  if (hipMalloc(&p, 1u << 20) == hipSuccess) (void)hipFree(p);
  pt.mark("malloc");
}

// One pair of pinned 8-MiB staging buffers (+ their events) per device for the staged copies below, created
// at the device's first large copy and kept for the process beside its build stream (allocating
// and freeing pinned memory per copy can synchronise the device, stalling frames other scenes have in
// flight, and added to the setup time). Copies to one device serialise on its staging mutex.
struct Staging {
  std::mutex mu;
  void* buf[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
};
constexpr size_t kStageChunk = 8u << 20;
static int staging(int device, Staging** out) {
  static Staging st[64];
  if (device < 0 || device >= 64) { set_error("device %d out of range for staging", device); return RT_ERR_INVALID; }
  *out = &st[device];
  return RT_OK;
}
// (caller holds g.mu and has made `device` current)
static int staging_ready(Staging& g) {
  for (int k = 0; k < 2; k++) {
    if (!g.buf[k]) HIPCHECK(hipHostMalloc(&g.buf[k], kStageChunk, hipHostMallocDefault));
    if (!g.ev[k]) HIPCHECK(hipEventCreateWithFlags(&g.ev[k], hipEventDisableTiming));
  }
  return RT_OK;
}

int h2d(void* dst, const void* src, size_t bytes) {
  if (bytes < 2 * kStageChunk) {
    HIPCHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return RT_OK;
  }
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  Staging* gp = nullptr;
  int rc = staging(dev, &gp);
  if (rc) return rc;
  Staging& g = *gp;
  std::lock_guard<std::mutex> lock(g.mu);
  if ((rc = staging_ready(g))) return rc;
  hipStream_t st = (hipStream_t)build_stream(dev);
  if (!st) { set_error("no build stream on device %d", dev); return RT_ERR_HIP; }
  // on any return the stream drains first: the staging buffers are reused by the next copy
  struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
  bool used[2] = {false, false};
  int k = 0;
  for (size_t off = 0; off < bytes; off += kStageChunk, k ^= 1) {
    const size_t n = std::min(kStageChunk, bytes - off);
    if (used[k]) HIPCHECK(hipEventSynchronize(g.ev[k]));  // this staging buffer's previous DMA is done
    memcpy(g.buf[k], static_cast<const char*>(src) + off, n);
    HIPCHECK(hipMemcpyAsync(static_cast<char*>(dst) + off, g.buf[k], n, hipMemcpyHostToDevice, st));
    HIPCHECK(hipEventRecord(g.ev[k], st));
    used[k] = true;
  }
  HIPCHECK(hipStreamSynchronize(st));
  return RT_OK;
}

// Device -> host copy into pageable memory, the same way round: DMA into one pinned 8-MiB staging buffer
// while the host copies the other out (the device builders' read-backs).
int d2h(void* dst, const void* src, size_t bytes) {
  if (bytes < 2 * kStageChunk) {
    HIPCHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return RT_OK;
  }
  int dev = 0;
  HIPCHECK(hipGetDevice(&dev));
  Staging* gp = nullptr;
  int rc = staging(dev, &gp);
  if (rc) return rc;
  Staging& g = *gp;
  std::lock_guard<std::mutex> lock(g.mu);
  if ((rc = staging_ready(g))) return rc;
  hipStream_t st = (hipStream_t)build_stream(dev);
  if (!st) { set_error("no build stream on device %d", dev); return RT_ERR_HIP; }
  struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
  const size_t nchunks = (bytes + kStageChunk - 1) / kStageChunk;
  auto issue = [&](size_t c) -> int {
    const size_t off = c * kStageChunk, n = std::min(kStageChunk, bytes - off);
    HIPCHECK(hipMemcpyAsync(g.buf[c & 1], static_cast<const char*>(src) + off, n, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipEventRecord(g.ev[c & 1], st));
    return RT_OK;
  };
  if ((rc = issue(0))) return rc;
  for (size_t c = 0; c < nchunks; c++) {
    if (c + 1 < nchunks && (rc = issue(c + 1))) return rc;  // the next chunk's DMA overlaps this copy-out
    HIPCHECK(hipEventSynchronize(g.ev[c & 1]));
    const size_t off = c * kStageChunk, n = std::min(kStageChunk, bytes - off);
    memcpy(static_cast<char*>(dst) + off, g.buf[c & 1], n);
  }
  return RT_OK;
}

template <typename T>
static int dalloc_copy(T** dst, const void* src, size_t bytes, int64_t& total) {
  *dst = nullptr;
  if (bytes == 0) bytes = 16;
  HIPCHECK(hipMalloc((void**)dst, bytes));
  total += (int64_t)bytes;
  if (src) return h2d(*dst, src, bytes);
  return RT_OK;
}

static size_t alloc_bytes(size_t bytes) { return bytes == 0 ? 16 : bytes; }  // what dalloc_copy allocates

// The scene's device and its frame-slot streams (one per frame in flight). Each slot stream gets a hardware
// queue of its own: an ordinary HIP stream is bound to one of a small per-process pool of queues
// (GPU_MAX_HW_QUEUES, 4 on the boxes), shared with every other stream of the process in creation order, and two
// slots on one queue run their frames one after the other -- measured in a fresh process: C5 with 4 frames in
// flight 8.3 Grays/s with the slots on the pool (kernel ms per frame 0.49, two frames overlapping) against 12.3
// when the pool had been used by two other streams first, or with 8 queues per process
// (profiles/ab/r05_queue_probe.txt). A stream created with a CU mask is given a dedicated queue outside that
// pool, so the slots are created with the full mask (every CU: no restriction), whatever streams the process
// made before; a runtime that refuses falls back to an ordinary stream.
// At most kDedicatedSlotQueues such queues per device and process (two scenes' worth of slots): beyond that the
// device's queues are oversubscribed and the hardware time-slices them -- eight replicas of one scene on one GPU
// (32 dedicated queues) ran 2.3x slower than two (profiles/ab/r05_queue_probe.txt) -- so further slots take the
// pool. dedicated_slots counts the live dedicated queues per device (released by release_slot_stream).
// A deliberate exception to the per-process GPU_MAX_HW_QUEUES pool: it is what lets one process's
// frames in flight overlap (C5 with 4 frames in flight 11.9 against 8.6 Grays/s on the pool); RT_SLOT_POOL (A/B
// knob) puts every slot on the pool.
constexpr int kDedicatedSlotQueues = 8;
// Across the processes that share a GPU (the cap was counted per process only; four renderer processes
// on one GPU held 32 dedicated queues and ran 4.1x slower than with every slot on the pool, and a shared cap of 8
// queues still halved them -- profiles/ab/r06_slot_queues_ab.txt), only one process per GPU holds dedicated slot
// queues. A lock file per physical GPU (/tmp/rtamd_hwq_<PCI bus id>) lists "pid count" of the processes holding
// them; entries of processes that no longer exist are dropped, and the file is removed when no holder is left.
// Without the file (no /tmp, another user's file) a process keeps its own cap only.
static bool hwq_registry(int dev, int delta) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, (int)sizeof bus - 1, dev) != hipSuccess) { (void)hipGetLastError(); return delta < 0; }
  std::string path = "/tmp/rtamd_hwq_";
  for (const char* c = bus; *c; c++) path += (isalnum((unsigned char)*c) ? *c : '_');
  const int fd = open(path.c_str(), O_RDWR | O_CREAT, 0666);
  if (fd < 0) return delta < 0;
  struct Close { int fd; ~Close() { flock(fd, LOCK_UN); close(fd); } } close_{fd};
  if (flock(fd, LOCK_EX) != 0) return delta < 0;
  std::string text;
  char buf[4096];
  ssize_t n;
  while ((n = read(fd, buf, sizeof buf)) > 0) text.append(buf, (size_t)n);
  const long me = (long)getpid();
  long mine = 0, others = 0;
  std::string out;
  size_t pos = 0;
  while (pos < text.size()) {
    const size_t e = std::min(text.find('\n', pos), text.size());
    long pid = 0, cnt = 0;
    if (sscanf(text.c_str() + pos, "%ld %ld", &pid, &cnt) == 2 && pid > 0 && cnt > 0) {
      if (pid == me) mine = cnt;
      else if (kill((pid_t)pid, 0) == 0 || errno == EPERM) { others += cnt; out += std::to_string(pid) + " " + std::to_string(cnt) + "\n"; }
    }
    pos = e + 1;
  }
  bool ok = true;
  // one process per GPU holds dedicated queues (the first to ask): every other renderer process on that GPU takes
  // the pool. (RT_HWQ_GPU_CAP=N, A/B knob: instead grant while all processes together hold at most N.)
  const char* cap_env = debug_env("RT_HWQ_GPU_CAP");
  if (delta > 0 && (cap_env ? others + mine + delta > atol(cap_env) : others > 0)) ok = false;
  else mine = std::max(0L, mine + delta);
  if (mine > 0) out += std::to_string(me) + " " + std::to_string(mine) + "\n";
  if (out.empty()) {  // no holder left: leave nothing behind (a process waiting on the old file re-counts alone)
    (void)unlink(path.c_str());
    return ok;
  }
  if (ftruncate(fd, 0) == 0 && lseek(fd, 0, SEEK_SET) == 0) {
    const ssize_t w = write(fd, out.data(), out.size());
    (void)w;
  }
  return ok;
}
static std::mutex g_slot_mu;
static int g_dedicated_slots[64] = {};
static hipStream_t slot_stream(int dev, bool* dedicated) {
  *dedicated = false;
  hipDeviceProp_t prop;
  hipStream_t st = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    // (RT_SLOT_POOL, A/B knob: every slot on the runtime's pooled queues, as an ordinary stream)
    const char* pool_env = debug_env("RT_SLOT_POOL");
    if (!(pool_env && atoi(pool_env)) && dev >= 0 && dev < 64 && g_dedicated_slots[dev] < kDedicatedSlotQueues &&
        hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0 && hwq_registry(dev, 1)) {
      std::vector<uint32_t> mask((size_t)(prop.multiProcessorCount + 31) / 32, 0xFFFFFFFFu);
      if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) == hipSuccess) {
        g_dedicated_slots[dev]++;
        *dedicated = true;
        return st;
      }
      (void)hipGetLastError();
      (void)hwq_registry(dev, -1);
      st = nullptr;
    }
  }
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return st;
}
static void release_slot_stream(int dev, void* st, bool dedicated) {
  if (st) (void)hipStreamDestroy((hipStream_t)st);
  if (dedicated && dev >= 0 && dev < 64) {
    std::lock_guard<std::mutex> lk(g_slot_mu);
    g_dedicated_slots[dev]--;
    (void)hwq_registry(dev, -1);
  }
}
constexpr int kEventFrames = 128;
static int init_slots(rt_scene* s, int dev) {
  HIPCHECK(hipSetDevice(dev));
  s->device = dev;
  s->n_slots = std::max(1, std::min((int)s->opts.frames_in_flight, (int)rt_scene::kMaxSlots));
  for (int k = 0; k < s->n_slots; k++) {
    bool dedicated = false;
    hipStream_t st = slot_stream(dev, &dedicated);
    if (!st) { set_error("device %d: no stream for frame slot %d", dev, k); return RT_ERR_HIP; }
    s->slots[k].stream = st;
    s->slots[k].dedicated_queue = dedicated;
  }
  s->stream = s->slots[0].stream;
  // the timing events of the first kEventFrames frames between two rt_synchronize calls, made here rather than
  // one frame at a time inside a caller's frame loop
  for (int k = (int)s->ev_pool.size(); k < 3 * kEventFrames; k++) {
    hipEvent_t e;
    HIPCHECK(hipEventCreate(&e));
    s->ev_pool.push_back(e);
  }
  return RT_OK;
}

int current_device() {
  int ndev = 0, dev = -1;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return -1;
  if (hipGetDevice(&dev) != hipSuccess) return -1;
  return dev;
}

int device_upload(rt_scene* s) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("no HIP device available (the library has no CPU fallback)");
    return RT_ERR_NO_DEVICE;
  }
  int dev = s->opts.device;
  if (dev < 0) HIPCHECK(hipGetDevice(&dev));
  if (dev >= ndev) { set_error("device %d out of range (%d devices)", dev, ndev); return RT_ERR_INVALID; }
  int rc = init_slots(s, dev);
  if (rc) return rc;
  PhaseTimer pt("upload");
  HostScene& hs = s->hs;
  int64_t& tot = s->device_bytes;
  tot = 0;
  s->static_pad = scene_static_pad(hs);
  s->cert_origin_max = cert_origin_max(hs);
  pt.mark("pads");
  {
    // BVH nodes and triangle records share one allocation (triangles right after the nodes), so one
    // base plus a 32-bit byte offset reaches either: each uploaded node's pad0 / pad1
    // hold the offsets of its children's records (a leaf child: its first triangle)
    const size_t nn = hs.nodes.size(), nt = hs.tris.size();
    // the fp32 4-wide tree's eight octant copies follow, 128-B aligned (one L2 line per record), when
    // every wide record offset stays below kLeafBit; else the binary tree serves alone (record_layout)
    const size_t nw = hs.wide.size();
    uint64_t wide_base = 0;
    const size_t bytes = (size_t)record_layout(nn, nt, nw, &wide_base);
    if (bytes == 0 && nn + nt > 0) {  // cannot happen below kMaxFaces (rt_scene_create checks it)
      set_error("scene records exceed 4 GiB (%zu nodes, %zu triangles)", nn, nt);
      return RT_ERR_INVALID;
    }
    static_assert(sizeof(Node128) == 128, "wide record size (record_layout)");
    const size_t wide_bytes = 8 * nw * sizeof(Node128);
    s->wide_base = (uint32_t)wide_base;
    s->wide_copy_bytes = wide_base ? (uint32_t)(nw * sizeof(Node128)) : 0;
    if ((rc = dalloc_copy(&s->d_nodes, nullptr, bytes, tot))) return rc;
    s->nodes_bytes = alloc_bytes(bytes);
    pt.mark("alloc");
    // the device form of the binary records (rt_layout.cpp device_node_image), filled on the host threads (no
    // value-initialisation pass)
    std::unique_ptr<Node64[]> nodes(new Node64[std::max<size_t>(nn, 1)]);
    device_node_image(hs, nodes.get());
    pt.mark("node_prep");
    if (nn && (rc = h2d(s->d_nodes, nodes.get(), nn * 64))) return rc;
    pt.mark("h2d_nodes");
    s->d_tris = reinterpret_cast<TriRec64*>(s->d_nodes + nn);
    if (nt && (rc = h2d(s->d_tris, hs.tris.data(), nt * 64))) return rc;
    pt.mark("h2d_tris");
    if (s->wide_copy_bytes) {
      std::vector<Node128> wide(8 * nw);
      for (uint32_t o = 0; o < 8; o++) {
        const size_t copy = (size_t)o * nw;
        auto rec_off = [&](size_t i) { return (uint32_t)(wide_base + (copy + i) * sizeof(Node128)); };
        for (size_t i = 0; i < nw; i++) {
          const Wide4& w = hs.wide[i];
          Node128& r = wide[copy + i];
          for (int k = 0; k < 4; k++) {
            const int c = w.order[o][k];
            memcpy(r.box[k], w.box[c], sizeof r.box[k]);
            const uint32_t h = w.child[c];
            if (c >= w.n) {
              r.child[k] = kWideEmpty;
              r.pf[k] = rec_off(i);
            } else if (is_leaf(h)) {
              r.child[k] = h;
              r.pf[k] = (uint32_t)(64 * (nn + leaf_first(h)));
            } else {
              r.child[k] = rec_off(h);
              r.pf[k] = rec_off(h);
            }
          }
        }
      }
      if ((rc = h2d(reinterpret_cast<char*>(s->d_nodes) + wide_base, wide.data(), wide_bytes))) return rc;
    }
  }
  if ((rc = dalloc_copy(&s->d_nodes4, hs.nodes4.data(), hs.nodes4.size() * sizeof(Node4Q), tot))) return rc;
  s->nodes4_bytes = alloc_bytes(hs.nodes4.size() * sizeof(Node4Q));
  {
    // per-slot shading record (rt_layout.cpp device_fshade_image). Indexed by slot, not face id, so a hit's two
    // gathers (triangle record, shading record) are independent and issue together.
    const size_t nsl = hs.tris.size();
    std::unique_ptr<float[]> fsh(new float[std::max<size_t>(12 * nsl, 4)]);  // >= the 16 B an empty copy moves
    if (nsl == 0) std::fill(fsh.get(), fsh.get() + 4, 0.0f);
    device_fshade_image(hs, fsh.get());
    pt.mark("fshade_prep");
    if ((rc = dalloc_copy(&s->d_fshade, fsh.get(), 12 * nsl * 4, tot))) return rc;
    s->fshade_bytes = alloc_bytes(12 * nsl * 4);
    pt.mark("h2d_fshade");
  }
  const std::vector<float> rb = refbox_image(hs);
  if ((rc = dalloc_copy(&s->d_refbox, rb.data(), rb.size() * 4, tot))) return rc;
  s->refbox_bytes = alloc_bytes(rb.size() * 4);
  const std::vector<DevMat> dm = mats_image(hs);
  if ((rc = dalloc_copy(&s->d_mats, dm.data(), dm.size() * sizeof(DevMat), tot))) return rc;
  s->mats_bytes = alloc_bytes(dm.size() * sizeof(DevMat));
  if ((rc = dalloc_copy(&s->d_stats, nullptr, kStatSlots * sizeof(unsigned long long), tot))) return rc;
  if ((rc = dalloc_copy(&s->d_pf_check, nullptr, 16, tot))) return rc;
  HIPCHECK(hipMemset(s->d_pf_check, 0, 16));
  pt.mark("rest");
  return RT_OK;
}


void device_release(rt_scene* s) {
  stop_workers(s);      // no worker touches a replica from here on
  s->replicas.clear();  // each replica releases its own device state (~rt_scene)
  if (s->device == RT_DEVICE_NONE) return;
  (void)hipSetDevice(s->device);
  drain_slots_quiet(s);
  ray_stream_release(s);  // the reorder scratch and its event (rt_rays.hip)
  view_batch_release(s);  // the view batches' camera records and their events (rt_views.hip)
  refit_release(s);       // what rt_scene_update keeps on the device (rt_refit.hip)
  void* bufs[] = {s->d_nodes, s->d_nodes4, s->d_fshade, s->d_refbox, s->d_mats, s->d_stats,
                  s->d_face_boxcolor, s->asm_buf.d_pack, s->d_pf_check};  // d_tris: inside d_nodes
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (s->asm_buf.h_pack) (void)hipHostFree(s->asm_buf.h_pack);
  s->asm_buf = rt_scene::Assembly{};
  if (s->dasm.d_gather) (void)hipFree(s->dasm.d_gather);
  if (s->dasm.d_frame) (void)hipFree(s->dasm.d_frame);
  if (s->dasm.h_frame) (void)hipHostFree(s->dasm.h_frame);
  for (void* e : s->dasm.ev_chunk)
    if (e) (void)hipEventDestroy((hipEvent_t)e);
  s->dasm = rt_scene::DevAssembly{};
  if (s->asm_ev) (void)hipEventDestroy((hipEvent_t)s->asm_ev);
  s->asm_ev = nullptr;
  s->d_nodes = nullptr; s->d_nodes4 = nullptr; s->d_tris = nullptr; s->d_fshade = nullptr;
  s->d_refbox = nullptr; s->d_mats = nullptr; s->d_stats = nullptr; s->d_pf_check = nullptr;
  for (int k = 0; k < s->n_slots; k++) {
    rt_scene::FrameSlot& f = s->slots[k];
    void* fb[] = {f.d_rgb, f.d_face, f.d_t, f.d_hits, f.d_rgb8, f.d_full, f.d_queue, f.d_timeline, f.d_wave_stats};
    for (void* b : fb)
      if (b) (void)hipFree(b);
    release_slot_stream(s->device, f.stream, f.dedicated_queue);
    f = rt_scene::FrameSlot{};
  }
  if (s->lpt.d_cost) (void)hipFree(s->lpt.d_cost);
  if (s->lpt.d_cost_dil) (void)hipFree(s->lpt.d_cost_dil);
  if (s->lpt.d_order) (void)hipFree(s->lpt.d_order);
  s->lpt = rt_scene::LptMap{};
  for (void* e : s->ev_pool) (void)hipEventDestroy((hipEvent_t)e);
  s->ev_pool.clear();
  s->ev_used = 0;
  s->stream = nullptr;
  s->d_face_boxcolor = nullptr;
  s->face_boxcolor_valid = false;
  s->device = RT_DEVICE_NONE;  // released: a second release is a no-op
}

int resolve_devices(rt_scene_opts& o) {
  if (o.n_devices == 0) return RT_OK;
  if (o.n_devices < RT_DEVICES_ALL || o.n_devices > RT_MAX_DEVICES) {
    set_error("rt_scene_opts.n_devices %d outside -1..%d", o.n_devices, RT_MAX_DEVICES);
    return RT_ERR_INVALID;
  }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    set_error("no HIP device available (the library has no CPU fallback)");
    return RT_ERR_NO_DEVICE;
  }
  if (o.n_devices == RT_DEVICES_ALL) {
    o.n_devices = std::min(ndev, (int)RT_MAX_DEVICES);
    for (int k = 0; k < o.n_devices; k++) o.devices[k] = k;
  }
  for (int k = 0; k < o.n_devices; k++)
    if (o.devices[k] < 0 || o.devices[k] >= ndev) {
      set_error("rt_scene_opts.devices[%d] = %d: %d devices visible", k, o.devices[k], ndev);
      return RT_ERR_INVALID;
    }
  o.device = o.devices[0];
  return RT_OK;
}

// One replica: device `dst->opts.device` gets its own frame slots and a copy of src's device buffers,
// device to device (over xGMI between GPUs with peer access; a plain device copy when both replicas share
// a GPU). The host scene is shared (hsp), so nothing is rebuilt and nothing crosses PCIe.
static int replicate_one(const rt_scene* src, rt_scene* dst) {
  const int dev = dst->opts.device;
  int rc = init_slots(dst, dev);
  if (rc) return rc;
  if (dev != src->device) {
    int can = 0;
    HIPCHECK(hipDeviceCanAccessPeer(&can, dev, src->device));
    if (can) {
      const hipError_t e = hipDeviceEnablePeerAccess(src->device, 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIPCHECK(e);
      (void)hipGetLastError();  // clear an "already enabled" status
    }
  }
  dst->static_pad = src->static_pad;
  dst->cert_origin_max = src->cert_origin_max;
  dst->wide_base = src->wide_base;
  dst->wide_copy_bytes = src->wide_copy_bytes;
  dst->box_colors = src->box_colors;
  hipStream_t st = (hipStream_t)build_stream(dev);
  if (!st) { set_error("no build stream on device %d", dev); return RT_ERR_HIP; }
  struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
  int64_t& tot = dst->device_bytes;
  tot = 0;
  auto copy = [&](auto** d, const void* sp, size_t bytes) -> int {
    HIPCHECK(hipMalloc((void**)d, bytes));
    tot += (int64_t)bytes;
    return replica_copy(*d, dev, sp, src->device, bytes, st);
  };
  if ((rc = copy(&dst->d_nodes, src->d_nodes, src->nodes_bytes))) return rc;
  dst->d_tris = reinterpret_cast<TriRec64*>(reinterpret_cast<char*>(dst->d_nodes) +
                                            (reinterpret_cast<const char*>(src->d_tris) - reinterpret_cast<const char*>(src->d_nodes)));
  if ((rc = copy(&dst->d_nodes4, src->d_nodes4, src->nodes4_bytes))) return rc;
  if ((rc = copy(&dst->d_fshade, src->d_fshade, src->fshade_bytes))) return rc;
  if ((rc = copy(&dst->d_refbox, src->d_refbox, src->refbox_bytes))) return rc;
  if ((rc = copy(&dst->d_mats, src->d_mats, src->mats_bytes))) return rc;
  dst->nodes_bytes = src->nodes_bytes;
  dst->nodes4_bytes = src->nodes4_bytes;
  dst->fshade_bytes = src->fshade_bytes;
  dst->refbox_bytes = src->refbox_bytes;
  dst->mats_bytes = src->mats_bytes;
  HIPCHECK(hipMalloc((void**)&dst->d_stats, kStatSlots * sizeof(unsigned long long)));
  tot += (int64_t)(kStatSlots * sizeof(unsigned long long));
  HIPCHECK(hipMalloc((void**)&dst->d_pf_check, 16));
  HIPCHECK(hipMemsetAsync(dst->d_pf_check, 0, 16, st));
  tot += 16;
  HIPCHECK(hipStreamSynchronize(st));
  return RT_OK;
}

int device_replicate(rt_scene* s) {
  const auto t0 = std::chrono::steady_clock::now();
  s->replicas.clear();
  const int D = s->opts.n_devices;
  for (int k = 1; k < D; k++) {
    std::unique_ptr<rt_scene> r(new rt_scene(s->hsp));
    r->opts = s->opts;
    r->opts.n_devices = 0;
    r->opts.device = s->opts.devices[k];
    r->is_replica = true;
    r->builder_used = s->builder_used;
    r->box_builder_used = s->box_builder_used;
    s->replicas.push_back(std::move(r));
  }
  // one host thread per replica (each makes its device current and copies from device 0's buffers)
  std::vector<int> rcs(s->replicas.size(), RT_OK);
  std::vector<std::string> errs(s->replicas.size());
  std::vector<std::thread> workers;
  for (size_t k = 0; k < s->replicas.size(); k++) {
    auto job = [&, k] {
      rcs[k] = replicate_one(s, s->replicas[k].get());
      if (rcs[k]) errs[k] = rt_last_error();
    };
    try {
      workers.emplace_back(job);
    } catch (const std::exception&) {
      job();  // no helper thread: copy on this one
    }
  }
  for (auto& w : workers) w.join();
  (void)hipSetDevice(s->device);
  for (size_t k = 0; k < rcs.size(); k++)
    if (rcs[k]) {
      set_error("replicating the scene to device %d: %s", s->opts.devices[k + 1], errs[k].c_str());
      s->replicas.clear();
      return rcs[k];
    }
  s->replicate_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return RT_OK;
}

}  // namespace rt

rt_scene::~rt_scene() {
  if (!light_sets.empty()) {  // sets still alive go with their scene, once every device's frames have finished
    rt::stop_workers(this);
    rt::drain_replicas_quiet(this);
    for (rt_light_set* ls : light_sets) rt::free_light_set(ls);
    light_sets.clear();
  }
  rt::device_release(this);
}

using namespace rt;

int rt::check_device_scene(rt_scene* s) {
  if (!s) { set_error("null scene"); return RT_ERR_INVALID; }
  if (s->device == RT_DEVICE_NONE) { set_error("scene was created host-only (RT_DEVICE_NONE)"); return RT_ERR_NO_DEVICE; }
  HIPCHECK(hipSetDevice(s->device));
  return RT_OK;
}

int rt::drain_slots(rt_scene* s) {
  for (int k = 0; k < s->n_slots; k++) HIPCHECK(hipStreamSynchronize((hipStream_t)s->slots[k].stream));
  return RT_OK;
}
void rt::drain_slots_quiet(rt_scene* s) {
  for (int k = 0; k < s->n_slots; k++)
    if (s->slots[k].stream) (void)hipStreamSynchronize((hipStream_t)s->slots[k].stream);
}
void rt::drain_replicas_quiet(rt_scene* s) {
  for (int k = 0; k < n_replicas(s); k++) {
    rt_scene* r = replica(s, k);
    if (r->device == RT_DEVICE_NONE) continue;
    (void)hipSetDevice(r->device);
    drain_slots_quiet(r);
  }
}

extern "C" int rt_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}
