// rt_download.hip -- frame download and assembly of the MI355X ray-traversal library: the 8-bit output path
// (k_frame_rgb8), the pack / unpack kernels of a shard's tiles, the assembly of a multi-device scene's frame from
// its replicas (on the host, or on device 0 behind RT_ASM_DEVICE), rt_frame_download*, and the shard API for
// callers that gather shards themselves (rt_frame_shard_*, rt_frame_pack_shard_rgb8, rt_frame_unpack_shards_rgb8).
#include <string>
#include <thread>
#include <vector>

#include "rt_device.h"
#include "rt_traverse.h"  // ballot, lane_id

namespace rt {

// Output path: the float frame -> the PPM's 8-bit values on the device, so the host
// reads 3 B/px instead of 12. Value = min(255, (int)(255*c)) as writePPMImage computes it
// (tucano/utils/ppmIO.hpp:135-156; x86 cvttss2si: NaN / out of range -> INT_MIN); values outside
// 0..255 (NaN or negative colours) are clamped and flagged, so the caller knows when the 8-bit frame is
// not exactly the PPM's numbers.
__global__ __launch_bounds__(256) void k_frame_rgb8(const float* rgb, uint8_t* out, uint32_t n, uint32_t* anomaly) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  if (i < n) {
    const float x = 255.0f * rgb[i];
    int v = (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN;
    v = min(255, v);
    bad = v < 0;
    out[i] = (uint8_t)max(v, 0);
  }
  if (ballot(bad) && lane_id() == 0) atomicOr(anomaly, 1u);
}

// Multi-GPU frame assembly (f3): a rank packs the 8-bit values of its own 16x16 tiles contiguously
// (tile order of its shard, 768 B per tile, pixels outside the frame zero) so that one gather of equal
// slices (RCCL over xGMI) brings every shard to one GPU, which unpacks them into the frame.
__device__ __forceinline__ uint8_t ppm_u8(float c) {
  const float x = 255.0f * c;
  const int v = (x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN;
  return (uint8_t)max(min(255, v), 0);
}
// anomaly (may be null): set when some value is NaN or negative (as k_frame_rgb8 flags it)
__global__ __launch_bounds__(256) void k_pack_shard(const float* rgb, uint8_t* out, int W, int H, int tiles_x,
                                                    int si, int sc, int n_tiles, int S, uint32_t* anomaly) {
  const int L = blockIdx.x;  // one block per tile slot of the shard, one thread per pixel
  if (L >= n_tiles) return;
  int tx, ty;
  shard_tile_xy(tiles_x, S, si, sc, L, tx, ty);
  const int x = tx * 16 + (threadIdx.x & 15), y = ty * 16 + (threadIdx.x >> 4);
  uint8_t* o = out + ((size_t)L * 256 + threadIdx.x) * 3;
  bool bad = false;
  if (x < W && y < H) {
    const float* c = rgb + 3 * ((size_t)y * W + x);
    for (int k = 0; k < 3; k++) {
      o[k] = ppm_u8(c[k]);
      const float x = 255.0f * c[k];  // k_frame_rgb8's test: the PPM's number (int)x below 0, or NaN
      bad = bad || ((x >= -2147483648.0f && x < 2147483648.0f) ? (int)x : INT_MIN) < 0;
    }
  } else {
    o[0] = o[1] = o[2] = 0;
  }
  if (anomaly && ballot(bad) && lane_id() == 0) atomicOr(anomaly, 1u);
}
// Multi-device frame assembly: a replica packs its tiles' 32-bit values (ch per pixel: colour 3, face id or
// t 1) contiguously in its shard's slot order (256 * ch words per tile, pixels outside the frame zero), so
// one copy per device brings them to the host, which places the tiles into the caller's frame.
__global__ __launch_bounds__(256) void k_pack_tiles32(const uint32_t* src, uint32_t* out, int W, int H, int tiles_x,
                                                      int si, int sc, int n_tiles, int S, int ch) {
  const int L = blockIdx.x;
  if (L >= n_tiles) return;
  int tx, ty;
  shard_tile_xy(tiles_x, S, si, sc, L, tx, ty);
  const int x = tx * 16 + (threadIdx.x & 15), y = ty * 16 + (threadIdx.x >> 4);
  const bool in = x < W && y < H;
  uint32_t* o = out + ((size_t)L * 256 + threadIdx.x) * ch;
  const uint32_t* c = src + (size_t)ch * (in ? (size_t)y * W + x : 0);
  for (int k = 0; k < ch; k++) o[k] = in ? c[k] : 0u;
}
__global__ __launch_bounds__(256) void k_unpack_shards(const uint8_t* packed, uint8_t* frame, int W, int H, int tiles_x,
                                                       int n, size_t slice_bytes, int S) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= (size_t)W * H) return;
  const int x = (int)(p % W), y = (int)(p / W);
  // the inverse of shard_tile_xy: tile -> super-tile s -> (owner s % n, slot (s / n) * S^2 + in-super index)
  const int tx = x >> 4, ty = y >> 4, sxn = (tiles_x + S - 1) / S;
  const int s = (ty / S) * sxn + tx / S, slot = (s / n) * S * S + (ty % S) * S + tx % S;
  const uint8_t* src = packed + (size_t)(s % n) * slice_bytes + ((size_t)slot * 256 + (y & 15) * 16 + (x & 15)) * 3;
  frame[3 * p + 0] = src[0];
  frame[3 * p + 1] = src[1];
  frame[3 * p + 2] = src[2];
}

// Device-side assembly of a multi-device scene's frame (assemble_device): block (L, k) places tile slot L of replica
// k's packed slice (k_pack_tiles32 / k_pack_shard layout: 256 pixels of E bytes per tile) into the frame on device 0
struct UnpackArgs {
  int32_t n_rep, W, H, tiles_x, E;
  int32_t si[RT_MAX_DEVICES], sc[RT_MAX_DEVICES], S[RT_MAX_DEVICES], n_tiles[RT_MAX_DEVICES];
  uint64_t off[RT_MAX_DEVICES], flag_off[RT_MAX_DEVICES];  // byte offsets of slice k and of its exactness flag
};
__global__ __launch_bounds__(256) void k_unpack_tiles(const uint8_t* gather, uint8_t* frame, UnpackArgs a) {
  const int k = (int)blockIdx.y, L = (int)blockIdx.x;
  if (k >= a.n_rep || L >= a.n_tiles[k]) return;
  int tx, ty;
  shard_tile_xy(a.tiles_x, a.S[k], a.si[k], a.sc[k], L, tx, ty);
  const int x = tx * 16 + (int)(threadIdx.x & 15), y = ty * 16 + (int)(threadIdx.x >> 4);
  if (x >= a.W || y >= a.H) return;
  const size_t src = a.off[k] + ((size_t)L * 256 + threadIdx.x) * (size_t)a.E, dst = ((size_t)y * a.W + x) * (size_t)a.E;
  if (a.E == 3) {
    frame[dst] = gather[src];
    frame[dst + 1] = gather[src + 1];
    frame[dst + 2] = gather[src + 2];
  } else {  // 4 or 12 bytes, 4-byte aligned (slices start on 16 B)
    const uint32_t* s4 = reinterpret_cast<const uint32_t*>(gather + src);
    uint32_t* d4 = reinterpret_cast<uint32_t*>(frame + dst);
    for (int w = 0; w < a.E / 4; w++) d4[w] = s4[w];
  }
}
// the 8-bit frame's exactness flags of every replica, OR-ed into the word after the frame
__global__ void k_or_flags(const uint8_t* gather, UnpackArgs a, uint32_t* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t f = 0;
  for (int k = 0; k < a.n_rep; k++) f |= *reinterpret_cast<const uint32_t*>(gather + a.flag_off[k]);
  *out = f;
}

}  // namespace rt

using namespace rt;

// Frame assembly of a multi-device scene: every replica packs its tiles of its last frame (contiguous, its
// shard's slot order: k_pack_tiles32 / k_pack_shard) and copies them into its pinned host buffer, all
// devices queued first; then one host worker per device waits for its copy and places the tiles into the
// caller's frame (rows of 16 pixels). Only the tiles of the replicas' shards are written.
static size_t asm_pixel_bytes(AsmKind kind) { return kind == ASM_RGB ? 12 : kind == ASM_RGB8 ? 3 : 4; }
// replica r's shard of its last frame, packed at `kind`'s pixel size
static ShardLayout last_shard(const rt_scene* r, AsmKind kind) {
  return shard_layout(r->last_W, r->last_H, r->last_shard_index, r->last_shard_count, asm_pixel_bytes(kind));
}

// the replicas' frames must be of the scene's last size (and carry hit records for face / t)
static int check_replica_frames(rt_scene* s, AsmKind kind, const char* what) {
  const int W = s->last_W, H = s->last_H;
  for (int k = 0; k < n_replicas(s); k++) {
    rt_scene* r = replica(s, k);
    int rc = check_device_scene(r);
    if (rc) return rc;
    const rt_scene::FrameSlot& f = r->slots[r->last_slot];
    if (!f.d_rgb || r->last_W != W || r->last_H != H || (size_t)W * H > f.fb_pixels) {
      set_error("%s: device %d has no frame of the scene's last size", what, r->device);
      return RT_ERR_INVALID;
    }
    if ((kind == ASM_FACE || kind == ASM_T) && !(r->last_flags & RT_FRAME_WRITE_HITS)) {
      set_error("last frame was rendered without RT_FRAME_WRITE_HITS");
      return RT_ERR_INVALID;
    }
  }
  return RT_OK;
}

// room for `need` bytes in a replica's pack buffer and its pinned copy; st: the stream of the frame to pack
static int ensure_pack(rt_scene::Assembly& a, size_t need, hipStream_t st) {
  if (need <= a.bytes) return RT_OK;
  HIPCHECK(hipStreamSynchronize(st));
  if (a.d_pack) (void)hipFree(a.d_pack);
  if (a.h_pack) (void)hipHostFree(a.h_pack);
  a = rt_scene::Assembly{};
  HIPCHECK(hipMalloc(&a.d_pack, need));
  HIPCHECK(hipHostMalloc(&a.h_pack, need, hipHostMallocDefault));
  a.bytes = need;
  return RT_OK;
}

// a slot's frame -> the tiles of shard l (l.slots > 0) packed at dst, on st: the 8-bit values with their exactness
// flag (cleared first; null: none kept), or the 32-bit words of kind
static int launch_pack(AsmKind kind, const rt_scene::FrameSlot& f, const ShardLayout& l, void* dst, uint32_t* flag, hipStream_t st) {
  if (kind == ASM_RGB8) {
    if (flag) HIPCHECK(hipMemsetAsync(flag, 0, 4, st));
    hipLaunchKernelGGL(k_pack_shard, dim3(l.slots), dim3(256), 0, st, (const float*)f.d_rgb, (uint8_t*)dst, l.W, l.H, l.tiles_x,
                       l.index, l.count, l.slots, l.S, flag);
  } else {
    const uint32_t* src = kind == ASM_RGB ? (const uint32_t*)f.d_rgb
                          : kind == ASM_FACE ? (const uint32_t*)f.d_face : (const uint32_t*)f.d_t;
    hipLaunchKernelGGL(k_pack_tiles32, dim3(l.slots), dim3(256), 0, st, src, (uint32_t*)dst, l.W, l.H, l.tiles_x,
                       l.index, l.count, l.slots, l.S, kind == ASM_RGB ? 3 : 1);
  }
  HIPCHECK(hipGetLastError());
  return RT_OK;
}

// Device-side assembly (SURVEY e1 "peer-writes to GPU0"; A/B knob RT_ASM_DEVICE, see assemble):
// when the replicas rendered the whole frame between them, each packs its tiles on its own stream and copies
// them into device 0's gather buffer (hipMemcpyPeerAsync over xGMI; a device copy when replicas share a GPU),
// device 0 waits for every slice (one event per replica), places all tiles with one kernel (k_unpack_tiles)
// and copies the frame to pinned host memory in kChunks pieces, which host threads move into the caller's
// buffer as each lands.
static int assemble_device(rt_scene* s, AsmKind kind, void* out, int32_t* exact, const char* what) {
  const int D = n_replicas(s);
  const int W = s->last_W, H = s->last_H;
  const size_t E = asm_pixel_bytes(kind);
  int rc;
  UnpackArgs ua;
  memset(&ua, 0, sizeof ua);
  ua.n_rep = D, ua.W = W, ua.H = H, ua.tiles_x = (W + 15) / 16, ua.E = (int32_t)E;
  std::vector<ShardLayout> lay((size_t)D);
  size_t total = 0;
  int max_tiles = 0;
  for (int k = 0; k < D; k++) {
    const ShardLayout& l = lay[k] = last_shard(replica(s, k), kind);
    ua.si[k] = l.index, ua.sc[k] = l.count, ua.S[k] = l.S, ua.n_tiles[k] = l.slots;
    max_tiles = std::max(max_tiles, l.slots);
    ua.off[k] = total;
    ua.flag_off[k] = total + l.flag_off;
    total += l.flag_off + 16;
  }
  const size_t frame_bytes = (size_t)W * H * E;
  rt_scene::DevAssembly& g = s->dasm;
  HIPCHECK(hipSetDevice(s->device));
  if (total > g.gather_bytes || frame_bytes + 16 > g.frame_bytes || frame_bytes + 16 > g.h_bytes) {
    for (int k = 0; k < D; k++) {  // no replica's copy into the old buffers may be in flight
      HIPCHECK(hipSetDevice(replica(s, k)->device));
      if ((rc = drain_slots(replica(s, k)))) return rc;
    }
    HIPCHECK(hipSetDevice(s->device));
    auto grow = [](void*& p, size_t& cap, size_t want, bool pinned) -> int {  // to exactly `want` bytes
      if (want <= cap) return RT_OK;
      if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
      p = nullptr, cap = 0;
      HIPCHECK(pinned ? hipHostMalloc(&p, want, hipHostMallocDefault) : hipMalloc(&p, want));
      cap = want;
      return RT_OK;
    };
    if ((rc = grow(g.d_gather, g.gather_bytes, total, false)) || (rc = grow(g.d_frame, g.frame_bytes, frame_bytes + 16, false)) ||
        (rc = grow(g.h_frame, g.h_bytes, frame_bytes + 16, true)))
      return rc;
  }
  for (int c = 0; c < rt_scene::DevAssembly::kChunks; c++)
    if ((rc = ensure_event(g.ev_chunk[c]))) return rc;
  uint8_t* gather = (uint8_t*)g.d_gather;
  // every replica: pack behind its share of the frame; replicas 1.. copy their slice to device 0
  for (int k = 0; k < D; k++) {
    rt_scene* r = replica(s, k);
    HIPCHECK(hipSetDevice(r->device));
    rt_scene::FrameSlot& f = r->slots[r->last_slot];
    hipStream_t st = (hipStream_t)f.stream;
    const ShardLayout& l = lay[k];
    const size_t need = l.flag_off + 16;
    uint8_t* dst;
    if (k == 0) {
      dst = gather + ua.off[0];
    } else {
      if ((rc = ensure_pack(r->asm_buf, need, st))) return rc;
      dst = (uint8_t*)r->asm_buf.d_pack;
      if ((rc = ensure_event(r->asm_ev))) return rc;
    }
    uint32_t* flag = (uint32_t*)(dst + l.flag_off);
    if (l.slots > 0) {
      if ((rc = launch_pack(kind, f, l, dst, flag, st))) return rc;
    } else if (kind == ASM_RGB8) {
      HIPCHECK(hipMemsetAsync(flag, 0, 4, st));
    }
    if (k > 0) {
      if (r->device == s->device) HIPCHECK(hipMemcpyAsync(gather + ua.off[k], dst, need, hipMemcpyDeviceToDevice, st));
      else HIPCHECK(hipMemcpyPeerAsync(gather + ua.off[k], s->device, dst, r->device, need, st));
      HIPCHECK(hipEventRecord((hipEvent_t)r->asm_ev, st));
    }
  }
  // device 0: every slice in, tiles placed, the frame to the host in chunks
  HIPCHECK(hipSetDevice(s->device));
  hipStream_t st0 = (hipStream_t)s->slots[s->last_slot].stream;
  for (int k = 1; k < D; k++) HIPCHECK(hipStreamWaitEvent(st0, (hipEvent_t)replica(s, k)->asm_ev, 0));
  uint8_t* frame = (uint8_t*)g.d_frame;
  if (max_tiles > 0) {
    hipLaunchKernelGGL(k_unpack_tiles, dim3((unsigned)max_tiles, (unsigned)D), dim3(256), 0, st0, (const uint8_t*)gather, frame, ua);
    HIPCHECK(hipGetLastError());
  }
  if (kind == ASM_RGB8) {
    hipLaunchKernelGGL(k_or_flags, dim3(1), dim3(64), 0, st0, (const uint8_t*)gather, ua, (uint32_t*)(frame + frame_bytes));
    HIPCHECK(hipGetLastError());
  }
  const int C = (int)std::max<size_t>(1, std::min<size_t>(rt_scene::DevAssembly::kChunks, frame_bytes >> 21));
  const size_t cb = ((frame_bytes + C - 1) / C + 63) & ~(size_t)63;
  auto span = [&](int c, size_t& o, size_t& n) {
    o = std::min(frame_bytes, (size_t)c * cb);
    n = std::min(frame_bytes, o + cb) - o;
  };
  for (int c = 0; c < C; c++) {
    size_t o, n;
    span(c, o, n);
    const size_t extra = (c == C - 1 && kind == ASM_RGB8) ? 4 : 0;  // the OR-ed flag follows the frame
    if (n + extra) HIPCHECK(hipMemcpyAsync((uint8_t*)g.h_frame + o, frame + o, n + extra, hipMemcpyDeviceToHost, st0));
    HIPCHECK(hipEventRecord((hipEvent_t)g.ev_chunk[c], st0));
  }
  std::vector<int> ok((size_t)C, 1);
  auto take = [&](int c) {
    if (hipEventSynchronize((hipEvent_t)g.ev_chunk[c]) != hipSuccess) { ok[c] = 0; return; }
    size_t o, n;
    span(c, o, n);
    if (n) memcpy((uint8_t*)out + o, (const uint8_t*)g.h_frame + o, n);
  };
  std::vector<std::thread> th;
  for (int c = 1; c < C; c++) {
    try {
      th.emplace_back(take, c);
    } catch (const std::exception&) {
      take(c);
    }
  }
  take(0);
  for (auto& t : th) t.join();
  for (int c = 0; c < C; c++)
    if (!ok[c]) { set_error("%s: frame copy to the host failed", what); return RT_ERR_HIP; }
  if (exact) {
    uint32_t fl = 0;
    memcpy(&fl, (const uint8_t*)g.h_frame + frame_bytes, 4);
    *exact = fl ? 0 : 1;
  }
  return RT_OK;
}

int rt::assemble(rt_scene* s, AsmKind kind, int64_t capacity_pixels, void* out, int32_t* exact, const char* what) {
  const int D = n_replicas(s);
  const int W = s->last_W, H = s->last_H;
  const size_t E = asm_pixel_bytes(kind);
  int rc;
  if (W <= 0 || H <= 0) { set_error("%s: no frame rendered", what); return RT_ERR_INVALID; }
  if (capacity_pixels < (int64_t)W * H) {
    set_error("%s: buffers hold %lld pixels, the last frame has %lld (%d x %d)", what, (long long)capacity_pixels,
              (long long)W * H, W, H);
    return RT_ERR_INVALID;
  }
  if ((rc = check_replica_frames(s, kind, what))) return rc;  // (assemble_device relies on it too)
  // The host path below is the default: with the replicas on distinct GPUs every device copies its own tiles
  // over its own PCIe link at once, where the device-side assembly funnels the whole frame through device 0's
  // link. With replicas sharing one GPU (the only measurable case here: one link either way) the two measured
  // level -- 8 replicas, 4K 8-bit frame: 1.10-1.36 vs 1.21-1.27 ms (profiles/ab/r06_assembly_ab.txt). The
  // device-side path (the whole frame split over the replicas) is kept behind the A/B knob RT_ASM_DEVICE.
  const bool whole = s->last_shard_count == D && s->last_shard_index == 0;
  const char* dev_env = debug_env("RT_ASM_DEVICE");
  if (whole && dev_env && atoi(dev_env)) {
    rc = assemble_device(s, kind, out, exact, what);
    HIPCHECK(hipSetDevice(s->device));
    return rc;
  }
  std::vector<ShardLayout> lay((size_t)D);
  for (int k = 0; k < D; k++) {  // every replica: pack behind its share of the frame, then the copy to its pinned buffer
    rt_scene* r = replica(s, k);
    HIPCHECK(hipSetDevice(r->device));
    rt_scene::FrameSlot& f = r->slots[r->last_slot];
    const ShardLayout& l = lay[k] = last_shard(r, kind);
    const size_t need = l.flag_off + 16;
    hipStream_t st = (hipStream_t)f.stream;
    rt_scene::Assembly& a = r->asm_buf;
    if ((rc = ensure_pack(a, need, st))) return rc;
    if (l.slots > 0) {
      if ((rc = launch_pack(kind, f, l, a.d_pack, (uint32_t*)((char*)a.d_pack + l.flag_off), st))) return rc;
      HIPCHECK(hipMemcpyAsync(a.h_pack, a.d_pack, kind == ASM_RGB8 ? need : l.bytes, hipMemcpyDeviceToHost, st));
    }
  }
  // host workers: device k's tiles into the caller's frame once its copy has landed
  std::vector<int> rcs((size_t)D, RT_OK);
  std::vector<std::string> errs((size_t)D);
  std::vector<uint32_t> flags((size_t)D, 0);
  auto place = [&](int k) {
    rt_scene* r = replica(s, k);
    if (hipSetDevice(r->device) != hipSuccess || hipStreamSynchronize((hipStream_t)r->slots[r->last_slot].stream) != hipSuccess) {
      rcs[k] = RT_ERR_HIP;
      errs[k] = "frame copy to the host failed";
      return;
    }
    const char* src = (const char*)r->asm_buf.h_pack;
    char* dst = (char*)out;
    for_each_shard_tile(lay[k], [&](int L, int tx, int ty) {
      const size_t w = (size_t)std::min(16, W - tx * 16) * E;
      const int h = std::min(16, H - ty * 16);
      for (int yy = 0; yy < h; yy++)
        memcpy(dst + ((size_t)(ty * 16 + yy) * W + (size_t)tx * 16) * E, src + ((size_t)L * 256 + (size_t)yy * 16) * E, w);
    });
    if (kind == ASM_RGB8 && lay[k].slots > 0) memcpy(&flags[k], src + lay[k].flag_off, 4);
  };
  std::vector<std::thread> workers;
  for (int k = 1; k < D; k++) {
    try {
      workers.emplace_back(place, k);
    } catch (const std::exception&) {
      place(k);
    }
  }
  place(0);
  for (auto& w : workers) w.join();
  HIPCHECK(hipSetDevice(s->device));
  for (int k = 0; k < D; k++)
    if (rcs[k]) { set_error("%s: device %d: %s", what, replica(s, k)->device, errs[k].c_str()); return rcs[k]; }
  if (exact) {
    *exact = 1;
    for (uint32_t fl : flags)
      if (fl) *exact = 0;
  }
  return RT_OK;
}

extern "C" int rt_frame_download(rt_scene* s, int64_t capacity_pixels, float* rgb, int32_t* face, float* t) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!s->replicas.empty()) {  // the devices' tiles assembled in the caller's buffers
    if (rgb && (rc = assemble(s, ASM_RGB, capacity_pixels, rgb, nullptr, "rt_frame_download"))) return rc;
    if (face && (rc = assemble(s, ASM_FACE, capacity_pixels, face, nullptr, "rt_frame_download"))) return rc;
    if (t && (rc = assemble(s, ASM_T, capacity_pixels, t, nullptr, "rt_frame_download"))) return rc;
    return RT_OK;
  }
  const rt_scene::FrameSlot& f = s->slots[s->last_slot];
  HIPCHECK(hipStreamSynchronize((hipStream_t)f.stream));
  const size_t npix = (size_t)s->last_W * s->last_H;
  if (!f.d_rgb || npix > f.fb_pixels) { set_error("rt_frame_download: no frame rendered"); return RT_ERR_INVALID; }
  if (capacity_pixels < (int64_t)npix) {
    set_error("rt_frame_download: buffers hold %lld pixels, the last frame has %zu (%d x %d)", (long long)capacity_pixels,
              npix, s->last_W, s->last_H);
    return RT_ERR_INVALID;
  }
  if (rgb) HIPCHECK(hipMemcpy(rgb, f.d_rgb, npix * 12, hipMemcpyDeviceToHost));
  if ((face || t) && !(s->last_flags & RT_FRAME_WRITE_HITS)) { set_error("last frame was rendered without RT_FRAME_WRITE_HITS"); return RT_ERR_INVALID; }
  if (face) HIPCHECK(hipMemcpy(face, f.d_face, npix * 4, hipMemcpyDeviceToHost));
  if (t) HIPCHECK(hipMemcpy(t, f.d_t, npix * 4, hipMemcpyDeviceToHost));
  return RT_OK;
}

extern "C" int rt_frame_download_rgb8(rt_scene* s, int64_t capacity_pixels, uint8_t* rgb8, int32_t* exact) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!rgb8) { set_error("rt_frame_download_rgb8: null output"); return RT_ERR_INVALID; }
  if (!s->replicas.empty()) return assemble(s, ASM_RGB8, capacity_pixels, rgb8, exact, "rt_frame_download_rgb8");
  rt_scene::FrameSlot& f = s->slots[s->last_slot];
  const size_t npix = (size_t)s->last_W * s->last_H;
  if (!f.d_rgb || npix == 0 || npix > f.fb_pixels) { set_error("rt_frame_download_rgb8: no frame rendered"); return RT_ERR_INVALID; }
  if (capacity_pixels < (int64_t)npix) {
    set_error("rt_frame_download_rgb8: buffer holds %lld pixels, the last frame has %zu (%d x %d)",
              (long long)capacity_pixels, npix, s->last_W, s->last_H);
    return RT_ERR_INVALID;
  }
  hipStream_t st = (hipStream_t)f.stream;
  if (npix > f.rgb8_pixels && (rc = regrow(f.d_rgb8, f.rgb8_pixels, npix, npix * 3 + 64, st))) return rc;
  uint32_t* flag = (uint32_t*)(f.d_rgb8 + ((npix * 3 + 15) / 16) * 16);
  HIPCHECK(hipMemsetAsync(flag, 0, 4, st));
  const uint32_t n = (uint32_t)(npix * 3);
  hipLaunchKernelGGL(k_frame_rgb8, dim3((n + 255) / 256), dim3(256), 0, st, (const float*)f.d_rgb, f.d_rgb8, n, flag);
  HIPCHECK(hipGetLastError());
  uint32_t h_flag = 0;
  HIPCHECK(hipMemcpyAsync(rgb8, f.d_rgb8, npix * 3, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipMemcpyAsync(&h_flag, flag, 4, hipMemcpyDeviceToHost, st));
  HIPCHECK(hipStreamSynchronize(st));
  if (exact) *exact = h_flag ? 0 : 1;
  return RT_OK;
}

extern "C" int64_t rt_frame_shard_bytes(int32_t W, int32_t H, int32_t shard_count) {
  if (W <= 0 || H <= 0 || shard_count <= 0) return 0;
  return (int64_t)shard_layout(W, H, 0, shard_count, 3).bytes;  // shard 0 has the most tile slots
}

extern "C" int32_t rt_frame_shard_tiles(int32_t W, int32_t H, int32_t shard_index, int32_t shard_count, int32_t* tiles_xy,
                                        int32_t capacity) {
  if (W <= 0 || H <= 0 || shard_count <= 0 || shard_index < 0 || shard_index >= shard_count) return 0;
  int32_t n = 0;
  for_each_shard_tile(shard_layout(W, H, shard_index, shard_count, 3), [&](int, int tx, int ty) {
    if (tiles_xy && n < capacity) { tiles_xy[2 * n] = tx; tiles_xy[2 * n + 1] = ty; }
    n++;
  });
  return n;
}

extern "C" int rt_frame_pack_shard_rgb8(rt_scene* s, void* dst_device) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!dst_device) { set_error("rt_frame_pack_shard_rgb8: null destination"); return RT_ERR_INVALID; }
  if (!s->replicas.empty()) {
    set_error("rt_frame_pack_shard_rgb8: a multi-device scene assembles its frame itself (rt_frame_download_rgb8)");
    return RT_ERR_UNSUPPORTED;
  }
  rt_scene::FrameSlot& f = s->slots[s->last_slot];
  if (!f.d_rgb || (size_t)s->last_W * s->last_H > f.fb_pixels) { set_error("rt_frame_pack_shard_rgb8: no frame rendered"); return RT_ERR_INVALID; }
  const ShardLayout l = last_shard(s, ASM_RGB8);
  hipStream_t st = (hipStream_t)f.stream;
  const size_t slice = (size_t)rt_frame_shard_bytes(l.W, l.H, l.count);  // a shard with fewer slots: zeros behind them
  if (l.bytes < slice) HIPCHECK(hipMemsetAsync((uint8_t*)dst_device + l.bytes, 0, slice - l.bytes, st));
  if (l.slots > 0 && (rc = launch_pack(ASM_RGB8, f, l, dst_device, nullptr, st))) return rc;
  HIPCHECK(hipStreamSynchronize(st));
  return RT_OK;
}

extern "C" int rt_frame_unpack_shards_rgb8(const void* packed_device, int32_t shard_count, int32_t W, int32_t H,
                                           void* frame_device, int32_t device) {
  if (!packed_device || !frame_device || shard_count <= 0 || W <= 0 || H <= 0) {
    set_error("rt_frame_unpack_shards_rgb8: invalid arguments");
    return RT_ERR_INVALID;
  }
  int dev = device;
  if (dev < 0) HIPCHECK(hipGetDevice(&dev));
  HIPCHECK(hipSetDevice(dev));
  const size_t npix = (size_t)W * H;
  hipLaunchKernelGGL(k_unpack_shards, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, 0, (const uint8_t*)packed_device,
                     (uint8_t*)frame_device, W, H, (W + 15) / 16, shard_count, (size_t)rt_frame_shard_bytes(W, H, shard_count),
                     frame_super_tile(shard_count));
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  return RT_OK;
}
