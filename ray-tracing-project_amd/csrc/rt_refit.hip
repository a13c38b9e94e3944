// rt_refit.hip -- rt_scene_update, device side: the slot records, the shading records and the binary tree's boxes
// recomputed on the device from compact per-vertex / per-face arrays (rt_update.cpp prepares them with
// rt_scene_create's own stages). The tree's shape and leaf order never change, so what describes them -- the face
// indices, each leaf handle's parent and side, each node's parent and side, the nodes grouped by level -- is
// uploaded once, at the first update. Three kernels: k_refit_slots (one lane per triangle slot), k_refit_leaves
// (one lane per leaf handle) and k_refit_level (one launch per tree level from the deepest up; the kernel boundary
// is the synchronisation between levels). Also here: the waits before an update, the replicas' copies, the lazy
// host mirror and rt_debug_scene_records.
#include <memory>

#include "rt_device.h"

namespace rt {

// fminf / fmaxf and the host refit's std::min / std::max agree on finite inputs (non-finite coordinates take the
// host path, rt_update.cpp); a single-leaf root's sentinel box (+inf, -inf) is the union's identity in both.

// One lane per triangle slot: the slot's face id stays (leaf order never changes); its record is gathered from the
// world vertices and the per-face words, its shading record from the unit vertex normals and the material id (as
// device_fshade_image), and its unpadded bounds -- of the accept-region triangle where given -- go to slotbox.
// Records are written as whole 16-byte stores.
__global__ void __launch_bounds__(256) k_refit_slots(uint32_t n_slots, uint32_t n_faces, TriRec64* tris, float4* fshade,
                                                     float* slotbox, const uint32_t* fidx, const float* wv, const float* vnn,
                                                     const FaceWords* face, const int32_t* fmat, const float* av) {
  const uint32_t sl = blockIdx.x * 256u + threadIdx.x;
  if (sl >= n_slots) return;
  const uint32_t f = tris[sl].face;
  if (f >= n_faces) return;  // (never: the records are the library's own)
  const uint32_t v0 = fidx[3 * (size_t)f], v1 = fidx[3 * (size_t)f + 1], v2 = fidx[3 * (size_t)f + 2];
  const float* a = wv + 3 * (size_t)v0;
  const float* b = wv + 3 * (size_t)v1;
  const float* c = wv + 3 * (size_t)v2;
  const float w[9] = {a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]};
  const FaceWords fw = face[f];
  float4* r = reinterpret_cast<float4*>(tris + sl);
  r[0] = make_float4(fw.nx, fw.ny, fw.nz, fw.dist);
  r[1] = make_float4(w[0], w[1], w[2], w[3]);
  r[2] = make_float4(w[4], w[5], w[6], w[7]);
  r[3] = make_float4(w[8], __uint_as_float(fw.rank), __uint_as_float(f), __uint_as_float(fw.box));
  const float* n0 = vnn + 3 * (size_t)v0;
  const float* n1 = vnn + 3 * (size_t)v1;
  const float* n2 = vnn + 3 * (size_t)v2;
  float4* sh = fshade + 3 * (size_t)sl;
  sh[0] = make_float4(n0[0], n0[1], n0[2], __int_as_float(fmat[f]));
  sh[1] = make_float4(n1[0], n1[1], n1[2], 0.0f);
  sh[2] = make_float4(n2[0], n2[1], n2[2], 0.0f);
  float p[9];
  for (int k = 0; k < 9; k++) p[k] = av ? av[9 * (size_t)f + k] : w[k];
  float* o = slotbox + 6 * (size_t)sl;
  for (int k = 0; k < 3; k++) {
    o[k] = fminf(fminf(p[k], p[3 + k]), p[6 + k]);
    o[3 + k] = fmaxf(fmaxf(p[k], p[3 + k]), p[6 + k]);
  }
}

// a child's box in its parent's record: lo.x hi.x lo.y hi.y lo.z hi.z, child 1's six floats behind child 0's
__device__ __forceinline__ void put_child_box(Node64* nodes, uint32_t where, const float lo[3], const float hi[3]) {
  float* b = reinterpret_cast<float*>(nodes + (where >> 1)) + 6 * (where & 1u);
  for (int k = 0; k < 3; k++) { b[2 * k] = lo[k]; b[2 * k + 1] = hi[k]; }
}

// One lane per leaf handle: the union of its 1..16 slot boxes, padded, into its parent's child box.
__global__ void __launch_bounds__(256) k_refit_leaves(uint32_t n_leaves, uint32_t n_slots, uint32_t n_nodes, const uint32_t* handle,
                                                      const uint32_t* where, const float* slotbox, Node64* nodes, float pad) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n_leaves) return;
  const uint32_t h = handle[k], first = leaf_first(h), count = leaf_count(h), wh = where[k];
  if (first + count > n_slots || (wh >> 1) >= n_nodes) return;  // (never)
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t sl = first; sl < first + count; sl++) {
    const float* b = slotbox + 6 * (size_t)sl;
    for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], b[c]); hi[c] = fmaxf(hi[c], b[3 + c]); }
  }
  for (int c = 0; c < 3; c++) { lo[c] = lo[c] - pad; hi[c] = hi[c] + pad; }
  put_child_box(nodes, wh, lo, hi);
}

// One lane per node of one tree level (everything below it is final): its order bits are recomputed beside its
// prefetch offsets, and the union of its two child boxes goes into its parent's record -- the union of two padded
// boxes is the padded union, exactly, since x - pad is monotone in x.
__global__ void __launch_bounds__(256) k_refit_level(uint32_t n, uint32_t n_nodes, const uint32_t* ids, const uint32_t* node_where,
                                                     Node64* nodes) {
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const uint32_t i = ids[k];
  if (i >= n_nodes) return;  // (never)
  const Node64 nd = nodes[i];
  const uint32_t order = octant_order(nd);
  nodes[i].pad0 = (nd.pad0 & ~0x3Fu) | (order & 0x3Fu);
  nodes[i].pad1 = (nd.pad1 & ~0x3u) | ((order >> 6) & 0x3u);
  const uint32_t wh = node_where[i];
  if (wh == kNoParent || (wh >> 1) >= n_nodes) return;
  const float lo[3] = {fminf(nd.c0lx, nd.c1lx), fminf(nd.c0ly, nd.c1ly), fminf(nd.c0lz, nd.c1lz)};
  const float hi[3] = {fmaxf(nd.c0hx, nd.c1hx), fmaxf(nd.c0hy, nd.c1hy), fmaxf(nd.c0hz, nd.c1hz)};
  put_child_box(nodes, wh, lo, hi);
}

// ------------------------------------------------------------------------------------------------
// Before an update: nothing queued on the scene may still read its device data
// ------------------------------------------------------------------------------------------------
int update_quiesce(rt_scene* s) {
  for (int k = 0; k < n_replicas(s); k++) {  // the frame slots of every device, as rt_synchronize waits for them
    rt_scene* r = replica(s, k);
    if (r->device == RT_DEVICE_NONE) continue;
    HIPCHECK(hipSetDevice(r->device));
    if (const int rc = drain_slots(r)) return rc;
  }
  HIPCHECK(hipSetDevice(s->device));
  // ray lists and view batches on caller streams: every caller stream's latest list call (in-order lists use no
  // scratch, so the scratch event does not cover them), then the scratch events recorded after their latest use
  for (const auto& u : s->list_use) HIPCHECK(hipEventSynchronize((hipEvent_t)u.second));
  if (s->rays.ev) HIPCHECK(hipEventSynchronize((hipEvent_t)s->rays.ev));
  if (s->views.ev_use) HIPCHECK(hipEventSynchronize((hipEvent_t)s->views.ev_use));
  return RT_OK;
}

template <class T>
static int keep_on_device(T*& dst, const void* src, size_t bytes, int64_t& total) {
  if (!dst) {
    HIPCHECK(hipMalloc((void**)&dst, std::max<size_t>(bytes, 16)));
    total += (int64_t)std::max<size_t>(bytes, 16);
  }
  if (src && bytes) return h2d(dst, src, bytes);
  return RT_OK;
}

// the first update's one-time uploads and allocations
int refit_prepare(rt_scene* s) {
  rt_scene::Refit& R = s->refit;
  if (R.device_ready) return RT_OK;
  const HostScene& hs = s->hs;
  const RefitTopo& t = R.topo;
  int64_t& tot = s->device_bytes;
  int rc;
  if ((rc = keep_on_device(R.d_fidx, hs.fidx.data(), hs.fidx.size() * 4, tot))) return rc;
  if ((rc = keep_on_device(R.d_leaf_handle, t.leaf_handle.data(), t.leaf_handle.size() * 4, tot))) return rc;
  if ((rc = keep_on_device(R.d_leaf_where, t.leaf_where.data(), t.leaf_where.size() * 4, tot))) return rc;
  if ((rc = keep_on_device(R.d_node_where, t.node_where.data(), t.node_where.size() * 4, tot))) return rc;
  if ((rc = keep_on_device(R.d_level_nodes, t.level_nodes.data(), t.level_nodes.size() * 4, tot))) return rc;
  if ((rc = keep_on_device(R.d_wv, nullptr, 12 * (size_t)hs.nv, tot))) return rc;
  if ((rc = keep_on_device(R.d_vnn, nullptr, 12 * (size_t)hs.nv, tot))) return rc;
  if ((rc = keep_on_device(R.d_face, nullptr, sizeof(FaceWords) * (size_t)hs.nf, tot))) return rc;
  if ((rc = keep_on_device(R.d_fmat, nullptr, 4 * (size_t)hs.nf, tot))) return rc;
  if ((rc = keep_on_device(R.d_slotbox, nullptr, 24 * hs.tris.size(), tot))) return rc;
  R.device_ready = true;
  return RT_OK;
}

void refit_release(rt_scene* s) {
  rt_scene::Refit& R = s->refit;
  void* bufs[] = {R.d_fidx, R.d_leaf_handle, R.d_leaf_where, R.d_node_where, R.d_level_nodes, R.d_wv,
                  R.d_vnn, R.d_av, R.d_slotbox, R.d_face, R.d_fmat};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  // ... and what the device update's pipeline keeps (rt_update_device.hip)
  void* more[] = {R.d_ov3, R.d_red, R.work.d_fv, R.work.d_fvt, R.work.d_ids, R.work.d_idt, R.work.d_flag, R.work.d_boxes,
                  R.work.d_child, R.d_seg_start, R.d_seg_box, R.d_seg_first, R.d_box_bounds};
  for (void* b : more)
    if (b) (void)hipFree(b);
  if (R.ev_in) (void)hipEventDestroy((hipEvent_t)R.ev_in);
  for (void* e : R.ev_t)
    if (e) (void)hipEventDestroy((hipEvent_t)e);
  RefitTopo keep = std::move(R.topo);
  R = rt_scene::Refit{};
  R.topo = std::move(keep);
}

// the three refit kernels on the scene's stream, over the per-vertex / per-face arrays on the device
int refit_launch(rt_scene* s, float pad, bool av) {
  rt_scene::Refit& R = s->refit;
  const HostScene& hs = s->hs;
  const RefitTopo& t = R.topo;
  const uint32_t nn = (uint32_t)hs.nodes.size(), nt = (uint32_t)hs.tris.size(), nf = (uint32_t)hs.nf;
  hipStream_t st = (hipStream_t)s->stream;
  auto blocks = [](uint32_t n) { return dim3((n + 255u) / 256u); };
  if (nt) {
    hipLaunchKernelGGL(k_refit_slots, blocks(nt), dim3(256), 0, st, nt, nf, s->d_tris, reinterpret_cast<float4*>(s->d_fshade),
                       R.d_slotbox, R.d_fidx, R.d_wv, R.d_vnn, R.d_face, R.d_fmat, av ? R.d_av : nullptr);
    HIPCHECK(hipGetLastError());
  }
  const uint32_t nl = (uint32_t)t.leaf_handle.size();
  if (nl) {
    hipLaunchKernelGGL(k_refit_leaves, blocks(nl), dim3(256), 0, st, nl, nt, nn, R.d_leaf_handle, R.d_leaf_where, R.d_slotbox,
                       s->d_nodes, pad);
    HIPCHECK(hipGetLastError());
  }
  for (size_t L = t.level_off.size() - 1; L-- > 0;) {
    const uint32_t n = t.level_off[L + 1] - t.level_off[L];
    if (!n) continue;
    hipLaunchKernelGGL(k_refit_level, blocks(n), dim3(256), 0, st, n, nn, R.d_level_nodes + t.level_off[L], R.d_node_where,
                       s->d_nodes);
    HIPCHECK(hipGetLastError());
  }
  return RT_OK;
}

int device_refit(rt_scene* s, const std::vector<TriRec64>& recs, float pad, double* upload_ms, double* refit_ms) {
  using clk = std::chrono::steady_clock;
  HIPCHECK(hipSetDevice(s->device));
  const auto t0 = clk::now();
  int rc = refit_prepare(s);
  if (rc) return rc;
  rt_scene::Refit& R = s->refit;
  const HostScene& hs = s->hs;
  const RefitTopo& t = R.topo;
  const uint32_t nn = (uint32_t)hs.nodes.size(), nt = (uint32_t)hs.tris.size(), nf = (uint32_t)hs.nf;
  static_assert(sizeof(f3) == 12, "packed vertices");
  if (hs.nv && (rc = h2d(R.d_wv, hs.wv.data(), 12 * (size_t)hs.nv))) return rc;
  if (hs.nv && (rc = h2d(R.d_vnn, hs.vnn.data(), 12 * (size_t)hs.nv))) return rc;
  if (nf) {
    std::unique_ptr<FaceWords[]> fw(new FaceWords[nf]);
    parallel_for(nf, [&](size_t b, size_t e) {
      for (size_t f = b; f < e; f++) {
        const TriRec64& r = recs[f];
        fw[f] = FaceWords{r.nx, r.ny, r.nz, r.dist, r.rank, r.box};
      }
    });
    if ((rc = h2d(R.d_face, fw.get(), sizeof(FaceWords) * (size_t)nf))) return rc;
    if ((rc = h2d(R.d_fmat, hs.fmat.data(), 4 * (size_t)nf))) return rc;
    if (!hs.av.empty()) {  // only scenes with a tilted normal carry the accept-region triangles (36 B per face)
      if ((rc = keep_on_device(R.d_av, hs.av.data(), 36 * (size_t)nf, s->device_bytes))) return rc;
    }
  }
  *upload_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  hipStream_t st = (hipStream_t)s->stream;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  struct Events { hipEvent_t *a, *b; ~Events() { if (*a) (void)hipEventDestroy(*a); if (*b) (void)hipEventDestroy(*b); } } ev_{&e0, &e1};
  HIPCHECK(hipEventCreate(&e0));
  HIPCHECK(hipEventCreate(&e1));
  HIPCHECK(hipEventRecord(e0, st));
  if ((rc = refit_launch(s, pad, !hs.av.empty()))) return rc;
  HIPCHECK(hipEventRecord(e1, st));
  HIPCHECK(hipStreamSynchronize(st));
  float ms = 0.0f;
  HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
  *refit_ms = ms;
  return RT_OK;
}

// after a host refit (geometry the device path does not take): the three record arrays in their device form
int device_reupload(rt_scene* s) {
  HIPCHECK(hipSetDevice(s->device));
  const HostScene& hs = s->hs;
  const size_t nn = hs.nodes.size(), nt = hs.tris.size();
  int rc;
  if (nn) {
    std::unique_ptr<Node64[]> nodes(new Node64[nn]);
    device_node_image(hs, nodes.get());
    if ((rc = h2d(s->d_nodes, nodes.get(), nn * 64))) return rc;
  }
  if (nt) {
    if ((rc = h2d(s->d_tris, hs.tris.data(), nt * 64))) return rc;
    std::unique_ptr<float[]> fsh(new float[12 * nt]);
    device_fshade_image(hs, fsh.get());
    if ((rc = h2d(s->d_fshade, fsh.get(), 48 * nt))) return rc;
  }
  return RT_OK;
}

// a device buffer replaced by one of another size (the scene's streams are drained)
template <class T>
static int resize_buffer(T*& p, size_t& bytes, size_t want, int64_t& total) {
  want = std::max<size_t>(want, 16);
  if (want == bytes) return RT_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  total -= (int64_t)bytes;
  bytes = 0;
  HIPCHECK(hipMalloc((void**)&p, want));
  bytes = want;
  total += (int64_t)want;
  return RT_OK;
}

int device_update_rest(rt_scene* s, bool replace4, bool boxes_changed) {
  HIPCHECK(hipSetDevice(s->device));
  const HostScene& hs = s->hs;
  int rc;
  const std::vector<float> rb = refbox_image(hs);
  if ((rc = resize_buffer(s->d_refbox, s->refbox_bytes, rb.size() * 4, s->device_bytes))) return rc;
  if (!rb.empty() && (rc = h2d(s->d_refbox, rb.data(), rb.size() * 4))) return rc;
  const std::vector<DevMat> dm = mats_image(hs);  // (as many as before: the buffer stays)
  if (!dm.empty() && (rc = h2d(s->d_mats, dm.data(), dm.size() * sizeof(DevMat)))) return rc;
  if (replace4) {
    const size_t b4 = hs.nodes4.size() * sizeof(Node4Q);
    if ((rc = resize_buffer(s->d_nodes4, s->nodes4_bytes, b4, s->device_bytes))) return rc;
    if (b4 && (rc = h2d(s->d_nodes4, hs.nodes4.data(), b4))) return rc;
  }
  // the replicas: the changed regions copied from device 0, the cached scalars and flags refreshed
  const size_t rec_bytes = (hs.nodes.size() + hs.tris.size()) * 64;
  for (auto& rp : s->replicas) {
    rt_scene* r = rp.get();
    HIPCHECK(hipSetDevice(r->device));
    hipStream_t st = (hipStream_t)build_stream(r->device);
    if (!st) { set_error("no build stream on device %d", r->device); return RT_ERR_HIP; }
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};
    if ((rc = resize_buffer(r->d_refbox, r->refbox_bytes, rb.size() * 4, r->device_bytes))) return rc;
    if (replace4 && (rc = resize_buffer(r->d_nodes4, r->nodes4_bytes, hs.nodes4.size() * sizeof(Node4Q), r->device_bytes))) return rc;
    if (rec_bytes && (rc = replica_copy(r->d_nodes, r->device, s->d_nodes, s->device, rec_bytes, st))) return rc;
    if ((rc = replica_copy(r->d_fshade, r->device, s->d_fshade, s->device, s->fshade_bytes, st))) return rc;
    if ((rc = replica_copy(r->d_refbox, r->device, s->d_refbox, s->device, s->refbox_bytes, st))) return rc;
    if ((rc = replica_copy(r->d_mats, r->device, s->d_mats, s->device, s->mats_bytes, st))) return rc;
    if (replace4 && (rc = replica_copy(r->d_nodes4, r->device, s->d_nodes4, s->device, s->nodes4_bytes, st))) return rc;
    HIPCHECK(hipStreamSynchronize(st));
    r->static_pad = s->static_pad;
    r->cert_origin_max = s->cert_origin_max;
    if (boxes_changed) r->box_colors.clear();
    r->face_boxcolor_valid = false;
    r->ray_bounds_valid = false;
    r->lpt.valid = false;
  }
  HIPCHECK(hipSetDevice(s->device));
  return RT_OK;
}

// hs.nodes / hs.tris from the device after a device refit: the boxes and order bits of the device form go back
// into the host form (whose handles never changed), the slot records are the same bytes
int host_mirror(const rt_scene* cs) {
  if (!cs->host_stale) return RT_OK;
  rt_scene* s = const_cast<rt_scene*>(cs);
  HIPCHECK(hipSetDevice(s->device));
  HostScene& hs = s->hs;
  const size_t nn = hs.nodes.size(), nt = hs.tris.size();
  int rc;
  if (nn) {
    std::unique_ptr<Node64[]> dev(new Node64[nn]);
    if ((rc = d2h(dev.get(), s->d_nodes, nn * 64))) return rc;
    parallel_for(nn, [&](size_t b, size_t e) {
      for (size_t i = b; i < e; i++) {
        Node64& h = hs.nodes[i];
        memcpy(&h, &dev[i], 48);  // the two child boxes
        h.pad0 = (dev[i].pad0 & 0x3Fu) | ((dev[i].pad1 & 0x3u) << 6);
      }
    });
  }
  if (nt && (rc = d2h(hs.tris.data(), s->d_tris, nt * 64))) return rc;
  s->host_stale = false;
  return RT_OK;
}

// hs's per-vertex / per-face arrays from what rt_scene_update_device keeps on the device: nothing is recomputed
int host_mirror_geometry(const rt_scene* cs) {
  if (!cs->geom_stale) return RT_OK;
  rt_scene* s = const_cast<rt_scene*>(cs);
  HIPCHECK(hipSetDevice(s->device));
  HostScene& hs = s->hs;
  rt_scene::Refit& R = s->refit;
  const size_t nv = (size_t)hs.nv, nf = (size_t)hs.nf;
  int rc;
  hs.ov3.resize(3 * nv);
  hs.wv.resize(nv);
  hs.vnn.resize(nv);
  if (nv) {
    if ((rc = d2h(hs.ov3.data(), R.d_ov3, 12 * nv))) return rc;
    if ((rc = d2h(hs.wv.data(), R.d_wv, 12 * nv))) return rc;
    if ((rc = d2h(hs.vnn.data(), R.d_vnn, 12 * nv))) return rc;
  }
  hs.fnn.resize(nf);
  hs.fdist.resize(nf);
  hs.face_rank.assign(nf, 0);
  hs.face_box.assign(nf, 0);
  hs.av.clear();
  if (nf) {
    std::unique_ptr<FaceWords[]> fw(new FaceWords[nf]);
    if ((rc = d2h(fw.get(), R.d_face, sizeof(FaceWords) * nf))) return rc;
    parallel_for(nf, [&](size_t b, size_t e) {
      for (size_t f = b; f < e; f++) {
        hs.fnn[f] = f3{fw[f].nx, fw[f].ny, fw[f].nz};
        hs.fdist[f] = fw[f].dist;
        hs.face_rank[f] = fw[f].rank;
        hs.face_box[f] = fw[f].box & kBoxIndexMask;
      }
    });
    if (R.tilted) {
      hs.av.resize(3 * nf);
      if ((rc = d2h(hs.av.data(), R.d_av, 36 * nf))) return rc;
    }
    std::vector<int32_t> ids(nf);
    if ((rc = d2h(ids.data(), R.work.d_ids, 4 * nf))) return rc;
    for (size_t i = 0; i < hs.boxes.size() && i < R.boxes.size(); i++) {
      const DBox& d = R.boxes[i];
      if (d.start < 0 || d.count < 0 || (size_t)d.start + (size_t)d.count > nf) { set_error("host mirror: bad box segment"); return RT_ERR_HIP; }
      hs.boxes[i].faces.assign(ids.begin() + d.start, ids.begin() + d.start + d.count);
    }
  }
  s->geom_stale = false;
  return RT_OK;
}

}  // namespace rt

using namespace rt;

extern "C" int rt_debug_scene_records(rt_scene* s, int32_t which, int64_t capacity_bytes, void* out, int64_t* n_bytes) {
  if (!s || !n_bytes) { set_error("rt_debug_scene_records: null argument"); return RT_ERR_INVALID; }
  if (which < 0 || which > 2) { set_error("rt_debug_scene_records: which = %d (0 nodes, 1 triangle records, 2 shading records)", which); return RT_ERR_INVALID; }
  const HostScene& hs = s->hs;
  const size_t bytes = which == 0 ? hs.nodes.size() * 64 : which == 1 ? hs.tris.size() * 64 : hs.tris.size() * 48;
  *n_bytes = (int64_t)bytes;
  if (!out) return RT_OK;
  if (capacity_bytes < (int64_t)bytes) { set_error("rt_debug_scene_records: %lld bytes for %zu", (long long)capacity_bytes, bytes); return RT_ERR_INVALID; }
  if (!bytes) return RT_OK;
  if (s->device != RT_DEVICE_NONE) {
    HIPCHECK(hipSetDevice(s->device));
    const void* src = which == 0 ? (const void*)s->d_nodes : which == 1 ? (const void*)s->d_tris : (const void*)s->d_fshade;
    return d2h(out, src, bytes);
  }
  // a host-only scene: the images device_upload would send (built in aligned storage, then copied out)
  if (which == 0) {
    std::unique_ptr<Node64[]> nodes(new Node64[hs.nodes.size()]);
    device_node_image(hs, nodes.get());
    memcpy(out, nodes.get(), bytes);
  } else if (which == 1) {
    memcpy(out, hs.tris.data(), bytes);
  } else {
    std::unique_ptr<float[]> fsh(new float[12 * hs.tris.size()]);
    device_fshade_image(hs, fsh.get());
    memcpy(out, fsh.get(), bytes);
  }
  return RT_OK;
}
