// rt_update_device.hip -- rt_scene_update_device: a scene's geometry replaced from arrays in device memory, every
// stage of rt_scene_update on the device (devices[0]). The kernels (rt_update_kernels.h) re-state the host stages
// from the shared RT_HD functions; the partition is rt_boxes.hip's own (ref_box_passes, over the caller's vertices);
// the refit kernels are rt_refit.hip's (refit_launch); the tail is rt_update.cpp's (update_finish). One stream --
// the scene's -- carries everything, behind an event recorded on the caller's stream. The host sees per update: the
// partition's pass loop (its first wait also brings the reduction words: the non-finite flag, the tilted flag, the
// largest object coordinate and the bounds the static pad is taken from), then nothing until the final wait (the
// boxes' segments go up from staging arrays kept with the scene). Coordinates the device stages do not take (not finite, or beyond 1e30) and face-less scenes are
// downloaded and handed to rt_scene_update: the only host fallback.
#include <chrono>
#include <cstring>

#include "rt_device.h"
#include "rt_update_kernels.h"

namespace rt {
namespace {

template <class T>
int keep(T*& p, size_t bytes, int64_t& total) {
  if (p) return RT_OK;
  bytes = std::max<size_t>(bytes, 16);
  HIPCHECK(hipMalloc((void**)&p, bytes));
  total += (int64_t)bytes;
  return RT_OK;
}

// segment / bounds arrays for at least n boxes (geometric growth: no allocation once the box count has settled)
int reserve_boxes(rt_scene* s, size_t n) {
  rt_scene::Refit& R = s->refit;
  if (n <= R.seg_cap) return RT_OK;
  size_t cap = std::max<size_t>(R.seg_cap, 1024);
  while (cap < n) cap *= 2;
  void* old[] = {R.d_seg_start, R.d_seg_box, R.d_seg_first, R.d_box_bounds};
  for (void* b : old)
    if (b) (void)hipFree(b);
  s->device_bytes -= (int64_t)(36 * R.seg_cap);
  R.d_seg_start = nullptr, R.d_seg_box = nullptr, R.d_seg_first = nullptr, R.d_box_bounds = nullptr, R.seg_cap = 0;
  HIPCHECK(hipMalloc((void**)&R.d_seg_start, 4 * cap));
  HIPCHECK(hipMalloc((void**)&R.d_seg_box, 4 * cap));
  HIPCHECK(hipMalloc((void**)&R.d_seg_first, 4 * cap));
  HIPCHECK(hipMalloc((void**)&R.d_box_bounds, 24 * cap));
  R.seg_cap = cap;
  s->device_bytes += (int64_t)(36 * cap);
  return RT_OK;
}

// the first device update's allocations (the scene's device is current)
int update_prepare(rt_scene* s) {
  rt_scene::Refit& R = s->refit;
  int rc;
  if ((rc = refit_prepare(s))) return rc;
  if (R.update_ready) return RT_OK;
  const HostScene& hs = s->hs;
  const size_t nv = (size_t)hs.nv, nf = (size_t)hs.nf;
  int64_t& tot = s->device_bytes;
  if ((rc = keep(R.d_ov3, 12 * nv, tot))) return rc;
  if ((rc = keep(R.d_av, 36 * nf, tot))) return rc;
  if ((rc = keep(R.d_red, 4 * UR_WORDS, tot))) return rc;
  BoxWork& w = R.work;
  if ((rc = keep(w.d_fv, 36 * nf, tot))) return rc;
  if ((rc = keep(w.d_fvt, 36 * nf, tot))) return rc;
  if ((rc = keep(w.d_ids, 4 * nf, tot))) return rc;
  if ((rc = keep(w.d_idt, 4 * nf, tot))) return rc;
  if ((rc = keep(w.d_flag, 4, tot))) return rc;
  if (!w.cap) {
    if ((rc = keep(w.d_boxes, 1024 * sizeof(DBox), tot))) return rc;
    if ((rc = keep(w.d_child, 1024 * sizeof(DBox), tot))) return rc;
    w.cap = 1024;
  }
  // a pass with more boxes than the records hold: the stream is idle between passes, so the old pair is freed
  w.grow = [s](BoxWork& bw, size_t cap) -> int {
    if (bw.d_boxes) (void)hipFree(bw.d_boxes);
    if (bw.d_child) (void)hipFree(bw.d_child);
    s->device_bytes -= (int64_t)(2 * bw.cap * sizeof(DBox));
    bw.d_boxes = nullptr, bw.d_child = nullptr, bw.cap = 0;
    HIPCHECK(hipMalloc((void**)&bw.d_boxes, cap * sizeof(DBox)));
    HIPCHECK(hipMalloc((void**)&bw.d_child, cap * sizeof(DBox)));
    bw.cap = cap;
    s->device_bytes += (int64_t)(2 * cap * sizeof(DBox));
    return RT_OK;
  };
  if ((rc = reserve_boxes(s, 1))) return rc;
  if (!R.ev_in) HIPCHECK(hipEventCreateWithFlags((hipEvent_t*)&R.ev_in, hipEventDisableTiming));
  for (void*& e : R.ev_t)
    if (!e) HIPCHECK(hipEventCreate((hipEvent_t*)&e));
  if (!R.fmat_sent && nf) {  // (the material ids never change)
    if ((rc = h2d(R.d_fmat, hs.fmat.data(), 4 * nf))) return rc;
    R.fmat_sent = true;
  }
  R.update_ready = true;
  return RT_OK;
}

// the host path over a download of the caller's arrays (the scene's streams are quiet, the arrays complete)
int update_through_host(rt_scene* s, const rt_device_geometry* g, const float* M, const std::vector<rt_material>& mats,
                        rt_update_stats* stats) {
  const HostScene& hs = s->hs;
  const size_t nv = (size_t)hs.nv, nf = (size_t)hs.nf;
  std::vector<float> v4(4 * nv), vn3(3 * nv), fn3(3 * nf);
  int rc;
  if (nv && (rc = d2h(v4.data(), g->vertices, 16 * nv))) return rc;
  if (nv && (rc = d2h(vn3.data(), g->vertex_normals, 12 * nv))) return rc;
  if (nf && (rc = d2h(fn3.data(), g->face_normals, 12 * nf))) return rc;
  const std::vector<uint32_t> fidx = hs.fidx;  // (copies: rt_scene_update writes the scene while it reads these)
  const std::vector<int32_t> fmat = hs.fmat;
  rt_mesh_desc d;
  memset(&d, 0, sizeof d);
  d.n_vertices = hs.nv, d.n_faces = hs.nf, d.n_materials = (int32_t)mats.size();
  d.vertices = v4.data(), d.vertex_normals = vn3.data(), d.face_normals = fn3.data();
  d.face_vertex_ids = fidx.data(), d.face_material_ids = fmat.data();
  d.materials = mats.data();
  memcpy(d.shape_model_matrix, M, 64);
  return rt_scene_update(s, &d, stats);
}

}  // namespace
}  // namespace rt

using namespace rt;

extern "C" int rt_scene_update_device(rt_scene* s, const rt_device_geometry* g, void* hip_stream, rt_update_stats* stats) {
  using clk = std::chrono::steady_clock;
  const char* who = "rt_scene_update_device";
  if (!s || !g) { set_error("%s: null argument", who); return RT_ERR_INVALID; }
  HostScene& hs = s->hs;
  if ((hs.nv > 0 && (!g->vertices || !g->vertex_normals)) || (hs.nf > 0 && !g->face_normals)) {
    set_error("%s: null geometry array", who);
    return RT_ERR_INVALID;
  }
  if (s->is_replica) { set_error("%s: a replica is updated through its scene", who); return RT_ERR_INVALID; }
  if (s->opts.wide_tree) {
    set_error("%s: scenes with the fp32 4-wide tree (wide_tree = 1) are not updated in this version", who);
    return RT_ERR_UNSUPPORTED;
  }
  if (s->device == RT_DEVICE_NONE) { set_error("%s: the scene is host-only", who); return RT_ERR_NO_DEVICE; }
  int rc;
  HIPCHECK(hipSetDevice(s->device));
  if ((rc = check_device_pointer(s, g->vertices, who, "vertices"))) return rc;
  if ((rc = check_device_pointer(s, g->vertex_normals, who, "vertex_normals"))) return rc;
  if ((rc = check_device_pointer(s, g->face_normals, who, "face_normals"))) return rc;
  // ---- nothing above touched the scene or a stream ----
  hipStream_t st = (hipStream_t)s->stream;
  if ((rc = update_quiesce(s))) return rc;
  if (!s->refit.topo.ready) {  // (before the first update of any kind the host nodes are create's own)
    if ((rc = host_mirror(s))) return rc;
    refit_topology(hs, s->refit.topo);
  }
  if ((rc = update_prepare(s))) return rc;
  rt_scene::Refit& R = s->refit;
  // the caller's arrays are read behind everything queued so far on the caller's stream
  HIPCHECK(hipEventRecord((hipEvent_t)R.ev_in, (hipStream_t)hip_stream));
  HIPCHECK(hipStreamWaitEvent(st, (hipEvent_t)R.ev_in, 0));
  const auto t0 = clk::now();
  float M[16];
  memcpy(M, g->shape_model_matrix ? g->shape_model_matrix : hs.M, 64);
  std::vector<rt_material> mats = hs.mats;
  if (g->materials) mats.assign(g->materials, g->materials + hs.mats.size());
  const uint32_t nv = (uint32_t)hs.nv, nf = (uint32_t)hs.nf, nt = (uint32_t)hs.tris.size();
  if (nf == 0 || nv == 0) {  // (as a face-less rt_scene_create: nothing for the device stages to do)
    HIPCHECK(hipStreamSynchronize(st));
    return update_through_host(s, g, M, mats, stats);
  }
  rt_update_stats us;
  memset(&us, 0, sizeof us);
  hipEvent_t* ev = reinterpret_cast<hipEvent_t*>(R.ev_t);
  auto blocks = [](uint32_t n) { return dim3((n + 255u) / 256u); };
  // ---- invariants: per vertex, per face, the slots' bounds ----
  Mat16 Mk;
  memcpy(Mk.m, M, 64);
  HIPCHECK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(k_upd_init, dim3(1), dim3(64), 0, st, R.d_red);
  hipLaunchKernelGGL(k_upd_vertices, blocks(nv), dim3(256), 0, st, nv, g->vertices, g->vertex_normals, Mk, R.d_ov3, R.d_wv, R.d_vnn,
                     R.d_red);
  hipLaunchKernelGGL(k_upd_faces, blocks(nf), dim3(256), 0, st, nf, nv, (const uint32_t*)R.d_fidx, g->face_normals,
                     (const float*)R.d_wv, R.d_face, R.d_av, R.d_red);
  if (nt)
    hipLaunchKernelGGL(k_upd_slot_bounds, blocks(nt), dim3(256), 0, st, nt, nf, nv, (const TriRec64*)s->d_tris,
                       (const uint32_t*)R.d_fidx, (const float*)R.d_wv, (const float*)R.d_av, R.d_red);
  HIPCHECK(hipGetLastError());
  uint32_t red[UR_WORDS] = {};
  HIPCHECK(hipMemcpyAsync(red, R.d_red, sizeof red, hipMemcpyDeviceToHost, st));  // (lands with the partition's first wait)
  HIPCHECK(hipEventRecord(ev[1], st));
  // ---- the partition over the caller's vertices ----
  bool nonfinite = false;
  std::vector<DBox> boxes;
  if ((rc = ref_box_passes(st, g->vertices, R.d_fidx, (int)nf, s->opts.min_faces, s->opts.max_boxes, R.work, boxes, &nonfinite)))
    return rc;
  if (nonfinite || red[UR_NONFINITE]) {
    // d_wv / d_vnn / d_face were written, the records and the tree were not: the host path rewrites all of them
    HIPCHECK(hipStreamSynchronize(st));
    return update_through_host(s, g, M, mats, stats);
  }
  HIPCHECK(hipEventRecord(ev[2], st));
  // ---- from here the scene changes ----
  const size_t boxes_before = hs.boxes.size();
  const size_t nb = boxes.size();
  memcpy(hs.M, M, 64);
  affinv(hs.M, hs.Minv);
  linear_of(hs.Minv, hs.MS);
  hs.mats = mats;
  hs.boxes.resize(nb);
  for (size_t i = 0; i < nb; i++) {  // bounds, shape and failed now; the face lists with the lazy mirror
    const DBox& d = boxes[i];
    RefBox& b = hs.boxes[i];
    for (int a = 0; a < 3; a++) {
      b.low[a] = d.low[a];
      b.high[a] = d.high[a];
      b.shape[a] = d.high[a] - d.low[a];
      b.failed[a] = d.failed[a] != 0;
    }
    b.faces.clear();
  }
  s->box_builder_used = RT_BOXES_GPU;
  s->geom_stale = true;
  s->host_stale = true;
  R.tilted = red[UR_TILTED] != 0;
  float lo[3], hi[3];
  for (int k = 0; k < 3; k++) {
    lo[k] = float_of_key(red[(R.tilted ? UR_ALO : UR_WLO) + k]);
    hi[k] = float_of_key(red[(R.tilted ? UR_AHI : UR_WHI) + k]);
  }
  const float pad = nt ? static_pad_of_bounds(lo, hi) : 0.0f;
  float max_abs;
  memcpy(&max_abs, &red[UR_MAXABS], 4);
  const float Ro = cert_origin_of(hs.M, max_abs);
  s->static_pad = pad;
  s->cert_origin_max = Ro;
  // ---- ranks, flags ----
  {
    // the staging arrays live with the scene: the copies below read them until the call's final wait
    std::vector<uint32_t>&first = R.h_first, &order = R.h_seg_box, &seg_first = R.h_seg_first;
    std::vector<int32_t>& seg_start = R.h_seg_start;
    std::vector<float>& bounds = R.h_box_bounds;
    first.resize(nb), order.resize(nb), seg_first.resize(nb), seg_start.resize(nb), bounds.resize(6 * nb);
    uint32_t run = 0;
    for (size_t i = 0; i < nb; i++) { first[i] = run; run += (uint32_t)boxes[i].count; order[i] = (uint32_t)i; }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return boxes[a].start < boxes[b].start; });
    for (size_t i = 0; i < nb; i++) {
      seg_start[i] = boxes[order[i]].start;
      seg_first[i] = first[order[i]];
      memcpy(&bounds[6 * i], boxes[i].low, 12);
      memcpy(&bounds[6 * i + 3], boxes[i].high, 12);
    }
    if ((rc = reserve_boxes(s, nb))) return rc;
    HIPCHECK(hipMemcpyAsync(R.d_seg_start, seg_start.data(), 4 * nb, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(R.d_seg_box, order.data(), 4 * nb, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(R.d_seg_first, seg_first.data(), 4 * nb, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(R.d_box_bounds, bounds.data(), 24 * nb, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_upd_ranks, blocks(nf), dim3(256), 0, st, nf, (uint32_t)nb, (const int32_t*)R.d_seg_start,
                       (const uint32_t*)R.d_seg_box, (const uint32_t*)R.d_seg_first, (const int32_t*)R.work.d_ids, R.d_face);
    hipLaunchKernelGGL(k_upd_face_words, blocks(nf), dim3(256), 0, st, nf, nv, (uint32_t)nb, (const uint32_t*)R.d_fidx,
                       (const float*)R.d_ov3, (const float*)R.d_wv, (const float*)R.d_vnn, (const float*)R.d_box_bounds, Ro,
                       R.d_face);
    HIPCHECK(hipGetLastError());
  }
  R.boxes = boxes;
  HIPCHECK(hipEventRecord(ev[3], st));
  // ---- the refit ----
  if ((rc = refit_launch(s, pad, R.tilted))) return rc;
  HIPCHECK(hipEventRecord(ev[4], st));
  HIPCHECK(hipStreamSynchronize(st));
  float ms[4] = {0, 0, 0, 0};
  for (int k = 0; k < 4; k++) HIPCHECK(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
  us.prep_ms = ms[0], us.boxes_ms = ms[1], us.records_ms = ms[2], us.refit_ms = ms[3];
  us.bounds_on_device = 1;
  // ---- the tail of every update ----
  const auto t1 = clk::now();
  if ((rc = update_finish(s, boxes_before))) return rc;
  us.upload_ms = std::chrono::duration<double, std::milli>(clk::now() - t1).count();
  us.total_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  if (stats) {
    double cost[4];
    if ((rc = rt_debug_tree_cost(s, 0.7, cost))) return rc;
    us.sah_cost = cost[0];
    *stats = us;
  }
  return RT_OK;
}
