// rt_host.cpp -- the host-only C ABI of the MI355X ray-traversal library around scene preparation: errors and
// debug knobs, rt_scene_create (which runs the stages: invariants, reference boxes -- rt_refboxes.cpp or
// rt_boxes.hip --, the traversal tree -- rt_builders.cpp or rt_layout.cpp's device builders --, upload), the
// scene accessors, the debug entry points of the math, record-layout and frame-plan code, and the ray keys.
// Ingest is rt_ingest.cpp, camera / lights / PPM output rt_view.cpp, validation rt_validate.cpp.
//
// Reference semantics restated here (file:line in plindhorst/Ray-Tracing-Project):
//   scene defaults      src/flyscene.hpp:168-169
//   per-face invariants src/flyscene.cpp:449-450,459,574-577,599
//   box colours         src/BoundingBox.cpp:163-165
#include <atomic>
#include <chrono>
#include <climits>
#include <cstdarg>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>

#include "rt_dispatch.h"
#include "rt_host.h"

using rt::f3;

namespace rt {
static thread_local std::string g_err;
static std::atomic<bool> g_debug_env{false};
void set_debug_env(bool on) { g_debug_env.store(on); }
const char* debug_env(const char* name) { return g_debug_env.load(std::memory_order_relaxed) ? getenv(name) : nullptr; }
int knob_int(const char* name, int def, int lo, int hi) {
  const char* e = debug_env(name);
  return e ? std::max(lo, std::min(hi, atoi(e))) : def;
}

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
}
}  // namespace rt

extern "C" const char* rt_last_error(void) { return rt::g_err.c_str(); }
extern "C" int rt_version(void) { return RT_API_VERSION; }

// [0, n) in contiguous chunks on up to 16 threads (one below 64k items): f(begin, end)
void rt::parallel_for(size_t n, const std::function<void(size_t, size_t)>& f) {
  rt::parallel_chunks(n, [&](size_t b, size_t e, int) { f(b, e); });
}

extern "C" void rt_scene_opts_default(rt_scene_opts* o) {
  memset(o, 0, sizeof *o);
  o->device = -1;
  o->min_faces = 300;       // flyscene.hpp:168
  o->max_boxes = INT32_MAX; // flyscene.hpp:169
  o->leaf_size = 0;
  o->frames_in_flight = 4;
  o->builder = RT_BUILDER_SBVH_GPU;  // host RT_BUILDER_SBVH when there is no device
  o->box_builder = RT_BOXES_GPU;     // host partition when there is no device (same boxes and order)
  for (int k = 0; k < 3; k++) { o->default_material.ka[k] = 0.2f; o->background[k] = 0.9f; }
  o->default_material.kd[0] = 0.9f; o->default_material.kd[1] = 0.9f; o->default_material.kd[2] = 0.0f;
  o->default_material.shininess = 0.0f;
  o->default_material.dissolve = 0.0f;
}

// =====================================================================================================
// Scene creation (host preparation + device upload)
// =====================================================================================================
// hoisted per-vertex / per-face invariants (same expressions as flyscene.cpp:449-450,459,574-577,599), of
// rt_scene_create and rt_scene_update alike: hs holds the topology (nv, nf, fidx)
void rt::scene_invariants(rt::HostScene& hs, const rt_mesh_desc* d) {
  memcpy(hs.M, d->shape_model_matrix, 64);
  rt::affinv(hs.M, hs.Minv);
  rt::linear_of(hs.Minv, hs.MS);
  hs.wv.resize(hs.nv);
  hs.vnn.resize(hs.nv);
  hs.ov3.resize(3 * (size_t)hs.nv);
  rt::parallel_for((size_t)hs.nv, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) {
      const float* v = d->vertices + 4 * i;
      memcpy(&hs.ov3[3 * i], v, 12);
      hs.wv[i] = rt::affv3(hs.M, f3{v[0] / v[3], v[1] / v[3], v[2] / v[3]});
      const float* n = d->vertex_normals + 3 * i;
      hs.vnn[i] = rt::normalized(f3{n[0], n[1], n[2]});
    }
  });
  hs.fnn.resize(hs.nf);
  hs.fdist.resize(hs.nf);
  rt::parallel_for((size_t)hs.nf, [&](size_t b, size_t e) {
    for (size_t f = b; f < e; f++) {
      const float* n = d->face_normals + 3 * f;
      hs.fnn[f] = rt::normalized(f3{n[0], n[1], n[2]});
      hs.fdist[f] = rt::dot(hs.fnn[f], hs.wv[hs.fidx[3 * f]]);
    }
  });
  rt::accept_region(hs);
}

// The reference-box partition by the scene's box_builder, with the ranks: on device `dev` (-1: none) where asked
// for and possible, else on the host (a face-less scene, non-finite coordinates). v4: the description's vertices.
int rt::partition_ref_boxes(rt_scene* s, int dev, const float* v4) {
  rt::HostScene& hs = s->hs;
  bool boxes_done = false;
  s->box_builder_used = RT_BOXES_HOST;
  if (s->opts.box_builder == RT_BOXES_GPU && dev >= 0 && hs.nf > 0) {  // (a face-less scene: host)
    bool nonfinite = false;
    const int rc = rt::gpu_build_ref_boxes(dev, hs, v4, s->opts.min_faces, s->opts.max_boxes, &s->boxes_gpu_ms, &nonfinite);
    if (rc) return rc;
    if (!nonfinite) {
      rt::PhaseTimer pr("boxes-gpu");
      rt::assign_box_ranks(hs);
      pr.mark("box_ranks");
      boxes_done = true;
      s->box_builder_used = RT_BOXES_GPU;
    }
  }
  if (!boxes_done) rt::build_ref_boxes(hs, v4, s->opts.min_faces, s->opts.max_boxes);
  return RT_OK;
}

extern "C" int rt_scene_create(const rt_mesh_desc* d, const rt_scene_opts* opts, rt_scene** out) {
  if (!d || !out) { rt::set_error("rt_scene_create: null argument"); return RT_ERR_INVALID; }
  *out = nullptr;
  if (d->n_vertices < 0 || d->n_faces < 0 || (d->n_faces && (!d->face_vertex_ids || !d->face_normals || !d->face_material_ids)) ||
      (d->n_vertices && (!d->vertices || !d->vertex_normals))) {
    rt::set_error("rt_scene_create: invalid mesh description");
    return RT_ERR_INVALID;
  }
  // leaf handles hold the first triangle slot in 27 bits (the all-ones handle is the traversal's pop
  // marker) and records are addressed by 32-bit byte offsets (kMaxFaces, rt_internal.h)
  static_assert(rt::kMaxFaces < rt::kLeafFirstMask - rt::kMaxLeaf, "leaf handle range");
  if ((int64_t)d->n_faces > (int64_t)rt::kMaxFaces) {
    rt::set_error("rt_scene_create: %d faces exceed the %u-face limit", d->n_faces, rt::kMaxFaces);
    return RT_ERR_INVALID;
  }
  auto t0 = std::chrono::steady_clock::now();
  std::unique_ptr<rt_scene> s(new rt_scene());
  if (opts) s->opts = *opts; else rt_scene_opts_default(&s->opts);
  if (s->opts.min_faces <= 0) s->opts.min_faces = 300;
  s->opts.frames_in_flight = std::max(1, std::min(s->opts.frames_in_flight, (int32_t)rt_scene::kMaxSlots));
  if (s->opts.max_boxes <= 0) s->opts.max_boxes = INT32_MAX;
  if (s->opts.device == RT_DEVICE_NONE && s->opts.n_devices != 0) {
    rt::set_error("rt_scene_create: a host-only scene (RT_DEVICE_NONE) lists no devices");
    return RT_ERR_INVALID;
  }
  if (s->opts.device != RT_DEVICE_NONE) {  // device list -> opts.device = devices[0] (builds and uploads there)
    const int rc = rt::resolve_devices(s->opts);
    if (rc) return rc;
  }
  // the device the boxes and the tree are built on (-1: none, everything on the host)
  const int dev = s->opts.device == RT_DEVICE_NONE ? -1 : s->opts.device >= 0 ? s->opts.device : rt::current_device();
  const int leaf = s->opts.leaf_size > 0 ? s->opts.leaf_size : 4;
  // the device's first-use initialisation overlaps the host preparation below (joined before the first
  // device step, or on any return)
  struct Joiner {
    std::thread t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } warm;
  if (dev >= 0) {
    try {
      warm.t = std::thread(rt::device_warmup, dev);
    } catch (const std::exception&) {
      // no helper thread (resource limits): the device initialises at its first use instead
    }
  }
  rt::HostScene& hs = s->hs;
  hs.nv = d->n_vertices;
  hs.nf = d->n_faces;
  hs.fidx.assign(d->face_vertex_ids, d->face_vertex_ids + 3 * (size_t)hs.nf);
  hs.fmat.assign(d->face_material_ids, d->face_material_ids + hs.nf);
  hs.mats.assign(d->materials, d->materials + d->n_materials);
  for (int32_t f = 0; f < hs.nf; f++) {
    for (int k = 0; k < 3; k++)
      if (hs.fidx[3 * f + k] >= (uint32_t)hs.nv) {
        rt::set_error("face %d references vertex %u of %d", f, hs.fidx[3 * f + k], hs.nv);
        return RT_ERR_INVALID;
      }
    if (hs.fmat[f] >= d->n_materials || hs.fmat[f] < -1) {
      rt::set_error("face %d has material id %d (n_materials %d)", f, hs.fmat[f], d->n_materials);
      return RT_ERR_INVALID;
    }
  }
  rt::scene_invariants(hs, d);
  using clk = std::chrono::steady_clock;
  auto ms_since = [](clk::time_point a) { return std::chrono::duration<double, std::milli>(clk::now() - a).count(); };
  if (warm.t.joinable()) warm.t.join();
  s->prep_ms = ms_since(t0);
  auto t1 = clk::now();
  if (const int rc = rt::partition_ref_boxes(s.get(), dev, d->vertices)) return rc;
  s->boxes_ms = ms_since(t1);
  if (rt::debug_env("RT_TIMING"))
    fprintf(stderr, "[rt] boxes %.1f ms (%s, device %.1f ms), %zu boxes\n", s->boxes_ms,
            s->box_builder_used == RT_BOXES_GPU ? "gpu" : "host", s->boxes_gpu_ms, hs.boxes.size());
  auto t2 = clk::now();
  bool built = false;
  const int32_t builder = s->opts.builder;
  if (dev >= 0 && (builder == RT_BUILDER_SAH_GPU || builder == RT_BUILDER_SBVH_GPU))
    built = rt::build_bvh_sah_gpu(hs, dev, leaf, builder == RT_BUILDER_SBVH_GPU, &s->bvh_gpu_ms);
  if (dev >= 0 && builder == RT_BUILDER_PLOC_GPU) built = rt::build_bvh_ploc(hs, dev, leaf, &s->bvh_gpu_ms);
  if (dev >= 0 && builder == RT_BUILDER_LBVH_GPU) {
    // LBVH default leaf bound 1: the Morton tree's small subtrees are poor leaves (measured at 1M tris:
    // 1 -> 97% of the SAH tree's traversal rate, 4 -> 85%)
    built = rt::build_bvh_gpu(hs, dev, s->opts.leaf_size > 0 ? s->opts.leaf_size : 1, &s->bvh_gpu_ms);
  }
  if (built) s->builder_used = builder;
  if (!built) {  // host build: spatial splits for either SBVH builder, binned SAH for the rest
    const bool spatial = builder == RT_BUILDER_SBVH || builder == RT_BUILDER_SBVH_GPU;
    rt::build_bvh(hs, leaf, spatial);
    s->builder_used = spatial ? RT_BUILDER_SBVH : RT_BUILDER_SAH;
    if (rt::debug_env("RT_TIMING")) fprintf(stderr, "[rt] build_bvh %.1f ms\n", ms_since(t2));
    rt::build_bvh4(hs);
  }
  if (s->opts.wide_tree) rt::build_wide(hs);  // fp32 4-wide collapse of the binary tree (PRIMARY packets)
  s->bvh_ms = ms_since(t2);
  if (3 * hs.depth4 + 4 > rt::kStack4) hs.nodes4.clear();  // too deep for the wide stack: binary traversal
  if (hs.depth > rt::kMaxDepth + 2) {  // the wave stack holds 64 entries
    rt::set_error("BVH depth %d exceeds the traversal stack", hs.depth);
    return RT_ERR_UNSUPPORTED;
  }
  s->build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (s->opts.device != RT_DEVICE_NONE) {
    auto t3 = clk::now();
    int rc = rt::device_upload(s.get());
    if (rc) return rc;
    s->upload_ms = ms_since(t3);
    if (s->opts.n_devices > 1 && (rc = rt::device_replicate(s.get()))) return rc;
  }
  *out = s.release();
  return RT_OK;
}

extern "C" void rt_scene_destroy(rt_scene* s) {
  delete s;  // ~rt_scene releases the device replicas and this scene's device state (rt_device.hip)
}

extern "C" int rt_scene_get_info(const rt_scene* s, rt_scene_info* o) {
  if (!s || !o) { rt::set_error("rt_scene_get_info: null argument"); return RT_ERR_INVALID; }
  o->n_faces = s->hs.nf;
  o->n_vertices = s->hs.nv;
  o->n_ref_boxes = (int32_t)s->hs.boxes.size();
  o->bvh_nodes = (int32_t)s->hs.nodes.size();
  o->bvh_leaves = s->hs.leaves;
  o->bvh_depth = s->hs.depth;
  o->device_bytes = s->device_bytes;
  for (const auto& r : s->replicas) o->device_bytes += r->device_bytes;
  o->n_devices = s->device == RT_DEVICE_NONE ? 0 : 1 + (int32_t)s->replicas.size();
  o->replicate_ms = s->replicate_ms;
  o->build_ms = s->build_ms;
  o->device = s->device;
  o->prep_ms = s->prep_ms;
  o->boxes_ms = s->boxes_ms;
  o->bvh_ms = s->bvh_ms;
  o->upload_ms = s->upload_ms;
  o->builder = s->builder_used;
  o->bvh_gpu_ms = s->bvh_gpu_ms;
  o->box_builder = s->box_builder_used;
  o->boxes_gpu_ms = s->boxes_gpu_ms;
  {
    // the wide tree is uploaded only where its record offsets fit below kLeafBit (record_layout)
    uint64_t wb = 0;
    rt::record_layout(s->hs.nodes.size(), s->hs.tris.size(), s->hs.wide.size(), &wb);
    o->wide_nodes = wb ? (int32_t)s->hs.wide.size() : 0;
  }
  o->wide_depth = s->hs.depth_wide;
  return RT_OK;
}

// BoundingBox::setRandomColor (BoundingBox.cpp:163-165) per box in creation order. The three rand() calls
// are constructor arguments, whose evaluation order C++ leaves open; the reference built with g++ (this
// image's compiler, and x86-64 MSVC alike) evaluates them right to left: a box's first call is its blue
// channel (tests/golden/boxcolor_kat.bin, generated from that expression by oracle/boxcolor_kat.cpp).
extern "C" int rt_box_colors_random(int32_t n_boxes, rt_rand_state* rng, float* out3) {
  if (n_boxes < 0 || (n_boxes && !out3)) { rt::set_error("rt_box_colors_random: bad arguments"); return RT_ERR_INVALID; }
  rt_rand_state local;
  if (!rng) { rt_rand_seed(&local, 1); rng = &local; }
  for (int64_t b = 0; b < (int64_t)n_boxes; b++)
    for (int k = 2; k >= 0; k--) out3[3 * b + k] = (float)rt_rand(rng) / (float)2147483647;
  return RT_OK;
}

extern "C" int rt_scene_set_box_colors(rt_scene* s, const float* colors3) {
  if (!s) { rt::set_error("rt_scene_set_box_colors: null scene"); return RT_ERR_INVALID; }
  const int32_t nb = (int32_t)s->hs.boxes.size();
  std::vector<float> c(3 * (size_t)nb);
  if (colors3) memcpy(c.data(), colors3, c.size() * 4);
  else rt_box_colors_random(nb, nullptr, c.data());
  // frames in flight may still read the per-face table: it is rebuilt at the next box-colour frame,
  // after the scene's streams have drained (rt_frame.hip: ensure_face_boxcolor)
  for (auto& r : s->replicas) {  // every device of a multi-device scene renders with the same colours
    r->box_colors = c;
    r->face_boxcolor_valid = false;
  }
  s->box_colors.swap(c);
  s->face_boxcolor_valid = false;
  return RT_OK;
}

extern "C" int rt_scene_ref_boxes(const rt_scene* s, float* bounds6, int32_t* counts, int32_t* face_order) {
  if (!s) { rt::set_error("rt_scene_ref_boxes: null scene"); return RT_ERR_INVALID; }
  if (const int rc = rt::host_mirror_geometry(s)) return rc;  // (the boxes' face lists after a device update)
  size_t off = 0;
  for (size_t i = 0; i < s->hs.boxes.size(); i++) {
    const rt::RefBox& b = s->hs.boxes[i];
    if (bounds6) { memcpy(bounds6 + 6 * i, b.low, 12); memcpy(bounds6 + 6 * i + 3, b.high, 12); }
    if (counts) counts[i] = (int32_t)b.faces.size();
    if (face_order) memcpy(face_order + off, b.faces.data(), sizeof(int32_t) * b.faces.size());
    off += b.faces.size();
  }
  return RT_OK;
}

// =====================================================================================================
// Verification hook: Eigen-order primitives on the host (op codes: oracle/eigen_kat.cpp)
// =====================================================================================================
#include "rt_kat.h"

extern "C" int rt_debug_math_host(int32_t op, int32_t n, const float* in, float* out) {
  static const int in_len[] = {6, 3, 6, 12, 19, 20, 9, 16, 4, 6, 6, 6, 6, 13, 3, 16, 24, 2};
  static const int out_len[] = {1, 3, 3, 3, 3, 4, 9, 16, 16, 3, 3, 3, 3, 3, 1, 3, 3, 1};
  if (op < 0 || op > 17 || n < 0 || !in || !out) { rt::set_error("rt_debug_math_host: bad op"); return RT_ERR_INVALID; }
  for (int32_t k = 0; k < n; k++)
    if (rt::debug_math_case(op, in + (size_t)k * in_len[op], out + (size_t)k * out_len[op])) return RT_ERR_INVALID;
  return RT_OK;
}

extern "C" int rt_debug_record_layout(int64_t n_nodes, int64_t n_tris, int64_t n_wide, int64_t out[2]) {
  if (!out || n_nodes < 0 || n_tris < 0 || n_wide < 0) { rt::set_error("rt_debug_record_layout: bad argument"); return RT_ERR_INVALID; }
  uint64_t wb = 0;
  out[0] = (int64_t)rt::record_layout((uint64_t)n_nodes, (uint64_t)n_tris, (uint64_t)n_wide, &wb);
  out[1] = (int64_t)wb;
  return RT_OK;
}

extern "C" int rt_debug_frame_plan(const int64_t in[], int32_t n_in, int32_t out[], int32_t n_out) {
  if (!in || !out || (n_in != 11 && n_in != 12) || n_out != 14 || (n_in == 12 && (in[11] < 0 || in[11] > RT_MAX_LIGHT_SET)) || in[3] <= 0 || in[4] <= 0 || in[3] > 65536 || in[4] > 65536 || in[6] < 1 ||
      in[5] < 0 || in[5] >= in[6] || in[8] < 0) {
    rt::set_error("rt_debug_frame_plan: bad argument");
    return RT_ERR_INVALID;
  }
  rt::FrameInputs fi;
  fi.mode = (int)in[0], fi.max_depth = (int)in[1], fi.flags = (int)in[2];
  fi.tiles_x = (int)in[3], fi.tiles_y = (int)in[4], fi.shard_index = (int)in[5], fi.shard_count = (int)in[6];
  fi.variant = (int)in[7];
  fi.record_bytes = (uint64_t)in[8];
  fi.has_wide4 = in[9] != 0;
  fi.alone = in[10] != 0;
  if (n_in == 12) fi.mem_lights = (int)in[11];  // lights read from a light set in device memory (0 = none)
  const rt::FramePlan p = rt::plan_frame(fi);
  const int32_t o[14] = {p.kernel, p.trav, p.needs_variants, p.grid, (int32_t)p.units, p.depth, p.l2_resident, p.xcd_remap,
                         p.writes_wave_stats, p.lpt, p.split_ceiling, p.rotate_bands, p.pipeline_buffers, p.full_small_build};
  memcpy(out, o, sizeof o);
  return RT_OK;
}

extern "C" int rt_debug_view_plan(const int64_t in[], int32_t n_in, int64_t out[], int32_t n_out) {
  if (!in || !out || n_in != 9 || n_out != 7) { rt::set_error("rt_debug_view_plan: bad argument"); return RT_ERR_INVALID; }
  for (int k = 0; k < 9; k++)  // every input fits its field (tiles: up to 2^27 a side, a frame of INT32_MAX pixels)
    if (in[k] < INT32_MIN || in[k] > INT32_MAX || ((k == 4 || k == 5) && in[k] > (1 << 27))) {
      rt::set_error("rt_debug_view_plan: input %d out of range", k);
      return RT_ERR_INVALID;
    }
  rt::ViewInputs vi;
  vi.mode = (int)in[0], vi.max_depth = (int)in[1], vi.flags = (int)in[2], vi.shard_count = (int)in[3];
  vi.tiles_x = (int)in[4], vi.tiles_y = (int)in[5];
  vi.n_views = in[6];
  vi.variant = (int)in[7];
  vi.mem_lights = (int)in[8];
  const rt::ViewPlan p = rt::plan_views(vi);
  const int64_t o[7] = {p.kernel, p.depth, p.units_per_view, p.total_blocks, p.light_source, p.status != RT_OK, p.status};
  memcpy(out, o, sizeof o);
  return RT_OK;
}

extern "C" int rt_debug_sample_plan(const int64_t in[], int32_t n_in, int64_t out[], int32_t n_out) {
  if (!in || !out || n_in != 10 || n_out != 10) { rt::set_error("rt_debug_sample_plan: bad argument"); return RT_ERR_INVALID; }
  for (int k = 0; k < 10; k++)  // as rt_debug_view_plan
    if (in[k] < INT32_MIN || in[k] > INT32_MAX || ((k == 4 || k == 5) && in[k] > (1 << 27))) {
      rt::set_error("rt_debug_sample_plan: input %d out of range", k);
      return RT_ERR_INVALID;
    }
  rt::ViewInputs vi;
  vi.mode = (int)in[0], vi.max_depth = (int)in[1], vi.flags = (int)in[2], vi.shard_count = (int)in[3];
  vi.tiles_x = (int)in[4], vi.tiles_y = (int)in[5];
  vi.n_views = in[6];
  vi.variant = (int)in[7];
  vi.mem_lights = (int)in[8];
  vi.samples = (int)in[9];
  const rt::ViewPlan p = rt::plan_views(vi);
  if (p.status != RT_OK) rt::set_error("rt_debug_sample_plan: %s", p.why);  // the refusal's message, for the tests
  const int64_t o[10] = {p.kernel, p.depth, p.units_per_view, p.total_blocks, p.light_source, p.status != RT_OK, p.status,
                         p.layout, p.pixels_per_wave, p.waves_per_tile};
  memcpy(out, o, sizeof o);
  return RT_OK;
}

// ------------------------------------------------------------------------------------------------
// Sample patterns of supersampled view batches (rt_render_views_ss): one offset per cell of an nx x ny grid over the
// pixel, cells row-major with j outer; the position within the cell is its centre (grid) or drawn from rng (jittered)
// ------------------------------------------------------------------------------------------------
static int sample_cells(const char* who, int32_t nx, int32_t ny, rt_rand_state* rng, bool jitter, rt_sample_pattern* out) {
  if (!out || nx < 1 || ny < 1 || (int64_t)nx * ny > RT_MAX_SAMPLES) {
    rt::set_error("%s: %d x %d cells (1..%d samples)", who, nx, ny, RT_MAX_SAMPLES);
    return RT_ERR_INVALID;
  }
  rt_rand_state local;
  if (jitter && !rng) { rt_rand_seed(&local, 1); rng = &local; }
  memset(out, 0, sizeof *out);
  out->n_samples = nx * ny;
  for (int32_t j = 0; j < ny; j++)
    for (int32_t i = 0; i < nx; i++) {
      const double ux = jitter ? rt_rand(rng) / (2147483647 + 1.0) : 0.5;  // x first, then y
      const double uy = jitter ? rt_rand(rng) / (2147483647 + 1.0) : 0.5;
      float* o = out->offsets[j * nx + i];
      o[0] = (float)((i + ux) / nx - 0.5);
      o[1] = (float)((j + uy) / ny - 0.5);
    }
  return RT_OK;
}

extern "C" int rt_sample_pattern_grid(int32_t nx, int32_t ny, rt_sample_pattern* out) {
  return sample_cells("rt_sample_pattern_grid", nx, ny, nullptr, false, out);
}

extern "C" int rt_sample_pattern_jittered(int32_t nx, int32_t ny, rt_rand_state* rng, rt_sample_pattern* out) {
  return sample_cells("rt_sample_pattern_jittered", nx, ny, rng, true, out);
}

// ------------------------------------------------------------------------------------------------
// Ray streams, host side: the coherence keys (rt_raykey.h, the function k_ray_keys runs) and their grid
// ------------------------------------------------------------------------------------------------
#include "rt_raykey.h"

const float* rt::scene_ray_bounds(rt_scene* s) {
  // hs.wv after a device update: mirrored by the callers that can report a failure (rt_scene_ray_bounds, the ray
  // lists' ensure_scratch); a replica is never asked -- lists and bounds go through its scene, whose HostScene it shares
  if (!s->ray_bounds_valid) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const rt::f3& v : s->hs.wv) {
      const float c[3] = {v.x, v.y, v.z};
      for (int k = 0; k < 3; k++) {  // comparisons: a NaN coordinate leaves both bounds alone
        if (c[k] < lo[k]) lo[k] = c[k];
        if (c[k] > hi[k]) hi[k] = c[k];
      }
    }
    for (int k = 0; k < 3; k++) {
      const bool ok = std::isfinite(lo[k]) && std::isfinite(hi[k]);
      s->ray_bounds[k] = ok ? lo[k] : 0.0f;
      s->ray_bounds[3 + k] = ok ? hi[k] : 0.0f;
    }
    s->ray_bounds_valid = true;
  }
  return s->ray_bounds;
}

extern "C" int rt_scene_ray_bounds(rt_scene* s, float bounds6[6]) {
  if (!s || !bounds6) { rt::set_error("rt_scene_ray_bounds: null argument"); return RT_ERR_INVALID; }
  if (const int rc = rt::host_mirror_geometry(s)) return rc;  // (hs.wv after a device update)
  memcpy(bounds6, rt::scene_ray_bounds(s), 24);
  return RT_OK;
}

extern "C" int rt_debug_ray_keys(int32_t query, int32_t n, const float* a3, const float* b3, const float bounds6[6],
                                 uint32_t* keys_out) {
  if (query < RT_RAYS_CLOSEST || query > RT_RAYS_COLOR) { rt::set_error("rt_debug_ray_keys: bad query %d", query); return RT_ERR_INVALID; }
  if (n < 0 || !bounds6 || (n && (!a3 || !b3 || !keys_out))) { rt::set_error("rt_debug_ray_keys: invalid arguments"); return RT_ERR_INVALID; }
  // every query keys its ray by (a, b): origin and direction, or a shadow ray's P and L
  const bool origin_major = (rt::kernel_variant() & rt::VB_RAYKEY_ORIGIN_MAJOR) != 0;
  for (int32_t i = 0; i < n; i++) keys_out[i] = rt::ray_key(a3 + 3 * (size_t)i, b3 + 3 * (size_t)i, bounds6, origin_major);
  return RT_OK;
}
