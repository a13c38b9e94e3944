// rt_update.cpp -- rt_scene_update, host side: a scene's geometry replaced in place. The topology stays (faces,
// materials per face, the traversal tree's shape and leaf order); everything rt_scene_create derives from the
// coordinates is derived again by create's own stages -- the invariants (rt_host.cpp scene_invariants), the
// reference-box partition with its ranks, the face records with their flags (rt_layout.cpp), the static pad and
// the certificate range -- and the tree's boxes are refit: here on the host (host-only scenes, geometry the
// device path does not take, and the oracle the kernels are held against), or by rt_refit.hip on the device.
// A hit is decided by the exact triangle test, the reference-box predicate and the rank; the tree only culls,
// so any conservative tree over the new geometry gives the bits of a freshly built one.
#include <chrono>
#include <cstring>

#include "rt_host.h"

namespace rt {

// One walk from the root, level by level. A single-leaf root's sentinel child (an inverted box over slot 0) is
// no leaf of the scene and keeps its box.
void refit_topology(const HostScene& hs, RefitTopo& t) {
  t = RefitTopo{};
  const size_t nn = hs.nodes.size();
  t.node_where.assign(nn, kNoParent);
  t.level_off.assign(1, 0u);
  t.ready = true;
  if (nn == 0 || is_leaf(hs.root) || hs.root >= nn) return;
  std::vector<uint32_t> cur{hs.root}, next;
  while (!cur.empty()) {
    for (uint32_t n : cur) {
      t.level_nodes.push_back(n);
      const Node64& nd = hs.nodes[n];
      for (uint32_t c = 0; c < 2; c++) {
        const uint32_t h = c ? nd.child1 : nd.child0;
        if (!is_leaf(h)) {
          t.node_where[h] = 2 * n + c;
          next.push_back(h);
        } else if (!(nn == 1 && c == 1 && h == make_leaf(0, 1) && is_sentinel_child(nd, 1))) {
          t.leaf_handle.push_back(h);
          t.leaf_where.push_back(2 * n + c);
        }
      }
    }
    t.level_off.push_back((uint32_t)t.level_nodes.size());
    cur.swap(next);
    next.clear();
  }
}

// Host refit of hs.nodes: each leaf's bounds from bound_vert (the accept-region vertices where hs.av holds them),
// each interior child's box the exact min / max union of everything below it, every box widened by `pad` as the
// builders widen theirs (set_child), the order bits recomputed. Levels from the deepest up, so any node layout
// serves (the default one, child index > parent index, included).
void refit_host(HostScene& hs, const RefitTopo& t, float pad) {
  std::vector<Aabb> sub(hs.nodes.size());  // unpadded bounds of each node's subtree
  auto put = [&](uint32_t where, const Aabb& b) {
    Node64& p = hs.nodes[where >> 1];
    const int c = (int)(where & 1u);
    set_child(p, c, b, pad, c ? p.child1 : p.child0);
    sub[where >> 1].merge(b);
  };
  for (size_t k = 0; k < t.leaf_handle.size(); k++) {
    const uint32_t h = t.leaf_handle[k];
    Aabb b;
    for (uint32_t sl = leaf_first(h); sl < leaf_first(h) + leaf_count(h); sl++)
      for (int j = 0; j < 3; j++) {
        const f3& w = bound_vert(hs, hs.tris[sl].face, j);
        const float p[3] = {w.x, w.y, w.z};
        b.growp(p);
      }
    put(t.leaf_where[k], b);
  }
  for (size_t L = t.level_off.size() - 1; L-- > 0;)
    for (uint32_t i = t.level_off[L]; i < t.level_off[L + 1]; i++) {
      const uint32_t n = t.level_nodes[i];
      if (t.node_where[n] != kNoParent) put(t.node_where[n], sub[n]);
      hs.nodes[n].pad0 = octant_order(hs.nodes[n]);
    }
}

// the device path takes what the device builders take: finite culling bounds well inside the float range
static bool refit_on_device(const HostScene& hs) {
  bool ok = true;
  for (const std::vector<f3>* pts : {&hs.wv, &hs.av})
    for (const f3& p : *pts)
      if (!(std::fabs(p.x) <= 1e30f) || !(std::fabs(p.y) <= 1e30f) || !(std::fabs(p.z) <= 1e30f)) ok = false;  // NaN fails too
  return ok;
}

// the quantised 4-wide tree of a host-built scene from the refit binary tree (create's depth rule), the
// invalidations, and the device's reference boxes, materials and replicas
int update_finish(rt_scene* s, size_t boxes_before) {
  HostScene& hs = s->hs;
  int rc;
  const bool replace4 = s->builder_used == RT_BUILDER_SAH || s->builder_used == RT_BUILDER_SBVH;
  if (replace4) {
    if ((rc = host_mirror(s))) return rc;
    build_bvh4(hs);
    if (3 * hs.depth4 + 4 > kStack4) hs.nodes4.clear();
  }
  const bool boxes_changed = hs.boxes.size() != boxes_before;
  if (boxes_changed) s->box_colors.clear();  // "not set yet"
  s->face_boxcolor_valid = false;
  s->ray_bounds_valid = false;
  s->lpt.valid = false;
  if (s->device != RT_DEVICE_NONE && (rc = device_update_rest(s, replace4, boxes_changed))) return rc;
  return RT_OK;
}

float static_pad_of_bounds(const float lo[3], const float hi[3]) { return bvh_pad(lo, hi); }
float cert_origin_of(const float* M, float R) {  // (cert_origin_max over the reduced maximum)
  if (!model_is_similarity(M)) return 0.0f;
  return std::isfinite(R) ? 16.0f * R : 0.0f;
}

}  // namespace rt

extern "C" int rt_scene_update(rt_scene* s, const rt_mesh_desc* d, rt_update_stats* stats) {
  using clk = std::chrono::steady_clock;
  if (!s || !d) { rt::set_error("rt_scene_update: null argument"); return RT_ERR_INVALID; }
  if (s->is_replica) { rt::set_error("rt_scene_update: a replica is updated through its scene"); return RT_ERR_INVALID; }
  if (s->opts.wide_tree) {
    rt::set_error("rt_scene_update: scenes with the fp32 4-wide tree (wide_tree = 1) are not updated in this version");
    return RT_ERR_UNSUPPORTED;
  }
  rt::HostScene& hs = s->hs;
  if (d->n_vertices != hs.nv || d->n_faces != hs.nf || d->n_materials != (int32_t)hs.mats.size()) {
    rt::set_error("rt_scene_update: the mesh has %d vertices, %d faces, %d materials; the scene %d, %d, %zu", d->n_vertices,
                  d->n_faces, d->n_materials, hs.nv, hs.nf, hs.mats.size());
    return RT_ERR_INVALID;
  }
  if ((d->n_faces && (!d->face_vertex_ids || !d->face_normals || !d->face_material_ids)) ||
      (d->n_vertices && (!d->vertices || !d->vertex_normals)) || (d->n_materials && !d->materials)) {
    rt::set_error("rt_scene_update: invalid mesh description");
    return RT_ERR_INVALID;
  }
  if (hs.nf && (memcmp(d->face_vertex_ids, hs.fidx.data(), 12 * (size_t)hs.nf) != 0 ||
                memcmp(d->face_material_ids, hs.fmat.data(), 4 * (size_t)hs.nf) != 0)) {
    rt::set_error("rt_scene_update: the mesh's faces differ from the scene's (vertex or material ids)");
    return RT_ERR_INVALID;
  }
  const bool on_device = s->device != RT_DEVICE_NONE;
  int rc = RT_OK;
  if (on_device && (rc = rt::update_quiesce(s))) return rc;
  auto t0 = clk::now(), tp = t0;
  auto lap = [&tp]() {
    const auto n = clk::now();
    const double ms = std::chrono::duration<double, std::milli>(n - tp).count();
    tp = n;
    return ms;
  };
  rt_update_stats st;
  memset(&st, 0, sizeof st);
  rt::PhaseTimer pt("update");
  rt::scene_invariants(hs, d);
  hs.mats.assign(d->materials, d->materials + d->n_materials);
  st.prep_ms = lap();
  pt.mark("invariants");
  const size_t boxes_before = hs.boxes.size();
  if ((rc = rt::partition_ref_boxes(s, on_device ? s->device : -1, d->vertices))) return rc;
  st.boxes_ms = lap();
  pt.mark("ref_boxes");
  std::vector<rt::TriRec64> recs;
  rt::face_records(hs, recs);  // ranks, boxes, flags (by face id; the slots keep their faces)
  if (!s->refit.topo.ready) rt::refit_topology(hs, s->refit.topo);
  const float pad = rt::scene_static_pad(hs);
  s->static_pad = pad;
  s->cert_origin_max = rt::cert_origin_max(hs);
  st.records_ms = lap();
  pt.mark("records");
  st.bounds_on_device = on_device && rt::refit_on_device(hs);
  if (st.bounds_on_device) {
    if ((rc = rt::device_refit(s, recs, pad, &st.upload_ms, &st.refit_ms))) return rc;
    s->host_stale = true;
    lap();
  } else {
    rt::parallel_for(hs.tris.size(), [&](size_t b, size_t e) {
      for (size_t sl = b; sl < e; sl++) hs.tris[sl] = recs[hs.tris[sl].face];
    });
    rt::refit_host(hs, s->refit.topo, pad);
    s->host_stale = false;
    st.refit_ms = lap();
    if (on_device) {
      if ((rc = rt::device_reupload(s))) return rc;
      st.upload_ms = lap();
    }
  }
  pt.mark("refit");
  s->geom_stale = false;  // (every array a device update leaves stale has been written above)
  if ((rc = rt::update_finish(s, boxes_before))) return rc;
  if (on_device) st.upload_ms += lap();
  st.total_ms = std::chrono::duration<double, std::milli>(clk::now() - t0).count();
  if (stats) {
    double cost[4];
    if ((rc = rt_debug_tree_cost(s, 0.7, cost))) return rc;
    st.sah_cost = cost[0];
    *stats = st;
  }
  return RT_OK;
}
