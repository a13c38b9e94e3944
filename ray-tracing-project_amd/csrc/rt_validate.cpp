// rt_validate.cpp -- the checks on a prepared scene: the acceleration-structure validator over the binary,
// quantised 4-wide and fp32 4-wide trees (rt_debug_validate_bvh), the trees' SAH cost (rt_debug_tree_cost)
// and the record flag counts (rt_debug_scene_flags). Restates no reference code: it checks that the boxes
// bound what the reference's edge tests (src/flyscene.cpp:580-590) can accept.
#include <cstring>

#include "rt_host.h"

namespace {
struct VBox {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  void add(const VBox& b) {
    for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], b.lo[k]); hi[k] = std::max(hi[k], b.hi[k]); }
  }
  bool inside(const double* l, const double* h) const {
    for (int k = 0; k < 3; k++)
      if (lo[k] <= hi[k] && (lo[k] < l[k] || hi[k] > h[k])) return false;
    return true;
  }
};

struct Validator {
  const rt::HostScene& hs;
  std::vector<int> seen2, seen4;
  int64_t bad = 0;
  // a tree without duplicated references must hold every triangle whole inside every ancestor box;
  // a spatial-split tree (more records than faces) holds each reference's part: its content is the
  // triangle's bounds cut to the path's boxes, and coverage() checks that the faces' leaf regions
  // together cover every face
  bool strict = true;
  std::vector<std::vector<VBox>> regions;  // per face: the path-intersected boxes of its leaves (split trees)
  // the box of the triangle the culling must bound (rt::bound_vert: the accept region)
  VBox tri_box(const rt::TriRec64& t) const {
    VBox b;
    for (int j = 0; j < 3; j++) {
      const rt::f3& w = rt::bound_vert(hs, t.face, j);
      const double v[3] = {w.x, w.y, w.z};
      for (int k = 0; k < 3; k++) { b.lo[k] = std::min(b.lo[k], v[k]); b.hi[k] = std::max(b.hi[k], v[k]); }
    }
    return b;
  }
  VBox leaf(uint32_t h, std::vector<int>& seen, const VBox& region, bool record) {
    VBox b;
    for (uint32_t i = rt::leaf_first(h); i < rt::leaf_first(h) + rt::leaf_count(h); i++) {
      if (i >= hs.tris.size()) { bad++; continue; }
      seen[i]++;
      VBox t = tri_box(hs.tris[i]);
      if (!strict) {
        for (int k = 0; k < 3; k++) { t.lo[k] = std::max(t.lo[k], region.lo[k]); t.hi[k] = std::min(t.hi[k], region.hi[k]); }
        if (t.lo[0] > t.hi[0] || t.lo[1] > t.hi[1] || t.lo[2] > t.hi[2]) { bad++; continue; }  // reference outside its region
        if (record && hs.tris[i].face < regions.size()) regions[hs.tris[i].face].push_back(region);
      }
      b.add(t);
    }
    return b;
  }
  static VBox cut(const VBox& a, const double* l, const double* u) {
    VBox r;
    for (int k = 0; k < 3; k++) { r.lo[k] = std::max(a.lo[k], l[k]); r.hi[k] = std::min(a.hi[k], u[k]); }
    return r;
  }
  VBox bin(uint32_t n, int d, int64_t& depth, const VBox& region) {
    depth = std::max<int64_t>(depth, d + 1);
    const rt::Node64& nd = hs.nodes[n];
    VBox all;
    for (int c = 0; c < 2; c++) {
      if (rt::is_sentinel_child(nd, c)) continue;
      const rt::ChildBox cb = rt::child_box(nd, c);
      const double l[3] = {cb.lo[0], cb.lo[1], cb.lo[2]}, u[3] = {cb.hi[0], cb.hi[1], cb.hi[2]};
      const VBox sub = cut(region, l, u);
      const VBox b = rt::is_leaf(cb.h) ? leaf(cb.h, seen2, sub, true) : bin(cb.h, d + 1, depth, sub);
      if (!b.inside(l, u)) bad++;
      all.add(b);
    }
    return all;
  }
  VBox wide(uint32_t n, int d, int64_t& depth, const VBox& region) {
    depth = std::max<int64_t>(depth, d + 1);
    const rt::Node4Q& nd = hs.nodes4[n];
    const double org[3] = {nd.ox, nd.oy, nd.oz};
    const uint8_t e[3] = {nd.ex, nd.ey, nd.ez};
    const uint32_t ql[3] = {nd.qlx, nd.qly, nd.qlz}, qh[3] = {nd.qhx, nd.qhy, nd.qhz};
    VBox all;
    for (int c = 0; c < 4; c++) {
      if (!((nd.valid >> c) & 1)) continue;
      const uint32_t h = nd.child[c];
      double l[3], u[3];
      for (int k = 0; k < 3; k++) {
        // the device's cell size: the float with biased exponent e (2^(e-127))
        const double sc = std::ldexp(1.0, (int)e[k] - 127);
        l[k] = org[k] + ((ql[k] >> (8 * c)) & 255u) * sc;
        u[k] = org[k] + ((qh[k] >> (8 * c)) & 255u) * sc;
      }
      const VBox sub = cut(region, l, u);
      const VBox b = rt::is_leaf(h) ? leaf(h, seen4, sub, false) : wide(h, d + 1, depth, sub);
      if (!b.inside(l, u)) bad++;
      all.add(b);
    }
    return all;
  }
  // the fp32 4-wide tree (device Node128): its boxes are the binary tree's, copied; every octant order
  // a permutation of the slots with the occupied ones first
  std::vector<int> seenw;
  VBox widef(uint32_t n, int d, int64_t& depth, const VBox& region) {
    depth = std::max<int64_t>(depth, d + 1);
    if (n >= hs.wide.size()) { bad++; return VBox{}; }
    const rt::Wide4& w = hs.wide[n];
    for (int o = 0; o < 8; o++) {
      int mask = 0;
      for (int k = 0; k < 4; k++) {
        mask |= 1 << w.order[o][k];
        if ((k < w.n) != (w.order[o][k] < w.n)) bad++;
      }
      if (mask != 15) bad++;
    }
    VBox all;
    for (int c = 0; c < w.n; c++) {
      const uint32_t h = w.child[c];
      const double l[3] = {w.box[c][0], w.box[c][2], w.box[c][4]}, u[3] = {w.box[c][1], w.box[c][3], w.box[c][5]};
      const VBox sub = cut(region, l, u);
      const VBox b = rt::is_leaf(h) ? leaf(h, seenw, sub, false) : widef(h, d + 1, depth, sub);
      if (!b.inside(l, u)) bad++;
      all.add(b);
    }
    return all;
  }
  // split trees: points of every face on a barycentric grid (vertices, edges, interior) each lie in
  // one of that face's leaf regions
  void coverage() {
    constexpr int G = 8;
    for (uint32_t f = 0; f < (uint32_t)hs.nf; f++) {
      const std::vector<VBox>& rs = regions[f];
      if (rs.empty()) { bad++; continue; }
      const rt::f3& a = rt::bound_vert(hs, f, 0);
      const rt::f3& b = rt::bound_vert(hs, f, 1);
      const rt::f3& c = rt::bound_vert(hs, f, 2);
      for (int i = 0; i <= G; i++)
        for (int j = 0; i + j <= G; j++) {
          const double s = (double)i / G, t = (double)j / G, r = 1.0 - s - t;
          const double p[3] = {r * a.x + s * b.x + t * c.x, r * a.y + s * b.y + t * c.y, r * a.z + s * b.z + t * c.z};
          bool in = false;
          for (const VBox& q : rs) {
            in = true;
            for (int k = 0; k < 3; k++) in = in && p[k] >= q.lo[k] && p[k] <= q.hi[k];
            if (in) break;
          }
          if (!in) bad++;
        }
    }
  }
};
}  // namespace

extern "C" int rt_debug_scene_flags(const rt_scene* s, int64_t counts[3], float* cert_origin_max, uint32_t* face_flags) {
  if (!s || !counts) { rt::set_error("rt_debug_scene_flags: null argument"); return RT_ERR_INVALID; }
  if (const int rc = rt::host_mirror_all(s)) return rc;  // (hs.nodes / hs.tris after a device refit, ov3 after a device update)
  counts[0] = (int64_t)s->hs.tris.size();
  counts[1] = counts[2] = 0;
  if (face_flags) memset(face_flags, 0, sizeof(uint32_t) * (size_t)s->hs.nf);
  for (const rt::TriRec64& t : s->hs.tris) {
    counts[1] += (t.box & rt::kSafeNormalBit) != 0;
    counts[2] += (t.box & rt::kBoxCertBit) != 0;
    if (face_flags && t.face < (uint32_t)s->hs.nf) face_flags[t.face] |= t.box & (rt::kSafeNormalBit | rt::kBoxCertBit);
  }
  if (cert_origin_max) *cert_origin_max = rt::cert_origin_max(s->hs);
  return RT_OK;
}

extern "C" int rt_debug_tree_cost(const rt_scene* s, double k_trav, double out[4]) {
  if (!s || !out) { rt::set_error("rt_debug_tree_cost: null argument"); return RT_ERR_INVALID; }
  if (const int rc = rt::host_mirror(s)) return rc;  // (hs.nodes / hs.tris after a device refit)
  const rt::HostScene& hs = s->hs;
  for (int k = 0; k < 4; k++) out[k] = 0.0;
  if (hs.nodes.empty()) return RT_OK;
  auto area = [](const float* b) {  // lx hx ly hy lz hz
    const double dx = (double)b[1] - b[0], dy = (double)b[3] - b[2], dz = (double)b[5] - b[4];
    return dx < 0 || dy < 0 || dz < 0 ? 0.0 : dx * dy + dy * dz + dz * dx;
  };
  double inner = 0.0, leafc = 0.0, leaves = 0.0, tris = 0.0;
  std::vector<std::pair<uint32_t, double>> st{{hs.root, -1.0}};
  double root_area = 0.0;
  while (!st.empty()) {
    const auto [h, a] = st.back();
    st.pop_back();
    if (rt::is_leaf(h)) {
      leafc += a * rt::leaf_count(h);
      leaves += 1;
      tris += rt::leaf_count(h);
      continue;
    }
    const rt::Node64& nd = hs.nodes[h];
    const float* b0 = &nd.c0lx;
    const float* b1 = &nd.c1lx;
    double an = a;
    if (an < 0) {  // the root: the union of its children's boxes
      float u[6];
      for (int k = 0; k < 3; k++) {
        u[2 * k] = std::min(b0[2 * k], b1[2 * k]);
        u[2 * k + 1] = std::max(b0[2 * k + 1], b1[2 * k + 1]);
      }
      an = root_area = area(u);
    }
    inner += an;
    st.push_back({nd.child0, area(b0)});
    st.push_back({nd.child1, area(b1)});
  }
  if (!(root_area > 0)) return RT_OK;
  out[0] = (k_trav * inner + leafc) / root_area;  // SAH cost in triangle tests per random ray
  out[1] = inner / root_area;                      // expected node visits (interior) per random ray
  out[2] = leafc / root_area;                      // expected triangle tests per random ray
  out[3] = leaves > 0 ? tris / leaves : 0.0;       // mean leaf size
  return RT_OK;
}

extern "C" int rt_debug_validate_bvh(const rt_scene* s, int64_t info[7]) {
  if (!s || !info) { rt::set_error("rt_debug_validate_bvh: null argument"); return RT_ERR_INVALID; }
  if (const int rc = rt::host_mirror_all(s)) return rc;  // (hs.nodes / hs.tris after a device refit, the bound vertices after a device update)
  const rt::HostScene& hs = s->hs;
  Validator v{hs, std::vector<int>(hs.tris.size()), std::vector<int>(hs.tris.size())};
  v.strict = hs.tris.size() == (size_t)hs.nf;
  if (!v.strict) v.regions.resize((size_t)hs.nf);
  for (int k = 0; k < 7; k++) info[k] = 0;
  info[0] = (int64_t)hs.nodes.size();
  info[2] = (int64_t)hs.nodes4.size();
  const VBox everywhere = [] {
    VBox b;
    for (int k = 0; k < 3; k++) { b.lo[k] = -INFINITY; b.hi[k] = INFINITY; }
    return b;
  }();
  if (!hs.nodes.empty()) v.bin(hs.root, 0, info[1], everywhere);
  if (!hs.nodes4.empty()) v.wide(0, 0, info[3], everywhere);
  if (!v.strict && !hs.nodes.empty()) v.coverage();
  int64_t wide_depth = 0, wide_once = 0;
  v.seenw.assign(hs.tris.size(), 0);
  if (!hs.wide.empty()) {
    v.widef(0, 0, wide_depth, everywhere);
    if (wide_depth != hs.depth_wide || 3 * wide_depth + 4 > rt::kStackW) v.bad++;
  }
  for (size_t i = 0; i < hs.tris.size(); i++) {
    info[4] += v.seen2[i] == 1;
    info[5] += v.seen4[i] == 1;
    wide_once += v.seenw[i] == 1;
  }
  info[6] = v.bad;
  const bool ok = v.bad == 0 && info[4] == (int64_t)hs.tris.size() &&
                  (hs.nodes4.empty() || info[5] == (int64_t)hs.tris.size()) &&
                  (hs.wide.empty() || wide_once == (int64_t)hs.tris.size());
  if (!ok) { rt::set_error("acceleration structure check failed (%lld violations)", (long long)v.bad); return RT_ERR_INVALID; }
  return RT_OK;
}
