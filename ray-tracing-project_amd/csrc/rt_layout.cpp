// rt_layout.cpp -- from faces to the records the kernels read: the exact-test triangle records with their
// safe-normal and reference-box certificates, the culling pads and bounds (world bounds, the accept region of
// tilted normals), the depth-first node re-layout with its octant order hints, the host halves of the three
// device builders (rt_build.hip), and the two 4-wide collapses of the binary tree.
//
// Reference semantics these bound (file:line in plindhorst/Ray-Tracing-Project):
//   plane and edge tests   src/flyscene.cpp:459-465,580-590
//   interpolated normal    src/flyscene.cpp:594-599
//   box predicate          src/flyscene.cpp:484-507
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "rt_host.h"

#include "rt_faceflags.h"

namespace rt {

// A face whose interpolated normal (interpolateNormal, flyscene.cpp:594-599) can never be the zero
// vector for a point that passed the inside test: its area A (same expression the kernel uses) is a
// positive normal number and every unit vertex normal leans into the face normal (n.nk >= 0.5). Then
// n.(sum_k nk a_k / A) >= 0.5 (sum a_k)/A >= 0.5 (sub-areas of a point in the plane sum to >= A),
// far above rounding, so norm() != 0 and the reference never rejects the face for it; when A would
// overflow the blend, the result is NaN, which the reference also accepts (NaN != 0).
static bool safe_normal(const HostScene& hs, uint32_t f) {
  const uint32_t* v = &hs.fidx[3 * (size_t)f];
  return safe_normal_of(hs.wv[v[0]], hs.wv[v[1]], hs.wv[v[2]], hs.fnn[f], hs.vnn[v[0]], hs.vnn[v[1]], hs.vnn[v[2]]);
}

// conservative padding of every BVH child box: covers the reference's rounding of P = o + t d and of
// the inclusive edge tests for ray origins within ~16 scene extents (DESIGN.md "Exactness of culling")
float bvh_pad(const float lo[3], const float hi[3]) {
  float ext = 0.0f, mag = 0.0f;
  for (int k = 0; k < 3; k++) {
    ext = std::max(ext, hi[k] - lo[k]);
    mag = std::max(mag, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
  }
  return 2e-5f * std::max(std::max(ext, mag), 1e-3f);
}

// the static pad the builders gave every box: bvh_pad of the triangles' bounds (the builders' `world`)
float scene_static_pad(const HostScene& hs) {
  // per-chunk bounds merged afterwards: min / max skip NaN coordinates the same way in any order
  float plo[16][3], phi[16][3];
  for (int t = 0; t < 16; t++)
    for (int k = 0; k < 3; k++) { plo[t][k] = INFINITY; phi[t][k] = -INFINITY; }
  const int T = parallel_chunks(hs.tris.size(), [&](size_t b, size_t e, int t) {
    float l[3] = {INFINITY, INFINITY, INFINITY}, h[3] = {-INFINITY, -INFINITY, -INFINITY};  // thread-local (no false sharing)
    for (size_t i = b; i < e; i++)
      for (int j = 0; j < 3; j++) {
        const f3& w = bound_vert(hs, hs.tris[i].face, j);
        const float v[3] = {w.x, w.y, w.z};
        for (int k = 0; k < 3; k++) { l[k] = std::min(l[k], v[k]); h[k] = std::max(h[k], v[k]); }
      }
    for (int k = 0; k < 3; k++) { plo[t][k] = l[k]; phi[t][k] = h[k]; }
  });
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int t = 0; t < T; t++)
    for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], plo[t][k]); hi[k] = std::max(hi[k], phi[t][k]); }
  return hs.tris.empty() ? 0.0f : bvh_pad(lo, hi);
}

static void world_bounds(const HostScene& hs, float lo[3], float hi[3]) {
  Aabb parts[16];
  const std::vector<f3>& pts = hs.av.empty() ? hs.wv : hs.av;
  const int T = parallel_chunks(pts.size(), [&](size_t b, size_t e, int t) {
    Aabb a;  // thread-local, stored once (adjacent per-thread slots written per item share cache lines)
    for (size_t i = b; i < e; i++) {
      const float c[3] = {pts[i].x, pts[i].y, pts[i].z};
      a.growp(c);
    }
    parts[t] = a;
  });
  Aabb w;
  for (int t = 0; t < T; t++) w.merge(parts[t]);
  for (int k = 0; k < 3; k++) { lo[k] = w.lo[k]; hi[k] = w.hi[k]; }
}

// Reference-box certificates (TriRec64::box kBoxCertBit). The accept path's box fast path (rt_traverse.h
// accept_candidate) accepts a candidate lane whose object-space hit point X = Minv p lies inside the
// face's reference box by m_k = 1e-5 ((hi - lo) + |lo| + |hi| + |o2_k|) per axis, o2 the ray's
// object-space origin -- margins far above the rounding of the reference's intersectBox
// (flyscene.cpp:484-507), so the reference accepts too. A face is certified when that fast path must
// succeed for every hit point its edge tests can accept, for any ray whose |o2|_inf <= Ro =
// cert_origin_max: its three object-space vertices lie inside the box by m_k(Ro) + delta_k, where
// delta_k = 1e-5 ((hi - lo) + |lo| + |hi|) + 4e-4 diam covers how far a hit point the reference's
// inclusive float edge tests accept can lie outside the triangle (at most a few ulp of |p - w| over
// sin(theta_min / 2), here <= 0.01 diam -- only triangles whose smallest angle has sin(theta/2) >= 0.01
// are certified) and the rounding of M / Minv (a similarity) and of X. Uncertified faces and rays
// beyond Ro take the fast path and, where it fails, the exact test, as before.
float cert_origin_max(const HostScene& hs) {
  if (!model_is_similarity(hs.M)) return 0.0f;  // no certificates (box_certified needs Ro > 0)
  float R = 0.0f;
  for (float v : hs.ov3) R = std::max(R, std::fabs(v));  // NaN coordinates are skipped by max
  return std::isfinite(R) ? 16.0f * R : 0.0f;
}

// The argument above holds for the triangle the edge tests actually accept on, which is the world
// triangle only when the face normal they use (hs.fnn, the caller's face_normals, never transformed by M)
// is the world triangle's own normal: with a tilted normal n the accepted region is the triangle projected
// along n onto n's plane, whose vertices move by up to diam * sin(angle(n, geometric normal)). And Minv
// must be a similarity for object-space distances to be world distances over one scale. So a
// model matrix whose linear part is not a uniform scale times a rotation certifies nothing
// (model_is_similarity), and a face certifies only if its normal is within kCertNormalSin of the world
// triangle's normal, with that projection offset (2 diam sin) added to the margin.
// (kCertNormalSin: rt_faceflags.h)
bool model_is_similarity(const float* M) {
  double c[3][3], n2[3];
  for (int j = 0; j < 3; j++) {
    for (int k = 0; k < 3; k++) c[j][k] = M[4 * j + k];  // column j of the column-major linear part
    n2[j] = c[j][0] * c[j][0] + c[j][1] * c[j][1] + c[j][2] * c[j][2];
    if (!std::isfinite(n2[j]) || !(n2[j] > 0.0)) return false;
  }
  for (int j = 0; j < 3; j++) {
    if (std::fabs(n2[j] - n2[0]) > 1e-5 * n2[0]) return false;
    const int i = (j + 1) % 3;
    const double d = c[j][0] * c[i][0] + c[j][1] * c[i][1] + c[j][2] * c[i][2];
    if (std::fabs(d) > 1e-5 * n2[0]) return false;
  }
  return M[3] == 0.0f && M[7] == 0.0f && M[11] == 0.0f && M[15] == 1.0f;
}

// sin of the angle between the face normal the edge tests use and the world triangle's normal (2 on
// degenerate or non-finite input: never certified)
static double face_normal_tilt(const HostScene& hs, uint32_t f) {
  const uint32_t* v = &hs.fidx[3 * (size_t)f];
  return face_tilt_of(hs.wv[v[0]], hs.wv[v[1]], hs.wv[v[2]], hs.fnn[f]);
}

// The edge tests (flyscene.cpp:580-590) accept P when n.(e_k x (P - w_k)) >= 0 for the three world edges,
// n the object-space face normal; P = o + t d lies on n's plane n.x = dist (:459-465). Adding multiples of
// n to e_k or P - w_k leaves those triple products unchanged, so the accepted set is the world triangle
// projected along n onto that plane, p_k = w_k - ((n.w_k - dist) / n.n) n -- the world triangle itself
// only when n is its normal. A face whose normal tilts by more than kBoundTilt (offsets above 1e-6 of
// its diameter, well inside the static pad's rounding allowance) is bounded by that projection; an
// untilted scene keeps hs.av empty and its builds unchanged. (A normal facing away from the triangle
// accepts nothing beyond rounding; its projection still bounds that.)
// (kBoundTilt: rt_faceflags.h)
void accept_region(HostScene& hs) {
  hs.av.clear();
  std::atomic<bool> any{false};
  parallel_chunks((size_t)hs.nf, [&](size_t b, size_t e, int) {
    for (size_t f = b; f < e && !any.load(std::memory_order_relaxed); f++)
      if (!(face_normal_tilt(hs, (uint32_t)f) <= kBoundTilt)) any = true;
  });
  if (!any) return;
  hs.av.resize(3 * (size_t)hs.nf);
  parallel_chunks((size_t)hs.nf, [&](size_t b, size_t e, int) {
    for (size_t f = b; f < e; f++) {
      const bool tilted = !(face_normal_tilt(hs, (uint32_t)f) <= kBoundTilt);
      for (int j = 0; j < 3; j++)
        hs.av[3 * f + j] = accept_vertex_of(hs.wv[hs.fidx[3 * f + j]], hs.fnn[f], hs.fdist[f], tilted);
    }
  });
}

static bool box_certified(const HostScene& hs, uint32_t f, float Ro) {
  if (!(Ro > 0.0f) || hs.ov3.empty()) return false;
  const double tilt = face_normal_tilt(hs, f);
  if (!(tilt <= kCertNormalSin)) return false;
  const RefBox& b = hs.boxes[hs.face_box[f]];
  const uint32_t* v = &hs.fidx[3 * (size_t)f];
  return box_certified_of(&hs.ov3[3 * (size_t)v[0]], &hs.ov3[3 * (size_t)v[1]], &hs.ov3[3 * (size_t)v[2]], b.low, b.high, Ro, tilt);
}

// the flag bits of face f's triangle records (kSafeNormalBit, kBoxCertBit): derived from the geometry
// alone, so the scene cache loader recomputes them instead of trusting the file
uint32_t tri_flags(const HostScene& hs, uint32_t f, float Ro) {
  return (safe_normal(hs, f) ? kSafeNormalBit : 0u) | (box_certified(hs, f, Ro) ? kBoxCertBit : 0u);
}

// exact-test record of face f (the kernels' TriRec64)
void tri_record(const HostScene& hs, uint32_t f, TriRec64& r, float Ro) {
  const f3& n = hs.fnn[f];
  const f3& w0 = hs.wv[hs.fidx[3 * f]];
  const f3& w1 = hs.wv[hs.fidx[3 * f + 1]];
  const f3& w2 = hs.wv[hs.fidx[3 * f + 2]];
  r.nx = n.x; r.ny = n.y; r.nz = n.z; r.dist = hs.fdist[f];
  r.w0x = w0.x; r.w0y = w0.y; r.w0z = w0.z;
  r.w1x = w1.x; r.w1y = w1.y; r.w1z = w1.z;
  r.w2x = w2.x; r.w2y = w2.y; r.w2z = w2.z;
  r.rank = hs.face_rank[f];
  r.face = f;
  r.box = hs.face_box[f] | tri_flags(hs, f, Ro);
}

void face_records(const HostScene& hs, std::vector<TriRec64>& out) {
  out.resize(hs.nf);
  const float Ro = cert_origin_max(hs);
  parallel_chunks((size_t)hs.nf, [&](size_t b, size_t e, int) {
    for (size_t f = b; f < e; f++) tri_record(hs, (uint32_t)f, out[f], Ro);
  });
}

// The device form of the binary node records (what device_upload sends and rt_debug_scene_records shows of a
// host-only scene): pad0 / pad1 = the children's record offsets (prefetch targets; a leaf child: its first
// triangle, behind the nodes) with the octant order bits in their low bits, interior children as byte offsets
// of their records. out holds hs.nodes.size() records.
void device_node_image(const HostScene& hs, Node64* out) {
  const size_t nn = hs.nodes.size();
  auto pf = [&](uint32_t c) -> uint32_t { return (uint32_t)(64 * (is_leaf(c) ? nn + leaf_first(c) : (size_t)c)); };
  parallel_for(nn, [&](size_t b, size_t e) {
    for (size_t i = b; i < e; i++) {
      Node64 nd = hs.nodes[i];
      const uint32_t order = nd.pad0;  // octant_order(), moved into the low offset bits
      nd.pad0 = pf(nd.child0) | (order & 0x3Fu);
      nd.pad1 = pf(nd.child1) | ((order >> 6) & 0x3u);
      if (!is_leaf(nd.child0)) nd.child0 *= 64u;
      if (!is_leaf(nd.child1)) nd.child1 *= 64u;
      out[i] = nd;
    }
  });
}

// Per-slot shading record (float4 x 3), in the triangle records' (BVH leaf) order: the unit normals of the
// slot's face's three vertices (Mesh normals as interpolateNormal normalises them, flyscene.cpp:599) and the
// material id in the first .w. out holds 12 floats per slot of hs.tris.
void device_fshade_image(const HostScene& hs, float* out) {
  parallel_for(hs.tris.size(), [&](size_t b, size_t e) {
    for (size_t sl = b; sl < e; sl++) {
      const uint32_t f = hs.tris[sl].face;
      float* r = out + 12 * sl;
      for (int k = 0; k < 3; k++) {
        const f3 n = hs.vnn[hs.fidx[3 * f + k]];
        r[4 * k] = n.x; r[4 * k + 1] = n.y; r[4 * k + 2] = n.z; r[4 * k + 3] = 0.0f;
      }
      const int32_t m = hs.fmat[f];
      memcpy(&r[3], &m, 4);
    }
  });
}

// the GPU builders bound the records' vertices: with a tilted normal anywhere (hs.av non-empty) they get
// the accept-region vertices, and world_records puts the world vertices back into the built leaf order
static void set_verts(TriRec64& r, const f3& w0, const f3& w1, const f3& w2) {
  r.w0x = w0.x; r.w0y = w0.y; r.w0z = w0.z;
  r.w1x = w1.x; r.w1y = w1.y; r.w1z = w1.z;
  r.w2x = w2.x; r.w2y = w2.y; r.w2z = w2.z;
}
static void bound_records(const HostScene& hs, std::vector<TriRec64>& recs) {
  if (hs.av.empty()) return;
  parallel_chunks(recs.size(), [&](size_t b, size_t e, int) {
    for (size_t i = b; i < e; i++) {
      TriRec64& r = recs[i];
      set_verts(r, bound_vert(hs, r.face, 0), bound_vert(hs, r.face, 1), bound_vert(hs, r.face, 2));
    }
  });
}
// the device builders take scenes whose culling bounds are finite and well inside the float range (their
// bin arithmetic, Morton codes and surface areas stay finite); anything else is built on the host
static bool device_buildable(const std::vector<TriRec64>& recs) {
  std::atomic<bool> ok{true};
  parallel_chunks(recs.size(), [&](size_t b, size_t e, int) {
    for (size_t i = b; i < e && ok.load(std::memory_order_relaxed); i++) {
      const TriRec64& r = recs[i];
      const float v[9] = {r.w0x, r.w0y, r.w0z, r.w1x, r.w1y, r.w1z, r.w2x, r.w2y, r.w2z};
      for (float x : v)
        if (!(std::fabs(x) <= 1e30f)) ok = false;  // NaN fails too
    }
  });
  return ok.load();
}
static void world_records(HostScene& hs) {
  if (hs.av.empty()) return;
  parallel_chunks(hs.tris.size(), [&](size_t b, size_t e, int) {
    for (size_t i = b; i < e; i++) {
      TriRec64& r = hs.tris[i];
      const uint32_t* v = &hs.fidx[3 * (size_t)r.face];
      set_verts(r, hs.wv[v[0]], hs.wv[v[1]], hs.wv[v[2]]);
    }
  });
}

// (a node's traversal-order hint: octant_order, rt_internal.h)

// interior nodes re-laid out depth-first (near child first) from `root`; unreferenced nodes dropped;
// sets hs.nodes, hs.root = 0, hs.depth (levels of interior nodes + the leaf level)
// Sibling-pair layout (RT_NODE_LAYOUT=pairs, A/B): the two interior children of a node occupy one
// 128-B aligned pair of records (one L2 line on MI355X), depth first over the pairs; a node with one
// interior child leaves the second record of its pair empty (never referenced). Root at 0, record 1 empty.
static void relayout_pairs(HostScene& hs, const std::vector<Node64>& tmp, uint32_t root) {
  Node64 empty;
  memset(&empty, 0, sizeof empty);
  empty.c0lx = empty.c0ly = empty.c0lz = empty.c1lx = empty.c1ly = empty.c1lz = INFINITY;
  empty.c0hx = empty.c0hy = empty.c0hz = empty.c1hx = empty.c1hy = empty.c1hz = -INFINITY;
  empty.child0 = empty.child1 = make_leaf(0, 1);
  std::vector<uint32_t> remap(tmp.size(), UINT32_MAX);
  std::vector<uint32_t> slot_src{root, UINT32_MAX};  // record index -> source node (UINT32_MAX = empty)
  remap[root] = 0;
  std::vector<std::pair<uint32_t, int>> st{{root, 1}};
  int depth = 0;
  while (!st.empty()) {
    const auto [n, d] = st.back();
    st.pop_back();
    depth = std::max(depth, d + 1);
    const Node64& nd = tmp[n];
    const bool i0 = !is_leaf(nd.child0), i1 = !is_leaf(nd.child1);
    if (!i0 && !i1) continue;
    const uint32_t base = (uint32_t)slot_src.size();
    slot_src.push_back(UINT32_MAX);
    slot_src.push_back(UINT32_MAX);
    uint32_t k = base;
    if (i0) { remap[nd.child0] = k; slot_src[k++] = nd.child0; }
    if (i1) { remap[nd.child1] = k; slot_src[k++] = nd.child1; }
    if (i1) st.push_back({nd.child1, d + 1});
    if (i0) st.push_back({nd.child0, d + 1});
  }
  hs.nodes.resize(slot_src.size());
  hs.leaves = 0;
  for (size_t i = 0; i < slot_src.size(); i++) {
    if (slot_src[i] == UINT32_MAX) { hs.nodes[i] = empty; continue; }
    Node64 nd = tmp[slot_src[i]];
    if (!is_leaf(nd.child0)) nd.child0 = remap[nd.child0];
    if (!is_leaf(nd.child1)) nd.child1 = remap[nd.child1];
    hs.leaves += (int)is_leaf(nd.child0) + (int)is_leaf(nd.child1);
    nd.pad0 = octant_order(nd);
    hs.nodes[i] = nd;
  }
  hs.root = 0;
  hs.depth = depth;
}

void relayout_dfs(HostScene& hs, const std::vector<Node64>& tmp, uint32_t root) {
  const char* layout_env = debug_env("RT_NODE_LAYOUT");
  const bool pairs = layout_env && !strcmp(layout_env, "pairs");
  if (pairs) { relayout_pairs(hs, tmp, root); return; }
  const size_t N = tmp.size();
  std::vector<uint32_t> remap(N, UINT32_MAX), order;
  int depth = 0;
  // Every builder allocates a node's children after the node itself (child index > parent index). Then the
  // pre-order position follows from subtree sizes in two streaming sweeps over tmp: sizes from the back,
  // positions (and levels) from the front -- pos(child0) = pos + 1, pos(child1) = pos + 1 + size(child0) --
  // the order the explicit-stack walk below gives, without its dependent random accesses (1M-node trees:
  // ~5x faster). Any child at a lower index than its parent takes the walk.
  bool forward = root < N;
  std::vector<uint32_t> size(N, 1);
  for (size_t i = N; forward && i-- > 0;) {
    const Node64& nd = tmp[i];
    for (uint32_t c : {nd.child0, nd.child1}) {
      if (is_leaf(c)) continue;
      if (c <= i || c >= N) { forward = false; break; }
      size[i] += size[c];
    }
  }
  if (forward) {
    std::vector<uint8_t> lev(N, 0);
    remap[root] = 0;
    lev[root] = 1;
    order.assign(size[root], UINT32_MAX);
    for (size_t i = root; i < N; i++) {
      const uint32_t p = remap[i];
      if (p == UINT32_MAX) continue;  // not reachable from root
      order[p] = (uint32_t)i;
      depth = std::max(depth, lev[i] + 1);
      const Node64& nd = tmp[i];
      uint32_t next = p + 1;
      for (uint32_t c : {nd.child0, nd.child1}) {
        if (is_leaf(c)) continue;
        remap[c] = next;
        lev[c] = (uint8_t)std::min(lev[i] + 1, 255);
        next += size[c];
      }
    }
  } else {
    std::fill(remap.begin(), remap.end(), UINT32_MAX);
    std::vector<std::pair<uint32_t, int>> st{{root, 1}};
    while (!st.empty()) {
      const auto [n, d] = st.back();
      st.pop_back();
      remap[n] = (uint32_t)order.size();
      order.push_back(n);
      depth = std::max(depth, d + 1);
      const Node64& nd = tmp[n];
      if (!is_leaf(nd.child1)) st.push_back({nd.child1, d + 1});
      if (!is_leaf(nd.child0)) st.push_back({nd.child0, d + 1});
    }
  }
  hs.nodes.resize(order.size());
  int leaves[16] = {};
  const int T = parallel_chunks(order.size(), [&](size_t b, size_t e, int t) {
    int lv = 0;  // thread-local count (no false sharing on leaves[])
    for (size_t i = b; i < e; i++) {
      Node64 nd = tmp[order[i]];
      if (!is_leaf(nd.child0)) nd.child0 = remap[nd.child0];
      if (!is_leaf(nd.child1)) nd.child1 = remap[nd.child1];
      lv += (int)is_leaf(nd.child0) + (int)is_leaf(nd.child1);
      nd.pad0 = octant_order(nd);
      hs.nodes[i] = nd;
    }
    leaves[t] = lv;
  });
  hs.root = 0;
  hs.depth = depth;
  hs.leaves = 0;
  for (int t = 0; t < T; t++) hs.leaves += leaves[t];
}

// What every device builder starts from: the bounds of what it builds over and the face records with the
// vertices to bound; false when the scene is not device-buildable
static bool gpu_build_inputs(const HostScene& hs, float lo[3], float hi[3], std::vector<TriRec64>& recs) {
  world_bounds(hs, lo, hi);
  face_records(hs, recs);
  bound_records(hs, recs);
  return device_buildable(recs);
}
// ... and ends with: a device-built tree (root 0) is re-laid out on trial and refused, with nothing changed,
// when it is too deep for the wave stack (the caller builds a host SAH tree instead); else it becomes the
// scene's, with `tris` its records. accepted(depth) runs between the two (the builders' RT_TIMING lines; it
// may still fill `tris`), pt gets the sbvh-gpu phase marks.
static bool adopt_tree(HostScene& hs, const std::vector<Node64>& tmp, std::vector<TriRec64>& tris,
                       const std::function<void(int)>& accepted = nullptr, PhaseTimer* pt = nullptr) {
  HostScene trial;
  relayout_dfs(trial, tmp, 0);
  if (trial.depth > kMaxDepth + 2) return false;
  if (accepted) accepted(trial.depth);
  hs.nodes = std::move(trial.nodes);
  hs.root = 0;
  hs.depth = trial.depth;
  hs.leaves = trial.leaves;
  hs.tris = std::move(tris);
  if (pt) pt->mark("tris");
  world_records(hs);
  if (pt) pt->mark("world_records");
  return true;
}

// GPU LBVH (rt_build.hip) + host depth-first re-layout; false (with nothing changed) if the device
// build is not possible, in which case the caller builds on the host
bool build_bvh_gpu(HostScene& hs, int device, int leaf_size, double* gpu_ms) {
  if (hs.nf <= leaf_size || hs.nf < 2) return false;
  float lo[3], hi[3];
  std::vector<TriRec64> recs, tris;
  if (!gpu_build_inputs(hs, lo, hi, recs)) return false;
  std::vector<Node64> tmp;
  if (gpu_build_lbvh(device, recs, lo, hi, std::max(1, std::min(leaf_size, kMaxLeaf)), bvh_pad(lo, hi), tmp, tris,
                     gpu_ms) != RT_OK)
    return false;
  return adopt_tree(hs, tmp, tris);
}

// GPU PLOC (rt_build.hip gpu_build_ploc) + host layout: the device returns the clustered binary tree
// (n - 1 interior nodes, root n - 2) with the SAH collapse flags; here its kept interior nodes get
// pre-order indices, every collapsed subtree / single triangle becomes a leaf whose triangles take
// consecutive slots in depth-first order (child 0 first), and relayout_dfs re-lays out the nodes as for the
// host builders. false (nothing changed) when the device build is impossible or the tree too deep.
// clusters searched either side: on the C3 soup a wider search gives a worse tree (radius 4 / 16 / 32: SAH
// cost 506 / 513 / 517, C3 8.3 / 7.0 / 6.3 Grays/s, profiles/ab/r04_builders.txt), so 4, not the paper's ~25
constexpr int kPlocRadius = 4;
constexpr float kPlocTrav = 0.7f;     // node-step cost relative to a triangle test (as the host builders)
bool build_bvh_ploc(HostScene& hs, int device, int leaf_size, double* gpu_ms) {
  if (hs.nf < 2) return false;
  float lo[3], hi[3];
  std::vector<TriRec64> recs;
  if (!gpu_build_inputs(hs, lo, hi, recs)) return false;
  std::vector<int32_t> child;
  std::vector<float> box;
  std::vector<uint8_t> leaf;
  int iters = 0;
  const int lb = std::max(1, std::min(leaf_size, kMaxLeaf));
  int radius = kPlocRadius, rule = 0;
  float trav = kPlocTrav;
  if (const char* e = debug_env("RT_PLOC_RADIUS")) radius = std::max(1, std::min(32, atoi(e)));
  if (const char* e = debug_env("RT_PLOC_TRAV")) trav = std::max(0.05f, (float)atof(e));
  if (const char* e = debug_env("RT_PLOC_RULE")) rule = atoi(e);
  if (gpu_build_ploc(device, recs, lo, hi, lb, radius, trav, child, box, leaf, gpu_ms, &iters, rule) != RT_OK)
    return false;
  const int n = hs.nf, ni = n - 1, root = n - 2;
  const float pad = bvh_pad(lo, hi);
  // pre-order walk (child 0 first): kept interior nodes get tmp indices, leaves get their slots
  std::vector<uint32_t> handle_int((size_t)ni, 0), handle_tri((size_t)n, 0);
  std::vector<int32_t> kept;  // tmp index -> PLOC node
  std::vector<TriRec64> tris;
  tris.reserve((size_t)n);
  std::vector<int32_t> st{root}, sub;
  auto tri_of = [&](int32_t c) { return (uint32_t)~c; };
  while (!st.empty()) {
    const int32_t c = st.back();
    st.pop_back();
    if (c < 0) {  // a single-triangle leaf
      handle_tri[tri_of(c)] = make_leaf((uint32_t)tris.size(), 1u);
      tris.push_back(recs[tri_of(c)]);
    } else if (leaf[(size_t)c] && c != root) {  // a collapsed subtree: its triangles in depth-first order
      const uint32_t first = (uint32_t)tris.size();
      sub.assign(1, c);
      while (!sub.empty()) {
        const int32_t q = sub.back();
        sub.pop_back();
        if (q < 0) { tris.push_back(recs[tri_of(q)]); continue; }
        sub.push_back(child[2 * (size_t)q + 1]);
        sub.push_back(child[2 * (size_t)q]);
      }
      handle_int[(size_t)c] = make_leaf(first, (uint32_t)tris.size() - first);
    } else {
      handle_int[(size_t)c] = (uint32_t)kept.size();
      kept.push_back(c);
      st.push_back(child[2 * (size_t)c + 1]);
      st.push_back(child[2 * (size_t)c]);
    }
  }
  std::vector<Node64> tmp(kept.size());
  for (size_t k = 0; k < kept.size(); k++) {
    const int32_t q = kept[k];
    Node64 nd{};
    for (int side = 0; side < 2; side++) {
      const int32_t c = child[2 * (size_t)q + side];
      float b[6];  // lo xyz, hi xyz
      uint32_t h;
      if (c < 0) {
        const TriRec64& t = recs[tri_of(c)];
        b[0] = std::min(std::min(t.w0x, t.w1x), t.w2x); b[3] = std::max(std::max(t.w0x, t.w1x), t.w2x);
        b[1] = std::min(std::min(t.w0y, t.w1y), t.w2y); b[4] = std::max(std::max(t.w0y, t.w1y), t.w2y);
        b[2] = std::min(std::min(t.w0z, t.w1z), t.w2z); b[5] = std::max(std::max(t.w0z, t.w1z), t.w2z);
        h = handle_tri[tri_of(c)];
      } else {
        for (int j = 0; j < 6; j++) b[j] = box[6 * (size_t)c + j];
        h = handle_int[(size_t)c];
      }
      set_child(nd, side, b, b + 3, pad, h);
    }
    tmp[k] = nd;
  }
  return adopt_tree(hs, tmp, tris, [&](int depth) {
    if (debug_env("RT_TIMING")) fprintf(stderr, "[rt] ploc: %d iterations, %zu nodes, depth %d\n", iters, tmp.size(), depth);
  });
}

// GPU top-down binned SAH (rt_build.hip gpu_build_sah) + host layout: interior node 0 is the root, child
// handles are node ids or leaf handles over the returned slot order; the host pads the boxes and re-lays
// the nodes out depth first. false (nothing changed) when the device build is impossible or too deep.
bool build_bvh_sah_gpu(HostScene& hs, int device, int leaf_size, bool spatial, double* gpu_ms) {
  if (hs.nf < 2) return false;
  PhaseTimer pt("sbvh-gpu");
  float lo[3], hi[3];
  std::vector<TriRec64> recs;
  if (!gpu_build_inputs(hs, lo, hi, recs)) return false;
  pt.mark("records");
  std::vector<uint32_t> nchild, slot_face;
  std::vector<float> ncb;
  int levels = 0;
  float trav = 0.7f;
  if (const char* e = debug_env("RT_SAH_TRAV")) trav = std::max(0.05f, (float)atof(e));
  float budget = 0.5f;  // as the host SBVH (rt_builders.cpp build_sbvh)
  if (const char* e = debug_env("RT_SBVH_BUDGET")) budget = std::max(0.0f, (float)atof(e));
  constexpr float kSbvhGpuAlpha = 1e-3f;  // the host SBVH's overlap threshold (build_bvh)
  if (gpu_build_sah(device, recs, lo, hi, std::max(1, std::min(leaf_size, kMaxLeaf)), trav, spatial, budget, kSbvhGpuAlpha,
                    nchild, ncb, slot_face, gpu_ms, &levels) != RT_OK)
    return false;
  pt.mark("gpu_build_sah");
  const size_t nn = nchild.size() / 2;
  const float pad = bvh_pad(lo, hi);
  std::vector<Node64> tmp(nn);
  std::atomic<bool> bad{false};
  parallel_chunks(nn, [&](size_t kb, size_t ke, int) {
    for (size_t k = kb; k < ke; k++) {
      Node64 nd{};
      for (int side = 0; side < 2; side++) {
        const float* b = &ncb[12 * k + 6 * side];  // lo xyz, hi xyz
        const uint32_t h = nchild[2 * k + side];
        if (!is_leaf(h) && h >= nn) bad = true;
        set_child(nd, side, b, b + 3, pad, h);
      }
      tmp[k] = nd;
    }
  });
  if (bad) return false;
  pt.mark("nodes");
  std::vector<TriRec64> tris;
  return adopt_tree(hs, tmp, tris, [&](int depth) {
    pt.mark("relayout");
    if (debug_env("RT_TIMING"))
      fprintf(stderr, "[rt] %s: %d levels, %zu nodes, %zu references, depth %d\n", spatial ? "sbvh-gpu" : "sah-gpu", levels, nn,
              slot_face.size(), depth);
    tris.resize(slot_face.size());
    parallel_chunks(slot_face.size(), [&](size_t b, size_t e, int) {
      for (size_t sl = b; sl < e; sl++) tris[sl] = recs[slot_face[sl]];
    });
  }, &pt);
}

// ---------------------------------------------------------------------------------------------------
// 4-wide collapse: each wide node takes a binary node's two children and keeps opening the interior
// child with the largest surface area until it has four children (or only leaves remain). Child
// boxes (already padded) are quantised outward to 8 bits on a per-node, per-axis power-of-two grid.
// ---------------------------------------------------------------------------------------------------
namespace {
float warea(const ChildBox& w) {
  float d[3];
  for (int k = 0; k < 3; k++) d[k] = std::max(0.0f, w.hi[k] - w.lo[k]);
  return d[0] * d[1] + d[1] * d[2] + d[2] * d[0];
}

void quantize(Node4Q& q, const ChildBox* ch, int n) {
  float L[3] = {INFINITY, INFINITY, INFINITY}, U[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int c = 0; c < n; c++)
    for (int k = 0; k < 3; k++) { L[k] = std::min(L[k], ch[c].lo[k]); U[k] = std::max(U[k], ch[c].hi[k]); }
  uint8_t eb[3];
  double scale[3];
  for (int k = 0; k < 3; k++) {
    const double ext = (double)U[k] - (double)L[k];
    int e = -100;
    if (ext > 0) {
      e = (int)std::ceil(std::log2(ext / 255.0));
      while (std::ldexp(255.0, e) < ext) e++;
      e = std::max(e, -100);
    }
    eb[k] = (uint8_t)(e + 127);
    scale[k] = std::ldexp(1.0, e);
  }
  q.ox = L[0]; q.oy = L[1]; q.oz = L[2];
  q.ex = eb[0]; q.ey = eb[1]; q.ez = eb[2];
  q.valid = 0;
  uint32_t* ql[3] = {&q.qlx, &q.qly, &q.qlz};
  uint32_t* qh[3] = {&q.qhx, &q.qhy, &q.qhz};
  for (int k = 0; k < 3; k++) { *ql[k] = 0; *qh[k] = 0; }
  const double org[3] = {q.ox, q.oy, q.oz};
  for (int c = 0; c < 4; c++) {
    if (c >= n) { q.child[c] = 0; continue; }
    q.valid |= (uint8_t)(1u << c);
    q.child[c] = ch[c].h;
    for (int k = 0; k < 3; k++) {
      double a = std::floor(((double)ch[c].lo[k] - org[k]) / scale[k]);
      double b = std::ceil(((double)ch[c].hi[k] - org[k]) / scale[k]);
      a = std::min(std::max(a, 0.0), 255.0);
      b = std::min(std::max(b, 0.0), 255.0);
      while (a > 0 && org[k] + a * scale[k] > (double)ch[c].lo[k]) a -= 1;
      while (b < 255 && org[k] + b * scale[k] < (double)ch[c].hi[k]) b += 1;
      *ql[k] |= (uint32_t)a << (8 * c);
      *qh[k] |= (uint32_t)b << (8 * c);
    }
  }
  q.pad0 = q.pad1 = 0;
}

// the walk both collapses share; emit(record, children, n) writes one wide node from its n children, whose
// handles are leaf handles or the indices of the wide nodes made for them
template <typename Rec, typename Emit>
uint32_t collapse(const std::vector<Node64>& bin, uint32_t n2, std::vector<Rec>& out, int depth, int& maxd, Emit&& emit) {
  maxd = std::max(maxd, depth);
  ChildBox ch[4] = {child_box(bin[n2], 0), child_box(bin[n2], 1)};
  int n = is_sentinel_child(bin[n2], 1) ? 1 : 2;  // a single-leaf root's never-hit child is dropped
  while (n < 4) {
    int best = -1;
    float ba = -1.0f;
    for (int c = 0; c < n; c++)
      if (!is_leaf(ch[c].h) && warea(ch[c]) > ba) { ba = warea(ch[c]); best = c; }
    if (best < 0) break;
    const Node64& sub = bin[ch[best].h];
    ch[best] = child_box(sub, 0);
    ch[n++] = child_box(sub, 1);
  }
  const uint32_t me = (uint32_t)out.size();
  out.emplace_back();
  for (int c = 0; c < n; c++)
    if (!is_leaf(ch[c].h)) ch[c].h = collapse(bin, ch[c].h, out, depth + 1, maxd, emit);
  emit(out[me], ch, n);
  return me;
}
}  // namespace

void build_bvh4(HostScene& hs) {
  hs.nodes4.clear();
  hs.depth4 = 0;
  if (hs.nodes.empty()) return;
  hs.nodes4.reserve(hs.nodes.size() / 2 + 1);
  int maxd = 0;
  collapse(hs.nodes, hs.root, hs.nodes4, 0, maxd, quantize);
  hs.depth4 = maxd + 1;
}
// (the wide traversal pushes at most 3 entries per level and writes up to 3 slots past the top)

// ---------------------------------------------------------------------------------------------------
// fp32 4-wide tree (Node128 on the device): the same collapse as above (each wide node opens the interior
// child of largest surface area until it has four children), with the BVH2 child boxes kept exactly --
// they are already padded, so culling stays conservative -- and, per ray-direction octant, the children's
// near-to-far order. Order rule (the binary tree's octant_order, pairwise): of two children, along the
// axis on which their centres are furthest apart, the one on the ray's entry side of that axis comes
// first (insertion sort; only the visit order depends on it, never a result).
// ---------------------------------------------------------------------------------------------------
namespace {
bool wide_before(const float* a, const float* b, uint32_t oct) {
  int axis = 0;
  float best = -1.0f;
  for (int k = 0; k < 3; k++) {
    const float sep = std::fabs((b[2 * k] + b[2 * k + 1]) - (a[2 * k] + a[2 * k + 1]));
    if (sep > best) best = sep, axis = k;
  }
  const float ca = a[2 * axis] + a[2 * axis + 1], cb = b[2 * axis] + b[2 * axis + 1];
  return ((oct >> axis) & 1u) ? ca > cb : ca < cb;
}

void wide_record(Wide4& w, const ChildBox* ch, int n) {
  memset(&w, 0, sizeof w);
  w.n = (uint8_t)n;
  for (int c = 0; c < 4; c++) {
    for (int k = 0; k < 3; k++) {
      w.box[c][2 * k] = c < n ? ch[c].lo[k] : INFINITY;
      w.box[c][2 * k + 1] = c < n ? ch[c].hi[k] : -INFINITY;
    }
    w.child[c] = c < n ? ch[c].h : kWideEmpty;
  }
  for (uint32_t oct = 0; oct < 8; oct++) {
    uint8_t* o = w.order[oct];
    for (int c = 0; c < 4; c++) o[c] = (uint8_t)c;
    for (int i = 1; i < n; i++)  // insertion sort of the occupied slots; empty slots stay last
      for (int j = i; j > 0 && wide_before(w.box[o[j]], w.box[o[j - 1]], oct); j--) std::swap(o[j], o[j - 1]);
  }
}
}  // namespace

void build_wide(HostScene& hs) {
  hs.wide.clear();
  hs.depth_wide = 0;
  if (hs.nodes.empty() || is_leaf(hs.root)) return;
  hs.wide.reserve(hs.nodes.size() / 2 + 1);
  int maxd = 0;
  collapse(hs.nodes, hs.root, hs.wide, 0, maxd, wide_record);
  hs.depth_wide = maxd + 1;
  if (3 * hs.depth_wide + 4 > kStackW) {  // too deep for the wave stack: binary traversal only
    hs.wide.clear();
    hs.depth_wide = 0;
  }
}

}  // namespace rt
