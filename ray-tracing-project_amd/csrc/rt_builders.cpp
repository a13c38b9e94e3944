// rt_builders.cpp -- the host tree builders: binned SAH (BvhBuilder) and spatial-split SBVH (SbvhBuilder),
// a BVH2 over the bounds of what each face's edge tests can accept, handed to rt_layout.cpp for the
// depth-first re-layout. Child boxes are padded outward so node culling is conservative with respect to the
// reference's (rounded) triangle test (src/flyscene.cpp:459-465,580-590 in plindhorst/Ray-Tracing-Project):
// a triangle the reference accepts is never behind a culled box. The reference itself has no tree (its flat
// boxes: rt_refboxes.cpp), so only the time depends on these, never a result.
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <future>

#include "rt_host.h"

namespace rt {
namespace {
struct Prim {
  float lo[3], hi[3], c[3];
  uint32_t id;  // face index
};

// one more concurrent subtree task if fewer than `cap` run (the build order and result do not depend on it)
static bool take_task(std::atomic<int>& live, unsigned cap) {
  if (live.fetch_add(1) < (int)cap) return true;
  live.fetch_sub(1);
  return false;
}

constexpr int kBins = 32;
constexpr float kIsect = 1.0f;
// per axis and bin: the bounds and count of what entered it (cnt2: what exits there, spatial bins only)
struct Bins {
  Aabb box[3][kBins];
  uint32_t cnt[3][kBins] = {}, cnt2[3][kBins] = {};
  void clear() { *this = Bins(); }
  void merge(const Bins& o) {
    for (int k = 0; k < 3; k++)
      for (int i = 0; i < kBins; i++) { box[k][i].merge(o.box[k][i]); cnt[k][i] += o.cnt[k][i]; cnt2[k][i] += o.cnt2[k][i]; }
  }
};
// best plane of binned boxes on axis k: left of plane i = bins 0..i (counted by cnt), right = bins
// i+1.. (counted by cnt2 for spatial bins, cnt otherwise)
void sweep(const Bins& B, int k, bool spatial, float& best, int& axis, int& bin, Aabb* lbest = nullptr, Aabb* rbest = nullptr) {
  const uint32_t* rcnt = spatial ? B.cnt2[k] : B.cnt[k];
  Aabb racc[kBins];
  uint32_t rc[kBins];
  Aabb acc;
  uint32_t c = 0;
  for (int i = kBins - 1; i > 0; i--) { acc.merge(B.box[k][i]); c += rcnt[i]; racc[i] = acc; rc[i] = c; }
  Aabb lacc;
  uint32_t lc = 0;
  for (int i = 0; i < kBins - 1; i++) {
    lacc.merge(B.box[k][i]);
    lc += B.cnt[k][i];
    if (lc == 0 || rc[i + 1] == 0) continue;
    const float cost = lacc.area() * lc + racc[i + 1].area() * rc[i + 1];
    if (cost < best) {
      best = cost; axis = k; bin = i;
      if (lbest) { *lbest = lacc; *rbest = racc[i + 1]; }
    }
  }
}

// Binned SAH over the working array of primitives (partitioned in place, so a subtree's primitives are
// contiguous and become the leaf order). Large ranges bin and bound in parallel chunks (min/max/count
// merges are order-independent, so the splits do not depend on the thread count); subtrees above
// 16k primitives build as separate tasks.
struct BvhBuilder {
  std::vector<Prim>& prims;
  std::vector<Node64>& nodes;
  std::atomic<uint32_t> next{0};
  int leaf_size;
  float pad;
  unsigned hw = 1;
  std::atomic<int> max_depth{0}, leaves{0};
  // concurrent subtree tasks of this build, at most hw (a torchrun job builds one scene per rank on the
  // same host: without a bound each rank would start ~250 threads at once)
  std::atomic<int> tasks{0};
  // node-visit cost relative to one triangle test (RT_SAH_TRAV, A/B knob). 0.7: once the packet node
  // step had lost its SALU overhead (order bits, byte handles) a node became cheaper than a triangle
  // test; measured C3 7,440 -> 7,810 Mrays/s (0.3-0.5 within 2% of 0.7, 1.5 -11%), bunny +1-2%
  float kTrav = 0.7f;

  // builds [b,e); returns the handle and the (unpadded) bounds of the subtree
  uint32_t build(uint32_t b, uint32_t e, int depth, Aabb& box) {
    const uint32_t n = e - b;
    Aabb cb;
    {
      Aabb pb[16], pc[16];
      const int T = parallel_chunks(b, e, [&](size_t lo, size_t hi, int t) {
        Aabb a, c;  // thread-local, stored once (no false sharing on pb / pc)
        for (size_t i = lo; i < hi; i++) { a.grow(prims[i].lo, prims[i].hi); c.growp(prims[i].c); }
        pb[t] = a;
        pc[t] = c;
      });
      box = Aabb();
      for (int t = 0; t < T; t++) { box.merge(pb[t]); cb.merge(pc[t]); }
    }
    int md = max_depth.load();
    while (depth > md && !max_depth.compare_exchange_weak(md, depth)) {}
    auto make_leaf_h = [&]() { leaves++; return make_leaf(b, n); };
    if (n == 1) return make_leaf_h();
    // choose split
    int axis = -1;
    uint32_t mid = b;
    float best_cost = INFINITY;
    float ext[3];
    for (int k = 0; k < 3; k++) ext[k] = cb.hi[k] - cb.lo[k];
    const bool force_median = depth >= kMaxDepth - 20;
    if (!force_median) {
      int best_bin = -1;
      float sc[3];
      for (int k = 0; k < 3; k++) sc[k] = ext[k] > 0.0f ? kBins / ext[k] : 0.0f;
      // one pass bins all three axes
      std::vector<Bins> part((size_t)chunk_count(n));
      const int T = parallel_chunks(b, e, [&](size_t lo, size_t hi, int t) {
        Bins& B = part[t];
        for (size_t i = lo; i < hi; i++) {
          const Prim& p = prims[i];
          for (int k = 0; k < 3; k++) {
            if (!(ext[k] > 0.0f)) continue;
            const int bi = std::min(kBins - 1, (int)((p.c[k] - cb.lo[k]) * sc[k]));
            B.box[k][bi].grow(p.lo, p.hi);
            B.cnt[k][bi]++;
          }
        }
      });
      for (int t = 1; t < T; t++) part[0].merge(part[t]);
      for (int k = 0; k < 3; k++)
        if (ext[k] > 0.0f) sweep(part[0], k, false, best_cost, axis, best_bin);
      const float parent_area = std::max(box.area(), 1e-30f);
      const float split_cost = kTrav + kIsect * best_cost / parent_area;
      if ((int)n <= leaf_size && (axis < 0 || (float)n * kIsect <= split_cost)) return make_leaf_h();
      if (axis >= 0) {
        const float s = sc[axis];
        const float lo = cb.lo[axis];
        auto it = std::partition(prims.begin() + b, prims.begin() + e, [&](const Prim& p) {
          return std::min(kBins - 1, (int)((p.c[axis] - lo) * s)) <= best_bin;
        });
        mid = (uint32_t)(it - prims.begin());
      }
    } else if ((int)n <= leaf_size) {
      return make_leaf_h();
    }
    if (axis < 0 || mid == b || mid == e) {
      // degenerate centroids or forced: object median along the widest centroid axis
      if ((int)n <= kMaxLeaf && !(ext[0] > 0 || ext[1] > 0 || ext[2] > 0)) return make_leaf_h();
      int k = (ext[0] >= ext[1] && ext[0] >= ext[2]) ? 0 : (ext[1] >= ext[2] ? 1 : 2);
      mid = b + n / 2;
      std::nth_element(prims.begin() + b, prims.begin() + mid, prims.begin() + e,
                       [&](const Prim& x, const Prim& y) { return x.c[k] < y.c[k]; });
    }
    const uint32_t me = next.fetch_add(1);
    Aabb lb, rb;
    uint32_t lh, rh;
    if (n > 4096 && depth < 16 && take_task(tasks, hw)) {
      auto fut = std::async(std::launch::async, [&]() { return build(b, mid, depth + 1, lb); });
      rh = build(mid, e, depth + 1, rb);
      lh = fut.get();
      tasks.fetch_sub(1);
    } else {
      lh = build(b, mid, depth + 1, lb);
      rh = build(mid, e, depth + 1, rb);
    }
    Node64 nd{};
    set_child(nd, 0, lb, pad, lh);
    set_child(nd, 1, rb, pad, rh);
    nodes[me] = nd;
    return me;
  }
};

// Spatial-split BVH (SBVH: object splits as above, plus splits of the space that cut triangles
// straddling the plane into two references with clipped bounds; the host builder's default when
// RT_BUILDER_SBVH). A triangle referenced by several leaves is tested more than once, with
// identical (t, rank), so the (t, rank) argmin, hence every result, is unchanged; culling stays
// conservative because each reference's box bounds the part of the triangle it stands for (clip
// points in double, rounded outward) and every child box is padded as before.
struct SbvhBuilder {
  const HostScene& hs;
  std::vector<Node64>& nodes;                      // sized to the node capacity
  std::vector<std::vector<uint32_t>> leaf_lists;   // face ids per leaf, sized to the leaf capacity
  std::atomic<uint32_t> next{0}, nleaf{0};
  std::atomic<int64_t> refs{0};  // references made (statistics); the budget itself is per subtree
  int leaf_size = 4;
  float pad = 0.0f, kTrav = 0.7f, alpha = 1e-5f, root_area = 1.0f;
  std::atomic<int> max_depth{0};
  std::atomic<int> tasks{0};  // concurrent subtree tasks, at most hw (as BvhBuilder)
  unsigned hw = 1;

  void verts(uint32_t f, double v[3][3]) const {
    for (int j = 0; j < 3; j++) {
      const f3& w = bound_vert(hs, f, j);
      v[j][0] = w.x; v[j][1] = w.y; v[j][2] = w.z;
    }
  }
  static float down(double x) { float f = (float)x; return (double)f > x ? std::nextafter(f, -INFINITY) : f; }
  static float up(double x) { float f = (float)x; return (double)f < x ? std::nextafter(f, INFINITY) : f; }
  // bounds of (triangle f) within [a, b] on axis k, intersected with `within`; false if empty
  bool clip(uint32_t f, int k, float a, float b, const Prim& within, Prim& out) const {
    double v[3][3];
    verts(f, v);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    auto add = [&](const double* q) {
      for (int i = 0; i < 3; i++) { lo[i] = std::min(lo[i], q[i]); hi[i] = std::max(hi[i], q[i]); }
    };
    for (int j = 0; j < 3; j++) {
      const double* p = v[j];
      const double* q = v[(j + 1) % 3];
      if (p[k] >= a && p[k] <= b) add(p);
      for (double pl : {(double)a, (double)b}) {
        if ((p[k] < pl && q[k] > pl) || (p[k] > pl && q[k] < pl)) {
          const double t = (pl - p[k]) / (q[k] - p[k]);
          double x[3];
          for (int i = 0; i < 3; i++) x[i] = p[i] + t * (q[i] - p[i]);
          x[k] = pl;
          add(x);
        }
      }
    }
    out.id = f;
    for (int i = 0; i < 3; i++) {
      out.lo[i] = std::max(down(lo[i]), within.lo[i]);
      out.hi[i] = std::min(up(hi[i]), within.hi[i]);
      if (i == k) { out.lo[i] = std::max(out.lo[i], a); out.hi[i] = std::min(out.hi[i], b); }
      if (!(out.lo[i] <= out.hi[i])) return false;
      out.c[i] = 0.5f * (out.lo[i] + out.hi[i]);
    }
    return true;
  }

  uint32_t leaf(std::vector<Prim>& r) {
    const uint32_t li = nleaf.fetch_add(1);
    std::vector<uint32_t>& ids = leaf_lists[li];
    ids.reserve(r.size());
    for (const Prim& p : r) ids.push_back(p.id);
    const uint32_t n = (uint32_t)r.size();
    std::vector<Prim>().swap(r);
    return make_leaf(li, n);  // leaf index for now; triangle slots are assigned depth first afterwards
  }

  // builds the subtree over `r` (consumed); returns its handle and the bounds of its references.
  // budget: references this subtree may add by spatial splits. Each split spends what it duplicates and
  // hands the rest to its children in proportion to their reference counts, so the tree (which splits
  // are taken) never depends on the order the parallel subtree tasks run in.
  uint32_t build(std::vector<Prim>& r, int depth, Aabb& box, int64_t budget) {
    const uint32_t n = (uint32_t)r.size();
    Aabb cb;
    box = Aabb();
    {
      Aabb pb[16], pc[16];
      const int T = parallel_chunks(n, [&](size_t b, size_t e, int t) {
        Aabb a, c;  // thread-local, stored once
        for (size_t i = b; i < e; i++) { a.grow(r[i].lo, r[i].hi); c.growp(r[i].c); }
        pb[t] = a;
        pc[t] = c;
      });
      for (int t = 0; t < T; t++) { box.merge(pb[t]); cb.merge(pc[t]); }
    }
    int md = max_depth.load();
    while (depth > md && !max_depth.compare_exchange_weak(md, depth)) {}
    if (n == 1) return leaf(r);
    const bool forced = depth >= kMaxDepth - 20;
    const float parent_area = std::max(box.area(), 1e-30f);
    const int TB = chunk_count(n);
    std::vector<Bins> part((size_t)TB);
    // object split: binned SAH over reference centroids
    int o_axis = -1, o_bin = -1;
    float o_cost = INFINITY;
    Aabb o_lb, o_rb;
    float ext[3], sc[3];
    for (int k = 0; k < 3; k++) { ext[k] = cb.hi[k] - cb.lo[k]; sc[k] = ext[k] > 0.0f ? kBins / ext[k] : 0.0f; }
    auto obin = [&](const Prim& p, int k) { return std::min(kBins - 1, (int)((p.c[k] - cb.lo[k]) * sc[k])); };
    if (!forced) {
      for (Bins& B : part) B.clear();
      const int T = parallel_chunks(n, [&](size_t b, size_t e, int t) {
        Bins& B = part[t];
        for (size_t i = b; i < e; i++)
          for (int k = 0; k < 3; k++) {
            if (!(ext[k] > 0.0f)) continue;
            const int bi = obin(r[i], k);
            B.box[k][bi].grow(r[i].lo, r[i].hi);
            B.cnt[k][bi]++;
          }
      });
      for (int t = 1; t < T; t++) part[0].merge(part[t]);
      for (int k = 0; k < 3; k++)
        if (ext[k] > 0.0f) sweep(part[0], k, false, o_cost, o_axis, o_bin, &o_lb, &o_rb);
    }
    // spatial split, tried when the object split's children overlap by more than alpha of the root:
    // kBins slabs per axis; a reference enters the bin of its low end, exits the bin of its high end,
    // and adds the bounds of its clipped part to every bin it spans
    int s_axis = -1, s_bin = -1;
    float s_cost = INFINITY;
    float pl[3][kBins + 1];
    float ov = 0.0f;
    if (o_axis >= 0) {
      float d[3];
      for (int k = 0; k < 3; k++) d[k] = std::max(0.0f, std::min(o_lb.hi[k], o_rb.hi[k]) - std::max(o_lb.lo[k], o_rb.lo[k]));
      ov = 2.0f * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
    }
    if (!forced && budget > 0 && (o_axis < 0 || ov > alpha * root_area)) {
      float w[3];
      for (int k = 0; k < 3; k++) {
        w[k] = (box.hi[k] - box.lo[k]) / kBins;
        for (int i = 0; i <= kBins; i++) pl[k][i] = box.lo[k] + w[k] * i;
        pl[k][kBins] = box.hi[k];
      }
      auto sbin = [&](float x, int k) {
        int bi = std::min(kBins - 1, std::max(0, (int)((x - box.lo[k]) / w[k])));
        while (bi > 0 && x < pl[k][bi]) bi--;
        while (bi < kBins - 1 && x >= pl[k][bi + 1]) bi++;
        return bi;
      };
      for (Bins& B : part) B.clear();
      const int T = parallel_chunks(n, [&](size_t b, size_t e, int t) {
        Bins& B = part[t];
        for (size_t i = b; i < e; i++) {
          const Prim& p = r[i];
          for (int k = 0; k < 3; k++) {
            if (!(w[k] > 0.0f)) continue;
            const int b0 = sbin(p.lo[k], k), b1 = sbin(p.hi[k], k);
            B.cnt[k][b0]++;
            B.cnt2[k][b1]++;
            if (b0 == b1) { B.box[k][b0].grow(p.lo, p.hi); continue; }
            for (int bi = b0; bi <= b1; bi++) {
              Prim q;
              if (clip(p.id, k, std::max(pl[k][bi], p.lo[k]), std::min(pl[k][bi + 1], p.hi[k]), p, q)) B.box[k][bi].grow(q.lo, q.hi);
            }
          }
        }
      });
      for (int t = 1; t < T; t++) part[0].merge(part[t]);
      for (int k = 0; k < 3; k++)
        if (w[k] > 0.0f) sweep(part[0], k, true, s_cost, s_axis, s_bin);
    }
    const float best = std::min(o_cost, s_cost);
    if (!forced && (int)n <= leaf_size && (best == INFINITY || (float)n * kIsect <= kTrav + kIsect * best / parent_area))
      return leaf(r);
    if (forced && (int)n <= leaf_size) return leaf(r);
    std::vector<Prim> L, R;
    bool spatial = s_axis >= 0 && s_cost < o_cost;
    const float s_pos = spatial ? pl[s_axis][s_bin + 1] : 0.0f;
    if (spatial) {
      // the references this split adds are reserved against the budget first (a hard bound on the
      // reference count, hence on the leaf and node storage); without room it is an object split
      std::vector<int64_t> cnt((size_t)TB, 0);
      const int T = parallel_chunks(n, [&](size_t b, size_t e, int t) {
        int64_t k = 0;  // thread-local
        for (size_t i = b; i < e; i++) k += r[i].lo[s_axis] < s_pos && r[i].hi[s_axis] > s_pos;
        cnt[t] = k;
      });
      int64_t straddle = 0;
      for (int t = 0; t < T; t++) straddle += cnt[t];
      if (straddle > budget) spatial = false;
      else {
        budget -= straddle;
        refs += straddle;
      }
    }
    if (spatial || o_axis >= 0) {
      std::vector<std::vector<Prim>> pL((size_t)TB), pR((size_t)TB);
      const int k = spatial ? s_axis : o_axis;
      const int T = parallel_chunks(n, [&](size_t b, size_t e, int t) {
        std::vector<Prim>& l = pL[t];
        std::vector<Prim>& rr = pR[t];
        for (size_t i = b; i < e; i++) {
          const Prim& p = r[i];
          if (!spatial) { (obin(p, k) <= o_bin ? l : rr).push_back(p); continue; }
          if (p.hi[k] <= s_pos) { l.push_back(p); continue; }
          if (p.lo[k] >= s_pos) { rr.push_back(p); continue; }
          Prim ql, qr;
          const bool hl = clip(p.id, k, p.lo[k], s_pos, p, ql), hr = clip(p.id, k, s_pos, p.hi[k], p, qr);
          if (hl && hr) { l.push_back(ql); rr.push_back(qr); }
          else if (hl) l.push_back(ql);
          else if (hr) rr.push_back(qr);
          else (p.c[k] < s_pos ? l : rr).push_back(p);
        }
      });
      for (int t = 0; t < T; t++) {
        L.insert(L.end(), pL[t].begin(), pL[t].end());
        R.insert(R.end(), pR[t].begin(), pR[t].end());
      }
    }
    if (L.empty() || R.empty()) {
      L.clear();
      R.clear();
      // degenerate centroids or forced: object median along the widest centroid axis
      if ((int)n <= kMaxLeaf && !(ext[0] > 0 || ext[1] > 0 || ext[2] > 0)) return leaf(r);
      const int k = (ext[0] >= ext[1] && ext[0] >= ext[2]) ? 0 : (ext[1] >= ext[2] ? 1 : 2);
      std::nth_element(r.begin(), r.begin() + n / 2, r.end(), [&](const Prim& x, const Prim& y) { return x.c[k] < y.c[k]; });
      L.assign(r.begin(), r.begin() + n / 2);
      R.assign(r.begin() + n / 2, r.end());
    }
    std::vector<Prim>().swap(r);
    const uint32_t me = next.fetch_add(1);
    const int64_t bl = (int64_t)((double)budget * (double)L.size() / (double)(L.size() + R.size())), br = budget - bl;
    Aabb lb, rb;
    uint32_t lh, rh;
    if (n > 4096 && depth < 16 && take_task(tasks, hw)) {
      auto fut = std::async(std::launch::async, [&]() { return build(L, depth + 1, lb, bl); });
      rh = build(R, depth + 1, rb, br);
      lh = fut.get();
      tasks.fetch_sub(1);
    } else {
      lh = build(L, depth + 1, lb, bl);
      rh = build(R, depth + 1, rb, br);
    }
    Node64 nd{};
    set_child(nd, 0, lb, pad, lh);
    set_child(nd, 1, rb, pad, rh);
    nodes[me] = nd;
    return me;
  }
};

// SBVH build (SbvhBuilder) from the face references; leaves get their triangle slots depth first (the
// order the DFS re-layout visits them), so the result does not depend on the build's thread timing
void build_sbvh(HostScene& hs, int leaf_size, std::vector<Prim>& prims, const Aabb& world, float alpha) {
  const char* budget_env = debug_env("RT_SBVH_BUDGET");
  const float budget = budget_env ? (float)atof(budget_env) : 0.5f;
  const int64_t cap = std::min<int64_t>((int64_t)hs.nf + (int64_t)(budget * hs.nf) + 1, (int64_t)kMaxFaces);
  std::vector<Node64> tmp((size_t)cap);
  SbvhBuilder B{hs, tmp};
  B.hw = std::max(1u, std::thread::hardware_concurrency());
  B.leaf_lists.resize((size_t)cap);
  B.refs = hs.nf;
  B.leaf_size = std::max(1, std::min(leaf_size, kMaxLeaf));
  if (const char* e = debug_env("RT_SAH_TRAV")) B.kTrav = std::max(0.05f, (float)atof(e));
  B.pad = bvh_pad(world.lo, world.hi);
  B.alpha = alpha;
  B.root_area = std::max(world.area(), 1e-30f);
  Aabb rootb;
  const auto tb0 = std::chrono::steady_clock::now();
  uint32_t root = B.build(prims, 0, rootb, cap - hs.nf);
  uint32_t nn = B.next.load();
  if (is_leaf(root)) {  // (the sentinel's slot 0 exists after the assignment below)
    tmp[0] = wrap_single_leaf_root(rootb, B.pad, root);
    nn = 1;
    root = 0;
  }
  tmp.resize(nn);
  // triangle slots in depth-first leaf order (child 0 first)
  std::vector<uint32_t> order;
  std::vector<uint32_t> st{root};
  while (!st.empty()) {
    Node64& nd = tmp[st.back()];
    st.pop_back();
    uint32_t* hc[2] = {&nd.child0, &nd.child1};
    for (int c = 0; c < 2; c++) {
      const uint32_t h = *hc[c];
      if (!is_leaf(h) || is_sentinel_child(nd, c)) continue;
      const std::vector<uint32_t>& ids = B.leaf_lists[leaf_first(h)];
      *hc[c] = make_leaf((uint32_t)order.size(), leaf_count(h));
      order.insert(order.end(), ids.begin(), ids.end());
    }
    if (!is_leaf(nd.child1)) st.push_back(nd.child1);
    if (!is_leaf(nd.child0)) st.push_back(nd.child0);
  }
  relayout_dfs(hs, tmp, root);
  hs.leaves = (int)B.nleaf.load();
  hs.tris.resize(order.size());
  const float Ro = cert_origin_max(hs);
  parallel_chunks(order.size(), [&](size_t sb, size_t se, int) {
    for (size_t i = sb; i < se; i++) tri_record(hs, order[i], hs.tris[i], Ro);
  });
  if (debug_env("RT_TIMING")) {
    size_t cert = 0;
    for (const TriRec64& t : hs.tris) cert += (t.box & kBoxCertBit) != 0;
    fprintf(stderr, "[rt] sbvh build %.1f ms: %zu references for %d faces, %u nodes, %zu references box-certified\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count(), order.size(),
            hs.nf, nn, cert);
  }
}

}  // namespace

void build_bvh(HostScene& hs, int leaf_size, bool spatial) {
  hs.nodes.clear();
  hs.tris.clear();
  hs.depth = 0;
  hs.leaves = 0;
  if (hs.nf == 0) { hs.root = 0; return; }
  std::vector<Prim> prims(hs.nf);
  Aabb wparts[16];
  const int TW = parallel_chunks((size_t)hs.nf, [&](size_t b, size_t e, int t) {
    Aabb wa;  // thread-local, stored once
    for (size_t f = b; f < e; f++) {
      Prim& p = prims[f];
      p.id = (uint32_t)f;
      for (int k = 0; k < 3; k++) { p.lo[k] = INFINITY; p.hi[k] = -INFINITY; }
      for (int j = 0; j < 3; j++) {
        const f3& w = bound_vert(hs, (uint32_t)f, j);
        const float c[3] = {w.x, w.y, w.z};
        for (int k = 0; k < 3; k++) { p.lo[k] = std::min(p.lo[k], c[k]); p.hi[k] = std::max(p.hi[k], c[k]); }
      }
      for (int k = 0; k < 3; k++) p.c[k] = 0.5f * (p.lo[k] + p.hi[k]);
      wa.grow(p.lo, p.hi);
    }
    wparts[t] = wa;
  });
  Aabb world;
  for (int t = 0; t < TW; t++) world.merge(wparts[t]);
  // spatial splits (RT_BUILDER_SBVH): alpha 1e-3 keeps the gain of 1e-5..1e-7 (the same node / triangle
  // counts within 0.2%) at less than half the build time (profiles/ab/r02_sbvh_sweep.txt)
  constexpr float kSbvhAlpha = 1e-3f;
  if (spatial && hs.nf > 1) { build_sbvh(hs, leaf_size, prims, world, kSbvhAlpha); return; }
  std::vector<Node64> tmp((size_t)std::max(hs.nf, 1));
  BvhBuilder B{prims, tmp};
  B.hw = std::max(1u, std::thread::hardware_concurrency());
  B.leaf_size = std::max(1, std::min(leaf_size, kMaxLeaf));
  if (const char* e = debug_env("RT_SAH_TRAV")) B.kTrav = std::max(0.05f, (float)atof(e));
  B.pad = bvh_pad(world.lo, world.hi);
  Aabb rootb;
  const bool timing = debug_env("RT_TIMING") != nullptr;
  auto tb0 = std::chrono::steady_clock::now();
  uint32_t root = B.build(0, (uint32_t)hs.nf, 0, rootb);
  if (timing) fprintf(stderr, "[rt] bvh recursive build %.1f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb0).count());
  uint32_t nn = B.next.load();
  if (is_leaf(root)) {  // whole scene in one leaf
    tmp[0] = wrap_single_leaf_root(rootb, B.pad, root);
    nn = 1;
    root = 0;
  }
  tmp.resize(nn);
  relayout_dfs(hs, tmp, root);
  hs.leaves = B.leaves.load();
  // triangle records in leaf order
  hs.tris.resize(hs.nf);
  const float Ro = cert_origin_max(hs);
  parallel_chunks((size_t)hs.nf, [&](size_t sb, size_t se, int) {
    for (size_t s = sb; s < se; s++) tri_record(hs, prims[s].id, hs.tris[s], Ro);
  });
}

}  // namespace rt
