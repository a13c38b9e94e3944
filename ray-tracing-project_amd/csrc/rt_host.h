// rt_host.h -- what the host scene-preparation sources share (rt_host.cpp, rt_refboxes.cpp, rt_builders.cpp,
// rt_layout.cpp, rt_validate.cpp): the box type, the one chunked parallel-for, the Node64 child-box writer and
// reader, the never-hit sentinel child, and the stages' entry points. Private to those files: no .hip file
// includes it (rt_scene.h carries what the device side and the scene cache need).
#pragma once
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "rt_scene.h"

namespace rt {

struct Aabb {
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  void grow(const float* l, const float* h) {
    for (int k = 0; k < 3; k++) { lo[k] = std::min(lo[k], l[k]); hi[k] = std::max(hi[k], h[k]); }
  }
  void growp(const float* p) { grow(p, p); }
  void merge(const Aabb& o) { grow(o.lo, o.hi); }
  float area() const {
    float d[3];
    for (int k = 0; k < 3; k++) d[k] = std::max(0.0f, hi[k] - lo[k]);
    return 2.0f * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
  }
};

// The chunking rule of every host loop: one chunk below 64k items, otherwise up to 16 (at most one per
// hardware thread). f(begin, end, chunk) runs over [b, e) cut at b + n * t / T; callers merge their per-chunk
// partial results in chunk order, so nothing depends on the thread count. Returns the number of chunks.
inline int chunk_count(size_t n) {
  return n >= 65536 ? (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency())) : 1;
}
template <typename F>
int parallel_chunks(size_t b, size_t e, F&& f) {
  const size_t n = e - b;
  const int T = chunk_count(n);
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back([&, t]() { f(b + n * t / T, b + n * (t + 1) / T, t); });
  f(b, b + n / T, 0);
  for (auto& x : th) x.join();
  return T;
}
template <typename F>
int parallel_chunks(size_t n, F&& f) { return parallel_chunks(0, n, f); }

// Child c of a binary node: its box padded outward by `pad` (conservative culling, bvh_pad) and its handle
inline void set_child(Node64& n, int c, const float lo[3], const float hi[3], float pad, uint32_t h) {
  if (c == 0) {
    n.c0lx = lo[0] - pad; n.c0hx = hi[0] + pad; n.c0ly = lo[1] - pad; n.c0hy = hi[1] + pad; n.c0lz = lo[2] - pad; n.c0hz = hi[2] + pad;
    n.child0 = h;
  } else {
    n.c1lx = lo[0] - pad; n.c1hx = hi[0] + pad; n.c1ly = lo[1] - pad; n.c1hy = hi[1] + pad; n.c1lz = lo[2] - pad; n.c1hz = hi[2] + pad;
    n.child1 = h;
  }
}
inline void set_child(Node64& n, int c, const Aabb& b, float pad, uint32_t h) { set_child(n, c, b.lo, b.hi, pad, h); }

struct ChildBox {
  float lo[3], hi[3];
  uint32_t h;
};
inline ChildBox child_box(const Node64& n, int c) {
  if (c == 0) return {{n.c0lx, n.c0ly, n.c0lz}, {n.c0hx, n.c0hy, n.c0hz}, n.child0};
  return {{n.c1lx, n.c1ly, n.c1lz}, {n.c1hx, n.c1hy, n.c1hz}, n.child1};
}

// A scene whose root is one leaf is wrapped in a node whose second child never hits: an inverted box over
// a leaf handle of triangle slot 0 (which exists). Walks that count or collect leaves skip it.
inline bool is_sentinel_child(const Node64& n, int c) { return (c ? n.c1lx : n.c0lx) > (c ? n.c1hx : n.c0hx); }
inline Node64 wrap_single_leaf_root(const Aabb& box, float pad, uint32_t leaf) {
  Node64 nd{};
  set_child(nd, 0, box, pad, leaf);
  nd.c1lx = nd.c1ly = nd.c1lz = INFINITY;
  nd.c1hx = nd.c1hy = nd.c1hz = -INFINITY;
  nd.child1 = make_leaf(0, 1);
  return nd;
}

// rt_refboxes.cpp
void build_ref_boxes(HostScene& hs, const float* v4, int32_t min_faces, int32_t max_boxes);
void assign_box_ranks(HostScene& hs);  // face_rank / face_box from hs.boxes (creation order, in-box face order)
// rt_host.cpp: the partition by the scene's box_builder (device `dev`, -1: host), ranks assigned
int partition_ref_boxes(rt_scene* s, int dev, const float* v4);
// rt_builders.cpp
void build_bvh(HostScene& hs, int leaf_size, bool spatial);  // spatial: SBVH (RT_BUILDER_SBVH)
// rt_layout.cpp
float bvh_pad(const float lo[3], const float hi[3]);
bool model_is_similarity(const float* M);
void tri_record(const HostScene& hs, uint32_t f, TriRec64& r, float Ro);  // exact-test record of face f
void relayout_dfs(HostScene& hs, const std::vector<Node64>& tmp, uint32_t root);
bool build_bvh_gpu(HostScene& hs, int device, int leaf_size, double* gpu_ms);
bool build_bvh_ploc(HostScene& hs, int device, int leaf_size, double* gpu_ms);
bool build_bvh_sah_gpu(HostScene& hs, int device, int leaf_size, bool spatial, double* gpu_ms);
void build_bvh4(HostScene& hs);

}  // namespace rt
