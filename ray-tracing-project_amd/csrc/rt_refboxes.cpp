// rt_refboxes.cpp -- the reference's flat box partition on the host, which defines closest-hit tie-breaking
// (the face ranks) and the per-face box predicate; rt_boxes.hip builds the same boxes on the device.
//
// Reference semantics restated here (file:line in plindhorst/Ray-Tracing-Project):
//   flat box partition  src/BoundingBox.cpp:41-161, src/flyscene.cpp:399-428
#include <atomic>
#include <cstring>

#include "rt_host.h"

namespace rt {
namespace {
// The partition is a sequence of passes; within a pass every box that still qualifies is split (with
// axis retries) independently of the others, and the boxes it creates are appended in box order. So a
// pass runs its boxes in parallel and appends the results in order: the same boxes, face lists and
// order as the sequential reference loop. Vertex coordinates are copied per face (9 floats, face
// order) so the passes stream instead of gathering from the shared vertex array.
struct BoxBuilder {
  const float* fv;  // [nf][3 vertices][3] object-space coordinates (v / w is not taken: Tucano uses x,y,z)
  const float* V(int32_t face, int k) const { return fv + 9 * (size_t)face + 3 * k; }

  static void reshape(RefBox& b) { for (int k = 0; k < 3; k++) b.shape[k] = b.high[k] - b.low[k]; }

  bool has_face(const RefBox& b, int32_t face) const {  // hasFace / hasVertex (inclusive)
    for (int k = 0; k < 3; k++) {
      const float* v = V(face, k);
      if (!(v[0] >= b.low[0] && v[0] <= b.high[0] && v[1] >= b.low[1] && v[1] <= b.high[1] &&
            v[2] >= b.low[2] && v[2] <= b.high[2]))
        return false;
    }
    return true;
  }
  void fit(RefBox& b) const {  // fitFaces: first-vertex init, if/else-if min/max
    if (b.faces.empty()) return;
    const float* t = V(b.faces[0], 0);
    float mn[3] = {t[0], t[1], t[2]}, mx[3] = {t[0], t[1], t[2]};
    for (int32_t face : b.faces)
      for (int j = 0; j < 3; j++) {
        const float* v = V(face, j);
        for (int a = 0; a < 3; a++) {
          if (v[a] < mn[a]) mn[a] = v[a];
          else if (v[a] > mx[a]) mx[a] = v[a];
        }
      }
    for (int a = 0; a < 3; a++) { b.low[a] = mn[a]; b.high[a] = mx[a]; }
    reshape(b);
  }
  float average(const RefBox& b, int axis) const {  // averageVertexCoord: sequential float sum
    float avg = 0.0f;
    for (int32_t face : b.faces) {
      avg += V(face, 0)[axis];
      avg += V(face, 1)[axis];
      avg += V(face, 2)[axis];
    }
    avg /= (float)(b.faces.size() * 3);
    return avg;
  }
  // splitBox: 1 = split, `out` receives the new box; 0 = axis failed (returned `this`); -1 = nullptr
  int split(RefBox& b, RefBox& out) const {
    float oldLow[3], oldHigh[3];
    memcpy(oldLow, b.low, 12);
    memcpy(oldHigh, b.high, 12);
    const float w = b.shape[0], h = b.shape[1], d = b.shape[2];
    int choice;
    if ((w >= h || b.failed[1]) && (w >= d || b.failed[2]) && !b.failed[0]) choice = 0;
    else if ((h >= w || b.failed[0]) && (h >= d || b.failed[2]) && !b.failed[1]) choice = 1;
    else if (!(b.failed[0] && b.failed[1] && b.failed[2])) choice = 2;
    else return -1;
    b.high[choice] = average(b, choice);
    reshape(b);
    std::vector<int32_t> inside, outside;  // outsideFaces: stable partition
    inside.reserve(b.faces.size());
    for (int32_t face : b.faces) (has_face(b, face) ? inside : outside).push_back(face);
    if (inside.empty() || outside.empty()) {
      b.faces = inside.empty() ? std::move(outside) : std::move(inside);
      b.failed[choice] = true;
      memcpy(b.low, oldLow, 12);
      memcpy(b.high, oldHigh, 12);
      reshape(b);
      return 0;
    }
    b.faces = std::move(inside);
    b.failed[0] = b.failed[1] = b.failed[2] = false;
    out = RefBox();
    out.faces = std::move(outside);
    fit(out);
    fit(b);
    return 1;
  }
};
}  // namespace

void build_ref_boxes(HostScene& hs, const float* v4, int32_t min_faces, int32_t max_boxes) {
  hs.boxes.clear();
  std::vector<float> fv(9 * (size_t)hs.nf);
  for (int32_t f = 0; f < hs.nf; f++)
    for (int k = 0; k < 3; k++) memcpy(&fv[9 * (size_t)f + 3 * k], v4 + 4 * (size_t)hs.fidx[3 * (size_t)f + k], 12);
  BoxBuilder bb{fv.data()};
  RefBox b0;
  b0.faces.resize(hs.nf);
  for (int32_t i = 0; i < hs.nf; i++) b0.faces[i] = i;
  hs.boxes.push_back(std::move(b0));
  bb.fit(hs.boxes[0]);
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  bool notDone = true;
  while (notDone && (int64_t)hs.boxes.size() < (int64_t)max_boxes) {
    notDone = false;
    const size_t ncur = hs.boxes.size();
    std::vector<size_t> todo;
    for (size_t bi = 0; bi < ncur; bi++) {
      const RefBox& b = hs.boxes[bi];
      if ((int64_t)b.faces.size() > min_faces && (!b.failed[0] || !b.failed[1] || !b.failed[2])) todo.push_back(bi);
    }
    if (todo.empty()) break;
    notDone = true;
    std::vector<RefBox> created(todo.size());
    std::vector<char> made(todo.size(), 0);
    auto work = [&](size_t i) {
      RefBox& b = hs.boxes[todo[i]];
      int r = bb.split(b, created[i]);
      while (r == 0) r = bb.split(b, created[i]);
      made[i] = r == 1;
    };
    // larger boxes first across the workers (the first passes hold few, huge boxes)
    std::atomic<size_t> cursor{0};
    std::vector<size_t> order(todo.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) {
      return hs.boxes[todo[a]].faces.size() > hs.boxes[todo[b]].faces.size();
    });
    const unsigned nth = (unsigned)std::min<size_t>(hw, todo.size());
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nth; t++)
      th.emplace_back([&]() { for (size_t k; (k = cursor.fetch_add(1)) < order.size();) work(order[k]); });
    for (size_t k; (k = cursor.fetch_add(1)) < order.size();) work(order[k]);
    for (auto& t : th) t.join();
    // the reference appends each new box right after splitting, i.e. in box order within the pass
    for (size_t i = 0; i < todo.size(); i++)
      if (made[i]) hs.boxes.push_back(std::move(created[i]));
  }
  assign_box_ranks(hs);
}

void assign_box_ranks(HostScene& hs) {
  hs.face_rank.assign(hs.nf, 0);
  hs.face_box.assign(hs.nf, 0);
  uint32_t rank = 0;
  for (size_t bi = 0; bi < hs.boxes.size(); bi++)
    for (int32_t face : hs.boxes[bi].faces) {
      hs.face_rank[face] = rank++;
      hs.face_box[face] = (uint32_t)bi;
    }
}

}  // namespace rt
