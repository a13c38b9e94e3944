// Host-side AddressSanitizer / UBSan harness (CPU only; tools/asan/run.sh builds it): drives the host
// entry points of the C ABI -- OBJ ingest (valid and malformed files), host-only scene creation with
// both box builders' host path, the BVH validator, the binary scene cache (save, load, and every
// truncation / byte flip of a small file), PPM writers, lights and camera helpers, light sets and the host-only
// parts of the view batches (their plan hook, both entry points without a device) -- so that heap
// errors in the host code surface as sanitizer reports instead of later crashes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt/rt_api.h"

static int g_fail = 0;
#define EXPECT(c)                                                          \
  do {                                                                     \
    if (!(c)) { std::fprintf(stderr, "FAIL %s:%d %s\n", __FILE__, __LINE__, #c); g_fail++; } \
  } while (0)

// A directory of this run's own under $TMPDIR (mkdtemp), removed with its files at the end of main: fixed
// names in the shared directory collide with another user's (or an earlier run's) files there.
static std::string g_tmp;
static const char* const kTmpFiles[] = {"rt_asan_bad.obj", "rt_asan.rtscene", "rt_asan_bad.rtscene", "rt_asan.ppm",
                                        "rt_asan8.ppm"};

static std::string tmpdir() {
  if (g_tmp.empty()) {
    const char* t = std::getenv("TMPDIR");
    std::string tmpl = std::string(t && *t ? t : "/tmp") + "/rt_asan_XXXXXX";
    if (!mkdtemp(&tmpl[0])) { std::perror(("mkdtemp " + tmpl).c_str()); std::exit(2); }
    g_tmp = tmpl;
  }
  return g_tmp;
}

static void remove_tmpdir() {
  if (g_tmp.empty()) return;
  for (const char* n : kTmpFiles) std::remove((g_tmp + "/" + n).c_str());
  if (std::remove(g_tmp.c_str()) != 0) { std::perror(("remove " + g_tmp).c_str()); g_fail++; }
}

static void write_file(const std::string& p, const std::string& s) {
  FILE* f = std::fopen(p.c_str(), "wb");
  if (!f) { std::perror(("fopen " + p).c_str()); std::exit(2); }
  std::fwrite(s.data(), 1, s.size(), f);
  std::fclose(f);
}

static std::string read_file(const std::string& p) {
  std::string s;
  FILE* f = std::fopen(p.c_str(), "rb");
  if (!f) return s;
  std::fseek(f, 0, SEEK_END);
  s.resize((size_t)std::ftell(f));
  std::fseek(f, 0, SEEK_SET);
  if (!s.empty() && std::fread(&s[0], 1, s.size(), f) != s.size()) s.clear();
  std::fclose(f);
  return s;
}

static void malformed_objs() {
  const std::string p = tmpdir() + "/rt_asan_bad.obj";
  const char* cases[] = {
      "v 0 0 0\nv 1 0 0\nf 1 2\n",                  // not a multiple of 3
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 9\n",       // index past the end (computeNormals path)
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n",       // index 0 -> -1
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 2 3\n",      // negative
      "f 1 2 3\n",                                  // faces without vertices
      "v 0 0 0\nv 1 0 0\nv 0 1 0\nvn 0 0 1\nf 1 2 3\n",  // #vn != #v
      "mtllib\n",                                   // malformed mtllib
      "usemtl\n",                                   // malformed usemtl
      "v 1e40 -1e40 nan\nv 1 0 0\nv 0 1 0\nf 1 2 3\n",
      "v\nvn\nf\n",
      "",
  };
  for (const char* c : cases) {
    write_file(p, c);
    rt_mesh* m = nullptr;
    int rc = rt_mesh_load_obj(p.c_str(), &m);
    if (rc == RT_OK) {
      rt_mesh_desc d;
      EXPECT(rt_mesh_get_desc(m, &d) == RT_OK);
      rt_mesh_destroy(m);
    } else {
      EXPECT(m == nullptr);
    }
  }
  rt_mesh* m = nullptr;
  EXPECT(rt_mesh_load_obj((tmpdir() + "/rt_asan_missing.obj").c_str(), &m) != RT_OK);
}

static void from_arrays() {
  const float v[9] = {0, 0, 0, 1, 0, 0, 0, 1, 0};
  const uint32_t bad[3] = {0, 1, 7};
  const int32_t gc[1] = {3}, gm[1] = {-1};
  rt_mesh* m = nullptr;
  EXPECT(rt_mesh_from_arrays(3, v, nullptr, 1, gc, bad, gm, 0, nullptr, &m) != RT_OK);
  const uint32_t good[3] = {0, 1, 2};
  EXPECT(rt_mesh_from_arrays(3, v, nullptr, 1, gc, good, gm, 0, nullptr, &m) == RT_OK);
  rt_mesh_destroy(m);
  const int32_t gneg[1] = {-3};
  EXPECT(rt_mesh_from_arrays(3, v, nullptr, 1, gneg, good, gm, 0, nullptr, &m) != RT_OK);
}

// light sets on a host-only scene: create, get and destroy, the invalid arguments, and one set left to the scene
static void light_sets(rt_scene* s) {
  std::vector<rt_light> in(7);
  const int kinds[7] = {1, 0, 1, 0, 0, 1, 0};
  for (int i = 0; i < 7; i++) {
    std::memset(&in[i], 0, sizeof in[i]);
    in[i].position[0] = (float)i;
    in[i].kind = kinds[i];
  }
  rt_light_set* ls = nullptr;
  EXPECT(rt_light_set_create(s, in.data(), 7, &ls) == RT_OK && ls);
  std::vector<rt_light> out(7);
  int32_t n = -1;
  EXPECT(rt_light_set_get(ls, 7, out.data(), &n) == RT_OK && n == 7);
  const float want[7] = {1, 3, 4, 6, 0, 2, 5};  // points in array order, then directionals
  for (int i = 0; i < 7; i++) EXPECT(out[i].position[0] == want[i] && out[i].kind == (i >= 4));
  EXPECT(rt_light_set_get(ls, 6, out.data(), &n) == RT_ERR_INVALID);
  EXPECT(rt_light_set_get(ls, 0, nullptr, &n) == RT_OK && n == 7);
  EXPECT(rt_light_set_get(nullptr, 7, out.data(), &n) == RT_ERR_INVALID);
  rt_light_set_destroy(ls);
  rt_light_set_destroy(nullptr);
  rt_light_set* bad = nullptr;
  EXPECT(rt_light_set_create(s, in.data(), -1, &bad) == RT_ERR_INVALID && !bad);
  EXPECT(rt_light_set_create(s, in.data(), RT_MAX_LIGHT_SET + 1, &bad) == RT_ERR_INVALID && !bad);
  EXPECT(rt_light_set_create(s, nullptr, 3, &bad) == RT_ERR_INVALID && !bad);
  EXPECT(rt_light_set_create(nullptr, in.data(), 7, &bad) == RT_ERR_INVALID && !bad);
  EXPECT(rt_light_set_create(s, in.data(), 7, nullptr) == RT_ERR_INVALID);
  rt_light_set* empty = nullptr;
  EXPECT(rt_light_set_create(s, nullptr, 0, &empty) == RT_OK && empty);
  EXPECT(rt_light_set_get(empty, 0, out.data(), &n) == RT_OK && n == 0);
  rt_light_set_destroy(empty);
  std::vector<rt_light> big(RT_MAX_LIGHT_SET, in[1]);
  rt_light_set* full = nullptr;
  EXPECT(rt_light_set_create(s, big.data(), RT_MAX_LIGHT_SET, &full) == RT_OK && full);
  rt_camera cam;
  rt_camera_flycam(64, 48, 0.0f, 0.0f, 0.0f, &cam);
  const rt_frame fr{64, 48, RT_MODE_FULL, 0, 1, 0, 0};
  EXPECT(rt_render_lit(s, &cam, full, &fr, nullptr, nullptr) == RT_ERR_NO_DEVICE);
  // `full` stays alive: rt_scene_destroy frees it
}

// view batches, the host-only parts: the plan hook over valid, refused and malformed inputs, and both entry points
// on a host-only scene and on NULL arguments (nothing may be read or written before the device check)
static void view_batches(rt_scene* s) {
  int64_t out[7];
  const int64_t ok[9] = {RT_MODE_FULL, 0, 0, 0, 3, 2, 4, 0, 0};
  EXPECT(rt_debug_view_plan(ok, 9, out, 7) == RT_OK && out[0] == 2 && out[2] == 24 && out[3] == 96 && out[5] == 0);
  const int64_t box[9] = {RT_MODE_BOX_COLORS, 0, 0, 0, 3, 2, 4, 0, 0};
  EXPECT(rt_debug_view_plan(box, 9, out, 7) == RT_OK && out[0] == 0 && out[5] == 1 && out[6] == RT_ERR_UNSUPPORTED);
  const int64_t huge[9] = {RT_MODE_PRIMARY, 0, 0, 0, (int64_t)1 << 27, (int64_t)1 << 27, RT_MAX_VIEWS, 0, 0};
  EXPECT(rt_debug_view_plan(huge, 9, out, 7) == RT_OK && out[5] == 1 && out[6] == RT_ERR_INVALID);
  const int64_t wild[9] = {INT64_MAX, INT64_MIN, -1, -1, -1, -1, INT64_MAX, -1, INT64_MIN};
  EXPECT(rt_debug_view_plan(wild, 9, out, 7) == RT_ERR_INVALID);
  for (int64_t mode = -2; mode < 5; mode++)
    for (int64_t n : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)RT_MAX_VIEWS, (int64_t)RT_MAX_VIEWS + 1}) {
      const int64_t in[9] = {mode, 17, 31, 3, 0, 1 << 27, n, -1, RT_MAX_LIGHT_SET};
      (void)rt_debug_view_plan(in, 9, out, 7);
    }
  EXPECT(rt_debug_view_plan(ok, 8, out, 7) == RT_ERR_INVALID && rt_debug_view_plan(ok, 9, out, 6) == RT_ERR_INVALID);
  EXPECT(rt_debug_view_plan(nullptr, 9, out, 7) == RT_ERR_INVALID && rt_debug_view_plan(ok, 9, nullptr, 7) == RT_ERR_INVALID);

  rt_camera cams[2];
  rt_camera_flycam(16, 16, 0.0f, 0.0f, 0.0f, &cams[0]);
  rt_camera_flycam(16, 16, 1.0f, 0.0f, 0.0f, &cams[1]);
  std::vector<float> rgb(2 * 16 * 16 * 3, 7.0f);
  const rt_view_batch vb{2, cams, rgb.data(), nullptr, nullptr};
  const rt_frame fr{16, 16, RT_MODE_PRIMARY, 0, 1, 0, 0};
  rt_light l;
  std::memset(&l, 0, sizeof l);
  rt_light_set* ls = nullptr;
  EXPECT(rt_light_set_create(s, &l, 1, &ls) == RT_OK && ls);
  EXPECT(rt_render_views(s, &vb, &l, 1, &fr, nullptr) == RT_ERR_NO_DEVICE);
  EXPECT(rt_render_views_lit(s, &vb, ls, &fr, nullptr) == RT_ERR_NO_DEVICE);
  EXPECT(rt_render_views(s, nullptr, nullptr, 99, nullptr, nullptr) == RT_ERR_NO_DEVICE);
  EXPECT(rt_render_views_lit(s, nullptr, nullptr, nullptr, nullptr) == RT_ERR_NO_DEVICE);
  EXPECT(rt_render_views(nullptr, &vb, &l, 1, &fr, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_render_views_lit(nullptr, &vb, ls, &fr, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_render_views(nullptr, nullptr, nullptr, 0, nullptr, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_render_views_lit(nullptr, nullptr, nullptr, nullptr, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_last_error()[0] != 0);
  for (float v : rgb) EXPECT(v == 7.0f);
  rt_light_set_destroy(ls);
}

// rt_scene_update on the host-only scene: vertices moved twice and put back, the record images, and the refusals
// (another face count, null arguments). Finite coordinates only: the reference's box partition, which create and
// update both run, does not terminate for every placement of a NaN (tests/test_scene_update_host.py has a NaN step).
static void scene_update(rt_scene* s, const rt_mesh_desc& d) {
  std::vector<float> v(d.vertices, d.vertices + 4 * (size_t)d.n_vertices);
  rt_mesh_desc moved = d;
  moved.vertices = v.data();
  rt_update_stats st;
  int64_t info[7], n = 0;
  for (int pass = 0; pass < 2; pass++) {
    for (size_t i = 0; i < v.size(); i += 4) v[i] += 0.01f * (float)((i / 4) % 7);
    EXPECT(rt_scene_update(s, &moved, &st) == RT_OK && st.bounds_on_device == 0);
    EXPECT(rt_debug_validate_bvh(s, info) == RT_OK);
    for (int which = 0; which < 3; which++) {
      EXPECT(rt_debug_scene_records(s, which, 0, nullptr, &n) == RT_OK);
      std::vector<uint8_t> img((size_t)n + 1, 0xAB);
      EXPECT(rt_debug_scene_records(s, which, n, img.data(), &n) == RT_OK && img[(size_t)n] == 0xAB);
      EXPECT(n == 0 || rt_debug_scene_records(s, which, n - 1, img.data(), &n) == RT_ERR_INVALID);
    }
  }
  EXPECT(rt_scene_update(s, &d, nullptr) == RT_OK);
  rt_mesh_desc fewer = d;
  fewer.n_faces = d.n_faces - 1;
  EXPECT(rt_scene_update(s, &fewer, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_scene_update(s, nullptr, nullptr) == RT_ERR_INVALID && rt_scene_update(nullptr, &d, nullptr) == RT_ERR_INVALID);
  EXPECT(rt_debug_scene_records(s, 3, 0, nullptr, &n) == RT_ERR_INVALID);
}

static void scene_roundtrip(const std::string& obj, int box_builder) {
  rt_mesh* m = nullptr;
  if (rt_mesh_load_obj(obj.c_str(), &m) != RT_OK) { std::fprintf(stderr, "skip %s\n", obj.c_str()); return; }
  rt_mesh_desc d;
  EXPECT(rt_mesh_get_desc(m, &d) == RT_OK);
  rt_scene_opts o;
  rt_scene_opts_default(&o);
  o.device = RT_DEVICE_NONE;
  o.box_builder = box_builder;
  rt_scene* s = nullptr;
  EXPECT(rt_scene_create(&d, &o, &s) == RT_OK);
  if (!s) { rt_mesh_destroy(m); return; }
  int64_t info[7];
  EXPECT(rt_debug_validate_bvh(s, info) == RT_OK);
  rt_scene_info si;
  EXPECT(rt_scene_get_info(s, &si) == RT_OK);
  std::vector<float> b6(6 * (size_t)si.n_ref_boxes);
  std::vector<int32_t> cnt(si.n_ref_boxes), order(si.n_faces);
  EXPECT(rt_scene_ref_boxes(s, b6.data(), cnt.data(), order.data()) == RT_OK);
  const std::string p = tmpdir() + "/rt_asan.rtscene", q = tmpdir() + "/rt_asan_bad.rtscene";
  EXPECT(rt_scene_save(s, p.c_str()) == RT_OK);
  rt_scene* l = nullptr;
  EXPECT(rt_scene_load(p.c_str(), &o, &l) == RT_OK);
  if (l) rt_scene_destroy(l);
  // damaged copies: every truncation length on a coarse grid and single-bit flips across the file
  const std::string raw = read_file(p);
  const size_t step = raw.size() / 97 + 1;
  for (size_t n = 0; n < raw.size(); n += step) {
    write_file(q, raw.substr(0, n));
    l = nullptr;
    if (rt_scene_load(q.c_str(), &o, &l) == RT_OK) rt_scene_destroy(l);
  }
  for (size_t i = 0; i < raw.size(); i += step) {
    std::string c = raw;
    c[i] ^= 0x10;
    write_file(q, c);
    l = nullptr;
    if (rt_scene_load(q.c_str(), &o, &l) == RT_OK) rt_scene_destroy(l);
  }
  light_sets(s);
  view_batches(s);
  scene_update(s, d);
  rt_scene_destroy(s);  // frees the set light_sets() left alive
  rt_mesh_destroy(m);
}

static void misc() {
  const int W = 7, H = 5;
  std::vector<float> rgb(3 * W * H, 0.5f);
  std::vector<uint8_t> rgb8(3 * W * H, 200);
  EXPECT(rt_write_ppm((tmpdir() + "/rt_asan.ppm").c_str(), rgb.data(), W, H) == RT_OK);
  EXPECT(rt_write_ppm_rgb8((tmpdir() + "/rt_asan8.ppm").c_str(), rgb8.data(), W, H) == RT_OK);
  rt_rand_state st;
  rt_rand_seed(&st, 1);
  for (int i = 0; i < 1000; i++) (void)rt_rand(&st);
  rt_camera cam;
  rt_camera_flycam(64, 48, 0.0f, 0.0f, 20.0f, &cam);
  rt_light c;
  std::memset(&c, 0, sizeof c);
  c.position[0] = 1.0f; c.color[0] = c.color[1] = c.color[2] = 1.0f;
  std::vector<rt_light> out(9);
  (void)rt_lights_spherical(&c, 0.5f, 8, &st, out.data());
  const float col[3] = {1, 1, 1};
  rt_light_directional(&cam, col, &out[0]);
  std::vector<float> soup(9 * 1000);
  rt_generate_soup(1000, 12345, soup.data());
}

int main(int argc, char** argv) {
  const std::string scenes = argc > 1 ? argv[1] : "scenes";
  malformed_objs();
  from_arrays();
  for (const char* n : {"cube.obj", "testding.obj", "dodgeColorTest.obj"})
    for (int bb : {RT_BOXES_HOST}) scene_roundtrip(scenes + "/" + n, bb);
  misc();
  remove_tmpdir();
  std::printf("host_asan: %s (%d failed expectations)\n", g_fail ? "FAILED" : "ok", g_fail);
  return g_fail ? 1 : 0;
}
