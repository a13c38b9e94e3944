// rt_view.cpp -- what a caller needs around a frame: the PPM writers, glibc's rand(), the lights, the camera
// helpers and the debug ray.
//
// Reference semantics restated here (file:line in plindhorst/Ray-Tracing-Project):
//   camera              tucano/camera.hpp:115-118,155-173,263-266; tucano/utils/flycamera.hpp:76-202
//   PPM writer          tucano/utils/ppmIO.hpp:135-156
//   lights, debug ray   src/flyscene.cpp:129-173
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "rt_scene.h"

using rt::f3;

// (int)(255*c) with x86 cvttss2si semantics for out-of-range / NaN (0x80000000)
static inline int to_int_x86(float x) {
  if (!(x >= -2147483648.0f && x < 2147483648.0f)) return INT_MIN;
  return (int)x;
}

extern "C" int rt_write_ppm(const char* path, const float* rgb, int32_t W, int32_t H) {
  if (!path || !rgb || W <= 0 || H <= 0) { rt::set_error("rt_write_ppm: invalid arguments"); return RT_ERR_INVALID; }
  FILE* f = fopen(path, "wb");
  if (!f) { rt::set_error("cannot write %s", path); return RT_ERR_IO; }
  std::string out;
  out.reserve((size_t)W * H * 12 + 64);
  out += "P3\n" + std::to_string(W) + " " + std::to_string(H) + "\n255\n";
  char tmp[64];
  for (int32_t j = 0; j < H; j++) {
    for (int32_t i = 0; i < W; i++) {
      const float* c = rgb + 3 * ((size_t)j * W + i);
      int n = snprintf(tmp, sizeof tmp, "%d %d %d ", std::min(255, to_int_x86(255 * c[0])),
                       std::min(255, to_int_x86(255 * c[1])), std::min(255, to_int_x86(255 * c[2])));
      out.append(tmp, (size_t)n);
    }
    out += "\n";
  }
  size_t wr = fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  if (wr != out.size()) { rt::set_error("short write %s", path); return RT_ERR_IO; }
  return RT_OK;
}

// writePPMImage's text for 8-bit values (same bytes as rt_write_ppm when every value is in 0..255),
// without per-number formatting calls: a table of the 256 "%d " strings
extern "C" int rt_write_ppm_rgb8(const char* path, const uint8_t* rgb8, int32_t W, int32_t H) {
  if (!path || !rgb8 || W <= 0 || H <= 0) { rt::set_error("rt_write_ppm_rgb8: invalid arguments"); return RT_ERR_INVALID; }
  struct Tab {
    char s[256][5];  // "255 " plus the terminator
    uint8_t len[256];
    Tab() {
      for (int v = 0; v < 256; v++) len[v] = (uint8_t)snprintf(s[v], sizeof s[v], "%d ", v);
    }
  };
  static const Tab t;  // thread-safe one-time initialisation
  const auto& tab = t.s;
  const auto& len = t.len;
  std::string out;
  out.reserve((size_t)W * H * 12 + 64);
  out += "P3\n" + std::to_string(W) + " " + std::to_string(H) + "\n255\n";
  for (int32_t j = 0; j < H; j++) {
    const uint8_t* row = rgb8 + (size_t)j * W * 3;
    for (int32_t i = 0; i < 3 * W; i++) out.append(tab[row[i]], len[row[i]]);
    out += "\n";
  }
  FILE* f = fopen(path, "wb");
  if (!f) { rt::set_error("cannot write %s", path); return RT_ERR_IO; }
  const size_t wr = fwrite(out.data(), 1, out.size(), f);
  fclose(f);
  if (wr != out.size()) { rt::set_error("short write %s", path); return RT_ERR_IO; }
  return RT_OK;
}

// ---------------------------------------------------------------------------------------------------
// Lights
// ---------------------------------------------------------------------------------------------------
// glibc rand(): TYPE_3 additive feedback generator, r[i] = r[i-31] + r[i-3] (mod 2^32) after a
// Park-Miller seeding of r[0..30], r[31..33] = r[0..2] and 310 discarded outputs; rand() = r[i] >> 1.
// The state is the ring of the last 34 values.
extern "C" void rt_rand_seed(rt_rand_state* st, uint32_t seed) {
  if (!st) return;
  uint32_t r[344];
  r[0] = seed ? seed : 1u;
  for (int i = 1; i < 31; i++) {
    const int64_t w = (16807LL * (int64_t)(int32_t)r[i - 1]) % 2147483647LL;
    r[i] = (uint32_t)(w < 0 ? w + 2147483647LL : w);
  }
  for (int i = 31; i < 34; i++) r[i] = r[i - 31];
  for (int i = 34; i < 344; i++) r[i] = r[i - 31] + r[i - 3];
  for (int i = 310; i < 344; i++) st->r[i % 34] = r[i];
  st->k = 344 % 34;
}

extern "C" int32_t rt_rand(rt_rand_state* st) {
  const uint32_t k = st->k;  // slot of r[i - 34]; r[i - 31] is k + 3, r[i - 3] is k + 31 (mod 34)
  const uint32_t v = st->r[(k + 3) % 34] + st->r[(k + 31) % 34];
  st->r[k] = v;
  st->k = (k + 1) % 34;
  return (int32_t)(v >> 1);
}

extern "C" int32_t rt_lights_spherical(const rt_light* centre, float radius, int32_t n_points, rt_rand_state* rng,
                                       rt_light* out) {
  if (!centre || !out || n_points < 0) { rt::set_error("rt_lights_spherical: invalid arguments"); return RT_ERR_INVALID; }
  rt_rand_state local;
  if (!rng) { rt_rand_seed(&local, 1); rng = &local; }
  const float div = (float)(n_points + 1);
  float col[3];
  for (int k = 0; k < 3; k++) col[k] = centre->color[k] / div;  // light.second / (nLightpoints + 1)
  for (int32_t i = 0; i < n_points; i++) {
    float off[3];
    for (int k = 0; k < 3; k++) {  // -radius + (rand() / (RAND_MAX / (radius * 2))), x then y then z
      const float q = (float)2147483647 / (radius * 2);
      off[k] = -radius + ((float)rt_rand(rng) / q);
    }
    for (int k = 0; k < 3; k++) {
      out[i].position[k] = centre->position[k] + off[k];
      out[i].color[k] = col[k];
    }
    out[i].kind = RT_LIGHT_POINT;
  }
  for (int k = 0; k < 3; k++) {
    out[n_points].position[k] = centre->position[k];
    out[n_points].color[k] = col[k];  // light.second /= (Nlights + 1)
  }
  out[n_points].kind = RT_LIGHT_POINT;
  return n_points + 1;
}

// Camera::screenToWorld (camera.hpp:155-173) of a (float) screen position
static f3 screen_to_world(const rt_camera* c, float px, float py) {
  f3 nc;
  nc.x = (float)(2.0 * (double)(px - c->viewport[0]) / (double)c->viewport[2] - 1.0);
  nc.y = (float)(1.0 - 2.0 * (double)(py - c->viewport[1]) / (double)c->viewport[3]);
  nc.z = -1.0f;
  const float persp = (float)((double)1.0f / tan((double)(c->fovy / 2.0f) * (M_PI / 180.0)));
  const float scale = (float)(1.0 / (double)persp);
  nc.x = nc.x * (c->aspect_ratio * scale);
  nc.y = nc.y * scale;
  float vinv[16];
  rt::affinv(c->view_matrix, vinv);
  return rt::affv3(vinv, nc);
}

// Camera::getCenter (camera.hpp:115-118): view.linear().inverse() * (-view.translation())
static f3 camera_center(const rt_camera* c) {
  float L[9], Li[9];
  rt::linear_of(c->view_matrix, L);
  rt::m3inv(L, Li);
  return rt::m3v3(Li, f3{-c->view_matrix[12], -c->view_matrix[13], -c->view_matrix[14]});
}

extern "C" void rt_light_directional(const rt_camera* c, const float color[3], rt_light* out) {
  // screenToWorld(Vector2f(viewport(2) / 2, viewport(3) / 2)): the point itself is stored
  const f3 w = screen_to_world(c, c->viewport[2] / 2, c->viewport[3] / 2);
  out->position[0] = w.x; out->position[1] = w.y; out->position[2] = w.z;
  for (int k = 0; k < 3; k++) out->color[k] = color[k];
  out->kind = RT_LIGHT_DIRECTIONAL;
}

// createDebugRay (flyscene.cpp:129-173) without the GL cylinders: the camera ray through the mouse
// position, its traceRay colour, and the chain of reflections. As the reference, every segment gets the
// first ray's colour, each reflection reflects the *first* direction about the new hit's interpolated
// normal, and a miss ends the chain with a 10-unit segment. All ray queries run on the device.
extern "C" int rt_debug_ray(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, float mouse_x,
                            float mouse_y, int32_t max_depth, rt_ray_segment* out, int32_t* n_out) {
  if (!s || !cam || !out || !n_out || max_depth < 1) { rt::set_error("rt_debug_ray: invalid arguments"); return RT_ERR_INVALID; }
  *n_out = 0;
  const f3 origin = camera_center(cam);
  const f3 dir = rt::normalized(rt::sub(screen_to_world(cam, mouse_x, mouse_y), origin));
  float o[3] = {origin.x, origin.y, origin.z}, d[3] = {dir.x, dir.y, dir.z}, rgb[3];
  int rc = rt_trace_color(s, 1, o, d, lights, n_lights, rgb, nullptr, nullptr);
  if (rc) return rc;
  for (int32_t i = 1; i <= max_depth; i++) {
    int32_t face;
    float t, P[3], N[3];
    if ((rc = rt_trace_closest_normal(s, 1, o, d, &face, &t, P, N))) return rc;
    rt_ray_segment& g = out[i - 1];
    memcpy(g.origin, o, 12);
    memcpy(g.direction, d, 12);
    memcpy(g.color, rgb, 12);
    *n_out = i;
    if (t == INFINITY) {
      g.length = 10.0f;
      return RT_OK;
    }
    g.length = t;
    if (i != max_depth) {
      const f3 dn = rt::reflect(dir, f3{N[0], N[1], N[2]});
      const f3 start = rt::offset(f3{P[0], P[1], P[2]}, dn, 0.001f);
      o[0] = start.x; o[1] = start.y; o[2] = start.z;
      d[0] = dn.x; d[1] = dn.y; d[2] = dn.z;
    }
  }
  return RT_OK;
}

extern "C" void rt_camera_flycam(int32_t W, int32_t H, float dx, float dy, float dz, rt_camera* c) {
  // Flycamera::translate (flycamera.hpp:196-202), yaw = identity at rotation_Y_axis = 0
  const float I9[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float speed = 0.05f;  // flycamera.hpp:107
  f3 yv = rt::m3v3(I9, f3{-dx, -dy, dz});
  f3 tv{0.0f + yv.x * speed, 0.0f + yv.y * speed, 0.0f + yv.z * speed};
  // updateViewMatrix (flycamera.hpp:166-191) at zero rotation
  rt::identity4(c->view_matrix);
  rt::translate4(c->view_matrix, f3{0.0f, 0.0f, -2.0f});
  rt::translate4(c->view_matrix, tv);
  c->viewport[0] = 0.0f; c->viewport[1] = 0.0f; c->viewport[2] = (float)W; c->viewport[3] = (float)H;
  c->fovy = 60.0f;                     // flyscene.cpp:14
  c->aspect_ratio = (float)W / (float)H;
}
