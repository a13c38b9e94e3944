// rt_faceflags.h -- the per-face arithmetic of scene preparation over plain pointers, shared by the host stages
// (rt_layout.cpp: safe_normal, face_normal_tilt, accept_region, box_certified call these) and the device update's
// kernels (rt_update_kernels.h). One copy of every expression: float parts from rt_math.h's primitives, double parts
// as fixed sequences of IEEE operations (no contraction: -ffp-contract=off on both sides; division and square root
// correctly rounded on both sides), min / max spelled as std::min / std::max evaluate them. What each function
// bounds is argued where the host stage documents it (rt_layout.cpp).
#pragma once
#include "rt_math.h"

// always inlined on the host as well: the host stages call these once or twice per face from their parallel loops
#if defined(__HIPCC__) || defined(__HIP__)
#define RT_FF RT_HD
#else
#define RT_FF inline __attribute__((always_inline))
#endif

namespace rt {

constexpr double kCertNormalSin = 1e-3;  // a face certifies only within this sine of its world triangle's normal
constexpr double kBoundTilt = 1e-6;      // beyond this sine a face is bounded by its accept-region triangle

RT_FF double dmin_std(double a, double b) { return (b < a) ? b : a; }  // std::min(a, b)
RT_FF double dmax_std(double a, double b) { return (a < b) ? b : a; }  // std::max(a, b)
RT_FF bool finite_f(float x) { return fabsf(x) <= 3.402823466e+38f; }  // std::isfinite (NaN compares false)
RT_FF bool finite_d(double x) { return fabs(x) <= 1.7976931348623157e+308; }

RT_FF f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }

// safe_normal of a face: world vertices w0 w1 w2, unit face normal n, unit vertex normals n0 n1 n2
RT_FF bool safe_normal_of(f3 w0, f3 w1, f3 w2, f3 n, f3 n0, f3 n1, f3 n2) {
  const f3 e0 = sub(w1, w0), e2 = sub(w0, w2);
  const float A = norm(cross(e0, neg(e2))) / 2;
  if (!(A > 1e-30f) || !finite_f(A)) return false;
  const f3 nk[3] = {n0, n1, n2};
  for (int k = 0; k < 3; k++) {
    if (!finite_f(nk[k].x) || !finite_f(nk[k].y) || !finite_f(nk[k].z)) return false;
    if (fabsf(sqnorm(nk[k]) - 1.0f) > 1e-3f) return false;
    if (!(dot(n, nk[k]) >= 0.5f)) return false;
  }
  return true;
}

// sin of the angle between the face normal the edge tests use and the world triangle's normal (2 on degenerate or
// non-finite input: never certified)
RT_FF double face_tilt_of(f3 p0, f3 p1, f3 p2, f3 nf) {
  const double w[3][3] = {{p0.x, p0.y, p0.z}, {p1.x, p1.y, p1.z}, {p2.x, p2.y, p2.z}};
  const double a[3] = {w[1][0] - w[0][0], w[1][1] - w[0][1], w[1][2] - w[0][2]};
  const double c[3] = {w[2][0] - w[0][0], w[2][1] - w[0][1], w[2][2] - w[0][2]};
  const double g[3] = {a[1] * c[2] - a[2] * c[1], a[2] * c[0] - a[0] * c[2], a[0] * c[1] - a[1] * c[0]};
  const double n[3] = {nf.x, nf.y, nf.z};
  const double gg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2], nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  if (!finite_d(gg) || !finite_d(nn) || !(gg > 0.0) || !(nn > 0.0)) return 2.0;
  const double x[3] = {g[1] * n[2] - g[2] * n[1], g[2] * n[0] - g[0] * n[2], g[0] * n[1] - g[1] * n[0]};
  const double dn = g[0] * n[0] + g[1] * n[1] + g[2] * n[2];
  if (!(dn > 0.0)) return 2.0;  // opposite orientation: the edge tests' inside is the other side
  return sqrt((x[0] * x[0] + x[1] * x[1] + x[2] * x[2]) / (gg * nn));
}

// one accept-region vertex: w itself, or on a tilted face w projected along n onto the plane n.x = dist
RT_FF f3 accept_vertex_of(f3 w, f3 nf, float dist, bool tilted) {
  const double n[3] = {nf.x, nf.y, nf.z}, nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
  if (!tilted || !(nn > 0.0) || !finite_d(nn)) return w;
  const double s = (n[0] * w.x + n[1] * w.y + n[2] * w.z - (double)dist) / nn;
  return f3{(float)(w.x - s * n[0]), (float)(w.y - s * n[1]), (float)(w.z - s * n[2])};
}

// box_certified of a face behind its Ro / tilt gates: object-space vertices o0 o1 o2 (raw xyz), its reference box
RT_FF bool box_certified_of(const float* o0, const float* o1, const float* o2, const float* blow, const float* bhigh, float Ro,
                            double tilt) {
  const float* o[3] = {o0, o1, o2};
  double v[3][3];
  for (int j = 0; j < 3; j++)
    for (int k = 0; k < 3; k++) {
      v[j][k] = o[j][k];
      if (!finite_d(v[j][k])) return false;
    }
  // edge lengths and the smallest angle (law of cosines, in double)
  double L[3];
  for (int j = 0; j < 3; j++) {
    const double* a = v[j];
    const double* c = v[(j + 1) % 3];
    L[j] = sqrt((c[0] - a[0]) * (c[0] - a[0]) + (c[1] - a[1]) * (c[1] - a[1]) + (c[2] - a[2]) * (c[2] - a[2]));
  }
  const double diam = dmax_std(L[0], dmax_std(L[1], L[2]));
  if (!(diam > 0.0)) return false;
  for (int j = 0; j < 3; j++) {  // angle opposite edge j: between edges j+1 and j+2
    const double a = L[(j + 1) % 3], c = L[(j + 2) % 3], e = L[j];
    if (!(a > 0.0 && c > 0.0)) return false;
    const double cosv = dmin_std(1.0, dmax_std(-1.0, (a * a + c * c - e * e) / (2.0 * a * c)));
    const double s_half = sqrt(dmax_std(0.0, (1.0 - cosv) / 2.0));  // sin(theta / 2)
    if (!(s_half >= 0.01)) return false;
  }
  for (int k = 0; k < 3; k++) {
    const double lo = blow[k], hi = bhigh[k];
    if (!finite_d(lo) || !finite_d(hi)) return false;
    const double S = (hi - lo) + fabs(lo) + fabs(hi);
    const double need = 1e-5 * (S + Ro) + 1e-30 + 1e-5 * S + 4e-4 * diam + 2.0 * tilt * diam;
    for (int j = 0; j < 3; j++)
      if (!(v[j][k] - lo >= need && hi - v[j][k] >= need)) return false;
  }
  return true;
}

}  // namespace rt
