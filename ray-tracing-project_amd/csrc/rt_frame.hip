// rt_frame.hip -- the single-device frame path of the MI355X ray-traversal library: a frame's parameters, the
// longest-first dispatch order (k_order_lpt), the frame buffers, the box-colour table, the launch of the kernel the
// plan names (rt_dispatch.h plan_frame), and the wait for it; rt_render* and the debug readers. The frame
// kernels are rt_frame_kernels.h (with k_render_depth of rt_trace_ray.h; shared with the A/B variants of
// rt_variants.hip): this is the one product translation unit that instantiates them, and it holds the weak default
// of variant_launch (rt_variant_api.h).
#include <atomic>
#include <vector>

#include "rt_device.h"
#include "rt_frame_kernels.h"
#include "rt_variant_api.h"

namespace rt {

// Longest-first dispatch order for the next frame of the same shape (after the frame, one workgroup per
// XCD class). The default order hands XCD x the dispatch positions p = 8r + x and fills them with the
// logical waves of class x (below `full`: runs of C consecutive waves, j = (k / C) 8C + x C + k % C for
// k = p / 8, so an XCD's L2 serves neighbouring tiles; the trailing partial group identity-mapped).
// This keeps every wave in its class and stably reorders each class by the wave's measured cost,
// longest first: LPT scheduling -- the waves that finish a frame late become the cheap ones (the
// measured one-frame tail was 40% of the frame) -- while waves of equal cost keep their spatial order.
// Counting sort over kLptBuckets log-spaced cost buckets (4 per octave, from the float exponent and two
// mantissa bits): per-thread counts in LDS, one wave-parallel exclusive scan per bucket, then every
// thread places its contiguous run of waves. Any order is a permutation: every frame renders identical
// bits.
constexpr int kLptBuckets = 32, kLptThreads = 512, kLptRefresh = 8;
constexpr bool kLptMoved = true;  // re-sort after every lone frame whose camera moved since the map's frame
constexpr int kLptDilate = 2;     // a moving camera's map: each wave's cost = the max over (2r+1)^2 waves around it
// ... or around the waves where its content is expected next frame (FrameParams::pred), then over a ring of 1
// (profiles/ab/r06_moving_prediction_ab.txt: C5 moving lone frames 0.295 -> 0.26 ms)
constexpr bool kLptPred = true;
constexpr int kLptDilatePred = 1;

// The camera's last step as a view-space transform, D = V_n V_(n-1)^-1 (both world -> view, column-major 4 x 4
// affine, tucano Camera::view_matrix); its translation (FrameParams::pred_step). Flycamera::translate (the
// reference's WASD keys, flycamera.hpp:196-202) moves translation_vector under a fixed rotation, so D is a pure
// translation there; a rotated step keeps only its translation (the prediction is a dispatch-order hint).
static void camera_step(const float* vp_prev, const float* v_cur, float* step3) {
  double R[3][3], t[3], Ri[3][3];
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) R[i][j] = vp_prev[4 * j + i];
    t[i] = vp_prev[12 + i];
  }
  const double det = R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
                     R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]);
  step3[0] = step3[1] = step3[2] = 0.0f;
  if (!(std::fabs(det) > 1e-30)) return;  // degenerate previous view: no step
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int a = (j + 1) % 3, b = (j + 2) % 3, c = (i + 1) % 3, d = (i + 2) % 3;
      Ri[i][j] = (R[a][c] * R[b][d] - R[a][d] * R[b][c]) / det;  // inverse = adjugate / det
    }
  for (int i = 0; i < 3; i++) {  // D's translation: t_n - R_n R_(n-1)^-1 t_(n-1)
    double m = v_cur[12 + i];
    for (int j = 0; j < 3; j++) {
      double rr = 0.0;
      for (int k = 0; k < 3; k++) rr += (double)v_cur[4 * k + i] * Ri[k][j];
      m -= rr * t[j];
    }
    step3[i] = (float)m;
  }
}
__device__ __forceinline__ uint32_t lpt_bucket(uint32_t c, int shift) {
  // 4 buckets per octave: exponent and 2 mantissa bits of (float)c; costs of 2^10 .. 2^18 shader cycles
  // (0.5 .. 120 us at 2.1 GHz) spread over the buckets, longest first (bucket 0)
  const int q = (int)(__float_as_uint((float)(c | 1u)) >> 21) - ((127 + 10) << 2);
  const int b = (q < 0 ? 0 : (q > 4 * 8 - 1 ? 4 * 8 - 1 : q)) >> shift;
  return (uint32_t)((kLptBuckets >> shift) - 1 - b);
}
// The sort reads `cost` (the recording frame's per-wave costs, or with a moving camera their dilation: the
// render kernel's waves raised cost_dil over their neighbourhoods, wave_clock_end) and clears what it read in
// both arrays, so the next recording frame starts from zeros -- the atomic maxima of split sub-waves and of the
// dilation need them -- without a fill on the frame's own critical path. Counts live in LDS, one column per
// thread (a register array indexed by the bucket compiled to a waterfall loop per access: 15 us per sort).
__global__ __launch_bounds__(kLptThreads) void k_order_lpt(uint32_t* cost, uint32_t* clear2, uint32_t* order, int n, int C,
                                                           int shift) {
  __shared__ uint32_t cnt[kLptBuckets][kLptThreads];
  __shared__ uint32_t base[kLptBuckets];
  const int x = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, wv = t >> 6;
  const int full = (n / (8 * C)) * 8 * C;
  const int m = (n - x + 7) / 8;  // positions 8r + x < n of this class
  const int chunk = (m + kLptThreads - 1) / kLptThreads, r0 = t * chunk, r1 = min(m, r0 + chunk);
  const int nb = kLptBuckets >> shift;
  auto item = [&](int r) {  // the logical wave the default order puts at position 8r + x
    const int p = 8 * r + x;
    if (p >= full) return p;
    const int k = p >> 3;
    return (k / C) * 8 * C + x * C + (k % C);
  };
  for (int b = 0; b < nb; b++) cnt[b][t] = 0;
  for (int r = r0; r < r1; r++) cnt[lpt_bucket(cost[item(r)], shift)][t]++;
  __syncthreads();
  // exclusive scan of each bucket's per-thread counts: wave w scans buckets w, w + 8, ..; lane i owns
  // threads 8i .. 8i + 7
  for (int b = wv; b < nb; b += kLptThreads / 64) {
    uint32_t v[8], s = 0;
    for (int k = 0; k < 8; k++) { v[k] = cnt[b][8 * lane + k]; s += v[k]; }
    uint32_t incl = s;
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    uint32_t run = incl - s;
    for (int k = 0; k < 8; k++) { cnt[b][8 * lane + k] = run; run += v[k]; }
    if (lane == 63) base[b] = incl;  // bucket total
  }
  __syncthreads();
  if (wv == 0) {  // bucket totals -> start ranks, longest bucket first (one lane per bucket)
    const uint32_t v = lane < nb ? base[lane] : 0u;
    uint32_t incl = v;
    for (int off = 1; off < 32; off <<= 1) {
      const uint32_t o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    if (lane < nb) base[lane] = incl - v;
  }
  __syncthreads();
  for (int r = r0; r < r1; r++) {
    const int j = item(r);
    const uint32_t b = lpt_bucket(cost[j], shift);
    const uint32_t rr = base[b] + cnt[b][t]++;
    order[8 * rr + x] = (uint32_t)j;
    cost[j] = 0u;
    if (clear2) clear2[j] = 0u;
  }
}

// RT_MODE_BOX_COLORS, once per colour set: for every face id, color += box->color over the reference
// boxes in creation order whose [low, high] holds all three object-space vertices (BoundingBox::hasFace,
// BoundingBox.cpp:26-39; flyscene.cpp:337-341), summed in that order in fp32 as the reference does. One
// thread per face; the boxes (bounds from the refbox array, colours) are staged through LDS in chunks and
// read as wave-wide broadcasts.
constexpr int kBoxColorChunk = 1024;
__global__ __launch_bounds__(256) void k_face_box_colors(const float* fv9, const float* refbox, const float* col3,
                                                         int nb, int nf, float* out4) {
  __shared__ float sb[9][kBoxColorChunk];  // low xyz, high xyz, colour rgb
  const int f = (int)(blockIdx.x * 256u + threadIdx.x);
  const bool act = f < nf;
  float v[9];
  for (int k = 0; k < 9; k++) v[k] = act ? fv9[9 * (size_t)f + k] : 0.0f;
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  for (int b0 = 0; b0 < nb; b0 += kBoxColorChunk) {
    const int n = min(kBoxColorChunk, nb - b0);
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
      const float* rb = refbox + 8 * (size_t)(b0 + i);
      sb[0][i] = rb[0]; sb[1][i] = rb[1]; sb[2][i] = rb[2];
      sb[3][i] = rb[4]; sb[4][i] = rb[5]; sb[5][i] = rb[6];
      const float* c = col3 + 3 * (size_t)(b0 + i);
      sb[6][i] = c[0]; sb[7][i] = c[1]; sb[8][i] = c[2];
    }
    __syncthreads();
    if (act)
      for (int i = 0; i < n; i++) {
        bool in = true;
        for (int k = 0; k < 3; k++) {
          const float x = v[3 * k], y = v[3 * k + 1], z = v[3 * k + 2];
          in = in && x >= sb[0][i] && x <= sb[3][i] && y >= sb[1][i] && y <= sb[4][i] && z >= sb[2][i] && z <= sb[5][i];
        }
        if (in) { c0 += sb[6][i]; c1 += sb[7][i]; c2 += sb[8][i]; }
      }
  }
  if (act) reinterpret_cast<float4*>(out4)[f] = make_float4(c0, c1, c2, 0.0f);
}

// the known-answer cases of rt_kat.h (rt_debug_math_device): here, because they share the frame kernels' device functions
__global__ void k_debug_math(int op, int n, int in_len, int out_len, const float* in, float* out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) debug_math_case(op, in + (size_t)k * in_len, out + (size_t)k * out_len);
}

// RT_MODE_BOX_COLORS: (re)computes the per-face box-colour sums when the colours changed. The scene's
// streams are drained first (earlier box-colour frames in flight read the table). A replica never sets
// colours itself: render_multi gives the scene its default colours, and with them every replica, before any
// enqueue worker runs (a replica's worker calling rt_scene_set_box_colors wrote every replica's
// colour vector while the other workers read theirs).
static int ensure_face_boxcolor(rt_scene* s) {
  if (s->face_boxcolor_valid) return RT_OK;
  HostScene& hs = s->hs;
  if (s->box_colors.size() != 3 * hs.boxes.size()) {
    if (s->is_replica) { set_error("device %d: replica without box colours", s->device); return RT_ERR_INVALID; }
    const int rc = rt_scene_set_box_colors(s, nullptr);
    if (rc) return rc;
  }
  // (hs.ov3 after a device update: a replica's scene has mirrored before its workers run, rt_multi.hip)
  if (!s->is_replica)
    if (const int rc = host_mirror_geometry(s)) return rc;
  if (hs.ov3.size() != 3 * (size_t)hs.nv) { set_error("scene has no object-space vertices"); return RT_ERR_INVALID; }
  if (const int rc = drain_slots(s)) return rc;
  const size_t nf = (size_t)hs.nf, nb = hs.boxes.size();
  if (!s->d_face_boxcolor) {
    HIPCHECK(hipMalloc((void**)&s->d_face_boxcolor, 16 * std::max<size_t>(nf, 1)));
    s->device_bytes += (int64_t)(16 * std::max<size_t>(nf, 1));
  }
  if (nf > 0) {
    std::vector<float> fv(9 * nf);
    for (size_t f = 0; f < nf; f++)
      for (int k = 0; k < 3; k++) memcpy(&fv[9 * f + 3 * k], &hs.ov3[3 * (size_t)hs.fidx[3 * f + k]], 12);
    float *d_fv = nullptr, *d_col = nullptr;
    struct Free { float** a; float** b; ~Free() { if (*a) (void)hipFree(*a); if (*b) (void)hipFree(*b); } } free_{&d_fv, &d_col};
    HIPCHECK(hipMalloc((void**)&d_fv, fv.size() * 4));
    HIPCHECK(hipMalloc((void**)&d_col, std::max<size_t>(nb, 1) * 12));
    HIPCHECK(hipMemcpy(d_fv, fv.data(), fv.size() * 4, hipMemcpyHostToDevice));
    if (nb) HIPCHECK(hipMemcpy(d_col, s->box_colors.data(), nb * 12, hipMemcpyHostToDevice));
    hipStream_t st = (hipStream_t)s->stream;
    hipLaunchKernelGGL(k_face_box_colors, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, st, d_fv, s->d_refbox, d_col,
                       (int)nb, (int)nf, s->d_face_boxcolor);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
  }
  s->face_boxcolor_valid = true;
  return RT_OK;
}

void fill_scene_params(const rt_scene* s, FrameParams& P) {
  memset(&P, 0, sizeof P);
  const HostScene& hs = s->hs;
  P.sc.nodes = s->d_nodes;
  P.sc.tris = s->d_tris;
  P.sc.fshade = s->d_fshade;
  P.sc.refbox = s->d_refbox;
  P.sc.mats = s->d_mats;
  P.sc.root = !is_leaf(hs.root) ? hs.root * 64u : hs.root;
  P.sc.n_nodes = (int32_t)hs.nodes.size();
  P.sc.nodes4 = s->d_nodes4;
  P.sc.root4 = 0;
  P.sc.n_nodes4 = (int32_t)hs.nodes4.size();
  P.sc.static_pad = s->static_pad;
  P.sc.cert_origin_max = s->cert_origin_max;
  P.sc.wide_base = s->wide_base;
  P.sc.wide_copy_bytes = s->wide_copy_bytes;
  P.sc.rec_bytes = (uint32_t)((hs.nodes.size() + hs.tris.size()) * 64);
  P.sc.tri_bytes = (uint32_t)(hs.tris.size() * 64);
  P.sc.all_bytes = (uint32_t)std::min<size_t>(s->nodes_bytes, 0xFFFFFFFFu);
  P.sc.pf_check = s->d_pf_check;
  memcpy(P.sc.Minv, hs.Minv, 64);
  memcpy(P.Minv, hs.Minv, 64);
  memcpy(P.MS, hs.MS, 36);
  const rt_material& dm = s->opts.default_material;
  for (int k = 0; k < 3; k++) { P.defmat.ka[k] = dm.ka[k]; P.defmat.kd[k] = dm.kd[k]; P.defmat.ks[k] = dm.ks[k]; }
  P.defmat.ns = dm.shininess;
  memcpy(P.bg, s->opts.background, 12);
}

// FULL pipeline hand-off buffers: state0, state1 (32 B), refl (32 B), hits1 (8 B), blk0, blk1, list0,
// list1 (4 B) per pixel; then per list wave wcount0/1, woff0/1; then the counters
constexpr size_t kFullBytesPerPixel = 32 + 32 + 32 + 8 + 4 + 4 + 4 + 4;
static size_t full_waves(size_t npix) { return (npix + 63) / 64 + 8; }
static int ensure_full(rt_scene::FrameSlot& f, size_t npix) {
  if (npix <= f.full_pixels) return RT_OK;
  return regrow(f.d_full, f.full_pixels, npix, npix * kFullBytesPerPixel + 16 * full_waves(npix) + 64, (hipStream_t)f.stream);
}
static void bind_full(const rt_scene::FrameSlot& f, FrameParams& P) {
  char* b = (char*)f.d_full;
  const size_t n = f.full_pixels;
  P.state0 = (HitState*)b;
  P.state1 = (HitState*)(b + 32 * n);
  P.refl = (RayRec*)(b + 64 * n);
  P.hits1 = (uint2*)(b + 96 * n);
  P.blk0 = (uint32_t*)(b + 104 * n);
  P.blk1 = (uint32_t*)(b + 108 * n);
  P.list0 = (uint32_t*)(b + 112 * n);
  P.list1 = (uint32_t*)(b + 116 * n);
  const size_t q = full_waves(n);
  char* w = b + 120 * n;
  P.wcount0 = (uint32_t*)w;
  P.wcount1 = (uint32_t*)(w + 4 * q);
  P.woff0 = (uint32_t*)(w + 8 * q);
  P.woff1 = (uint32_t*)(w + 12 * q);
  P.counters = (uint32_t*)(w + 16 * q);
  P.n_waves_max = (int32_t)q;
}

static int ensure_fb(rt_scene::FrameSlot& f, size_t npix) {
  if (npix <= f.fb_pixels) return RT_OK;
  HIPCHECK(hipStreamSynchronize((hipStream_t)f.stream));  // the slot's previous frames may still use them
  if (f.d_rgb) (void)hipFree(f.d_rgb);
  if (f.d_face) (void)hipFree(f.d_face);
  if (f.d_t) (void)hipFree(f.d_t);
  if (f.d_hits) (void)hipFree(f.d_hits);
  f.d_rgb = nullptr; f.d_face = nullptr; f.d_t = nullptr; f.d_hits = nullptr;
  f.fb_pixels = 0;
  HIPCHECK(hipMalloc((void**)&f.d_rgb, npix * 12));
  HIPCHECK(hipMalloc((void**)&f.d_face, npix * 4));
  HIPCHECK(hipMalloc((void**)&f.d_t, npix * 4));
  HIPCHECK(hipMalloc((void**)&f.d_hits, npix * 8));
  f.fb_pixels = npix;
  return RT_OK;
}

// The variants library defines the strong variant_launch / variants_linked (rt_variants.hip); in the
// product library these weak defaults stand, and rt_render_async refuses a variant-only frame up front.
__attribute__((weak)) bool variants_linked() { return false; }
__attribute__((weak)) int variant_launch(int, const VariantCall&) { return RT_ERR_UNSUPPORTED; }

static std::atomic<int> g_variant{0};  // rt_debug_set_variant(), or RT_KERNEL_VARIANT once rt_debug_env_knobs(1)
int kernel_variant() { return g_variant.load(std::memory_order_relaxed); }

}  // namespace rt

using namespace rt;

// the last frame's diagnostic records (8 words per wave) of kind `what`, which it kept if `have`
static int read_wave_records(rt_scene* s, const char* who, const char* what, bool have, uint32_t* rt_scene::FrameSlot::*buf,
                             int64_t waves, int64_t capacity_waves, uint32_t* out8, int64_t* n_waves) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  const rt_scene::FrameSlot& f = s->slots[s->last_slot];
  if (!have || !(f.*buf)) { set_error("%s: last frame had no %s", who, what); return RT_ERR_INVALID; }
  if (n_waves) *n_waves = waves;
  if (!out8) return RT_OK;
  if (capacity_waves < waves) { set_error("%s: buffer too small", who); return RT_ERR_INVALID; }
  HIPCHECK(hipStreamSynchronize((hipStream_t)f.stream));
  HIPCHECK(hipMemcpy(out8, f.*buf, (size_t)waves * 32, hipMemcpyDeviceToHost));
  return RT_OK;
}
extern "C" int rt_debug_timeline(rt_scene* s, int64_t capacity_waves, uint32_t* out8, int64_t* n_waves) {
  return read_wave_records(s, "rt_debug_timeline", "RT_FRAME_TIMELINE", s && (s->last_flags & RT_FRAME_TIMELINE),
                           &rt_scene::FrameSlot::d_timeline, s ? s->last_timeline_waves : 0, capacity_waves, out8, n_waves);
}
extern "C" int rt_debug_wave_stats(rt_scene* s, int64_t capacity_waves, uint32_t* out8, int64_t* n_waves) {
  const int both = RT_FRAME_STATS | RT_FRAME_WAVE_STATS;
  return read_wave_records(s, "rt_debug_wave_stats", "RT_FRAME_STATS | RT_FRAME_WAVE_STATS", s && (s->last_flags & both) == both,
                           &rt_scene::FrameSlot::d_wave_stats, s ? s->last_wave_stats_waves : 0, capacity_waves, out8, n_waves);
}

extern "C" int rt_debug_counters(rt_scene* s, int64_t n, int64_t* out) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  if (!out || n < 0) { set_error("rt_debug_counters: no output"); return RT_ERR_INVALID; }
  if (!(s->last_flags & RT_FRAME_STATS)) { set_error("rt_debug_counters: last frame had no RT_FRAME_STATS"); return RT_ERR_INVALID; }
  HIPCHECK(hipSetDevice(s->device));
  HIPCHECK(hipDeviceSynchronize());
  unsigned long long c[kStatSlots];
  HIPCHECK(hipMemcpy(c, s->d_stats, sizeof c, hipMemcpyDeviceToHost));
  for (int64_t i = 0; i < n; i++) out[i] = i < ST_COUNT ? (int64_t)c[i] : 0;
  return RT_OK;
}

extern "C" int rt_debug_lpt_stats(const rt_scene* s, int64_t* out3) {
  if (!s || !out3) { set_error("rt_debug_lpt_stats: null argument"); return RT_ERR_INVALID; }
  out3[0] = s->lpt.frames;
  out3[1] = s->lpt.sorts;
  out3[2] = s->lpt.valid ? 1 : 0;
  return RT_OK;
}

extern "C" int rt_debug_math_device(int32_t op, int32_t n, const float* in, float* out) {
  static const int in_len[] = {6, 3, 6, 12, 19, 20, 9, 16, 4, 6, 6, 6, 6, 13, 3, 16, 24, 2};
  static const int out_len[] = {1, 3, 3, 3, 3, 4, 9, 16, 16, 3, 3, 3, 3, 3, 1, 3, 3, 1};
  if (op < 0 || op > 17 || n <= 0 || !in || !out) { set_error("rt_debug_math_device: bad arguments"); return RT_ERR_INVALID; }
  if (rt_device_count() == 0) { set_error("no HIP device"); return RT_ERR_NO_DEVICE; }
  float *di = nullptr, *dout = nullptr;
  struct Free { float** a; float** b; ~Free() { if (*a) (void)hipFree(*a); if (*b) (void)hipFree(*b); } } free_{&di, &dout};
  const size_t ib = (size_t)n * in_len[op] * 4, ob = (size_t)n * out_len[op] * 4;
  HIPCHECK(hipMalloc((void**)&di, ib));
  HIPCHECK(hipMalloc((void**)&dout, ob));
  HIPCHECK(hipMemcpy(di, in, ib, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_debug_math, dim3((n + 255) / 256), dim3(256), 0, 0, (int)op, (int)n, in_len[op], out_len[op], di, dout);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost));
  return RT_OK;
}

extern "C" int rt_debug_env_knobs(int32_t on) {
  set_debug_env(on != 0);
  if (on) {  // RT_KERNEL_VARIANT: the A/B kernel variant of this process (rt_debug_set_variant overrides it)
    const char* e = debug_env("RT_KERNEL_VARIANT");
    const int v = e ? atoi(e) : 0;
    g_variant.store(v < 0 ? 0 : v);
  }
  return RT_OK;
}

extern "C" int rt_debug_set_variant(int32_t v) {
  const int prev = kernel_variant();
  g_variant.store(v < 0 ? 0 : v);
  return prev;
}

static int check_frame_args(const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* fr) {
  if (!cam || !fr || fr->width <= 0 || fr->height <= 0 || n_lights < 0 || n_lights > RT_MAX_LIGHTS ||
      (n_lights && !lights)) {
    set_error("rt_render: invalid arguments");
    return RT_ERR_INVALID;
  }
  if (fr->mode != RT_MODE_PRIMARY && fr->mode != RT_MODE_FULL && fr->mode != RT_MODE_BOX_COLORS) { set_error("rt_render: bad mode %d", fr->mode); return RT_ERR_INVALID; }
  if (fr->max_depth < 0 || fr->max_depth > RT_MAX_TRACE_DEPTH) {
    set_error("rt_render: max_depth %d outside 0..%d", fr->max_depth, RT_MAX_TRACE_DEPTH);
    return RT_ERR_INVALID;
  }
  const int sc = fr->shard_count > 0 ? fr->shard_count : 1;
  if (fr->shard_index < 0 || fr->shard_index >= sc) { set_error("rt_render: shard %d of %d", fr->shard_index, sc); return RT_ERR_INVALID; }
  return RT_OK;
}

// camera (camera.hpp:115-118,155-173,263-266) and lights of a frame; P.Minv is set (fill_scene_params)
void rt::fill_camera_lights(FrameParams& P, const rt_camera* cam, const rt_light* lights, int32_t n_lights) {
  affinv(cam->view_matrix, P.vinv);
  float L[9], Li[9];
  linear_of(cam->view_matrix, L);
  m3inv(L, Li);
  const f3 e = m3v3(Li, f3{-cam->view_matrix[12], -cam->view_matrix[13], -cam->view_matrix[14]});
  P.eye[0] = e.x; P.eye[1] = e.y; P.eye[2] = e.z;
  const f3 eo = affv3(P.Minv, e);
  P.eye_obj[0] = eo.x; P.eye_obj[1] = eo.y; P.eye_obj[2] = eo.z;
  memcpy(P.vp, cam->viewport, 16);
  const float persp = (float)((double)1.0f / tan((double)(cam->fovy / 2.0f) * (M_PI / 180.0)));
  const float scale = (float)(1.0 / (double)persp);
  P.xscale = cam->aspect_ratio * scale;
  P.yscale = scale;
  fill_lights(P, lights, n_lights);
}

// a slot's diagnostic records (timeline, per-wave counts; 8 words per wave): room for `waves`, cleared on st
static int ensure_wave_records(uint32_t*& ptr, size_t& capacity, size_t waves, hipStream_t st) {
  int rc;
  if (waves > capacity && (rc = regrow(ptr, capacity, waves, waves * 32, st))) return rc;
  HIPCHECK(hipMemsetAsync(ptr, 0, waves * 32, st));
  return RT_OK;
}

// Longest-first dispatch of a lone frame (plan.lpt): binds the order the scene's previous lone frame of this shape
// left; `sort`: this frame records its costs and lpt_end sorts them after it, `dilated`: from a moving camera's map
static int lpt_begin(rt_scene* s, const FramePlan& plan, const rt_camera* cam, hipStream_t st, FrameParams& P, bool& sort,
                     bool& dilated) {
  rt_scene::LptMap& lm = s->lpt;
  const size_t waves = plan.units;
  if (waves > lm.waves) {
    if (const int rc = drain_slots(s)) return rc;
    lm.waves = 0, lm.valid = false;
    for (uint32_t** p : {&lm.d_cost, &lm.d_cost_dil, &lm.d_order}) {
      if (*p) (void)hipFree(*p);
      *p = nullptr;
      HIPCHECK(hipMalloc((void**)p, waves * 4));
    }
    HIPCHECK(hipMemsetAsync(lm.d_cost, 0, waves * 4, st));  // (each sort clears what it read after this)
    HIPCHECK(hipMemsetAsync(lm.d_cost_dil, 0, waves * 4, st));
    lm.waves = waves;
  }
  const int64_t key[8] = {P.W, P.H, P.shard_index, P.shard_count, P.mode, plan.depth, plan.xcd_remap, (int64_t)waves};
  const bool same = lm.valid && memcmp(key, lm.key, sizeof key) == 0;
  if (same) P.order = lm.d_order;
  // The order is recomputed from this frame's costs after the frame when it is missing, has served
  // kLptRefresh frames, or -- kLptMoved -- the camera has moved since the frame that recorded it (the
  // reference's Flycamera moves every frame while a key is held, flyscene.cpp:116-127): a moving camera then
  // dispatches every lone frame by the previous frame's costs. The sort costs a few microseconds on the frame's
  // stream. (RT_LPT_REFRESH / RT_LPT_MOVED: A/B knobs, debug environment only.)
  const int refresh = knob_int("RT_LPT_REFRESH", kLptRefresh, 1, INT_MAX);
  const int moved_knob = knob_int("RT_LPT_MOVED", kKnobUnset, INT_MIN, INT_MAX);
  const bool moved = memcmp(cam->view_matrix, lm.view, sizeof lm.view) != 0;
  // moving: this frame's camera differs from the previous lone frame's -> its costs are placed where each wave's
  // content is expected in the next frame (the camera repeating its step, FrameParams::pred) and dilated before the
  // sort (whole frames only: the wave grid of a shard is not contiguous). RT_LPT_DILATE / RT_LPT_PRED: A/B knobs
  const bool moving = memcmp(cam->view_matrix, lm.prev_view, sizeof lm.prev_view) != 0;
  float prev_view[16];
  memcpy(prev_view, lm.prev_view, sizeof prev_view);
  memcpy(lm.prev_view, cam->view_matrix, sizeof lm.prev_view);
  // Measured under the reference's moving camera (profiles/ab/r06_moving_camera_ab.txt, one frame at a time):
  // an L2-resident scene whose lone frames split their costliest waves (C5: the bunny's silhouette tiles) loses
  // the split's gain with a map even one frame old (0.38 ms against 0.227 with an exact map) and regains most
  // of it with a fresh, dilated map (0.31 ms), more with the costs moved to their predicted waves (0.26 ms,
  // profiles/ab/r06_moving_prediction_ab.txt); the soup's per-wave costs decorrelate within a frame of motion
  // (fresh or 8 frames old, dilated or not: 0.233-0.237 ms, no map 0.245; predicted: 0.226 ms, but the sort on
  // every frame's path takes it back), so large scenes keep the 8-frame refresh and spend no sort per frame.
  // (RT_LPT_MOVED forces either rule.)
  const bool resort_on_motion = moved_knob != kKnobUnset ? moved_knob != 0 : (kLptMoved && plan.l2_resident);
  // (a dilated map is replaced by the first frame after the camera stopped: dilated, the map spends the split on
  // the costly waves' neighbours -- 0.30 ms instead of 0.22 on C5 at an exact pose)
  sort = !same || ++lm.age >= refresh || (resort_on_motion && moved) || (lm.dilated_map && !moving);
  lm.frames++;
  if (!sort) return RT_OK;
  memcpy(lm.key, key, sizeof key);
  memcpy(lm.view, cam->view_matrix, sizeof lm.view);
  lm.valid = false;  // until this frame's k_order_lpt has been queued
  P.cost = lm.d_cost;
  lm.sorts++;
  // RT_LPT_PRED (A/B knob): each wave's cost lands where its content is expected next frame (FrameParams::pred)
  const bool pred = knob_int("RT_LPT_PRED", kLptPred, INT_MIN, INT_MAX) != 0;
  const int r = knob_int("RT_LPT_DILATE", pred ? kLptDilatePred : kLptDilate, 0, 3);  // (2 + 2 r)^2 <= 64 lanes
  dilated = moving && resort_on_motion && P.shard_count == 1 && plan.kernel != FK_PRIMARY_DUAL && (r > 0 || pred);
  lm.dilated_map = dilated;
  if (!dilated) return RT_OK;
  lm.dilated++;
  P.cost_dil = lm.d_cost_dil;
  P.dil_r = r;
  if (pred) {  // a pixel's view-space direction (nx xscale, ny yscale, -1) as (a px + b, c py + e, -1)
    P.pred = 1;
    P.pred_proj[0] = 2.0f * P.xscale / P.vp[2];
    P.pred_proj[1] = -(2.0f * P.vp[0] / P.vp[2] + 1.0f) * P.xscale;
    P.pred_proj[2] = -2.0f * P.yscale / P.vp[3];
    P.pred_proj[3] = (1.0f + 2.0f * P.vp[1] / P.vp[3]) * P.yscale;
    camera_step(prev_view, cam->view_matrix, P.pred_step);
  }
  return RT_OK;
}

// the sort for the scene's next lone frame of this shape, on this frame's stream before its done event: the next
// lone frame is queued only once every other slot's done event has passed (`alone`), so it finds the order
// complete whichever slot it takes
static int lpt_end(rt_scene* s, const FramePlan& plan, hipStream_t st, bool dilated) {
  rt_scene::LptMap& lm = s->lpt;
  hipLaunchKernelGGL(k_order_lpt, dim3(8), dim3(kLptThreads), 0, st, dilated ? lm.d_cost_dil : lm.d_cost,
                     dilated ? lm.d_cost : (uint32_t*)nullptr, lm.d_order, (int)plan.units, plan.xcd_remap,
                     plan.lpt_coarse ? 1 : 0);
  HIPCHECK(hipGetLastError());
  lm.valid = true, lm.age = 0;
  return RT_OK;
}

// the frame's render launches; ev_m is recorded after the traversal kernel
static_assert(kTraceWPB == 1 && kFullWPB == 1, "the wave split (FrameParams::split_k) is per one-wave block");
static int launch_frame(const FramePlan& plan, rt_scene* s, rt_scene::FrameSlot& slot, FrameParams& P, hipStream_t st,
                        hipEvent_t ev_m) {
  const int grid = plan.grid;
  const bool stats = (P.flags & RT_FRAME_STATS) != 0, hits = (P.flags & RT_FRAME_WRITE_HITS) != 0;
  const bool boxcol = P.mode == RT_MODE_BOX_COLORS;
  // A lone frame of a small (L2-resident) scene, dispatched longest-first, splits its costliest waves
  // into 16-lane sub-waves (FrameParams::split_k; RT_SPLIT_K / RT_SPLIT_KP waves, rounded down to a multiple
  // of 8 and at most a quarter of the frame's waves), in k_render_full and in k_primary_fused: such a frame's
  // span is its slowest waves' (C5 one frame alone: 2.2 resident waves per SIMD on average), and a 16-ray packet
  // of their incoherent secondary rays finishes sooner. A large scene's FULL frame is not tail bound (5.7
  // resident waves per SIMD on the soup) and the extra waves only cost (-6%), so it keeps whole waves. Results do
  // not depend on the grouping (exact per-lane culling, (t, rank) argmin).
  // (sub-waves take the max into the cost map, which the previous sort left at zero)
  P.split_k = P.order ? plan.split_ceiling : 0;
  VariantCall vc;
  switch (plan.kernel) {
    case FK_NONE: break;
    case FK_GENERIC_DEPTH:  // one 8x8 wave per block; a light set in device memory: its own instantiations
      with_light_source(plan.light_source, [&](auto LS) {
        with_bools([&](auto S, auto H) { hipLaunchKernelGGL((k_render_depth<S.value, H.value, decltype(LS)::value>), dim3(grid * 4), dim3(64), 0, st, P); },
                   stats, hits);
      });
      break;
    case FK_PRIMARY_DUAL:
      vc.P = P, vc.units = plan.units, vc.st = st, vc.hits = hits, vc.boxcol = boxcol;
      variant_launch(VOP_PRIMARY_DUAL, vc);
      break;
    case FK_PRIMARY_FUSED: {
      const dim3 g(grid * (4 / kTraceWPB) + 3 * P.split_k), b(64 * kTraceWPB);
      // RT_LDS_PAD (diagnostics): extra dynamic LDS per block, to cap the resident waves per CU in
      // occupancy experiments (160 KiB / (pad + 1 KiB) blocks per CU)
      const unsigned lds_pad = (unsigned)knob_int("RT_LDS_PAD", 0, INT_MIN, INT_MAX);
      // a frame without the 4-wide tree (none built, or VB_PRIMARY_BINARY_TREE) takes the binary-only instantiation
      with_bools([&](auto H, auto B, auto WD) {
        hipLaunchKernelGGL((k_primary_fused<H.value, B.value, WD.value>), g, b, lds_pad, st, P);
      }, hits, boxcol, P.sc.wide_copy_bytes != 0);
      break;
    }
    case FK_PRIMARY_TRACE_SHADE:
      if (plan.trav != TRAV_B2_LDS) {
        vc.P = P, vc.grid = grid, vc.st = st, vc.trav = plan.trav, vc.stats = stats;
        variant_launch(VOP_TRACE_PRIMARY, vc);
      } else {
        with_bools([&](auto S) { hipLaunchKernelGGL((k_trace_primary<S.value, TRAV_B2_LDS>), dim3(grid * (4 / kTraceWPB)), dim3(64 * kTraceWPB), 0, st, P); },
                   stats);
      }
      break;
    case FK_PRIMARY_TWO_RAYS:
      vc.P = P, vc.grid = grid, vc.st = st;
      variant_launch(VOP_PRIMARY_X2, vc);
      break;
    case FK_PRIMARY_PERSISTENT:
      if (!slot.d_queue) HIPCHECK(hipMalloc((void**)&slot.d_queue, 8 * sizeof(uint32_t)));
      HIPCHECK(hipMemsetAsync(slot.d_queue, 0, 8 * sizeof(uint32_t), st));
      vc.P = P, vc.grid = grid, vc.st = st, vc.variant = plan.variant, vc.device = s->device, vc.queue = slot.d_queue;
      variant_launch(VOP_PRIMARY_PERSISTENT, vc);
      break;
    case FK_FULL_MEGAKERNEL:  // occupancy by scene size (plan.full_small_build; a counting run keeps the 8-wave build)
      if (plan.trav != TRAV_B2_LDS) {
        vc.P = P, vc.grid = grid, vc.st = st, vc.trav = plan.trav, vc.stats = stats, vc.hits = hits, vc.small = plan.full_small_build;
        variant_launch(VOP_RENDER_FULL, vc);
      } else {
        const dim3 g(grid * (4 / kFullWPB) + 3 * P.split_k), b(64 * kFullWPB);
        with_bools([&](auto S, auto H, auto SMALL) {
          hipLaunchKernelGGL((k_render_full<S.value, H.value, TRAV_B2_LDS, SMALL.value ? kFullWavesPerEuSmall : kFullWavesPerEu>), g, b, 0, st, P);
        }, stats, hits, !stats && plan.full_small_build);
      }
      break;
    case FK_FULL_PIPELINE:  // records ev_m itself, before its last stage
      vc.P = P, vc.grid = grid, vc.st = st, vc.trav = plan.trav, vc.variant = plan.variant, vc.stats = stats, vc.hits = hits,
      vc.ev_m = ev_m;
      variant_launch(VOP_FULL_PIPELINE, vc);
      break;
  }
  HIPCHECK(hipGetLastError());
  if (plan.kernel != FK_FULL_PIPELINE) HIPCHECK(hipEventRecord(ev_m, st));
  if (plan.kernel == FK_PRIMARY_TRACE_SHADE || plan.kernel == FK_PRIMARY_TWO_RAYS || plan.kernel == FK_PRIMARY_PERSISTENT) {
    with_bools([&](auto H, auto B) { hipLaunchKernelGGL((k_shade_primary<H.value, B.value>), dim3(grid), dim3(256), 0, st, P); },
               hits, boxcol);
    HIPCHECK(hipGetLastError());
  }
  return RT_OK;
}

// what rt_synchronize, the downloads and the debug readers need to know about the frame just queued
static void note_frame(rt_scene* s, int slot_id, const rt_frame* fr, const FrameParams& P) {
  const int si = P.shard_index, sc = P.shard_count;
  s->last_slot = slot_id, s->next_slot = (slot_id + 1) % s->n_slots;
  s->last_W = fr->width, s->last_H = fr->height, s->last_shard_index = si, s->last_shard_count = sc, s->last_flags = fr->flags;
  // primary rays of this shard: pixels inside the frame of the shard's tiles (a walk over the shard's tiles,
  // done once per frame shape: it is host time on every frame's enqueue path otherwise)
  const int64_t rkey[4] = {fr->width, fr->height, si, sc};
  if (memcmp(rkey, s->rays_key, sizeof rkey) != 0) {
    int64_t rays = 0;
    for_each_shard_tile(shard_layout(fr->width, fr->height, si, sc, 0), [&](int, int tx, int ty) {
      rays += (int64_t)std::min(16, fr->width - tx * 16) * std::min(16, fr->height - ty * 16);
    });
    memcpy(s->rays_key, rkey, sizeof rkey);
    s->rays_of_key = rays;
  }
  s->last_rays = s->rays_of_key;
  s->pending = true;
}

// one device's share of a frame (the whole frame on a single-device scene; a replica's shard otherwise)
// ls (rt_render_lit): the frame's lights are that set's instead of lights / n_lights; rep = this replica's index in
// the set's device copies
int rt::render_one(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* fr,
                   const rt_light_set* ls, int rep) {
  int rc = check_device_scene(s);
  if (ls) lights = nullptr, n_lights = 0;
  if (rc || (rc = check_frame_args(cam, lights, n_lights, fr))) return rc;
  const int sc = fr->shard_count > 0 ? fr->shard_count : 1, si = fr->shard_index;
  if (fr->mode == RT_MODE_BOX_COLORS && (rc = ensure_face_boxcolor(s))) return rc;
  // frames in flight: round-robin over the slots; a slot's stream orders its own frames, frames on
  // different slots overlap (tail of one frame with the start of the next)
  const int slot_id = s->next_slot;
  rt_scene::FrameSlot& slot = s->slots[slot_id];
  if ((rc = ensure_fb(slot, (size_t)fr->width * fr->height))) return rc;
  hipStream_t st = (hipStream_t)slot.stream;
  FrameParams P;
  fill_scene_params(s, P);
  fill_camera_lights(P, cam, lights, n_lights);
  // (a box-colours frame ignores lights: none are handed to its kernel, whatever the set holds)
  const int light_source = (ls && fr->mode != RT_MODE_BOX_COLORS) ? fill_light_set(P, ls, rep) : LS_KERNARG;
  P.W = fr->width, P.H = fr->height, P.tiles_x = (fr->width + 15) / 16, P.tiles_y = (fr->height + 15) / 16;
  P.shard_index = si, P.shard_count = sc, P.super_tile = frame_super_tile(sc);
  P.mode = fr->mode, P.flags = fr->flags, P.shadows = fr->mode == RT_MODE_FULL ? 1 : 0;
  P.rgb = slot.d_rgb, P.face_out = slot.d_face, P.t_out = slot.d_t, P.hits = slot.d_hits;
  P.stats = s->d_stats, P.face_boxcolor = s->d_face_boxcolor;
  if (fr->flags & RT_FRAME_STATS) {
    // the counters are shared: a counting frame waits for every frame in flight on the other slots
    for (int k = 0; k < s->n_slots; k++)
      if (k != slot_id && s->slots[k].last_done) HIPCHECK(hipStreamWaitEvent(st, (hipEvent_t)s->slots[k].last_done, 0));
    HIPCHECK(hipMemsetAsync(s->d_stats, 0, kStatSlots * sizeof(unsigned long long), st));
  }
  FrameInputs in;
  in.mode = fr->mode, in.max_depth = fr->max_depth, in.flags = fr->flags;
  in.tiles_x = P.tiles_x, in.tiles_y = P.tiles_y, in.shard_index = si, in.shard_count = sc;
  in.variant = kernel_variant(), in.has_wide4 = P.sc.n_nodes4 > 0;
  in.record_bytes = (uint64_t)(s->hs.nodes.size() + s->hs.tris.size()) * 64;
  in.mem_lights = light_source == LS_KERNARG ? 0 : P.n_lights;
  in.occluder_cache = light_source != LS_MEMORY;
  // a frame alone on the GPU: no other frame of this scene in flight (the block order and the longest-first
  // order depend on it)
  for (int k = 0; k < s->n_slots; k++)
    if (k != slot_id && s->slots[k].last_done && hipEventQuery((hipEvent_t)s->slots[k].last_done) == hipErrorNotReady)
      in.alone = false;
  in.split_k = knob_int("RT_SPLIT_K", kSplitK, 0, INT_MAX);
  in.split_kp = knob_int("RT_SPLIT_KP", kSplitKPrimary, 0, INT_MAX);
  // (RT_TIMELINE_SPLIT, diagnostics only: a timeline frame keeps the lone-frame split of its costliest
  // waves; one record per block, so room for the 3 K extra blocks)
  in.timeline_split = knob_int("RT_TIMELINE_SPLIT", kKnobUnset, INT_MIN, INT_MAX) != kKnobUnset;
  const FramePlan plan = plan_frame(in);
  P.n_tiles_shard = plan.grid;
  P.max_depth = plan.depth;
  if (plan.primary_binary_tree) P.sc.wide_copy_bytes = 0;
  if (fr->flags & RT_FRAME_TIMELINE) {  // one record per one-wave block of the render kernel
    const size_t waves = in.timeline_split ? 2 * plan.units : plan.units;
    if ((rc = ensure_wave_records(slot.d_timeline, slot.timeline_waves, waves, st))) return rc;
    P.timeline = slot.d_timeline;
    s->last_timeline_waves = (int64_t)waves;
  }
  if ((fr->flags & RT_FRAME_STATS) && (fr->flags & RT_FRAME_WAVE_STATS)) {  // per logical wave (tile * 4 + quarter)
    // the generic traceRay kernel writes no per-wave records: refuse the frame instead of returning all-zero records
    if (!plan.writes_wave_stats) {
      set_error(in.mem_lights ? "rt_render_lit: RT_FRAME_WAVE_STATS is not available with a light set read from device memory (the generic-depth kernel keeps no per-wave counts)"
                              : "rt_render: RT_FRAME_WAVE_STATS needs the mode's own max_depth (the generic-depth kernel keeps no per-wave counts)");
      return RT_ERR_UNSUPPORTED;
    }
    const size_t lw = (size_t)plan.grid * 4;
    if ((rc = ensure_wave_records(slot.d_wave_stats, slot.wave_stats_waves, lw, st))) return rc;
    P.wave_stats = slot.d_wave_stats;
    s->last_wave_stats_waves = (int64_t)lw;
  }
  if (plan.pipeline_buffers) {
    if (sc > 1) { set_error("rt_render: the FULL stage-pipeline variant renders whole frames only"); return RT_ERR_UNSUPPORTED; }
    // sized by the 16x16-padded frame: every wave of the tile grid has a count slot
    if ((rc = ensure_full(slot, (size_t)P.tiles_x * 16 * (size_t)P.tiles_y * 16))) return rc;
    bind_full(slot, P);
  }
  P.xcd_remap = plan.xcd_remap;
  if (plan.rotate_bands) P.xcd_rot = (int32_t)(s->band_rot++ & 7u);  // frames in flight: a large scene's XCD bands rotate
  if (plan.needs_variants && !variants_linked()) {
    set_error("rt_render: kernel variant %d is an A/B build option, not in this library (make variants)", in.variant);
    return RT_ERR_UNSUPPORTED;
  }
  bool lpt_sort = false, lpt_dilated = false;
  if (plan.lpt && (rc = lpt_begin(s, plan, cam, st, P, lpt_sort, lpt_dilated))) return rc;
  if (s->ev_used + 3 > s->ev_pool.size()) {  // (init_slots creates kEventFrames frames' worth up front)
    if (s->ev_pool.size() >= 3 * 2048) { set_error("more than 2048 renders without rt_synchronize"); return RT_ERR_INVALID; }
    for (int k = 0; k < 3; k++) {
      hipEvent_t e;
      HIPCHECK(hipEventCreate(&e));
      s->ev_pool.push_back(e);
    }
  }
  // three events per frame: start | after the traversal kernel | after the frame
  hipEvent_t* ev = (hipEvent_t*)&s->ev_pool[s->ev_used];
  s->ev_used += 3;
  HIPCHECK(hipEventRecord(ev[0], st));
  if ((rc = launch_frame(plan, s, slot, P, st, ev[1]))) return rc;
  if (lpt_sort && (rc = lpt_end(s, plan, st, lpt_dilated))) return rc;
  HIPCHECK(hipEventRecord(ev[2], st));
  slot.last_done = ev[2];
  note_frame(s, slot_id, fr, P);
  return RT_OK;
}

// RT_CHECK_PREFETCH debug build: an out-of-range scalar prefetch offset recorded by the kernels fails the call
int rt::check_prefetch_word(rt_scene* s) {
#ifdef RT_CHECK_PREFETCH
  uint32_t w = 0;
  HIPCHECK(hipMemcpy(&w, s->d_pf_check, 4, hipMemcpyDeviceToHost));
  if (w) {
    set_error("RT_CHECK_PREFETCH: out-of-range scalar load offset (sites 0x%x: 0 node, 1/2 child prefetch, 3 leaf "
              "prefetch, 4 wide prefetch, 5 wide node)", w);
    return RT_ERR_HIP;
  }
#endif
  (void)s;
  return RT_OK;
}

int rt::sync_one(rt_scene* s, rt_stats* out) {
  int rc = check_device_scene(s);
  if (rc) return rc;
  // every slot's stream drained. (Round 6 tried waiting for each slot's frame-done event only, so that a lone
  // frame's trailing sort could overlap the caller's turn: the same frames with 4 in flight then ran 4-25% slower
  // from one process to the next -- C2 29.8-35.0 against 37.6-38.5 Grays/s, profiles/ab/r06_sync_ab.txt.)
  if ((rc = drain_slots(s)) || (rc = check_prefetch_word(s))) return rc;
  struct Reset {
    rt_scene* s;
    ~Reset() {
      s->ev_used = 0;
      s->pending = false;
      for (int k = 0; k < s->n_slots; k++) s->slots[k].last_done = nullptr;
    }
  } reset_{s};
  if (out) {
    memset(out, 0, sizeof *out);
    double tot = 0.0, trav = 0.0;
    for (size_t k = 0; k + 3 <= s->ev_used; k += 3) {
      float ms = 0.0f, ms1 = 0.0f;
      HIPCHECK(hipEventElapsedTime(&ms, (hipEvent_t)s->ev_pool[k], (hipEvent_t)s->ev_pool[k + 2]));
      HIPCHECK(hipEventElapsedTime(&ms1, (hipEvent_t)s->ev_pool[k], (hipEvent_t)s->ev_pool[k + 1]));
      tot += ms;
      trav += ms1;
    }
    out->kernel_ms = tot;
    out->trace_kernel_ms = trav;
    out->launches = (int64_t)(s->ev_used / 3);
    out->primary_rays = s->last_rays;
    out->total_rays = s->last_rays;
    if (s->last_flags & RT_FRAME_STATS) {
      unsigned long long c[kStatSlots];
      HIPCHECK(hipMemcpy(c, s->d_stats, sizeof c, hipMemcpyDeviceToHost));
      out->node_visits = (int64_t)c[ST_NODE];
      out->tri_tests = (int64_t)c[ST_TRI];
      out->wave_node_fetches = (int64_t)(c[ST_WNODE] + c[ST_WWIDE]);
      out->wave_node_bytes = (int64_t)(64 * c[ST_WNODE] + sizeof(Node128) * c[ST_WWIDE]);
      out->wave_tri_fetches = (int64_t)c[ST_WTRI];
      out->hits = (int64_t)c[ST_HITS];
      out->total_rays = (int64_t)c[ST_TOTAL];
    }
  }
  return RT_OK;
}

// the synchronous half of rt_render / rt_render_lit: waits for the frame just queued and copies it to out_rgb
static int finish_render(rt_scene* s, const rt_frame* fr, float* out_rgb, rt_stats* stats) {
  int rc;
  const int W = fr->width, H = fr->height;
  if (!s->replicas.empty() && out_rgb) {
    // multi-device: each device's tile packing and copy are queued right behind its share of the frame, and
    // its host worker writes its tiles into the caller's frame as soon as that device is done (the rest of
    // the frame untouched); the stats are collected after
    if ((rc = assemble(s, ASM_RGB, (int64_t)W * H, out_rgb, nullptr, "rt_render"))) {
      (void)rt_synchronize(s, nullptr);
      return rc;
    }
    return rt_synchronize(s, stats);
  }
  if ((rc = rt_synchronize(s, stats))) return rc;
  if (!out_rgb) return RT_OK;
  const int sc = fr->shard_count > 0 ? fr->shard_count : 1;
  if (sc == 1) return rt_frame_download(s, (int64_t)W * H, out_rgb, nullptr, nullptr);
  std::vector<float> full((size_t)W * H * 3);
  if ((rc = rt_frame_download(s, (int64_t)W * H, full.data(), nullptr, nullptr))) return rc;
  for_each_shard_tile(shard_layout(W, H, fr->shard_index, sc, 12), [&](int, int tx, int ty) {
    for (int y = ty * 16; y < std::min(H, ty * 16 + 16); y++) {
      const size_t o = ((size_t)y * W + tx * 16) * 3;
      memcpy(out_rgb + o, full.data() + o, sizeof(float) * 3 * (size_t)(std::min(W, tx * 16 + 16) - tx * 16));
    }
  });
  return RT_OK;
}

extern "C" int rt_render_lit(rt_scene* s, const rt_camera* cam, const rt_light_set* ls, const rt_frame* fr, float* out_rgb,
                             rt_stats* stats) {
  int rc = rt_render_lit_async(s, cam, ls, fr);
  if (rc) return rc;
  return finish_render(s, fr, out_rgb, stats);
}

extern "C" int rt_render(rt_scene* s, const rt_camera* cam, const rt_light* lights, int32_t n_lights, const rt_frame* fr,
                         float* out_rgb, rt_stats* stats) {
  int rc = rt_render_async(s, cam, lights, n_lights, fr);
  if (rc) return rc;
  return finish_render(s, fr, out_rgb, stats);
}
