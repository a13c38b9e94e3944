#!/usr/bin/env python3
"""Benchmark of the MI355X ray-traversal hot path (BASELINE.json metric).

Metric: "Mrays/s (primary) + frame ms at 1920x1080, 1M-tri BVH, 1/2/4/8 GPU".
Workloads: 1,000,000 random triangles (SplitMix64 seed 12345), Flycamera eye (0,0,1)
(translate(0,0,20)), fovy 60, one white light at (-0.5,2,3), PRIMARY mode (closest hit + unshadowed
Phong). A step = one frame: one launch of the render kernel over this rank's 16x16 tiles. Scene and
frame buffer are resident in HBM before the timed region; no host copies inside it.
  N = 1: C3, the 1920x1080 frame on one GPU.
  N > 1: C4, the 3840x2160 frame split over the N ranks (strong scaling: the frame is fixed; 16x16 tiles
         interleaved over ranks, scene replicated, no collective on the data path -- barrier + MAX/SUM of
         the timing only). The line also carries the 1080p frame split the same way ("c3_frame").
  --frame WxH overrides the frame.

A plain run (`bench.py --gpus N --steps K --warmup W`) does only what the headline figure needs: scene setup,
the prewarm and warmup frames, the K timed frames, the outputs of --dump-outputs, and the result line (`value`,
`ms_per_step`, the configuration). Everything else below -- the cold rate, the lone-frame kernel time, the second
frame size, the C2 / C5 side lines, the moving camera, the roofline, the parity checks, the end-to-end frame and
the CPU baseline -- runs only with --full (where the --no-* options still drop single legs).
  --dump-outputs DIR: after the timed frames, the frame a caller of the timed path receives from its last step
            (rt_frame_download of the last timed frame: float32 rgb [H, W, 3]) as DIR/rgb.npy; a frame over
            64 MB as a fixed seeded sample of its pixels (DIR/rgb.npy [n, 3] + DIR/rgb_pixel_index.npy). Scene
            (seed 12345), camera and lights are fixed, so two builds can be compared output for output.

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, steps, ms_per_step (milliseconds per
timed step), the configuration and the build's identity; with --full also:
  roofline: HBM roofline of the dominant kernel (k_primary_fused). achieved = the packet algorithm's bytes
            per launch (64-B node record per wave per visited node, 64-B triangle record per wave per
            tested triangle -- the counting run's wave fetch counts -- plus per hit lane the 64-B hit
            triangle record and the 48-B shading record, plus the 12-B pixel) / the kernel's launch
            duration measured with HIP events with one frame on the GPU; traffic = measured HBM bytes per
            launch (rocprofv3 FETCH_SIZE/WRITE_SIZE, profiles/pmc_latest.json, only when that profile was
            taken of this same build and workload) over the same duration; "limiter" and "issue": what
            actually bounds the kernel per the same profile's SQ counters (VALU / SALU issue fractions at
            the measured clock, wave cycles spent waiting).
  cpu_baseline: the CPU restatement of the reference algorithm (oracle/, "port") on a bounded pixel
            sample of the same frame on this host's CPU share, with the parity of those pixels against
            the GPU frame and the calibration of the port against the reference's own measured rate.
"""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "ray-tracing-project_amd")
HBM_PEAK_GBPS = 8000.0          # MI355X HBM3E (MI355X_MICROARCH.md)
N_CU, SIMD_PER_CU = 256, 4


def load_rtamd():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rtamd", os.path.join(PKG, "rtamd.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def frame_for(n_gpus, override):
    if override:
        w, h = override.lower().split("x")
        return int(w), int(h)
    return (1920, 1080) if n_gpus == 1 else (3840, 2160)


SHARD_SUPER_TILE = 4  # rt_internal.h kShardSuperTile
MAX_FRAME_SLOTS = 4   # rt_scene.h rt_scene::kMaxSlots: frames a device runs at once (one stream per slot)


def shard_tiles(W, H, rank, n):
    """16x16 tiles this rank renders, in its slot order (rt_api.h rt_frame.shard_index: with n > 1 the
    tiles are grouped into 4x4 super-tiles, super-tile s going to rank s % n; rt_frame_shard_tiles)."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    S = SHARD_SUPER_TILE if n > 1 else 1
    sxn = (tx + S - 1) // S
    ns = sxn * ((ty + S - 1) // S)
    out = []
    for s in range(rank, ns, n):
        for k in range(S * S):
            x, y = (s % sxn) * S + k % S, (s // sxn) * S + k // S
            if x < tx and y < ty:
                out.append((x, y))
    return out


def cpu_threads():
    """The CPU share this process may use: the GPU box exports OMP_NUM_THREADS=16 per GPU (its machine has
    far more cores, shared with other jobs); elsewhere every core in the affinity mask."""
    avail = len(os.sched_getaffinity(0))
    share = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    return (min(avail, share) if share > 0 else avail), avail


def cpu_model():
    try:
        for line in subprocess.run(["lscpu"], capture_output=True, text=True).stdout.splitlines():
            if line.startswith("Model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(scene, soup_args, W, H, full, target_s, threads, avail, gpu_frame):
    """Oracle ("port" of the reference algorithm) on a strided pixel sample of the same frame, and the
    parity of those pixels against the GPU frame (rgb, face, t of the same camera)."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle as O
    t0 = time.perf_counter()
    if scene == "soup":
        n_tris, seed, mat = soup_args
        v = O.generate_soup(n_tris, seed)
        f = np.arange(3 * n_tris, dtype=np.uint32).reshape(-1, 3)
        sc = O.Scene(O.Mesh.from_arrays(v, f, np.array([mat], np.float32)))
        what = f"{n_tris}-tri soup"
    else:
        sc = O.Scene(O.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj")))
        what = "bunny"
    build_s = time.perf_counter() - t0
    cam = O.flycam(W, H, 0, 0, 20)

    def run(k):  # every k-th pixel of the frame in row-major order (a deterministic, spread sample)
        idx = np.arange(k // 2, W * H, k, dtype=np.int64)
        pix = np.stack([idx % W, idx // W], axis=1).astype(np.int32)
        t = time.perf_counter()
        out = sc.render(cam, O.DEFAULT_LIGHTS, W, H, full=full, pixels=pix, threads=threads)
        return idx, out, time.perf_counter() - t

    idx, out, dt = run(509)  # calibration sample (~4k rays)
    k = 509
    for _ in range(3):
        rate = len(idx) / max(dt, 1e-6)
        k = max(1, math.ceil(W * H / max(rate * target_s, 1.0)))
        idx, out, dt = run(k)
        if dt > 0.6 * target_s or k == 1:
            break
    n = len(idx)
    res = {"value": round(n / dt / 1e6, 6), "unit": "Mrays/s", "cores": threads, "kind": "port",
           "sample": f"{n} primary rays = every {k}th pixel (row-major) of the same {W}x{H} frame "
                     f"({what}, eye (0,0,1), {'FULL' if full else 'PRIMARY'}); {dt:.1f} s of CPU work on "
                     f"{threads} threads; box partition build {build_s:.1f} s excluded",
           "cores_available": avail, "model": cpu_model(),
           "rays_per_s_per_thread": round(n / dt / threads, 1)}
    calib = os.path.join(ROOT, "profiles", "cpu_calibration.json")
    if os.path.exists(calib):
        c = json.load(open(calib))
        res["calibration"] = {
            "port_over_reference": c["port_over_reference"],
            "how": f"port {c['port_rays_per_s_per_thread']} vs the unmodified reference's "
                   f"{c['reference_rays_per_s_per_core']} primary rays/s per core, same scene / camera / 32x18 "
                   f"sample, one thread, both in the survey's container ({c['host']}): profiles/cpu_calibration.json",
            "reference_equivalent_mrays_per_s": round(n / dt / 1e6 / c["port_over_reference"], 6)}
    if gpu_frame is not None:
        grgb, gface, gt = gpu_frame
        orgb, oface, ot = out
        gr = grgb.reshape(-1, 3)[idx]
        err = np.abs(gr.astype(np.float64) - orgb.astype(np.float64))
        err = np.where(np.isnan(gr) & np.isnan(orgb), 0.0, err)
        res["parity"] = {"pixels": n, "face_mismatch": int((gface.reshape(-1)[idx] != oface).sum()),
                         "t_mismatch": int((gt.reshape(-1)[idx].view(np.uint32) != ot.view(np.uint32)).sum()),
                         "linf": float(np.nanmax(err)) if err.size else 0.0,
                         "what": "the oracle's sampled pixels vs the same pixels of the GPU frame (face id and t "
                                 "bits, colour L_inf)"}
    return res


def e2e_frame_ms(rt, sc, cam, W, H, mode, rank, n, dist, iters=5):
    """End-to-end frame with the output path: render this rank's tiles, pack them as 8-bit,
    gather every rank's slice on rank 0 (RCCL all-gather over xGMI; gloo via host when rehearsing), unpack
    there and copy the 8-bit frame to the host. Not the bench value: the PCIe-inclusive latency."""
    import torch
    slice_b = rt.shard_bytes(W, H, n)
    on_gpu = dist is None or backend_is_nccl(dist)
    slc = torch.empty(slice_b, dtype=torch.uint8, device="cuda")
    gathered = torch.empty(n * slice_b, dtype=torch.uint8, device="cuda" if on_gpu else "cpu")
    frame = torch.empty(W * H * 3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ts, ta = [], []
    for _ in range(iters + 1):
        if dist is not None:
            dist.barrier()
        t = time.perf_counter()
        sc.render_async(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=(rank, n))
        sc.synchronize()
        t_a = time.perf_counter()
        if n == 1 or dist is None:  # (an in-process multi-device scene assembles its frame itself: rt_frame_download_rgb8)
            host, _ = sc.download_rgb8(W, H)
        else:
            sc.pack_shard_rgb8(slc.data_ptr())
            if on_gpu:
                dist.all_gather_into_tensor(gathered, slc)
            else:
                dist.all_gather_into_tensor(gathered, slc.cpu())
            if rank == 0:
                src = gathered if on_gpu else gathered.cuda()
                torch.cuda.synchronize()
                rt.unpack_shards_rgb8(src.data_ptr(), n, W, H, frame.data_ptr(), torch.cuda.current_device())
                host = frame.cpu()
        ts.append((time.perf_counter() - t) * 1e3)
        ta.append((time.perf_counter() - t_a) * 1e3)
    med = lambda v: sorted(v[1:])[len(v[1:]) // 2]
    return med(ts), med(ta)


def backend_is_nccl(dist):
    return dist is not None and dist.get_backend() == "nccl"


def make_reducer(dist, dev):
    import torch

    def reduce(x, op):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=getattr(dist.ReduceOp, op))
        return float(t.item())
    return reduce


def gather_all(dist, dev, x):
    """Every rank's value of x, in rank order (timing metadata only)."""
    import torch
    if dist is None:
        return [x]
    t = torch.tensor([x], dtype=torch.float64, device=dev)
    out = torch.zeros(dist.get_world_size(), dtype=torch.float64, device=dev)
    dist.all_gather_into_tensor(out, t)
    return [float(v) for v in out.tolist()]


def same_build_profile(W, H, n_faces, mode, kernel, src_hash, latest="pmc_latest.json"):
    """The committed rocprofv3 summary (profiles/pmc_latest.json for the headline workload,
    profiles/pmc_latest_c5.json for C5; tools/profile.sh + tools/summarize_profile.py) when it was taken of
    this build (embedded source hash), this kernel and this workload, one frame on the GPU at a time; else
    None."""
    p = os.path.join(ROOT, "profiles", latest)
    if not os.path.exists(p):
        return None, f"no profiles/{latest}"
    d = json.load(open(p))
    bl = d.get("bench_line_under_trace", {})
    cfg = bl.get("config", {})
    why = []
    if cfg.get("frame") != f"{W}x{H}" or cfg.get("triangles") != n_faces or cfg.get("mode") != mode:
        why.append("other workload")
    if not str(d.get("kernel", "")).startswith(kernel + "<"):
        why.append("other kernel")
    if bl.get("build", {}).get("source_hash") != src_hash:
        why.append(f"other build ({bl.get('build', {}).get('source_hash')} vs {src_hash})")
    if why:
        return None, f"profiles/{latest} ({d.get('tag')}): " + ", ".join(why)
    return d, f"profiles/{d.get('tag')}_pmc.json"


def shared_scene(build, load, rank, barrier, path):
    """Rank 0 builds the scene and writes it to `path` (f1 scene cache); after a barrier every other rank
    loads it; rank 0 removes the file once all have. Returns (scene, seconds): rank 0's build + save time,
    the other ranks' load + upload time."""
    t0 = time.perf_counter()
    sc = None
    if rank == 0:
        sc = build()
        sc.save(path)
    setup_s = time.perf_counter() - t0
    barrier()
    if rank != 0:
        t1 = time.perf_counter()
        sc = load(path)
        setup_s = time.perf_counter() - t1
    barrier()
    if rank == 0:
        os.remove(path)
    return sc, setup_s


def kernel_bound(kernel, latest=None):
    """The limiter of `kernel`: from the workload's own committed profile (profiles/<latest>, e.g.
    pmc_latest_c2.json for the C2 sub-line) when that profile is of this kernel, else from the newest
    committed rocprofv3 summary of the kernel (profiles/*_pmc.json, by tag order): "latency", "hbm", "valu"
    or "salu" from its `limiter` text."""
    import glob
    if latest:
        try:
            d = json.load(open(os.path.join(ROOT, "profiles", latest)))
            if str(d.get("kernel", "")).startswith(kernel + "<") and d.get("limiter"):
                lim = str(d["limiter"]).split(":")[0].strip().lower()
                return lim, f"profiles/{d.get('tag')}_pmc.json: {d['limiter']}"
        except (OSError, ValueError):
            pass
    best = None
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json"))):
        try:
            d = json.load(open(p))
        except (OSError, ValueError):
            continue
        if not str(d.get("kernel", "")).startswith(kernel + "<") or not d.get("limiter"):
            continue
        if best is None or str(d.get("tag", "")) >= str(best[1].get("tag", "")):
            best = (p, d)
    if best is None:
        return None, "no committed profile of " + kernel
    lim = str(best[1]["limiter"]).split(":")[0].strip().lower()
    return lim, f"profiles/{os.path.basename(best[0])}: {best[1]['limiter']}"


DIGESTS = os.path.join(ROOT, "tests", "golden", "fullframe_digests.json")
SAMPLES = os.path.join(ROOT, "tests", "golden", "fullframe_samples.npz")


def frame_parity(rt, sc, W, H, mode, case, cam=None):
    """Parity of the frame this bench times, outside the timed region: one render of the
    same camera with hit records, its per-pixel face ids and t bits hashed (SHA-256) against the oracle's
    committed full-frame digests (tests/golden/fullframe_digests.json, tools/gen_fullframe_digests.py), and
    its colours against the committed strided oracle sample (every 257th pixel). No oracle run needed."""
    import hashlib
    dig = json.load(open(DIGESTS)).get(case)
    if dig is None or (dig["W"], dig["H"]) != (W, H) or dig["mode"] != ("full" if mode == rt.RT_MODE_FULL else "primary"):
        return {"case": case, "face_t_digest_equal": None, "why": "no committed digest of this frame"}
    if cam is None:
        cam = rt.flycam(W, H, 0, 0, 20)
    rgb, face, t, _ = sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True)
    sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
    face_ok, t_ok = sha(face) == dig["face_sha256"], sha(t) == dig["t_sha256"]
    out = {"case": case, "pixels": W * H, "face_t_digest_equal": bool(face_ok and t_ok),
           "face_digest_equal": bool(face_ok), "t_digest_equal": bool(t_ok),
           "hits": int((np.asarray(face) >= 0).sum()), "oracle_hits": dig["hits"]}
    smp = np.load(SAMPLES)
    if case + "_idx" in smp:
        idx = smp[case + "_idx"]
        a = np.asarray(rgb, np.float64).reshape(-1, 3)[idx]
        b = smp[case + "_rgb"].astype(np.float64)
        err = np.where(np.isnan(a) & np.isnan(b), 0.0, np.abs(a - b))
        out["colour_linf_sampled"] = float(np.nanmax(err)) if err.size else 0.0
        out["colour_sample_pixels"] = int(len(idx))
    out["what"] = ("face ids + t bits of every pixel: SHA-256 against the oracle's committed digests; colour L_inf "
                   "against the committed oracle sample")
    return out


def algorithmic_bytes(stats):
    """The packet algorithm's bytes per launch from a counting run's stats: node / triangle records once per
    wave, the hit lanes' triangle + shading records, the pixel (module docstring)."""
    wave_bytes = float(stats["wave_node_bytes"]) + 64.0 * stats["wave_tri_fetches"]
    return wave_bytes + stats["hits"] * (64 + 48) + 12.0 * max(stats["primary_rays"], 1)


def roofline_of(rt, sc, cam, W, H, mode, kern_ms, ms_per_step, n_faces, src_hash, mode_name, latest, split=False,
                shard=(0, 1), prefer_trace=False):
    """The dominant kernel's packet-byte roofline for one workload (see the module docstring): a counting run
    of the same frame for the bytes, the isolated launch duration kern_ms (HIP events on the library's stream
    around the kernel), the same build's profile (if committed) for the measured HBM traffic and the limiter.
    prefer_trace (the C2 / C5 sub-lines): when that profile matches this build and workload,
    the duration is its rocprofv3 kernel-trace average -- a short kernel's HIP-event interval also holds the
    dispatch gap (C2: 87 vs 75 us) -- and both durations are reported."""
    sc.render_async(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard, flags=rt.RT_FRAME_STATS)
    stats = sc.synchronize()
    rays = max(stats["primary_rays"], 1)
    n_node = stats["node_visits"] / rays
    n_tri = stats["tri_tests"] / rays
    hit = stats["hits"] / rays
    kname = ("k_trace_primary" if split else "k_primary_fused") if mode == rt.RT_MODE_PRIMARY else "k_render_full"
    alg_bytes = algorithmic_bytes(stats)
    prof, prof_src = same_build_profile(W, H, n_faces, mode_name, kname, src_hash, latest)
    trace_ms = (prof.get("avg_kernel_ns_trace") or 0) / 1e6 if prof is not None else 0.0
    hip_ms = kern_ms
    basis = "hip_events"
    if prefer_trace and trace_ms > 0:
        kern_ms, basis = trace_ms, "rocprofv3_trace_average"
    achieved = alg_bytes / (kern_ms * 1e-3) / 1e9
    traffic = traffic_b = issue = limiter = None
    if prof is not None:
        traffic_b = prof.get("hbm_bytes_per_launch")
        if traffic_b:
            traffic = round(traffic_b / (kern_ms * 1e-3) / 1e9, 1)
        issue = prof.get("issue")
        limiter = prof.get("limiter")
    # what bounds the kernel, as the newest committed profile of it measured: the
    # roofline below is still priced against HBM bandwidth, the resource north_star names
    bound, bound_src = kernel_bound(kname, latest)
    roof = {"bound": bound, "bound_source": bound_src, "priced_against": "hbm",
            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
            "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
            "traffic_bytes_per_launch": traffic_b, "traffic_source": prof_src,
            "kernel": kname, "kernel_ms_isolated": round(kern_ms, 4), "kernel_ms_basis": basis,
            "kernel_ms_hip_events": round(hip_ms, 4), "kernel_ms_trace": round(trace_ms, 4) if trace_ms else None,
            "algorithmic_bytes_per_launch": int(alg_bytes),
            "algorithmic_bytes_per_ray": round(alg_bytes / rays, 1),
            "per_step_GBps": round(alg_bytes / (ms_per_step * 1e-3) / 1e9, 1),
            # the same bytes over the throughput interval (frames in flight overlap, so this is the GPU's
            # sustained rate; `frac` above prices one launch alone)
            "frac_per_step": round(alg_bytes / (ms_per_step * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
            "limiter": limiter, "issue": issue,
            # SURVEY 8(d) d3's per-ray demand (every node / triangle a ray visits, as if each ray read
            # its own records): served from SGPRs / L2 / MALL, not HBM -- reported, not priced
            "survey_demand_bytes_per_ray": round(64 * n_node + 40 * n_tri + 92 * hit + 12, 1),
            "n_node": round(n_node, 2), "n_tri": round(n_tri, 2), "hit": round(hit, 4)}
    return roof, stats


def side_config(rt, scene_name, mode, steps, warmup, device, src_hash=None, prewarm_ms=0.0, moving=False):
    """A single-GPU BASELINE config beside the headline one: C2 = bunny PRIMARY,
    C5 = bunny FULL, 1920x1080: rate with frames in flight and one frame at a time."""
    import torch
    W, H = 1920, 1080
    mesh = rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj"))
    m = rt.RT_MODE_FULL if mode == "full" else rt.RT_MODE_PRIMARY
    cam = rt.flycam(W, H, 0, 0, 20)
    out = {"workload": f"{scene_name}: Stanford bunny (69,451 triangles), {W}x{H} {mode}, eye (0,0,1), 1 light"}
    for fif in (4, 1):
        sc = rt.Scene(mesh, device=device, frames_in_flight=fif)
        el, st = timed_frames(rt, sc, cam, W, H, m, (0, 1), steps, warmup, lambda: None,
                              lambda: torch.cuda.synchronize(device), prewarm_ms)
        key = "" if fif == 4 else "_one_frame_at_a_time"
        out["mrays_per_s" + key] = round(st["primary_rays"] * steps / el / 1e6, 2)
        out["ms_per_frame" + key] = round(el / steps * 1e3, 4)
        if fif == 4:
            # the frame's kernel alone on the GPU (HIP events around the render kernel, 20 frames each
            # synchronised before the next; the dispatch-order sort after a frame is not counted)
            _, iso = isolated_kernel_ms(rt, sc, cam, W, H, m, (0, 1))
            roof, s2 = roofline_of(rt, sc, cam, W, H, m, iso, el / steps * 1e3, sc.info()["n_faces"], src_hash, mode,
                                   "pmc_latest_c5.json" if mode == "full" else "pmc_latest_c2.json", prefer_trace=True)
            out["kernel_ms_isolated"] = roof["kernel_ms_isolated"]
            out["roofline"] = roof
            out["limiter"] = roof["limiter"]
            out["total_mrays_per_s"] = round(s2["total_rays"] * steps / el / 1e6, 2)
            out["parity"] = frame_parity(rt, sc, W, H, m, scene_name)
            if moving:
                out["moving_camera"] = moving_camera(
                    rt, lambda f: rt.Scene(mesh, device=device, frames_in_flight=f), sc, W, H, m, scene_name, steps,
                    warmup, lambda: torch.cuda.synchronize(device), prewarm_ms)
        del sc
    return out


MOVE_POSE = 37  # the pose (frames along rtamd.CameraPath) whose oracle digest is committed ("<case>-moving")


def moving_camera(rt, make_scene, sc4, W, H, mode, case, steps, warmup, sync_device, prewarm_ms):
    """The workload under the reference's moving camera: every frame a new Flycamera pose
    (rtamd.CameraPath: WASD held, 0.01 units per axis per frame, flyscene.cpp:116-127, flycamera.hpp:196-202),
    beside the same measurements with the fixed camera. sc4: the bench's scene (4 frames in flight);
    make_scene(fif): a new scene of the same workload. Reports the rate with frames in flight, one frame at a time
    (where the longest-first order comes from an earlier frame's wave costs), the first frame of a fresh scene (no
    cost map), one frame alone with the default order (no cost map at all, variant 131072), and the roofline of
    one frame alone under motion."""
    static = rt.flycam(W, H, 0, 0, 20)
    out = {"path": "rtamd.CameraPath: Flyscene::simulate with W/S and D/A held (translate(+-0.2, 0, +-0.2) x speed "
                   "0.05 per frame, turning every 40 / 25 frames), from eye (0,0,1); a new pose every frame"}
    el, st = timed_frames(rt, sc4, None, W, H, mode, (0, 1), steps, warmup, lambda: None, sync_device, prewarm_ms,
                          path=rt.CameraPath(W, H))
    out["mrays_per_s"] = round(st["primary_rays"] * steps / el / 1e6, 2)
    out["ms_per_frame"] = round(el / steps * 1e3, 4)
    sc1 = make_scene(1)
    path = rt.CameraPath(W, H)
    sc1.render_async(path.next(), rt.DEFAULT_LIGHTS, W, H, mode=mode)  # a fresh scene's first frame: no cost map
    first = sc1.synchronize()
    out["first_frame_kernel_ms"] = round(first["trace_kernel_ms"], 4)
    for key, pth, cam in (("_static", None, static), ("", path, None)):
        el1, st1 = timed_frames(rt, sc1, cam, W, H, mode, (0, 1), steps, warmup, lambda: None, sync_device, prewarm_ms,
                                path=pth)
        out["mrays_per_s_one_frame_at_a_time" + key] = round(st1["primary_rays"] * steps / el1 / 1e6, 2)
    # one frame alone (HIP events around the render kernel, 20 frames each synchronised before the next)
    lpt0 = sc1.lpt_stats()
    iso_m = isolated_kernel_ms(rt, sc1, None, W, H, mode, (0, 1), path=path)
    lpt1 = sc1.lpt_stats()
    iso_s = isolated_kernel_ms(rt, sc1, static, W, H, mode, (0, 1))
    prev = rt.set_variant(131072)  # the default chunked-XCD order: no cost map
    try:
        iso_n = isolated_kernel_ms(rt, sc1, None, W, H, mode, (0, 1), path=path)
    finally:
        rt.set_variant(prev)
    out["kernel_ms_isolated"] = round(iso_m[1], 4)
    out["kernel_ms_isolated_static"] = round(iso_s[1], 4)
    out["kernel_ms_isolated_no_cost_map"] = round(iso_n[1], 4)
    out["frame_ms_isolated_incl_sort"] = round(iso_m[0], 4)
    out["lpt_resorts"] = f"{lpt1['sorts'] - lpt0['sorts']} of {lpt1['frames'] - lpt0['frames']} lone moving frames"
    # the packet bytes of one frame, averaged over four poses of the path (counting runs), over the kernel time
    pb = rt.CameraPath(W, H)
    ab = []
    for k in range(4):
        for _ in range(12 if k else 0):
            pb.next()
        sc1.render_async(pb.next(), rt.DEFAULT_LIGHTS, W, H, mode=mode, flags=rt.RT_FRAME_STATS)
        ab.append(algorithmic_bytes(sc1.synchronize()))
    sc1.render_async(static, rt.DEFAULT_LIGHTS, W, H, mode=mode, flags=rt.RT_FRAME_STATS)
    ab_s = algorithmic_bytes(sc1.synchronize())
    ab_m = float(np.mean(ab))
    out["roofline"] = {"algorithmic_bytes_per_launch": int(ab_m), "unit": "GB/s", "peak": HBM_PEAK_GBPS,
                       "achieved": round(ab_m / (iso_m[1] * 1e-3) / 1e9, 1),
                       "frac": round(ab_m / (iso_m[1] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "frac_static": round(ab_s / (iso_s[1] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "frac_no_cost_map": round(ab_m / (iso_n[1] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4),
                       "kernel_ms_basis": "hip_events (ev_a -> ev_m: the render kernel of a lone frame)"}
    cp = rt.CameraPath(W, H)
    cp.take(MOVE_POSE)
    out["parity"] = frame_parity(rt, sc1, W, H, mode, case + "-moving", cam=cp.camera())
    del sc1
    return out


DUMP_CAP_BYTES = 64 * 1000 * 1000  # --dump-outputs: all files of a run together stay under this
DUMP_SEED = 12345


def dump_arrays(out_dir, arrays, cap=DUMP_CAP_BYTES, suffix=""):
    """--dump-outputs: each array of `arrays` ({name: per-pixel array [H, W, c] or [H, W]}) as
    <out_dir>/<name><suffix>.npy in float32 (float64 stays float64). When the arrays together exceed `cap` bytes,
    each is cut to the same fixed sample of its pixels -- the sorted first n of a seeded permutation (DUMP_SEED),
    so every run and every build samples the same pixels -- and the pixels' row-major indices go to
    <out_dir>/<name>_pixel_index<suffix>.npy (float64, exact). Returns {file name: shape}."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.asarray(v, np.float64 if np.asarray(v).dtype == np.float64 else np.float32)
              for k, v in arrays.items()}
    written = {}
    share = cap // max(len(arrays), 1)
    for name, a in arrays.items():
        if a.nbytes > share:
            px = a.reshape(a.shape[0] * a.shape[1], -1)
            n = share // (px.shape[1] * a.itemsize + 8)  # a pixel's values + its float64 index
            idx = np.sort(np.random.default_rng(DUMP_SEED).permutation(len(px))[:n])
            a = np.ascontiguousarray(px[idx])
            np.save(os.path.join(out_dir, f"{name}_pixel_index{suffix}.npy"), idx.astype(np.float64))
            written[f"{name}_pixel_index{suffix}.npy"] = [len(idx)]
        np.save(os.path.join(out_dir, f"{name}{suffix}.npy"), a)
        written[f"{name}{suffix}.npy"] = list(a.shape)
    return written


def enqueue_cost_ms(rt, sc, cams, W, H, mode, shard):
    """Host cost of queueing one frame (rt_render_async through the Python binding), frames not waited on."""
    t1 = time.perf_counter()
    for c in cams:
        sc.render_async(c, rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard)
    ms = (time.perf_counter() - t1) / len(cams) * 1e3
    sc.synchronize()
    return ms


MAX_PENDING_FRAMES = 2048  # rt_render_async refuses more renders than this between two rt_synchronize calls


def merge_stats(a, b):
    """(totals, [per device]) of two consecutive rt_synchronize_devices read-outs as one: kernel times and launch
    counts add up, everything else (the rays of a frame, a counting run's counters) is the later read-out's."""
    if a is None:
        return b
    def add(x, y):
        out = dict(y)
        for key in ("kernel_ms", "trace_kernel_ms", "launches"):
            if key in x or key in y:
                out[key] = x.get(key, 0) + y.get(key, 0)
        return out
    return add(a[0], b[0]), [add(x, y) for x, y in zip(a[1], b[1])]


def timed_frames(rt, sc, cam, W, H, mode, shard, steps, warmup, barrier, sync_device, prewarm_ms=0.0, path=None,
                 enqueue=True):
    """W untimed warmup frames, then EXACTLY `steps` timed frames bracketed by barrier + device synchronisation
    (any number of steps: see MAX_PENDING_FRAMES below).
    enqueue: afterwards also measure the host's cost of queueing a frame (up to 3 more, untimed frames) into
    st["enqueue_ms"]; without it the scene's last frame is the last timed one.
    prewarm_ms: before the warmup frames, frames of the same workload rendered back to back (untimed) for that
    long, so that the timed frames see the GPU in its loaded state rather than just out of idle (a steady-state
    rate; the cold start is in profiles/ab/r05_prewarm_ab.txt); their count is returned as st["prewarm_frames"].
    path (rtamd.CameraPath): every frame -- prewarm, warmup and timed -- takes the path's next pose (the
    reference's camera moving while a key is held) instead of the fixed `cam`; the timed frames' cameras are
    made before the clock starts."""
    nxt = (lambda: path.next()) if path is not None else (lambda: cam)
    t_pw = time.perf_counter()
    n_pw = 0
    while (time.perf_counter() - t_pw) * 1e3 < prewarm_ms:
        for _ in range(4):
            sc.render_async(nxt(), rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard)
        n_pw += 4
        sc.synchronize()
    for k in range(warmup):
        if k and k % MAX_PENDING_FRAMES == 0:
            sc.synchronize()
        sc.render_async(nxt(), rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard)
    sc.synchronize()
    cams = path.take(steps) if path is not None else [cam] * steps
    barrier()
    sync_device()
    done = None
    t0 = time.perf_counter()
    for k, c in enumerate(cams):
        # the library's bound on queued frames: a longer run is drained inside the window after every
        # MAX_PENDING_FRAMES frames (one pipeline drain and that many frames' event read-out, ~1 us each, per
        # MAX_PENDING_FRAMES frames: well under 1% of their time); up to that many steps nothing is added
        if k and k % MAX_PENDING_FRAMES == 0:
            done = merge_stats(done, sc.synchronize_devices())
        sc.render_async(c, rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard)
    # every device of the scene drained (rt_render_async returns once each device's share is queued, so a
    # device synchronise covers every frame); the last frames' event times are read after the clock stops
    # (rt_synchronize_devices: ~1 us of host time per frame, not part of a frame; profiles/ab/r05_sync_readout_ab.txt)
    sync_device()
    barrier()
    el = time.perf_counter() - t0
    st, per = merge_stats(done, sc.synchronize_devices())
    st["per_device"] = per
    # the window holds every timed frame of every device: a frame slot's stream runs its frames one
    # after the other, each frame's HIP-event interval (start event -> end event, both recorded on that stream
    # after the warmup had drained) lies inside the window, so per device the summed frame times cannot exceed
    # slots x window; and every device rendered every timed frame
    slots = MAX_FRAME_SLOTS
    for k, p in enumerate(per or [st]):
        if p["launches"] != steps:
            raise RuntimeError(f"device {k}: {p['launches']} frames timed, {steps} queued")
        if el * 1e3 * slots * 1.001 < p["kernel_ms"]:
            raise RuntimeError(f"device {k}: frames' kernel time {p['kernel_ms']:.3f} ms exceeds {slots} slots x the "
                               f"timed window {el * 1e3:.3f} ms: frames not drained")
    st["prewarm_frames"] = n_pw
    if enqueue:
        more = path.take(min(steps, 3)) if path is not None else [cam] * min(steps, 3)
        st["enqueue_ms"] = enqueue_cost_ms(rt, sc, more, W, H, mode, shard)
    return el, st


def isolated_kernel_ms(rt, sc, cam, W, H, mode, shard, iters=20, path=None):
    """The render kernel's launch duration with one frame on the GPU (each frame synchronised before the
    next is queued): HIP events on the library's stream around each launch, averaged. path: a new camera pose
    every frame (rtamd.CameraPath) instead of `cam`."""
    tot, trav = 0.0, 0.0
    for _ in range(iters):
        sc.render_async(path.next() if path is not None else cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, shard=shard)
        st = sc.synchronize()
        tot += st["kernel_ms"]
        trav += st["trace_kernel_ms"]
    return tot / iters, trav / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tris", type=int, default=1_000_000)
    ap.add_argument("--frame", default=None, help="WxH; default 1920x1080 on 1 GPU (C3), 3840x2160 split over N>1 (C4)")
    ap.add_argument("--mode", choices=["primary", "full"], default="primary")
    ap.add_argument("--scene", default="soup", help="soup | bunny")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beside the headline figure (cold rate, lone-frame kernel "
                         "time, second frame size, C2 / C5, moving camera, roofline, parity against the committed "
                         "oracle digests, end-to-end frame, CPU baseline); the --no-* options drop single legs of it")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the frame of the last timed step (what rt_frame_download hands the caller) as "
                         "DIR/rgb.npy, float32; over 64 MB a fixed seeded sample of its pixels")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-stats", action="store_true")
    ap.add_argument("--no-e2e", action="store_true", help="skip the end-to-end (render + 8-bit frame to host) timing")
    ap.add_argument("--no-extra", action="store_true", help="skip the second frame size (c4_frame / c3_frame)")
    ap.add_argument("--no-side", action="store_true", help="skip the C2 / C5 lines of the N=1 run")
    ap.add_argument("--no-shared-build", action="store_true",
                    help="N > 1: every rank builds the scene itself instead of loading rank 0's scene cache")
    ap.add_argument("--leaf", type=int, default=0, help="BVH leaf size bound (0 = library default)")
    ap.add_argument("--builder", choices=["sbvh", "sah", "lbvh", "ploc", "sahgpu", "sbvhgpu"], default="sbvhgpu",
                    help="BVH builder: SAH with spatial splits on the device (default) or the host, binned SAH on "
                         "the host or the device, or the device LBVH or PLOC (SURVEY f2)")
    ap.add_argument("--boxes", choices=["gpu", "host"], default="gpu",
                    help="reference box partition builder (rt_scene_opts.box_builder; identical boxes either way)")
    ap.add_argument("--wide", action="store_true",
                    help="also build the fp32 4-wide tree and walk it for PRIMARY packets (rt_scene_opts.wide_tree)")
    ap.add_argument("--frames-in-flight", type=int, default=0,
                    help="frames that may overlap on the GPU (0 = library default, 4)")
    ap.add_argument("--rehearse-shards", type=int, default=0,
                    help="one GPU renders only shard 0 of K (the per-GPU work of a K-GPU C4 run, no collective): "
                         "rehearsal of strong scaling; the line reports that shard's rate")
    ap.add_argument("--prewarm-ms", type=float, default=50.0,
                    help="render the workload back to back for this long (untimed) before the warmup steps: the GPU "
                         "leaves its idle state over tens of milliseconds of load, which 5 warmup frames (~1 ms) do not "
                         "cover (C3 at 20 steps: 8.4 Grays/s cold, 9.7 after 30-300 ms; profiles/ab/r05_prewarm_ab.txt); "
                         "0 = off")
    ap.add_argument("--no-cold", action="store_true", help="skip the cold (no prewarm) rate of the headline frames")
    ap.add_argument("--no-moving", action="store_true", help="skip the moving-camera sub-lines (C3, C5)")
    ap.add_argument("--devices", default=None,
                    help="in-process multi-device run (no launcher): the HIP devices of the scene, e.g. 0,1,2,3 "
                         "(default 0..N-1 for --gpus N); repeats allowed to rehearse on one GPU (0,0)")
    a = ap.parse_args()
    if not a.full:  # a plain run: the headline frames only
        a.no_cpu = a.no_stats = a.no_e2e = a.no_extra = a.no_side = a.no_cold = a.no_moving = True

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # rehearsal knob: BENCH_DEVICE pins every rank to one device (several ranks sharing one GPU, with
    # BENCH_BACKEND=gloo for the timing reductions); unset in real runs (one GPU per rank)
    if "BENCH_DEVICE" in os.environ:
        local = int(os.environ["BENCH_DEVICE"])
    if world > 1 and world != a.gpus:
        print(f"error: WORLD_SIZE {world} != --gpus {a.gpus}", file=sys.stderr)
        sys.exit(2)
    # --gpus N without a launcher: the drop-in's own multi-device path -- one process renders every frame on
    # N devices (rt_scene_opts.n_devices / devices: the scene replicated by peer copy, the frame's super-tiles
    # interleaved over the devices, the tiles assembled on the host). It never falls back
    # to fewer GPUs: too few visible devices is an error, not an n_gpus 1 line.
    devices = None
    if world == 1 and (a.gpus > 1 or a.devices):
        devices = [int(x) for x in a.devices.split(",")] if a.devices else list(range(a.gpus))
        if len(devices) != a.gpus:
            print(f"error: --devices lists {len(devices)} devices, --gpus {a.gpus}", file=sys.stderr)
            sys.exit(2)
        import torch
        visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if max(devices) >= visible or min(devices) < 0:
            print(f"error: --gpus {a.gpus} needs devices {devices}, {visible} visible", file=sys.stderr)
            sys.exit(2)
    n = max(world, 1) if devices is None else len(devices)

    import torch
    dist = None
    if world > 1:
        import torch.distributed as dist
        backend = os.environ.get("BENCH_BACKEND") or ("nccl" if torch.cuda.is_available() else "gloo")
        if torch.cuda.is_available():
            torch.cuda.set_device(local)
        dist.init_process_group(backend=backend)
    elif torch.cuda.is_available():
        torch.cuda.set_device(local)
    dev = torch.device("cuda", local) if (torch.cuda.is_available() and backend_is_nccl(dist)) else torch.device("cpu")

    def barrier():
        if dist is not None:
            dist.barrier()

    def sync_device():
        # every device this process renders on (an in-process multi-device scene spans several)
        if torch.cuda.is_available():
            for d in (sorted(set(devices)) if devices else [local]):
                torch.cuda.synchronize(d)

    reduce = make_reducer(dist, dev)

    rt = load_rtamd()
    ident = rt.build_identity()
    K = a.rehearse_shards if (a.rehearse_shards > 1 and n == 1) else 0
    if K:
        a.no_cpu = True
    W, H = frame_for(K or n, a.frame)
    t0 = time.perf_counter()
    if a.scene == "soup":
        scene_name = f"{a.tris} random triangles (SplitMix64 seed 12345)"
    else:
        scene_name = "Stanford bunny (69,451 triangles)"
    builder = {"lbvh": rt.RT_BUILDER_LBVH_GPU, "sah": rt.RT_BUILDER_SAH, "sbvh": rt.RT_BUILDER_SBVH,
               "ploc": rt.RT_BUILDER_PLOC_GPU, "sahgpu": rt.RT_BUILDER_SAH_GPU,
               "sbvhgpu": rt.RT_BUILDER_SBVH_GPU}[a.builder]

    def build_scene():
        if a.scene == "soup":
            mesh, _, _ = rt.soup_mesh(a.tris, 12345)
        else:
            mesh = rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj"))
        return rt.Scene(mesh, device=local, leaf_size=a.leaf, frames_in_flight=a.frames_in_flight, builder=builder,
                        wide_tree=1 if a.wide else 0, box_builder=0 if a.boxes == "host" else 1, devices=devices)

    # N > 1 (one node): the scene is built once -- rank 0 builds it and writes the f1 scene cache
    # (rt_scene_save), the other ranks load it (rt_scene_load: no OBJ parse, no box partition, no BVH
    # build) -- instead of every rank building the same tree on the shared host
    cache_path = None
    if world > 1 and not a.no_shared_build:
        cache_path = os.path.join(os.environ.get("TMPDIR", "/tmp"),
                                  f"rtamd_{a.scene}_{a.tris}_{a.builder}_{a.leaf}_{os.environ.get('MASTER_PORT', '0')}.rtscene")
        sc, setup_s = shared_scene(
            build_scene, lambda p: rt.Scene.load(p, device=local, frames_in_flight=a.frames_in_flight,
                                                 wide_tree=1 if a.wide else 0), rank, barrier, cache_path)
    else:
        sc = build_scene()
        setup_s = time.perf_counter() - t0
    info = sc.info()
    info_fif = a.frames_in_flight or 4
    setup_per_rank = gather_all(dist, dev, setup_s)
    cam = rt.flycam(W, H, 0, 0, 20)
    mode = rt.RT_MODE_FULL if a.mode == "full" else rt.RT_MODE_PRIMARY
    # the library splits a multi-device scene's frame itself: the caller renders the whole frame
    shard = (0, K) if K else ((0, 1) if devices else (rank, n))

    # the cold rate first: the same timed frames with no prewarm, right after the scene setup --
    # the GPU coming out of idle inside the timed window; then the headline, after a.prewarm_ms of untimed frames
    cold = None
    if a.prewarm_ms > 0 and not a.no_cold:
        el_c, st_c = timed_frames(rt, sc, cam, W, H, mode, shard, a.steps, a.warmup, barrier, sync_device, 0.0)
        el_c = reduce(el_c, "MAX")
        cold = {"mrays_per_s": round(reduce(float(st_c["primary_rays"] * a.steps), "SUM") / el_c / 1e6, 2),
                "ms_per_step": round(el_c / a.steps * 1e3, 4), "steps": a.steps, "warmup": a.warmup, "prewarm_frames": 0,
                "what": "the same timed frames measured first, right after the scene setup, with no prewarm (the GPU "
                        "leaving idle inside the window); `value` is the steady state after `prewarm_frames` frames"}
    elapsed, st = timed_frames(rt, sc, cam, W, H, mode, shard, a.steps, a.warmup, barrier, sync_device, a.prewarm_ms,
                               enqueue=False)
    # what the timed path computed in its last step: the frame the caller downloads (a rank under a launcher:
    # the frame buffer with this rank's tiles filled in, one file set per rank)
    dumped = None
    if a.dump_outputs:
        dumped = dump_arrays(a.dump_outputs, {"rgb": sc.download(W, H)}, suffix=f"_rank{rank}" if world > 1 else "")
    if a.full:
        st["enqueue_ms"] = enqueue_cost_ms(rt, sc, [cam] * min(a.steps, 3), W, H, mode, shard)
    my_rays = st["primary_rays"] * a.steps
    elapsed_max = reduce(elapsed, "MAX")
    total_rays = reduce(float(my_rays), "SUM")
    kernel_ms_avg = st["kernel_ms"] / max(st["launches"], 1)
    kernel_ms_max = reduce(kernel_ms_avg, "MAX")
    ms_per_step = elapsed_max / a.steps * 1e3
    # per GPU (rank, or device of an in-process multi-device scene): kernel ms per frame and rays per frame,
    # so an N > 1 line shows its load balance
    if devices:
        per_gpu = [{"device": d, "kernel_ms_per_frame": round(p["kernel_ms"] / max(p["launches"], 1), 4),
                    "rays_per_frame": p["primary_rays"]} for d, p in zip(devices, st["per_device"])]
    else:
        ks = gather_all(dist, dev, kernel_ms_avg)
        rs = gather_all(dist, dev, float(st["primary_rays"]))
        per_gpu = [{"rank": i, "kernel_ms_per_frame": round(k, 4), "rays_per_frame": int(r)}
                   for i, (k, r) in enumerate(zip(ks, rs))]

    # the dominant kernel's launch duration with one frame on the GPU (roofline denominator)
    iso_ms = iso_trace_ms = iso_ms_max = None
    if a.full:
        iso_ms, iso_trace_ms = isolated_kernel_ms(rt, sc, cam, W, H, mode, shard)
        iso_ms_max = reduce(iso_ms, "MAX")

    # the second frame size: N = 1 -> the C4 frame on this one GPU (strong-scaling base of C4);
    # N > 1 -> the metric's 1080p frame split over the N ranks
    extra = None
    if not a.no_extra and a.frame is None and a.scene == "soup" and not K:
        W2, H2 = (3840, 2160) if n == 1 else (1920, 1080)
        cam2 = rt.flycam(W2, H2, 0, 0, 20)
        k2 = max(10, a.steps // 2)
        el2, st2 = timed_frames(rt, sc, cam2, W2, H2, mode, shard, k2, a.warmup, barrier, sync_device, a.prewarm_ms)
        el2 = reduce(el2, "MAX")
        rays2 = reduce(float(st2["primary_rays"] * k2), "SUM")
        extra = {"frame": f"{W2}x{H2}", "workload": "C4 frame on 1 GPU" if n == 1 else f"C3 frame split over {n} GPUs",
                 "mrays_per_s": round(rays2 / el2 / 1e6, 2), "ms_per_step": round(el2 / k2 * 1e3, 4), "steps": k2}
        if n == 1 and a.tris == 1_000_000 and mode == rt.RT_MODE_PRIMARY:
            extra["parity"] = frame_parity(rt, sc, W2, H2, mode, "C4")

    # the other single-GPU BASELINE configs on the same GPU (N = 1 headline run only)
    side = {}
    if n == 1 and not a.no_side and a.frame is None and a.scene == "soup" and a.mode == "primary" and not K:
        for cn, md in (("c2", "primary"), ("c5", "full")):
            side[cn] = side_config(rt, cn.upper(), md, max(20, a.steps), a.warmup, local, ident["source_hash"], a.prewarm_ms,
                                   moving=(cn == "c5" and not a.no_moving))

    moving = None
    if (n == 1 and not a.no_moving and a.frame is None and a.scene == "soup" and a.tris == 1_000_000 and not K
            and devices is None):
        def make_scene(fif):
            mesh, _, _ = rt.soup_mesh(a.tris, 12345)
            return rt.Scene(mesh, device=local, leaf_size=a.leaf, frames_in_flight=fif, builder=builder,
                            wide_tree=1 if a.wide else 0, box_builder=0 if a.boxes == "host" else 1)
        moving = moving_camera(rt, make_scene, sc, W, H, mode, "C3" if a.mode == "primary" else "C3-full", a.steps,
                               a.warmup, sync_device, a.prewarm_ms)

    roof = None
    stats = None
    if rank == 0 and not a.no_stats:
        split = mode == rt.RT_MODE_PRIMARY and os.environ.get("RTAMD_DEBUG_KNOBS") == "1" and (int(os.environ.get("RT_KERNEL_VARIANT", "0") or 0) & (32768 | 256 | 2048))
        kern_ms = iso_trace_ms if mode == rt.RT_MODE_PRIMARY else iso_ms
        roof, stats = roofline_of(rt, sc, cam, W, H, mode, kern_ms, ms_per_step, info["n_faces"], ident["source_hash"],
                                  a.mode, "pmc_latest.json", split, shard)

    # the headline frame's parity against the committed oracle digests (every pixel; N = 1, C3)
    headline_parity = None
    if not a.full:
        pass
    elif rank == 0 and n == 1 and not K and a.frame is None and a.scene == "soup" and a.tris == 1_000_000:
        headline_parity = frame_parity(rt, sc, W, H, mode, "C3" if a.mode == "primary" else "C3-full")
    elif devices and not K and a.frame is None and a.scene == "soup" and a.tris == 1_000_000 and a.mode == "primary":
        # the in-process multi-device C4 frame, assembled from every device's tiles, against the oracle's digests
        headline_parity = frame_parity(rt, sc, W, H, mode, "C4")

    gpu_frame = None
    if rank == 0 and n == 1 and not a.no_cpu:
        sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True)
        gpu_frame = sc.download(W, H, want_hits=True)

    e2e = asm_ms = None
    if not a.no_e2e and torch.cuda.is_available():
        e2e, asm_ms = e2e_frame_ms(rt, sc, cam, W, H, mode, rank, n, dist)
        e2e, asm_ms = reduce(e2e, "MAX"), reduce(asm_ms, "MAX")

    cpu = None
    if rank == 0 and n == 1 and not a.no_cpu:
        threads, avail = cpu_threads()
        cpu = cpu_baseline(a.scene, (a.tris, 12345, rt.SOUP_MATERIAL), W, H, a.mode == "full", a.cpu_seconds,
                           threads, avail, gpu_frame)

    if rank == 0:
        value = total_rays / elapsed_max / 1e6
        if a.scene == "soup":
            cname = "C3" if (W, H) == (1920, 1080) else ("C4" if (W, H) == (3840, 2160) else "soup")
        else:
            cname = "C5" if a.mode == "full" else "C2"
        more = {}
        if e2e is not None:
            # one frame end to end: render + 8-bit frame assembled on rank 0 (RCCL all-gather for N>1) + D2H
            more["e2e_frame_ms"] = round(e2e, 3)
            # of it, after the render: the 8-bit frame assembled and on the host (one GPU: conversion + copy; an
            # in-process multi-device scene: its device-side assembly; torchrun: pack, all-gather, unpack, copy)
            more["assembly_ms"] = round(asm_ms, 3)
        if stats is not None:
            more["rays_per_frame_total"] = stats["total_rays"]  # primary + shadow + reflection (FULL)
            # (a rank's own rays times the ranks; a multi-device scene's stats already cover every device)
            more["total_mrays_per_s"] = round(stats["total_rays"] * (1 if devices else n) * a.steps / elapsed_max / 1e6, 2)
        out = {
            "metric": "Mrays/s (primary) + frame ms at 1920x1080, 1M-tri BVH, 1/2/4/8 GPU",
            "value": round(value, 2),
            "unit": "Mrays/s",
            "n_gpus": n,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {"workload": f"{cname}: {scene_name}, {W}x{H} {a.mode} rays, eye (0,0,1), 1 light"
                                   + (f", split over {n} GPUs" if n > 1 else "")
                                   + (f", REHEARSAL: shard 0 of {K} on one GPU (value = that shard's rate)" if K else ""),
                       "frame": f"{W}x{H}", "triangles": info["n_faces"], "mode": a.mode,
                       "parallelism": (f"tiles/{n} in one process over devices {devices} (rt_scene_opts.devices: "
                                       "scene replicated by peer copy, 64x64-pixel super-tiles interleaved over "
                                       "the devices, tiles assembled on the host)" if devices else
                                       f"tiles/{n} (64x64-pixel super-tiles interleaved over ranks, scene replicated)"
                                       if n > 1 else "tiles/1 (one GPU, whole frame)"),
                       "launcher": "in-process devices" if devices else ("torchrun" if world > 1 else "none"),
                       "per_gpu": per_gpu if n > 1 else None,
                       "frames_in_flight": info_fif, "prewarm_ms": a.prewarm_ms,
                       # untimed frames rendered back to back before the warmup (the headline is the steady state
                       # after them; `cold` below is the same timed frames with none)
                       "prewarm_frames": st["prewarm_frames"],
                       # HIP hardware queues per process: the environment's GPU_MAX_HW_QUEUES (0 = unset, the
                       # runtime's default 4); bench.py leaves it alone
                       "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "0") or 0),
                       # per-frame latency with frames in flight (first kernel start to last kernel end of one
                       # frame; frames overlap, so ms_per_step is the throughput interval) and alone
                       "kernel_ms_per_frame": round(kernel_ms_max, 4),
                       # (the lone frame, the enqueue cost and the tree's SAH cost: runs of their own, --full)
                       "kernel_ms_one_frame_alone": round(iso_ms_max, 4) if iso_ms_max is not None else None,
                       "host_enqueue_ms_per_frame": round(st["enqueue_ms"], 4) if "enqueue_ms" in st else None,
                       "bvh_nodes": info["bvh_nodes"], "bvh_depth": info["bvh_depth"],
                       "bvh_sah_cost": {k: round(v, 3) for k, v in sc.tree_cost().items()} if a.full else None,
                       "wide_tree": {"nodes_per_copy": info["wide_nodes"], "depth": info["wide_depth"]} if info["wide_nodes"] else None,
                       "ref_boxes": info["n_ref_boxes"], "scene_setup_s": round(setup_s, 2),
                       "scene_setup_s_per_rank": [round(x, 2) for x in setup_per_rank],
                       "scene_shared_build": cache_path is not None,
                       "scene_replicate_ms": round(info["replicate_ms"], 1) if info["n_devices"] > 1 else None,
                       "builder": {0: "sah-host", 1: "lbvh-gpu", 2: "sbvh-host", 3: "ploc-gpu", 4: "sah-gpu", 5: "sbvh-gpu"}.get(info["builder"], str(info["builder"])),
                       "build_ms": {"prep": round(info["prep_ms"], 1), "ref_boxes": round(info["boxes_ms"], 1),
                                    "bvh": round(info["bvh_ms"], 1), "bvh_gpu_kernels": round(info["bvh_gpu_ms"], 2),
                                    "upload": round(info["upload_ms"], 1)}, **more},
            "roofline": roof,
            "cpu_baseline": cpu,
            "build": ident,
            "full": a.full,
        }
        if dumped is not None:
            out["dumped_outputs"] = {"dir": a.dump_outputs, "files": dumped}
        if cold is not None:
            out["cold"] = cold
        if moving is not None:
            out["moving_camera"] = moving
        if extra is not None:
            out["c4_frame" if n == 1 else "c3_frame"] = extra
        out.update(side)
        if headline_parity is not None:
            out["parity"] = headline_parity
            c5m = (side.get("c5") or {}).get("moving_camera")
            checked = [headline_parity] + [v["parity"] for v in (side.get("c2"), side.get("c5"), extra, moving, c5m)
                                           if v and "parity" in v]
            out["parity_all_configs"] = {p["case"]: p["face_t_digest_equal"] for p in checked}
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
