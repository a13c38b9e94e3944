#!/usr/bin/env python3
"""Ray-stream measurement (MI355X): in-order against RT_RAYS_REORDER on four ray lists, and the host-pointer API
beside the stream API. Prints and writes profiles/ab/ray_streams_ab.txt.

  A  the bunny C2 frame's 1920x1080 camera rays (rt_rays_camera) in 8x8-pixel blocks: the coherent best case
  B  list A under a fixed-seed shuffle
  C  2M rays drawn as tests/test_gpu_parity.py::test_trace_queries_match_oracle draws them
  D  the RT_RAYS_SHADOW rays from list B's hit points to the default light

Per list: Mrays/s in order; Mrays/s reordered (key + sort included); the key + sort time on its own (the
reordered call minus an in-order call on the list physically permuted into that order, so what remains is keys,
sort and the indexed loads); ST_WNODE per ray for both (counting runs, untimed), under both key layouts; for A
and C the host-pointer API's end-to-end rate (upload, trace, download; host clock). Stream calls are timed with
HIP events on a torch stream, after an untimed warm-up, `--repeats` times; median and min..max are reported.

  --host-api-only   only the host-pointer figures of A and C (camera rays from numpy, so that a library built
                    before ray streams -- RTAMD_LIB -- can run it: the parent-commit comparison)
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-project_amd"))
import rtamd as rt  # noqa: E402

W, H = 1920, 1080
C2_CAMERA = (0.0, 0.0, 20.0)
ORIGIN_MAJOR = 4194304  # rt_debug_set_variant bit: the other key layout


def med(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):.3f}..{max(xs):.3f})"


def tile_order(w, h):
    idx = np.arange(w * h).reshape(h, w)
    return np.concatenate([idx[y:y + 8, x:x + 8].reshape(-1) for y in range(0, h, 8) for x in range(0, w, 8)])


def aimed_rays(n, seed=7):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32) - o
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def numpy_camera_rays(cam, w, h):
    """screenToWorld in numpy (timing input only; rt_rays_camera is the exact generator)"""
    V = np.array(cam.view_matrix, np.float64).reshape(4, 4).T
    Vi = np.linalg.inv(V)
    scale = np.tan(np.radians(cam.fovy / 2.0))
    px, py = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    nx = 2.0 * (px - cam.viewport[0]) / cam.viewport[2] - 1.0
    ny = 1.0 - 2.0 * (py - cam.viewport[1]) / cam.viewport[3]
    p = np.stack([nx * cam.aspect_ratio * scale, ny * scale, -np.ones_like(nx), np.ones_like(nx)], -1).reshape(-1, 4)
    wpt = (p @ Vi.T)[:, :3]
    eye = Vi[:3, 3]
    d = wpt - eye
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.tile(eye, (w * h, 1)).astype(np.float32), d.astype(np.float32)


def time_stream(sc, query, a, b, reorder, repeats, stream):
    out = {k: v for k, v in sc.trace_stream(query, a, b, reorder=reorder, stream=stream.cuda_stream).items()
           if k in ("face", "t", "blocked")}
    stream.synchronize()  # warm-up: code objects loaded, scratch grown
    inner = 50  # calls per timed window: tens of milliseconds of device work
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            sc.trace_stream(query, a, b, reorder=reorder, stream=stream.cuda_stream, out=out)
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return ms


def wnode(sc, query, a, b, reorder):
    sc.trace_stream(query, a, b, reorder=reorder, stats=True)
    return sc.counters(8)[2] / a.shape[0]


def time_host(sc, query, a, b, repeats):
    f = sc.trace_shadow if query == rt.RT_RAYS_SHADOW else sc.trace_closest
    f(a, b)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        f(a, b)
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--host-api-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "ray_streams_ab.txt"))
    args = ap.parse_args()
    if rt.device_count() == 0:
        sys.exit("ray_stream_ab: no GPU (a measurement needs one)")
    sc = rt.Scene(rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj")))
    cam = rt.flycam(W, H, *C2_CAMERA)
    lines = [f"ray streams A/B: {rt.lib().rt_version_string().decode()}; bunny, {W}x{H} camera {C2_CAMERA}; "
             f"{args.repeats} repeats, median (min..max)"]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tiles = tile_order(W, H)
    shuffle = np.random.default_rng(2024).permutation(W * H)
    co, cd = aimed_rays(2_000_000)
    if args.host_api_only:
        ao, ad = numpy_camera_rays(cam, W, H)
        for name, (o, d) in {"A": (ao[tiles], ad[tiles]), "C": (co, cd)}.items():
            ms = time_host(sc, rt.RT_RAYS_CLOSEST, np.ascontiguousarray(o), np.ascontiguousarray(d), args.repeats)
            say(f"host-pointer API list {name}: {len(o)} rays, {med(ms)} ms end to end, "
                f"{len(o) / statistics.median(ms) / 1e3:.1f} Mrays/s")
        return
    stream = torch.cuda.Stream()
    o, d = sc.camera_rays(cam, W, H)
    t_tiles, t_shuffle = torch.from_numpy(tiles).cuda(), torch.from_numpy(shuffle).cuda()
    A = (o[t_tiles].contiguous(), d[t_tiles].contiguous())
    B = (A[0][t_shuffle].contiguous(), A[1][t_shuffle].contiguous())
    Cl = (torch.from_numpy(co).cuda(), torch.from_numpy(cd).cuda())
    hit = sc.trace_stream(rt.RT_RAYS_CLOSEST, *B)
    keep = hit["face"] >= 0
    P = hit["P"][keep].contiguous()
    light = torch.tensor(rt.DEFAULT_LIGHTS[0][0], dtype=torch.float32, device="cuda")
    L = torch.nn.functional.normalize(light - P, dim=1).contiguous()
    lists = {"A": (rt.RT_RAYS_CLOSEST, A), "B": (rt.RT_RAYS_CLOSEST, B), "C": (rt.RT_RAYS_CLOSEST, Cl),
             "D": (rt.RT_RAYS_SHADOW, (P, L))}
    rate = {}
    for name, (query, (a, b)) in lists.items():
        n = a.shape[0]
        plain = time_stream(sc, query, a, b, False, args.repeats, stream)
        reord = time_stream(sc, query, a, b, True, args.repeats, stream)
        perm = torch.from_numpy(sc.ray_order().astype(np.int64)).cuda()
        sorted_list = time_stream(sc, query, a[perm].contiguous(), b[perm].contiguous(), False, args.repeats, stream)
        w_plain, w_reord = wnode(sc, query, a, b, False), wnode(sc, query, a, b, True)
        prev = rt.set_variant(ORIGIN_MAJOR)
        try:
            w_oct = wnode(sc, query, a, b, True)
            reord_oct = time_stream(sc, query, a, b, True, args.repeats, stream)
        finally:
            rt.set_variant(prev)
        rate[name] = (n / statistics.median(plain) / 1e3, n / statistics.median(reord) / 1e3)
        say(f"list {name}: {n} rays")
        say(f"  in order            {med(plain)} ms  {rate[name][0]:8.1f} Mrays/s   ST_WNODE/ray {w_plain:7.3f}")
        say(f"  reordered (total)   {med(reord)} ms  {rate[name][1]:8.1f} Mrays/s   ST_WNODE/ray {w_reord:7.3f} (octant-major key, the default)")
        say(f"  reordered, origin-major key {med(reord_oct)} ms                  ST_WNODE/ray {w_oct:7.3f}")
        say(f"  same order, list permuted beforehand {med(sorted_list)} ms -> key + sort + indexed loads "
            f"{statistics.median(reord) - statistics.median(sorted_list):.3f} ms")
        if name in ("A", "C"):
            ms = time_host(sc, query, a.cpu().numpy(), b.cpu().numpy(), args.repeats)
            say(f"  host-pointer API    {med(ms)} ms end to end  {n / statistics.median(ms) / 1e3:8.1f} Mrays/s")
    say(f"reordered B / in-order B = {rate['B'][1] / rate['B'][0]:.2f}x; reordered B / in-order A = "
        f"{rate['B'][1] / rate['A'][0]:.2f}")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
