#!/usr/bin/env python3
"""rt_trace_stream_color measurement (MI355X): the in-order list kernel, RT_RAYS_REORDER, RT_RAYS_WAVEFRONT and both,
at FULL depth 2, FULL depth 4 and PRIMARY depth 3. Prints and writes profiles/ab/ray_wavefront_ab.txt.

  A       the bunny C2 frame's 1920x1080 camera rays in 8x8-pixel blocks (coherent)
  B       list A under a fixed-seed shuffle
  C       2M rays drawn as tests/test_gpu_parity.py::test_trace_queries_match_oracle draws them
  soup-B  the 1M-triangle soup's camera rays, blocks then the same shuffle

Per list, setting and flag combination: Mrays/s (HIP events on a torch stream, an untimed warm-up, `--repeats` windows,
median and min..max), the wave node fetches per ray of a counting run (ST_WNODE / n, untimed), and for the wavefront
combinations the per-level live and hit counts (rt_debug_ray_levels).

  --parent LIB   only the parent comparison: rt_trace_stream(RT_RAYS_COLOR) on A and B, this build against the
                 library LIB (a build of the parent commit), alternating child processes (one library per process:
                 each run is `--color-only` under RTAMD_LIB); appended to the output file
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np
import torch  # before the library: one HIP runtime per process

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-project_amd"))
import rtamd as rt  # noqa: E402

W, H = 1920, 1080
C2_CAMERA = (0.0, 0.0, 20.0)
SETTINGS = (("FULL depth 2", rt.RT_MODE_FULL, 2), ("FULL depth 4", rt.RT_MODE_FULL, 4), ("PRIMARY depth 3", rt.RT_MODE_PRIMARY, 3))
COMBOS = (("in order", False, False), ("REORDER", True, False), ("WAVEFRONT", False, True), ("WAVEFRONT | REORDER", True, True))


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


def timed(call, repeats, stream, inner):
    call()
    stream.synchronize()  # warm-up: code objects loaded, scratch grown
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(inner):
            call()
        e1.record(stream)
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / inner)
    return ms


def camera_lists(sc):
    o, d = sc.camera_rays(rt.flycam(W, H, *C2_CAMERA), W, H)
    t_tiles = torch.from_numpy(tile_order(W, H)).cuda()
    t_shuffle = torch.from_numpy(np.random.default_rng(2024).permutation(W * H)).cuda()
    A = (o[t_tiles].contiguous(), d[t_tiles].contiguous())
    return A, (A[0][t_shuffle].contiguous(), A[1][t_shuffle].contiguous())


def color_only(repeats):
    """rt_trace_stream(RT_RAYS_COLOR) on A and B with whatever library RTAMD_LIB names: one JSON line"""
    sc = rt.Scene(rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj")))
    stream = torch.cuda.Stream()
    res = {}
    lists = camera_lists(sc)
    torch.cuda.synchronize()  # the lists were built on torch's default stream
    for name, (a, b) in zip("AB", lists):
        out = sc.trace_stream(rt.RT_RAYS_COLOR, a, b, lights=rt.DEFAULT_LIGHTS, stream=stream.cuda_stream)
        ms = timed(lambda: sc.trace_stream(rt.RT_RAYS_COLOR, a, b, lights=rt.DEFAULT_LIGHTS, stream=stream.cuda_stream, out=out),
                   repeats, stream, 10)
        res[name] = statistics.median(ms)
    print(json.dumps(res), flush=True)


def parent_comparison(parent_lib, repeats, rounds, say):
    runs = {"parent": [], "this build": []}
    for _ in range(rounds):
        for label, lib in (("parent", parent_lib), ("this build", None)):
            env = dict(os.environ)
            env.pop("RTAMD_LIB", None)
            if lib:
                env["RTAMD_LIB"] = lib
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--color-only", "--repeats", str(repeats)],
                               env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"ray_wavefront_ab: {label} run failed: {p.stderr[-1500:]}")
            runs[label].append(json.loads(p.stdout.strip().splitlines()[-1]))
    say(f"parent comparison: rt_trace_stream(RT_RAYS_COLOR), {rounds} alternating processes each, ms per call "
        f"(each process: median of {repeats} windows of 10 calls); median (min..max) over the processes")
    inside = True
    for name in "AB":
        par, new = [r[name] for r in runs["parent"]], [r[name] for r in runs["this build"]]
        say(f"  list {name}: parent {med(par)} ms   this build {med(new)} ms")
        inside = inside and min(new) <= max(par)  # the two ranges overlap, or this build is the faster one
    say("  this build's runs " + ("overlap the parent's range (or lie below it) on both lists" if inside
                                   else "lie ABOVE the parent's range on at least one list"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5, help="--parent: processes per library")
    ap.add_argument("--parent", default=None, help="library of the parent commit: only the parent comparison")
    ap.add_argument("--color-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--no-soup", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "ray_wavefront_ab.txt"))
    args = ap.parse_args()
    if rt.device_count() == 0:
        sys.exit("ray_wavefront_ab: no GPU (a measurement needs one)")
    if args.color_only:
        return color_only(args.repeats)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.parent:
        parent_comparison(args.parent, args.repeats, args.rounds, say)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
        return
    say(f"ray wavefront A/B: {rt.lib().rt_version_string().decode()}; {W}x{H} camera {C2_CAMERA}, default light; "
        f"{args.repeats} windows, ms per call median (min..max)")
    stream = torch.cuda.Stream()
    bunny = rt.Scene(rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj")))
    A, B = camera_lists(bunny)
    co, cd = aimed_rays(2_000_000)
    lists = [("A", bunny, A), ("B", bunny, B), ("C", bunny, (torch.from_numpy(co).cuda(), torch.from_numpy(cd).cuda()))]
    if not args.no_soup:
        soup = rt.Scene(rt.soup_mesh(1_000_000, 12345)[0])
        lists.append(("soup-B", soup, camera_lists(soup)[1]))
    rate = {}
    torch.cuda.synchronize()  # the lists were built on torch's default stream
    for name, sc, (a, b) in lists:
        n = a.shape[0]
        for sname, mode, depth in SETTINGS:
            say(f"list {name}, {sname}: {n} rays")
            for cname, reorder, wavefront in COMBOS:
                kw = dict(mode=mode, max_depth=depth, reorder=reorder, wavefront=wavefront)
                out = sc.trace_stream_color(a, b, rt.DEFAULT_LIGHTS, stream=stream.cuda_stream, **kw)
                ms = timed(lambda: sc.trace_stream_color(a, b, rt.DEFAULT_LIGHTS, stream=stream.cuda_stream, out=out, **kw),
                           args.repeats, stream, 5)
                sc.trace_stream_color(a, b, rt.DEFAULT_LIGHTS, stats=True, out=out, **kw)
                wn = sc.counters(8)[2] / n
                rate[(name, sname, cname)] = n / statistics.median(ms) / 1e3
                say(f"  {cname:20s} {med(ms)} ms  {rate[(name, sname, cname)]:8.1f} Mrays/s   ST_WNODE/ray {wn:7.3f}")
                if wavefront and reorder:
                    say("      levels (live, hits): " + " ".join(f"({lv[0]}, {lv[1]})" for lv in sc.ray_levels().tolist()))
    for name in ("B", "soup-B"):
        for sname, _, _ in SETTINGS:
            if (name, sname, "REORDER") in rate:
                r = rate[(name, sname, "WAVEFRONT | REORDER")] / rate[(name, sname, "REORDER")]
                say(f"list {name}, {sname}: WAVEFRONT | REORDER / REORDER = {r:.2f}x")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
