#!/usr/bin/env python3
"""Supersampling measurement (MI355X): prints and writes profiles/ab/supersample_ab.txt.

S rays per pixel (grid patterns of every power-of-two count, 2 to 64), PRIMARY depth 1 and FULL depth 2, on the
bunny and the 1M soup, for one 1920x1080 view and for 64 views of 128x128, three ways:
  (a) what a caller could do before rt_render_views_ss: S rt_render_views batches with the viewport-shifted cameras
      on one torch stream, summed in order by torch on the device (add_ per batch, one division);
  (b) rt_render_views_ss in the loop layout;
  (c) rt_render_views_ss in the packed layout (the variant bit selects whichever is not the default).
All three produce the same bits (tests/test_gpu_supersample.py); here only the time is taken.

Figures: wall ms from the first call until the result is complete (a stream synchronise ends all three), and the
device ms between two events around the enqueued work. Method as tools/view_batch_ab.py: one process per scene
builds the scene once, per case every side is prewarmed, then the sides alternate `--reps` times and the process
reports the median per side; `--rounds` such processes per scene after one discarded process; the record gives
median (min..max) over the processes. No ratio is fixed in advance. The default layout of a sample count is the one
that is faster beyond the spread on both scenes (in every case of that count); where the ranges overlap the loop
stays."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (first: the process must use one copy of the HIP runtime, torch's)

sys.path.insert(0, os.path.join(ROOT, "ray-tracing-project_amd"))
import rtamd as rt  # noqa: E402

SHAPES = [(1, 1920, 1080), (64, 128, 128)]
MODES = [("PRIMARY depth 1", rt.RT_MODE_PRIMARY), ("FULL depth 2", rt.RT_MODE_FULL)]
GRIDS = [(2, 1), (2, 2), (4, 2), (4, 4), (8, 4), (8, 8)]  # every sample count the packed layout takes
SIDES = ("batches", "loop", "packed")


def med(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):.3f}..{max(xs):.3f})"


def shifted(cam, ox, oy):
    c = rt.Camera()
    C.memmove(C.addressof(c), C.addressof(cam), C.sizeof(c))
    c.viewport[0] = float(np.float32(cam.viewport[0]) - np.float32(ox))
    c.viewport[1] = float(np.float32(cam.viewport[1]) - np.float32(oy))
    return c


def child(args):
    """one process, one scene, every case: a JSON line {case: {side: [wall, device]}} (ms, medians over the reps)"""
    if args.scene == "bunny":
        mesh = rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj"))
    else:
        mesh = rt.soup_mesh(1_000_000)[0]
    sc = rt.Scene(mesh)
    L = rt.lib()
    lights = rt.Scene._lights(rt.DEFAULT_LIGHTS)
    lp = C.cast(lights, C.c_void_p)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    res = {}
    for nx, ny in GRIDS:
        pat = rt.sample_grid(nx, ny)
        S = pat.n_samples
        offs = pat.array()
        variant = {}
        for v in (0, rt.VARIANT_SAMPLE_LAYOUT):
            variant["packed" if rt.sample_plan(rt.RT_MODE_FULL, 0, 1, 1, 1, S, variant=v)["layout"] else "loop"] = v
        for label, mode in MODES:
            for n, W, H in SHAPES:
                base = rt.CameraPath(W, H).take(n)
                cams = (rt.Camera * n)(*base)
                per_sample = [(rt.Camera * n)(*[shifted(c, ox, oy) for c in base]) for ox, oy in offs]
                rgb = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
                tmp = torch.empty_like(rgb)
                fr = rt.Frame(W, H, mode, 0, 1, 0, 0)
                vb = rt.ViewBatch(n, C.cast(cams, C.c_void_p), rgb.data_ptr(), None, None)
                vbs = [rt.ViewBatch(n, C.cast(per_sample[k], C.c_void_p), (rgb if k == 0 else tmp).data_ptr(), None, None)
                       for k in range(S)]

                def enqueue(side):
                    if side == "batches":
                        for k in range(S):
                            rt.check(L.rt_render_views(sc.h, C.byref(vbs[k]), lp, 1, C.byref(fr), sp))
                            if k:
                                rgb.add_(tmp)
                        rgb.div_(float(S))
                    else:
                        rt.check(L.rt_render_views_ss(sc.h, C.byref(vb), lp, 1, C.byref(fr), C.byref(pat), sp))

                def timed(side):
                    """(wall ms from the first call to completion, device ms between two events)"""
                    prev = rt.set_variant(variant.get(side, 0))
                    try:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        with torch.cuda.stream(stream):
                            t0 = time.perf_counter()
                            e0.record()
                            enqueue(side)
                            e1.record()
                            stream.synchronize()
                            wall = (time.perf_counter() - t0) * 1e3
                        return wall, e0.elapsed_time(e1)
                    finally:
                        rt.set_variant(prev)

                for _ in range(args.warmup):
                    for side in SIDES:
                        timed(side)
                got = {side: [] for side in SIDES}
                for _ in range(args.reps):  # the sides alternate
                    for side in SIDES:
                        got[side].append(timed(side))
                res[f"{S}|{label}|{n}|{W}x{H}"] = {side: [statistics.median(x[0] for x in got[side]),
                                                         statistics.median(x[1] for x in got[side])] for side in SIDES}
                del rgb, tmp
    print(json.dumps(res), flush=True)


def run_child(scene, args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scene", scene, "--reps", str(args.reps),
                        "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        sys.exit(f"supersample_ab: child {scene} failed ({p.returncode}): {p.stderr[-1500:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="processes per scene (after one discarded)")
    ap.add_argument("--reps", type=int, default=5, help="alternating repetitions of the sides per case and process")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="bunny,soup")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "supersample_ab.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="bunny", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if rt.device_count() == 0:
        sys.exit("supersample_ab: no GPU (a measurement needs one)")
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"supersampling A/B: {rt.lib().rt_version_string().decode()}")
    say(f"S rays per pixel (grid patterns), one point light, cameras of CameraPath; (a) batches = S rt_render_views batches "
        f"with shifted cameras summed in order by torch on the device, (b) loop and (c) packed = rt_render_views_ss in that "
        f"layout; wall ms from the first call to completion / device ms between two events; per process the median of "
        f"{args.reps} alternating repetitions after {args.warmup} warm-up rounds; {args.rounds} processes per scene after one "
        f"discarded, median (min..max) over the processes")
    # verdict[S][scene] = per case: which layout is faster beyond the spread (wall and device), or None
    verdict = {}
    for scene in args.scenes.split(","):
        run_child(scene, args)  # discarded: the first process after the GPU sat idle runs at ramping clocks
        runs = [run_child(scene, args) for _ in range(args.rounds)]
        say(f"{scene}:")
        for case in runs[0]:
            S, label, n, size = case.split("|")
            say(f"  S = {int(S):2d}  {label:16s} {int(n):3d} x {size}:")
            dev = {}
            for side, name in zip(SIDES, ("(a) batches", "(b) loop", "(c) packed")):
                wall = [r[case][side][0] for r in runs]
                dev[side] = [r[case][side][1] for r in runs]
                say(f"    {name:12s} wall {med(wall)} ms   device {med(dev[side])} ms")
            a, b, c = (statistics.median(dev[s]) for s in SIDES)
            winner = "packed" if max(dev["packed"]) < min(dev["loop"]) else "loop" if max(dev["loop"]) < min(dev["packed"]) else None
            best = min(dev["loop"], dev["packed"], key=statistics.median)
            note = "" if max(best) < min(dev["batches"]) else "   ((a) is not slower beyond the spread)"
            say(f"    device: batches / loop = {a / b:5.2f}x   batches / packed = {a / c:5.2f}x   loop / packed = {b / c:5.2f}x"
                f"   ({'ranges overlap' if winner is None else winner + ' is faster beyond the spread'}){note}")
            verdict.setdefault(int(S), []).append(winner)
    say("default layout per sample count (packed only where it is faster beyond the spread in every case on every scene measured):")
    for S, ws in sorted(verdict.items()):
        say(f"  S = {S:2d}: {'packed' if all(w == 'packed' for w in ws) else 'loop'}   (per case: {', '.join(w or 'overlap' for w in ws)})")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
