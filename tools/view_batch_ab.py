#!/usr/bin/env python3
"""View-batch measurement (MI355X): prints and writes profiles/ab/view_batches_ab.txt.

One rt_render_views batch against the same cameras rendered by a loop of rt_render_async (a scene with 4 frames in
flight) followed by rt_synchronize, on the bunny and the 1M soup, PRIMARY depth 1 and FULL depth 2, at the
(views, size) pairs (256, 64x64), (64, 128x128), (16, 256x256), (4, 512x512), (1, 1920x1080). Cameras: CameraPath.

Headline figure: wall time from the first call to completion (the loop's enqueue cost is the point) -- the batch
with hip_stream NULL, which returns after completion; the loop until rt_synchronize returns. Both sides call the C
ABI through prebuilt ctypes arguments, so the binding's per-call work is not in the loop. Beside it: the batch's
device time between two events on a torch stream around the enqueued call.

Method: one process per scene builds the scene once; per case both sides are prewarmed (code objects, frame
buffers, the camera array, the loop's longest-first map), then alternate `--reps` times; the process reports the
median per side. `--rounds` such processes per scene after one discarded process (clocks ramping up out of idle);
the record gives median (min..max) over the processes. No threshold is fixed: the record states the ratios."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402,F401  (first: the process must use one copy of the HIP runtime, torch's)

sys.path.insert(0, os.path.join(ROOT, "ray-tracing-project_amd"))
import rtamd as rt  # noqa: E402

SHAPES = [(256, 64, 64), (64, 128, 128), (16, 256, 256), (4, 512, 512), (1, 1920, 1080)]
MODES = [("PRIMARY depth 1", rt.RT_MODE_PRIMARY), ("FULL depth 2", rt.RT_MODE_FULL)]


def med(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):.3f}..{max(xs):.3f})"


def child(args):
    """one process, one scene, every case: a JSON line {case: {loop, batch, device}} (ms, medians over the reps)"""
    if args.scene == "bunny":
        mesh = rt.Mesh.load_obj(os.path.join(ROOT, "scenes", "bunny.obj"))
    else:
        mesh = rt.soup_mesh(1_000_000)[0]
    sc = rt.Scene(mesh, frames_in_flight=4)
    L = rt.lib()
    lights = rt.Scene._lights(rt.DEFAULT_LIGHTS)
    lp = C.cast(lights, C.c_void_p)
    stream = torch.cuda.Stream()
    sp = C.c_void_p(stream.cuda_stream)
    res = {}
    for label, mode in MODES:
        for n, W, H in SHAPES:
            cams = (rt.Camera * n)(*rt.CameraPath(W, H).take(n))
            rgb = torch.empty((n, H, W, 3), dtype=torch.float32, device="cuda")
            vb = rt.ViewBatch(n, C.cast(cams, C.c_void_p), rgb.data_ptr(), None, None)
            fr = rt.Frame(W, H, mode, 0, 1, 0, 0)
            st = rt.Stats()

            def loop():
                t0 = time.perf_counter()
                for k in range(n):
                    rt.check(L.rt_render_async(sc.h, C.byref(cams[k]), lp, 1, C.byref(fr)))
                rt.check(L.rt_synchronize(sc.h, C.byref(st)))
                return (time.perf_counter() - t0) * 1e3

            def batch():
                t0 = time.perf_counter()
                rt.check(L.rt_render_views(sc.h, C.byref(vb), lp, 1, C.byref(fr), None))
                return (time.perf_counter() - t0) * 1e3

            def batch_device():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with torch.cuda.stream(stream):
                    e0.record()
                    rt.check(L.rt_render_views(sc.h, C.byref(vb), lp, 1, C.byref(fr), sp))
                    e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1)

            for _ in range(args.warmup):
                loop(), batch(), batch_device()
            lo, ba, de = [], [], []
            for _ in range(args.reps):  # the two sides alternate
                lo.append(loop())
                ba.append(batch())
                de.append(batch_device())
            res[f"{label}|{n}|{W}x{H}"] = {"loop": statistics.median(lo), "batch": statistics.median(ba),
                                           "device": statistics.median(de)}
            del rgb
    print(json.dumps(res), flush=True)


def run_child(scene, args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scene", scene, "--reps", str(args.reps),
                        "--warmup", str(args.warmup)], capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit(f"view_batch_ab: child {scene} failed ({p.returncode}): {p.stderr[-1500:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="processes per scene (after one discarded)")
    ap.add_argument("--reps", type=int, default=5, help="alternating repetitions of both sides per case and process")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--scenes", default="bunny,soup")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "view_batches_ab.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="bunny", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if rt.device_count() == 0:
        sys.exit("view_batch_ab: no GPU (a measurement needs one)")
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"view batches A/B: {rt.lib().rt_version_string().decode()}")
    say(f"one rt_render_views batch against a loop of rt_render_async (4 frames in flight) + rt_synchronize, same cameras "
        f"(CameraPath), one point light; wall ms from the first call to completion, and the batch's device ms between two "
        f"events; per process the median of {args.reps} alternating repetitions after {args.warmup} warm-up rounds; "
        f"{args.rounds} processes per scene after one discarded, median (min..max) over the processes; "
        f"loop / batch = ratio of the medians (> 1: the batch is faster)")
    for scene in args.scenes.split(","):
        run_child(scene, args)  # discarded: the first process after the GPU sat idle runs at ramping clocks
        runs = [run_child(scene, args) for _ in range(args.rounds)]
        say(f"{scene}:")
        for case in runs[0]:
            label, n, size = case.split("|")
            lo, ba, de = ([r[case][k] for r in runs] for k in ("loop", "batch", "device"))
            ratio = statistics.median(lo) / statistics.median(ba)
            clear = "" if (max(ba) < min(lo) or max(lo) < min(ba)) else "   (ranges overlap)"
            say(f"  {label:16s} {int(n):4d} x {size:9s}: loop {med(lo)} ms   batch {med(ba)} ms   loop / batch = {ratio:6.2f}x{clear}"
                f"   batch device {med(de)} ms")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
