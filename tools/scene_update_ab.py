#!/usr/bin/env python3
"""Scene-update measurement (MI355X): prints and writes profiles/ab/scene_update_ab.txt.

Three questions, none with a threshold fixed in advance:
  (a) update against create: the wall time of rt_scene_update (a host clock around the call, which ends
      synchronised) with its phase split from rt_update_stats, against rt_scene_create of the same mesh timed on
      the parent commit's build (--parent-lib) and on this one, for the bunny and the 1M soup;
  (b) what the refit costs in traversal: a 1920x1080 PRIMARY and FULL frame (the render kernels' device ms) on the
      updated scene against a fresh scene of the same geometry, along the deformation at three amplitudes, with
      rt_debug_tree_cost beside each;
  (c) regression check (--bench): bench.py's C3 / C2 / C5 rates and scene setup on both builds, alternating.

Method as the other *_ab.py tools: one process per (scene, build) does every case and prints one JSON line; after
one discarded process, `--rounds` processes per side, alternating where two builds are compared; the record gives
median (min..max) over the processes. The deformation is tests/update_scenes.py's seeded sine displacement."""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtamd as rt  # noqa: E402
from update_scenes import deform, obj_arrays  # noqa: E402  (the tests' deformation: one definition)
from update_scenes import mesh_of as update_mesh_of  # noqa: E402

AMPLITUDES = (0.02, 0.05, 0.15)
W, H = 1920, 1080
CHILD_TIMEOUT_S = 300  # a child process (one scene's cases, or one bench.py run) that takes longer has hung
F = np.float32


def med(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def scene_arrays(name):
    if name == "bunny":
        return obj_arrays(rt, os.path.join(ROOT, "scenes", "bunny.obj"))
    v = rt.generate_soup(1_000_000, 12345)
    f = np.arange(3 * 1_000_000, dtype=np.uint32).reshape(-1, 3)
    return v, f, np.array([rt.SOUP_MATERIAL], F), None


def mesh_of(arr, v=None):
    return update_mesh_of(rt, arr, v)


def timed(f):
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def kernel_ms(sc, mode, reps=9):
    cam = rt.flycam(W, H, 0, 0, 20)
    sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode)
    sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode)
    return statistics.median(sc.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode)[1]["trace_kernel_ms"] for _ in range(reps))


def child(args):
    arr = scene_arrays(args.scene)
    mesh0 = mesh_of(arr)
    res = {"create_ms": [], "lib": os.path.basename(rt.LIB_PATH)}
    rt.Scene(mesh0)  # the process's first scene pays the device's first use
    for _ in range(3):
        ms, sc = timed(lambda: rt.Scene(mesh0))
        res["create_ms"].append(ms)
        res["create_phases"] = {k: sc.info()[k] for k in ("prep_ms", "boxes_ms", "bvh_ms", "upload_ms")}
    if not hasattr(rt.lib(), "rt_scene_update"):
        print(json.dumps(res), flush=True)
        return
    res["update"], res["traverse"] = {}, {}
    sc.update(mesh_of(arr, deform(arr[0], 0.01)))  # the first update's one-time uploads are not part of a step
    for amp in AMPLITUDES + (0.0,):
        mesh = mesh_of(arr, deform(arr[0], amp))
        ms, _ = timed(lambda: sc.update(mesh))  # stats = NULL: no SAH cost, no host mirror
        ms2, st = timed(lambda: sc.update(mesh, stats=True))
        res["update"][str(amp)] = {"wall_ms": ms, **{k: st[k] for k in ("prep_ms", "boxes_ms", "records_ms", "upload_ms",
                                                                      "refit_ms", "total_ms", "bounds_on_device", "sah_cost")}}
        if amp:
            fresh = rt.Scene(mesh)
            tr = {"sah_updated": sc.tree_cost()["sah"], "sah_fresh": fresh.tree_cost()["sah"]}
            for key, mode in (("primary", rt.RT_MODE_PRIMARY), ("full", rt.RT_MODE_FULL)):
                a, b = [], []
                for _ in range(3):  # the two scenes alternate
                    a.append(kernel_ms(sc, mode))
                    b.append(kernel_ms(fresh, mode))
                tr[key + "_updated_ms"], tr[key + "_fresh_ms"] = statistics.median(a), statistics.median(b)
            res["traverse"][str(amp)] = tr
            del fresh
    print(json.dumps(res), flush=True)


def run_child(scene, lib):
    env = dict(os.environ)
    if lib:
        env["RTAMD_LIB"] = lib
    else:
        env.pop("RTAMD_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scene", scene], env=env, check=True,
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT_S).stdout
    return json.loads(out.strip().splitlines()[-1])


def run_bench(lib, steps):
    env = dict(os.environ)
    if lib:
        env["RTAMD_LIB"] = lib
    else:
        env.pop("RTAMD_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5",
                          "--full", "--no-cpu", "--no-e2e", "--no-extra", "--no-cold", "--no-moving"], env=env, check=True,
                         capture_output=True, text=True, timeout=CHILD_TIMEOUT_S).stdout
    j = json.loads(out.strip().splitlines()[-1])
    return {"c3": j["value"], "c2": j["c2"]["mrays_per_s"], "c5": j["c5"]["mrays_per_s"], "setup_s": j["config"]["scene_setup_s"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--scene", default="bunny")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="librtamd.so of the parent commit (create times, bench)")
    ap.add_argument("--bench", action="store_true", help="also bench.py on both builds, alternating")
    ap.add_argument("--only-bench", action="store_true", help="the bench.py section alone (appended to --out)")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "scene_update_ab.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    lines = [] if args.only_bench else [
        "scene update A/B (tools/scene_update_ab.py): median (min..max) over %d processes, ms" % args.rounds]
    for scene in () if args.only_bench else ("bunny", "soup"):
        run_child(scene, None)  # discarded
        new, old = [], []
        for _ in range(args.rounds):  # the builds alternate
            if args.parent_lib:
                old.append(run_child(scene, args.parent_lib))
            new.append(run_child(scene, None))
        lines.append(f"\n== {scene} ==")
        cn = [statistics.median(r["create_ms"]) for r in new]
        lines.append(f"rt_scene_create, this build     {med(cn)}   phases {json.dumps({k: round(v, 1) for k, v in new[-1]['create_phases'].items()})}")
        co = [statistics.median(r["create_ms"]) for r in old] if old else None
        if co:
            lines.append(f"rt_scene_create, parent build   {med(co)}")
        for amp in new[0]["update"]:
            u = [r["update"][amp] for r in new]
            wall = [x["wall_ms"] for x in u]
            ref = statistics.median(co or cn)
            lines.append(f"rt_scene_update amplitude {amp:>4}  {med(wall)}   create / update = {ref / statistics.median(wall):.2f}"
                         f"   device bounds {u[0]['bounds_on_device']}")
            lines.append("    phases: " + "  ".join(f"{k[:-3]} {med([x[k] for x in u]).strip()}" for k in
                                                    ("prep_ms", "boxes_ms", "records_ms", "upload_ms", "refit_ms", "total_ms")))
        lines.append("traversal, 1920x1080, render kernels' device ms (updated scene | fresh scene of the same geometry):")
        for amp in new[0]["traverse"]:
            t = [r["traverse"][amp] for r in new]
            lines.append(f"  amplitude {amp:>4}: SAH {t[0]['sah_updated']:.2f} | {t[0]['sah_fresh']:.2f}")
            for key in ("primary", "full"):
                a, b = [x[key + "_updated_ms"] for x in t], [x[key + "_fresh_ms"] for x in t]
                lines.append(f"    {key:8s} {med(a)} | {med(b)}   ratio {statistics.median(a) / statistics.median(b):.3f}")
    if (args.bench or args.only_bench) and args.parent_lib:
        new, old = [], []
        for _ in range(args.rounds):
            old.append(run_bench(args.parent_lib, args.bench_steps))
            new.append(run_bench(None, args.bench_steps))
        lines.append("\n== bench.py, parent build | this build (alternating) ==")
        for k, unit in (("c3", "Mrays/s"), ("c2", "Mrays/s"), ("c5", "Mrays/s"), ("setup_s", "s scene setup")):
            lines.append(f"  {k:8s} {med([r[k] for r in old])} | {med([r[k] for r in new])}  {unit}")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.only_bench else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
