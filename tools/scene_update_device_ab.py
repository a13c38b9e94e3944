#!/usr/bin/env python3
"""Device-resident update measurement (MI355X): prints and writes profiles/ab/scene_update_device_ab.txt.

A caller who deforms a mesh with torch on the GPU holds three device tensors per step (vertices [nv,4], vertex
normals, face normals). Per step of tests/update_scenes.py's sequence (small, large, back) on the bunny and the 1M
soup:
  host path    the three tensors copied to the host, then rt_scene_update on the parent commit's build
               (--parent-lib) -- what such a caller pays today -- and the same on this build (a regression pair);
  device path  rt_scene_update_device on this build, with its phase split from rt_update_stats.
Wall times are a host clock around the whole step (both paths end synchronised). Alongside, the usual regression
pairs against the parent build: rt_scene_create on both scenes, and (--bench) bench.py's C3 / C2 / C5.

Method as the other *_ab.py tools: one process per (scene, build) does every case and prints one JSON line; after
one discarded process, `--rounds` processes per side, alternating; the record gives median (min..max) over the
processes. No threshold is fixed in advance: the record says what was measured."""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rtamd as rt  # noqa: E402
import update_scenes as U  # noqa: E402  (the tests' scenes and deformation: one definition)

CHILD_TIMEOUT_S = 400  # a child process that takes longer has hung
F = np.float32
PHASES = ("prep_ms", "boxes_ms", "records_ms", "upload_ms", "refit_ms", "total_ms")


def med(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def scene_arrays(name):
    if name == "bunny":
        return U.obj_arrays(rt, os.path.join(ROOT, "scenes", "bunny.obj"))
    v = rt.generate_soup(1_000_000, 12345)
    f = np.arange(3 * 1_000_000, dtype=np.uint32).reshape(-1, 3)
    return v, f, np.array([rt.SOUP_MATERIAL], F), None


def timed(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    return (time.perf_counter() - t0) * 1e3, r


def child(args):
    arr = scene_arrays(args.scene)
    mesh0 = U.mesh_of(rt, arr)
    res = {"create_ms": [], "lib": os.path.basename(rt.LIB_PATH), "host": [], "device": []}
    rt.Scene(mesh0)  # the process's first scene pays the device's first use
    for _ in range(3):
        ms, sc = timed(lambda: rt.Scene(mesh0))
        res["create_ms"].append(ms)
    on_device = args.path == "device"  # one path per process: neither disturbs the other's caches and allocations
    steps = []
    for v in [U.deform(arr[0], 0.01)] + U.steps(arr):  # the first: each path's one-time uploads, not a step
        mesh = U.mesh_of(rt, arr, v)
        ex = mesh.export()
        steps.append((mesh, ex["M16"], [torch.from_numpy(np.ascontiguousarray(ex[k], F)).cuda() for k in ("v4", "vn3", "fn3")]))
    for k, (mesh, M, (tv, tvn, tfn)) in enumerate(steps):
        d = mesh.desc()  # topology, materials and matrix; the three coordinate arrays come from the device

        def host_step(stats):
            hv, hvn, hfn = tv.cpu().numpy(), tvn.cpu().numpy(), tfn.cpu().numpy()
            d.vertices, d.vertex_normals, d.face_normals = hv.ctypes.data, hvn.ctypes.data, hfn.ctypes.data
            st = rt.UpdateStats()
            rt.check(rt.lib().rt_scene_update(sc.h, C.byref(d), C.byref(st) if stats else None))
            return st.as_dict()

        if on_device:
            ms, _ = timed(lambda: sc.update_device(tv, tvn, tfn, model_matrix=M))  # stats = NULL: no SAH cost, no mirror
            _, st = timed(lambda: sc.update_device(tv, tvn, tfn, model_matrix=M, stats=True))
        else:
            ms, _ = timed(lambda: host_step(False))
            _, st = timed(lambda: host_step(True))
        if k:
            res[args.path].append({"wall_ms": ms, **{p: st[p] for p in PHASES}, "bounds_on_device": st["bounds_on_device"]})
    print(json.dumps(res), flush=True)


def run_child(scene, lib, path="host"):
    env = dict(os.environ)
    if lib:
        env["RTAMD_LIB"] = lib
    else:
        env.pop("RTAMD_LIB", None)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--scene", scene, "--path", path], env=env, check=True,
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
    ap.add_argument("--path", default="host", choices=("host", "device"), help="(child) the path this process measures")
    ap.add_argument("--scene", default="bunny")
    ap.add_argument("--scenes", default="bunny,soup")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-lib", required=False, help="librtamd.so of the parent commit")
    ap.add_argument("--bench", action="store_true", help="also bench.py on both builds, alternating")
    ap.add_argument("--only-bench", action="store_true", help="the bench.py section alone")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "scene_update_device_ab.txt"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    if not args.parent_lib:
        ap.error("--parent-lib is required")
    names = ("small", "large", "back")
    lines = [] if args.append else [
        "device-resident update A/B (tools/scene_update_device_ab.py): median (min..max) over %d alternating processes, ms" % args.rounds,
        "host path = three device tensors copied to the host + rt_scene_update; device path = rt_scene_update_device"]
    for scene in () if args.only_bench else [s for s in args.scenes.split(",") if s]:
        run_child(scene, None, "device")  # discarded
        new, old, devs = [], [], []
        for _ in range(args.rounds):  # the builds and paths alternate
            old.append(run_child(scene, args.parent_lib))
            new.append(run_child(scene, None))
            devs.append(run_child(scene, None, "device"))
        lines.append(f"\n== {scene} ==")
        lines.append(f"rt_scene_create              parent {med([statistics.median(r['create_ms']) for r in old])} | this build "
                     f"{med([statistics.median(r['create_ms']) for r in new + devs])}")
        for k, step in enumerate(names):
            ho = [r["host"][k] for r in old]
            hn = [r["host"][k] for r in new]
            dv = [r["device"][k] for r in devs]
            how, hnw, dw = ([x["wall_ms"] for x in xs] for xs in (ho, hn, dv))
            lines.append(f"step {step:5s} host path     parent {med(how)} | this build {med(hnw)}")
            lines.append("    host phases, parent:     " + "  ".join(f"{p[:-3]} {med([x[p] for x in ho]).strip()}" for p in PHASES))
            lines.append("    host phases, this build: " + "  ".join(f"{p[:-3]} {med([x[p] for x in hn]).strip()}" for p in PHASES))
            lines.append(f"step {step:5s} device path   this build {med(dw)}   parent host / device = "
                         f"{statistics.median(how) / statistics.median(dw):.2f}   device bounds {dv[0]['bounds_on_device']}")
            lines.append("    device phases:           " + "  ".join(f"{p[:-3]} {med([x[p] for x in dv]).strip()}" for p in PHASES))
    if args.bench or args.only_bench:
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
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
