#!/usr/bin/env python3
"""Light-set measurement (MI355X): prints and writes profiles/ab/light_sets_ab.txt. All frames FULL at depth 2, 1000x1000
(the reference's window), one frame at a time; kernel time from HIP events on the scene's stream (rt_stats.kernel_ms).
Every figure is the median over a process's timed frames; every pairing alternates `--rounds` fresh processes of each
side -- after one discarded process, which meets the GPU's clocks ramping up out of idle -- and reports median
(min..max) over the processes.

  (a) soft lights: bunny and cornell under a spherical light of 99 and of 199 points plus the centre, radius 0.15
      (bunny: at the default light's place; cornell: inside the box), the memory-lights kernel with the wave-level
      occluder cache (the default) against the same kernel without it (variant 16777216); plus, untimed, the wave
      node / triangle record fetches of a counting frame of each. --alt NAME=LIB (repeatable) adds a side that runs
      the cached kernel of another build of the library, e.g. one compiled with another kOccK (rt_traverse.h);
      --scenes / --counts narrow the section
  (b) memory path against kernel arguments: 32 ring lights on the bunny through rt_render_lit, k_render_depth reading
      them from the kernel arguments (variant 65536), from memory without the cache (8388608 | 16777216) and from
      memory with it (8388608)
  (c) no regression of the default kernels: rt_render with 32 ring lights, this build against --parent LIB (a build
      of the parent commit), when given
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ray-tracing-project_amd"))
import rtamd as rt  # noqa: E402

W = H = 1000
MEM, NO_CACHE, GENERIC = rt.VARIANT_MEM_LIGHTS, rt.VARIANT_NO_OCCLUDER_CACHE, 65536
SOFT = {"bunny": ((-0.5, 2.0, 3.0), 0.15), "cornell": ((0.3, 0.45, 0.2), 0.15)}


def ring_lights(n, colour=0.05):
    """n point lights on two rings around the z axis in front of the scene (as tests/edge_scenes.py)"""
    out = []
    for k in range(n):
        th = 2 * np.pi * k / max(n, 1)
        rad, z = (2.0, 2.5) if k % 2 == 0 else (0.8, 1.5)
        out.append(((float(np.float32(rad * np.cos(th))), float(np.float32(rad * np.sin(th))), z),
                    (colour, colour * (0.6 + 0.4 * (k % 3) / 2), colour * (1.0 - 0.5 * (k % 4) / 3))))
    return out


def med(xs):
    return f"{statistics.median(xs):9.3f} ({min(xs):.3f}..{max(xs):.3f})"


def child(args):
    """one process, one configuration: a JSON line {ms: median kernel ms per frame, wnode, wtri}"""
    sc = rt.Scene(rt.Mesh.load_obj(os.path.join(ROOT, "scenes", args.scene + ".obj")))
    cam = rt.flycam(W, H)
    if args.points:
        pos, radius = SOFT[args.scene]
        lights = rt.spherical_light(pos, (1.0, 1.0, 1.0), radius, args.points)
    else:
        lights = ring_lights(32)
    rt.set_variant(args.variant)
    if args.array:  # rt_render, the array call (a parent build has nothing else)
        frame = lambda flags=0: sc.render(cam, lights, W, H, mode=rt.RT_MODE_FULL, flags=flags)[1]
    else:
        ls = sc.light_set(lights)
        frame = lambda flags=0: sc.render_lit(cam, ls, W, H, mode=rt.RT_MODE_FULL, flags=flags)[1]
    for _ in range(args.warmup):  # code objects, frame buffers, the longest-first order of lone frames
        frame()
    ms = [frame()["kernel_ms"] for _ in range(args.frames)]
    res = {"ms": statistics.median(ms), "lo": min(ms), "hi": max(ms)}
    if args.stats:
        st = frame(rt.RT_FRAME_STATS)
        res.update(wnode=st["wave_node_fetches"], wtri=st["wave_tri_fetches"], rays=st["total_rays"])
    print(json.dumps(res), flush=True)


def run_child(extra, lib=None):
    env = dict(os.environ)
    env.pop("RTAMD_LIB", None)
    if lib:
        env["RTAMD_LIB"] = lib
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + [str(x) for x in extra], env=env,
                       capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        sys.exit(f"light_sets_ab: child {extra} failed: {p.stderr[-1500:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def pairing(sides, rounds):
    """sides: [(label, child args, lib)]; alternating processes; returns {label: [result per round]}"""
    runs = {label: [] for label, _, _ in sides}
    run_child(sides[0][1], sides[0][2])  # discarded: the first process after the GPU sat idle runs at ramping clocks
    for _ in range(rounds):
        for label, extra, lib in sides:
            runs[label].append(run_child(extra, lib))
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5, help="processes per side of a pairing")
    ap.add_argument("--frames", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None, help="(c): a library built from the parent commit")
    ap.add_argument("--only", default="abc", help="which of the sections a, b, c to run")
    ap.add_argument("--alt", action="append", default=[], metavar="NAME=LIB", help="(a): another build's cached kernel")
    ap.add_argument("--scenes", default="bunny,cornell", help="(a): scenes")
    ap.add_argument("--counts", default="100,200", help="(a): lights per soft light")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ab", "light_sets_ab.txt"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--scene", default="bunny", help=argparse.SUPPRESS)
    ap.add_argument("--points", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--variant", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--array", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--stats", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if rt.device_count() == 0:
        sys.exit("light_sets_ab: no GPU (a measurement needs one)")
    if args.child:
        return child(args)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    common = ["--frames", args.frames, "--warmup", args.warmup]
    say(f"light sets A/B: {rt.lib().rt_version_string().decode()}; {W}x{H} FULL depth 2, one frame at a time, kernel ms "
        f"per frame (HIP events); per process the median of {args.frames} frames after {args.warmup} warm-up frames; "
        f"{args.rounds} alternating processes per side, median (min..max) over the processes")
    if "a" in args.only:
        say("(a) soft lights: memory-lights kernel with the occluder cache (K = 2) against the same kernel without it")
        wins = []
        alts = [tuple(x.split("=", 1)) for x in args.alt]
        for scene in args.scenes.split(","):
            for points in [int(x) - 1 for x in args.counts.split(",")]:
                base = ["--scene", scene, "--points", points, "--stats"] + common
                runs = pairing([("cache", base + ["--variant", 0], None), ("no cache", base + ["--variant", NO_CACHE], None)] +
                               [(name, base + ["--variant", 0], lib) for name, lib in alts], args.rounds)
                on, off = [r["ms"] for r in runs["cache"]], [r["ms"] for r in runs["no cache"]]
                c, u = runs["cache"][0], runs["no cache"][0]
                clear = max(on) < min(off)
                if points == 99 or "100" not in args.counts.split(","):
                    wins.append(clear)
                say(f"  {scene:8s} {points + 1:3d} lights: cache {med(on)} ms   no cache {med(off)} ms   "
                    f"no cache / cache = {statistics.median(off) / statistics.median(on):.3f}x"
                    f"{'' if clear else '   (ranges overlap)'}")
                for name, _ in alts:
                    ms = [r["ms"] for r in runs[name]]
                    a0 = runs[name][0]
                    say(f"      {name}: {med(ms)} ms   no cache / {name} = {statistics.median(off) / statistics.median(ms):.3f}x   "
                        f"wave node fetches {a0['wnode']}, wave triangle fetches {a0['wtri']}")
                say(f"      counting frame, {c['rays']} rays: wave node fetches {c['wnode']} vs {u['wnode']} "
                    f"({c['wnode'] / u['wnode']:.3f}x), wave triangle fetches {c['wtri']} vs {u['wtri']} ({c['wtri'] / u['wtri']:.3f}x)")
        say("  the cache is " + ("faster beyond the spread on both 100-light workloads" if all(wins)
                                 else "NOT faster beyond the spread on both 100-light workloads"))
    if "b" in args.only:
        say("(b) 32 ring lights on the bunny through rt_render_lit, all k_render_depth")
        base = ["--scene", "bunny"] + common
        runs = pairing([("kernel arguments (65536)", base + ["--variant", GENERIC], None),
                        ("memory, no cache (8388608 | 16777216)", base + ["--variant", MEM | NO_CACHE], None),
                        ("memory, cache (8388608)", base + ["--variant", MEM], None)], args.rounds)
        ref = [r["ms"] for r in runs["kernel arguments (65536)"]]
        for label, rs in runs.items():
            ms = [r["ms"] for r in rs]
            say(f"  {label:40s} {med(ms)} ms   / kernel arguments = {statistics.median(ms) / statistics.median(ref):.3f}x")
    if "c" in args.only and args.parent:
        say("(c) rt_render with 32 ring lights on the bunny, default kernels (k_render_full): parent build against this build")
        base = ["--scene", "bunny", "--array"] + common
        runs = pairing([("parent", base, args.parent), ("this build", base, None)], args.rounds)
        par, new = [r["ms"] for r in runs["parent"]], [r["ms"] for r in runs["this build"]]
        say(f"  parent {med(par)} ms   this build {med(new)} ms   this / parent = {statistics.median(new) / statistics.median(par):.3f}x")
        say("  this build's runs " + ("overlap the parent's range (or lie below it)" if min(new) <= max(par)
                                       else "lie ABOVE the parent's range"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.only != "abc" else "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
