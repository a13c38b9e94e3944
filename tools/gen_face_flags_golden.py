#!/usr/bin/env python3
"""Writes tests/golden/face_flags.npz: the per-face flag bits (safe normal, box certificate) and the certificate
range of host-only scenes -- cornell, the tie scene, the material scene, the bunny, each at its original vertices
and after every step of tests/update_scenes.py -- as the loaded library computes them. Generated once from the
build before the flag arithmetic moved into the shared RT_HD functions (rt_faceflags.h); RTAMD_LIB selects the
library. tests/test_update_device_host.py holds every later build to it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import update_scenes as U  # noqa: E402
from conftest import rtamd as rt  # noqa: E402


def flags_of(rt, name):
    arr, M, seq = U.scene_steps(rt, name)
    out = []
    for v in [None] + list(seq):
        sc = rt.Scene(U.mesh_of(rt, arr, v), device=-2, shape_model_matrix=M, builder=rt.RT_BUILDER_SAH)
        ff, ro = sc.face_flags()
        out.append(((ff >> 30).astype(np.uint8), np.float32(ro)))
    return out


def main():
    rt.lib()
    data = {}
    for name in U.SCENES:
        for k, (ff, ro) in enumerate(flags_of(rt, name)):
            data[f"{name}_{k}_flags"] = ff
            data[f"{name}_{k}_ro"] = np.array([ro], np.float32)
    path = os.path.join(ROOT, "tests", "golden", "face_flags.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
