"""Child process of test_variants_library_renders_identical_bits (tests/test_gpu_parity.py): loads the
library named by RTAMD_LIB (lib/librtamd_variants.so: the product kernels plus the A/B kernels of
rt_variants.hip) and renders, for every A/B variant, bunny (PRIMARY + FULL, 1080p) and the 1M soup (FULL
640x360, PRIMARY 1000x563) and the 64x40 frame of the tie scene (tests/edge_scenes.py: three faces at
bit-identical t under every pixel; PRIMARY + FULL) and of the normal scene (explicit vertex normals whose blend
is the zero vector, NaN or unnormalised: every A/B kernel's own accept path must reject and accept as the default
kernels do; PRIMARY + FULL) and the 64x64 frame of the limit scene (tests/deep_scenes.py: the PLOC chain at
bvh_depth 62, from the deep-tree battery's camera, every pixel's ray crossing the whole chain: the VGPR stack's 64
lanes and the lane kernels' kMaxDepth + 4 private entries at their fullest; PRIMARY + FULL) with the default kernels
and with the variant. Prints one JSON line:
{variant name: [differing cases]}. Not a test module (no test_ functions); needs a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import conftest  # noqa: E402  (loads ray-tracing-project_amd/rtamd.py, honouring RTAMD_LIB)
import deep_scenes  # noqa: E402
import edge_scenes  # noqa: E402
from conftest import scene_path  # noqa: E402
from kernel_variants import VARIANTS_LIB  # noqa: E402
from test_gpu_parity import variant_frames_identical  # noqa: E402


def main():
    rt = conftest.rtamd
    assert os.path.basename(rt.LIB_PATH).startswith("librtamd_variants"), rt.LIB_PATH
    # host SBVH scenes: they also carry the quantised 4-wide tree the W4 variant walks (the device builders
    # build the binary tree only, and a variant without its tree would render with the default kernels)
    bunny = rt.Scene(rt.Mesh.load_obj(scene_path("bunny.obj")), builder=rt.RT_BUILDER_SBVH)
    mesh, _, _ = rt.soup_mesh(1_000_000)
    soup = rt.Scene(mesh, builder=rt.RT_BUILDER_SBVH)
    (v, f, m, g), _ = edge_scenes.tie_scene()
    tie = rt.Scene(rt.Mesh.from_arrays(v, f, m, groups=g), builder=rt.RT_BUILDER_SBVH, min_faces=8)
    (v, f, m, g), vn, _ = edge_scenes.normal_scene()
    normal = rt.Scene(rt.Mesh.from_arrays(v, f, m, vn3=vn, groups=g), builder=rt.RT_BUILDER_SBVH, min_faces=8)
    v, f, m, g = deep_scenes.spine()
    deep_mesh = rt.Mesh.from_arrays(v, f, m, groups=g)
    deep = rt.Scene(deep_mesh, builder=rt.RT_BUILDER_PLOC_GPU, leaf_size=1, min_faces=8)
    assert deep.info()["builder"] == rt.RT_BUILDER_PLOC_GPU and deep.info()["bvh_depth"] == deep_scenes.MAX_DEPTH, deep.info()
    dW, dH = deep_scenes.FRAME
    at = deep_scenes.camera_args(deep_mesh.export(), dW, dH)[2:]
    extra = [(tie, 64, 40, rt.RT_MODE_PRIMARY), (tie, 64, 40, rt.RT_MODE_FULL),
             (normal, 64, 40, rt.RT_MODE_PRIMARY), (normal, 64, 40, rt.RT_MODE_FULL),
             (deep, dW, dH, rt.RT_MODE_PRIMARY, at), (deep, dW, dH, rt.RT_MODE_FULL, at)]
    out = {}
    for name, bits in sorted(VARIANTS_LIB.items()):
        out[name] = [list(map(int, c[:3])) for c in variant_frames_identical(rt, (bunny, soup), bits, extra)]
        print(f"{name}: {'identical' if not out[name] else out[name]}", file=sys.stderr, flush=True)
    # the FULL stage pipeline (variant 16) sizes its ray lists for whole frames: a sharded frame is refused
    # with an error, never rendered wrong
    prev = rt.set_variant(16)
    try:
        cam = rt.flycam(256, 256, 0, 0, 20)
        try:
            bunny.render(cam, rt.DEFAULT_LIGHTS, 256, 256, mode=rt.RT_MODE_FULL, shard=(0, 2))
            out["_pipeline_shard_refused"] = [[0]]
        except rt.RTError as e:
            out["_pipeline_shard_refused"] = [] if "whole frames only" in str(e) else [[1]]
    finally:
        rt.set_variant(prev)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
