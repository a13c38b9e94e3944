"""Child process of test_wide4_variant_reads_the_permutation (tests/test_gpu_ray_streams.py): loads the library
named by RTAMD_LIB (lib/librtamd_variants.so) and traces 257 rays through rt_trace_stream with the default
kernels in order, then with variant 2 (the quantised 4-wide tree's packets, rt_variants.hip) in order and
reordered. Prints one JSON line: {"differing": [cases], "reordered": the permutation was not the identity}.
Not a test module (no test_ functions); needs a GPU."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import conftest  # noqa: E402  (loads ray-tracing-project_amd/rtamd.py, honouring RTAMD_LIB)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from conftest import scene_path  # noqa: E402


def main():
    rt = conftest.rtamd
    assert os.path.basename(rt.LIB_PATH).startswith("librtamd_variants"), rt.LIB_PATH
    # a host SBVH scene: it also carries the quantised 4-wide tree the variant walks
    sc = rt.Scene(rt.Mesh.load_obj(scene_path("cornell.obj")), builder=rt.RT_BUILDER_SBVH)
    rng = np.random.default_rng(7)
    n = 257
    o = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    d = rng.uniform(-0.3, 0.3, (n, 3)).astype(np.float32) - o
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()

    def run(query, reorder):
        lights = rt.DEFAULT_LIGHTS if query == rt.RT_RAYS_COLOR else None
        res = sc.trace_stream(query, to, td, lights=lights, reorder=reorder)
        return {k: v.cpu().numpy().tobytes() for k, v in res.items()}

    queries = (rt.RT_RAYS_CLOSEST, rt.RT_RAYS_SHADOW, rt.RT_RAYS_COLOR)
    want = {q: run(q, False) for q in queries}
    differing, moved = [], False
    prev = rt.set_variant(2)
    try:
        for q in queries:
            for reorder in (False, True):
                if run(q, reorder) != want[q]:
                    differing.append([q, int(reorder)])
                if reorder:
                    moved = moved or bool((sc.ray_order() != np.arange(n)).any())
    finally:
        rt.set_variant(prev)
    print(json.dumps({"differing": differing, "reordered": moved}), flush=True)


if __name__ == "__main__":
    main()
