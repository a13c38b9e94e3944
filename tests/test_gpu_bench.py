"""bench.py as later measurements run it (MI355X): a plain run times its frames and nothing else, and
--dump-outputs writes the frame of the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def test_plain_run_is_lean_and_dumps_its_last_frame(rt, tmp_path):
    """One plain run of a small workload (20,000 triangles, a 200x120 frame: a partial tile row): the line has the
    headline figures of exactly the steps asked for and none of the --full legs; DIR/rgb.npy is the float32 frame
    a caller downloads, bit for bit the library's render of the same scene and camera in this process."""
    # (2050 steps: one more drain than the library's 2048 renders between synchronisations allow in one go)
    W, H, tris, steps = 200, 120, 20000, 2050
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--tris", str(tris), "--frame", f"{W}x{H}", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == 1 and d["n_gpus"] == 1 and d["full"] is False
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    # value = the frame's rays x steps over the timed window, ms_per_step = that window / steps
    assert d["value"] == pytest.approx(W * H / (d["ms_per_step"] * 1e-3) / 1e6, rel=2e-2)
    assert d["roofline"] is None and d["cpu_baseline"] is None
    for leg in ("cold", "moving_camera", "c4_frame", "c2", "c5", "parity", "parity_all_configs"):
        assert leg not in d, leg
    cfg = d["config"]
    assert cfg["kernel_ms_one_frame_alone"] is None and cfg["bvh_sah_cost"] is None and "e2e_frame_ms" not in cfg
    assert sorted(os.listdir(out)) == ["rgb.npy"] and d["dumped_outputs"]["files"] == {"rgb.npy": [H, W, 3]}
    got = np.load(out / "rgb.npy")
    assert got.dtype == np.float32 and got.shape == (H, W, 3)
    mesh, _, _ = rt.soup_mesh(tris, 12345)
    rgb, _ = rt.Scene(mesh).render(rt.flycam(W, H, 0, 0, 20), rt.DEFAULT_LIGHTS, W, H)
    assert got.tobytes() == rgb.tobytes()
    assert np.unique(got.reshape(-1, 3), axis=0).shape[0] > 100  # a picture, not a cleared buffer
