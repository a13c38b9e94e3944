"""The fused PRIMARY kernel's two instantiations through the public API (MI355X): launch_frame gives a frame whose
scene has no 4-wide tree the binary-only instantiation and a frame whose scene has one the wide instantiation.
Which one ran is not observable through the API and is not asserted here (the choice is one condition on
DevScene::wide_copy_bytes, and the frame plan is deliberately unchanged); what is asserted is that scenes built
without and with the wide tree render the same frames -- equal digests of rgb, face ids and t -- in PRIMARY and
box-colours mode, with and without hit records."""
import hashlib

import numpy as np
import pytest

from conftest import scene_path

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def need_gpu(rt):
    if rt.device_count() == 0:
        pytest.skip("no GPU")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", ["bunny", "soup"])
def test_wide_and_binary_scenes_render_the_same_digests(rt, name):
    if name == "bunny":
        mesh = rt.Mesh.load_obj(scene_path("bunny.obj"))
    else:
        mesh = rt.soup_mesh(20_000)[0]
    plain, wide = rt.Scene(mesh, wide_tree=0), rt.Scene(mesh, wide_tree=1)
    for W, H in ((480, 270), (40, 24)):
        cam = rt.flycam(W, H, 0, 0, 20)
        for mode in (rt.RT_MODE_PRIMARY, rt.RT_MODE_BOX_COLORS):
            a = plain.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True)
            b = wide.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode, want_hits=True)
            assert [digest(x) for x in a[:3]] == [digest(x) for x in b[:3]], (name, W, H, mode)
            assert (np.asarray(a[1]) >= 0).any()
            c = plain.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode)
            d = wide.render(cam, rt.DEFAULT_LIGHTS, W, H, mode=mode)
            assert digest(c[0]) == digest(d[0]) == digest(a[0]), (name, W, H, mode, "no hit records")
