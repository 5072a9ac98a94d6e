"""svo_host_demo `klt`: the bootstrap of three cameras (one radtan) through svo::initialization::KltInit (hip_bridge::KltInitT,
include/svo_dropin/klt_init_hip.h) -- camera 0's first frame detected on the device, the others from given features, then three
frames, each one device call for all cameras -- against the same schedule through hip.KltTracker: the lists of every camera
after every frame byte-equal, and the return codes the reference's gates give."""
import os
import subprocess

import numpy as np
import pytest

import klt_reference as K
from test_gpu_host_cpp import DEMO
from test_gpu_klt import _rig
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

W, H, N_CAMS = 346, 260, 3
GATES = dict(min_features=50, min_tracked=40, min_disparity=3.0)


def test_cpp_bootstrap_equals_the_python_mirror(tmp_path):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    first, _, px = K.gpu_case(W, H, 128, 11)
    images = [first]
    for s in [(1.7, -0.9), (3.9, -2.2), (6.5, -3.1)]:
        images.append(K.gpu_case(W, H, 24, 11, shift=s)[1])
    cams = _rig(W, H)
    meta = [W, H, N_CAMS, len(images), len(px), GATES["min_features"], GATES["min_tracked"], GATES["min_disparity"]]
    for c in cams:
        meta += [c.fx, c.fy, c.cx, c.cy] + list(getattr(c, "dist", (0.0,) * 5))
    np.array(meta, dtype=np.float64).tofile(case / "klt_meta.bin")
    np.stack(images).tofile(case / "klt_images.bin")
    px.tofile(case / "klt_px.bin")
    p = subprocess.run([DEMO, str(case), str(out), "klt"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "klt OK (3 cameras)" in p.stdout, p.stdout + p.stderr
    print(p.stdout)
    results = np.fromfile(out / "klt_results.bin", np.float64)

    ctx = hip.Context(0)
    pyr = hip.Pyramid(ctx, W, H, 3, len(images))
    pyr.upload_level0_batch_and_build(0, images)
    klt = hip.KltTracker(ctx, W, H, N_CAMS, 1024)
    try:
        f = np.stack([0.001 * px[:, 0].astype(np.float64), 0.001 * px[:, 1].astype(np.float64), np.ones(len(px))], axis=1)
        n_det = klt.set_reference_detected(0, pyr, 0, cams[0], 3, 20, 10.0)
        assert n_det >= GATES["min_features"]
        for c in (1, 2):
            klt.set_reference(c, pyr, 0, px, f)
        want = [2.0] * N_CAMS                                   # addFirstFrame: SUCCESS
        seen = set()
        for k in range(3):
            slots = [1 + (k + c) % 3 for c in range(N_CAMS)]
            res = klt.track(list(range(N_CAMS)), pyr, slots, cams)
            for c in range(N_CAMS):
                d = klt.download(c)
                for name, dt in (("px_ref", np.float32), ("px_cur", np.float32), ("f_ref", np.float64), ("f_cur", np.float64),
                                 ("disparity", np.float64), ("index", np.int32)):
                    got = np.fromfile(out / ("klt_c%d_k%d_%s.bin" % (c, k, name)), dt)
                    assert got.tobytes() == np.ascontiguousarray(d[name]).tobytes(), (c, k, name)
                med = res[c]["disparity_median"]
                code = 0.0 if d["n"] < GATES["min_tracked"] else 1.0 if med < GATES["min_disparity"] else 2.0
                want += [code, med]
                seen.add(code)
        np.testing.assert_array_equal(results, np.array(want))
        assert {1.0, 2.0} <= seen                               # NO_KEYFRAME and "on to computeFundamental" both occur
    finally:
        klt.destroy()
        pyr.destroy()
        ctx.close()
