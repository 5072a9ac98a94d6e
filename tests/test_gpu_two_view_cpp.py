"""svo_host_demo `bootstrap`: lists from files -> svo::initialization::KltInit::setLists / addSecondFrame (two-view on the device, the
second frame's pose, Points and Features in both frames in the order of S/initialization.cpp:117-138) -> the twin map's flatten,
against the same case through the Python mirror (hip.KltTracker.set_lists / two_view / map_tables): result, inlier list, xyz and
every table byte-equal.  One OK case with a non-identity T_ref_w and map_scale 0.5, and one case the FEW_INLIERS gate stops."""
import os
import subprocess

import numpy as np
import pytest

import two_view_cases as C
import two_view_reference as M
from test_gpu_host_cpp import DEMO
from test_gpu_two_view import CAM, new_handle, set_case
from android_svo_amd import hip

pytestmark = pytest.mark.gpu

TABLES = dict(kf_slot=np.int32, T_kf_w=np.float64, kf_key_point=np.int32, kf_ftr_offset=np.int32, kf_ftr_point=np.int32, pt_pos=np.float64,
              pt_type=np.int32, pt_n_failed=np.int32, pt_n_succeeded=np.int32, pt_obs_offset=np.int32, obs_kf=np.int32, obs_px=np.float64,
              obs_f=np.float64, obs_level=np.int32, obs_edgelet=np.uint8, obs_grad=np.float64, cand_point=np.int32)


@pytest.mark.parametrize("name", ["pose-0.5", "gates-39"])
def test_cpp_bootstrap_equals_the_python_mirror(tmp_path, name):
    assert os.path.exists(DEMO), "build() must have produced android_svo_amd/host/svo_host_demo"
    case, out = tmp_path / "case", tmp_path / "out"
    case.mkdir(); out.mkdir()
    c, p = C.case(name), C.case(name)["params"]
    T = M.IDENTITY if c["T_ref_w"] is None else c["T_ref_w"]
    meta = [C.W, C.H, C.FX, C.FY, C.CX, C.CY, len(c["f_ref"]), p["reproj_thresh"], p["min_inliers"], p["map_scale"], p["n_hypotheses"], p["seed"]]
    np.array(meta + list(T), dtype=np.float64).tofile(case / "boot_meta.bin")
    for k in ("px_ref", "px_cur", "f_ref", "f_cur"):
        np.ascontiguousarray(c[k]).tofile(case / ("boot_%s.bin" % k))
    r = subprocess.run([DEMO, str(case), str(out), "bootstrap"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bootstrap OK" in r.stdout, r.stdout + r.stderr
    got = np.fromfile(out / "boot_results.bin", np.float64)

    ctx = hip.Context(0)
    klt = new_handle(ctx, 1)
    try:
        set_case(klt, 0, c)
        res = klt.two_view([0], [CAM], np.asarray(T)[None], **p)[0]
        dl = klt.download_two_view(0)
        ok = res["status"] == hip.TWO_VIEW_OK
        assert ok == (name == "pose-0.5")
        want = np.concatenate([[2.0 if ok else 0.0, res["status"], res["n_inliers"], res["n_points"], res["depth_median"], res["scale"]],
                               res["T_cur_from_ref"], res["T_cur_w"]])
        assert got.tobytes() == want.tobytes() or (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(got)] == want[~np.isnan(want)]).all()
        assert np.fromfile(out / "boot_inliers.bin", np.int32).tobytes() == dl["inliers"].tobytes()
        assert np.fromfile(out / "boot_xyz_in_cur.bin", np.float64).tobytes() == dl["xyz_in_cur"].tobytes()
        if ok:
            mp = klt.map_tables(0, res, T)
            assert res["n_points"] > 100
            for key, dt in TABLES.items():
                assert np.fromfile(out / ("boot_%s.bin" % key), dt).tobytes() == np.ascontiguousarray(mp[key], dt).tobytes(), key
        else:                                                    # a failure: an empty map
            for key, dt in TABLES.items():
                assert len(np.fromfile(out / ("boot_%s.bin" % key), dt)) == (1 if key in ("kf_ftr_offset", "pt_obs_offset") else 0), key
    finally:
        klt.destroy()
        ctx.close()
