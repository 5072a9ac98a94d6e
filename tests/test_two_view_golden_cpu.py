"""The pin of tests/two_view_reference.py to the reference's COMPILED code: tests/golden/two_view_ref.npz holds, for every family
case whose model run passes the cheirality gate, what vk::computeInliers (xyz, inliers, outliers), vk::getMedian of the depths,
Eigen's Quaterniond(R) and the SE3 products and inverse of S/initialization.cpp:108-125 with the point positions return for the
model's (R, t) and inputs (tools/gen_two_view_golden.py, run where the reference tree is).  The model's values must be
bit-equal.  This test reads the fixture alone.  One omission: the depth median, and what follows from it, of the two cases with
a NaN depth (median-nan, border-singular) -- nth_element has no defined answer there."""
import os

import numpy as np
import pytest

import two_view_cases as C
import two_view_reference as M

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "two_view_ref.npz"))
PINNED = sorted({k.split("/")[0] for k in GOLD.files})


def bits(a):
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def test_the_fixture_covers_every_case_with_a_pose():
    assert PINNED == sorted(n for n in C.NAMES if C.model(n)["xyz_in_cur"] is not None) and len(PINNED) >= 25
    assert [n for n in PINNED if n + "/median" not in GOLD.files] == ["border-singular", "median-nan"]


@pytest.mark.parametrize("name", PINNED)
def test_model_equals_the_compiled_reference_by_bits(name):
    c, r = C.case(name), C.model(name)
    g = {k.split("/")[1]: GOLD[k] for k in GOLD.files if k.startswith(name + "/")}
    np.testing.assert_array_equal(bits(r["xyz_in_cur"]), bits(g["xyz"]))
    inl = M.compute_inliers(list(r["R"]), list(r["t"]), c["f_cur"], c["f_ref"], c["params"]["reproj_thresh"], C.FX)[1]
    np.testing.assert_array_equal(np.nonzero(inl)[0], g["inliers"])
    np.testing.assert_array_equal(np.nonzero(~inl)[0], g["outliers"])
    np.testing.assert_array_equal(bits(r["T_cur_from_ref"][3:]), bits(g["quaternion"]))
    if "median" not in g:
        return
    assert bits(r["depth_median"])[()] == bits(g["median"])[0]
    if r["status"] == M.OK:
        np.testing.assert_array_equal(r["inliers"], g["inliers"])
        np.testing.assert_array_equal(bits(r["T_cur_w"]), bits(g["T_cur_w"]))
        np.testing.assert_array_equal(bits(r["point_pos"]), bits(g["pos"]))
        T_cur_w, T_world_cur = M.second_pose(list(r["T_cur_from_ref"]), list(r["T_ref_w"]), r["scale"])
        np.testing.assert_array_equal(bits(np.array(T_world_cur)), bits(g["T_world_cur"]))
