"""The host twin of the two-view kernels (tests/host_mock/two_view_twin.cpp: the functions of csrc/svo_two_view_math.h that the
kernels call, run serially by g++ with -ffp-contract=off) against the numpy model on every family case, BY BITS: result
block, hypothesis counts, mask, inlier list, xyz, points.  Built plain and with the address / undefined-behaviour sanitizers
(a stand-alone program)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import two_view_cases as C
import two_view_reference as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_case(path, c):
    p, n = c["params"], len(c["f_ref"])
    T = M.IDENTITY if c["T_ref_w"] is None else c["T_ref_w"]
    with open(path, "wb") as f:
        f.write(struct.pack("<6iQ10d", n, C.W, C.H, p["n_hypotheses"], p["min_inliers"], 0, p["seed"], C.FX, p["reproj_thresh"], p["map_scale"], *T))
        for k in ("f_ref", "f_cur", "px_ref", "px_cur"):
            f.write(np.ascontiguousarray(c[k]).tobytes())


def read_result(path, n, n_hyp):
    b = open(path, "rb").read()
    head = struct.unpack_from("<8i16d", b, 0)
    r = dict(zip(("status", "n_in", "hypothesis", "hypothesis_count", "candidate", "candidate_count", "n_inliers", "n_points"), head[:8]))
    r["depth_median"], r["scale"], r["T_cur_from_ref"], r["T_cur_w"] = head[8], head[9], np.array(head[10:17]), np.array(head[17:24])
    o = 32 + 128

    def take(dtype, count):
        nonlocal o
        a = np.frombuffer(b, dtype, count, o)
        o += a.nbytes
        return a
    r["counts"] = take(np.int32, n_hyp if r["status"] != M.TOO_FEW else 0)
    r["mask"] = take(np.uint8, n)
    r["inliers"] = take(np.int32, r["n_inliers"])
    r["xyz_in_cur"] = take(np.float64, 3 * n).reshape(n, 3) if r["status"] in (M.OK, M.FEW_INLIERS) else None
    r["point_index"] = take(np.int32, r["n_points"])
    r["point_pos"] = take(np.float64, 3 * r["n_points"]).reshape(-1, 3)
    assert o == len(b)
    return r


def bits(a):
    """the bit patterns; every NaN counts as the same NaN (its sign and payload are the processor's choice)"""
    a = np.ascontiguousarray(a, np.float64)
    return np.where(np.isnan(a), np.uint64(0x7FF8000000000000), a.view(np.uint64))


def assert_equal_by_bits(got, want):
    for k in ("status", "n_in", "hypothesis", "hypothesis_count", "candidate", "candidate_count", "n_inliers", "n_points"):
        assert got[k] == want[k], k
    for k in ("depth_median", "scale", "T_cur_from_ref", "T_cur_w", "point_pos"):
        np.testing.assert_array_equal(bits(got[k]), bits(want[k]), err_msg=k)
    for k in ("counts", "mask", "inliers", "point_index"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    assert (got["xyz_in_cur"] is None) == (want["xyz_in_cur"] is None)
    if want["xyz_in_cur"] is not None:
        np.testing.assert_array_equal(bits(got["xyz_in_cur"]), bits(want["xyz_in_cur"]))


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_twin_equals_the_model_by_bits(tmp_path, flags):
    exe = tmp_path / "two_view_twin"
    src = os.path.join(ROOT, "tests", "host_mock", "two_view_twin.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unknown-pragmas", *flags, src, "-o", str(exe)])
    names = C.NAMES if flags == ["-O2"] else ["volume-65", "outliers-200-45-0.3", "gates-39", "border", "median-nan", "pose-0.5", "gates-n7",
                                             "gates-identical", "degenerate-rotation"]
    args = []
    for i, name in enumerate(names):
        write_case(tmp_path / ("c%d.bin" % i), C.case(name))
        args += [str(tmp_path / ("c%d.bin" % i)), str(tmp_path / ("r%d.bin" % i))]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "two view twin OK" in r.stdout
    for i, name in enumerate(names):
        c = C.case(name)
        got = read_result(tmp_path / ("r%d.bin" % i), len(c["f_ref"]), c["params"]["n_hypotheses"])
        try:
            assert_equal_by_bits(got, C.model(name))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e))
