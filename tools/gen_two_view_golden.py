#!/usr/bin/env python3
"""Writes tests/golden/two_view_ref.npz: for every family case of tests/two_view_cases.py whose model run passes the cheirality
gate, what the reference's COMPILED code computes from the model's (R, t) and inputs (tools/gen_two_view_golden.cpp linked
against oracle/_ref/math_utils.o).  Runs only where the reference tree is; the test reads the fixture alone.

    python tools/gen_two_view_golden.py --reference <root of the reference tree>
"""
import argparse
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import two_view_cases as C  # noqa: E402
import two_view_reference as M  # noqa: E402


def build(reference, out):
    svo, jni = os.path.join(reference, "app/src/main/cpp/svo"), os.path.join(reference, "app/src/main/jniLibs")
    obj = os.path.join(ROOT, "oracle", "_ref", "math_utils.o")
    if not os.path.exists(obj):
        raise SystemExit("%s is missing: run build() first" % obj)
    subprocess.check_call(["g++", "-O2", "-std=c++11", "-I" + os.path.join(svo, "include"), "-I" + jni,
                           "-I" + os.path.join(jni, "OpenCV-android-sdk/sdk/native/jni/include"),
                           os.path.join(ROOT, "tools", "gen_two_view_golden.cpp"), obj, "-o", out])


def run_case(gen, tmp, c, r):
    n, pts = r["n_in"], np.ascontiguousarray(r["point_index"], np.int32)
    T = M.IDENTITY if c["T_ref_w"] is None else c["T_ref_w"]
    p = c["params"]
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        f.write(struct.pack("<2i22d", n, len(pts), *r["R"], *r["t"], C.FX, p["reproj_thresh"], p["map_scale"], *T))
        f.write(np.ascontiguousarray(c["f_cur"]).tobytes() + np.ascontiguousarray(c["f_ref"]).tobytes() + pts.tobytes())
    subprocess.check_call([gen, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
    b = open(os.path.join(tmp, "out.bin"), "rb").read()
    o = 0

    def take(dtype, count):
        nonlocal o
        a = np.frombuffer(b, dtype, count, o).copy()
        o += a.nbytes
        return a
    out = dict(xyz=take(np.float64, 3 * n).reshape(n, 3))
    out["inliers"] = take(np.int32, int(take(np.int32, 1)[0]))
    out["outliers"] = take(np.int32, int(take(np.int32, 1)[0]))
    has_nan = bool(np.isnan(out["xyz"][:, 2]).any())
    if not has_nan:
        out["median"] = take(np.float64, 1)
    out["quaternion"] = take(np.float64, 4)
    if not has_nan:
        out["T_cur_w"], out["T_world_cur"] = take(np.float64, 7), take(np.float64, 7)
        out["pos"] = take(np.float64, 3 * len(pts)).reshape(-1, 3)
    assert o == len(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "two_view_ref.npz"))
    a = ap.parse_args()
    arrays = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen = os.path.join(tmp, "gen_two_view_golden")
        build(a.reference, gen)
        for name in C.NAMES:
            r = C.model(name)
            if r["xyz_in_cur"] is None:
                continue
            for k, v in run_case(gen, tmp, C.case(name), r).items():
                arrays["%s/%s" % (name, k)] = v
    np.savez_compressed(a.out, **arrays)
    print("%s: %d arrays, %d bytes" % (a.out, len(arrays), os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
