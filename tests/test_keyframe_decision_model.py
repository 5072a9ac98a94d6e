"""The numpy models of the keyframe decision (tests/keyframe_decision_reference.py: frame_utils::getSceneDepth with vk::getMedian,
FrameHandlerMono::needNewKf, Map::getFurthestKeyframe) on the CPU: their own properties on seeded input families, and -- the pin to
the library routine the reference calls -- the same inputs through the C++ twins of android_svo_amd/host/svo_host.h in a small
stand-alone host program (tests/host_mock/keyframe_decision_twin.cpp, plain g++, no device) whose std::nth_element median,
minimum, needNewKf answer and furthest keyframe have to equal the models' exactly."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import keyframe_decision_reference as kd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEDIAN_COUNTS = (1, 2, 3, 4, 5, 8, 9, 64, 65, 257)


def _bits(v):
    return struct.pack("<d", float(v))


# ---- the median and the minimum
@pytest.mark.parametrize("kind", ["random", "duplicates", "equal", "behind"])
@pytest.mark.parametrize("n", MEDIAN_COUNTS)
def test_scene_depth_is_the_upper_median_and_the_minimum(n, kind):
    tables, T, feat = kd.depth_case(n, kind)
    got_n, n_nan, mean, dmin = kd.scene_depth(tables, T, feat)
    z = np.array([kd.synth.se3_act(T, tables["pt_pos"][p])[2] for p in feat if p >= 0])
    assert (got_n, n_nan) == (n, 0) and len(feat) > n                               # point-less features are interleaved
    below, above = int((z < mean).sum()), int((z > mean).sum())
    assert below <= n // 2 < n - above                                              # the element of rank n // 2
    assert mean in z and dmin == z.min()
    if n % 2 == 0 and kind == "random":
        assert mean > np.sort(z)[n // 2 - 1]                                        # the UPPER median
    if kind == "equal":
        assert mean == dmin == 2.5
    if kind == "duplicates" and n >= 4:
        s = np.sort(z)
        assert s[n // 2 - 1] == s[n // 2] == mean and (n // 2 + 1 >= n or s[n // 2 + 1] == mean)    # equal depths straddle the rank
    if kind == "behind" and n >= 8:
        assert dmin < 0.0


def test_scene_depth_without_a_depth_and_with_a_nan():
    tables, T, _ = kd.depth_case(3, "random")
    n, n_nan, mean, dmin = kd.scene_depth(tables, T, np.array([-1, -1], np.int32))
    assert (n, n_nan) == (0, 0) and math.isnan(mean) and dmin == kd.DBL_MAX
    tables, T, feat = kd.depth_case(9, "nan")
    n, n_nan, mean, dmin = kd.scene_depth(tables, T, feat)
    assert (n, n_nan) == (8, 1) and math.isnan(mean) and 0.5 < dmin < 4.5
    assert kd.need_new_kf(tables, T, [0], mean, 0.12) == (1, -1)                    # a NaN depth compares false: a new keyframe


# ---- needNewKf
def test_need_new_kf_families():
    seen = set()
    for name, tables, T, overlap, depth, d, want in kd.overlap_families():
        got = kd.need_new_kf(tables, T, overlap, depth, d)
        assert got == want, name
        seen.add(got[0])
        # which axes are inside the box, for the keyframe that decides (or the only one)
        if "decides alone" in name:
            r = np.abs(kd.rel_pos(tables, T, overlap[0])) / depth
            inside = [r[0] < d, r[1] < d * 0.8, r[2] < d * 1.3]
            assert inside.count(False) == 1 and inside.index(False) == "xyz".index(name[0]), name
    assert seen == {0, 1}


def test_the_flip_distance_brackets_the_answer():
    name, tables, T, overlap, depth, d, want = [f for f in kd.overlap_families() if f[0] == "inside, first blocks"][0]
    flip = kd.flip_distance(tables, T, overlap[0], depth)
    lo, hi = np.nextafter(flip, -np.inf), np.nextafter(np.nextafter(flip, np.inf), np.inf)
    assert kd.need_new_kf(tables, T, overlap, depth, lo)[0] == 1 and kd.need_new_kf(tables, T, overlap, depth, hi) == (0, 0)


# ---- the furthest keyframe
def test_furthest_keyframe_tie_and_none():
    tables, T = kd.tie_map()
    pos = kd.frame_pos(T)
    d = [float(np.linalg.norm(kd.frame_pos(Tk) - pos)) for Tk in tables["T_kf_w"]]
    assert d[1] == d[3] == 2.0 == max(d)                                            # an exact tie, on every machine
    assert kd.furthest_keyframe(tables, pos) == (1, 2.0)                            # the lower index wins
    tables, T = kd.coincident_map()
    assert kd.furthest_keyframe(tables, kd.frame_pos(T)) == (-1, 0.0)
    for n_kf in (1, 2, 64, 65):
        assert kd.furthest_keyframe(kd.line_map(n_kf), np.array([-0.5, 0.0, 0.0])) == (n_kf - 1, 0.5 + 0.25 * (n_kf - 1))


# ---- against the C++ twins
def _hex(v):
    return "nan" if v != v else float(v).hex()


def _write_case(fh, name, tables, T, feat, overlap, ask_depth, min_dist):
    pos, Tk = np.asarray(tables["pt_pos"]).reshape(-1, 3), np.asarray(tables["T_kf_w"]).reshape(-1, 7)
    fh.write("case %s\nT %s\n" % (name, " ".join(_hex(v) for v in T)))
    fh.write("points %d %s\n" % (len(pos), " ".join(_hex(v) for v in pos.ravel())))
    fh.write("features %d %s\n" % (len(feat), " ".join(str(int(p)) for p in feat)))
    fh.write("keyframes %d %s\n" % (len(Tk), " ".join(_hex(v) for v in Tk.ravel())))
    fh.write("overlap %d %s\n" % (len(overlap), " ".join(str(int(k)) for k in overlap)))
    fh.write("decide %s %s\n" % (_hex(ask_depth), _hex(min_dist)))


def _twin_cases():
    """[(name, tables, T, feat, overlap, depth asked with, min_dist)]"""
    cases = []
    for kind in ("random", "duplicates", "equal", "behind"):
        for n in MEDIAN_COUNTS:
            tables, T, feat = kd.depth_case(n, kind)
            cases.append(("depth_%s_%d" % (kind, n), tables, T, feat, [0], kd.scene_depth(tables, T, feat)[2], 0.12))
    tables, T, _ = kd.depth_case(3, "random")
    cases.append(("no_depth", tables, T, np.array([-1, -1, -1], np.int32), [], 2.0, 0.12))
    for i, (name, tables, T, overlap, depth, d, want) in enumerate(kd.overlap_families()):
        cases.append(("overlap_%d" % i, tables, T, np.array([0], np.int32), overlap, depth, d))
        if want[0] == 0:                                                            # ... and both sides of its flip
            flip = kd.flip_distance(tables, T, want[1], depth)
            earlier = overlap[:overlap.index(want[1])]
            if all(kd.flip_distance(tables, T, k, depth) > flip for k in earlier):
                cases.append(("overlap_%d_below" % i, tables, T, np.array([0], np.int32), overlap, depth, float(np.nextafter(flip, -np.inf))))
                cases.append(("overlap_%d_above" % i, tables, T, np.array([0], np.int32), overlap, depth,
                              float(np.nextafter(np.nextafter(flip, np.inf), np.inf))))
    for name, (tables, T) in (("tie", kd.tie_map()), ("coincident", kd.coincident_map())):
        cases.append((name, tables, T, np.array([0], np.int32), [], 2.0, 0.12))
    for n_kf in (1, 2, 64, 65):
        cases.append(("line_%d" % n_kf, kd.line_map(n_kf), np.array([0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), np.array([0], np.int32), [n_kf - 1], 2.0, 0.12))
    return cases


def test_the_models_equal_the_cpp_twins(tmp_path):
    exe, txt = tmp_path / "keyframe_decision_twin", tmp_path / "cases.txt"
    src = os.path.join(ROOT, "tests", "host_mock", "keyframe_decision_twin.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), src, "-o", str(exe), "-lpthread"])
    cases = _twin_cases()
    with open(txt, "w") as fh:
        for c in cases:
            _write_case(fh, *c)
    r = subprocess.run([str(exe), str(txt)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == len(cases) >= 50
    needs, blocked_later, flips = set(), False, 0
    for line, (name, tables, T, feat, overlap, depth, d) in zip(lines, cases):
        w = line.split()
        want = kd.decision(tables, T, feat, overlap, d)
        need, blocking = kd.need_new_kf(tables, T, overlap, depth, d)
        assert w[0] == name
        assert (int(w[1]), int(w[2])) == (1 if want["n_depths"] else 0, want["n_depths"]), name
        if want["n_depths"]:
            assert bytes.fromhex(w[3])[::-1] == _bits(want["depth_mean"]), (name, "the std::nth_element median")
        assert bytes.fromhex(w[4])[::-1] == _bits(want["depth_min"]), (name, "the minimum")
        assert (int(w[5]), int(w[6])) == (need, blocking), (name, "needNewKf")
        assert int(w[7]) == want["furthest_kf"], (name, "the furthest keyframe")
        assert bytes.fromhex(w[8])[::-1] == _bits(want["furthest_distance"]), (name, "its distance")
        needs.add(need)
        blocked_later = blocked_later or (need == 0 and overlap.index(blocking) > 0)
        flips += name.endswith("_below") and need == 1
        flips += name.endswith("_above") and need == 0
    assert needs == {0, 1} and blocked_later and flips >= 4
