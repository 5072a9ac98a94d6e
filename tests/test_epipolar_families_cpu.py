"""The constructed families of tests/epipolar_families.py on the CPU oracle alone: the oracle's trace against its untraced
entry, the proof that every family reaches the path of the search kernel it is built for, and the proof that the cases can
tell a wrong kernel from a right one (four wrong search rules, computed from the trace, each change the outcome).
No GPU: the device side of the same families is tests/test_gpu_epipolar_search_paths.py."""
import copy
import ctypes

import numpy as np
import pytest

from android_svo_amd import seedsynth, synth
from oracle import orc

import epipolar_families as ef

FAMILY_NAMES = list(ef.FAMILIES)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_trace_against_untraced(cam, ref_pyr, cur_pyr, T_cur_ref, px, f, level, d_est, d_min, d_max, n_pyr_levels=3, max_steps=1000):
    kw = dict(n_pyr_levels=n_pyr_levels, max_steps=max_steps)
    r0 = orc.find_epipolar_match(cam, ref_pyr, cur_pyr, T_cur_ref, px, f, level, d_est, d_min, d_max, **kw)
    r, tr = orc.find_epipolar_match(cam, ref_pyr, cur_pyr, T_cur_ref, px, f, level, d_est, d_min, d_max, trace=True, **kw)
    assert (r.ok, r.path, r.search_level, r.n_zmssd, r.n_align_iters) == (r0.ok, r0.path, r0.search_level, r0.n_zmssd, r0.n_align_iters)
    np.testing.assert_array_equal(_bits(list(r.px_cur)), _bits(list(r0.px_cur)))
    np.testing.assert_array_equal(_bits([r.depth, r.epi_length]), _bits([r0.depth, r0.epi_length]))
    assert bytes(r.patch_with_border) == bytes(r0.patch_with_border)
    ev = ef.evaluated(tr)
    assert int(ev.sum()) == r.n_zmssd
    assert (tr["score"][~ev] == -1).all() and (ev == ((tr["dup"] == 0) & (tr["in_frame"] != 0))).all()
    if r.path != 1:
        assert len(tr) == 0
        return r, tr
    # the search hands the FIRST minimum below the threshold to align2D: run align2D from that candidate's pixel
    found, n_eval, win = ef.outcome(tr)
    assert n_eval == r.n_zmssd
    if not found:
        assert r.ok == 0 and r.n_align_iters == 0 and list(r.px_cur) == [0.0, 0.0]
        return r, tr
    assert win == int(np.nonzero(ev & (tr["score"] == tr["score"][ev].min()))[0][0])
    sc = float(1 << r.search_level)
    pwb = np.frombuffer(bytes(r.patch_with_border), dtype=np.uint8).reshape(10, 10)
    a_ok, p, it = orc.align2d(cur_pyr[r.search_level], pwb, pwb[1:9, 1:9], 10, tr["px"][win] / sc)
    want = p * sc if a_ok else tr["px"][win]
    np.testing.assert_array_equal(_bits(list(r.px_cur)), _bits(want))
    assert it == r.n_align_iters and (a_ok or not r.ok)
    return r, tr


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_trace_agrees_with_the_untraced_oracle(name):
    for case in ef.family(name):
        for i in range(case.n):
            _check_trace_against_untraced(case.cam, case.ref_pyr, case.cur_pyr, case.T_cur_ref, case.px[i], case.f[i], int(case.level[i]),
                                          case.d_est[i], case.d_min[i], case.d_max[i], max_steps=case.max_steps)


def _golden_epi_traces():
    from oracle import gen_golden
    sc, d_est, d_min, d_max = gen_golden.epi_case_inputs()
    T_cur_ref = synth.se3_mul(sc.T_cur_w, synth.se3_inv(sc.T_ref_w))
    return sc, [_check_trace_against_untraced(sc.cam, sc.ref_pyr, sc.cur_pyr, T_cur_ref, sc.px[i], sc.f[i], int(sc.level[i]), d_est[i],
                                              d_min[i], d_max[i]) for i in range(len(d_est))]


def test_trace_agrees_with_the_untraced_oracle_on_the_fixture_inputs():
    sc, res = _golden_epi_traces()
    assert sum(1 for r, tr in res if len(tr) > 16) > 100
    for r, tr in res:                                   # and the dead-fallback claim on rendered frames
        assert all(b is None or (b[0] <= 32 and b[1] <= 32) for b in ef.chunk_boxes(tr))


def _tagged(name, prefix):
    """[(case, i, result, trace)] of the seeds of a family whose tag starts with `prefix`"""
    out = []
    for case in ef.family(name):
        res = ef.oracle_results(case)
        out += [(case, i, res[i][0], res[i][1]) for i in range(case.n) if case.tags[i].startswith(prefix)]
    return out


def test_families_are_small():
    for name in FAMILY_NAMES:
        n = sum(c.n for c in ef.family(name))
        assert 16 <= n <= 64, (name, n)


def test_chunk_edges_reaches_its_paths():
    all_seeds = _tagged("chunk_edges", "")
    counts = {len(tr) for _, _, r, tr in all_seeds if r.path == 1}
    assert counts >= set(ef.CHUNK_COUNTS) | {41}
    for N in ef.CHUNK_COUNTS:
        for case, i, r, tr in _tagged("chunk_edges", "count:"):
            if case.tags[i].split(":")[1] != str(N):
                continue
            assert case.max_steps == 40 or (r.path == 1 and len(tr) == N and r.search_level == 0), (case.tags[i], len(tr))
    below = _tagged("chunk_edges", "below2")
    assert len(below) == 5 and all(r.path == 0 and r.epi_length < 2.0 for _, _, r, _ in below)
    # one whole wave (seeds 24..27) without a search, the waves before and after it with one
    paths = [r.path for r, _ in ef.oracle_results(ef.family("chunk_edges")[0])]
    assert all(p == 0 for p in paths[24:28]) and 1 in paths[20:24] and 1 in paths[28:32]
    just_above = [r for _, _, r, tr in all_seeds if 2.0 <= r.epi_length < 2.0 + 1e-6]
    assert len(just_above) == 1 and just_above[0].path == 1
    assert max(b.epi_length for _, _, b, _ in below) > 2.0 - 1e-6
    over = _tagged("chunk_edges", "path2")
    assert len(over) == 2 and all(r.path == 2 and r.ok == 0 and c.max_steps == 40 for c, _, r, _ in over)
    assert any(int(r.epi_length / 0.7) == 41 for _, _, r, _ in over)                   # one step above the limit ...
    assert any(c.max_steps == 40 and r.path == 1 and len(tr) == 41 for c, _, r, tr in all_seeds)   # ... and exactly at it
    for k in (16, 32):
        dup = [bool(tr["dup"][k]) for _, _, r, tr in all_seeds if len(tr) > k]
        assert sum(dup) >= 3 and len(dup) - sum(dup) >= 3, (k, dup)
        for want, label in ((True, "dup%d" % k), (False, "nodup%d" % k)):
            sel = [(c, i, r, tr) for c, i, r, tr in all_seeds if c.tags[i].endswith(":" + label)]
            assert len(sel) >= 3 and all(bool(tr["dup"][k]) == want and tr["in_frame"][k] for _, _, _, tr in sel)
    assert all(not any(ef.risky_chunks(tr, r.search_level)) for _, _, r, tr in all_seeds)


def test_ties_reaches_its_paths():
    per = _tagged("ties", "same") + _tagged("ties", "cross")
    assert {r.search_level for _, _, r, _ in per} == {0, 1}
    n_tied = {"same": 0, "cross": 0}
    for case, i, r, tr in per:
        assert r.path == 1 and r.epi_length >= 20.0
        t = ef.tie_indices(tr)
        assert len(t) >= 2 and tr["score"][t[0]] == 0
        kind = "same" if t[0] // 16 == t[1] // 16 else "cross"
        assert case.tags[i].startswith(kind)
        n_tied[kind] += 1
        assert ef.outcome(tr)[2] == t[0]
    assert n_tied["same"] >= 3 and n_tied["cross"] >= 3 and sum(n_tied.values()) >= 8
    const = _tagged("ties", "const:")
    assert len(const) >= 3
    for case, i, r, tr in const:                       # a constant image: every score 0, the first evaluated candidate wins, align2D fails
        ev = ef.evaluated(tr)
        assert (tr["score"][ev] == 0).all() and ev.sum() > 16 and r.ok == 0 and r.n_align_iters >= 1
        assert ef.outcome(tr)[2] == int(np.nonzero(ev)[0][0])
    for case, i, r, tr in _tagged("ties", "const_cur"):   # a constant current image under a textured patch: every score equal, none below the threshold
        ev = ef.evaluated(tr)
        assert len(set(tr["score"][ev])) == 1 and tr["score"][ev][0] >= ef.ZMSSD_THRESHOLD and r.ok == 0


def test_threshold_reaches_its_paths():
    for key in ef.THRESHOLD_PATTERNS:
        sel = _tagged("threshold", "score:%d" % key)
        assert len(sel) == 6
        for case, i, r, tr in sel:
            ev = ef.evaluated(tr)
            s = np.sort(tr["score"][ev])
            assert s[0] == key and s[1] >= ef.ZMSSD_THRESHOLD, (key, s[:3])
            assert ef.outcome(tr)[0] == (key < ef.ZMSSD_THRESHOLD) and (r.n_align_iters > 0) == (key < ef.ZMSSD_THRESHOLD)
            assert bytes(r.patch_with_border) == case.ref_pyr[0][int(case.px[i, 1]) - 5:int(case.px[i, 1]) + 5,
                                                                 int(case.px[i, 0]) - 5:int(case.px[i, 0]) + 5].tobytes()


def test_replay_reaches_its_paths():
    seen = set()
    for case in ef.family("replay"):
        for i, (r, tr) in enumerate(ef.oracle_results(case)):
            pattern, orient, lvl = case.tags[i].split(":")
            assert r.path == 1 and r.search_level == int(lvl[1]) and len(tr) > 32
            assert ef.risky_chunks(tr, r.search_level, margin=1e-9) == ef.REPLAY_PATTERNS[pattern], case.tags[i]
            along = 0 if orient == "h" else 1
            assert len(set(tr["pxi"][:, along])) > 20 and len(set(tr["pxi"][:, 1 - along])) <= 2
            assert ef.outcome(tr)[2] >= 16 and r.ok == 1            # the match lies in a chunk whose start depends on the hand-over
            seen.add((pattern, orient, r.search_level))
    assert seen == {(p, o, l) for p in ef.REPLAY_PATTERNS for o in "hv" for l in (0, 1)}


def test_warp_windows_reaches_its_paths():
    seeds = _tagged("warp_windows", "")
    fps = [ef.footprint(c, i, r.search_level) for c, i, r, _ in seeds]
    # both sides of the search-level thresholds, at every rotation
    for deg in ef.WARP_ANGLES:
        got = {}
        for (c, i, r, _), fp in zip(seeds, fps):
            if c.tags[i].startswith("sweep") and c.tags[i].endswith("rot%d" % deg):
                got[(int(c.level[i]), round(fp["D"], 1))] = r.search_level
        assert got == {(0, 0.6): 0, (1, 2.9): 0, (1, 3.1): 1, (2, 2.9): 0, (2, 3.1): 1, (2, 11.9): 1, (2, 12.1): 2}, got
    for (c, i, r, _), fp in zip(seeds, fps):
        if c.tags[i].startswith("sweep"):
            assert abs(fp["D"] - float(c.tags[i].split(":")[2][1:])) < 0.051 and fp["use_win"]
    # both sides of the window limit: a box of exactly 32 is copied, one of 33 is not
    far = [(c.tags[i], fp) for (c, i, _, _), fp in zip(seeds, fps) if c.tags[i].startswith("far")]
    sizes = {max(fp["ww"], fp["wh"]): fp["use_win"] for _, fp in far}
    assert sizes[32] is True and sizes[33] is False and sizes[31] is True
    assert sum(1 for _, fp in far if not fp["use_win"]) >= 4
    assert all(fp["use_win"] == (max(fp["ww"], fp["wh"]) <= 32) and fp["D"] < 0.1 for _, fp in far)
    # the degenerate warps: NaN (patch zeroed) and a depth estimate of 1e-12 (a finite warp far outside the image)
    nan = [(r, fp) for (c, i, r, _), fp in zip(seeds, fps) if c.tags[i] == "nan_warp"]
    assert len(nan) == 2 and all(fp["nan"] and not fp["use_win"] and bytes(r.patch_with_border) == bytes(100) for r, fp in nan)
    assert {r.path for r, _ in nan} == {0, 1}
    tiny = [(r, fp) for (c, i, r, _), fp in zip(seeds, fps) if c.tags[i] == "tiny_depth"]
    assert len(tiny) == 1 and not tiny[0][1]["nan"] and not tiny[0][1]["use_win"]
    pwb = np.frombuffer(bytes(tiny[0][0].patch_with_border), dtype=np.uint8)
    assert (pwb != 0).sum() == 1 and pwb[55] != 0                  # only the centre sample lands in the image
    assert {int(c.level[i]) for c, i, _, _ in seeds} == {0, 1, 2}


def test_borders_reaches_its_paths():
    seeds = _tagged("borders", "")
    for lvl in range(ef.N_LEVELS):
        cols, rows = ef.W >> lvl, ef.H >> lvl
        # (axis, pixel just outside the band, pixel just inside it) for the four sides
        for axis, out_px, in_px in ((0, 7, 8), (0, cols - 8, cols - 9), (1, 7, 8), (1, rows - 8, rows - 9)):
            hit = 0
            for c, i, r, tr in seeds:
                if r.search_level != lvl or r.path != 1:
                    continue
                a = tr["pxi"][:, axis]
                for k in range(len(tr) - 1):
                    pair = {(int(a[k]), bool(tr["in_frame"][k])), (int(a[k + 1]), bool(tr["in_frame"][k + 1]))}
                    if pair == {(out_px, False), (in_px, True)}:
                        hit += 1
            assert hit >= 1, (lvl, axis, out_px)
    # reference features 3 px from each side: zeroed samples, window corner clamped to 0 on the low sides
    clamp_x = clamp_y = zero_hi_x = zero_hi_y = 0
    for c, i, r, tr in seeds:
        fp = ef.footprint(c, i, r.search_level)
        assert fp["use_win"] and fp["overrun"] <= 30
        pwb = np.frombuffer(bytes(r.patch_with_border), dtype=np.uint8).reshape(10, 10)
        clamp_x += fp["wx0"] == 0 and (pwb[:, 0] == 0).all()
        clamp_y += fp["wy0"] == 0 and (pwb[0, :] == 0).all()
        zero_hi_x += (pwb[:, 9] == 0).all() and pwb[:, 5].any()
        zero_hi_y += (pwb[9, :] == 0).all() and pwb[5, :].any()
    assert min(clamp_x, clamp_y, zero_hi_x, zero_hi_y) >= 3
    # the last bytes of the reference allocation: the window fill of these seeds runs past the end of level 2 of the last slot,
    # by less than the 64 bytes of slack the pyramid allocation carries
    last = _tagged("borders", "last_slot_corner")
    assert len(last) == 2 and all(c.ref_slot == c.n_ref_slots - 1 == 1 and int(c.level[i]) == ef.N_LEVELS - 1 for c, i, _, _ in last)
    over = [ef.footprint(c, i, r.search_level)["overrun"] for c, i, r, _ in last]
    assert all(0 < o <= 30 for o in over), over
    assert all(r.n_zmssd > 0 for _, _, r, _ in last) and any(r.ok for _, _, r, _ in last)


@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_fillers_take_other_paths(name):
    """the seeds that the device test puts between a family's own: a short segment, a segment of three steps and a long one"""
    paths, counts = set(), set()
    for case in ef.family(name):
        mixed = ef.with_fillers(case)
        assert mixed.n == 2 * case.n and mixed.tags[0::2] == case.tags
        for (r, tr), tag in zip(ef.oracle_results(mixed), mixed.tags):
            if tag.startswith("filler"):
                paths.add(r.path)
                counts.add(len(tr))
                assert r.path == {"filler:short": 0, "filler:3step": 1}.get(tag, r.path), (case.name, tag, r.epi_length)
    assert {0, 1} <= paths and 3 in counts
    if name != "warp_windows":                 # (a camera that moves along z sees a bounded segment however close d_min is)
        assert 2 in paths


# ---- power: a wrong search rule changes what the device test compares ---------------------------------------------------
@pytest.mark.parametrize("name,variant", [("ties", "last_tie"), ("threshold", "le_threshold"), ("chunk_edges", "no_dedupe_at_chunk"),
                                          ("replay", "late_tail"), ("chunk_edges", "late_tail")])
def test_wrong_search_rules_change_the_outcome(name, variant):
    changed = 0
    for case, i, r, tr in _tagged(name, ""):
        if r.path != 1:
            continue
        right = ef.outcome(tr)
        assert right[1] == r.n_zmssd
        changed += ef.outcome(tr, variant) != right
    assert changed >= 3, changed


# ---- the direct-load fallback of phase B is dead ------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_every_chunk_of_candidates_fits_the_window(name):
    """Candidates are epi_length / n_steps apart with n_steps = floor(epi_length / 0.7) >= 2, i.e. 0.7 .. 1.05 level px: the
    16 candidates of a chunk span at most 15.75 px, their 8x8 patches at most 24 < 32.  Checked on every chunk here."""
    n_chunks = 0
    for case, i, r, tr in _tagged(name, ""):
        for b in ef.chunk_boxes(tr):
            if b is not None:
                n_chunks += 1
                assert b[0] <= 25 and b[1] <= 25, (case.tags[i], b)
    assert n_chunks >= 10


def test_every_chunk_fits_the_window_with_a_distorted_camera():
    """the same with the radtan camera of test_depth_filter_and_detector_with_a_distorted_camera: distortion bends the
    segment, the steps stay uniform on the unit plane -- the level-pixel spacing changes by the local magnification only"""
    sc = seedsynth.make_seed_case(n_seeds=400, seed=5)
    cam = copy.copy(sc.cam)
    cam.dist = (-0.12, 0.03, 2e-4, -1e-4, 0.0)
    c = orc.camera(cam)
    T_cur_ref = synth.se3_mul(sc.T_cur_w, synth.se3_inv(sc.T_ref_w))
    n_chunks, widest = 0, 0
    for i in range(len(sc.px)):
        f = np.zeros(3)
        orc.lib().svo_orc_cam2world(ctypes.byref(c), ctypes.c_double(sc.px[i, 0]), ctypes.c_double(sc.px[i, 1]), orc._p(f, ctypes.c_double))
        mu, s = np.float32(sc.mu[i]), np.sqrt(np.float32(sc.sigma2[i]))
        d_min, d_max = 1.0 / float(mu + s), 1.0 / float(max(mu - s, np.float32(0.00000001)))
        r, tr = orc.find_epipolar_match(cam, sc.ref_pyr, sc.cur_pyr, T_cur_ref, sc.px[i], f, int(sc.level[i]), 1.0 / float(mu), d_min, d_max,
                                        trace=True)
        for b in ef.chunk_boxes(tr):
            if b is not None:
                n_chunks += 1
                widest = max(widest, b[0], b[1])
    assert n_chunks > 200 and widest <= 32, (n_chunks, widest)
