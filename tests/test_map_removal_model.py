"""The model of tests/map_removal_reference.py on its own (no device): what tests/test_gpu_map_removal.py rests on.

    * the tables it writes are canonical and consistent after every removal;
    * the removals the GPU test uses cover what a removal can meet: points with one, two and more observations in the keyframe
      that leaves, candidates seeded there, the first and the last keyframe, a removal that costs no keyframe a key feature, one
      that costs three keyframes one each, one that makes a single keyframe choose again three times or more;
    * on all of them the reference's rule (Frame::setKeyPoints at every Frame::removeKeyPoint hit) and the device's (once per
      keyframe, afterwards) give the same key points -- random double pixels do not tie -- which is the condition under which the
      GPU test may hold the device to the reference's own rule;
    * one constructed case with integer pixels, as promoted seed features have them, where the two rules differ in exactly one
      slot: the deviation DESIGN.md section 7 documents ("once per keyframe instead of once per deletion")."""
import numpy as np
import pytest

import map_removal_reference as mr
from map_removal_scenario import REMOVALS, small_case, tie_case, wide_case
from android_svo_amd import synth


@pytest.fixture(scope="module")
def cases():
    return dict(small=small_case(), wide=wide_case())


@pytest.fixture(scope="module")
def removed(cases):
    """every removal of REMOVALS under both rules, once: {(family, k): (tables, info, tables_once, info_once)}"""
    return {(fam, k): mr.remove_keyframe(cases[fam], k) + mr.remove_keyframe(cases[fam], k, rekey="once") for fam, k in REMOVALS}


def _row(cs, k):
    return cs["kf_ftr_point"][cs["kf_ftr_offset"][k]:cs["kf_ftr_offset"][k + 1]]


@pytest.mark.parametrize("fam,k", REMOVALS, ids=["%s-%d" % r for r in REMOVALS])
def test_tables_are_canonical(cases, removed, fam, k):
    cs = mr.normalised(cases[fam])
    out, info = removed[fam, k][:2]
    gone = np.zeros(cs["n_points"], bool)
    gone[info["deleted_points"] + info["deleted_candidates"]] = True
    mr.check_invariants(out, gone)
    assert np.array_equal(mr.unlinked_of(out) & ~mr.unlinked_of(cs), gone)
    assert out["n_kf"] == cs["n_kf"] - 1 and out["n_points"] == cs["n_points"]
    assert info["slot"] == cs["kf_slot"][k] and info["slot"] not in out["kf_slot"]
    # ---- what the removal is, spelled out on the input tables
    row = _row(cs, k)
    n_obs = np.diff(cs["pt_obs_offset"])
    assert sorted(info["deleted_points"]) == sorted(row[n_obs[row] <= 2].tolist())
    seed_kf = cs["obs_kf"][cs["pt_obs_offset"][cs["cand_point"] + 1] - 1]
    assert info["deleted_candidates"] == cs["cand_point"][seed_kf == k].tolist()                 # list order
    assert out["cand_point"].tolist() == cs["cand_point"][seed_kf != k].tolist()
    assert (out["pt_type"][gone] == synth.TYPE_DELETED).all() and np.array_equal(out["pt_type"][~gone], cs["pt_type"][~gone])
    for name in ("pt_pos", "pt_n_failed", "pt_n_succeeded"):
        assert out[name].tobytes() == cs[name].tobytes()
    # every surviving point keeps its observations outside keyframe k, in order, renumbered
    keep = ~gone[np.repeat(np.arange(cs["n_points"]), n_obs)] & (cs["obs_kf"] != k)
    assert out["obs_px"].tobytes() == cs["obs_px"][keep].tobytes()
    assert np.array_equal(out["obs_kf"], cs["obs_kf"][keep] - (cs["obs_kf"][keep] > k))
    others = [j for j in range(cs["n_kf"]) if j != k]
    for j_new, j in enumerate(others):
        old = _row(cs, j)
        assert _row(out, j_new).tolist() == old[~gone[old]].tolist()
        assert out["T_kf_w"][j_new].tobytes() == cs["T_kf_w"][j].tobytes()
        if j not in info["rekeys"]:
            assert np.array_equal(out["kf_key_point"][j_new], cs["kf_key_point"][j])           # incumbents stay
        else:
            assert gone[cs["kf_key_point"][j][cs["kf_key_point"][j] >= 0]].any()


def test_the_removals_cover_the_ground(cases, removed):
    stats = {}
    for (fam, k), (out, info, _, _) in removed.items():
        cs = cases[fam]
        n = np.diff(cs["pt_obs_offset"])[_row(cs, k)]
        stats[fam, k] = dict(row=len(n), one=int((n == 1).sum()), two=int((n == 2).sum()), more=int((n >= 3).sum()),
                             cands=len(info["deleted_candidates"]), rekeys=info["rekeys"])
        print(fam, k, stats[fam, k])
    # The exact figures of the model, so that a change of the model shows.  They differ a little from the count the issue quotes
    # (small: 32-44 / 79-104 points with 2 / >= 3 observations, wide k=6: keyframe 8 three times): that count left out the points
    # the fixtures mark TYPE_DELETED while features still refer to them (2 % of synth.make_map_case's points).  Such a point is not
    # unlinked: its features have a point, as in the reference (ftr->point != NULL), so the removal walks it like any other.
    want = {("small", 0): (135, 12, 38, 85, 6, {2: 1}), ("small", 1): (156, 9, 41, 106, 10, {}), ("small", 2): (149, 7, 36, 106, 6, {3: 1}),
            ("small", 3): (165, 16, 46, 103, 12, {1: 1, 2: 1, 4: 1}), ("small", 4): (133, 15, 35, 83, 6, {}),
            ("wide", 1): (220, 24, 89, 107, 6, {0: 4}), ("wide", 6): (238, 23, 77, 138, 10, {7: 1, 8: 5})}
    got = {r: (s["row"], s["one"], s["two"], s["more"], s["cands"], s["rekeys"]) for r, s in stats.items()}
    assert got == want
    # ... and what they are there for
    assert ("small", 0) in stats and ("small", cases["small"]["n_kf"] - 1) in stats           # the first and the last keyframe
    assert any(s["rekeys"] == {} for s in stats.values())                                     # no keyframe loses a key feature: incumbents stay
    assert any(sorted(s["rekeys"].values()) == [1, 1, 1] for s in stats.values())              # three keyframes, one each
    # a single keyframe chooses again three times or more: a feature that wins a slot is itself deleted later
    assert stats["wide", 1]["rekeys"] == {0: 4} and stats["wide", 6]["rekeys"][8] == 5
    small = [stats["small", k] for k in range(5)]
    for name, lo, hi in (("row", 133, 165), ("one", 7, 16), ("two", 35, 46), ("more", 83, 106), ("cands", 6, 12)):
        assert (min(s[name] for s in small), max(s[name] for s in small)) == (lo, hi), name


def test_both_rules_agree_on_every_removal(removed):
    """the condition under which the device (once per keyframe) can be held to the reference's rule (once per deletion)"""
    assert len(removed) == 7
    for (fam, k), (a, ia, b, ib) in removed.items():
        mr.assert_tables_equal(a, b)
        assert ia["deleted_points"] == ib["deleted_points"] and ia["deleted_candidates"] == ib["deleted_candidates"]
        assert set(ia["rekeys"]) == set(ib["rekeys"]) and set(ib["rekeys"].values()) <= {1}


def test_owed_reselection_comes_first(cases):
    """points an earlier frame unlinked: their features have no point, they are in no table afterwards, and the keyframes that had
    one of them as a key feature choose again on the rows as they were"""
    cs = mr.normalised(cases["wide"])
    k = 6
    key = cs["kf_key_point"]
    unl = np.zeros(cs["n_points"], bool)
    unl[[key[0][0], key[8][1], cs["cand_point"][0], _row(cs, k)[0]]] = True
    out, info = mr.remove_keyframe(cases["wide"], k, unlinked=unl)
    gone = unl.copy()
    gone[info["deleted_points"] + info["deleted_candidates"]] = True
    mr.check_invariants(out, gone)
    assert not unl[info["deleted_points"] + info["deleted_candidates"]].any()                   # (they were gone already)
    assert key[0][0] not in out["kf_key_point"][0] and key[8][1] not in out["kf_key_point"][7]
    assert np.array_equal(out["pt_type"][unl], cs["pt_type"][unl])                               # (their types were the frame's to set)


def test_last_frame_features_lose_deleted_points(cases):
    cs = cases["small"]
    _, info = mr.remove_keyframe(cs, 3)
    gone = info["deleted_points"][:3] + info["deleted_candidates"][:1]
    last = np.array([5, gone[0], -1, gone[3], 7, gone[1]], np.int32)
    assert mr.remove_keyframe(cs, 3, last_point=last)[1]["last_lost"] == [1, 3, 5]


def test_constructed_tie_shows_the_inherited_deviation():
    """integer pixels: a feature that takes a slot from a living incumbent and is itself deleted later leaves the slot to the first
    of two tied features under the reference's rule, to the incumbent under the device's"""
    cs = tie_case()
    a, ia = mr.remove_keyframe(cs, 1)
    b, ib = mr.remove_keyframe(cs, 1, rekey="once")
    assert ia["deleted_points"] == ib["deleted_points"] == [3, 2] and ia["rekeys"] == {0: 2} and ib["rekeys"] == {0: 1}
    differ = a["kf_key_point"] != b["kf_key_point"]
    assert differ.sum() == 1 and differ[0, 1]
    assert a["kf_key_point"][0].tolist() == [1, 0, -1, -1, -1] and b["kf_key_point"][0].tolist() == [1, 1, -1, -1, -1]
    for name in mr.TABLES:
        if name != "kf_key_point":
            assert a[name].tobytes() == b[name].tobytes(), name
