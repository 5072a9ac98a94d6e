"""The model of tests/map_compaction_reference.py on its own (no device): what tests/test_gpu_map_compaction.py rests on.

On the maps of map_removal_scenario (small, wide, tie) and of map_growth_scenario (its base map with the candidates appended):
the identity without dead points, idempotence, the index checks svo_hip_tracker_set_map makes, and that compaction commutes -- up
to the relabelling by old_to_new -- with the three calls that change the map in place: append_candidates, promote,
remove_keyframe.  Every comparison is exact.

Each scenario has two states.  "tracked": tables as a tracked frame leaves them -- some points unlinked and TYPE_DELETED while
their observations, row entries, candidate entries and key-point entries are still in the tables, the re-selection owed.
"removed": a keyframe has left after that (map_removal_reference.remove_keyframe), the tables canonical."""
import numpy as np
import pytest

import map_compaction_reference as mc
import map_growth_reference as mg
import map_growth_scenario as sc
import map_removal_reference as mr
import map_removal_scenario as ms
from android_svo_amd import synth

FAMILIES = ("small", "wide", "tie", "growth")
REMOVED_KF = dict(small=3, wide=6, tie=1)


def _row(t, j):
    return t["kf_ftr_point"][t["kf_ftr_offset"][j]:t["kf_ftr_offset"][j + 1]]


def _scenario(fam):
    if fam == "growth":
        s = sc.make()
        cs = dict(mg.append_candidates(s["base_map"], **s["cand"])[0], cam=s["seq"]["cam"])
    else:
        cs = dict(small=ms.small_case, wide=ms.wide_case, tie=ms.tie_case)[fam]()
    t = dict(mg.normalised(cs), cam=cs["cam"])
    k = REMOVED_KF.get(fam)
    unl = np.zeros(t["n_points"], bool)
    if fam != "tie":
        j = 0 if k != 0 else 1
        cand = t["cand_point"]
        # deleted by tracking: a key point of a keyframe that stays, the second candidate of the list, two entries of a row
        unl[[t["kf_key_point"][j][0], cand[1], _row(t, j)[3], _row(t, j)[7]]] = True
        t["pt_type"] = np.where(unl, synth.TYPE_DELETED, t["pt_type"]).astype(np.int32)
    out = dict(fam=fam, k=k, tracked=t, unl=unl)
    if k is not None:
        out["removed"], out["info"] = mr.remove_keyframe(t, k, unlinked=unl)
        out["dead"] = unl.copy()
        out["dead"][out["info"]["deleted_points"] + out["info"]["deleted_candidates"]] = True
    else:                                                               # one keyframe: nothing to remove; the canonical state by compaction's own rule
        out["removed"], out["info"], out["dead"] = None, None, None
    return out


@pytest.fixture(scope="module")
def scen():
    return {fam: _scenario(fam) for fam in FAMILIES}


def _states(s):
    """(tables, dead) of a scenario: as tracked, and after the removal where there is one"""
    return [(s["tracked"], s["unl"])] + ([(dict(s["removed"], cam=s["tracked"]["cam"]), s["dead"])] if s["k"] is not None else [])


def test_the_scenarios_cover_the_ground(scen):
    for fam in ("small", "wide"):
        s = scen[fam]
        t, unl, info, dead = s["tracked"], s["unl"], s["info"], s["dead"]
        by_removal_pt, by_removal_cand = info["deleted_points"], info["deleted_candidates"]
        # dead points of all three origins, disjoint
        assert unl.sum() >= 3 and len(by_removal_pt) >= 20 and len(by_removal_cand) >= 5
        assert not unl[by_removal_pt + by_removal_cand].any() and not set(by_removal_pt) & set(by_removal_cand)
        assert dead.sum() == unl.sum() + len(by_removal_pt) + len(by_removal_cand)
        # a dead point that was a key point: one deleted by tracking, and one deleted by the removal in a keyframe that stays
        key = t["kf_key_point"]
        assert unl[key[key >= 0]].any()
        stay = np.delete(key, s["k"], axis=0)
        assert np.isin(stay[stay >= 0], by_removal_pt).any() and info["rekeys"]
        # a dead point between two living candidates
        cand = t["cand_point"]
        d = dead[cand]
        assert any(d[i] and not d[i - 1] and not d[i + 1] for i in range(1, len(cand) - 1))
        # the points deleted by tracking are still everywhere in the tables as the frame left them
        assert np.diff(t["pt_obs_offset"])[unl].all() and unl[t["kf_ftr_point"]].sum() >= 3 and unl[cand].sum() == 1
        # the first and the last point live or die in some scenario; both a dead and a living point follow a dead one
        assert (dead[:-1] & dead[1:]).any() and (dead[:-1] & ~dead[1:]).any()
    assert scen["tie"]["info"]["deleted_points"] == [3, 2] and scen["tie"]["dead"].tolist() == [False, False, True, True]   # the tail dies
    assert scen["growth"]["tracked"]["n_kf"] == 1 and scen["growth"]["unl"].sum() == 4


@pytest.mark.parametrize("fam", FAMILIES)
def test_identity_without_dead_points(scen, fam):
    for t, _ in _states(scen[fam]):
        out, info = mc.compact_points(t, np.zeros(t["n_points"], bool), last_point=np.array([3, -1, 0, t["n_points"] - 1]))
        mc.assert_tables_equal(out, t)
        assert info["old_to_new"].tolist() == list(range(t["n_points"])) and info["n_points"] == t["n_points"] and info["rekeyed"] == []
        assert info["last_point"].tolist() == [3, -1, 0, t["n_points"] - 1]
    empty = mg.normalised({k: np.zeros(0) for k in mg.TABLES})
    out, info = mc.compact_points(empty, np.zeros(0, bool))
    assert out["n_points"] == 0 and info["n_points"] == 0 and len(info["old_to_new"]) == 0


@pytest.mark.parametrize("fam", FAMILIES)
def test_output_is_canonical_and_idempotent(scen, fam):
    for t, dead in _states(scen[fam]):
        last = np.concatenate([[-1], np.arange(t["n_points"], dtype=np.int32)[::3]])
        out, info = mc.compact_points(t, dead, last_point=last)
        o2n = info["old_to_new"]
        alive = ~dead
        # ---- the numbering
        assert info["n_points"] == alive.sum() == out["n_points"]
        assert (o2n[dead] == -1).all() and o2n[alive].tolist() == list(range(alive.sum()))
        assert info["last_point"].tolist() == [-1] + o2n[last[1:]].tolist()
        # ---- what set_map would check, and the canonical form: no dead point is left to be in any list
        mc.check_set_map_indices(out, n_levels=5)
        mr.check_invariants(out, np.zeros(out["n_points"], bool))
        # ---- the rows of the living points, their observations in order, the lists in order
        for c in ("pt_pos", "pt_type", "pt_n_failed", "pt_n_succeeded"):
            assert out[c].tobytes() == t[c][alive].tobytes(), c
        keep = np.repeat(alive, np.diff(t["pt_obs_offset"]))
        for c in ("obs_kf", "obs_px", "obs_f", "obs_level", "obs_edgelet", "obs_grad"):
            assert out[c].tobytes() == t[c][keep].tobytes(), c
        assert np.array_equal(np.diff(out["pt_obs_offset"]), np.diff(t["pt_obs_offset"])[alive])
        for j in range(t["n_kf"]):
            old = _row(t, j)
            assert _row(out, j).tolist() == o2n[old[alive[old]]].tolist()
            incumbents = t["kf_key_point"][j]
            if j not in info["rekeyed"]:
                assert out["kf_key_point"][j].tolist() == [int(o2n[p]) if p >= 0 else -1 for p in incumbents]
            else:
                assert dead[incumbents[incumbents >= 0]].any()
                got = out["kf_key_point"][j]
                assert set(got[got >= 0].tolist()) <= set(_row(out, j).tolist())
        cand = t["cand_point"]
        assert out["cand_point"].tolist() == o2n[cand[alive[cand]]].tolist()
        # ---- once more: nothing is dead any more
        again, info2 = mc.compact_points(out, np.zeros(out["n_points"], bool))
        mc.assert_tables_equal(again, out)
        assert info2["old_to_new"].tolist() == list(range(out["n_points"]))
    s = scen[fam]
    if s["k"] is not None:                                              # the owed re-selection: the same whether the removal or the compaction pays it
        a = mc.compact_points(s["tracked"], s["unl"])[0]
        owed = [j for j in range(s["tracked"]["n_kf"]) if s["unl"][np.maximum(s["tracked"]["kf_key_point"][j], 0)][s["tracked"]["kf_key_point"][j] >= 0].any()]
        assert owed == mc.compact_points(s["tracked"], s["unl"])[1]["rekeyed"] and (fam == "tie" or owed)
        assert a["n_points"] == s["tracked"]["n_points"] - s["unl"].sum()


def _new_seeds(t, n=7):
    rng = np.random.default_rng(5)
    px = rng.uniform(10, 200, (n, 2))
    kf = (np.arange(n) % t["n_kf"]).astype(np.int32)
    kf[2] = -1                                                          # its keyframe has left
    return dict(pos=rng.uniform(-1, 1, (n, 3)), kf_index=kf, px=px, f=rng.uniform(-1, 1, (n, 3)), level=(np.arange(n) % 3).astype(np.int32),
                edgelet=(np.arange(n) % 2).astype(np.uint8), grad=rng.uniform(-1, 1, (n, 2)))


@pytest.mark.parametrize("fam", FAMILIES)
def test_commutes_with_append_candidates(scen, fam):
    for t, dead in _states(scen[fam]):
        seeds = _new_seeds(t)
        n = len(seeds["kf_index"])
        grown, first = mg.append_candidates(t, **seeds)
        a, ia = mc.compact_points(dict(grown, cam=t["cam"]), np.concatenate([dead, np.zeros(n, bool)]))
        small, ib = mc.compact_points(t, dead)
        b, first_b = mg.append_candidates(small, **seeds)
        mc.assert_tables_equal(a, b)
        assert ia["old_to_new"][first] == first_b == ib["n_points"]
        assert ia["old_to_new"][:first].tolist() == ib["old_to_new"].tolist()


def _frame(t, dead):
    """a tracked frame on tables t as hip.Tracker.track returns it: features on every fourth living point, the first living
    candidates among them, some features without a point; no feature on a dead point"""
    rng = np.random.default_rng(11)
    alive = np.where(~dead)[0]
    cand = [int(p) for p in t["cand_point"] if p >= 0 and not dead[p]][:4]
    pts = np.array(sorted(set(alive[::4].tolist()) | set(cand)), np.int32)
    rng.shuffle(pts)
    fp = np.concatenate([pts[:2], [-1], pts[2:], [-1]]).astype(np.int32)
    n = len(fp)
    cam = t["cam"]
    px = np.stack([rng.uniform(0, cam.width, n), rng.uniform(0, cam.height, n)], axis=1)
    return dict(feat_point=fp, feat_px=px, feat_f=rng.uniform(-1, 1, (n, 3)), feat_level=(np.arange(n) % 3).astype(np.int32),
                feat_type=(np.arange(n) % 5 == 0).astype(np.int32), feat_grad=rng.uniform(-1, 1, (n, 2)), T_f_w=np.array([.1, .2, .3, 0, 0, 0, 1.0]),
                type=t["pt_type"].copy(), n_failed=t["pt_n_failed"] + 1, n_succeeded=t["pt_n_succeeded"] + 2)


@pytest.mark.parametrize("fam", FAMILIES)
def test_commutes_with_promote(scen, fam):
    s = scen[fam]
    # the device pays the owed re-selection before it promotes: the state to promote from is one where none is owed
    t, dead = _states(s)[-1] if s["k"] is not None else (dict(s["tracked"], kf_key_point=np.where(s["unl"][np.maximum(s["tracked"]["kf_key_point"], 0)],
                                                                                                 -1, s["tracked"]["kf_key_point"])), s["unl"])
    cam, slot = t["cam"], int(t["kf_slot"].max()) + 1
    r = _frame(t, dead)
    grown, n_a = mg.promote(t, r, slot, cam)
    a, ia = mc.compact_points(dict(grown, cam=cam), dead)
    small, ib = mc.compact_points(t, dead, last_point=r["feat_point"])
    alive = ~dead
    r2 = dict(r, feat_point=ib["last_point"], type=r["type"][alive], n_failed=r["n_failed"][alive], n_succeeded=r["n_succeeded"][alive])
    b, n_b = mg.promote(small, r2, slot, cam)
    mc.assert_tables_equal(a, b)
    assert n_a == n_b and (fam == "tie" or n_a >= 1) and ia["old_to_new"].tolist() == ib["old_to_new"].tolist()
    assert ia["rekeyed"] == [] and ib["rekeyed"] == []


@pytest.mark.parametrize("fam", [f for f in FAMILIES if f in REMOVED_KF])
def test_commutes_with_remove_keyframe(scen, fam):
    s = scen[fam]
    t, unl, k = s["tracked"], s["unl"], s["k"]
    for rule in ("per_deletion", "once"):
        # remove, then compact
        A, info_a = mr.remove_keyframe(t, k, unlinked=unl, rekey=rule)
        dead_a = unl.copy()
        dead_a[info_a["deleted_points"] + info_a["deleted_candidates"]] = True
        a, ia = mc.compact_points(A, dead_a)
        # compact, then remove (nothing is unlinked any more), then compact what the removal deleted
        B, ib = mc.compact_points(t, unl)
        C, info_c = mr.remove_keyframe(dict(B, cam=t["cam"]), k, rekey=rule)
        o2n = ib["old_to_new"]
        assert o2n[info_a["deleted_points"]].tolist() == info_c["deleted_points"]
        assert o2n[info_a["deleted_candidates"]].tolist() == info_c["deleted_candidates"]
        assert info_a["slot"] == info_c["slot"]
        # the tables of both orders under one numbering: C still holds the rows of the points its removal deleted
        dead_c = np.zeros(C["n_points"], bool)
        dead_c[info_c["deleted_points"] + info_c["deleted_candidates"]] = True
        c, ic = mc.compact_points(C, dead_c)
        mc.assert_tables_equal(a, c)
        assert ia["old_to_new"].tolist() == [int(ic["old_to_new"][q]) if q >= 0 else -1 for q in o2n]
        # ... and before the last compaction, list by list
        Ar = mc.relabel(A, o2n)
        for name in ("kf_ftr_offset", "kf_ftr_point", "kf_key_point", "cand_point", "kf_slot", "T_kf_w"):
            assert Ar[name].tobytes() == C[name].tobytes(), name
        assert C["pt_type"].tolist() == A["pt_type"][~unl].tolist()
