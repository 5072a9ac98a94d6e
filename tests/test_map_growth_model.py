"""The numpy model of map growth (tests/map_growth_reference.py) on the CPU: against the existing helper that grows
tracking_chain's map by one keyframe, its own invariants, and -- through the oracle's tracking chain -- the coverage the device
tests rely on: at the promoted frame some candidates are matched and some are not."""
import numpy as np
import pytest

import map_growth_reference as mg
import map_growth_scenario as sc
import tracking_chain as tc
from android_svo_amd import synth
from oracle import orc


def _oracle_frames(mp, state, seq, last, frames):
    out = []
    for k in frames:
        r = tc.oracle_track_frame(orc, mp, state, last, seq["pyrs"][k - 1], seq["pyrs"][k], 2)
        out.append(sc.snapshot(r))
        last = sc.as_last(r)
    return out, last


def _state(mp):
    return {"pt_type": mp["pt_type"].copy(), "pt_n_failed": mp["pt_n_failed"].copy(), "pt_n_succeeded": mp["pt_n_succeeded"].copy(),
            "unlinked": np.zeros(mp["n_points"], np.uint8)}


@pytest.fixture(scope="module")
def chain():
    """the scenario through the oracle: frames 1-2 on the base map, the candidates appended, frames 3-5"""
    s = sc.make()
    seq, mp = s["seq"], s["base_map"]
    state = _state(mp)
    rs, last = _oracle_frames(mp, state, seq, sc.first_last(s["base"]), range(1, sc.APPEND_AFTER + 1))
    mp2, first = mg.append_candidates(mp, **s["cand"])
    n_new = len(s["cand"]["kf_index"])
    state2 = {"pt_type": mp2["pt_type"].copy(), "pt_n_failed": mp2["pt_n_failed"].copy(), "pt_n_succeeded": mp2["pt_n_succeeded"].copy(),
              "unlinked": np.concatenate([state["unlinked"], np.zeros(n_new, np.uint8)])}
    for k, name in (("pt_type", "type"), ("pt_n_failed", "n_failed"), ("pt_n_succeeded", "n_succeeded")):
        state2[k][:first] = rs[-1][name]
    rs2, _ = _oracle_frames(mp2, state2, seq, last, range(sc.APPEND_AFTER + 1, sc.PROMOTE_AT + 1))
    return dict(s, mp=mp, mp2=mp2, first=first, n_new=n_new, r_promote=rs2[-1])


def test_promote_equals_the_existing_keyframe_helper():
    """a map without candidates: promote == tracking_chain.map_with_tracked_frame_as_keyframe, array for array"""
    seq = tc.make_sequence(n_frames=sc.N_FRAMES)
    mp = tc.sequence_map(seq)
    rs, _ = _oracle_frames(mp, _state(mp), seq, sc.first_last(seq), range(1, sc.PROMOTE_AT + 1))
    r = rs[-1]
    assert (r["feat_point"] >= 0).sum() >= 20
    got, n_promoted = mg.promote(mp, r, 1, seq["cam"])
    assert n_promoted == 0
    mg.assert_tables_equal(got, tc.map_with_tracked_frame_as_keyframe(seq, mp, r))


def _check_csr(t):
    for off, n in ((t["kf_ftr_offset"], len(t["kf_ftr_point"])), (t["pt_obs_offset"], len(t["obs_kf"]))):
        assert off[0] == 0 and off[-1] == n and (np.diff(off) >= 0).all()
    assert len(t["kf_ftr_offset"]) == t["n_kf"] + 1 and len(t["pt_obs_offset"]) == t["n_points"] + 1


def _obs_of(t, p):
    o0, o1 = t["pt_obs_offset"][p], t["pt_obs_offset"][p + 1]
    return [(int(t["obs_kf"][o]), t["obs_px"][o].tobytes(), t["obs_f"][o].tobytes(), int(t["obs_level"][o]), int(t["obs_edgelet"][o]),
             t["obs_grad"][o].tobytes()) for o in range(o0, o1)]


def test_model_invariants(chain):
    mp, mp2, first, n_new, r = (chain[k] for k in ("mp", "mp2", "first", "n_new", "r_promote"))
    base = mg.normalised(mp)
    # ---- append: nothing that existed moved, the new entries sit at the tails
    _check_csr(mp2)
    assert first == base["n_points"] and mp2["n_points"] == first + n_new
    for k in mg.TABLES:
        n = len(base[k])
        assert mp2[k][:n].tobytes() == base[k].tobytes(), k
    np.testing.assert_array_equal(mp2["cand_point"], np.arange(first, first + n_new))
    assert (mp2["pt_type"][first:] == synth.TYPE_CANDIDATE).all() and not mp2["pt_n_failed"][first:].any() and not mp2["pt_n_succeeded"][first:].any()
    np.testing.assert_array_equal(np.diff(mp2["pt_obs_offset"])[first:], 1)
    # a seed whose keyframe has left the map brings no observation
    kfi = chain["cand"]["kf_index"].copy()
    kfi[1::3] = -1
    mp3, _ = mg.append_candidates(mp, **dict(chain["cand"], kf_index=kfi))
    _check_csr(mp3)
    np.testing.assert_array_equal(np.diff(mp3["pt_obs_offset"])[first:], (kfi >= 0).astype(int))
    # ---- promote with candidates
    for before in (mp2, mp3):
        after, n_promoted = mg.promote(before, r, 1, chain["seq"]["cam"])
        _check_csr(after)
        k = before["n_kf"]
        assert after["n_kf"] == k + 1 and after["n_points"] == before["n_points"]
        seen = set(int(p) for p in r["feat_point"] if p >= 0)
        for p in range(before["n_points"]):
            old, new = _obs_of(before, p), _obs_of(after, p)
            if p in seen:
                assert new[1:] == old and new[0][0] == k               # every old observation kept in order behind the new one
            else:
                assert new == old
        matched = [int(p) for p in before["cand_point"] if int(p) in seen]
        unmatched = [int(p) for p in before["cand_point"] if int(p) not in seen]
        assert n_promoted == len(matched) >= 5 and len(unmatched) >= 5
        np.testing.assert_array_equal(after["cand_point"], unmatched)             # they leave the list, the others keep their order
        assert (after["pt_type"][matched] == synth.TYPE_UNKNOWN).all() and not after["pt_n_failed"][matched].any()
        for name, key in (("pt_type", "type"), ("pt_n_failed", "n_failed"), ("pt_n_succeeded", "n_succeeded")):
            np.testing.assert_array_equal(after[name][unmatched], r[key][unmatched])     # unmatched candidates: as the frame left them
        # each matched candidate with a seed observation: exactly one more entry, at the end of its seed keyframe's row
        with_seed = [p for p in matched if before["pt_obs_offset"][p + 1] > before["pt_obs_offset"][p]]
        assert len(with_seed) >= 1 and (before is mp2 or len(with_seed) < len(matched))
        for j in range(k):
            old_row = before["kf_ftr_point"][before["kf_ftr_offset"][j]:before["kf_ftr_offset"][j + 1]]
            new_row = after["kf_ftr_point"][after["kf_ftr_offset"][j]:after["kf_ftr_offset"][j + 1]]
            mine = [p for p in with_seed if before["obs_kf"][before["pt_obs_offset"][p + 1] - 1] == j]
            np.testing.assert_array_equal(new_row, np.concatenate([old_row, np.array(mine, np.int32)]))
        np.testing.assert_array_equal(after["kf_ftr_point"][after["kf_ftr_offset"][k]:], r["feat_point"][r["feat_point"] >= 0])


def test_the_promoted_frame_matches_some_candidates_and_misses_others(chain):
    """coverage of the device tests: the oracle's reprojector, fed the candidate tables, matches at least 5 of the held-back
    points in the frame that will be promoted and leaves at least 5 unmatched"""
    r, first, n_new = chain["r_promote"], chain["first"], chain["n_new"]
    fp = r["feat_point"]
    matched = np.unique(fp[fp >= first])
    assert len(matched) >= 5 and n_new - len(matched) >= 5, (len(matched), n_new)
    assert int(r["n_matches"]) >= 50
