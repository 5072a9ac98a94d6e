"""The numpy models of tests/relocalise_reference.py on their own, on the CPU: Map::getClosestKeyframe and "the last frame becomes
a keyframe" on the index tables.  The map cases are those of the removal tests (small: five keyframes, wide: nine) and the same
cases after the removal and compaction models have run -- tables with dropped rows and renumbered points.  What is established
here is what tests/test_gpu_relocalise.py rests on: the probes tell keyframes apart, some keyframes are not close, the exclusion
matters, a probe sees nothing, an exact tie goes to the lower index, and the feature list is the host flatten's."""
import numpy as np
import pytest

import map_compaction_reference as mc
import map_removal_reference as mr
import map_removal_scenario as ms
import relocalise_reference as rl
from android_svo_amd import synth


def derived_cases():
    """{name: (tables, unlinked or None)}: the two cases, each after a removal (dead points still numbered, nothing refers to them)
    and after the compaction that follows (renumbered)."""
    out = {}
    for name, cs, k in (("small", ms.small_case(), 2), ("wide", ms.wide_case(), 6)):
        out[name] = (cs, None)
        removed, info = mr.remove_keyframe(cs, k)
        dead = np.zeros(cs["n_points"], bool)
        dead[info["deleted_points"] + info["deleted_candidates"]] = True
        out[name + "-removed"] = (dict(removed, cam=cs["cam"]), dead)
        compacted, _ = mc.compact_points(removed, dead, cam=cs["cam"])
        out[name + "-compacted"] = (dict(compacted, cam=cs["cam"]), None)
    return out


@pytest.fixture(scope="module")
def cases():
    return derived_cases()


def test_probes_tell_the_keyframes_apart(cases):
    for name, (cs, _) in cases.items():
        K = cs["n_kf"]
        ans = [rl.closest_keyframe(cs, T) for T in rl.probes(cs)]
        chosen = {a["kf_index"] for a in ans}
        assert len(chosen - {-1}) >= 3, (name, chosen)                              # the chosen keyframe is not constant
        assert any(0 < a["n_close"] < K for a in ans), name                         # some keyframes are not close
        assert any(a["kf_index"] == -1 and a["n_close"] == 0 for a in ans), name    # a probe has no close keyframe
        for a in ans:
            if a["kf_index"] >= 0:
                d = dict(a["close"])
                assert a["distance"] == min(d.values()) and a["kf_index"] == min(k for k in d if d[k] == a["distance"])


def test_a_keyframe_pose_finds_itself_and_the_exclusion_moves_on(cases):
    for name, (cs, _) in cases.items():
        changed = 0
        for k in range(cs["n_kf"]):
            T = np.asarray(cs["T_kf_w"], np.float64).reshape(-1, 7)[k]
            a = rl.closest_keyframe(cs, T)
            if a["kf_index"] != k:
                continue                                                              # (its own key points may lie outside its image border)
            assert a["distance"] == 0.0
            b = rl.closest_keyframe(cs, T, exclude=k)
            assert b["n_close"] == a["n_close"] and b["kf_index"] != k
            assert b["kf_index"] == -1 or b["distance"] > 0.0
            changed += b["kf_index"] != a["kf_index"]
        assert changed >= 2, name                                                   # the exclusion changes the answer


def test_an_exact_tie_goes_to_the_lower_index():
    tm, T = rl.tie_map()
    a = rl.closest_keyframe(tm, T)
    d = dict(a["close"])
    assert sorted(d) == [0, 1] and d[0] == d[1] and a["n_close"] == 2                # keyframe 2 is nearer, but not close
    assert rl.distance(T, tm["T_kf_w"][2]) < d[0]
    assert a["kf_index"] == 0
    assert rl.closest_keyframe(tm, T, exclude=0)["kf_index"] == 1
    swapped = dict(tm, T_kf_w=tm["T_kf_w"][[1, 0, 2]], kf_key_point=tm["kf_key_point"][[1, 0, 2]])
    assert rl.closest_keyframe(swapped, T)["kf_index"] == 0                         # the index decides, not the keyframe
    assert rl.closest_keyframe(tm, T, exclude=0)["n_close"] == 2
    only = rl.closest_keyframe(dict(tm, kf_key_point=np.full((3, 5), -1, np.int32)), T)
    assert only["kf_index"] == -1 and only["n_close"] == 0                           # no key point, no close keyframe


def test_the_first_visible_key_point_decides():
    tm, T = rl.tie_map()
    key = tm["kf_key_point"].copy()
    key[0] = [2, -1, 0, -1, -1]                                                      # an invisible one first, a -1, then the visible one
    assert rl.closest_keyframe(dict(tm, kf_key_point=key), T)["close"][0][0] == 0
    key[0] = [2, -1, -1, -1, -1]
    assert [k for k, _ in rl.closest_keyframe(dict(tm, kf_key_point=key), T)["close"]] == [1]


def test_the_feature_list_is_the_host_flatten(cases):
    seen_dropped = 0
    for name, (cs, dead) in cases.items():
        t = mr.normalised(cs)
        for k in range(t["n_kf"]):
            a, b = rl.last_frame_from_keyframe(cs, k, dead), rl.flatten_keyframe(cs, k, dead)
            assert a["point"].tolist() == b["point"].tolist(), (name, k)
            for c in ("T_f_w", "px", "f"):
                assert a[c].tobytes() == b[c].tobytes(), (name, k, c)
            row = t["kf_ftr_point"][t["kf_ftr_offset"][k]:t["kf_ftr_offset"][k + 1]]
            assert len(a["point"]) == len(row) and a["T_f_w"].tobytes() == t["T_kf_w"][k].tobytes()      # canonical tables: nothing to drop
            assert len(a["point"]) >= 20, (name, k)
    # tables that still hold the entries of unlinked points (a tracked frame deleted them): they are dropped, not kept as -1
    cs = ms.small_case()
    t = mr.normalised(cs)
    dead = np.zeros(t["n_points"], bool)
    dead[t["kf_ftr_point"][::3]] = True
    for k in range(t["n_kf"]):
        a, b = rl.last_frame_from_keyframe(cs, k, dead), rl.flatten_keyframe(cs, k, dead)
        row = t["kf_ftr_point"][t["kf_ftr_offset"][k]:t["kf_ftr_offset"][k + 1]]
        assert a["point"].tolist() == b["point"].tolist() == [int(p) for p in row if not dead[p]]
        assert a["px"].tobytes() == b["px"].tobytes() and (a["point"] >= 0).all()
        seen_dropped += len(row) - len(a["point"])
    assert seen_dropped >= 50
    # a point uploaded as TYPE_DELETED but never unlinked is a living row
    typed = dict(cs, pt_type=np.where(dead, synth.TYPE_DELETED, t["pt_type"]).astype(np.int32))
    assert len(rl.last_frame_from_keyframe(typed, 0)["point"]) == t["kf_ftr_offset"][1] - t["kf_ftr_offset"][0]


def test_a_point_seen_twice_by_a_keyframe_takes_its_first_observation():
    tm, _ = rl.tie_map()
    t = mr.normalised(tm)
    # point 0 gains a second observation in keyframe 0, behind the first
    twice = dict(tm, pt_obs_offset=np.array([0, 2, 3, 4], np.int32), obs_kf=np.array([0, 0, 1, 2], np.int32),
                 obs_px=np.concatenate([t["obs_px"][:1], [[10.0, 20.0]], t["obs_px"][1:]]),
                 obs_f=np.concatenate([t["obs_f"][:1], [[0.0, 0.0, 1.0]], t["obs_f"][1:]]), obs_level=np.zeros(4, np.int32),
                 obs_edgelet=np.zeros(4, np.uint8), obs_grad=np.tile([1.0, 0.0], (4, 1)))
    a = rl.last_frame_from_keyframe(twice, 0)
    assert a["point"].tolist() == [0] and a["px"].tolist() == [[159.5, 119.5]]
    assert rl.flatten_keyframe(twice, 0)["px"].tolist() == a["px"].tolist()
