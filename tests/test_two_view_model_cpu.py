"""tests/two_view_reference.py, the definition of the bootstrap's two-view stage, against GROUND TRUTH on the families of
tests/two_view_cases.py.  Discrete conditions only: every true inlier is in the inlier list, no constructed outlier is; the
chosen pose candidate is the one under which the ground-truth points lie in front of both cameras; the status is the one the
family is named for; map_tables keeps the index rules svo_hip_tracker_set_map documents.  Each case also proves that it
reaches what it is named for.  Pose errors are recorded in DESIGN.md section 7, not asserted: a wrong pose cannot pass the
inlier conditions at 2 px.  volume-8 / volume-9 run with min_inliers = n (the default 40 would name them FEW_INLIERS)."""
import numpy as np
import pytest

import two_view_cases as C
import two_view_reference as M


def front_counts(res, c):
    """for each of the four candidates of the winner: the number of TRUE correspondences in front of both cameras"""
    xy = M.normalised(c["f_ref"], c["f_cur"])
    F, _ = M.solve_hypotheses(xy, M.sample(c["params"]["seed"], res["hypothesis"] + 1, res["n_in"])[-1:])
    R1, R2, u3 = M.decompose(F[0])
    return M.cheirality_counts(R1, R2, u3, c["f_cur"], c["f_ref"], c["truth"])


@pytest.mark.parametrize("name", C.NAMES)
def test_family_against_ground_truth(name):
    c, r = C.case(name), C.model(name)
    n = len(c["f_ref"])
    assert r["n_in"] == n
    if c["expect"] is None:                                  # degenerate: a status and finite-or-NaN outputs, nothing raised
        assert r["status"] in range(5)
        assert r["T_cur_w"].shape == (7,) and r["point_pos"].shape == (r["n_points"], 3)
        return
    assert r["status"] == c["expect"], M.STATUS_NAMES[r["status"]]
    if r["status"] != M.OK:
        assert r["n_inliers"] == 0 and r["n_points"] == 0 and len(r["inliers"]) == 0 and len(r["point_index"]) == 0
        return
    inl = np.zeros(n, bool)
    inl[r["inliers"]] = True
    assert inl[c["truth"]].all(), "a true inlier is missing"
    rows = np.nonzero(~c["truth"])[0]
    extra = [i for i in rows if inl[i] and i != c.get("nan_row", -1)]
    assert not extra, "a constructed outlier is in the inlier list"
    assert (np.diff(r["inliers"]) > 0).all()
    fc = front_counts(r, c)
    assert fc[r["candidate"]] == int(c["truth"].sum()) and sorted(fc)[-2] < fc[r["candidate"]]
    assert r["scale"] == r["scale"] or "nan_row" in c


def test_cases_reach_what_they_are_named_for():
    r8 = C.model("volume-8")
    assert (M.sample(0, 1024, 8) == np.arange(8)).all() and r8["hypothesis"] == 0            # every sample the same: the tie rule
    assert (r8["counts"] == 8).all()
    assert C.model("gates-39")["hypothesis_count"] == 39 and C.model("gates-40")["n_inliers"] == 40
    assert (C.model("gates-identical")["counts"] == -1).all()
    ch = C.model("gates-cheirality")
    assert ch["candidate_count"] < 100 and ch["hypothesis"] >= 0
    b, cb = C.model("border"), C.case("border")
    pts = set(b["point_index"].tolist())
    assert [i in pts for i in cb["border_rows"]] == cb["border_in"] and b["n_inliers"] == 120
    assert C.model("median-even")["n_in"] % 2 == 0 and C.model("median-odd")["n_in"] % 2 == 1
    run = C.model("median-run")
    z = np.sort(run["xyz_in_cur"][:, 2])
    k = len(z) // 2
    assert z[k] == run["depth_median"] and z[k - 1] == z[k] == z[k + 1]                      # a run of equal depths across the rank
    neg = C.model("median-negative")
    assert (neg["xyz_in_cur"][:, 2] < 0).any() and neg["depth_median"] == np.sort(neg["xyz_in_cur"][:, 2])[len(neg["xyz_in_cur"]) // 2]
    nan, cn = C.model("median-nan"), C.case("median-nan")
    assert np.isnan(nan["xyz_in_cur"][cn["nan_row"]]).all() and np.isnan(nan["depth_median"])
    assert cn["nan_row"] in nan["inliers"] and cn["nan_row"] not in nan["point_index"]        # an inlier that yields no point
    sg, cs = C.model("border-singular"), C.case("border-singular")
    f1, f2 = cs["f_cur"][16], np.array(M._matvec(list(sg["R"]), list(cs["f_ref"][16])))
    assert f1 @ f1 * -(f2 @ f2) - (f1 @ f2) * -(f1 @ f2) == 0.0                                # det = 0: invdet = inf, the singular route
    assert np.isnan(sg["xyz_in_cur"][16]).all() and 16 in sg["inliers"] and 16 not in sg["point_index"] and sg["mask"][16] == 0
    p1, p5 = C.model("pose-1.0"), C.model("pose-0.5")
    assert p5["scale"] == 0.5 * p1["scale"] and not np.array_equal(p1["T_cur_w"][:3], p5["T_cur_w"][:3])
    # the scene's depth median is the map scale
    z = np.array([M.se3_act(list(p5["T_cur_w"]), list(p))[2] for p in p5["point_pos"]])
    assert abs(np.sort(z)[len(z) // 2] - 0.5) < 0.05


def test_sampling_is_a_function_of_seed_h_draw_and_n():
    for n in (8, 9, 65, 1000):
        s = M.sample(3, 300, n)
        assert (np.diff(s, axis=1) > 0).all() and s.min() >= 0 and s.max() < n               # 8 distinct indices
        assert (M.sample(3, 100, n) == s[:100]).all()
    assert not (M.sample(3, 64, 65) == M.sample(4, 64, 65)).all()
    assert len({tuple(r) for r in M.sample(0, 4096, 400)}) > 4000


@pytest.mark.parametrize("name", ["volume-65", "border", "pose-0.5", "median-nan"])
def test_map_tables_keep_the_index_rules(name):
    r = C.model(name)
    mp = M.map_tables(r)
    m = r["n_points"]
    assert len(mp["kf_slot"]) == 2 and mp["T_kf_w"].shape == (2, 7) and mp["kf_key_point"].shape == (2, 5)
    assert mp["kf_ftr_offset"].tolist() == [0, m, 2 * m] and (mp["kf_ftr_point"] == np.tile(np.arange(m), 2)).all()
    assert (mp["pt_type"] == 2).all() and mp["pt_obs_offset"].tolist() == list(range(0, 2 * m + 1, 2))
    assert (mp["obs_kf"].reshape(m, 2) == [0, 1]).all() and (mp["obs_level"] == 0).all() and not mp["obs_edgelet"].any()
    assert len(mp["cand_point"]) == 0 and mp["pt_pos"].shape == (m, 3)
    np.testing.assert_array_equal(mp["obs_f"][0::2], r["f_ref"][r["point_index"]])
    np.testing.assert_array_equal(mp["obs_px"][1::2], r["px_cur"][r["point_index"]].astype(np.float64))
