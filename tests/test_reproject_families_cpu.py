"""The constructed map families of tests/reproject_families.py, without a GPU:

  * every family reaches what it is named for -- asserted on the oracle's outputs (orc.reproject_map) with the numpy predicates:
    the class of n_cells and n_kept, the winner of every distance tie, the side of every boundary each tagged point fell on;
  * the oracle is pinned to the reference's own compiled Reprojector::reprojectMap on every one of them
    (tests/golden/reproject_paths_ref.npz, made by oracle/gen_golden.py --map-only: results only, the inputs are regenerated
    here and guarded by CRCs) -- no family is left out of the comparison;
  * the comparison has teeth: check_map_result accepts the numpy restatement of the cell loop (rf.replay) and rejects three
    wrong variants of it -- tied keyframes swapped, a crowded cell tried in point-index order, the cut applied at >= max_fts.

tests/test_gpu_reproject_paths.py runs the same cases through the planning and replay kernels."""
import os

import numpy as np
import pytest

import reproject_families as rf
from test_oracle_reproject_map import check_map_result
from android_svo_amd.synth import TYPE_CANDIDATE, TYPE_DELETED, TYPE_GOOD, TYPE_UNKNOWN
from oracle import orc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reproject_paths_ref.npz")
NAMES = [cs["name"] for cs in rf.all_cases()]
ORACLE_ONLY = ()          # cases the reference harness cannot hold: none


def as_fixture(name, res):
    """a result in the layout check_map_result compares against"""
    g = {name + "_n": np.array([int(res["n_matches"]), int(res["n_trials"])], dtype=np.int64)}
    for k in rf.RESULT_KEYS:
        g[name + "_" + k] = np.asarray(res[k])
    return g


def changed(cs, res, p):
    """did the frame touch point p's counters (a point that was kept and tried, or a candidate out of the frame)"""
    return bool(res["n_failed"][p] != cs["pt_n_failed"][p] or res["n_succeeded"][p] != cs["pt_n_succeeded"][p])


def cell_of_point(cs, p):
    return rf.cell_of(cs, rf.project_cur(cs, p)[1])


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_no_family_is_left_out_of_the_reference_comparison():
    g = np.load(GOLD)
    recorded = sorted(k[:-len("_crc")] for k in g.files if k.endswith("_crc"))
    assert recorded == sorted(n for n in NAMES if n not in ORACLE_ONLY)
    assert len(ORACLE_ONLY) == 0                                      # the share of cases excluded is zero
    assert len(set(NAMES)) == len(NAMES) == 25


@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_reference_fixture(name):
    g = np.load(GOLD)
    cs = rf.case_named(name)
    assert rf.input_crc(cs) == [int(v) for v in g[name + "_crc"]], "the family code no longer reproduces the inputs the fixture was recorded on"
    check_map_result(g, name, rf.oracle_result(cs))


@pytest.mark.parametrize("name", NAMES)
def test_numpy_restatement_agrees_with_the_oracle(name):
    """the predicates the reach assertions and the stand-ins are built from say what the oracle says (and what the device is asked
    for: the overflow-free item count)"""
    cs = rf.case_named(name)
    res = rf.oracle_result(cs)
    pl = rf.plan(cs)
    assert pl["n_kept"] == rf.n_kept_of_result(cs, res) <= cs["cfg"]["max_items"]
    check_map_result(as_fixture(name, res), name, rf.replay(cs, res))


# ---- reach: cells -----------------------------------------------------------------------------------------------------------
def test_cells_reach_both_sides_of_the_counter_limit_and_the_scan_chunks():
    by = {cs["name"]: cs for cs in rf.family("cells")}
    n_cells = {n: rf.grid(cs)[2] for n, cs in by.items()}
    assert n_cells["cells_lds_2048"] == rf.LDS_CELLS                   # the last size with the counters in LDS
    assert n_cells["cells_global_2112"] == 2112 > rf.LDS_CELLS         # the next size a 2 px grid reaches
    cs = by["cells_cut_54x40"]
    assert rf.grid(cs)[:2] == (54, 40) and cs["cam"].width % 3 and cs["cam"].height % 3 and n_cells["cells_cut_54x40"] > rf.LDS_CELLS
    for name, cs in by.items():
        res, t = rf.oracle_result(cs), cs["tags"]
        feats = set(int(p) for p in res["feat_point"])
        for tag, index in (("cell_first", t["index_first"]), ("cell_last", t["index_last"]), ("cell_below_1024", t["index_below"]),
                           ("cell_from_1024", t["index_above"])):
            assert t[tag] in feats and cell_of_point(cs, t[tag]) == index, (name, tag)
        assert t["index_below"] < 1024 <= t["index_above"]
        # more cells than the scan has threads (1024): every thread sums a chunk of two or three counters, and counters of one
        # chunk are both non-zero somewhere
        per_cell = rf.plan(cs)["per_cell"]
        chunk = -(-(n_cells[name]) // 1024)
        assert chunk >= 2 and any(per_cell[i] and per_cell[i + 1] for i in range(0, n_cells[name] - 1, chunk))
        assert int(res["n_trials"]) > int(res["n_matches"]) > 300       # failures ahead of matches, and cells without any match
        assert (res["unlinked"] == 1).any()
    cs = by["cells_cut_54x40"]
    res, t = rf.oracle_result(cs), cs["tags"]
    on, below = t["edge3_on"], t["edge3_below"]
    assert {on, below} <= set(int(p) for p in res["feat_point"])
    assert rf.project_cur(cs, on)[1][0] == 51.0 and rf.project_cur(cs, below)[1][0] == np.nextafter(51.0, 0.0)
    assert cell_of_point(cs, on) % 54 == 17 and cell_of_point(cs, below) % 54 == 16


# ---- reach: items -----------------------------------------------------------------------------------------------------------
def test_items_reach_both_sides_of_the_sort_key_limit():
    cases = rf.family("items")
    assert [rf.plan(cs)["n_kept"] for cs in cases] == list(rf.ITEM_COUNTS) == [2047, 2048, 2049, 2600]
    assert rf.ITEM_COUNTS[1] == rf.LDS_ITEMS
    for cs in cases:
        res, pl = rf.oracle_result(cs), rf.plan(cs)
        assert rf.n_kept_of_result(cs, res) == pl["n_kept"] <= cs["cfg"]["max_items"]
        crowd = int(np.argmax(pl["per_cell"]))
        assert pl["per_cell"][crowd] > 64
        types = {int(cs["pt_type"][p]) for p, _, c in pl["items"] if c == crowd}
        assert types == {TYPE_DELETED, TYPE_CANDIDATE, TYPE_UNKNOWN, TYPE_GOOD}
        assert len(pl["selected"]) == 4 and min(pl["overlap_count"]) > 0
        assert len(pl["out_candidates"]) > 0
        # the trial order matters: in most cells points fail ahead of the winner, and points that would match are never tried
        assert int(res["n_trials"]) > 3 * int(res["n_matches"]) and int(res["n_matches"]) >= 40


# ---- reach: the crowded cell ------------------------------------------------------------------------------------------------
def test_crowded_cell_holds_what_it_claims():
    cs = rf.family("crowded")[0]
    res, pl = rf.oracle_result(cs), rf.plan(cs)
    crowd = [(seq, p) for seq, (p, _, c) in enumerate(pl["items"]) if c == 1]
    assert len(crowd) >= 300
    pts = np.array([p for _, p in crowd])
    assert {int(t) for t in cs["pt_type"][pts]} == {TYPE_DELETED, TYPE_CANDIDATE, TYPE_UNKNOWN, TYPE_GOOD}
    n_obs = cs["pt_obs_offset"][pts + 1] - cs["pt_obs_offset"][pts]
    assert (n_obs == 3).sum() >= 5                                      # seen from three selected keyframes, projected once
    assert sum(pl["overlap_count"]) + len(cs["cand_point"]) == pl["n_kept"]
    from_kf = {int(cs["obs_kf"][cs["pt_obs_offset"][p]]) for p in pts if cs["pt_type"][p] != TYPE_CANDIDATE}
    assert {0, 1} <= from_kf and (cs["pt_type"][pts] == TYPE_CANDIDATE).sum() >= 30
    assert (cs["kf_ftr_point"] == -1).sum() == 1                        # a feature without a point
    assert res["feat_type"].sum() >= 1 and cs["tags"]["edgelet"] in res["feat_point"]
    grad = res["feat_grad"][list(res["feat_point"]).index(cs["tags"]["edgelet"])]
    assert not np.array_equal(grad, [1.0, 0.0]) and abs(float(grad @ grad) - 1.0) < 1e-12
    # failures ahead of the first success, and untried points behind it
    winner = [p for p in res["feat_point"] if cell_of_point(cs, p) == 1]
    assert len(winner) == 1 and cs["pt_type"][winner[0]] == TYPE_UNKNOWN
    failed = res["n_failed"][pts] - cs["pt_n_failed"][pts]
    assert failed.sum() >= 50 and (failed[cs["pt_type"][pts] == TYPE_GOOD] == 1).all()
    assert (failed[cs["pt_type"][pts] == TYPE_CANDIDATE] == 0).all()
    # the cell whose first success is a point candidate, the cell without one (its deleted points count as trials)
    w2 = [p for p in res["feat_point"] if cell_of_point(cs, p) == 2]
    assert len(w2) == 1 and cs["pt_type"][w2[0]] == TYPE_CANDIDATE
    assert not [p for p in res["feat_point"] if cell_of_point(cs, p) == 3]
    assert int(res["n_trials"]) > int((res["n_failed"] - cs["pt_n_failed"]).sum()) + int(res["n_matches"])


def test_second_frame_over_the_crowded_map_meets_unlinked_points():
    """the first frame deletes points; the frame after it walks feature lists and a candidate list that still name them"""
    cs = rf.family("crowded")[0]
    first = rf.oracle_result(cs)
    assert (first["unlinked"] == 1).sum() >= 3
    state = rf.state_of(first)
    second = orc.reproject_map(cs, cs["kf_key_point"], max_fts=cs["cfg"]["max_fts"], max_n_kfs=cs["cfg"]["reproj_max_n_kfs"], state=rf.state_of(first))
    pl = rf.plan(cs, state)
    assert pl["n_kept"] == rf.plan(cs)["n_kept"] - int((first["unlinked"] == 1).sum())
    check_map_result(as_fixture("second", second), "second", rf.replay(cs, second, state=state))
    assert int(second["n_trials"]) != int(first["n_trials"])


# ---- reach: keyframe selection ----------------------------------------------------------------------------------------------
def test_keyframe_selection_reaches_every_count_limit_and_tie():
    cases = rf.family("kf_selection")
    assert sorted({(cs["n_kf"], cs["cfg"]["reproj_max_n_kfs"]) for cs in cases}) == sorted((n, m) for n in (1, 16, 17, 256) for m in (1, 10, rf.MAX_SEL))
    more = fewer = straddles = inside = 0
    for cs in cases:
        res, t, m = rf.oracle_result(cs), cs["tags"], cs["cfg"]["reproj_max_n_kfs"]
        close, ranked = rf.close_keyframes(cs)
        assert len(close) == t["n_close"]
        sel = [int(k) for k in res["overlap_kf"]]
        assert sel == [k for k, _ in ranked[:m]] and len(sel) == min(m, t["n_close"])
        more += t["n_close"] > m
        fewer += t["n_close"] < m
        dist = dict(close)
        for (first, other), (a, c) in zip(t["tied"], t["tied_ranks"]):
            assert dist[first] == dist[other] and first < other                       # exactly equal: only the index decides
            assert cs["T_kf_w"][first][0] == -cs["T_kf_w"][other][0] > 0
            assert sel[a] == first
            if c < m:
                assert sel[c] == other
                inside += 1
            else:
                assert other not in sel and a == m - 1
                straddles += 1
        assert not set(t["not_close"]) & {k for k, _ in close}
        if t["not_close"]:
            assert len(t["not_close"]) == 3
            if m >= 10:                                    # nearer than the last keyframe selected: taken for close, they would be in
                assert max(abs(cs["T_kf_w"][k][0]) for k in t["not_close"]) < ranked[len(sel) - 1][1]
            assert rf.project_cur(cs, cs["tags"]["key_px_width"])[1][0] == cs["cam"].width
            assert sum(1 for k in t["not_close"] if (cs["kf_key_point"][k] < 0).all()) == 1
            assert sum(1 for k in t["not_close"] if all(cs["pt_pos"][p][2] < 0 for p in cs["kf_key_point"][k] if p >= 0)
                       and (cs["kf_key_point"][k] >= 0).sum() == 2) == 1
        if t["kf_px_0"] >= 0:
            k0 = t["kf_px_0"]
            assert k0 in dist and list(rf.project_cur(cs, cs["tags"]["key_px_0"])[1]) == [0.0, 0.0]
            assert [p for p in cs["kf_key_point"][k0] if p >= 0] == [cs["tags"]["key_px_0"]]
            if m >= 10:
                assert k0 in sel
        # the point every keyframe sees is projected once and counted for the first selected keyframe only
        assert cs["tags"]["shared"] in res["feat_point"] or cs["n_kf"] == 0
        if len(sel) > 1:
            assert res["overlap_count"][0] == 2 and (res["overlap_count"][1:] <= 1).all()
    assert more == 8 and fewer == 3 and straddles >= 5 and inside >= 6
    assert any(cs["n_kf"] == 256 for cs in cases)


# ---- reach: boundaries ------------------------------------------------------------------------------------------------------
def test_boundary_points_fall_on_the_side_they_were_made_for():
    cs = rf.family("boundaries")[0]
    res, t = rf.oracle_result(cs), cs["tags"]
    w, h = cs["cam"].width, cs["cam"].height
    for name, inside in t["expect_in"].items():
        p = t[name]
        px = rf.project_cur(cs, p)[1]
        axis = 0 if name.startswith("x_") else 1
        bound = {"at_8": 8.0, "at_max": (w, h)[axis] - 8.0}.get(name[2:name.rindex("_")])
        if bound is not None:
            assert px[axis] == bound, name
        else:
            upper = 8.0 if "below_8" in name else (w, h)[axis] - 8.0
            assert px[axis] < upper and upper - px[axis] < 1e-13, name
        if name.endswith("_map"):
            assert changed(cs, res, p) == inside, name                  # a map point out of the frame is not touched
            if inside:
                assert p in res["feat_point"], name
        else:
            d = int(res["n_failed"][p] - cs["pt_n_failed"][p])
            assert d == (0 if inside else 3), name
            assert (p in res["feat_point"]) == inside, name
    feats = [int(p) for p in res["feat_point"]]
    for a, b in (("cell_edge_x_below", "cell_edge_x_on"), ("cell_edge_y_below", "cell_edge_y_on")):
        assert t[a] in feats and t[b] in feats and feats.index(t[a]) < feats.index(t[b])
        assert cell_of_point(cs, t[b]) - cell_of_point(cs, t[a]) == (1 if "_x_" in a else 16)
    assert rf.project_cur(cs, t["cell_edge_x_on"])[1][0] == 48.0 and rf.project_cur(cs, t["cell_edge_x_below"])[1][0] == np.nextafter(48.0, 0.0)
    assert rf.project_cur(cs, t["cell_edge_y_on"])[1][1] == 40.0 and rf.project_cur(cs, t["cell_edge_y_below"])[1][1] == np.nextafter(40.0, 0.0)
    # z == 0: not in the frame -- a map point is left alone, a candidate takes its three failures
    assert np.isinf(rf.project_cur(cs, t["z0_inf_map"])[1][0]) and np.isnan(rf.project_cur(cs, t["z0_nan_map"])[1]).all()
    for tag in ("z0_inf_map", "z0_nan_map"):
        assert not changed(cs, res, t[tag])
    for tag in ("z0_inf_cand", "z0_nan_cand"):
        assert res["n_failed"][t[tag]] - cs["pt_n_failed"][t[tag]] == 3
    # behind the camera: projected into the frame and tried like any other point
    for tag in ("behind_map", "behind_cand"):
        assert cs["pt_pos"][t[tag]][2] < 0 and rf.in_frame(cs, rf.project_cur(cs, t[tag])[1]) and changed(cs, res, t[tag])
    after = lambda tag: (int(res["type"][t[tag]]), int(res["n_failed"][t[tag]]), int(res["n_succeeded"][t[tag]]), int(res["unlinked"][t[tag]]))
    assert after("out_27") == (TYPE_CANDIDATE, 30, 0, 0) and after("out_28") == (TYPE_DELETED, 31, 0, 1)
    assert after("unknown_14") == (TYPE_UNKNOWN, 15, 0, 0) and after("unknown_15") == (TYPE_DELETED, 16, 0, 1)
    assert after("good_40") == (TYPE_GOOD, 41, 0, 0)
    assert after("cand_29") == (TYPE_CANDIDATE, 30, 0, 0) and after("cand_30") == (TYPE_DELETED, 31, 0, 1)
    assert after("succeeded_9") == (TYPE_UNKNOWN, 0, 10, 0) and after("succeeded_10") == (TYPE_GOOD, 0, 11, 0)
    assert after("no_close_view") == (TYPE_DELETED, 16, 0, 1) and not rf.close_view_obs(cs, t["no_close_view"])[1]


# ---- reach: the cut ---------------------------------------------------------------------------------------------------------
def test_cut_cases_stop_where_they_claim():
    by = {cs["name"]: cs for cs in rf.family("cut")}
    n = rf.N_CUT_MATCHES
    res = {name: rf.oracle_result(cs) for name, cs in by.items()}
    after = [by["cut_none"]["tags"]["after_%d" % i] for i in range(6)]
    assert by["cut_max_fts_0"]["cfg"]["max_fts"] == 0 and int(res["cut_max_fts_0"]["n_matches"]) == 1 and int(res["cut_max_fts_0"]["n_trials"]) == 1
    r = res["cut_in_last_match"]
    assert by["cut_in_last_match"]["cfg"]["max_fts"] == n - 1 and int(r["n_matches"]) == n                # n_matches EXCEEDS max_fts, then stops
    assert list(r["feat_point"]) == [by["cut_none"]["tags"]["match_%d" % i] for i in range(n)]
    assert (r["n_failed"][after] == 15).all() and not r["unlinked"].any()                              # the cells behind the cut stay untried
    r = res["cut_none"]
    assert int(r["n_matches"]) == n and list(r["feat_point"]) == list(res["cut_in_last_match"]["feat_point"])
    assert (r["n_failed"][after] == 16).all() and (r["unlinked"][after] == 1).all()
    assert int(r["n_trials"]) > int(res["cut_in_last_match"]["n_trials"])
    # the refinement's threshold: n_matches < quality_min_fts returns before it
    assert by["cut_none"]["cfg"]["quality_min_fts"] == int(r["n_matches"])
    assert by["cut_quality_above"]["cfg"]["quality_min_fts"] == int(res["cut_quality_above"]["n_matches"]) + 1


# ---- the comparison has teeth -----------------------------------------------------------------------------------------------
def rejected(name, res, wrong):
    with pytest.raises(AssertionError):
        check_map_result(as_fixture(name, res), name, wrong)
    return True


def test_comparison_rejects_swapped_tied_keyframes():
    n_rejected = 0
    for name in ("kf_n17_m10", "kf_n256_m16", "kf_n16_m1"):
        cs = rf.case_named(name)
        res = rf.oracle_result(cs)
        check_map_result(as_fixture(name, res), name, rf.replay(cs, res))
        sel = [int(k) for k in res["overlap_kf"]]
        for first, other in cs["tags"]["tied"]:
            swapped = [other if k == first else first if k == other else k for k in sel]
            assert swapped != sel
            n_rejected += rejected(name, res, rf.replay(cs, res, selection=swapped))
    assert n_rejected == 5


def test_comparison_rejects_a_crowded_cell_tried_in_point_index_order():
    for name in ("crowded", "items_2049"):
        cs = rf.case_named(name)
        res = rf.oracle_result(cs)
        check_map_result(as_fixture(name, res), name, rf.replay(cs, res))
        assert rejected(name, res, rf.replay(cs, res, order="index"))


def test_comparison_rejects_the_cut_at_max_fts():
    cs = rf.case_named("cut_in_last_match")
    res = rf.oracle_result(cs)
    check_map_result(as_fixture(cs["name"], res), cs["name"], rf.replay(cs, res))
    wrong = rf.replay(cs, res, cut="ge")
    assert int(wrong["n_matches"]) == int(res["n_matches"]) - 1
    assert rejected(cs["name"], res, wrong)
