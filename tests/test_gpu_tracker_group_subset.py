"""svo_hip_tracker_group_track_some: any subset of a group's cameras tracks in one call, the others sit it out untouched.
What is checked, every comparison byte for byte (tests/test_gpu_tracker_invariance.py's _same: every field of the result, the
frame's features, the point counters, the overlap lists): a camera's frames through subset calls are a lone tracker's on the
same frames; a camera that sits out keeps its result block, its map tables, its key points, its keyframe decision and the bytes
of its last frame's pyramid; the full list is svo_hip_tracker_group_track; every refusal leaves the group as it was."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_growth_scenario as sc
import tracker_odd_cases as toc
import tracking_chain as tc
from test_gpu_tracker_invariance import CFG, _same, _start, _tile_order
from android_svo_amd import hip, synth

pytestmark = pytest.mark.gpu

N_FRAMES = 12


@pytest.fixture(scope="module")
def ctx():
    c = hip.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _seq(n_map):
    return tc.make_sequence(n_frames=N_FRAMES, n_map=n_map)


def _lone(ctx, seq, frames, tile_order=True, mp=None, cfg=CFG):
    """a lone tracker over `frames` of seq from keyframe 0: the per-frame results"""
    trk = hip.Tracker(ctx, seq["cam"], **cfg)
    if tile_order:
        _tile_order(trk)
    _start(trk, seq, mp or tc.sequence_map(seq))
    out = [trk.track(seq["pyrs"][k][0]) for k in frames]
    trk.destroy()
    return out


def _map_bytes(m):
    return {k: (v.tobytes() if hasattr(v, "tobytes") else v) for k, v in m.items()}


def _assert_pyramid(cam_trk, want, what):
    pyr, slot = cam_trk.last_frame_pyramid()
    for l in range(pyr.n_levels):
        assert pyr.download_level(slot, l).tobytes() == want[l].tobytes(), (what, slot, l)


def test_staggered_schedule(ctx):
    """A group of 4 over 10 calls: camera 0 in every call, camera 1 in every other one, camera 3 in exactly one, camera 2 set up
    only before call 4 and in every call from then on.  Both rules of the frame batches occur (one, two and three of four)."""
    seqs = [_seq(600), _seq(530), _seq(600), _seq(530)]
    active_in = lambda i: [0] + ([1] if i % 2 == 0 else []) + ([2] if i >= 4 else []) + ([3] if i == 5 else [])
    n_tracked = [sum(c in active_in(i) for i in range(10)) for c in range(4)]
    assert n_tracked == [10, 5, 6, 1]
    want = [_lone(ctx, seqs[c], range(1, n_tracked[c] + 1)) for c in range(4)]
    grp = hip.TrackerGroup(ctx, seqs[0]["cam"], 4, **CFG)
    _tile_order(grp)
    for c in (0, 1, 3):
        _start(grp.cameras[c], seqs[c], tc.sequence_map(seqs[c]))
    done = [0, 0, 0, 0]                         # frames tracked per camera: its last frame is frame done[c] of its sequence
    held = {}                                   # what a camera showed after its last tracked frame
    for i in range(10):
        if i == 4:
            _start(grp.cameras[2], seqs[2], tc.sequence_map(seqs[2]))
        maps_before = {c: _map_bytes(grp.cameras[c].download_map()) for c in range(4) if c != 2 or i >= 4}
        act = active_in(i)
        res = grp.track_some(act, [seqs[c]["pyrs"][done[c] + 1][0] for c in act])
        for j, c in enumerate(act):
            done[c] += 1
            got = grp.cameras[c].last_result()
            _same(got, want[c][done[c] - 1], (i, c))
            assert list(res[j].T_f_w) == list(got["T_f_w"])
            held[c] = got
        for c in range(4):
            if c == 2 and i < 4:                # never set up: no result, no map, no last frame
                with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
                    grp.cameras[c].last_result()
                with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
                    grp.cameras[c].last_frame_pyramid()
                continue
            if c not in act:
                if c in held:
                    _same(grp.cameras[c].last_result(), held[c], (i, c, "sat out"))
                else:
                    with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
                        grp.cameras[c].last_result()
                assert _map_bytes(grp.cameras[c].download_map()) == maps_before[c], (i, c)
            _assert_pyramid(grp.cameras[c], seqs[c]["pyrs"][done[c]], (i, c))
        views = [grp.cameras[c].last_frame_pyramid() for c in range(4) if c != 2 or i >= 4]
        assert len({p.h.value for p, _ in views}) == 1                         # one batch holds every camera's last frame
    assert done == n_tracked
    grp.destroy()


def test_shape_is_chosen_by_the_cameras_of_the_call(ctx):
    """The default reduction: cameras 1 and 3 of a group of 4 equal a group of 2 made of those two cameras -- same slot count,
    same feature counts -- although camera 0 holds a 600-feature last frame, another shape class than their 420 (7 against 10
    tiles: tests/test_gpu_tracker_group.py) and camera 2 was never set up."""
    big, small = _seq(600), _seq(420)
    two = hip.TrackerGroup(ctx, small["cam"], 2, **CFG)
    for t in two.cameras:
        _start(t, small, tc.sequence_map(small))
    want = []
    for k in range(1, 4):
        two.track([small["pyrs"][k][0], small["pyrs"][k + 1][0]])
        want.append([t.last_result() for t in two.cameras])
    two.destroy()
    grp = hip.TrackerGroup(ctx, small["cam"], 4, **CFG)
    _start(grp.cameras[0], big, tc.sequence_map(big))
    for c in (1, 3):
        _start(grp.cameras[c], small, tc.sequence_map(small))
    for k in range(1, 4):
        grp.track_some([1, 3], [small["pyrs"][k][0], small["pyrs"][k + 1][0]])
        _same(grp.cameras[1].last_result(), want[k - 1][0], (k, 1))
        _same(grp.cameras[3].last_result(), want[k - 1][1], (k, 3))
    grp.destroy()


@pytest.mark.parametrize("n", [1, 2, 17])
def test_full_list_is_the_group_call(ctx, n):
    seq = _seq(530)
    mp = tc.sequence_map(seq)
    grps = [hip.TrackerGroup(ctx, seq["cam"], n, **CFG) for _ in range(2)]
    for g in grps:
        for t in g.cameras:
            _start(t, seq, mp)
    for k in range(1, 4):
        imgs = [seq["pyrs"][k + c % 3][0] for c in range(n)]
        a = grps[0].track_some(range(n), imgs)
        b = grps[1].track(imgs)
        for c in range(n):
            _same(grps[0].cameras[c].last_result(), grps[1].cameras[c].last_result(), (n, k, c))
            assert list(a[c].T_f_w) == list(b[c].T_f_w) and a[c].n_matches == b[c].n_matches
    for g in grps:
        g.destroy()


def test_one_and_sixteen_of_seventeen(ctx):
    """One camera of 17 in the call: the kernel shape is a lone tracker's, so the results are too in the default reduction.
    16 of 17 (tile order on both sides): every camera its lone tracker."""
    seq = _seq(530)
    mp = tc.sequence_map(seq)
    want = _lone(ctx, seq, [1, 2], tile_order=False)
    grp = hip.TrackerGroup(ctx, seq["cam"], 17, **CFG)
    _start(grp.cameras[5], seq, mp)
    for k in (1, 2):
        grp.track_some([5], [seq["pyrs"][k][0]])
        _same(grp.cameras[5].last_result(), want[k - 1], ("one of 17", k))
    grp.destroy()
    want = _lone(ctx, seq, [1, 2])
    grp = hip.TrackerGroup(ctx, seq["cam"], 17, **CFG)
    _tile_order(grp)
    act = [c for c in range(17) if c != 3]
    for c in act:
        _start(grp.cameras[c], seq, mp)
    for k in (1, 2):
        grp.track_some(act, [seq["pyrs"][k][0]] * 16)
        for c in act:
            _same(grp.cameras[c].last_result(), want[k - 1], ("16 of 17", k, c))
    grp.destroy()


def test_edits_while_a_camera_sits_out(ctx):
    """Camera 0 sits out two calls and meanwhile gets candidates, turns its last frame into a keyframe, loses that keyframe
    again and has its points renumbered; camera 1 sits out the second of them and gets a map uploaded.  Both rejoin and equal
    lone trackers that did the same between the same frames."""
    s = sc.make()
    seq, base = s["seq"], s["base"]
    full_map = tc.sequence_map(seq)
    cfg = dict(CFG, max_points=2048, max_obs=8192, max_kf_features=4096, max_candidates=512)

    def edits0_a(t):
        return t.add_candidates(**s["cand"]), t.promote_last_frame(1)

    def edits0_b(t):
        r = t.remove_keyframe(1)
        return r, t.compact_points()["n_points"]

    def run(track, cams):
        """cams[c]: the tracker; track(active, frames) -> nothing.  Returns what the edits reported."""
        track([0, 1, 2], [1, 1, 1]); track([0, 1, 2], [2, 2, 2])
        a = edits0_a(cams[0])
        track([1, 2], [3, 3])
        b = edits0_b(cams[0])
        cams[1].set_map(full_map)
        track([2], [4])
        track([0, 1, 2], [3, 4, 5]); track([0, 1, 2], [4, 5, 6])
        return a, b
    want, lone = [[], [], []], []
    for c in range(3):
        t = hip.Tracker(ctx, seq["cam"], **cfg)
        _tile_order(t)
        _start(t, base if c == 0 else seq, s["base_map"] if c == 0 else full_map)
        lone.append(t)

    def lone_track(active, frames):
        for c, k in zip(active, frames):
            want[c].append(lone[c].track(seq["pyrs"][k][0]))
    want_edits = run(lone_track, lone)
    want_maps = [_map_bytes(t.download_map()) for t in lone]
    for t in lone:
        t.destroy()
    grp = hip.TrackerGroup(ctx, seq["cam"], 3, **cfg)
    _tile_order(grp)
    _start(grp.cameras[0], base, s["base_map"])
    for c in (1, 2):
        _start(grp.cameras[c], seq, full_map)
    got = [[], [], []]

    def group_track(active, frames):
        grp.track_some(active, [seq["pyrs"][k][0] for k in frames])
        for c in active:
            got[c].append(grp.cameras[c].last_result())
    got_edits = run(group_track, grp.cameras)
    assert repr(got_edits) == repr(want_edits) and got_edits[0] == (s["base_map"]["n_points"], (1, 0))
    for c in range(3):
        assert len(got[c]) == len(want[c]) == (4, 5, 6)[c]
        for i, (a, b) in enumerate(zip(got[c], want[c])):
            _same(a, b, (c, i))
        assert _map_bytes(grp.cameras[c].download_map()) == want_maps[c], c
    grp.destroy()


def test_a_reselection_owed_across_a_call(ctx):
    """tests/test_gpu_tracker_group.py::test_group_cameras_over_maps_that_lose_points with the camera whose frame deleted points
    sitting out the next call: the re-selection of key points it owes stays owed across that call."""
    from test_oracle_reproject_map import CASES, GOLD
    tag, kw, max_fts = [c for c in CASES if c[0] == "rekey"][0]
    g = np.load(GOLD)
    cs = synth.make_map_case(**kw)
    key = g[tag + "_kf_key_point"].copy()
    scene = synth.PlaneScene(seed=kw.get("seed", 31), depth=2.0, tilt=(0.08, -0.05))
    step = synth.se3_from_twist([0.011, -0.005, 0.003], [0.0015, -0.0025, 0.001])
    poses = [cs["T_cur_w"]]
    for _ in range(5):
        poses.append(synth.se3_mul(step, poses[-1]))
    pyrs = [cs["cur_pyr"]] + [synth.build_pyramid(scene.render(cs["cam"], T)) for T in poses[1:]]
    cfg = dict(max_keyframes=max(cs["n_kf"], 1), grid_size=cs["cell_size"], max_fts=max_fts, quality_min_fts=20, max_items=16384)
    frames = [[0, 1, 2, 3, 4, 5], [0, 0, 1, 2, 3, 4]]

    def setup(trk):
        _tile_order(trk)
        for k in range(cs["n_kf"]):
            trk.upload_keyframe(k, cs["kf_pyr"][k][0])
        trk.set_map(dict(cs, kf_slot=np.arange(cs["n_kf"], dtype=np.int32), kf_key_point=key))
        trk.set_last_frame(cs["T_cur_w"], np.zeros((0, 2)), np.zeros((0, 3)), np.zeros(0, np.int32), img=pyrs[0][0])
    grp = hip.TrackerGroup(ctx, cs["cam"], 2, **cfg)
    for t in grp.cameras:
        setup(t)
    got, owed_across, sits_out = [[], []], 0, {1}          # (camera 1 joins a call later, so that the two do not sit out together)
    for _ in range(9):
        act = [c for c in range(2) if c not in sits_out and len(got[c]) < 6]
        owed_across += sum(1 for c in sits_out if act and got[c] and got[c][-1]["map_changed"])
        sits_out = set()
        grp.track_some(act, [pyrs[frames[c][len(got[c])]][0] for c in act])
        for c in act:
            got[c].append(grp.cameras[c].last_result())
            if got[c][-1]["map_changed"]:
                sits_out.add(c)
    keys = [t.download_key_points(cs["n_kf"]) for t in grp.cameras]
    grp.destroy()
    assert sum(r["map_changed"] for rs in got for r in rs) >= 3 and owed_across >= 2
    assert min(len(rs) for rs in got) >= 4
    for c in range(2):
        trk = hip.Tracker(ctx, cs["cam"], **cfg)
        setup(trk)
        for i in range(len(got[c])):
            _same(got[c][i], trk.track(pyrs[frames[c][i]][0]), (c, i))
        np.testing.assert_array_equal(keys[c], trk.download_key_points(cs["n_kf"]))
        trk.destroy()
    assert (keys[0] != key).any() or (keys[1] != key).any()


def _decision_bytes(d):
    return {k: (v.tobytes() if hasattr(v, "tobytes") else np.float64(v).tobytes() if isinstance(v, float) else v) for k, v in d.items()}


def test_keyframe_decision_after_a_subset_call(ctx):
    seq = _seq(530)
    mp = tc.sequence_map(seq)
    lone = hip.Tracker(ctx, seq["cam"], **CFG)
    _tile_order(lone)
    _start(lone, seq, mp)
    want = []
    for k in (1, 2):
        lone.track(seq["pyrs"][k][0])
        want.append(_decision_bytes(lone.finish_frame([], 0)[2]))
    lone.destroy()
    grp = hip.TrackerGroup(ctx, seq["cam"], 3, **CFG)
    _tile_order(grp)
    for t in grp.cameras:
        _start(t, seq, mp)
    grp.track_some([0, 1, 2], [seq["pyrs"][1][0]] * 3)
    before = [_decision_bytes(d) for _, _, d in grp.finish_frames()]
    assert before == [want[0]] * 3 and want[0]["overlap_valid"] == 1
    grp.track_some([0, 2], [seq["pyrs"][2][0]] * 2)
    after = [_decision_bytes(d) for _, _, d in grp.finish_frames()]
    assert after[0] == after[2] == want[1] and want[1] != want[0]
    assert after[1] == before[1]                                               # camera 1 sat out: the decision it gave before
    grp.destroy()


def test_odd_size_staggered(ctx):
    """346x260 (pyramids of 120 063 bytes, no multiple of 16: the slot copy's head and tail; the per-level build over a list of
    slots): two of three cameras, then one, then all."""
    w, h = toc.SIZES[0]
    seq = toc.sequence(w, h)
    mp = tc.sequence_map(seq)
    calls = [[0, 2], [1], [0, 1, 2]]
    n_tracked = [sum(c in a for a in calls) for c in range(3)]
    want = [_lone(ctx, seq, [c + 1 + i for i in range(n_tracked[c])]) for c in range(3)]
    grp = hip.TrackerGroup(ctx, seq["cam"], 3, **CFG)
    _tile_order(grp)
    for t in grp.cameras:
        _start(t, seq, mp)
    assert grp.cameras[0].last_frame_pyramid()[0].download_level(0, 0).size == w * h
    done, last = [0, 0, 0], [0, 0, 0]
    for i, act in enumerate(calls):
        grp.track_some(act, [seq["pyrs"][c + 1 + done[c]][0] for c in act])
        for c in act:
            last[c] = c + 1 + done[c]
            done[c] += 1
            _same(grp.cameras[c].last_result(), want[c][done[c] - 1], (i, c))
        for c in range(3):
            _assert_pyramid(grp.cameras[c], seq["pyrs"][last[c]], (i, c))
    assert all(r["n_matches"] >= 50 for rs in want for r in rs)
    grp.destroy()


def test_refusals_change_nothing(ctx):
    seq = _seq(530)
    mp = tc.sequence_map(seq)
    want = _lone(ctx, seq, range(1, N_FRAMES))
    img = np.ascontiguousarray(seq["pyrs"][1][0])
    p8 = C.POINTER(C.c_uint8)
    imgs3 = (p8 * 3)(*[img.ctypes.data_as(p8)] * 3)
    res = (hip.CTrackResult * 3)()
    lib = ctx.lib
    grp = hip.TrackerGroup(ctx, seq["cam"], 3, **CFG)
    _tile_order(grp)
    for t in grp.cameras:
        _start(t, seq, mp)
    idx = lambda *v: (C.c_int32 * max(len(v), 1))(*v)
    two_imgs_one_null = (p8 * 3)(img.ctypes.data_as(p8), None, None)
    refusals = [
        ("null group", lambda: lib.svo_hip_tracker_group_track_some(None, 1, idx(0), imgs3, res)),
        ("n_active < 0", lambda: lib.svo_hip_tracker_group_track_some(grp.h, -1, idx(0), imgs3, res)),
        ("n_active > n_cameras", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 4, idx(0, 1, 2, 3), imgs3, res)),
        ("null list", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, None, imgs3, res)),
        ("null images", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(0, 1), None, res)),
        ("index out of range", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(1, 3), imgs3, res)),
        ("negative index", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(-1, 1), imgs3, res)),
        ("repeated index", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(1, 1), imgs3, res)),
        ("decreasing list", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(2, 1), imgs3, res)),
        ("null image", lambda: lib.svo_hip_tracker_group_track_some(grp.h, 2, idx(0, 1), two_imgs_one_null, res)),
    ]
    assert len(refusals) + 1 <= len(want)
    for k, (what, call) in enumerate(refusals, 1):
        assert call() == -1, what                                              # SVO_HIP_ERR_INVALID
        grp.track([seq["pyrs"][k][0]] * 3)                                     # the lone tracker's next frame: nothing was enqueued or changed
        for c in range(3):
            _same(grp.cameras[c].last_result(), want[k - 1], (what, c))
    # nobody in the call: nothing happens
    assert lib.svo_hip_tracker_group_track_some(grp.h, 0, None, None, None) == 0
    assert grp.track_some([], []) == []
    k = len(refusals) + 1
    grp.track([seq["pyrs"][k][0]] * 3)
    _same(grp.cameras[1].last_result(), want[k - 1], "after the empty call")
    with pytest.raises(hip.SvoHipError, match=r"\(-1\)"):                       # svo_hip_tracker_group_track keeps refusing a null image
        ctx.check(lib.svo_hip_tracker_group_track(grp.h, two_imgs_one_null, None), "tracker_group_track")
    grp.destroy()
    # a camera of the call without its map / last frame: SVO_HIP_ERR_STATE; without it in the call: tracked
    grp = hip.TrackerGroup(ctx, seq["cam"], 3, **CFG)
    _tile_order(grp)
    _start(grp.cameras[0], seq, mp)
    grp.cameras[2].upload_keyframe(0, seq["pyrs"][0][0])
    grp.cameras[2].set_map(mp)                                                  # a map, no last frame
    for act in ([0, 1], [1], [0, 2]):
        with pytest.raises(hip.SvoHipError, match=r"\(-4\)"):
            grp.track_some(act, [seq["pyrs"][1][0]] * len(act))
    grp.track_some([0], [seq["pyrs"][1][0]])
    _same(grp.cameras[0].last_result(), want[0], "after the state refusals")
    grp.destroy()
