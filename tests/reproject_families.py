"""Constructed maps for Reprojector::reprojectMap that reach, by construction, the data-dependent paths of the planning and
replay kernels (trk_plan_body / trk_replay_body, csrc/svo_track_chain.h), and those kernels' path conditions restated as
predicates in numpy.

Plain numpy, no GPU.  A case is a dict in the table layout of synth.make_map_case (what hip.Tracker.set_map and
orc.reproject_map take) plus name, kf_slot, kf_key_point, cfg (the tracker configuration the case runs under) and tags (names
for the points and keyframes the reach assertions look at).  The predicates (plan, replay) only say which path a case takes
and build deliberately wrong stand-ins; expected results always come from the oracle.

Construction: a dyadic pinhole camera (fx = fy = 128, cx = cy powers of two) and points at depth 2 seen from a current frame
at the identity, so that a point made for pixel (u, v) projects to exactly (u, v) whenever u and v are dyadic.  Keyframe 0
sits at the identity too and holds the current image: a point observed there matches at once.  A keyframe translated by t
along x or y holds either the current image rolled by 64 t pixels (the same fronto-parallel plane: its points match) or
the image of bland() (its points fail in the alignment).  Two more ways to fail, both decided before any image is read: an
observation within 6 px of its keyframe's border (the matcher's frame test) and a keyframe 8 m to the side (no close view).

isInFrame(px, 8) keeps every item 8 px away from the border, so the cells of the first and last rows and columns of a fine
grid can never hold one: "first" and "last" cell below mean the first and last cell that can.
"""
import math
import zlib

import numpy as np

from android_svo_amd import synth
from android_svo_amd.synth import TYPE_CANDIDATE, TYPE_DELETED, TYPE_GOOD, TYPE_UNKNOWN

IDENTITY = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
DEPTH = 2.0
F = 128.0
LDS_CELLS = 2048          # TRK_LDS_CELLS
LDS_ITEMS = 2048          # TRK_LDS_ITEMS
MAX_SEL = 16              # TRK_MAX_SEL
DEFAULT_CFG = dict(max_fts=1200, reproj_max_n_kfs=10, quality_min_fts=8, max_items=4096)


def camera(width, height):
    return synth.Camera(width, height, F, F, 64.0, 32.0 if height <= 64 else 64.0)


def texture(rng, h, w):
    """noise with structure at two scales (the alignment needs gradients)"""
    coarse = np.kron(rng.integers(0, 256, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), dtype=np.int64))[:h, :w]
    fine = rng.integers(0, 256, (h, w))
    return np.ascontiguousarray((0.6 * coarse + 0.4 * fine).astype(np.uint8))


def bland(h, w):
    """a keyframe image whose points fail in the matcher: slow waves of small amplitude -- the alignment has gradients to work
    with (no singular system), takes steps far too large on the current image's texture and does not converge.  (Unrelated noise
    does not do: the alignment settles on it.)"""
    return np.ascontiguousarray((128 + 20 * np.sin(np.arange(w) / 9.0)[None, :] + 20 * np.cos(np.arange(h) / 7.0)[:, None]).astype(np.uint8))


def pose(tx=0.0, ty=0.0, tz=0.0):
    return np.array([tx, ty, tz, 0.0, 0.0, 0.0, 1.0])


def rolled(img, T):
    """the image a keyframe at the pure x/y translation T sees of the plane z = 2 that shows `img` to the identity"""
    sx, sy = 64.0 * T[0], 64.0 * T[1]
    assert sx == int(sx) and sy == int(sy)
    return np.ascontiguousarray(np.roll(img, (int(sy), int(sx)), axis=(0, 1)))


class MapBuilder:
    def __init__(self, name, cam, cell_size, cur_img, kfs, **cfg):
        """kfs: [(T_kf_w, image)]"""
        self.name, self.cam, self.cell_size, self.cur_img = name, cam, int(cell_size), cur_img
        self.kf_T = [np.asarray(T, dtype=np.float64) for T, _ in kfs]
        self.kf_img = [img for _, img in kfs]
        self.cfg = dict(DEFAULT_CFG, **cfg)
        self.pos, self.type, self.nf, self.ns, self.obs_off = [], [], [], [], [0]
        self.o_point, self.o_kf, self.o_px, self.o_level, self.o_edge, self.o_grad = [], [], [], [], [], []
        self.fts = [[] for _ in kfs]
        self.cand, self.key, self.tags = [], {}, {}

    def at(self, u, v, z=DEPTH):
        """the point of depth z that the identity frame sees at pixel (u, v)"""
        return np.array([(u - self.cam.cx) / F * z, (v - self.cam.cy) / F * z, z])

    def project(self, k, pos):
        p = synth.se3_act(self.kf_T[k], np.asarray(pos, dtype=np.float64))
        return np.array([F * (p[0] / p[2]) + self.cam.cx, F * (p[1] / p[2]) + self.cam.cy])

    def point(self, pos, ptype, kfs, n_failed=0, n_succeeded=0, tag=None, candidate=False, px=None, edgelet=None, level=0):
        """a map point observed from the keyframes `kfs` (Point::obs_ order); px: {kf: pixel} instead of the projection;
        edgelet: {kf: (gx, gy)}.  A candidate has one observation that lies in no feature list."""
        p = len(self.pos)
        self.pos.append(np.asarray(pos, dtype=np.float64)); self.type.append(int(ptype)); self.nf.append(int(n_failed)); self.ns.append(int(n_succeeded))
        assert not candidate or (len(kfs) == 1 and ptype == TYPE_CANDIDATE)
        for k in kfs:
            o = len(self.o_point)
            q = np.asarray(px[k], dtype=np.float64) if px and k in px else self.project(k, pos)
            if not np.isfinite(q).all():
                q = np.array([self.cam.cx, self.cam.cy])
            self.o_point.append(p); self.o_kf.append(k); self.o_px.append(q); self.o_level.append(level)
            g = edgelet.get(k) if edgelet else None
            self.o_edge.append(0 if g is None else 1); self.o_grad.append((1.0, 0.0) if g is None else g)
            if candidate:
                self.cand.append((p, o))
            else:
                self.fts[k].append(o)
        self.obs_off.append(len(self.o_point))
        if tag:
            self.tags[tag] = p
        return p

    def hole(self, k):
        """a feature of keyframe k without a point (kf_ftr_point == -1)"""
        self.fts[k].append(-1)

    def case(self):
        cam, n_kf = self.cam, len(self.kf_T)
        o_point = np.array(self.o_point, np.int32)
        pyr_of = {}

        def pyr(img):
            if id(img) not in pyr_of:
                pyr_of[id(img)] = synth.build_pyramid(img)
            return pyr_of[id(img)]
        off, ftr_obs = [0], []
        for k in range(n_kf):
            ftr_obs.extend(self.fts[k])
            off.append(len(ftr_obs))
        ftr_obs = np.array(ftr_obs, np.int32).reshape(-1)
        ftr_point = np.where(ftr_obs >= 0, o_point[np.maximum(ftr_obs, 0)] if len(o_point) else -1, -1).astype(np.int32)
        key = np.full((n_kf, 5), -1, np.int32)
        for k in range(n_kf):
            if k in self.key:
                key[k, :len(self.key[k])] = self.key[k]
            else:
                own = [o for o in self.fts[k] if o >= 0]
                if own:
                    key[k, 0] = o_point[own[0]]
            for p in key[k]:                  # the reference harness finds a key feature among the keyframe's own features
                assert p < 0 or any(o >= 0 and o_point[o] == p for o in self.fts[k]), (self.name, k, p)
        obs_px = np.array(self.o_px, dtype=np.float64).reshape(-1, 2)
        return dict(name=self.name, cfg=dict(self.cfg), tags=dict(self.tags), cam=cam, cell_size=self.cell_size,
                    kf_pyr=[pyr(img) for img in self.kf_img], cur_pyr=pyr(self.cur_img), T_kf_w=np.stack(self.kf_T), T_cur_w=IDENTITY.copy(),
                    n_kf=n_kf, n_points=len(self.pos), pt_pos=np.array(self.pos, dtype=np.float64).reshape(-1, 3),
                    pt_type=np.array(self.type, np.int32), pt_n_failed=np.array(self.nf, np.int32), pt_n_succeeded=np.array(self.ns, np.int32),
                    pt_obs_offset=np.array(self.obs_off, np.int32), obs_point=o_point, obs_kf=np.array(self.o_kf, np.int32), obs_px=obs_px,
                    obs_f=np.ascontiguousarray(synth.cam2world(cam, obs_px)), obs_level=np.array(self.o_level, np.int32),
                    obs_edgelet=np.array(self.o_edge, np.uint8), obs_grad=np.array(self.o_grad, dtype=np.float64).reshape(-1, 2),
                    kf_ftr_offset=np.array(off, np.int32), kf_ftr_obs=ftr_obs, kf_ftr_point=ftr_point,
                    cand_point=np.array([c[0] for c in self.cand], np.int32), cand_obs=np.array([c[1] for c in self.cand], np.int32),
                    kf_slot=np.arange(n_kf, dtype=np.int32), kf_key_point=key)


def reference_view(cs):
    """the case as the reference harness can hold it: a feature without a point takes part in nothing, so the feature lists go
    without their holes (the order of the others, which is all that counts, stays)"""
    keep = cs["kf_ftr_obs"] >= 0
    off = np.concatenate([[0], np.cumsum([keep[cs["kf_ftr_offset"][k]:cs["kf_ftr_offset"][k + 1]].sum() for k in range(cs["n_kf"])])]).astype(np.int32)
    return dict(cs, kf_ftr_offset=off, kf_ftr_obs=cs["kf_ftr_obs"][keep], kf_ftr_point=cs["kf_ftr_point"][keep])


def fresh_state(cs):
    return {"pt_type": cs["pt_type"].astype(np.int32).copy(), "pt_n_failed": cs["pt_n_failed"].astype(np.int32).copy(),
            "pt_n_succeeded": cs["pt_n_succeeded"].astype(np.int32).copy(), "unlinked": np.zeros(cs["n_points"], np.uint8)}


def state_of(res):
    """the map state a result leaves behind, for the next frame over the same map"""
    return {"pt_type": np.asarray(res["type"], np.int32).copy(), "pt_n_failed": np.asarray(res["n_failed"], np.int32).copy(),
            "pt_n_succeeded": np.asarray(res["n_succeeded"], np.int32).copy(), "unlinked": np.asarray(res["unlinked"], np.uint8).copy()}


# ---- the planning kernel's decisions in numpy (predicates; not a reference) ---------------------------------------------
def project_cur(cs, p):
    with np.errstate(all="ignore"):
        q = synth.se3_act(cs["T_cur_w"], cs["pt_pos"][p])
        return q, np.array([cs["cam"].fx * (q[0] / q[2]) + cs["cam"].cx, cs["cam"].fy * (q[1] / q[2]) + cs["cam"].cy])


def in_frame(cs, px, boundary=8):
    if not np.isfinite(px).all():
        return False                      # (the reference's cast of such a value is undefined; every build at hand leaves the frame)
    ix, iy = int(px[0]), int(px[1])
    return boundary <= ix < cs["cam"].width - boundary and boundary <= iy < cs["cam"].height - boundary


def grid(cs):
    g = cs["cell_size"]
    cols, rows = -(-cs["cam"].width // g), -(-cs["cam"].height // g)
    return cols, rows, cols * rows


def cell_of(cs, px):
    g = cs["cell_size"]
    return int(px[1] / g) * grid(cs)[0] + int(px[0] / g)


def close_keyframes(cs, key=None):
    """[(keyframe, distance)] of Map::getCloseKeyframes in map order, and the same after the stable sort by distance"""
    key = cs["kf_key_point"] if key is None else key
    close = []
    for k in range(cs["n_kf"]):
        for p in key[k]:
            if p < 0:
                continue
            q, px = project_cur(cs, p)
            if not q[2] < 0.0 and px[0] >= 0.0 and px[1] >= 0.0 and px[0] < cs["cam"].width and px[1] < cs["cam"].height:
                d = cs["T_cur_w"][:3] - cs["T_kf_w"][k][:3]
                close.append((k, float(np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))))
                break
    return close, sorted(close, key=lambda e: e[1])


def plan(cs, state=None, key=None, max_n_kfs=None, selection=None):
    """what trk_plan_body decides: the selected keyframes, the items kept in arrival order (point, pixel, cell), the candidates out
    of the frame, the counts per selected keyframe.  selection: the keyframes to project, in that order, instead of the rule's
    (for wrong stand-ins)"""
    state = fresh_state(cs) if state is None else state
    m = cs["cfg"]["reproj_max_n_kfs"] if max_n_kfs is None else max_n_kfs
    close, ranked = close_keyframes(cs, key)
    sel = [k for k, _ in ranked[:m]] if selection is None else list(selection)
    items, overlap, seen = [], [], set()
    for k in sel:
        n = 0
        for j in range(cs["kf_ftr_offset"][k], cs["kf_ftr_offset"][k + 1]):
            p = int(cs["kf_ftr_point"][j])
            if p < 0 or state["unlinked"][p] or p in seen:
                continue
            seen.add(p)
            _, px = project_cur(cs, p)
            if in_frame(cs, px):
                items.append((p, px, cell_of(cs, px)))
                n += 1
        overlap.append(n)
    out = []
    for p in cs["cand_point"]:
        p = int(p)
        if p < 0 or state["unlinked"][p]:
            continue
        _, px = project_cur(cs, p)
        if in_frame(cs, px):
            items.append((p, px, cell_of(cs, px)))
        else:
            out.append(p)
    cols, rows, n_cells = grid(cs)
    per_cell = np.bincount(np.array([c for _, _, c in items], np.int64), minlength=n_cells) if items else np.zeros(n_cells, np.int64)
    return dict(close=close, ranked=ranked, selected=sel, overlap_count=overlap, items=items, out_candidates=out, n_kept=len(items),
                n_cells=n_cells, per_cell=per_cell)


def n_kept_of_result(cs, res):
    """the number of items the oracle kept, from its outputs: the selected keyframes' counts plus the candidates that did not
    take the three failures of a candidate out of the frame (a candidate in the frame is tried once at most)"""
    cand = cs["cand_point"][cs["cand_point"] >= 0]
    d = np.asarray(res["n_failed"])[cand] - cs["pt_n_failed"][cand]
    return int(np.sum(res["overlap_count"])) + int((d != 3).sum())


def close_view_obs(cs, p):
    """Point::getCloseViewObs in numpy: (observation, whether it is within 60 degrees)"""
    pos = cs["pt_pos"][p]

    def unit(v):
        n2 = float(v @ v)
        return v / math.sqrt(n2) if n2 > 0 else v
    od = unit(synth.se3_inv(cs["T_cur_w"])[:3] - pos)
    best, best_cos = int(cs["pt_obs_offset"][p]), 0.0
    for o in range(cs["pt_obs_offset"][p], cs["pt_obs_offset"][p + 1]):
        c = float(od @ unit(synth.se3_inv(cs["T_kf_w"][cs["obs_kf"][o]])[:3] - pos))
        if c > best_cos:
            best, best_cos = o, c
    return best, not best_cos < 0.5


_match_cache = {}


def match_alone(cs, p, px):
    """would point p, tried on its own, match: (ok, pixel, level, observation).  The oracle's findMatchDirect on the observation
    the numpy close_view_obs picks; used by replay() only"""
    from oracle import orc
    key = (cs["name"], int(p))
    if key not in _match_cache:
        if cs["pt_obs_offset"][p + 1] == cs["pt_obs_offset"][p]:
            _match_cache[key] = (False, None, 0, -1)
        else:
            o, ok = close_view_obs(cs, p)
            res = (False, None, 0, o)
            if ok:
                k = int(cs["obs_kf"][o])
                good, pc, sl = orc.find_match_direct(cs["cam"], cs["kf_pyr"][k], cs["cur_pyr"], cs["T_kf_w"][k], cs["T_cur_w"], cs["obs_px"][o],
                                                     cs["obs_f"][o], int(cs["obs_level"][o]), cs["pt_pos"][p], px, edgelet=bool(cs["obs_edgelet"][o]),
                                                     grad=tuple(cs["obs_grad"][o]))
                res = (bool(good), np.array(pc), int(sl), o)
            _match_cache[key] = res
    return _match_cache[key]


def replay(cs, res_oracle=None, state=None, order="type_seq", cut="gt", selection=None, max_fts=None):
    """The cell loop restated in numpy over plan(): per cell the candidates in trial order, the first success wins, the loop
    stops after the cell that takes n_matches beyond max_fts.  The default arguments restate the reference's rules; the others build
    wrong stand-ins: order="index" tries a cell's candidates by point index, cut="ge" stops once n_matches >= max_fts,
    selection=[...] projects those keyframes instead of the ones the distance rule selects.  Gradients of edgelet features
    are looked up in res_oracle (same point), else left at (1, 0)."""
    state = {k: v.copy() for k, v in (fresh_state(cs) if state is None else state).items()}
    max_fts = cs["cfg"]["max_fts"] if max_fts is None else max_fts
    pl = plan(cs, state, selection=selection)
    for p in pl["out_candidates"]:
        state["pt_n_failed"][p] += 3
        if state["pt_n_failed"][p] > 30:
            state["pt_type"][p] = TYPE_DELETED; state["unlinked"][p] = 1
    grad_of = {}
    if res_oracle is not None:
        grad_of = {int(p): (int(t), g) for p, t, g in zip(res_oracle["feat_point"], res_oracle["feat_type"], res_oracle["feat_grad"])}
    n_matches = n_trials = 0
    feat_point, feat_px, feat_level, feat_type, feat_grad = [], [], [], [], []
    by_cell = {}
    for seq, (p, px, c) in enumerate(pl["items"]):
        by_cell.setdefault(c, []).append((seq, p, px))
    for c in range(pl["n_cells"]):
        if cut == "ge" and n_matches >= max_fts:
            break
        cell = by_cell.get(c, [])
        if order == "index":
            cell = sorted(cell, key=lambda e: e[1])
        else:
            cell = sorted(cell, key=lambda e: (-int(state["pt_type"][e[1]]), e[0]))
        found = False
        for seq, p, px in cell:
            n_trials += 1
            if state["pt_type"][p] == TYPE_DELETED:
                continue
            ok, pc, sl, o = match_alone(cs, p, px)
            if not ok:
                state["pt_n_failed"][p] += 1
                if (state["pt_type"][p] == TYPE_UNKNOWN and state["pt_n_failed"][p] > 15) or \
                        (state["pt_type"][p] == TYPE_CANDIDATE and state["pt_n_failed"][p] > 30):
                    state["pt_type"][p] = TYPE_DELETED; state["unlinked"][p] = 1
                continue
            state["pt_n_succeeded"][p] += 1
            if state["pt_type"][p] == TYPE_UNKNOWN and state["pt_n_succeeded"][p] > 10:
                state["pt_type"][p] = TYPE_GOOD
            feat_point.append(p); feat_px.append(pc); feat_level.append(sl)
            t, g = grad_of.get(int(p), (int(cs["obs_edgelet"][o]), np.array([1.0, 0.0])))
            feat_type.append(t); feat_grad.append(g)
            found = True
            break
        if found:
            n_matches += 1
        if cut == "gt" and n_matches > max_fts:
            break
    return {"type": state["pt_type"], "n_failed": state["pt_n_failed"], "n_succeeded": state["pt_n_succeeded"], "unlinked": state["unlinked"],
            "overlap_kf": np.array(pl["selected"], np.int32), "overlap_count": np.array(pl["overlap_count"], np.int32),
            "feat_point": np.array(feat_point, np.int32), "feat_px": np.array(feat_px, dtype=np.float64).reshape(-1, 2),
            "feat_level": np.array(feat_level, np.int32), "feat_type": np.array(feat_type, np.int32),
            "feat_grad": np.array(feat_grad, dtype=np.float64).reshape(-1, 2), "n_matches": n_matches, "n_trials": n_trials}


# ---- the fixture of the reference's own outputs -----------------------------------------------------------------------------
RESULT_KEYS = ("type", "n_failed", "n_succeeded", "unlinked", "overlap_kf", "overlap_count", "feat_point", "feat_px", "feat_level", "feat_type",
               "feat_grad")


def input_crc(cs):
    """CRCs over the inputs of a case: the fixture holds results only, and these tell when the family code no longer makes the
    inputs they were recorded on"""
    crc = lambda a: zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF
    kf_images = np.concatenate([pyr[0].ravel() for pyr in {id(pyr): pyr for pyr in cs["kf_pyr"]}.values()])
    return [crc(cs["cur_pyr"][0]), crc(kf_images), crc(cs["obs_px"]), crc(cs["pt_pos"]), crc(cs["kf_ftr_obs"]), crc(cs["kf_key_point"]),
            crc(cs["T_kf_w"]), crc(np.concatenate([cs["pt_type"], cs["pt_n_failed"], cs["pt_n_succeeded"], cs["obs_kf"], cs["cand_point"]])),
            crc(np.concatenate([cs["obs_grad"].ravel(), cs["obs_edgelet"].astype(np.float64)]))]


# ---- family: cells ------------------------------------------------------------------------------------------------------
CELL_SIZES = (("lds_2048", 128, 64, 2), ("global_2112", 132, 64, 2), ("cut_54x40", 160, 119, 3))


def _reachable(cam, g, col, row):
    """can the cell hold an item: some pixel of it has integer parts within the frame's 8 px margin"""
    x0, x1 = col * g, min((col + 1) * g, cam.width) - 1
    y0, y1 = row * g, min((row + 1) * g, cam.height) - 1
    return x1 >= 8 and x0 < cam.width - 8 and y1 >= 8 and y0 < cam.height - 8


def cells():
    """Grids of exactly 2048 cells (the last size with the counters in LDS), of 2112 (the next one a 2 px grid reaches: counters in
    global memory) and of 54 x 40 with a cut last column and row.  Matching points in the first and the last cell that can
    hold one, in the cells next to index 1024 on both sides (index 1024 itself where it can hold an item) and in every seventh
    cell and its neighbour in between; failing points share some of those cells and fill others."""
    out = []
    for tag, w, h, g in CELL_SIZES:
        rng = np.random.default_rng(700 + w + g)
        cam = camera(w, h)
        img = texture(rng, h, w)
        dull = bland(h, w)
        b = MapBuilder("cells_" + tag, cam, g, img, [(IDENTITY, img), (pose(0.125), dull)])
        cols, rows = -(-w // g), -(-h // g)
        reach = [r * cols + c for r in range(rows) for c in range(cols) if _reachable(cam, g, c, r)]
        below = max(i for i in reach if i < 1024)
        above = min(i for i in reach if i >= 1024)
        chosen = {reach[0]: "first", reach[-1]: "last", below: "below_1024", above: "from_1024"}
        for i in reach:
            if i % 7 == 0 or (i - 1) % 7 == 0:
                chosen.setdefault(i, None)
        for n, i in enumerate(sorted(chosen)):
            c, r = i % cols, i // cols
            u, v = max(c * g, 8) + 0.5, max(r * g, 8) + 0.25          # inside the cell, and inside the frame
            assert int(u / g) == c and int(v / g) == r
            if n % 3 == 1:                                             # a failing point of higher type first
                b.point(b.at(u, v), TYPE_GOOD, [1], n_failed=3)
            b.point(b.at(u, v), TYPE_UNKNOWN if n % 2 else TYPE_GOOD, [0], n_succeeded=5, tag=chosen[i] and "cell_" + chosen[i])
        for n, i in enumerate(reach):
            if i % 11 == 3 and i not in chosen:                        # cells whose only candidate fails
                c, r = i % cols, i // cols
                b.point(b.at(max(c * g, 8) + 0.75, max(r * g, 8) + 0.5), TYPE_UNKNOWN, [1], n_failed=n % 20)
        if g == 3:                                                     # a pixel on an edge of the 3 px grid and the last double below it
            b.point(b.at(51.0, 90.25), TYPE_GOOD, [0], tag="edge3_on")                       # (cells that hold nothing else)
            b.point(b.at(float(np.nextafter(51.0, 0.0)), 93.25), TYPE_GOOD, [0], tag="edge3_below")
        cs = b.case()
        cs["tags"].update(index_below=below, index_above=above, index_first=reach[0], index_last=reach[-1])
        out.append(cs)
    return out


# ---- family: items ------------------------------------------------------------------------------------------------------
ITEM_COUNTS = (2047, 2048, 2049, 2600)


def _items_case(n_target):
    w, h, g = 160, 120, 20
    rng = np.random.default_rng(811)                                   # one stream for every count: a smaller map holds the first points of a larger one
    cam = camera(w, h)
    img = texture(rng, h, w)
    dull = bland(h, w)
    T1, T2 = pose(0.125), pose(0.0, -0.125)
    b = MapBuilder("items_%d" % n_target, cam, g, img, [(IDENTITY, img), (T1, dull), (T2, rolled(img, T2)), (pose(8.0), dull)])
    kf_sets = ([0], [1], [2], [1, 0], [2, 1, 0], [2, 1], [1], [3], [3, 1])
    n_in = 0
    while n_in < n_target:
        crowded = rng.uniform() < 0.12
        if crowded:                                                    # one cell takes far more than 64 items
            u, v = 60.0 + rng.integers(0, 80) / 4.0, 40.0 + rng.integers(0, 80) / 4.0
        else:
            u, v = 8.0 + rng.integers(0, (w - 16) * 4) / 4.0, 8.0 + rng.integers(0, (h - 16) * 4) / 4.0
        outside = rng.uniform() < 0.04
        if outside:
            u = float(rng.choice([3.5, 7.75, w - 8.0, w - 2.25]))
        kind = int(rng.integers(0, 10))
        nf, ns = int(rng.integers(0, 33)), int(rng.integers(7, 13))
        if kind < 2:
            b.point(b.at(u, v), TYPE_CANDIDATE, [int(rng.integers(0, 3))], n_failed=nf, candidate=True)
        else:
            ptype = (TYPE_GOOD, TYPE_GOOD, TYPE_UNKNOWN, TYPE_UNKNOWN, TYPE_UNKNOWN, TYPE_DELETED, TYPE_GOOD, TYPE_UNKNOWN)[kind - 2]
            kfs = kf_sets[int(rng.integers(0, len(kf_sets)))]
            if ptype == TYPE_GOOD and rng.uniform() < 0.9:             # most points of the type tried first fail
                kfs = ([1], [3], [3, 1], [1])[int(rng.integers(0, 4))]
            px = {3: (60.0, 30.0)}
            if kfs == [1] and rng.uniform() < 0.3:
                px[1] = (3.5, v)                                       # within 6 px of the keyframe's border: the matcher's frame test fails
            b.point(b.at(u, v), ptype, kfs, n_failed=min(nf, 20) if ptype == TYPE_UNKNOWN else nf, n_succeeded=ns, px=px)
        n_in += 0 if outside else 1
    for k in range(4):                                                # feature lists in a shuffled order, as a real keyframe's
        order = rng.permutation(len(b.fts[k]))
        b.fts[k] = [b.fts[k][j] for j in order]
    order = rng.permutation(len(b.cand))
    b.cand = [b.cand[j] for j in order]
    return b.case()


def items():
    """Maps that put exactly 2047, 2048 (the last frame with the sort keys in LDS), 2049 and 2600 items into the frame: map points of
    every type seen from one, two or three of four selected keyframes, and point candidates; a cell of more than 64 items.
    Points fail in all three ways (the bland keyframe, the matcher's frame test, no close view), so that successes and failures
    alternate in the trial order of every cell."""
    return [_items_case(n) for n in ITEM_COUNTS]


# ---- family: crowded ----------------------------------------------------------------------------------------------------
def crowded():
    """One cell of a 4 x 2 grid holds several hundred candidates of all four types from two selected keyframes (a third selected
    keyframe sees some of them again) and from the candidate list, with failing points of every type ahead of the first success;
    a second cell succeeds only among its point candidates, a third not at all."""
    w, h, g = 128, 64, 32
    rng = np.random.default_rng(905)
    cam = camera(w, h)
    img = texture(rng, h, w)
    dull = bland(h, w)
    T1, T2 = pose(0.125), pose(-0.25)
    b = MapBuilder("crowded", cam, g, img, [(IDENTITY, img), (T1, dull), (T2, rolled(img, T2)), (pose(8.0), dull)])

    def spot(cell_col):
        return cell_col * 32 + rng.integers(0, 24 * 4) / 4.0, 8.0 + rng.integers(0, 24 * 4) / 4.0
    # cell 1: the crowd.  GOOD points all fail; UNKNOWN ones fail for a while, then succeed
    for n in range(330):
        u, v = spot(1)
        r = rng.uniform()
        if n == 17:
            b.hole(0)
        if r < 0.25:
            px = {3: (60.0, 30.0)}
            if n % 5 == 0:
                px[1] = (3.5, v)                   # the matcher's frame test fails
            b.point(b.at(u, v), TYPE_GOOD, [3] if n % 7 == 0 else [1], n_failed=int(rng.integers(0, 45)), px=px)
        elif r < 0.55:
            fails = n < 250 or rng.uniform() < 0.5
            # keyframe 0 comes first in the distance order: only an observation THERE that fails is tried ahead of its successes
            px = {0: (3.5, v)} if fails and n % 2 else None
            if px:
                kfs = [2, 1, 0] if n % 4 == 1 else [0]
            elif fails:
                kfs = [1]
            else:
                kfs = ([2, 1, 0], [0], [1, 0], [2])[n % 4]
            b.point(b.at(u, v), TYPE_UNKNOWN, kfs, n_failed=int(rng.integers(12, 17)), n_succeeded=int(rng.integers(8, 12)), px=px)
        elif r < 0.8:
            b.point(b.at(u, v), TYPE_CANDIDATE, [int(rng.integers(0, 2))], n_failed=int(rng.integers(20, 32)), candidate=True)
        else:
            b.point(b.at(u, v), TYPE_DELETED, [0, 1][: 1 + n % 2], n_failed=int(rng.integers(0, 40)))
    # cell 2: every map point fails, the first success is a point candidate; deleted points in between
    for n in range(40):
        u, v = spot(2)
        if n % 4 == 0:
            b.point(b.at(u, v), TYPE_DELETED, [0])
        elif n % 4 == 1:
            b.point(b.at(u, v), TYPE_GOOD if n % 8 == 1 else TYPE_UNKNOWN, [1], n_failed=int(rng.integers(0, 14)))
        else:
            b.point(b.at(u, v), TYPE_CANDIDATE, [1 if n < 24 else 0], n_failed=int(rng.integers(0, 29)), candidate=True)
    # cell 3: nothing succeeds -- every candidate is tried, the deleted ones are counted as trials
    for n in range(24):
        u, v = spot(3)
        b.point(b.at(u, v), (TYPE_GOOD, TYPE_UNKNOWN, TYPE_DELETED)[n % 3], [1], n_failed=int(rng.integers(0, 15)))
    # cell 0 (and 4): an edgelet observation that succeeds -- the new feature's gradient goes through the warp
    b.point(b.at(28.5, 20.25), TYPE_GOOD, [0, 2], tag="edgelet", edgelet={0: (0.6, 0.8), 2: (0.8, -0.6)})
    b.point(b.at(28.5, 40.25), TYPE_GOOD, [2], tag="edgelet_kf2", edgelet={2: (0.8, -0.6)})
    for k in range(4):
        order = rng.permutation(len(b.fts[k]))
        b.fts[k] = [b.fts[k][j] for j in order]
    return [b.case()]


# ---- family: kf_selection -----------------------------------------------------------------------------------------------
KF_COUNTS = (1, 16, 17, 256)
KF_LIMITS = (1, 10, 16)
N_TRUE_IMAGES = 24        # keyframes up to this distance rank see the rolled plane, the others share the bland image


def _kf_case(n_kf, m):
    """n_kf keyframes under reproj_max_n_kfs = m.  The keyframes are laid out by distance rank and given map indices in a
    scrambled order.  Ranks (m-1, m) are a mirrored pair (+d and -d along x: exactly equal distances) whenever more than m
    keyframes are close, ranks (1, 2) another when they lie inside the selection apart from the first pair.  Where the counts
    allow, three keyframes of low rank are not close at all (no key point; every key point behind the camera; a key point at
    px == width) and one is close through a key point at px == 0.0 alone."""
    w, h, g = 128, 64, 8
    rng = np.random.default_rng(1000 + 17 * n_kf + m)
    cam = camera(w, h)
    img = texture(rng, h, w)
    dull = bland(h, w)
    specials = n_kf >= 16 and (n_kf - 3 >= m + 1 or n_kf <= m)
    n_close = n_kf - (3 if specials else 0)
    # distance by rank among the CLOSE keyframes: rank r sits r/64 (one pixel of shift) away, beyond N_TRUE_IMAGES a little further each
    tied = []
    if n_close > m:
        tied.append((m - 1, m))
    if n_close >= 3 and (not tied or m - 1 >= 3):
        tied.append((1, 2))
    dist = [r / 64.0 if r < N_TRUE_IMAGES else N_TRUE_IMAGES / 64.0 + (r - N_TRUE_IMAGES) / 1024.0 for r in range(n_close)]
    sign = [1.0 if r % 2 else -1.0 for r in range(n_close)]
    for a, c in tied:
        dist[a] = dist[c]
        sign[a], sign[c] = -1.0, 1.0
    roles = ["close"] * n_close
    if specials:                                   # low ranks: taken for close, they would be selected
        for j, role in enumerate(("no_key", "behind", "px_width")):
            at = min(3 + j, len(roles))
            roles.insert(at, role); dist.insert(at, (3 + j) / 64.0 + 1.0 / 256.0); sign.insert(at, 1.0)
    index = list(rng.permutation(n_kf))            # rank position -> keyframe index
    # a tied pair must be told apart by the index alone: the keyframe at +d gets the lower index, whatever the permutation gave
    close_pos = [j for j, role in enumerate(roles) if role == "close"]
    for a, c in tied:
        ja, jc = close_pos[a], close_pos[c]
        if index[ja] < index[jc]:
            index[ja], index[jc] = index[jc], index[ja]      # -d (laid out first) takes the higher index: +d has to come first
    kfs = [None] * n_kf
    for j in range(n_kf):
        T = pose(sign[j] * dist[j])
        true_img = dist[j] * 64.0 == int(dist[j] * 64.0) and dist[j] * 64.0 < N_TRUE_IMAGES
        kfs[index[j]] = (T, (img if dist[j] == 0 else rolled(img, T)) if true_img else dull)
    b = MapBuilder("kf_n%d_m%d" % (n_kf, m), cam, g, img, kfs, reproj_max_n_kfs=m)
    # the point the 40 nearest keyframes see (projected once, counted for the first selected keyframe only)
    sees_shared = sorted((index[j] for j in range(min(n_kf, 40)) if roles[j] != "no_key"), reverse=True)
    shared = b.point(b.at(64.5, 36.25), TYPE_GOOD, sees_shared, tag="shared")
    rank_close = 0
    for j in range(n_kf):
        k = index[j]
        u, v = 36.0 + 8.0 * (j % 7) + 3.5, 12.0 + 8.0 * ((j // 7) % 5) + 3.25
        own = b.point(b.at(u, v), TYPE_UNKNOWN if j % 2 else TYPE_GOOD, [k], n_succeeded=9 + j % 3)
        if roles[j] == "no_key":
            b.key[k] = [-1] * 5
        elif roles[j] == "behind":
            p1 = b.point(np.array([0.25, 0.0, -2.0]), TYPE_GOOD, [k], px={k: (70.0, 30.0)})
            p2 = b.point(np.array([-0.5, 0.25, -0.5]), TYPE_GOOD, [k], px={k: (40.0, 30.0)})
            b.key[k] = [p1, p2, -1, -1, -1]
        elif roles[j] == "px_width":
            b.key[k] = [b.point(b.at(float(w), 32.0), TYPE_GOOD, [k], px={k: (100.0, 30.0)}, tag="key_px_width"), -1, -1, -1, -1]
        else:
            if rank_close == 3 and n_close > 4:                          # close through px == 0.0 alone
                b.key[k] = [-1, b.point(b.at(0.0, 0.0), TYPE_GOOD, [k], px={k: (20.0, 20.0)}, tag="key_px_0"), -1, -1, -1]
            elif k in sees_shared and j % 2 == 0:
                b.key[k] = [-1, -1, shared, -1, -1]
            else:
                b.key[k] = [own, -1, -1, -1, -1]
            rank_close += 1
    cs = b.case()
    close_index = [index[j] for j in close_pos]
    # tied: (the keyframe that has to come first = the lower index, the other one), tied_ranks: the ranks they share
    cs["tags"].update(tied=[(int(close_index[c]), int(close_index[a])) for a, c in tied], tied_ranks=tied, n_close=n_close,
                      not_close=[int(index[j]) for j, role in enumerate(roles) if role != "close"],
                      kf_px_0=int(close_index[3]) if n_close > 4 else -1)
    return cs


def kf_selection():
    return [_kf_case(n, m) for n in KF_COUNTS for m in KF_LIMITS]


# ---- family: boundaries -------------------------------------------------------------------------------------------------
def _largest_below(b, bound, axis):
    """the coordinate u, as large as possible, whose projection at the identity is still below `bound`, and that projection"""
    c = b.cam.cx if axis == 0 else b.cam.cy

    def proj(u):
        return F * (((u - c) / F * DEPTH) / DEPTH) + c
    u = float(bound)
    while not proj(u) < bound:
        u = float(np.nextafter(u, -np.inf))
    return u, proj(u)


def boundaries():
    """One point per side of every comparison of the two kernels: the frame test at 8 and at width - 8 / height - 8, a cell edge,
    z == 0, a point behind the camera, and the counters one step before and at their thresholds.  Every point has a cell of
    the 8 px grid to itself unless said otherwise; map points and candidates alike."""
    w, h, g = 128, 64, 8
    rng = np.random.default_rng(1203)
    cam = camera(w, h)
    img = texture(rng, h, w)
    dull = bland(h, w)
    b = MapBuilder("boundaries", cam, g, img, [(IDENTITY, img), (pose(0.125), dull), (pose(8.0), dull)], quality_min_fts=N_CUT_MATCHES)
    b.tags["expect_in"] = {}
    for axis, size in ((0, w), (1, h)):
        lo_u, lo_px = _largest_below(b, 8.0, axis)
        hi_u, hi_px = _largest_below(b, size - 8.0, axis)
        # the last double below width - 8 is reached exactly; below 8 the projection's own rounding leaves 8 - 7e-15
        assert hi_px == np.nextafter(size - 8.0, 0.0) and lo_px < 8.0 and 8.0 - lo_px < 1e-13
        for tag, u, inside in (("at_8", 8.0, True), ("below_8", lo_u, False), ("at_max", size - 8.0, False), ("below_max", hi_u, True)):
            for kind in ("map", "cand"):
                # x boundaries: map points in the grid's row 1, candidates in row 2; y boundaries: columns 3 and 4
                across = (12.5 if kind == "map" else 20.5) if axis == 0 else (28.5 if kind == "map" else 36.5)
                uv = (u, across) if axis == 0 else (across, u)
                name = "%s_%s_%s" % ("xy"[axis], tag, kind)
                if kind == "map":
                    b.point(b.at(*uv), TYPE_GOOD, [0], tag=name)
                else:
                    b.point(b.at(*uv), TYPE_CANDIDATE, [0], n_failed=5, candidate=True, tag=name)
                b.tags["expect_in"][name] = inside
    # a cell edge and the last double below it, on both axes
    b.point(b.at(48.0, 28.5), TYPE_GOOD, [0], tag="cell_edge_x_on")
    b.point(b.at(float(np.nextafter(48.0, 0.0)), 28.25), TYPE_GOOD, [0], tag="cell_edge_x_below")
    b.point(b.at(100.5, 40.0), TYPE_GOOD, [0], tag="cell_edge_y_on")
    b.point(b.at(100.25, float(np.nextafter(40.0, 0.0))), TYPE_GOOD, [0], tag="cell_edge_y_below")
    # z == 0: an infinite and an undefined pixel, as map points and as candidates
    b.point(np.array([0.5, 0.25, 0.0]), TYPE_GOOD, [0], tag="z0_inf_map", px={0: (60.0, 30.0)})
    b.point(np.array([0.0, 0.0, 0.0]), TYPE_GOOD, [0], tag="z0_nan_map", px={0: (61.0, 30.0)})
    b.point(np.array([-0.5, 0.25, 0.0]), TYPE_CANDIDATE, [0], n_failed=4, candidate=True, tag="z0_inf_cand", px={0: (62.0, 30.0)})
    b.point(np.array([0.0, 0.0, 0.0]), TYPE_CANDIDATE, [0], n_failed=6, candidate=True, tag="z0_nan_cand", px={0: (63.0, 30.0)})
    # behind the camera, projected into the frame: the reference tests no depth there
    q = b.at(76.5, 44.25)
    b.point(-q, TYPE_GOOD, [0], tag="behind_map", px={0: (76.5, 44.25)})
    q = b.at(84.5, 44.25)
    b.point(-q, TYPE_CANDIDATE, [0], n_failed=2, candidate=True, tag="behind_cand", px={0: (84.5, 44.25)})
    # candidates out of the frame: 27 + 3 stays, 28 + 3 is deleted
    b.point(b.at(3.5, 30.0), TYPE_CANDIDATE, [0], n_failed=27, candidate=True, tag="out_27")
    b.point(b.at(3.5, 31.0), TYPE_CANDIDATE, [0], n_failed=28, candidate=True, tag="out_28")
    # the cell loop's counters: failing points (their only view is the bland keyframe), one to a cell
    slots = iter([(44.5 + 8.0 * i, 52.25) for i in range(9)])
    for tag, ptype, nf in (("unknown_14", TYPE_UNKNOWN, 14), ("unknown_15", TYPE_UNKNOWN, 15), ("good_40", TYPE_GOOD, 40)):
        b.point(b.at(*next(slots)), ptype, [1], n_failed=nf, tag=tag)
    for tag, nf in (("cand_29", 29), ("cand_30", 30)):
        b.point(b.at(*next(slots)), TYPE_CANDIDATE, [1], n_failed=nf, candidate=True, tag=tag)
    for tag, ns in (("succeeded_9", 9), ("succeeded_10", 10)):
        b.point(b.at(*next(slots)), TYPE_UNKNOWN, [0], n_succeeded=ns, tag=tag)
    # a point whose only view is more than 60 degrees away fails without a search
    # (keyframe 2 stands 8 m to the side: 76 degrees)
    b.point(b.at(68.5, 20.25), TYPE_UNKNOWN, [2], n_failed=15, tag="no_close_view", px={2: (60.0, 30.0)})
    return [b.case()]


# ---- family: cut --------------------------------------------------------------------------------------------------------
N_CUT_MATCHES = 12


def _cut_case(name, **cfg):
    w, h, g = 128, 64, 8
    rng = np.random.default_rng(1301)
    cam = camera(w, h)
    img = texture(rng, h, w)
    dull = bland(h, w)
    b = MapBuilder(name, cam, g, img, [(IDENTITY, img), (pose(0.125), dull)], **cfg)
    for n in range(N_CUT_MATCHES):
        u, v = 12.5 + 8.0 * (n % 6) * 2, 12.25 + 8.0 * (n // 6) * 2
        if n % 4 == 2:
            b.point(b.at(u + 1.0, v), TYPE_GOOD, [1], n_failed=n)                  # fails ahead of the cell's match
        b.point(b.at(u, v), TYPE_GOOD if n % 2 else TYPE_UNKNOWN, [0], n_succeeded=10, tag="match_%d" % n)
        b.point(b.at(u + 8.0, v), TYPE_UNKNOWN, [1], n_failed=n)                   # the next cell: fails
    for n in range(6):                                                              # cells behind the last match: failures only
        b.point(b.at(20.5 + 8.0 * n, 52.25), TYPE_UNKNOWN, [1], n_failed=15, tag="after_%d" % n)
    return b.case()


def cut():
    """Twelve cells with a match, failing candidates between and behind them (the latter at the deletion threshold, so that a
    loop that goes on changes the map): max_fts 0, max_fts = matches - 1 (the cut falls in the last matching cell: the cells behind
    it stay untried), no cut; quality_min_fts equal to the number of matches (the refinement runs) and one above (it does not)."""
    n = N_CUT_MATCHES
    return [_cut_case("cut_max_fts_0", max_fts=0),
            _cut_case("cut_in_last_match", max_fts=n - 1, quality_min_fts=n),
            _cut_case("cut_none", max_fts=1200, quality_min_fts=n),
            _cut_case("cut_quality_above", max_fts=1200, quality_min_fts=n + 1)]


FAMILIES = {"cells": cells, "items": items, "crowded": crowded, "kf_selection": kf_selection, "boundaries": boundaries, "cut": cut}

_cache = {}


def family(name):
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def all_cases():
    return [cs for name in FAMILIES for cs in family(name)]


def case_named(name):
    return [cs for cs in all_cases() if cs["name"] == name][0]


_oracle_cache = {}


def oracle_result(cs):
    """orc.reproject_map on a fresh state of the case (computed once per case and shared: do not modify)"""
    from oracle import orc
    if cs["name"] not in _oracle_cache:
        _oracle_cache[cs["name"]] = orc.reproject_map(cs, cs["kf_key_point"], max_fts=cs["cfg"]["max_fts"], max_n_kfs=cs["cfg"]["reproj_max_n_kfs"])
    return _oracle_cache[cs["name"]]
