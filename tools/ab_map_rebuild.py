"""A/B of builds on the SAME box for the in-place map rebuilds (promotion, removal, renumbering) through the C++ host twin:

    python tools/ab_map_rebuild.py parent=<dir>/android_svo_amd/host/svo_host_demo tree=android_svo_amd/host/svo_host_demo

(a demo finds its library next to itself, ../csrc).  Two runs of `svo_host_demo <case> <out> track times ...` over
tracking_chain's sequence, 30 frames, every frame a keyframe:
    incremental   kf_every 1 max_kfs 10 incremental, maxFts 600: every frame from the tenth on follows a
                  promotion and a removal
    compact       tests/test_gpu_map_compaction.py::test_host_twin_compacts_points' run with `compact`: max_kfs 3, new_seeds 40,
                  max_points at what the living points need
The figure is the host-side duration of track() (times_track.bin), median over the frames from the tenth on; the builds
alternate, RUNS times each; per build the median of those medians and their spread (max - min).  Every track_*.bin the builds
write (poses, features, statistics) is compared byte for byte.  Prints one JSON line per run kind; stops at the first failure."""
import json
import os
import pathlib
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import tracking_chain as tc
from test_gpu_host_cpp import _write_track_case

N, RUNS = 30, 6
OUT = pathlib.Path(ROOT) / "build" / "ab_map_rebuild"            # (build/ is ignored by git)


def make_case(name, max_fts):
    seq = tc.make_sequence(n_frames=N + 1)
    mp = tc.sequence_map(seq)
    n = len(seq["px0"])
    cs = dict(mp, obs_point=np.arange(n, dtype=np.int32), kf_ftr_obs=np.arange(n, dtype=np.int32), cand_obs=np.zeros(0, np.int32))
    cfg = dict(grid_size=tc.CELL, max_fts=max_fts, quality_min_fts=40, klt_min_level=2, max_frame_features=1024, keyframe_at=0)
    case = OUT / name
    case.mkdir(parents=True, exist_ok=True)
    _write_track_case(case, cs, [seq["pyrs"][k][0] for k in range(1, N + 1)], cfg, last_kf=0)
    return case


def run(demo, case, tag, args):
    out = OUT / tag
    out.mkdir(exist_ok=True)
    p = subprocess.run([demo, str(case), str(out), "track"] + args, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    if p.returncode != 0:
        sys.exit("%s failed (%d): %s" % (tag, p.returncode, (p.stdout + p.stderr)[-2000:]))      # nothing more is started
    return out


def track_files(d):
    return {f: (d / f).read_bytes() for f in sorted(os.listdir(d)) if f.startswith("track_") and f.endswith(".bin")}


def main():
    demos = dict(a.split("=", 1) for a in sys.argv[1:])
    assert len(demos) >= 2, __doc__
    demos = {k: os.path.abspath(v) for k, v in demos.items()}
    case_a, case_b = make_case("case_incremental", 600), make_case("case_compact", tc.MAX_FTS)
    twin = ["incremental", "kf_every", "1", "max_kfs", "3", "new_seeds", "40"]
    roomy = run(next(iter(demos.values())), case_b, "roomy", twin)
    max_points = int(np.fromfile(roomy / "map_points_room.bin")[0])
    kinds = dict(incremental=(case_a, ["times", "kf_every", "1", "max_kfs", "10", "incremental"]),
                 compact=(case_b, ["times"] + twin + ["max_points", str(max_points), "compact"]))
    for kind, (case, args) in kinds.items():
        med = {b: [] for b in demos}
        for _ in range(RUNS):
            for b, demo in demos.items():
                t = np.fromfile(run(demo, case, kind + "_" + b, args) / "times_track.bin")
                assert len(t) == N, len(t)
                med[b].append(round(float(np.median(t[10:])), 2))
        files = [track_files(OUT / (kind + "_" + b)) for b in demos]
        res = dict(kind=kind, track_files=len(files[0]), track_files_byte_equal=all(f == files[0] for f in files[1:]))
        if kind == "compact":
            res.update(max_points=max_points, compactions=[float(np.fromfile(OUT / (kind + "_" + b) / "map_compactions.bin")[-1]) for b in demos])
        for b in demos:
            res[b] = dict(median_us=round(float(np.median(med[b])), 2), spread_us=round(max(med[b]) - min(med[b]), 2), runs_us=med[b])
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
