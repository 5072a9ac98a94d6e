"""bench.py's options and its --dump-outputs writer on the host (the GPU run of both: tests/test_gpu_bench_ranks.py)."""
import numpy as np

import bench
from android_svo_amd import hip


def test_plain_run_is_the_default_and_full_is_opt_in(monkeypatch):
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse_args()
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs is None
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse_args()
    assert a.full is True and a.dump_outputs == "out"


def test_dump_outputs_writes_every_result_field_as_float64(tmp_path):
    rs = (hip.CSiaResult * 3)()
    for i, r in enumerate(rs):
        r.T_cur_w[:] = [0.5 * i + k for k in range(7)]
        r.n_tracked = 1000 + i
        r.H[:] = [i * 36 + k + 0.25 for k in range(36)]
        r.chi2 = 1.0 / (i + 3)
        r.stop = i
        r.iters[:] = [i + k for k in range(hip.MAX_LEVELS)]
        r.n_precompute_patches = 2 ** 40 + i
        r.n_residual_patches = 7 * i
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), list(rs))
    names = [n for n, _ in hip.CSiaResult._fields_]
    assert sorted(f.name for f in out.iterdir()) == sorted(n + ".npy" for n in names)
    got = {n: np.load(out / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 and len(a) == 3 for a in got.values())
    assert got["T_cur_w"].shape == (3, 7) and got["H"].shape == (3, 36) and got["iters"].shape == (3, hip.MAX_LEVELS)
    for i, r in enumerate(rs):
        assert list(got["T_cur_w"][i]) == list(r.T_cur_w) and list(got["H"][i]) == list(r.H)
        assert got["chi2"][i] == r.chi2 and got["stop"][i] == r.stop and list(got["iters"][i]) == list(r.iters)
        assert got["n_tracked"][i] == r.n_tracked and got["n_precompute_patches"][i] == r.n_precompute_patches
        assert got["n_residual_patches"][i] == r.n_residual_patches
