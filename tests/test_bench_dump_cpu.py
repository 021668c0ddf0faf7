"""bench.py --dump-outputs on CPU: the arrays written are the solver's results (every pose, a fixed sample of landmarks and
edges), float64 and finite, the same rows in every run, and under 64 MB for any batch size."""
from types import SimpleNamespace

import numpy as np

import bench
from oracle import binding as ob
from orb_slam3_study_kr_amd import synth


def _load(d):
    return {p.stem: np.load(p) for p in sorted(d.glob("*.npy"))}


def test_dump_holds_the_results_and_repeats(tmp_path):
    windows = [synth.make_window(3 + i, n_free=6, n_fixed=2, n_points=400, stereo=True) for i in range(9)]   # traces of 8 and 9 iterations: padded rows
    results = [ob.lba_solve(w) for w in windows]
    info = bench.dump_lba_outputs(tmp_path / "a", windows, results)
    bench.dump_lba_outputs(tmp_path / "b", windows, results)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert info["files"] == len(a) and a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == np.float64, k
        assert np.isfinite(a[k]).all(), k
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(a["lba_pose_qt"], np.stack([r.pose_qt for r in results]))
    np.testing.assert_array_equal(a["lba_iterations"], [r.iterations for r in results])
    np.testing.assert_array_equal(a["lba_trace_length"], [len(r.chi2_trace) for r in results])
    for i, r in enumerate(results):
        ip = a["lba_points_sample_index"][i]
        ip = ip[ip >= 0].astype(int)
        assert len(ip) == windows[i].n_points   # fewer landmarks than the sample: all of them
        np.testing.assert_array_equal(a["lba_points_sample"][i, :len(ip)], r.points[ip])
        ie = a["lba_edge_sample_index"][i]
        ie = ie[ie >= 0].astype(int)
        np.testing.assert_array_equal(a["lba_edge_chi2_sample"][i, :len(ie)], r.edge_chi2[ie])
        n_tr = len(r.chi2_trace)
        np.testing.assert_array_equal(a["lba_chi2_trace"][i, :n_tr], r.chi2_trace)
        assert not a["lba_chi2_trace"][i, n_tr:].any()   # zero past the window's trace


def test_dump_of_a_large_batch_stays_under_64_mb(tmp_path):
    n, L, E = 4096, 10000, 75000   # config-2 shaped windows, eight times bench.py's default batch
    w = SimpleNamespace(n_points=L, n_edges=E)
    r = SimpleNamespace(status=0, iterations=10, trials=10, chi2_initial=1.0, chi2_trace=np.ones(10), lambda_trace=np.ones(10),
                        trials_trace=np.ones(10), pose_qt=np.zeros((50, 7)), points=np.zeros((L, 3)), edge_chi2=np.zeros(E),
                        edge_depth_pos=np.zeros(E, dtype=np.uint8))
    info = bench.dump_lba_outputs(tmp_path, [w] * n, [r] * n)
    on_disk = sum(p.stat().st_size for p in tmp_path.glob("*.npy"))
    assert info["bytes"] <= 64 << 20 and on_disk <= 64 << 20
    assert info["points_per_window"] >= 64 and info["edges_per_window"] >= 64
