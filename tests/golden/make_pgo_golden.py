"""Writes tests/golden/pgo_f64_small.npz: the float64 outputs of tests/pgo_numpy.py (linearize and optimize) on one small
Sim3 pose graph, so that later changes to the reference (its extended-precision path) can be checked not to move a bit of
the float64 path the GPU tests compare against.  Run from the repo root:  python tests/golden/make_pgo_golden.py
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import pgo_numpy as pn  # noqa: E402
from orb_slam3_study_kr_amd import synth_pgo as sp  # noqa: E402

OUT = Path(__file__).resolve().parent / "pgo_f64_small.npz"


def main():
    m = sp.make_map(14, seed=11, mono=True, earlier_loop=True)
    g, _, _ = sp.pack_loop(m)
    fix_scale = np.zeros(len(g.fixed), dtype=bool)
    fix_scale[1::3] = True    # mixed per-vertex _fix_scale
    G = pn.PgoGraph(g.estimate, g.fixed, fix_scale, g.edge_ij, g.measurement)
    chi2, H, b = pn.linearize(G, G.estimate)
    sol = pn.optimize(G)
    np.savez_compressed(OUT, estimate=G.estimate, fixed=G.fixed, fix_scale=G.fix_scale, edge_ij=G.edge_ij, measurement=G.measurement,
                        chi2=np.float64(chi2), H=H, b=b, opt_estimate=sol.estimate, opt_iterations=sol.iterations, opt_trials=sol.trials,
                        opt_chi2_initial=sol.chi2_initial, opt_chi2_final=sol.chi2_final)
    print(f"wrote {OUT}: n={len(G.fixed)} E={len(G.edge_ij)} it={sol.iterations} tr={sol.trials} chi2 {chi2:.6g} -> {sol.chi2_final:.6g}")


if __name__ == "__main__":
    main()
