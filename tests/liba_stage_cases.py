"""The windows and frames of the inertial stage tests, shared by their CPU side (test_liba_stage_cpu.py) and their GPU side
(test_gpu_liba_stages.py, test_gpu_posei_stages.py), with the oracle stage functions in the form liba_stage_numpy.noise_floor takes."""
import functools

import numpy as np

import liba_stage_numpy as ls
from orb_slam3_study_kr_amd import synth_inertial as si

# A run-time bound of 2 x noise_floor must not grow past these, or it could hide a wrong Jacobian block (1e-4 .. 1e-3 relative)
CAP_H = 1e-6      # J (relative to the link's largest entry) and H scaled by its diagonal
CAP_B = 5e-6      # b, W r relative to their largest entry
K_LM_TAU = 1e-5   # g2o's computeLambdaInit: tau x the largest diagonal entry of the whole Hessian

LIBA_MEASURES = dict(H=ls.scaled_h, chi2=ls.rel_scalar)
POSEI_MEASURES = dict(H=ls.scaled_h)


def _small():
    return si.make_inertial_window(21, n_opt=3, n_fixed=2, n_points=80)


def _without_links_at(w, kfs):
    from test_gpu_liba import _without_links_at as cut
    return cut(w, kfs)


_WINDOWS = {
    "small_stereo": _small,                                                                       # 235 edges, 3 links
    "no_fixed": lambda: si.make_inertial_window(24, n_opt=5, n_fixed=0, n_points=300),
    "fisheye": lambda: si.make_inertial_window(13, n_opt=3, n_fixed=2, n_points=100, fisheye=True),
    "rig": lambda: si.make_inertial_rig_window(18, n_opt=3, n_fixed=2, n_points=200),            # left + right pairs on one block
    "shared_bias": lambda: si.with_shared_bias(si.make_inertial_window(304, n_opt=4, n_fixed=6, n_points=440)),   # 4 colours, the priors
    "some_links": lambda: _without_links_at(_small(), [2]),                                       # keyframe 2 keeps no link
    "visual_only": lambda: _without_links_at(_small(), [0, 1, 2]),
    "lds_panels": lambda: si.make_inertial_window(61, n_opt=25, n_fixed=10, n_points=1500, large=True),
    # 508 / 492 / 471 edges per optimisable keyframe: each of the 8 chunks of 64 of every pose row holds edges (see chunk_occupancy)
    "eight_chunks": lambda: si.make_inertial_window(21, n_opt=3, n_fixed=2, n_points=720),
}
WINDOWS = list(_WINDOWS)


@functools.lru_cache(maxsize=None)
def window(name):
    return _WINDOWS[name]()


_FRAME_KINDS = {"stereo": {}, "mono": dict(stereo=False), "fisheye": dict(fisheye=True), "rig": dict(rig=True)}
# 60-edge frames of tests/test_oracle_posei.py; 1400 edges: the largest frame the kernel keeps in LDS (ecap 1408), 1401: global memory,
# 1344 = 21 x 64 = its own ecap
FRAMES = [f"{k}-m{m}" for m in (0, 1) for k in _FRAME_KINDS] + [f"n{n}-m{m}" for n in (1344, 1400, 1401) for m in (0, 1)]


@functools.lru_cache(maxsize=None)
def frame(name):
    kind, m = name.split("-m")
    if kind in _FRAME_KINDS:
        return si.make_posei_frame(5, mode=int(m), n_points=60, **_FRAME_KINDS[kind])
    f = si.make_posei_frame(50, mode=int(m), n_points=int(kind[1:]))
    assert f.n_edges == int(kind[1:])
    return f


def chunk_occupancy(w, C):
    """Per optimisable keyframe, how many of the C chunks of its pose row hold at least one edge (the split of liba_pose_pass: chunks
    of ceil(count / C) edges rounded up to whole wavefronts of 64)."""
    out = []
    for i in range(w.n_opt):
        cnt = int((w.edge_pose == i).sum())
        per = ((cnt + C - 1) // C + 63) // 64 * 64
        out.append(sum(1 for ch in range(C) if ch * per < cnt))
    return out


# ---- oracle stage functions as {name: array} -------------------------------------------------------------------------
def liba_system(ob):
    def fn(w):
        d = ob.liba_linearize(w)
        n = 15 * w.n_opt
        return dict(H=d["H"], b=d["b"][:n], bl=d["b"][n:], Hll=d["Hll"], Hpl=d["Hpl"], chi2=d["chi2"])
    return fn


def link_forms(ob, w, l):
    """(J [9][24], -W r [9], rho') of link l from the oracle's residual and Jacobian, the link's information and Huber's rho'."""
    r, J = ob.liba_inertial_edge(w, l)
    Om = np.asarray(w.link_info[l], np.float64).reshape(9, 9)
    chi = float(r @ Om @ r)
    rho1 = 1.0
    if w.link_robust[l] and chi > w.huber_inertial ** 2:
        rho1 = w.huber_inertial / np.sqrt(chi)
    return J, -(Om @ r), rho1, chi


def liba_links(ob):
    def fn(w):
        out = {}
        for l in range(w.n_links):
            J, Wr, rho1, _ = link_forms(ob, w, l)
            out[f"J{l}"], out[f"Wr{l}"], out[f"rho{l}"] = J, Wr, np.float64(rho1)
        return out
    return fn


def posei_system(ob):
    def fn(f):
        H, b = ob.posei_linearize(f)
        return dict(H=H, b=b)
    return fn


def default_lambda(d):
    """kLmTau x the largest diagonal entry of the oracle's full system, landmarks included."""
    dl = d["Hll"][:, [0, 1, 2], [0, 1, 2]]
    return K_LM_TAU * max(np.abs(np.diag(d["H"])).max(), np.abs(dl).max() if dl.size else 0.0)
