"""Host-side packer of osh_liba_solve and the inertial debug exports (csrc/liba_pack.h) on CPU: ``osh_liba_pack_check`` describes,
bands, lays out and packs the windows exactly as the device path does (into malloc'ed instead of pinned staging) and verifies what
k_liba relies on -- window offsets, landmark-major edge order with a rig's left + right pairs, the pose-by-pose walk order, the
(landmark, pose) -> block table, link colours, the band of a map-sized problem, the arena layout -- and refuses what the device path
refuses, with the same code and message."""
import dataclasses

import numpy as np
import pytest

import liba_stage_cases as lc
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_inertial as si

CASES = ["small_stereo", "no_fixed", "fisheye", "rig", "shared_bias", "some_links", "visual_only", "eight_chunks"]
STATS = ("edges", "free_edges", "merged", "colours", "banded", "arena_bytes", "NB", "W")


def pack_check(windows):
    lib = capi.load_library()
    arr = (capi.LibaProblem * len(windows))()
    for i, w in enumerate(windows):
        arr[i] = w.as_struct()
    st = np.zeros(8, dtype=np.int64)
    rc = lib.osh_liba_pack_check(len(windows), arr, capi.ptr(st, capi.c_int64_p))
    return rc, lib.osh_last_error().decode(), dict(zip(STATS, (int(v) for v in st)))


@pytest.mark.parametrize("name", CASES)
def test_single_windows_pack(name):
    w = lc.window(name)
    rc, msg, st = pack_check([w])
    assert rc == 0, msg
    assert st["edges"] == w.n_edges and st["free_edges"] == int((w.edge_pose < w.n_opt).sum())
    assert (st["NB"], st["banded"], st["W"]) == (24, 0, (15 * w.n_opt + 25) & ~1)
    if name == "rig":
        key = w.edge_pose.astype(np.int64) * w.n_points + w.edge_point
        assert st["merged"] == w.n_edges - len(np.unique(key)) > 0
    else:
        assert st["merged"] == 0
    if name == "shared_bias":
        assert st["colours"] == 4                       # every link shares the bias keyframe with every other
    else:
        assert st["colours"] == min(2, w.n_links)       # a chain of links takes two colours


def test_heterogeneous_batch_packs_at_running_offsets():
    ws = [lc.window(n) for n in CASES]
    rc, msg, st = pack_check(ws)
    assert rc == 0, msg
    assert st["edges"] == sum(w.n_edges for w in ws) and st["colours"] == 4 and st["merged"] > 0
    assert st["W"] == (15 * max(w.n_opt for w in ws) + 25) & ~1


def _map(n_kf):
    """The generator of test_gpu_liba_stages._banded() at n_kf keyframes."""
    return si.make_inertial_window(905, n_opt=n_kf, n_fixed=0, n_points=400, large=True, kf_dt=0.5)


def test_band_threshold(monkeypatch):
    """60 keyframes half a second apart take the banded layout; with 59 the band is no longer under half the system."""
    rc, msg, st = pack_check([_map(60)])
    assert rc == 0, msg
    assert (st["NB"], st["banded"]) == (6, 1)
    rc, msg, st = pack_check([_map(59)])
    assert rc == 0, msg
    assert (st["NB"], st["banded"]) == (6, 0)
    monkeypatch.setenv("OSH_LIBA_DENSE", "1")
    rc, msg, st = pack_check([_map(60), lc.window("small_stereo")])
    assert rc == 0, msg
    assert (st["NB"], st["banded"]) == (6, 0)


def _set(a, k, v):
    a = np.array(a).copy()
    a[k] = v
    return a


def _refused():
    w, fe, rig, sb = lc.window("small_stereo"), lc.window("fisheye"), lc.window("rig"), lc.window("shared_bias")
    NV = w.n_opt + w.n_fixed_imu
    key = rig.edge_pose.astype(np.int64) * rig.n_points + rig.edge_point
    left = set(key[rig.edge_kind == capi.OSH_EDGE_MONO].tolist())
    right = next(e for e in range(rig.n_edges) if rig.edge_kind[e] == capi.OSH_EDGE_RIGHT and int(key[e]) in left)   # the right edge of a pair
    return {
        "bad sizes": (dataclasses.replace(w, n_fixed_imu=2), capi.OSH_ERR_INVALID, "bad sizes"),
        "edge index": (dataclasses.replace(w, edge_pose=_set(w.edge_pose, 7, NV + w.n_fixed)), capi.OSH_ERR_INVALID, "edge 7: index or kind out of range"),
        "edge kind": (dataclasses.replace(w, edge_kind=_set(w.edge_kind, 5, capi.OSH_EDGE_RIGHT + 1)), capi.OSH_ERR_INVALID, "edge 5: index or kind out of range"),
        "right edge without a rig": (dataclasses.replace(fe, edge_kind=_set(fe.edge_kind, 3, capi.OSH_EDGE_RIGHT)), capi.OSH_ERR_INVALID, "needs kb8, cam2 and trl"),
        "stereo edge in a KB8 window": (dataclasses.replace(fe, edge_kind=_set(fe.edge_kind, 3, capi.OSH_EDGE_STEREO)), capi.OSH_ERR_UNSUPPORTED, "monocular edges only (edge 3)"),
        "link keyframe": (dataclasses.replace(w, link_cur=_set(w.link_cur, 1, w.n_opt)), capi.OSH_ERR_INVALID, "link 1: keyframe index out of range"),
        "bias keyframe": (dataclasses.replace(w, link_bias=_set(w.link_prev, 1, NV)), capi.OSH_ERR_INVALID, "link 1: bias keyframe out of range"),
        "bias on the later keyframe": (dataclasses.replace(w, link_bias=_set(w.link_prev, 1, w.link_cur[1])), capi.OSH_ERR_UNSUPPORTED, "cannot be those of its later keyframe"),
        "shared bias with a random walk": (dataclasses.replace(sb, link_info_g=_set(sb.link_info_g, (1, 4), 1.0)), capi.OSH_ERR_UNSUPPORTED, "link 1: a link whose bias vertices belong to another keyframe carries no random-walk edges"),
        "unpaired duplicate": (dataclasses.replace(rig, edge_kind=_set(rig.edge_kind, right, capi.OSH_EDGE_MONO)), capi.OSH_ERR_UNSUPPORTED, "do not form a left + right pair"),
        "max_iterations": (dataclasses.replace(w, max_iterations=capi.OSH_LBA_MAX_TRACE + 1), capi.OSH_ERR_INVALID, "bad sizes"),
    }


@pytest.mark.parametrize("what", ["bad sizes", "edge index", "edge kind", "right edge without a rig", "stereo edge in a KB8 window", "link keyframe", "bias keyframe",
                                  "bias on the later keyframe", "shared bias with a random walk", "unpaired duplicate", "max_iterations"])
def test_refusals(what):
    bad, code, text = _refused()[what]
    rc, msg, _ = pack_check([bad])
    assert rc == code and text in msg, (rc, msg)
    # behind a good window the message names window 1
    rc, msg, _ = pack_check([lc.window("no_fixed"), bad])
    assert rc == code and text in msg and "window 1" in msg, (rc, msg)


def test_shuffled_edges_pack_to_the_same_stats():
    w = lc.window("rig")
    perm = np.random.default_rng(4).permutation(w.n_edges)
    w2 = dataclasses.replace(w, **{k: np.ascontiguousarray(getattr(w, k)[perm]) for k in ("edge_pose", "edge_point", "edge_kind", "edge_obs", "edge_info")})
    a, b = pack_check([w]), pack_check([w2])
    assert a[0] == 0 and b[0] == 0, (a[1], b[1])
    assert a[2] == b[2] and a[2]["merged"] > 0
