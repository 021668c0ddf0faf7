"""Frame::ComputeStereoMatches (reference src/Frame.cc:816-986) without a device: known answers of the numpy restatement
(tests/stereo_numpy.py), the branch census of the committed cases, the C++ restatement of the test library against the numpy one,
and the pack of the host drop-in (order, widths, strided pyramids)."""
import ctypes as C

import numpy as np
import pytest

import stereo_numpy as sn
from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_stereo as ss

F = np.float32


@pytest.fixture(scope="module")
def cases():
    out = {}
    for name, kw in sn.CASES:
        fr = ss.make_stereo_frame(**kw)
        out[name] = (fr, sn.compute_stereo_matches(fr))
    return out


def _bits(a):
    return np.asarray(a, dtype=F).view(np.uint32)


def test_whole_pixel_shift_gives_exact_answers():
    # right(x) = left(x + d), symmetric images, perfect level-0 keypoints: the SADs beside the minimum are equal, deltaR == 0
    for d in (3, 7, 21):
        fr, n = ss.make_shift_frame(11 + d, d)
        r = sn.compute_stereo_matches(fr)
        assert (r["stage"][:n] == capi.OSH_STEREO_ACCEPTED).all(), np.bincount(r["stage"][:n])
        assert (r["best_inc"][:n] == 0).all() and (r["sad"][:n, 5] == 0).all()
        assert (r["sad"][:n, 4] == r["sad"][:n, 6]).all()                       # deltaR == 0
        u_l = fr.left_xy[:n, 0]
        assert np.array_equal(_bits(r["u_right"][:n]), _bits(u_l - F(d)))
        assert np.array_equal(_bits(r["depth"][:n]), _bits(np.full(n, F(fr.bf) / F(d), F)))
        assert r["undefined"] == [0, 0, 0, 0]


def test_zero_shift_takes_the_small_disparity_branch():
    fr, n = ss.make_shift_frame(5, 0)
    r = sn.compute_stereo_matches(fr)
    assert (r["stage"][:n] == capi.OSH_STEREO_ACCEPTED).all() and ((r["flags"][:n] & 1) == 1).all()
    u_l = fr.left_xy[:n, 0]
    assert np.array_equal(_bits(r["u_right"][:n]), _bits((u_l.astype(np.float64) - 0.01).astype(F)))
    assert np.array_equal(_bits(r["depth"][:n]), _bits(np.full(n, F(fr.bf) / F(0.01), F)))


def test_constant_image_stops_every_keypoint_at_the_first_increment():
    fr, _ = ss.make_shift_frame(9, 4, constant=True)
    r = sn.compute_stereo_matches(fr)
    assert (r["stage"] == capi.OSH_STEREO_BORDER_INC).all()
    assert (r["best_inc"] == -5).all() and (r["sad"] == 0).all()
    assert (r["u_right"] == -1).all() and (r["depth"] == -1).all()


def test_round_is_half_away_from_zero():
    assert [float(sn.round_away(F(x))) for x in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 2.4999998)] == [1, 2, 3, -1, -3, 0, 2]


def test_every_branch_is_taken_on_the_committed_cases(cases):
    """Conditions on the inputs, checked on the restatement alone: a green device test cannot be an empty one."""
    st = np.concatenate([r["stage"] for _, r in cases.values()])
    fl = np.concatenate([r["flags"] for _, r in cases.values()])
    ham = np.concatenate([r["hamming"] for _, r in cases.values()])
    count = {name: int((st == getattr(capi, "OSH_STEREO_" + name)).sum()) for name in
             ("NO_CANDIDATE", "HAMMING", "RIGHT_GUARD", "BORDER_INC", "DISPARITY", "ACCEPTED", "MEDIAN_CUT")}
    print(count, "0.01 branch", int((fl & 1).sum()), "SAD ties", int((fl >> 1).sum()))
    for name, c in count.items():
        assert c >= 1, name
    assert int((fl & 1).sum()) >= 1, "0.01 branch"
    assert int((fl >> 1).sum()) >= 1, "SAD tie"
    # Hamming >= 75 both ways: a best candidate in [75, 100) and no candidate below TH_HIGH
    assert ((st == capi.OSH_STEREO_HAMMING) & (ham < 100)).any() and ((st == capi.OSH_STEREO_HAMMING) & (ham == 100)).any()
    both = np.concatenate([r["best_inc"][r["stage"] == capi.OSH_STEREO_BORDER_INC] for _, r in cases.values()])
    assert (both == -5).any() and (both == 5).any()
    assert (st != capi.OSH_STEREO_DELTA).all()           # deltaR outside [-1, 1] cannot happen


def test_margin_respecting_keypoints_meet_no_undefined_case(cases):
    for name in sn.DEFAULT_CASES + ("low_contrast", "median_band", "zero_band"):
        fr, r = cases[name]
        assert r["undefined"] == [0, 0, 0, 0], (name, r["undefined"])
        assert (r["stage"] != capi.OSH_STEREO_PATCH).all() and (r["stage"] != capi.OSH_STEREO_RIGHT_GUARD).all()
    # the extractor's margin holds on every default frame
    for name in sn.DEFAULT_CASES:
        fr, _ = cases[name]
        for xy, octv, pyr in ((fr.left_xy, fr.left_octave, fr.left_pyramid), (fr.right_xy, fr.right_octave, fr.right_pyramid)):
            lvl = xy * fr.inv_scale_factors[octv][:, None]
            shape = np.array([pyr[o].shape for o in octv]).reshape(-1, 2)
            assert (lvl >= ss.MARGIN - 0.01).all() and (lvl[:, 0] <= shape[:, 1] - ss.MARGIN).all() and (lvl[:, 1] <= shape[:, 0] - ss.MARGIN).all()


def test_median_cut_case_spreads_the_accepted_sads(cases):
    _, r = cases["median_band"]
    acc = r["stage"] >= capi.OSH_STEREO_ACCEPTED
    best = r["sad"][acc, r["best_inc"][acc] + 5]
    assert best.max() > 2.1 * np.sort(best)[best.size // 2]
    assert int((r["stage"] == capi.OSH_STEREO_MEDIAN_CUT).sum()) >= 10


@pytest.mark.parametrize("name", [n for n, _ in sn.CASES])
def test_cpp_restatement_equals_numpy_bit_for_bit(cases, name):
    fr, exp = cases[name]
    got = sn.cpp_restatement(fr)
    sn.assert_same(got, exp, sn.OUTPUTS + ("flags",), name)
    assert got["undefined"] == exp["undefined"]


def test_cpp_restatement_on_known_answers_and_odd_sizes():
    frames = [ss.make_shift_frame(3, 5)[0], ss.make_shift_frame(4, 0)[0], ss.make_shift_frame(5, 2, constant=True)[0],
              ss.make_stereo_frame(21, n_left=0), ss.make_stereo_frame(22, n_left=50, n_right=0),
              ss.make_stereo_frame(23, n_left=1, n_levels=1), ss.make_stereo_frame(24, n_left=300, n_levels=3)]
    for k, fr in enumerate(frames):
        exp = sn.compute_stereo_matches(fr)
        got = sn.cpp_restatement(fr)
        sn.assert_same(got, exp, sn.OUTPUTS + ("flags",), f"frame {k}")
        assert got["undefined"] == exp["undefined"], k


def _pack(fr, border):
    lib = capi.load_host_library()
    h, keep = sn.host_input(fr)
    n, nr, nl = h.n_left, h.n_right, h.n_levels
    o = dict(sizes=np.zeros(3, np.int32), lxy=np.zeros((n, 2), F), loct=np.zeros(n, np.int32), ldesc=np.zeros((n, 32), np.uint8),
             rxy=np.zeros((nr, 2), F), roct=np.zeros(nr, np.int32), rdesc=np.zeros((nr, 32), np.uint8), scales=np.zeros((nl, 2), F),
             shape=np.zeros((2, nl, 3), np.int64), lpix=np.zeros_like(keep["lpix"]), rpix=np.zeros_like(keep["rpix"]), bf_b=np.zeros(2, F))
    rc = lib.osh_host_pack_stereo(C.byref(h), border, capi.ptr(o["sizes"], capi.c_int32_p), capi.ptr(o["lxy"], capi.c_float_p),
                                  capi.ptr(o["loct"], capi.c_int32_p), capi.ptr(o["ldesc"], capi.c_uint8_p), capi.ptr(o["rxy"], capi.c_float_p),
                                  capi.ptr(o["roct"], capi.c_int32_p), capi.ptr(o["rdesc"], capi.c_uint8_p), capi.ptr(o["scales"], capi.c_float_p),
                                  capi.ptr(o["shape"], capi.c_int64_p), capi.ptr(o["lpix"], capi.c_uint8_p), capi.ptr(o["rpix"], capi.c_uint8_p),
                                  capi.ptr(o["bf_b"], capi.c_float_p))
    assert rc == 0, rc
    return o, keep


def test_pack_keeps_order_and_widths_and_walks_strided_pyramids():
    fr = ss.make_stereo_frame(31, n_left=200, n_levels=4)
    flat, keep = _pack(fr, 0)
    assert list(flat["sizes"]) == [200, fr.right_xy.shape[0], 4]
    assert np.array_equal(_bits(flat["lxy"]), _bits(fr.left_xy)) and np.array_equal(_bits(flat["rxy"]), _bits(fr.right_xy))
    assert np.array_equal(flat["loct"], fr.left_octave) and np.array_equal(flat["roct"], fr.right_octave)
    assert np.array_equal(flat["ldesc"], fr.left_desc) and np.array_equal(flat["rdesc"], fr.right_desc)
    assert np.array_equal(_bits(flat["scales"][:, 0]), _bits(fr.scale_factors)) and np.array_equal(_bits(flat["scales"][:, 1]), _bits(fr.inv_scale_factors))
    assert np.array_equal(_bits(flat["bf_b"]), _bits([fr.bf, fr.b]))
    assert np.array_equal(flat["lpix"], keep["lpix"]) and np.array_equal(flat["rpix"], keep["rpix"])
    for side, pyr in enumerate((fr.left_pyramid, fr.right_pyramid)):
        for l, m in enumerate(pyr):
            assert list(flat["shape"][side, l]) == [m.shape[0], m.shape[1], m.shape[1]]
    # levels stored as views into bordered images: stride > cols, the same bytes
    for border in (1, 19):
        view, _ = _pack(fr, border)
        for k in ("lxy", "loct", "ldesc", "rxy", "roct", "rdesc", "scales", "lpix", "rpix", "bf_b", "sizes"):
            assert np.array_equal(view[k], flat[k]), (border, k)
        assert np.array_equal(view["shape"][..., :2], flat["shape"][..., :2])
        assert np.array_equal(view["shape"][..., 2], flat["shape"][..., 1] + 2 * border)


def test_stereo_structs_match_the_header_layout():
    assert C.sizeof(capi.StereoImage) == 24
    assert C.sizeof(capi.StereoFrame) == 8 + 6 * 8 + 8 + 4 * 8 + 8
    assert C.sizeof(capi.StereoResult) == 7 * 8
