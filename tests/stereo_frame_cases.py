"""What the tests of the calls that extract and match a rectified stereo frame share: the extract items of the named pairs of
synth_stereo_pair, the chain of the CPU restatements that extracts an image without a device, the level-0 scaling of the
reference's write-back (src/ORBextractor.cc:1143-1150) that turns two extract results into the frame the stereo matcher reads, and
the census every named pair must meet."""
import functools

import numpy as np

import octree_numpy as on
import pyramid_numpy as pn
from orb_slam3_study_kr_amd import capi, orb
from orb_slam3_study_kr_amd import synth_fast as sf
from orb_slam3_study_kr_amd import synth_stereo as ss
from orb_slam3_study_kr_amd import synth_stereo_pair as sp

F = np.float32
PAIR_NAMES = tuple(sp.PAIRS)


def scales(nlevels, scale_factor=1.2):
    """mvScaleFactor as the constructor forms it: a running float32 product."""
    s = [F(1)]
    for _ in range(1, nlevels):
        s.append(F(s[-1] * F(scale_factor)))
    return np.asarray(s, F)


def item(image, nlevels, nfeatures=1000, ini_th=20, min_th=7):
    """An item of OrbMatcher.extract with the stand-in extractor's tables."""
    return dict(image=np.ascontiguousarray(image, np.uint8), inv_scale=np.asarray(pn.standin_inv_scale(nlevels), F), scale=scales(nlevels),
                n_features=np.asarray(on.features_per_level(nfeatures, 1.2, nlevels), np.int32), pattern=orb.standin_pattern(), ini_th=ini_th,
                min_th=min_th, border=19)


@functools.lru_cache(maxsize=None)
def pair(name):
    """dict(left, right, bf, b) of a named pair, left / right items of extract."""
    p = sp.named_pair(name)
    return dict(left=item(p["left"], p["n_levels"], p["n_features"]), right=item(p["right"], p["n_levels"], p["n_features"]), bf=p["bf"], b=p["b"])


def custom_pair(left, right, nlevels, nfeatures, bf=40.0, b=1.0):
    return dict(left=item(left, nlevels, nfeatures), right=item(right, nlevels, nfeatures), bf=bf, b=b)


def extract_cpu(it) -> dict:
    """ORBextractor::operator() up to its write-back through the CPU restatements of the test library, chained: pyramid, detector,
    quadtree per level, minBorder added, IC_Angle, descriptors.  The keys of OrbMatcher.extract that the stereo frame needs, and
    levels."""
    built = orb.pyramid_cpu([it])[0][0]
    levels = [np.ascontiguousarray(lv) for lv in built["levels"]]
    nl = len(levels)
    det = orb.fast_cpu([sf.FastFrame(tuple(levels), it["ini_th"], it["min_th"])])[0][0]
    xy, level = [], []
    for l, lv in enumerate(levels):
        sel = det["level"] == l
        if not sel.any():
            continue
        cxy, cr = det["xy"][sel], det["response"][sel]
        res, rc, _ = orb.octree_cpu([(cxy, cr, lv.shape[1] - 32, lv.shape[0] - 32, int(it["n_features"][l]))])
        assert rc == 0 and res[0]["index"] is not None
        kept = res[0]["index"]
        xy.append(cxy[kept] + F(16))
        level.append(np.full(len(kept), l, np.int32))
    n = sum(len(v) for v in level)
    xy = np.concatenate(xy) if n else np.zeros((0, 2), F)
    level = np.concatenate(level) if n else np.zeros(0, np.int32)
    angle = orb.ic_angle_cpu([dict(xy=xy, level=level, pyramid=levels)])[0][0]["angle"] if n else np.zeros(0, F)
    desc = orb.describe_cpu([dict(xy=xy, level=level, angle=angle, pattern=it["pattern"], pyramid=levels)])[0][0]["descriptors"] if n else np.zeros((0, 32), np.uint8)
    return dict(n_out=n, xy=xy, level=level, angle=angle, descriptors=desc, levels=levels)


def level0(xy, level, scale):
    """`if (level != 0) pt *= scale` of the write-back: one float32 multiply per coordinate."""
    out = np.array(xy, F, copy=True).reshape(-1, 2)
    up = np.asarray(level) != 0
    s = np.asarray(scale, F)[np.asarray(level)[up]]
    out[up, 0] = (out[up, 0] * s).astype(F)
    out[up, 1] = (out[up, 1] * s).astype(F)
    return out


def stereo_frame(p, left, right, left_levels, right_levels) -> ss.StereoFrame:
    """The frame Frame::ComputeStereoMatches reads after the two extractions `left` / `right` (dicts of extract) of pair p."""
    c = np.ascontiguousarray
    return ss.StereoFrame(left_xy=level0(left["xy"], left["level"], p["left"]["scale"]), left_octave=c(left["level"], np.int32),
                          left_desc=c(left["descriptors"], np.uint8),
                          right_xy=level0(right["xy"], right["level"], p["right"]["scale"]), right_octave=c(right["level"], np.int32),
                          right_desc=c(right["descriptors"], np.uint8), scale_factors=c(p["left"]["scale"], F),
                          inv_scale_factors=c(p["left"]["inv_scale"], F), left_pyramid=[c(lv) for lv in left_levels],
                          right_pyramid=[c(lv) for lv in right_levels], bf=float(p["bf"]), b=float(p["b"]))


def assert_census(stage, octave, what):
    """The condition on the inputs: enough of every outcome for a comparison to mean something."""
    stage, octave = np.asarray(stage), np.asarray(octave)
    n = len(stage)
    count = lambda *s: int(np.isin(stage, s).sum())
    assert n > 0, what
    assert 4 * count(capi.OSH_STEREO_ACCEPTED) >= n, f"{what}: {count(capi.OSH_STEREO_ACCEPTED)} of {n} accepted"
    assert count(capi.OSH_STEREO_MEDIAN_CUT) >= 1, f"{what}: no keypoint cut at the median"
    assert count(capi.OSH_STEREO_NO_CANDIDATE, capi.OSH_STEREO_HAMMING) >= 1, f"{what}: none without candidate or beyond the distance"
    assert count(capi.OSH_STEREO_DISPARITY, capi.OSH_STEREO_BORDER_INC) >= 1, f"{what}: none at the disparity test or the window border"
    levels = np.unique(octave[stage == capi.OSH_STEREO_ACCEPTED])
    assert len(levels) >= 3, f"{what}: accepted keypoints on levels {levels.tolist()} only"
