"""The refusals of osh_orb_extract, which need no device and no context: its own checks come before those of the pyramid build, and
a valid frame stops at the missing context."""
import numpy as np

import octree_numpy as on
import pyramid_numpy as pn
from orb_slam3_study_kr_amd import capi, orb

F = np.float32


def _item(**kw):
    scale = [F(1), F(1.2), F(F(1.2) * F(1.2))]
    it = dict(image=np.full((90, 120), 100, np.uint8), inv_scale=np.asarray(pn.standin_inv_scale(3), F), scale=np.asarray(scale, F),
              n_features=np.asarray(on.features_per_level(200, 1.2, 3), np.int32), pattern=orb.standin_pattern(), ini_th=20, min_th=7)
    it.update(kw)
    return it


def _rc(item, capacity=0):
    lib = capi.load_library()
    cf, cr, _keep, _ = orb.extract_args([item], [capacity])
    return lib.osh_orb_extract(None, 1, cf, cr), capi.last_error(lib)


def test_refusals_need_no_device():
    I, U = capi.OSH_ERR_INVALID, capi.OSH_ERR_UNSUPPORTED
    far = orb.standin_pattern().copy()
    far[0] = (15, 15)
    wide = orb.standin_pattern().astype(np.int16)
    for what, item, code in (("ini_th 0", _item(ini_th=0), I), ("ini_th 256", _item(ini_th=256), I), ("min_th above ini_th", _item(ini_th=5, min_th=9), I),
                             ("a table that reaches 22 pixels", _item(pattern=far), I),
                             ("blur weights that do not sum to 256", _item(blur_q8=np.asarray([1, 2, 3, 4, 3, 2, 1], np.uint16)), I),
                             ("scale nan", _item(scale=np.asarray([1, np.nan, 1.44], F)), I), ("scale 0", _item(scale=np.asarray([1, 0, 1.44], F)), I),
                             ("n_features above the limit", _item(n_features=np.asarray([capi.OSH_OCTREE_MAX_FEATURES + 1, 5, 5], np.int32)), U),
                             ("inv_scale negative (the pyramid build's)", _item(inv_scale=np.asarray([1, -1, 0.5], F)), I),
                             ("level 0 is not the image (the pyramid build's)", _item(inv_scale=np.asarray([0.5, 0.4, 0.3], F)), I)):
        rc, msg = _rc(item)
        assert rc == code and msg, what
    assert wide.max() <= 15          # the stand-in's table itself is inside the limits
    rc, msg = _rc(_item())
    assert rc == capi.OSH_ERR_INVALID and "no context" in msg
    lib = capi.load_library()
    assert lib.osh_orb_extract(None, -1, None, None) == capi.OSH_ERR_INVALID
    assert lib.osh_orb_extract_get_times(None, None) == capi.OSH_ERR_INVALID
