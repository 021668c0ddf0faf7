"""The level list, the token lookup and the keypoint check that osh_orb_ic_angle, osh_orb_describe and the two calls that fill the
resident pyramid share (csrc/orb_pyramid_set.h), without a GPU: the sanitizer program."""
import subprocess

from orb_slam3_study_kr_amd import capi

CSRC = capi.LIB_PATH.parent


def test_pyramid_set_check_runs_clean_under_the_sanitizers():
    """make pyramid-set-check: csrc/orb_pyramid_set.h in a stand-alone host program under AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", str(CSRC), "pyramid-set-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "pyramid_set_check ok" in r.stdout and "ERROR" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
