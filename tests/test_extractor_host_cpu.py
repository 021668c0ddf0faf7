"""The steps the bodies of csrc/host/ORBextractor.cc share and that make no device call (csrc/host/orb_extract_steps.h: the level
shapes, the sampling table, the write-back), without a GPU: the sanitizer program."""
import subprocess

from orb_slam3_study_kr_amd import capi

CSRC = capi.LIB_PATH.parent


def test_extractor_host_check_runs_clean_under_the_sanitizers():
    """make extractor-host-check: csrc/host/orb_extract_steps.h in a stand-alone host program under AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", str(CSRC), "extractor-host-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "extractor_host_check ok" in r.stdout and "ERROR" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
