"""The minimal-set validator, the batch bookkeeping and the null vector of a row array that osh_orb_two_view_reconstruct,
osh_orb_mlpnp_solve and osh_orb_sim3_ransac share (csrc/ransac_stage.h, csrc/jacobi_rows.h), without a GPU: the sanitizer program."""
import subprocess

from orb_slam3_study_kr_amd import capi

CSRC = capi.LIB_PATH.parent


def test_ransac_stage_check_runs_clean_under_the_sanitizers():
    """make ransac-stage-check: csrc/ransac_stage.h and csrc/jacobi_rows.h in a stand-alone host program under AddressSanitizer and UBSan."""
    r = subprocess.run(["make", "-C", str(CSRC), "ransac-stage-check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ransac_stage_check ok" in r.stdout and "ERROR" not in r.stdout + r.stderr and "runtime error" not in r.stdout + r.stderr
