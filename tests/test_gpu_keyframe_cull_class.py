"""LocalMapping::KeyFrameCulling (csrc/host/LocalMapping.cc) through the reference's signature on stand-in maps, counted on the
device: the culled keyframes, the links, the MergePrevious arguments and the points against the restatement of
tests/keyframe_cull_numpy.py, and one device call more than keyframes culled."""
import pytest

from orb_slam3_study_kr_amd import capi
from orb_slam3_study_kr_amd import synth_keyframe_cull as sk
from orb_slam3_study_kr_amd.host import HostCullGraph
from test_keyframe_cull_cpu import CLASS_SCENES, run_host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CLASS_SCENES))
def test_class_on_the_device(hip_lib, name):
    make, culled_ids = CLASS_SCENES[name]
    sc = make()
    got, kfs, _want = run_host(sc)
    assert [sc.kfs[k]["id"] for k in got["culled"]] == culled_ids
    assert got["device_calls"] == 1 + len(culled_ids)   # a keyframe with mbNotErase that is judged redundant adds none
    if name == "not_erase":
        a = sc.covisible[0]
        assert kfs[a]["to_be_erased"] == 1 and kfs[a]["bad"] == 0


def test_more_candidates_than_the_device_takes(hip_lib):
    """140 keyframes in the list, the first 101 of them culled; the loop never reaches the ones beyond the packed 128."""
    sc = sk.count_limits(140, False)
    got, _kfs, _want = run_host(sc)
    assert len(got["culled"]) == 101 and got["device_calls"] == 102


def test_fallback_beyond_the_table_limit(hip_lib):
    """A table of OSH_KFCULL_MAX_KEYFRAMES + 1 entries is counted on the host and gives what the device gives on the same map with
    one observer less."""
    small, large = sk.big_table(capi.OSH_KFCULL_MAX_KEYFRAMES), sk.big_table(capi.OSH_KFCULL_MAX_KEYFRAMES + 1)
    with HostCullGraph(small) as g:
        on_device = g.keyframe_culling()
    with HostCullGraph(large) as g:
        on_host = g.keyframe_culling()
    assert on_device["device_calls"] == 1 + len(on_device["culled"]) and on_host["device_calls"] == 0
    assert [small.kfs[k]["id"] for k in on_device["culled"]] == [large.kfs[k]["id"] for k in on_host["culled"]] == [100, 101]
