"""SVO_HIP_SIA_OPT_REDUCTION in the header, in the Python mirror and in the library's exports (no GPU needed)."""
import os
import re

from android_svo_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_define(name):
    text = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    m = re.search(r"^#define %s\s+\(?(-?\d+)\)?" % re.escape(name), text, re.M)
    assert m, name
    return int(m.group(1))


def test_the_constants_of_the_header_and_of_the_mirror_agree():
    assert _header_define("SVO_HIP_SIA_OPT_REDUCTION") == hip.SIA_OPT_REDUCTION == 10
    assert _header_define("SVO_HIP_SIA_REDUCTION_PER_WAVE") == hip.SIA_REDUCTION_PER_WAVE == 0
    assert _header_define("SVO_HIP_SIA_REDUCTION_TILE_ORDER") == hip.SIA_REDUCTION_TILE_ORDER == 1


def test_the_header_declares_and_the_library_exports_the_tracker_entry():
    text = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    assert re.search(r"int svo_hip_tracker_set_sia_option\(svo_hip_tracker\* trk, int option, int value\);", text)
    assert hasattr(hip.load_library(), "svo_hip_tracker_set_sia_option")
    assert hasattr(hip.Tracker, "set_sia_option") and hasattr(hip.TrackerGroup, "set_sia_option")
