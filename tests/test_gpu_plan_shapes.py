"""Plan creation reproduces the recorded launch shapes (tests/golden/plan_shapes.json).

Every case of tests/golden/make_plan_shapes.py's table creates a plan and reads it back -- no kernel runs --
and the status of msa_plan_create, the launch info, the cells size, the stripe count, every pair's layout and
the static run-info fields must equal what the recorder wrote on the same device type: the host-side plan
code decides which kernel family launches and in which shape, and this pins every such decision.
"""
import importlib.util
import json
import os

import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_plan_shapes", GOLDEN / "make_plan_shapes.py")
MK = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(MK)

RECORDED = json.loads((GOLDEN / "plan_shapes.json").read_text())


@pytest.fixture(scope="module")
def same_setting(dev):
    """The recorded shapes hold on the device type they were recorded on, with the library's defaults."""
    facts = MK.device_facts()
    assert facts == RECORDED["device"], (
        f"plan_shapes.json was recorded on {RECORDED['device']}, this device is {facts}: grids and occupancies "
        "differ between them; record the file on this device type with tests/golden/make_plan_shapes.py")
    set_ = [k for k in MK.ONCE_PER_PROCESS if k in os.environ]
    assert not set_, f"{set_} set in the environment: libmsa reads them once per process and the shapes move"


def test_case_table_matches_recording():
    assert [c["name"] for c in MK.CASES] == list(RECORDED["cases"])


MODES = {"stripe": 0, "flow": 1, "chunked": 2, "split": 3, "band": 4, "band_chunked": 5, "cflow": 6}
# what the table is there to reach: case -> (launch mode, separate pass-2 launch)
REACHES = {
    "stripe_batch_h": ("stripe", False), "stripe_single_gotoh_tab_st1": ("stripe", False),
    "stripe_single_gotoh_dir_st1": ("stripe", False), "stripe_single_partial_tab": ("stripe", False),
    "stripe_single_sw_score_end": ("stripe", False), "stripe_single_nw_unbanded": ("stripe", False),
    "split_h": ("split", False), "cflow_4": ("cflow", False), "cflow_4_lockstep": ("stripe", False),
    "packed_1024": ("stripe", False), "unpacked_score_batch": ("stripe", False),
    "flow_score": ("flow", False), "flow_h_whole_rows": ("flow", False), "flow_h_code_rings": ("flow", False),
    "flow_h_end_packed": ("flow", False), "flow_h_end_unpacked": ("flow", False),
    "flow_affine_dir_nneg": ("flow", False), "flow_affine_dir_floor": ("flow", False),
    "flow_gotoh_dir": ("flow", False), "fill_swl_h": ("flow", True), "fill_affine": ("flow", True),
    "fill_gotoh": ("flow", True), "band_exact_h": ("band", False), "band_exact_score": ("band", False),
    "band_chunked_h16": ("band_chunked", False), "band_chunked_i32": ("band_chunked", False),
}


def test_recording_reaches_every_family():
    """The recorded file itself: the success rows reach the launch paths they are named for."""
    for name, (mode, fill) in REACHES.items():
        rec = RECORDED["cases"][name]
        assert rec["status"] == 0, name
        assert rec["launch_info"][0] == MODES[mode], (name, rec["launch_info"])
        assert (rec["launch_info"][5] > 0) == fill, (name, rec["launch_info"])
    assert RECORDED["cases"]["band_chunked_h16"]["run_info_0_1_3"][2] >> 16 == 1
    assert RECORDED["cases"]["band_chunked_i32"]["run_info_0_1_3"][2] >> 16 == 0
    assert all(rec["status"] != 0 for name, rec in RECORDED["cases"].items() if name.startswith("bad_"))


@pytest.mark.parametrize("c", MK.CASES, ids=[c["name"] for c in MK.CASES])
def test_plan_shape(same_setting, c):
    got = MK.probe(c)
    print(c["name"], got if len(c["ms"]) <= 4 else {k: v for k, v in got.items() if k != "layout"})
    assert got == RECORDED["cases"][c["name"]]
