"""The plans the executor makes of the repo's five cfgs, pinned: kernel_count, arena_bytes, the step_model() list of layers and bytes, and under
FFGPU_KEEP_ALL the set of layers read_layer accepts, per case of tools/plan_pin.py (batches 1, 2, 3 -- 1 patches the batch input into add steps, 2
inserts the CNHW conversion and allows a split, 3 refuses it -- x flags 0, NO_FUSE, KEEP_ALL, CONCURRENT, SPLIT2 at batch 2, and FFGPU_BRANCH=1 /
FFGPU_DWPW=1 on yolo-fastest).  tests/data/plan_pin.json was recorded with that script on an MI355X BEFORE the planner's layout pass moved into
ffgpu_plan.hpp: a refactor of the planner changes none of it.  Create only: no forward runs.

(File name: the suite orders GPU test files by their base name (tests/conftest.py); this one runs with the other walks over cfgs.)"""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tools"))
import plan_pin                                                  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pins():
    with open(plan_pin.PIN) as fp:
        return json.load(fp)


@pytest.fixture(scope="module")
def nets():
    from ffcnn_amd import capi
    open_nets = {}

    def get(name):
        if name not in open_nets:
            open_nets[name] = capi.Net(plan_pin.cfg_path(name), os.path.join(ROOT, "data", "yolo-fastest-1.1.weights") if name == plan_pin.YOLO else None)
        return capi, open_nets[name]
    yield get
    for n in open_nets.values():
        n.close()


def test_the_table_has_every_case(pins):
    assert sorted(pins) == sorted(plan_pin.case_id(c) for c in plan_pin.CASES) and len(pins) == 5 * 13 + 6


@pytest.mark.parametrize("case", plan_pin.CASES, ids=plan_pin.case_id)
def test_plan_is_the_pinned_one(case, pins, nets, monkeypatch):
    for k in ("FFGPU_BRANCH", "FFGPU_DWPW", "FFGPU_NO_FUSE", "FFGPU_NO_INDIRECT"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case[3].items():
        monkeypatch.setenv(k, v)
    capi, net = nets(case[0])
    got = plan_pin.record(capi, net, case)
    want = pins[plan_pin.case_id(case)]
    assert got["kernel_count"] == want["kernel_count"] and got["arena_bytes"] == want["arena_bytes"]
    assert got == want
