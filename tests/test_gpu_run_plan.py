"""GPU pin test of the host's run plan (csrc/qn_host_minimize.hip.h: check_oracle, plan_run, plan_s2_args, pump_s2_sync / pump_s2_pipelined /
pump_ctl_sync / pump_ctl_pipelined, finish_stats; the launch helpers of csrc/qn_host_launch.hip.h; vec_minimize's share of them).

Every case of tests/run_plan_cases.py -- one short run per branch of the plan -- must leave exactly what the code left before minimize_impl was
split into those functions: the path flags, the launch and synchronisation counts, the iteration / evaluation / pass counters and byte totals of
qn_stats, for equality, and x bit for bit (the SHA-256 of its bytes).  The records are tests/golden/run_plan_pins.json, written by
tests/golden/make_run_plan_pins.py on the commit before the split.  A launch that moved, went missing or ran twice shows in `launches`; a predicate
that changed shows in `path`; anything that changed an argument shows in x."""
import json
import os

import pytest

import run_plan_cases as C

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_plan_pins.json")) as _fh:
    PINS = json.load(_fh)


def test_the_pins_cover_the_case_list():
    assert sorted(PINS["cases"]) == sorted(C.CASES)
    for name, fields in PINS["_omitted"].items():
        assert set(fields) <= {"host_syncs"}, name  # never path, launches or x


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_run_plan_leaves_what_it_left_before_the_split(qn, name):
    pinned = PINS["cases"][name]
    omitted = set(PINS["_omitted"].get(name, ()))
    got = C.CASES[name](qn)
    print(name, got)
    assert len(got) == len(pinned)
    for call, (rec, pin) in enumerate(zip(got, pinned)):
        assert {k: v for k, v in rec.items() if k not in omitted} == pin, (name, call)
