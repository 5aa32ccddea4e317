"""GPU pin test of the host layer that chooses between the device objective kinds (csrc/qn_host_objective.hip.h and the kinds' own host files: the
state blocks of qn_objective and the QnObjOps table of every kind; their callers in qn_host_vec.hip.h, qn_vec_exact.hip.h, qn_host_newton_cg.hip.h,
qn_host_minimize.hip.h and qn_host_newton.hip.h).

Every case of tests/objective_pin_cases.py -- per kind, every host entry point once and one short run of every solver family -- must leave exactly
what the code left before the kinds were given one state block and one operations table each: the bytes every entry point returns (their SHA-256),
the class and the full text of every refusal, the path flags, launch and synchronisation counts, evaluation / pass counters and byte totals of
qn_stats, for equality, x bit for bit, NewtonCG's and ExactQuadratic's counters, and which profiling classes were timed at all.  The records are
tests/golden/objective_pins.json, written by tests/golden/make_objective_pins.py on the commit before the regrouping."""
import json
import os

import pytest

import objective_pin_cases as C

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "objective_pins.json")) as _fh:
    PINS = json.load(_fh)


def test_the_pins_cover_the_case_list():
    assert sorted(PINS["cases"]) == sorted(C.CASES)
    for name, fields in PINS["_omitted"].items():
        assert set(fields) <= {"host_syncs"}, name  # never a hash, a message, path, launches or bytes


@pytest.mark.parametrize("name", sorted(C.CASES))
def test_objective_leaves_what_it_left_before_the_regrouping(qn, name):
    pinned = PINS["cases"][name]
    omitted = set(PINS["_omitted"].get(name, ()))
    got = C.CASES[name](qn)
    print(name, got)
    assert len(got) == len(pinned)
    for call, (rec, pin) in enumerate(zip(got, pinned)):
        assert {k: v for k, v in rec.items() if k not in omitted} == pin, (name, call)
