"""The training step's drivers (Model::d_backward, Model::g_backward and their stages) against tests/golden/step_fixture.json.

Every call sequence of tests/step_cases.py -- three passes each, so that every graph segment runs eagerly, is captured and is
replayed -- must return the losses, leave the variables, optimizer state and gradients, and issue the recurrence launches that the
commit named in the fixture did: the one before the drivers were split into stages.  The fixture was recorded by
tools/record_step_fixture.py; bits are reproducible across processes, so every comparison is exact.

Like tests/test_gpu_init_tables.py this is a statement about a whole, unpartitioned MI355X: which persistent launches apply depends on
the residency probes of handle construction."""
import json
import os

import pytest

from tests.step_cases import CASES, GROUPS, group_cases, run_group

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_fixture.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_the_case_list():
    assert sorted(GOLDEN["cases"]) == sorted(c["name"] for c in CASES)
    assert GOLDEN["recorded_from_commit"] and GOLDEN["command"]
    assert all(c["note"] for c in CASES)


@pytest.mark.parametrize("group", GROUPS)
def test_step_matches_recorded_parent(group):
    got = run_group(group)
    assert sorted(got) == sorted(c["name"] for c in group_cases(group))
    for name in sorted(got):
        want, have = GOLDEN["cases"][name], got[name]
        assert "error" not in have, "%s: %s" % (name, have.get("error"))
        assert have["device_status"] == 0 and want["device_status"] == 0, name
        if "refusals" in want:
            assert have["refusals"] == want["refusals"], name
        else:
            for i, (h, w) in enumerate(zip(have["calls"], want["calls"])):
                assert h == w, "%s: call %d of %d returned other losses (fp32 bits) %s, recorded %s" % (name, i, len(want["calls"]), h, w)
            assert have["state_sha256"] == want["state_sha256"], name
            assert have.get("grads_sha256") == want.get("grads_sha256"), name
            assert have["profile_kinds"] == want["profile_kinds"], name
            assert have["profile_launches"] == want["profile_launches"], name
        assert have == want, name
