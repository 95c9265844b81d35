"""Handle construction (Model::init and its stages, csrc/model_init.cpp) against tests/golden/init_tables.json.

Everything init decides is a deterministic function of (cfg, seed): the variable tables in the reference's graph-construction order,
the parameter counts, the bytes of device memory, the bits of the initial values, the gradient bucket ranges and the width of the
carried generator state.  The fixture was recorded by tools/record_init_tables.py from the commit named inside it -- the one before
init was split into stages -- so every comparison here is exact: no tolerance.

device_bytes includes the buffers that exist only where a residency probe succeeded (the rings of the persistent launches, the
in-kernel weight-gradient work space, the DPIPE ring), so this is a statement about a whole, unpartitioned MI355X -- as
__graft_entry__.smoke() already assumes when it asserts that the persistent launches ran."""
import json
import os

import pytest

from tests.init_cases import CASES, SEED, describe

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_tables.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_the_case_list():
    assert GOLDEN["seed"] == SEED
    assert sorted(GOLDEN["cases"]) == sorted(name for name, _ in CASES)


@pytest.mark.parametrize("name,kw", CASES, ids=[name for name, _ in CASES])
def test_init_matches_recorded_parent(name, kw):
    want = GOLDEN["cases"][name]
    got = json.loads(json.dumps(describe(kw)))          # (tuples -> lists, as the fixture went through JSON)
    assert got["tables"] == want["tables"], name
    assert got["param_count"] == want["param_count"], name
    assert got["device_bytes"] == want["device_bytes"], \
        "%s: device_bytes differ by %+d bytes (%d now, %d recorded)" % (name, got["device_bytes"] - want["device_bytes"],
                                                                        got["device_bytes"], want["device_bytes"])
    assert got["variables_sha256"] == want["variables_sha256"], name
    assert got["grad_buckets"] == want["grad_buckets"], name
    assert got["g_state_floats"] == want["g_state_floats"], name
    assert sorted(got) == sorted(want), name
