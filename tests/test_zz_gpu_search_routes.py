"""Which launches serve a batch (lance_amd/csrc/search_plan.h): the grid of tests/search_routes_spec.py -- one tiny search per route
of the plan, each called three times through the same buffers (plain, captured into a HIP graph, replayed), and one group per A/B
switch in a child process (the switches are read once per process) -- must make exactly the launches recorded in
tests/golden/search_routes.json (scripts/record_search_routes.py; the `count:<stage>` deltas of every call) and give the oracle's ids
and distances, bit for bit.

Gates that no search of a few thousand rows reaches -- a list of 65,536 rows or more, the two 2 GiB scratch limits, lists in the
thousands -- are covered on the CPU only (tests/test_search_plan_cpu.py), as is every threshold's other side."""
import os

import pytest

import search_routes_spec as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    return R.golden()


def test_the_golden_table_covers_the_grid(golden):
    assert set(golden) == {"default"} | set(R.SWITCHED) and set(golden["default"]) == set(R.CASES)
    for group, (_, names) in R.SWITCHED.items():
        assert set(golden[group]) == set(names), group


@pytest.mark.parametrize("name", list(R.CASES))
def test_route_and_answer(eng, oracle, golden, name):
    for sw in R.SWITCH_NAMES:      # a switch in this process's environment would have been read by the library already
        assert sw == "LANCE_HIP_DOT_FLOW_SKEW" or not os.environ.get(sw), f"{sw} is set: the default routes cannot be checked"
    got = R.run_case(eng, oracle, name)
    print(name, got)
    assert got == golden["default"][name]


@pytest.mark.parametrize("group", list(R.SWITCHED))
def test_route_and_answer_under_a_switch(golden, group):
    env, names = R.SWITCHED[group]
    got = R.run_in_child(env, names)
    print(group, got)
    assert got == golden[group]
