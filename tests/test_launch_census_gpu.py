"""What proof bytes cannot pin: which kernels ran, how often, and with what roofline bookkeeping.  Every choice of fold kernel and every MSM plan gives the
same bytes, so a slip in the chooser (host/fold_plan.hpp), in the planner (host/msm_plan.hpp) or in the counts that travel with an MSM's segments would
pass every parity test and only cost time.  tools/diag/launch_census.py runs five small cases, each on a fresh context under profile_set(2); this compares
what it reports with tests/golden/launch_census.json, a recording made with the engine as it was before the planners moved out of it.

Counts must match exactly.  alg_bytes, device_bytes and field_mults are sums of deterministic host arithmetic on fixed inputs, printed as whole numbers
(two recordings in separate processes were byte-identical): they must match to a relative 1e-12, which allows for the JSON round trip only.  total_ms is
never read."""
import importlib.util
import json

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

GOLDEN = json.loads((O.ROOT / "tests" / "golden" / "launch_census.json").read_text())


@pytest.fixture(scope="module")
def census_tool():
    spec = importlib.util.spec_from_file_location("launch_census", O.ROOT / "tools" / "diag" / "launch_census.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_launch_census_matches_the_recording(census_tool, name):
    want = GOLDEN[name]
    got = census_tool.run_case(name)
    print(name, json.dumps(got, sort_keys=True))
    if name == "d":
        assert got["schedule"]["merged_skipped_last"] > 0, "the merged A_I / A_O path (skipped and discounted terms) must really be taken"
    assert got["schedule"] == want["schedule"]
    assert {k: v["count"] for k, v in got["kernels"].items()} == {k: v["count"] for k, v in want["kernels"].items()}
    for kernel, w in want["kernels"].items():
        for key in census_tool.SUMS:
            assert got["kernels"][kernel][key] == pytest.approx(w[key], rel=1e-12, abs=0), (kernel, key)
