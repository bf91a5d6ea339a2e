"""The decisions of the MSM and of the generator fold live in host headers without HIP (csrc/host/msm_plan.hpp, csrc/host/fold_plan.hpp): checked here on the
CPU, as a stand-alone program under the sanitizers - no device, no preload."""
import json
import subprocess

import oracle_lib as O

CSRC = O.ROOT / "bulletproofs_gadgets_amd" / "csrc"


def test_msm_planner_fold_chooser_and_recoders_under_the_sanitizers(tmp_path):
    """tests/hostcheck/plans.cpp: plan_msm on the prover's shapes (every figure, the arena identities, the refusals by type), choose_fold row by row, and
    the three recoders against integer arithmetic mod l, into buffers of exactly the sizes the formulas give"""
    exe = tmp_path / "plans"
    src = O.ROOT / "tests" / "hostcheck" / "plans.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr
    assert r.stdout.split()[-1] == "ok"
    # the chosen scalars the program built by the rules of tests/fold_cases.py are the ones that module builds: the recoders were checked on the very values
    # the fold kernels are run on (test_fold_kernels_gpu.py)
    import re
    import fold_cases as F
    built = {name: int(value, 16) for name, value in re.findall(r"^chosen \[(.+)\] ([0-9a-f]{64})$", r.stdout, re.M)}
    want = dict(F.named())
    for w in range(3, 9):
        want.update(F.width_patterns(w))
        want.update({"w%d parts %d %s" % (w, parts, kind): F.parts_extreme(w, parts, kind) for parts in (1, 2, 4, 8) for kind in F.PARTS_KINDS})
    assert len(want) == 19 + 6 * 24 + 1 and built == want


def test_the_engine_keeps_no_plan_state_between_calls():
    """What an MSM skips and discounts travels with its segments (MsmJob), and the recoders and the plan live in the host headers: none of the names of the
    hidden call-to-call state, of the second plan record or of the recoders is left in the engine, and the planning headers include no HIP."""
    engine = (CSRC / "engine.hip").read_text()
    for name in ("msm_skipped_terms", "msm_alg_discount", "struct MsmLast", "naf256", "wnaf256", "scalar_bits"):
        assert name not in engine, name
    assert engine.count(">> (g_r - k)) & 1u") == 0            # the group-scalar product loop: once, in fold_plan.hpp
    for header in ("msm_plan.hpp", "fold_plan.hpp"):
        text = (CSRC / "host" / header).read_text()
        assert "#include <hip" not in text and "__global__" not in text and "__device__" not in text, header
    assert (CSRC / "host" / "fold_plan.hpp").read_text().count(">> (g_r - k)) & 1u") == 1


def test_launch_census_golden_is_the_shape_the_gpu_test_reads():
    """tests/golden/launch_census.json (recorded by tools/diag/launch_census.py): five cases, counts and the three bookkeeping sums per kernel, and the fold
    kernels the chooser names for each case"""
    census = json.loads((O.ROOT / "tests" / "golden" / "launch_census.json").read_text())
    assert sorted(census) == ["a", "b", "c", "d", "e"]
    for case in census.values():
        assert set(case) == {"kernels", "schedule"} and set(case["schedule"]) == {"merged_last", "merged_skipped_last", "shared_variants_last"}
        assert all(set(v) == {"count", "alg_bytes", "device_bytes", "field_mults"} and v["count"] > 0 for v in case["kernels"].values())
    folds = lambda name: {k: v["count"] for k, v in census[name]["kernels"].items() if k.startswith("k_fold_points")}
    assert folds("a") == {"k_fold_points_quad": 3, "k_fold_points_quadw": 1}
    assert folds("b") == {"k_fold_points_reg": 4, "k_fold_points_regw": 1}
    assert folds("c")["k_fold_points_wnaf"] == 1
    assert census["d"]["schedule"]["merged_skipped_last"] > 0
    assert folds("e") == {} and census["e"]["kernels"]["k_bucket_chunks"]["count"] == 1        # the table-driven path: the verifier's sum is the only MSM
