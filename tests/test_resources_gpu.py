"""Everything a context takes from the HIP runtime goes back with it: device buffers, pinned buffers, streams and events are owned by types that free
themselves (csrc/host/owned.hpp, csrc/hip_handles.hpp), and the process-wide census of what is alive (bpg_test_live_resources) returns to zero once the
contexts, circuits and trees of a scenario are gone - on the ordinary paths, on the failure paths, and however often contexts come and go.

The census is process-wide and the pytest process holds the contexts of other tests, so every scenario runs in a fresh child process: this file run as
`python tests/test_resources_gpu.py child <case>` prints one JSON line, which the test asserts on.  Sizes are the smallest that reach the code: generator
capacity 1024, the 8-bit BoundsCheck (16 multipliers) and its threefold repeat, a tree of 16 leaves.  Circuits come from the builders of the neighbouring
tests (tests/test_template_repeat_gpu.py, tests/test_check_gpu.py)."""
import json
import os
import pathlib
import subprocess
import sys

if __name__ == "__main__":
    _root = pathlib.Path(__file__).resolve().parent.parent
    sys.path[:0] = [str(_root), str(_root / "tests"), str(_root / "tests" / "golden")]

import pytest
import bulletproofs_gadgets_amd as bpg

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parent.parent
CAP = 1024
TABLE_BYTES = 2 * CAP * 96                  # [G | H] in affine Niels form, 96 bytes a point: 196,608
ZERO = [0] * 6
SEED = bytes(range(32))


def census():
    return [bpg.live_resources()[k] for k in bpg.LIVE_RESOURCE_KEYS]


# ------------------------------------------------------------------------------------------------ the scenarios (child process)
def bounds(ctx, tag, K):
    from test_template_repeat_gpu import host
    return host(ctx, "bounds8", tag, K)


def accepted(ctx, h, proof):
    return ctx.verify_flat(h.inst, h.state, h.coms, proof) == 0


def lockstep(ctx, tag, K):
    """K items proved in one lockstep call, every proof verified"""
    hs = [bounds(ctx, "%s-%d" % (tag, k), 1) for k in range(K)]
    res = ctx.prove_batch([(h.inst, h.state, h.inst.v_blinding, SEED, 0) for h in hs])
    return all(accepted(ctx, h, proof) for h, (proof, _) in zip(hs, res))


def case_everything():
    from test_template_repeat_gpu import template
    from test_check_gpu import bounds_values
    ok = {}
    ctx = bpg.Context(0)
    ctx.gens_ensure(CAP)
    ctx.profile_set(2)
    h = bounds(ctx, "res", 1)
    res = ctx.upload(h.inst)
    ctx.blinding_begin(h.state, h.inst.v_blinding, SEED, h.inst.n)          # slab, copy stream, block events; the prove below consumes the stream
    proof, _ = res.prove(h.state, h.inst.v_blinding, SEED)
    ok["stream proof"] = accepted(ctx, h, proof) and res.verify(h.state, h.coms, proof) == 0
    ok["lockstep batch"] = lockstep(ctx, "res-batch", 3)
    tmpl = template(ctx, "bounds8")
    tmpl.assign(h.inst.v, h.params)
    ok["template proof"] = accepted(ctx, h, tmpl.prove(h.state, h.inst.v_blinding, SEED)[0])
    tmpl.assign(bounds_values(0, True))
    report = tmpl.check()
    ok["check names the bad rows"] = (not report.ok) and report.bad_rows >= 1 and report.bad_multipliers == 0
    rep = tmpl.repeat(3)
    h3 = bounds(ctx, "res-rep", 3)
    ok["repeat proof"] = accepted(ctx, h3, h3.assign_and_prove(rep)[0])
    one = (1).to_bytes(32, "little")
    seg = {"table": "G", "first": 0, "len": 40, "result": 0, "lgblk": 31}
    skipped, _ = ctx.test_msm(1, [dict(seg, skip=[0b101, 0])], [one] * 40)
    plain, _ = ctx.test_msm(1, [seg], [bytes(32) if k in (0, 2) else one for k in range(40)])
    ok["msm with a skip bitmap"] = skipped == plain
    blocks = [bytes([k + 1]) + bytes(31) for k in range(6)]
    ok["sponges"] = ctx.mimc_sponge_many(blocks, 2) == [bpg.mimc_sponge(blocks[2 * k:2 * k + 2]) for k in range(3)]
    tree = ctx.merkle_tree([bytes([k]) * 32 for k in range(16)])
    ok["tree"] = len(tree.root()) == 32
    ok["bench_fe_mul"] = ctx.bench_fe_mul(1) > 0
    out = {"ok": ok, "open": census()}
    for c in (res, tmpl, rep):
        c.free()
    out["table_bytes_before_close"] = ctx.table_bytes()
    ctx.close()                                                             # the tree is still unfreed: its memory goes with the context
    out["closed_with_tree"] = census()
    tree.free()
    out["end"] = census()
    return out


def case_shared():
    a = bpg.Context(0); a.gens_ensure(CAP)
    one = census()
    b = bpg.Context(0)
    created = census()
    b.gens_ensure(CAP)
    two = census()
    a.close()
    after_first = census()
    ok = lockstep(b, "shared", 2)                                           # the survivor still proves on the tables the first context derived
    b.close()
    return {"one": one, "created": created, "two": two, "after_first": after_first, "ok": ok, "end": census()}


def case_failed_upload():
    ctx = bpg.Context(0); ctx.gens_ensure(CAP)
    h = bounds(ctx, "fail", 1)
    res = ctx.upload(h.inst)
    assert bpg.lib().bpg_test_fail_next_upload(ctx._h) == 0
    ctx.blinding_begin(h.state, h.inst.v_blinding, SEED, h.inst.n)
    try:
        res.prove(h.state, h.inst.v_blinding, SEED)
        status, message = 0, ""
    except bpg.BpgError as e:
        status, message = e.status, str(e)
    res.free()
    ctx.close()
    return {"status": status, "message": message, "end": census()}


def case_refused_create():
    """the parent sets BPG_RSEG=3 for `knob`, nothing for `device`"""
    try:
        bpg.Context(9999 if "BPG_RSEG" not in os.environ else 0)
        status = 0
    except bpg.BpgError as e:
        status = e.status
    return {"status": status, "end": census()}


def case_churn():
    open_bytes, closed, ok = [], [], True
    for k in range(8):
        ctx = bpg.Context(0); ctx.gens_ensure(CAP)
        ok = lockstep(ctx, "churn-%d" % k, 2) and ok
        open_bytes.append(census()[1])
        ctx.close()
        closed.append(census())
    return {"open_bytes": open_bytes, "closed": closed, "ok": ok}


CASES = {"everything": case_everything, "shared": case_shared, "failed_upload": case_failed_upload, "refused_knob": case_refused_create,
         "refused_device": case_refused_create, "churn": case_churn}


# ------------------------------------------------------------------------------------------------ the tests (parent process)
def run_child(case, env=None):
    e = dict(os.environ)
    e.pop("BPG_GENS_SHARE", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, str(ROOT / "tests" / "test_resources_gpu.py"), "child", case], env=e, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    print(case, out)
    return out


def test_everything_once_then_nothing_left():
    """One context runs every feature that owns memory, a stream or an event - the generator tables, the profile's events, a circuit, a blinding stream
    and the proof that consumes it, verification, a lockstep wave, a template with assign, check and repeat, an MSM with a skip bitmap, sponges, a tree, the
    field-multiplication bench.  Every proof verifies; then the circuits are freed, the context is closed over the unfreed tree, the tree handle is freed:
    nothing is alive."""
    out = run_child("everything")
    assert all(out["ok"].values()), out["ok"]
    dev, dev_bytes, pin, pin_bytes, streams, events = out["open"]
    assert dev > 0 and dev_bytes > TABLE_BYTES and pin > 0 and pin_bytes > 0 and streams >= 2 and events > 0, out["open"]
    assert out["table_bytes_before_close"] == 0
    assert out["closed_with_tree"] == ZERO and out["end"] == ZERO


def test_shared_tables_go_with_their_last_context():
    """Two contexts of one device share one generator table.  The issue's bound - the second context adds less than one table (196,608 bytes) - is asserted
    on what its gens_ensure adds (nothing: it adopts the table).  Creation is measured apart, because every context owns a Pedersen window table that happens
    to be a generator table's size (3 x 64 windows x 8 multiples x 128 bytes = 196,608), so creation plus gens_ensure together cannot stay under the bound;
    instead the second context must hold exactly what the first holds without the table."""
    out = run_child("shared")
    one, created, two = out["one"][1], out["created"][1], out["two"][1]
    assert two - created < TABLE_BYTES and two - created == 0
    assert two - one == one - TABLE_BYTES, (one, two)
    assert out["after_first"][1] >= TABLE_BYTES and out["after_first"][1] == one        # the first context is gone, the table it derived is not
    assert out["ok"] and out["end"] == ZERO


def test_a_failed_upload_leaves_nothing():
    out = run_child("failed_upload")
    assert out["status"] == 7 and "upload" in out["message"], out
    assert out["end"] == ZERO


@pytest.mark.parametrize("case,env,status", [("refused_knob", {"BPG_RSEG": "3"}, 4), ("refused_device", {}, 7)])
def test_a_refused_context_leaves_nothing(case, env, status):
    """BPG_RSEG=3 is no power of two (BPG_ERR_INVALID_ARGUMENT, before the device is touched); device 9999 does not exist (BPG_ERR_DEVICE)"""
    out = run_child(case, env)
    assert out["status"] == status and out["end"] == ZERO, out


def test_eight_contexts_in_sequence():
    out = run_child("churn")
    assert out["ok"]
    assert out["closed"] == [ZERO] * 8
    assert len(set(out["open_bytes"])) == 1 and out["open_bytes"][0] > TABLE_BYTES, out["open_bytes"]


if __name__ == "__main__":
    assert sys.argv[1] == "child"
    print(json.dumps(CASES[sys.argv[2]]()))
