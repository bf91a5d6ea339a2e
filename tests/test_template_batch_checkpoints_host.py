"""Checkpointed templates in lockstep batches without a GPU (bpg_r1cs_prove_template_batch_checkpointed): the batched witness interpreter with per-item
checkpoint values compiled for the host (bpg_test_template_eval_batch_checkpointed: poisoned vectors, the segments of every level in reverse order, then the
verify step per item), the symbol, the layout of the frozen bpg_template_ck_item and the refusal of a handle without device state.

The yardstick is the EXISTING batched interpreter on the same program WITHOUT checkpoints (bpg_test_template_eval_batch_hinted) - which the existing tests
hold against the prover's own host assembly - and that assembly itself.  The checkpoint VALUES never come from the circuit (checkpoint_cases.py).  The
template is made from ONE witness (seed 1) and evaluated on those of the other seeds."""
import ctypes as C
import re
import subprocess

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import checkpoint_cases as CK
from test_template_checkpoints_host import StubProver, FAKE, _err, _views, program

NONE = 2**64 - 1
CIRCUITS = {
    "chain": lambda seed: CK.chain(None, seed=seed, prover_cls=StubProver),
    "preimage3": lambda seed: CK.preimage3(None, seed=seed, prover_cls=StubProver),
    "path": lambda seed: CK.path(None, 5, depth=3, seed=seed, prover_cls=StubProver),
}
FIELDS = ("v", "param_values", "transcript_state", "v_blinding", "rng_seed", "flags", "proof_out", "proof_len", "commitments_out", "ck_values", "first_mismatch")


def eval_batch_ck(inst, prog, hints, ck_vars, vs, cks):
    """bpg_test_template_eval_batch_checkpointed -> (per item (aL, aR, aO) of N x 32 bytes each, per item first mismatch or None)"""
    K, N = len(vs), 1 << (inst.n - 1).bit_length()
    cs, cp, ch, ck = _views(inst, prog, hints, ck_vars)
    out = [C.create_string_buffer(32 * N * K) for _ in range(3)]
    first = (C.c_uint64 * max(K, 1))(*[12345] * max(K, 1))
    st = bpg.lib().bpg_test_template_eval_batch_checkpointed(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.byref(ck), C.c_uint64(K),
                                                             b"".join(vs), b"".join(b"".join(c) for c in cks) or None, *out, first)
    assert st == 0, _err()
    return [tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out) for k in range(K)], [None if first[k] == NONE else first[k] for k in range(K)]


def eval_batch_plain(inst, prog, hints, vs):
    """the existing hook: the same program without checkpoints"""
    K, N = len(vs), 1 << (inst.n - 1).bit_length()
    cs, cp, ch, _ = _views(inst, prog, hints, [])
    out = [C.create_string_buffer(32 * N * K) for _ in range(3)]
    st = bpg.lib().bpg_test_template_eval_batch_hinted(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, C.c_uint64(K), b"".join(vs), *out)
    assert st == 0, _err()
    return [tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out) for k in range(K)]


@pytest.fixture(scope="module", params=sorted(CIRCUITS))
def case(request):
    """(template instance, program, hints, checkpoint variables, the witnesses of seeds 2, 3, 4 and their plain evaluation) - computed once per circuit"""
    build = CIRCUITS[request.param]
    base = build(1)
    inst, prog, hints = program(base)
    others = [build(s) for s in (2, 3, 4)]
    insts = [a.prover.instance() for a in others]
    assert len({i.v for i in insts} | {inst.v}) == 4
    return inst, prog, hints, base.ck_vars, others, insts, eval_batch_plain(inst, prog, hints, [i.v for i in insts])


@pytest.mark.parametrize("count", [1, 3])
def test_correct_values_give_the_plain_witness(case, count):
    inst, prog, hints, ck_vars, others, insts, plain = case
    n, N = inst.n, 1 << (inst.n - 1).bit_length()
    got, first = eval_batch_ck(inst, prog, hints, ck_vars, [i.v for i in insts[:count]], [a.ck_values for a in others[:count]])
    assert first == [None] * count
    for k in range(count):
        assert got[k] == plain[k], "item %d: the checkpointed batch differs from the batch without checkpoints" % k
        for vec, host in zip(got[k], (insts[k].aL, insts[k].aR, insts[k].aO)):
            assert vec[:32 * n] == host, "item %d: differs from the host assembly" % k
            assert vec[32 * n:] == bytes(32 * (N - n)), "item %d: rows [n, N) must be zero" % k


def test_every_item_reports_its_own_lowest_mismatch(case):
    inst, prog, hints, ck_vars, others, insts, plain = case
    wrong = lambda b: bpg.scalar_op("add", b, bpg.scalar_from_int(1))
    n_ck = len(ck_vars)
    assert n_ck >= 3
    cks = [list(a.ck_values) for a in others]
    cks[1][n_ck - 1] = wrong(cks[1][n_ck - 1])                              # one value of item 1
    cks[2][n_ck - 1] = wrong(cks[2][n_ck - 1]); cks[2][1] = wrong(cks[2][1])    # two of item 2: the lowest is reported
    got, first = eval_batch_ck(inst, prog, hints, ck_vars, [i.v for i in insts], cks)
    assert first == [None, n_ck - 1, 1]
    assert got[0] == plain[0]
    # another witness's values under item 0's committed values: checkpoint 0 already differs
    got, first = eval_batch_ck(inst, prog, hints, ck_vars, [insts[0].v, insts[1].v], [others[1].ck_values, others[1].ck_values])
    assert first == [0, None] and got[1] == plain[1]


def test_an_empty_batch_and_no_checkpoints(case):
    inst, prog, hints, ck_vars, others, insts, plain = case
    got, first = eval_batch_ck(inst, prog, hints, ck_vars, [], [])
    assert got == [] and first == []
    got, first = eval_batch_ck(inst, prog, hints, [], [insts[0].v], [[]])       # no checkpoints: the existing hook, and nothing to report
    assert first == [None] and got[0] == plain[0]
    cs, cp, ch, ck = _views(inst, prog, hints, ck_vars)
    out = [C.create_string_buffer(32 * (1 << (inst.n - 1).bit_length())) for _ in range(3)]
    first = (C.c_uint64 * 1)()
    assert bpg.lib().bpg_test_template_eval_batch_checkpointed(C.byref(cs), C.byref(cp), None, C.byref(ck), C.c_uint64(1), insts[0].v, None, *out, first) == 4


def test_symbol_header_and_item_layout(tmp_path):
    lib = bpg.lib()
    assert all(hasattr(lib, f) for f in ("bpg_r1cs_prove_template_batch_checkpointed", "bpg_test_template_eval_batch_checkpointed"))
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "bpg_template_ck_item" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)
    assert re.search(r"#define BPG_ABI_VERSION 7u", hdr)                    # an addition to ABI version 7: no bump
    proto = [x.strip() for x in re.search(r"bpg_status bpg_r1cs_prove_template_batch_checkpointed\(([^)]*)\);", hdr).group(1).split(",")]
    assert proto == ["bpg_ctx *ctx", "bpg_circuit *tmpl", "uint64_t count", "const bpg_template_ck_item *items", "int32_t commit", "bpg_status *status_out"]
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_template_ck_item, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%zu' + " %zu" * len(FIELDS) +
                   '\\n", sizeof(bpg_template_ck_item), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert [f for f, _ in bpg._TemplateCkItem._fields_] == list(FIELDS)
    assert [f for f, _ in bpg._TemplateCommitItem._fields_] == list(FIELDS[:9])         # the nine fields of bpg_template_commit_item, same order
    assert [C.sizeof(bpg._TemplateCkItem)] + [getattr(bpg._TemplateCkItem, f).offset for f in FIELDS] == want


def test_a_handle_without_device_state_is_refused():
    lib = bpg.lib()
    a = CK.chain(None, seed=1, prover_cls=StubProver)
    inst, prog, hints = program(a)
    cs, cp, ch, _ = _views(inst, prog, hints, [])
    h = C.c_void_p()
    assert lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(cp), None, C.byref(h)) == 0, _err()
    res = bpg.ResidentCircuit(None, None, inst.n, inst.m, n_params=0)       # only the item builder is used: no handle, no context
    state = a.transcript.state
    arr, keep = res._template_items([(inst.v, [], state, inst.v_blinding, bytes(32), 0)] * 2, bpg._TemplateCkItem)
    firsts = [C.c_uint64(5), C.c_uint64(5)]
    ck = b"".join(a.ck_values)
    for k in range(2):
        arr[k].ck_values = ck; arr[k].first_mismatch = C.pointer(firsts[k])
    two = C.c_uint64(2)

    def untouched(status):
        return (list(status) == [77, 77] and [f.value for f in firsts] == [5, 5]
                and all(k[0].raw[:203] == state and k[1].raw == bytes(len(k[1])) and k[2].value == len(k[1]) for k in keep))
    try:
        status = (C.c_int32 * 2)(77, 77)
        for commit in (0, 1):
            assert lib.bpg_r1cs_prove_template_batch_checkpointed(None, h, two, arr, C.c_int32(commit), status) == 4 and "no device state" in _err() and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch_checkpointed(FAKE, h, two, arr, C.c_int32(commit), status) == 4 and "no device state" in _err() and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch_checkpointed(FAKE, h, C.c_uint64(0), None, C.c_int32(commit), None) == 4
            assert lib.bpg_r1cs_prove_template_batch_checkpointed(None, None, two, arr, C.c_int32(commit), status) == 4 and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch_checkpointed(FAKE, None, two, arr, C.c_int32(commit), status) == 4 and untouched(status)
    finally:
        lib.bpg_r1cs_free(None, h)
