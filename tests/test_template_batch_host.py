"""Lockstep template batches without a GPU: the batched witness interpreter compiled for the host (bpg_test_template_eval_batch), the refusals of
bpg_r1cs_prove_template_batch that need no device, and the layout of the frozen bpg_template_item.

The yardstick is the EXISTING host assembly: every item's slice of the wave layout must hold the a_L, a_R, a_O the prover itself exported for that
witness, and what the single interpreter (bpg_test_template_eval) gives for the item alone.  The template is always made from ONE witness (seed 1) and
evaluated on the committed values of the others: one shape, many witnesses."""
import ctypes as C
import re
import subprocess

import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
from test_template_host import StubProver, schedule, FAKE, _err

L = bpg.L
FIELDS = ("v", "param_values", "transcript_state", "v_blinding", "rng_seed", "flags", "proof_out", "proof_len")


def eval_batch(inst, prog, vs):
    """bpg_test_template_eval_batch -> per item (aL, aR, aO) of N x 32 bytes each, N = padded size"""
    K, N = len(vs), 1 << (inst.n - 1).bit_length()
    out = [C.create_string_buffer(32 * N * K) for _ in range(3)]
    cs, cp = inst.cstruct(), prog.cstruct()
    assert bpg.lib().bpg_test_template_eval_batch(C.byref(cs), C.byref(cp), C.c_uint64(K), b"".join(vs), *out) == 0, _err()
    return N, [tuple(o.raw[32 * N * k:32 * N * (k + 1)] for o in out) for k in range(K)]


def eval_single(inst, prog, v):
    out = [C.create_string_buffer(32 * inst.n) for _ in range(3)]
    cs, cp = inst.cstruct(), prog.cstruct()
    assert bpg.lib().bpg_test_template_eval(C.byref(cs), C.byref(cp), v, *out) == 0, _err()
    return tuple(o.raw for o in out)


def check_items(inst, prog, insts, vs):
    N, got = eval_batch(inst, prog, vs)
    assert N >= inst.n and N < 2 * inst.n
    for k, (want, v) in enumerate(zip(insts, vs)):
        assert want.n == inst.n
        for vec, alone, host in zip(got[k], eval_single(inst, prog, v), (want.aL, want.aR, want.aO)):
            assert vec[:32 * inst.n] == alone, "item %d: the batched interpreter differs from the single one" % k
            assert vec[:32 * inst.n] == host, "item %d: the batched interpreter differs from the host assembly" % k
            assert vec[32 * inst.n:] == bytes(32 * (N - inst.n)), "item %d: padding rows must be zero" % k


def test_eight_leaf_tree_five_witnesses():
    trees = [workloads.merkle_full_tree(None, leaves=8, seed=s, prover_cls=StubProver) for s in (1, 2, 3, 4, 5)]
    insts = [a.prover.instance() for a in trees]
    inst, prog = insts[0], trees[0].prover.witness_program()
    S = schedule(inst, prog)
    assert inst.n == 13608 and S["segments"] == 14 and S["levels"] == 6 and S["level_segments"] == [4, 4, 2, 2, 1, 1]
    assert len({i.v for i in insts}) == 5
    check_items(inst, prog, insts, [i.v for i in insts])


def two_leaf(leaf_ints):
    t = bpg.Transcript(b"MerkleTree"); p = StubProver(None, t)
    raw = [x.to_bytes(32, "little") for x in leaf_ints]
    vs = [p.commit(b, bytes(32))[1] for b in raw]
    bpg.MerkleTree256(bytes(32), [], bpg.vars_to_lc(vs), "(W W)").prove(p, [], [])
    return p, b"".join(raw)


def test_two_leaf_tree_with_an_unreduced_committed_value():
    """item 1 carries committed values >= l and below 2^255 (Scalar::from_bits range): reduced as the single call reduces them"""
    big = [(L + 5) | (1 << 254), (1 << 255) - 19]
    assert all(L <= x < (1 << 255) for x in big)
    built = [two_leaf(x) for x in ([11, 12], big, [L - 1, 0], [7, 7])]
    insts = [p.instance() for p, _ in built]
    inst, prog = insts[0], built[0][0].witness_program()
    assert schedule(inst, prog)["levels"] == 2 and inst.n == 1944
    check_items(inst, prog, insts, [raw for _, raw in built])               # the raw bytes, as handed to commit()
    N, none = eval_batch(inst, prog, [])                                     # an empty batch writes nothing
    assert none == []


def test_call_refusals_need_no_device():
    lib = bpg.lib()
    a = workloads.mimc_preimage(None, nbytes=40, seed=2, prover_cls=StubProver)
    inst, prog = a.prover.instance(), a.prover.witness_program()
    prog.param_rows = [inst.q - 1]
    cs, cp = inst.cstruct(), prog.cstruct()
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle(C.byref(cs), C.byref(cp), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 0, _err()
    res = bpg.ResidentCircuit(None, None, inst.n, inst.m, n_params=1)       # only the item builder is used: no handle, no context
    state = a.transcript.state
    arr, keep = res._template_items([(inst.v, [bytes(32)], state, inst.v_blinding, bytes(32), 0)] * 2)
    two = C.c_uint64(2)

    def untouched(status):
        return list(status) == [77, 77] and all(k[0].raw[:203] == state and k[1].raw == bytes(len(k[1])) and k[2].value == len(k[1]) for k in keep)
    try:
        status = (C.c_int32 * 2)(77, 77)
        assert lib.bpg_r1cs_prove_template_batch(None, tmpl, two, arr, status) == 4 and untouched(status)          # NULL ctx
        assert lib.bpg_r1cs_prove_template_batch(None, None, two, arr, status) == 4 and untouched(status)
        assert lib.bpg_r1cs_prove_template_batch(FAKE, None, two, arr, status) == 4 and untouched(status)          # NULL tmpl
        for h in (tmpl, plain):         # a handle without device state: refused whatever else is passed
            assert lib.bpg_r1cs_prove_template_batch(FAKE, h, two, arr, status) == 4 and "no device state" in _err() and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch(None, h, two, arr, status) == 4 and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch(FAKE, h, two, None, status) == 4 and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch(FAKE, h, two, arr, None) == 4 and untouched(status)
            assert lib.bpg_r1cs_prove_template_batch(FAKE, h, C.c_uint64(0), None, None) == 4
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)


def test_template_item_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_template_item, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%u %zu' + " %zu" * len(FIELDS) +
                   '\\n", BPG_ABI_VERSION, sizeof(bpg_template_item), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert want[0] == 7                                                     # an addition to ABI version 7: no bump
    assert [f for f, _ in bpg._TemplateItem._fields_] == list(FIELDS)
    got = [C.sizeof(bpg._TemplateItem)] + [getattr(bpg._TemplateItem, f).offset for f in FIELDS]
    assert got == want[1:], (got, want)
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "bpg_template_item" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)           # listed with the frozen structs
    proto = lambda name: [x.strip() for x in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    assert proto("bpg_r1cs_prove_template_batch") == ["bpg_ctx *ctx", "bpg_circuit *tmpl", "uint64_t count", "const bpg_template_item *items", "bpg_status *status_out"]
    assert proto("bpg_test_template_eval_batch") == ["const bpg_r1cs_instance *inst", "const bpg_witness_program *program", "uint64_t count", "const uint8_t *v",
                                                     "uint8_t *aL_out", "uint8_t *aR_out", "uint8_t *aO_out"]
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_prove_template_batch", "bpg_test_template_eval_batch"))
