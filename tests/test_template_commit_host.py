"""Template batches that make their own commitments, without a GPU: the append step of bpg_r1cs_prove_template_batch_commit alone
(bpg_test_append_commitments), the layout of the frozen bpg_template_commit_item, and the refusals of the call that need no device.

The yardstick of the append step is the mirror's Prover.commit_precomputed - Prover::commit with the commitment supplied - on the same encodings: the
state the library reaches from "as Prover::new leaves it" must be the state a prover that commits one value at a time reaches.

count = 0 returns BPG_OK on a real template only (a handle without device state is refused first, whatever else is passed - the rule of
bpg_r1cs_prove_template_batch): tests/test_template_commit_gpu.py checks it where a template exists."""
import ctypes as C
import hashlib
import re
import subprocess

import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
from test_template_host import StubProver, FAKE, _err

FIELDS = ("v", "param_values", "transcript_state", "v_blinding", "rng_seed", "flags", "proof_out", "proof_len", "commitments_out")


def encodings(m, tag="c"):
    """m distinct 32-byte strings: the transcript does not look inside an encoding"""
    return [hashlib.sha256(("%s %d" % (tag, j)).encode()).digest() for j in range(m)]


def append(state, coms):
    out = C.create_string_buffer(203)
    assert bpg.lib().bpg_test_append_commitments(state, C.c_uint64(len(coms)), b"".join(coms) if coms else None, out) == 0, _err()
    return out.raw[:203]


def mirror_state(label, coms):
    """(state as Prover::new leaves it, state after commit_precomputed of every encoding in order)"""
    t = bpg.Transcript(label); p = bpg.Prover(None, t)
    before = t.state
    for j, c in enumerate(coms):
        p.commit_precomputed(bpg.scalar_from_int(j + 1), bpg.scalar_from_int(100 + j), c)
    return before, t.state


@pytest.mark.parametrize("m", [0, 1, 3])
def test_append_step_equals_commit_precomputed(m):
    coms = encodings(m)
    before, after = mirror_state(b"BoundsCheck", coms)
    assert append(before, coms) == after
    assert (append(before, coms) == before) == (m == 0)                     # m = 0 appends nothing


def test_order_of_the_commitments_matters():
    coms = encodings(3)
    before, after = mirror_state(b"BoundsCheck", coms)
    swapped = [coms[1], coms[0], coms[2]]
    assert append(before, swapped) != after
    assert append(before, swapped) == mirror_state(b"BoundsCheck", swapped)[1]
    assert append(append(before, coms[:1]), coms[1:]) == after              # the appends compose
    assert mirror_state(b"other label", coms)[0] != before
    lib = bpg.lib()                                                          # NULL arguments
    out = C.create_string_buffer(203)
    assert lib.bpg_test_append_commitments(None, C.c_uint64(0), None, out) == 4
    assert lib.bpg_test_append_commitments(before, C.c_uint64(1), None, out) == 4
    assert lib.bpg_test_append_commitments(before, C.c_uint64(0), None, None) == 4


def test_template_commit_item_layout_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    offs = ", ".join("offsetof(bpg_template_commit_item, %s)" % f for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "bpg.h"\nint main(void) { printf("%u %zu' + " %zu" * len(FIELDS) +
                   '\\n", BPG_ABI_VERSION, sizeof(bpg_template_commit_item), ' + offs + '); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Werror", "-I", str(O.ROOT / "include"), "-o", str(exe), str(src)])
    want = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert want[0] == 7                                                     # an addition to ABI version 7: no bump
    assert [f for f, _ in bpg._TemplateCommitItem._fields_] == list(FIELDS)
    got = [C.sizeof(bpg._TemplateCommitItem)] + [getattr(bpg._TemplateCommitItem, f).offset for f in FIELDS]
    assert got == want[1:], (got, want)
    # the shared fields sit where bpg_template_item has them
    assert all(getattr(bpg._TemplateCommitItem, f).offset == getattr(bpg._TemplateItem, f).offset for f in FIELDS[:-1])
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    assert "bpg_template_commit_item" in re.search(r"or are frozen \(([^)]*)\)", hdr).group(1)    # listed with the frozen structs
    proto = lambda name: [x.strip() for x in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    assert proto("bpg_r1cs_prove_template_batch_commit") == ["bpg_ctx *ctx", "bpg_circuit *tmpl", "uint64_t count", "const bpg_template_commit_item *items",
                                                             "bpg_status *status_out"]
    assert proto("bpg_test_append_commitments") == ["const uint8_t state_in[BPG_TRANSCRIPT_STATE_BYTES]", "uint64_t m", "const uint8_t *coms",
                                                    "uint8_t state_out[BPG_TRANSCRIPT_STATE_BYTES]"]
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_prove_template_batch_commit", "bpg_test_append_commitments"))


def commit_items(res, items, sentinel=0xA5):
    """bpg_template_commit_item array over ResidentCircuit._template_items, every commitment buffer filled with a sentinel"""
    arr, keep = res._template_items(items, bpg._TemplateCommitItem)
    coms = [C.create_string_buffer(bytes([sentinel]) * (32 * res.m), 32 * res.m) for _ in items]
    for k in range(len(items)):
        arr[k].commitments_out = C.cast(coms[k], C.c_void_p)
    return arr, keep, coms


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
    state = bpg.Transcript(b"MiMCHash").state
    arr, keep, coms = commit_items(res, [(inst.v, [bytes(32)], state, inst.v_blinding, bytes(32), 0)] * 2)
    two = C.c_uint64(2)
    call = lib.bpg_r1cs_prove_template_batch_commit

    def untouched(status):
        return (list(status) == [77, 77] and all(k[0].raw[:203] == state and k[1].raw == bytes(len(k[1])) and k[2].value == len(k[1]) for k in keep)
                and all(c.raw == b"\xa5" * (32 * inst.m) for c in coms))
    try:
        status = (C.c_int32 * 2)(77, 77)
        assert call(None, tmpl, two, arr, status) == 4 and untouched(status)             # NULL ctx
        assert call(None, None, two, arr, status) == 4 and untouched(status)
        assert call(FAKE, None, two, arr, status) == 4 and untouched(status)             # NULL tmpl
        for h in (tmpl, plain):         # a handle without device state: refused whatever else is passed, before the device is touched
            assert call(FAKE, h, two, arr, status) == 4 and "no device state" in _err() and untouched(status)
            assert call(None, h, two, arr, status) == 4 and untouched(status)
            assert call(FAKE, h, two, None, status) == 4 and untouched(status)           # NULL items
            assert call(FAKE, h, two, arr, None) == 4 and untouched(status)              # NULL status_out
            assert call(FAKE, h, C.c_uint64(0), None, None) == 4                         # ... count = 0 included (BPG_OK needs a real template)
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)
