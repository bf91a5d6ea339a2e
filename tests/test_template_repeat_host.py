"""A template repeated K times, without a GPU: the repeated instance (bpg_test_template_repeat_instance), the repeat-layout witness interpreter compiled
for the host (bpg_test_template_eval_repeat), and the refusals of bpg_r1cs_template_repeat that need no device.

The yardstick is the EXISTING host assembly: ONE prover that commits item by item and assembles the same gadget code K times.  Its exported instance is
what the repeat must be, row by row - the non-constant terms in order as (variable, coefficient bytes), and the sum of the row's constant terms (a
parameter row of the template carries them as one term on a slot of its own) - and its a_L, a_R, a_O are what the interpreter must give, byte for byte.
The oracle's orc_r1cs_satisfied then judges the hook's instance with the hook's witness.  The template is always made from ONE item assembled alone (item
0 of another seed), never from the K-fold assembly.

Templates: an 8-bit BoundsCheck (n = 16, every multiplier a bit hint, 2 segments), SetMembership over two committed elements and one instance element
(n = 6: no power of two, so item k sits at 6 k where a wave layout would put it at 8 k; 4 segments), and the Merkle pattern ((W W) W) with the root row
as a parameter (n = 3888, four absorbed blocks on three levels)."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads
import oracle_lib as O
from test_template_host import StubProver, FAKE, _err

L = bpg.L
sc = lambda x: (x % L).to_bytes(32, "little")
KS = [1, 2, 3]


# ---- the three gadget codes: item(p, tag, k) commits item k's values on prover p and assembles the gadget; returns the rows that are parameters
def bounds8_values(tag, k):
    w = workloads.synth("rep-b8-%s" % tag, k, 1)
    return w


def bounds8_item(p, tag, k, values=None):
    g = bpg.BoundsCheck(b"\x00", b"\xff")
    if values is None:
        scalars, _, wvars = bpg.commit(p, bounds8_values(tag, k), [workloads.blinding("rep-b8-%s-%d" % (tag, k), 0)])
        _, derived = g.setup(p, scalars, [workloads.blinding("rep-b8-%s-%d" % (tag, k), 1 + i) for i in range(2)])
    else:                                                   # any three committed values (witness, a, b): an out-of-range witness
        _, vs = p.commit_many(values, [workloads.blinding("rep-b8-%s-%d" % (tag, k), i) for i in range(3)])
        wvars, derived = vs[:1], [(values[1], vs[1]), (values[2], vs[2])]
    g.prove(p, wvars, derived)
    return []


SET_INSTANCE = [bpg.be_to_scalar(b"\x11")]


def set3_item(p, tag, k):
    """the member is element k mod 3 of (two committed elements, one instance element)"""
    cfg = "rep-set-%s-%d" % (tag, k)
    wit = [b"\x21" + workloads.synth(cfg, i, 8) for i in range(2)]
    member = (wit + [b"\x11"])[k % 3]
    ms, _, mv = bpg.commit_single(p, member, workloads.blinding(cfg, 0))
    ws, _, wv = bpg.commit_all_single(p, wit, [workloads.blinding(cfg, 1), workloads.blinding(cfg, 2)])
    g = bpg.SetMembership(mv, ms, SET_INSTANCE, SET_INSTANCE)
    _, dw = g.setup(p, ws, [workloads.blinding(cfg, 3 + i) for i in range(3)])
    g.prove(p, wv, dw)
    return []


def merkle3_item(p, tag, k):
    cfg = "rep-mk-%s-%d" % (tag, k)
    leaves = [b"\x03" + workloads.synth(cfg, i, 31) for i in range(3)]
    _, _, vs = bpg.commit_all_single(p, leaves, [workloads.blinding(cfg, i) for i in range(3)])
    probe = bpg.Prover(None, bpg.Transcript(b"probe"))
    bpg.MerkleTree256(bytes(32), [bpg.be_to_scalar(x) for x in leaves], [], "((I I) I)").prove(probe, [], [])
    bpg.MerkleTree256(probe.instance().aO[-32:], [], bpg.vars_to_lc(vs), "((W W) W)").prove(p, [], [])
    return [p.num_constraints() - 1]


CIRCUITS = {"bounds8": (bounds8_item, b"BoundsCheck", 16), "set3": (set3_item, b"SetMembership", 6), "merkle3": (merkle3_item, b"MerkleTree", 3888)}


def assemble(name, tag, K, prover_cls=StubProver, ctx=None):
    """ONE prover, the gadget code K times, commits item by item -> (prover, transcript, parameter rows in item order)"""
    item, label, _ = CIRCUITS[name]
    t = bpg.Transcript(label)
    p = prover_cls(ctx, t)
    rows = []
    for k in range(K):
        rows += item(p, tag, k)
    return p, t, rows


def template_of(name, tag="tmpl"):
    """(instance, program with its parameter rows, hints) of the gadget code assembled ONCE"""
    p, _, rows = assemble(name, tag, 1)
    prog, hints = p.witness_program(hints=True)
    prog.param_rows = prog.param_rows + rows
    return p.instance(), prog, hints


def row_view(row_ptr, term_var, term_coef, coef, r):
    """(the non-constant terms in order as (variable, coefficient bytes), the sum of the constant terms)"""
    terms, const = [], 0
    for t in range(int(row_ptr[r]), int(row_ptr[r + 1])):
        c = coef[32 * int(term_coef[t]):32 * int(term_coef[t]) + 32]
        if int(term_var[t]) >> 29 == 4:
            const += int.from_bytes(c, "little")
        else:
            terms.append((int(term_var[t]), c))
    return terms, const % L


def constant_term(inst, row):
    return sc(row_view(inst.row_ptr, inst.term_var, inst.term_coef, inst.coef, row)[1])


@pytest.fixture(scope="module")
def templates():
    return {name: template_of(name) for name in CIRCUITS}


@pytest.fixture(scope="module")
def assemblies():
    """the K-fold host assemblies, made once: name -> K -> (instance, parameter values in item order)"""
    out = {}
    for name in CIRCUITS:
        out[name] = {}
        for K in KS:
            p, _, rows = assemble(name, "items", K)
            inst = p.instance()
            out[name][K] = (inst, [constant_term(inst, r) for r in rows])
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", list(CIRCUITS))
def test_instance_and_witness_equal_the_host_assembly(templates, assemblies, name, K):
    tinst, prog, hints = templates[name]
    want, params = assemblies[name][K]
    n = CIRCUITS[name][2]
    assert tinst.n == n and (want.n, want.q, want.m) == (K * tinst.n, K * tinst.q, K * tinst.m) and len(params) == K * len(prog.param_rows)
    row_ptr, tv, tc, coef = bpg.test_template_repeat_instance(tinst, prog, hints, K, params)
    assert len(row_ptr) == want.q + 1 and row_ptr[0] == 0 and int(row_ptr[-1]) == len(tv) == len(tc)
    assert len(coef) == 32 * (tinst.ncoef + K * len(prog.param_rows))
    for r in range(want.q):
        got, exp = row_view(row_ptr, tv, tc, coef, r), row_view(want.row_ptr, want.term_var, want.term_coef, want.coef, r)
        assert got == exp, "row %d (row %d of item %d)" % (r, r % tinst.q, r // tinst.q)
    # the witness: the repeat-layout interpreter against the host assembly's own vectors
    aL, aR, aO = bpg.test_template_eval_repeat(tinst, prog, hints, K, want.v)
    for k in range(K):
        for nm, a, b in (("a_L", aL, want.aL), ("a_R", aR, want.aR), ("a_O", aO, want.aO)):
            assert a[32 * n * k:32 * n * (k + 1)] == b[32 * n * k:32 * n * (k + 1)], "%s of item %d" % (nm, k)
    assert (aL, aR, aO) == (want.aL, want.aR, want.aO)
    # ... and the oracle on the hook's instance with the hook's witness
    assert O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, row_ptr, tv, tc, coef), want.v)
    if params:                                               # a wrong parameter in the LAST item alone: that item's row no longer holds
        bad = params[:-1] + [sc(int.from_bytes(params[-1], "little") + 1)]
        row_ptr, tv, tc, coef = bpg.test_template_repeat_instance(tinst, prog, hints, K, bad)
        assert not O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, row_ptr, tv, tc, coef), want.v)


def test_parameter_slots_without_values_keep_the_templates_constants(templates):
    """param_values NULL: every copy's slot holds the constant the template's own row carried"""
    tinst, prog, hints = templates["merkle3"]
    row_ptr, tv, tc, coef = bpg.test_template_repeat_instance(tinst, prog, hints, 2)
    root = constant_term(tinst, prog.param_rows[0])
    for k in range(2):
        r = k * tinst.q + prog.param_rows[0]
        assert sc(row_view(row_ptr, tv, tc, coef, r)[1]) == root
        assert int(tc[int(row_ptr[r + 1]) - 1]) == tinst.ncoef + k, "the slot of item %d" % k


def test_out_of_range_item_gives_the_hosts_witness(templates):
    """bits above bit 7 are ignored by the host and by the interpreter alike: item 2 alone holds a = 2^8 + 5"""
    tinst, prog, hints = templates["bounds8"]
    a = (1 << 8) + 5
    t = bpg.Transcript(b"BoundsCheck"); p = StubProver(None, t)
    for k in range(3):
        bounds8_item(p, "oob", k, [sc(7), sc(a), sc(255 - a)] if k == 2 else None)
    want = p.instance()
    assert bpg.test_template_eval_repeat(tinst, prog, hints, 3, want.v) == (want.aL, want.aR, want.aO)
    row_ptr, tv, tc, coef = bpg.test_template_repeat_instance(tinst, prog, hints, 3)
    assert not O.satisfied(O.FlatCircuit(want.n, want.m, want.aL, want.aR, want.aO, row_ptr, tv, tc, coef), want.v)


def test_refusals_need_no_device(templates):
    lib = bpg.lib()
    tinst, prog, hints = templates["bounds8"]
    cs, cp, ch = tinst.cstruct(), prog.cstruct(), hints.cstruct()
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(cp), C.byref(ch), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 0, _err()
    try:
        def refused(word, ctx, c, count, out=True):
            h = C.c_void_p(7)
            assert lib.bpg_r1cs_template_repeat(ctx, c, C.c_uint64(count), C.byref(h) if out else None) == 4, _err()
            assert word in _err(), _err()
            assert not out or not h.value
        refused("null", FAKE, tmpl, 2, out=False)
        refused("null", None, tmpl, 2)
        refused("null", FAKE, None, 2)
        refused("at least 1", FAKE, tmpl, 0)
        refused("not a template", FAKE, plain, 2)
        refused("no device state", FAKE, tmpl, 2)
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)
    # the size limits, through the hooks (the same check the device path starts with): n = 16 -> 2^23 copies reach 2^27 multipliers
    with pytest.raises(bpg.BpgError) as e:
        bpg.test_template_eval_repeat(tinst, prog, hints, 0, b"")
    assert e.value.status == 4 and "at least 1" in str(e.value)
    out = C.create_string_buffer(32)
    for count, word in ((1 << 23, "multipliers"), (1 << 60, "multipliers"), ((1 << 64) - 1, "multipliers")):
        rc = lib.bpg_test_template_eval_repeat(C.byref(cs), C.byref(cp), C.byref(ch), C.c_uint64(count), bytes(32), out, out, out)
        assert rc == 4 and word in _err(), (count, _err())
    # short buffers are named
    need = bpg.test_template_repeat_instance(tinst, prog, hints, 2)
    rows, terms, ncoef = len(need[0]), len(need[1]), len(need[3]) // 32
    bufs = lambda: (np.zeros(rows, np.uint64), np.zeros(terms, np.uint32), np.zeros(terms, np.uint32), C.create_string_buffer(32 * ncoef))
    for short, word in (((1, 0, 0), "row_ptr"), ((0, 1, 0), "term_var"), ((0, 0, 1), "coef")):
        rp, tv, tc, cf = bufs()
        nnz, nc = C.c_uint64(), C.c_uint64()
        rc = lib.bpg_test_template_repeat_instance(C.byref(cs), C.byref(cp), C.byref(ch), C.c_uint64(2), None, C.c_void_p(rp.ctypes.data), C.c_uint64(rows - short[0]),
                                                   C.c_void_p(tv.ctypes.data), C.c_void_p(tc.ctypes.data), C.c_uint64(terms - short[1]), cf, C.c_uint64(ncoef - short[2]),
                                                   C.byref(nnz), C.byref(nc))
        assert rc == 4 and word in _err() and "too short" in _err(), _err()
        assert not rp.any() and not tv.any() and cf.raw == bytes(32 * ncoef), "a refused call wrote into a buffer"


def test_index_map_and_interpreter_under_the_sanitizers(tmp_path):
    """tests/hostcheck/template_repeat.cpp: repeat_map and the repeat-layout interpreter of hip/k_repeat.cuh through the host compiler under ASan and UBSan (a
    stand-alone program: no preload, no device), on buffers of exactly the sizes the formulas give"""
    exe = tmp_path / "template_repeat"
    src = O.ROOT / "tests" / "hostcheck" / "template_repeat.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.split()[-1] == "ok"


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [a.strip() for a in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    assert proto("bpg_r1cs_template_repeat") == ["bpg_ctx *ctx", "bpg_circuit *tmpl", "uint64_t count", "bpg_circuit **out"]
    head = ["const bpg_r1cs_instance *inst", "const bpg_witness_program *program", "const bpg_witness_hints *hints", "uint64_t count"]
    assert proto("bpg_test_template_repeat_instance") == head + ["const uint8_t *param_values", "uint64_t *row_ptr", "uint64_t row_cap", "uint32_t *term_var",
                                                                 "uint32_t *term_coef", "uint64_t term_cap", "uint8_t *coef", "uint64_t coef_cap", "uint64_t *nnz_out",
                                                                 "uint64_t *ncoef_out"]
    assert proto("bpg_test_template_eval_repeat") == head + ["const uint8_t *v", "uint8_t *aL_out", "uint8_t *aR_out", "uint8_t *aO_out"]
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_template_repeat", "bpg_test_template_repeat_instance", "bpg_test_template_eval_repeat"))
    assert hasattr(bpg.ResidentCircuit, "repeat")
