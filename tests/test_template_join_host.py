"""Templates joined into one circuit, without a GPU: the joined instance (bpg_test_template_join_instance), the join-layout witness interpreter compiled for
the host (bpg_test_template_eval_join), and the refusals of bpg_r1cs_template_join that need no device.

The yardstick is the EXISTING host assembly: ONE prover that commits and assembles the same gadget code part by part, item by item (`mixed_assembly`).  Its
exported instance is what the join must be, row by row - the non-constant terms as (variable, coefficient bytes) and the sum of the row's constant terms - and
its a_L, a_R, a_O are what the interpreter must give, byte for byte.  Every template is made from ONE item assembled alone under another seed, never from the
mixed assembly, and the join is never compared with itself.

Shapes (the smallest at which the map can go wrong): set3 (n = 6, no power of two, no parameter), bounds8 (n = 16, m = 3, bit hints, one level), merkle3
(((W W) W), n = 3,888, one parameter, three levels - two with the digests of its two nodes as checkpoints).  The mixed statement is
[(set3, 2), (bounds8, 65), (merkle3, 2)]: n' = 12 + 1,040 + 7,776 = 8,828; 65 is one item more than a block of the lane map holds."""
import ctypes as C
import re
import subprocess

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
from test_template_host import StubProver, FAKE, _err
from test_template_repeat_host import CIRCUITS, assemble, constant_term, row_view, sc, template_of

MIXED = [("set3", 2), ("bounds8", 65), ("merkle3", 2)]
PART_LISTS = {
    "mixed": MIXED,
    "reversed": MIXED[::-1],
    "one part": [("bounds8", 3)],
    "bounds8 twice": [("bounds8", 2), ("set3", 1), ("bounds8", 3)],
}


def mixed_assembly(parts, tag, prover_cls=StubProver, ctx=None):
    """ONE prover: part 0's gadget code count_0 times, then part 1's, ..., commits item by item -> (prover, transcript, parameter rows in order).
    Items of different parts that name one circuit get different witnesses (the tag carries the part)."""
    t = bpg.Transcript(b"MixedStatement")
    p = prover_cls(ctx, t)
    rows = []
    for k, (name, count) in enumerate(parts):
        for i in range(count):
            rows += CIRCUITS[name][0](p, "%s-part%d" % (tag, k), i)
    return p, t, rows


def merkle3_checkpoints():
    """the checkpoint Variables of the merkle3 template: the digests of its two nodes (the notes that close a node), in assembly order"""
    p, _, _ = assemble("merkle3", "tmpl", 1)
    cks = [var for var, _, last in p.noted() if last]
    assert len(cks) == 2
    return cks


def merkle3_checkpoint_values(v):
    """the two node digests of one ((W W) W) item from its three committed leaves alone (the native host sponge): v = 3 x 32 bytes"""
    inner = bpg.mimc_sponge([v[0:32], v[32:64]])
    return [inner, bpg.mimc_sponge([inner, v[64:96]])]


@pytest.fixture(scope="module")
def templates():
    return {name: template_of(name) for name in CIRCUITS}


@pytest.fixture(scope="module")
def assemblies():
    """the host assemblies, made once: name of the part list -> (instance, parameter values in order)"""
    out = {}
    for key, parts in PART_LISTS.items():
        p, _, rows = mixed_assembly(parts, "items")
        inst = p.instance()
        out[key] = (inst, [constant_term(inst, r) for r in rows])
    return out


def hook_parts(templates, parts, checkpoints=None):
    return [templates[name] + (count,) + ((checkpoints or {}).get(name),) for name, count in parts]


@pytest.mark.parametrize("key", list(PART_LISTS))
def test_instance_and_witness_equal_the_host_assembly(templates, assemblies, key):
    parts = PART_LISTS[key]
    want, params = assemblies[key]
    dims = [(templates[nm][0].n, templates[nm][0].m, templates[nm][0].q, len(templates[nm][1].param_rows), 0, c) for nm, c in parts]
    layout = bpg.join_layout(dims)
    tot = lambda k: sum(p["count"] * p[k] for p in layout)
    assert (want.n, want.q, want.m, len(params)) == (tot("n"), tot("q"), tot("m"), tot("n_params"))
    if key == "mixed":
        assert want.n == 8828 and [p["base_n"] for p in layout] == [0, 12, 1052]
    hp = hook_parts(templates, parts)
    row_ptr, tv, tc, coef = bpg.test_template_join_instance(hp, params)
    joined = [list(row_ptr), list(tv), list(tc), coef]
    assert len(row_ptr) == want.q + 1 and row_ptr[0] == 0 and int(row_ptr[-1]) == len(tv) == len(tc)
    assert len(coef) == 32 * (sum(templates[nm][0].ncoef for nm, _ in parts) + tot("n_params"))
    for r in range(want.q):
        (gt, gc), (wt, wc) = row_view(row_ptr, tv, tc, coef, r), row_view(want.row_ptr, want.term_var, want.term_coef, want.coef, r)
        assert (sorted(gt), gc) == (sorted(wt), wc), "row %d: %r" % (r, bpg._join_place(layout, r, "q"))
    # the witness: the join-layout interpreter against the host assembly's own vectors
    aL, aR, aO, first = bpg.test_template_eval_join(hp, want.v)
    assert first is None
    for p, part in enumerate(layout):
        for k in range(part["count"]):
            a, b = 32 * (part["base_n"] + k * part["n"]), 32 * (part["base_n"] + (k + 1) * part["n"])
            for nm, x, y in (("a_L", aL, want.aL), ("a_R", aR, want.aR), ("a_O", aO, want.aO)):
                assert x[a:b] == y[a:b], "%s of item %d of part %d" % (nm, k, p)
    assert (aL, aR, aO) == (want.aL, want.aR, want.aO)
    # ... and the oracle on the hook's instance with the hook's witness
    assert O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, row_ptr, tv, tc, coef), want.v)
    if params:                                               # a wrong parameter in the LAST slot alone: that item's row no longer holds
        bad = params[:-1] + [sc(int.from_bytes(params[-1], "little") + 1)]
        row_ptr, tv, tc, coef = bpg.test_template_join_instance(hp, bad)
        assert not O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, row_ptr, tv, tc, coef), want.v)
    if len(parts) == 1:                                      # a join of one part is the repeat, hook for hook
        tinst, prog, hints = templates[parts[0][0]]
        rep = bpg.test_template_repeat_instance(tinst, prog, hints, parts[0][1], params)
        assert [list(x) for x in rep[:3]] + [rep[3]] == joined
        assert bpg.test_template_eval_repeat(tinst, prog, hints, parts[0][1], want.v) == (aL, aR, aO)


def test_parameter_slots_without_values_keep_the_templates_constants(templates):
    """param_values NULL: every copy's slot holds the constant its template's own row carried; the slots are one range behind ALL shared coefficients"""
    parts = [("merkle3", 2), ("set3", 1), ("merkle3", 1)]
    tinst, prog, _ = templates["merkle3"]
    row_ptr, tv, tc, coef = bpg.test_template_join_instance(hook_parts(templates, parts))
    shared = 2 * tinst.ncoef + templates["set3"][0].ncoef
    assert len(coef) == 32 * (shared + 3)
    root = constant_term(tinst, prog.param_rows[0])
    qs = templates["set3"][0].q
    for slot, first_row in enumerate((0, tinst.q, 2 * tinst.q + qs)):
        r = first_row + prog.param_rows[0]
        assert sc(row_view(row_ptr, tv, tc, coef, r)[1]) == root
        assert int(tc[int(row_ptr[r + 1]) - 1]) == shared + slot, "slot %d" % slot


def test_checkpointed_part_beside_a_plain_one(templates):
    parts = [("bounds8", 3), ("merkle3", 2)]
    p, _, _ = mixed_assembly(parts, "ck")
    want = p.instance()
    cks = merkle3_checkpoints()
    hp = hook_parts(templates, parts, {"merkle3": cks})
    m0 = 3 * templates["bounds8"][0].m
    values = []
    for k in range(2):
        values += merkle3_checkpoint_values(want.v[32 * (m0 + 3 * k):32 * (m0 + 3 * k + 3)])
    assert len(set(values)) == 4
    plain = bpg.test_template_eval_join(hook_parts(templates, parts), want.v)
    assert plain == (want.aL, want.aR, want.aO, None)
    assert bpg.test_template_eval_join(hp, want.v, values) == plain
    # the values are the circuit's own at the named variables of each item, and came from the sponge alone
    n0, n1 = 3 * 16, 3888
    for k in range(2):
        for c, var in enumerate(cks):
            at = 32 * (n0 + k * n1 + var.index)
            assert var.kind == 2 and want.aO[at:at + 32] == values[2 * k + c]
    # a wrong value in item 1: the flat index in the JOINED list (bounds8 has none: the part's base is 0), whichever of its two it is
    for c in (0, 1):
        bad = list(values); bad[2 + c] = sc(int.from_bytes(bad[2 + c], "little") + 1)
        assert bpg.test_template_eval_join(hp, want.v, bad)[3] == 2 + c
    bad = list(values); bad[1] = bytes(32); bad[3] = bytes(32)
    assert bpg.test_template_eval_join(hp, want.v, bad)[3] == 1, "the LOWEST mismatch"
    with pytest.raises(bpg.BpgError) as e:                      # checkpoints and no values
        bpg.test_template_eval_join(hp, want.v)
    assert e.value.status == 4 and "checkpoints" in str(e.value)
    # the checkpointed part first: its base is 0 and the plain part behind it shifts nothing
    parts2 = parts[::-1]
    p2, _, _ = mixed_assembly(parts2, "ck2")
    w2 = p2.instance()
    v2 = []
    for k in range(2):
        v2 += merkle3_checkpoint_values(w2.v[32 * 3 * k:32 * (3 * k + 3)])
    hp2 = hook_parts(templates, parts2, {"merkle3": cks})
    assert bpg.test_template_eval_join(hp2, w2.v, v2) == (w2.aL, w2.aR, w2.aO, None)
    bad = list(v2); bad[3] = bytes(32)
    assert bpg.test_template_eval_join(hp2, w2.v, bad)[3] == 3


def test_refusals_need_no_device(templates):
    lib = bpg.lib()
    tinst, prog, hints = templates["bounds8"]
    cs, cp, ch = tinst.cstruct(), prog.cstruct(), hints.cstruct()
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle_hinted(C.byref(cs), C.byref(cp), C.byref(ch), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 0, _err()
    try:
        def refused(word, ctx, parts, n_parts=None, out=True):
            arr = None
            if parts is not None:
                arr = (bpg.TemplatePart * max(len(parts), 1))()
                for k, (t, c) in enumerate(parts):
                    arr[k].tmpl, arr[k].count = t, c
            h = C.c_void_p(7)
            n = len(parts) if n_parts is None else n_parts
            assert lib.bpg_r1cs_template_join(ctx, C.c_uint64(n), arr, C.byref(h) if out else None) == 4, _err()
            assert word in _err(), _err()
            assert not out or not h.value
        good = (tmpl, 2)
        refused("null", FAKE, [good], out=False)
        refused("null", None, [good])
        refused("null", FAKE, None, n_parts=1)
        refused("at least 1", FAKE, [], n_parts=0)
        refused("at most 256", FAKE, [good] * 257)
        # (a handle made without a device is refused as such where it stands in the list: the part at fault comes first here, and the GPU test names later ones)
        refused("part 0: null", FAKE, [(None, 2), good])
        refused("part 0: count must be at least 1", FAKE, [(tmpl, 0), good])
        refused("part 0: the circuit is not a template", FAKE, [(plain, 2), good])
        refused("part 0: the handle has no device state", FAKE, [good])
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)
    # the size limits, through the hooks (the same check the device path starts with): n = 16 -> 2^23 copies reach 2^27 multipliers; the TOTAL counts
    b8, s3 = templates["bounds8"], templates["set3"]
    out, first = C.create_string_buffer(32), C.c_uint64()
    for parts, word in (([b8 + (0,)], "part 0: count must be at least 1"),
                        ([s3 + (1,), b8 + (1 << 23,)], "part 1: the joined multipliers"),
                        ([b8 + ((1 << 22) + 1,), s3 + (5,), b8 + ((1 << 22) - 2,)], "part 2: the joined multipliers"),     # each part fits: the TOTAL does not
                        ([b8 + ((1 << 64) - 1,)], "part 0: the joined multipliers"),
                        ([s3 + (1,)] * 257, "at most 256"),
                        ([], "at least 1")):
        arr, keep, _ = bpg._test_join_parts(parts)
        rc = lib.bpg_test_template_eval_join(C.c_uint64(len(parts)), arr, bytes(32), None, out, out, out, C.byref(first))
        assert rc == 4 and word in _err(), (word, _err())
        assert out.raw == bytes(32), "a refused call wrote into a buffer"


def synthetic(m, rows, param_rows=(), pad=0, empty=0):
    """the smallest template a count can drive over ONE limit while the other totals stay inside: one multiplier (v_0 * v_0: a program needs one), m
    committed values, `rows` constraints v_0 + ... + v_{m-1} - constant each, and `pad` more with constants of their own (a coefficient each)
    and `empty` without any term -> (instance, program, hints); param_rows index the `rows` constraints"""
    p = StubProver(None, bpg.Transcript(b"Synthetic"))
    vs = p.commit_many([sc(3 + i) for i in range(m)], [sc(100 + i) for i in range(m)])[1]
    p.multiply(bpg.LinearCombination.of(vs[0]), bpg.LinearCombination.of(vs[0]))
    first, total = p.num_constraints(), sum(3 + i for i in range(m))
    for r in range(rows + pad):
        lc = bpg.LinearCombination.of(vs[0])
        for v in vs[1:]:
            lc = lc + v
        p.constrain(lc - sc(total if r < rows else 1000 + r))
    for _ in range(empty):                                  # rows without a term: constraints that cost no entry
        p.constrain(bpg.LinearCombination.of(0))
    prog, hints = p.witness_program(hints=True)
    prog.param_rows = prog.param_rows + [first + r for r in param_rows]
    return p.instance(), prog, hints


def test_every_total_has_its_limit():
    """m' >= 2^29, q' >= 2^32, nnz' >= 2^32 and 2^30 coefficient slots, each reached alone through the hooks (the check the device path starts with), by
    whichever part takes the total over.  The column limit (3 n' + m' + 1 < 2^32) cannot be reached while n' < 2^27 and m' < 2^29 hold, and the refusal of a
    part on another context's device needs two devices: neither is exercised."""
    lib = bpg.lib()
    out, first = C.create_string_buffer(32), C.c_uint64()
    up = lambda limit, a: -(-limit // a)                    # the fewest copies of `a` apiece that reach the limit
    tm, tq, tn, ts = synthetic(8, 1), synthetic(1, 1, empty=64), synthetic(4, 8), synthetic(1, 16, param_rows=range(16))
    cases = ((tm, up(1 << 29, tm[0].m), "the joined committed values"),                          # 2^26 copies: n' = 2^26
             (tq, up(1 << 32, tq[0].q), "the joined constraints"),                                # 67 rows and 6 terms a copy: n' = m' = 6.4e7
             (tn, up(1 << 32, tn[0].nnz), "the joined terms"),                                    # about 40 terms a copy: n' = 1.1e8, m' = 4.3e8, q' = 1.1e9
             (ts, up((1 << 30) - ts[0].ncoef, 16), "the joined coefficient slots"))               # 2^26 copies: n' = m' = 2^26, q' = 18 x 2^26, nnz' = 36 x 2^26
    one = synthetic(1, 1)
    for tmpl, count, word in cases:
        lists = [([tmpl + (count,)], 0), ([one + (1,), tmpl + (count,)], 1), ([tmpl + (count - 2,), one + (1,), tmpl + (2,)], 2)]
        if word == "the joined constraints":                # every row holds a term or more, so count - 2 copies are over the TERM limit already: the part
            lists.pop()                                     # that brings too many rows brings them at once here (rows are looked at before terms)
        for parts, at in lists:
            arr, keep, _ = bpg._test_join_parts(parts)
            rc = lib.bpg_test_template_eval_join(C.c_uint64(len(parts)), arr, bytes(32), None, out, out, out, C.byref(first))
            assert rc == 4 and "part %d: %s" % (at, word) in _err(), (word, at, _err())
            assert out.raw == bytes(32)
    # the slot bound is the repeat's, to the slot: shared + count x n_params = 2^30 EXACTLY (one more than the largest index a record can name) is refused by
    # both.  13 constants of their own make the shared table 16 coefficients, so that 16 slots a copy reach 2^30 on the dot.
    inst, prog, hints = synthetic(1, 16, param_rows=range(16), pad=13)
    assert inst.ncoef == 16 and len(prog.param_rows) == 16
    count = ((1 << 30) - inst.ncoef) // 16
    cs, cp = inst.cstruct(), prog.cstruct()
    arr, keep, _ = bpg._test_join_parts([(inst, prog, hints, count)])
    assert lib.bpg_test_template_eval_join(C.c_uint64(1), arr, bytes(32), None, out, out, out, C.byref(first)) == 4 and "part 0: the joined coefficient slots" in _err(), _err()
    assert lib.bpg_test_template_eval_repeat(C.byref(cs), C.byref(cp), None, C.c_uint64(count), bytes(32), out, out, out) == 4 and "coefficient slots" in _err(), _err()


def test_layout_and_report_mapping():
    layout = bpg.join_layout([(6, 3, 10, 0, 0, 2), (16, 3, 20, 0, 0, 65), (3888, 3, 4000, 1, 2, 2)])
    assert [(p["base_n"], p["base_m"], p["base_q"], p["base_n_params"], p["base_n_ck"]) for p in layout] == [(0, 0, 0, 0, 0), (12, 6, 20, 0, 0), (1052, 201, 1320, 0, 0)]
    view = bpg.CheckReportView(1, 12 + 64 * 16 + 5, 3, 19)
    rep = bpg.CheckReport(view, [19, 20 + 64 * 20 + 7, 1320 + 4000 + 1])
    assert rep.parts(layout) == [(0, 1, 9), (1, 64, 7), (2, 1, 1)]
    assert rep.multiplier_part(layout) == (1, 64, 5)
    assert bpg._join_place(layout, 3, "n_ck") == (2, 1, 1)
    with pytest.raises(IndexError):
        bpg._join_place(layout, 1320 + 8000, "q")


def test_index_map_and_interpreter_under_the_sanitizers(tmp_path):
    """tests/hostcheck/template_join.cpp: join_map, the entry positions and the join-layout interpreter of hip/k_join.cuh through the host compiler under ASan
    and UBSan (a stand-alone program: no preload, no device), on buffers of exactly the sizes the formulas give"""
    exe = tmp_path / "template_join"
    src = O.ROOT / "tests" / "hostcheck" / "template_join.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.split()[-1] == "ok"


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [" ".join(a.split()) for a in re.search(r"bpg_status %s\(([^)]*)\);" % name, hdr).group(1).split(",")]
    assert proto("bpg_r1cs_template_join") == ["bpg_ctx *ctx", "uint64_t n_parts", "const bpg_template_part *parts", "bpg_circuit **out"]
    assert re.search(r"typedef struct \{ bpg_circuit \*tmpl; uint64_t count; \} bpg_template_part;", hdr)
    assert [(n, t) for n, t in bpg.TemplatePart._fields_] == [("tmpl", C.c_void_p), ("count", C.c_uint64)] and C.sizeof(bpg.TemplatePart) == 16
    head = ["uint64_t n_parts", "const bpg_test_join_part *parts"]
    assert proto("bpg_test_template_join_instance") == head + ["const uint8_t *param_values", "uint64_t *row_ptr", "uint64_t row_cap", "uint32_t *term_var",
                                                               "uint32_t *term_coef", "uint64_t term_cap", "uint8_t *coef", "uint64_t coef_cap", "uint64_t *nnz_out",
                                                               "uint64_t *ncoef_out"]
    assert proto("bpg_test_template_eval_join") == head + ["const uint8_t *v", "const uint8_t *ck_values", "uint8_t *aL_out", "uint8_t *aR_out", "uint8_t *aO_out",
                                                           "uint64_t *first_mismatch"]
    fields = re.search(r"typedef struct \{([^}]*)\} bpg_test_join_part;", hdr).group(1)
    assert [" ".join(f.split()).split("*")[-1].split()[-1] for f in fields.split(";") if f.strip()] == [n for n, _ in bpg.TestJoinPart._fields_]
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_template_join", "bpg_test_template_join_instance", "bpg_test_template_eval_join"))
    assert hasattr(bpg.Context, "join") and hasattr(bpg.CheckReport, "parts")
    assert "a circuit that is itself a repeat or a join" in " ".join(hdr.split()).replace(" * ", " ")      # bpg_r1cs_template_repeat refuses a join
