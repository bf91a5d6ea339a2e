"""Public inputs through repeat and join, without a GPU: the repeated and joined instances with their derived coefficient slots
(bpg_test_template_repeat_inputs_instance, bpg_test_template_join_inputs_instance), the repeat- and join-layout interpreters with per-item inputs compiled for
the host (bpg_test_template_eval_repeat_inputs, bpg_test_template_eval_join_inputs: poisoned vectors, reverse order within a level) and the refusals of
bpg_r1cs_template_repeat_inputs, bpg_r1cs_template_join_inputs and bpg_r1cs_set_inputs that need no device.

The yardstick (repeat_inputs_cases.Assembly, as_inputs=False) is ONE prover that assembles the gadget code K times with the public values baked in as
constants: its exported instance is what the hook's rows must be, row by row (test_template_repeat_host.row_view: the non-constant terms in order, the sum
of the constant terms mod l), its a_L, a_R, a_O what the interpreter must give byte for byte, and the oracle's orc_r1cs_satisfied judges the hook's instance
with the hook's witness.  The template always comes from one item of another seed, assembled with as_inputs=True."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import repeat_inputs_cases as RC
from repeat_inputs_cases import sc, L
from test_template_repeat_host import row_view
from test_template_host import FAKE, _err

KS = [1, 2, 3]
GADGETS = ["inequality", "set4", "less_than", "merkle_wi"]
RANDOM = [("random", s) for s in RC.RANDOM_SEEDS.values()]
ident = lambda name: name if isinstance(name, str) else "%s%d" % name
JOINS = {
    "with2_without3_with1": [("inequality", 2), (("plain", 2), 3), ("set4", 1)],
    "same_template_twice": [(("random", 1), 2), ("inequality", 1), (("random", 1), 1)],
    "a_part_with_m_0": [("set4", 1), (("random", 50), 2), (("random", 4), 2)],
}


def args_of(name, count, first=0):
    return list(range(first, first + count)) if isinstance(name, tuple) else RC.ARGS[name][first:first + count]


@pytest.fixture(scope="module")
def templates():
    cache = {}

    def get(name):
        if name not in cache:
            a = RC.template_of(name)
            inst, prog, hints, cks, n_in = RC.template_parts(a)
            cache[name] = (inst, prog, hints, cks, n_in, len(RC.input_pairs(inst)[0]))
        return cache[name]
    return get


def same_rows(got, want, q):
    row_ptr, tv, tc, coef = got
    assert len(row_ptr) == q + 1 and row_ptr[0] == 0 and int(row_ptr[-1]) == len(tv) == len(tc)
    for r in range(q):
        assert row_view(row_ptr, tv, tc, coef, r) == row_view(want.row_ptr, want.term_var, want.term_coef, want.coef, r), "row %d" % r


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", GADGETS + RANDOM, ids=ident)
def test_repeat_equals_the_host_assembly_with_constants(templates, name, K):
    tinst, prog, hints, cks, n_in, n_slots = templates(name)
    a = RC.Assembly([(name, args_of(name, K))], False)
    want = a.instance()
    assert (want.n, want.q, want.m) == (K * tinst.n, K * tinst.q, K * tinst.m) and len(a.inputs) == K * n_in and n_in > 0
    assert len(a.params) == K * len(prog.param_rows) and len(a.ck_values) == K * len(cks)
    got = bpg.test_template_repeat_inputs_instance(tinst, prog, hints, n_in, K, a.params or None, a.inputs, n_slots=n_slots)
    assert len(got[3]) == 32 * (tinst.ncoef + K * (len(prog.param_rows) + n_slots))
    same_rows(got, want, want.q)
    # every input term of item k is a constant term on item k's derived slot: [shared | K n_params | K n_slots]
    first = tinst.ncoef + K * len(prog.param_rows)
    named = [set() for _ in range(K)]
    for r in range(want.q):
        for t in range(int(got[0][r]), int(got[0][r + 1])):
            assert int(got[1][t]) >> 29 != bpg.VAR_INPUT
            if int(got[2][t]) >= first:
                assert int(got[1][t]) >> 29 == bpg.VAR_ONE
                named[r // tinst.q].add(int(got[2][t]))
    assert named == [set(range(first + k * n_slots, first + (k + 1) * n_slots)) for k in range(K)]
    aL, aR, aO, mismatch = bpg.test_template_eval_repeat_inputs(tinst, prog, hints, cks, n_in, K, want.v, a.ck_values or None, a.inputs)
    assert mismatch is None
    n = tinst.n
    for k in range(K):
        for nm, x, y in (("a_L", aL, want.aL), ("a_R", aR, want.aR), ("a_O", aO, want.aO)):
            assert x[32 * n * k:32 * n * (k + 1)] == y[32 * n * k:32 * n * (k + 1)], "%s of item %d" % (nm, k)
    assert O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, *got), want.v)
    if n_slots:                                             # the LAST item's inputs changed: its rows, and only its derived slots, differ
        bad = a.inputs[:-n_in] + [sc(int.from_bytes(x, "little") + 1) for x in a.inputs[-n_in:]]
        other = bpg.test_template_repeat_inputs_instance(tinst, prog, hints, n_in, K, a.params or None, bad, n_slots=n_slots)
        assert other[3][:32 * (first + (K - 1) * n_slots)] == got[3][:32 * (first + (K - 1) * n_slots)] and other[3] != got[3]
        assert not O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, *other), want.v)
    if cks:                                                 # a wrong checkpoint in the last item: reported by its flat index
        _, _, _, mismatch = bpg.test_template_eval_repeat_inputs(tinst, prog, hints, cks, n_in, K, want.v, a.ck_values[:-1] + [sc(12345)], a.inputs)
        assert mismatch == K * len(cks) - 1


@pytest.mark.parametrize("prop", sorted(RC.RANDOM_SEEDS))
def test_pinned_random_shapes_keep_their_property(templates, prop):
    seed = RC.RANDOM_SEEDS[prop]
    a = RC.template_of(("random", seed))
    assert RC.shape_properties(a)[prop], "shape %d of the public family no longer has the property it was chosen for" % seed
    tinst, prog, hints, cks, n_in, n_slots = templates(("random", seed))
    assert n_in > 0 and (n_slots == 0) == (prop == "operands_only")


@pytest.mark.parametrize("join", sorted(JOINS))
def test_join_equals_the_host_assembly_with_constants(templates, join):
    spec = JOINS[join]
    seen, parts_args = {}, []
    for name, count in spec:                                # a template named twice gives its second part fresh items
        parts_args.append((name, args_of(name, count, seen.get(name, 0))))
        seen[name] = seen.get(name, 0) + count
    a = RC.Assembly(parts_args, False)
    want = a.instance()
    parts, n_slots = [], []
    for name, count in spec:
        tinst, prog, hints, cks, n_in, ns = templates(name) if name[0] != "plain" else plain_template(name)
        parts.append((tinst, prog, hints, count, cks, n_in))
        n_slots.append(ns)
    if join == "a_part_with_m_0":
        assert parts[1][0].m == 0
    layout = bpg.join_layout([(t.n, t.m, t.q, len(p.param_rows), len(ck), c, ni) for t, p, _, c, ck, ni in parts])
    assert [d["base_n_inputs"] for d in layout] == [sum(c * ni for _, _, _, c, _, ni in parts[:k]) for k in range(len(parts))]
    assert (want.n, want.m, want.q) == tuple(sum(d["count"] * d[k] for d in layout) for k in ("n", "m", "q"))
    assert len(a.inputs) == sum(d["count"] * d["n_inputs"] for d in layout)
    got = bpg.test_template_join_inputs_instance(parts, a.params or None, a.inputs or None, n_slots=n_slots)
    assert len(got[3]) == 32 * sum(t.ncoef + c * (len(p.param_rows) + ns) for (t, p, _, c, _, _), ns in zip(parts, n_slots))
    same_rows(got, want, want.q)
    aL, aR, aO, mismatch = bpg.test_template_eval_join_inputs(parts, want.v, a.ck_values or None, a.inputs or None)
    assert mismatch is None and (aL, aR, aO) == (want.aL, want.aR, want.aO)
    assert O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, *got), want.v)
    bad = [sc(int.from_bytes(x, "little") + 1) for x in a.inputs]
    other = bpg.test_template_join_inputs_instance(parts, a.params or None, bad, n_slots=n_slots)
    assert not O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, *other), want.v)


def plain_template(name):
    a = RC.Assembly([(name, [1000 + name[1]])], True, tag="tmpl")
    prog, hints = a.prover.witness_program(hints=True)
    assert not a.inputs
    return a.instance(), prog, hints, [], 0, 0


def test_join_layout_on_six_tuples_is_unchanged():
    dims = [(3, 2, 4, 1, 0, 2), (5, 0, 7, 0, 2, 3)]
    names = ("n", "m", "q", "n_params", "n_ck")
    out = bpg.join_layout(dims)
    assert out == [dict(zip(names + ("count",), dims[0]), **{"base_" + k: 0 for k in names}),
                   dict(zip(names + ("count",), dims[1]), base_n=6, base_m=4, base_q=8, base_n_params=2, base_n_ck=0)]
    seven = bpg.join_layout([d + (k + 1,) for k, d in enumerate(dims)])
    assert [(d["n_inputs"], d["base_n_inputs"]) for d in seven] == [(1, 0), (2, 2)]
    assert all({k: v for k, v in s.items() if "n_inputs" not in k} == o for s, o in zip(seven, out))


def hand_instance(n_inputs, n_coefs):
    """n = 1, m = 0, and one row over n_inputs public inputs, each under n_coefs different coefficients: the coefficient and input limits are the first a growing
    count meets (count n < 2^27 lies behind them once n_slots > 8 or n_inputs > 4)"""
    t = bpg.Transcript(b"hand"); p = RC.StubProver(None, t)
    one = bpg.LinearCombination.of(1)
    p.multiply(one, one)
    lc, total = bpg.LinearCombination.of(0), 0
    for i in range(n_inputs):
        x = bpg.LinearCombination.of(p.input(sc(5 + i)))
        for c in range(2, 2 + n_coefs):
            lc, total = lc + x * sc(c + 100 * i), total + (5 + i) * (c + 100 * i)
    p.constrain(lc - sc(total))
    return p


def test_refusals_need_no_device(templates):
    lib = bpg.lib()
    tinst, prog, hints, cks, n_in, n_slots = templates("inequality")
    cs, cp = tinst.cstruct(), prog.cstruct()
    cs.aL = cs.aR = cs.aO = None
    ch = hints.cstruct() if len(hints) else None
    tmpl, plain = C.c_void_p(), C.c_void_p()
    assert lib.bpg_test_circuit_handle_inputs(C.byref(cs), C.byref(cp), C.byref(ch) if ch is not None else None, None, C.c_uint64(n_in), C.byref(tmpl)) == 0, _err()
    assert lib.bpg_test_circuit_handle(C.byref(cs), None, C.byref(plain)) == 4          # (an instance with input terms is no plain circuit)
    pinst, pprog, phints = plain_template(("plain", 2))[:3]
    pcs, pcp, pch = pinst.cstruct(), pprog.cstruct(), phints.cstruct()
    assert lib.bpg_test_circuit_handle_hinted(C.byref(pcs), C.byref(pcp), C.byref(pch), C.byref(plain)) == 0, _err()
    try:
        def refused(call, word):
            assert call() == 4, _err()
            assert word in _err(), _err()
        h = C.c_void_p(7)
        rep = lambda ctx, c, count, out=True: lambda: lib.bpg_r1cs_template_repeat_inputs(ctx, c, C.c_uint64(count), C.byref(h) if out else None)
        refused(rep(FAKE, tmpl, 2, out=False), "null")
        refused(rep(None, tmpl, 2), "null")
        refused(rep(FAKE, None, 2), "null")
        refused(rep(FAKE, tmpl, 0), "at least 1")
        refused(rep(FAKE, tmpl, 2), "no device state")
        assert not h.value
        for c in (tmpl, plain):                              # with or without inputs: a handle without device state is refused, part by part
            arr = (bpg.TemplatePart * 2)()
            arr[0].tmpl, arr[0].count, arr[1].tmpl, arr[1].count = c, 0, c, 1
            refused(lambda: lib.bpg_r1cs_template_join_inputs(FAKE, C.c_uint64(2), arr, C.byref(h)), "part 0: count must be at least 1")
            arr[0].count = 1
            refused(lambda: lib.bpg_r1cs_template_join_inputs(FAKE, C.c_uint64(2), arr, C.byref(h)), "part 0: the handle has no device state")
        refused(lambda: lib.bpg_r1cs_template_join_inputs(FAKE, C.c_uint64(0), arr, C.byref(h)), "no parts")
        refused(lambda: lib.bpg_r1cs_template_join_inputs(FAKE, C.c_uint64(1), None, C.byref(h)), "null")
        # the older calls keep their refusals, word for word
        refused(lambda: lib.bpg_r1cs_template_repeat(FAKE, tmpl, C.c_uint64(2), C.byref(h)), "the template has public inputs (a repeat carries none")
        arr[0].tmpl = tmpl
        refused(lambda: lib.bpg_r1cs_template_join(FAKE, C.c_uint64(1), arr, C.byref(h)), "the template has public inputs (a join carries none)")
        # set_inputs
        vals = bytes(32 * n_in)
        refused(lambda: lib.bpg_r1cs_set_inputs(FAKE, tmpl, C.c_uint64(n_in + 1), vals + bytes(32)), "n_inputs does not match")
        refused(lambda: lib.bpg_r1cs_set_inputs(FAKE, tmpl, C.c_uint64(n_in), None), "input_values is null")
        refused(lambda: lib.bpg_r1cs_set_inputs(FAKE, plain, C.c_uint64(0), None), "not a template with public inputs")
        refused(lambda: lib.bpg_r1cs_set_inputs(FAKE, tmpl, C.c_uint64(n_in), vals), "no device state")
        refused(lambda: lib.bpg_r1cs_set_inputs(None, tmpl, C.c_uint64(n_in), vals), "null")
    finally:
        lib.bpg_r1cs_free(None, tmpl); lib.bpg_r1cs_free(None, plain)


@pytest.mark.parametrize("n_inputs, n_coefs, word", [(1, 9, "coefficient slots"), (5, 1, "public inputs exceed")])
def test_size_limits_at_their_edges(n_inputs, n_coefs, word):
    """shared + count (n_params + n_slots) < 2^30 and count n_inputs < 2^29, through the hooks (the check the device path starts with), at the first count
    that breaks the formula and the last that keeps it.  A count that passes the size check is refused a line later for its zero-length buffers, before
    anything is built - so neither call allocates."""
    p = hand_instance(n_inputs, n_coefs)
    inst, values = p.template_instance()
    prog, hints = p.witness_program(hints=True)
    n_slots = len(RC.input_pairs(inst)[0])
    assert (inst.n, inst.m, len(values), n_slots, len(prog.param_rows)) == (1, 0, n_inputs, n_inputs * n_coefs, 0)
    slot_edge, input_edge = -(-((1 << 30) - inst.ncoef) // n_slots), -(-(1 << 29) // n_inputs)
    edge = min(slot_edge, input_edge)
    assert edge == (slot_edge if n_coefs > 1 else input_edge) and slot_edge != input_edge and edge * inst.n < 1 << 27 and edge * inst.nnz < 1 << 32
    assert inst.ncoef + edge * n_slots >= 1 << 30 or edge * n_inputs >= 1 << 29
    assert inst.ncoef + (edge - 1) * n_slots < 1 << 30 and (edge - 1) * n_inputs < 1 << 29
    lib = bpg.lib()
    cs, cp = inst.cstruct(), prog.cstruct()
    cs.aL = cs.aR = cs.aO = None
    nnz, nc = C.c_uint64(), C.c_uint64()
    rp = np.zeros(1, np.uint64)

    def call(count):
        return lib.bpg_test_template_repeat_inputs_instance(C.byref(cs), C.byref(cp), None, C.c_uint64(n_inputs), C.c_uint64(count), None, bytes(32), C.c_void_p(rp.ctypes.data),
                                                            C.c_uint64(0), None, None, C.c_uint64(0), None, C.c_uint64(0), C.byref(nnz), C.byref(nc))
    assert call(edge) == 4 and word in _err(), _err()
    assert call(edge - 1) == 4 and "row_ptr too short (%d entries" % ((edge - 1) * inst.q + 1) in _err(), _err()      # the sizes were accepted
    # the same limits through the join hook, one part
    part = (bpg.TestJoinInputsPart * 1)()
    part[0].inst, part[0].program, part[0].n_inputs = C.pointer(cs), C.pointer(cp), n_inputs

    def jcall(count):
        part[0].count = count
        return lib.bpg_test_template_join_inputs_instance(C.c_uint64(1), part, None, bytes(32), C.c_void_p(rp.ctypes.data), C.c_uint64(0), None, None, C.c_uint64(0), None,
                                                          C.c_uint64(0), C.byref(nnz), C.byref(nc))
    assert jcall(edge) == 4 and ("coefficient slots" if n_coefs > 1 else "public inputs exceed") in _err(), _err()
    assert jcall(edge - 1) == 4 and "row_ptr too short (%d entries" % ((edge - 1) * inst.q + 1) in _err(), _err()


def test_a_buffer_one_short_is_refused_named_and_nothing_is_written(templates):
    tinst, prog, hints, cks, n_in, n_slots = templates(("random", 1))
    K = 2
    a = RC.Assembly([(("random", 1), [0, 1])], False)
    need = bpg.test_template_repeat_inputs_instance(tinst, prog, hints, n_in, K, a.params, a.inputs, n_slots=n_slots)
    exact = (len(need[0]), len(need[1]), len(need[3]) // 32)
    assert exact[0] == K * tinst.q + 1 and exact[2] == tinst.ncoef + K * (len(prog.param_rows) + n_slots)
    assert bpg.test_template_repeat_inputs_instance(tinst, prog, hints, n_in, K, a.params, a.inputs, sizes=exact)[3] == need[3]      # exactly the formulas' sizes: served
    jparts = [(tinst, prog, hints, 1, cks, n_in), (tinst, prog, hints, 1, cks, n_in)]
    assert bpg.test_template_join_inputs_instance(jparts, a.params, a.inputs, sizes=(exact[0], exact[1], exact[2] + tinst.ncoef))[0].tolist() == need[0].tolist()
    for i, word in enumerate(("row_ptr", "term_var", "coef")):
        for hook in ("repeat", "join"):
            sizes = tuple(x - (i == j) for j, x in enumerate(exact if hook == "repeat" else (exact[0], exact[1], exact[2] + tinst.ncoef)))
            bufs = []
            with pytest.raises(bpg.BpgError) as e:
                if hook == "repeat":
                    bpg.test_template_repeat_inputs_instance(tinst, prog, hints, n_in, K, a.params, a.inputs, sizes=sizes, buffers=bufs)
                else:
                    bpg.test_template_join_inputs_instance(jparts, a.params, a.inputs, sizes=sizes, buffers=bufs)
            assert e.value.status == 4 and word in str(e.value) and "too short" in str(e.value), str(e.value)
            assert all((b == np.iinfo(b.dtype).max).all() for b in bufs[:3]) and set(bufs[3].raw) == {0xff}, "a refused call wrote into a buffer"
    # the eval hooks: missing inputs or checkpoint values are refused before a vector is touched
    with pytest.raises(bpg.BpgError) as e:
        bpg.test_template_eval_repeat_inputs(tinst, prog, hints, cks, n_in, K, a.instance().v, None, None)
    assert e.value.status == 4 and "public inputs" in str(e.value)
    with pytest.raises(bpg.BpgError) as e:
        bpg.test_template_eval_join_inputs(jparts, a.instance().v, None, None)
    assert e.value.status == 4 and "public inputs" in str(e.value)


def test_index_maps_slot_kernel_and_lanes_under_the_sanitizers(tmp_path):
    """tests/hostcheck/template_inputs_parts.cpp: the new branches of repeat_map and join_map, the index arithmetic of k_input_slots_join and the two lane
    functions with inputs through the host compiler under ASan and UBSan (a stand-alone program: no preload, no device), on exact-size buffers"""
    exe = tmp_path / "template_inputs_parts"
    src = O.ROOT / "tests" / "hostcheck" / "template_inputs_parts.cpp"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    assert r.stdout.split()[-1] == "ok"


def test_header_prototypes_match_the_binding():
    hdr = (O.ROOT / "include" / "bpg.h").read_text()
    proto = lambda name: [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", re.search(r"bpg_status %s\(([^;]*)\);" % name, hdr).group(1)).split(",")]
    assert proto("bpg_r1cs_template_repeat_inputs") == ["bpg_ctx *ctx", "bpg_circuit *tmpl", "uint64_t count", "bpg_circuit **out"]
    assert proto("bpg_r1cs_template_join_inputs") == ["bpg_ctx *ctx", "uint64_t n_parts", "const bpg_template_part *parts", "bpg_circuit **out"]
    assert proto("bpg_r1cs_set_inputs") == ["bpg_ctx *ctx", "bpg_circuit *c", "uint64_t n_inputs", "const uint8_t *input_values"]
    tail = ["uint64_t *row_ptr", "uint64_t row_cap", "uint32_t *term_var", "uint32_t *term_coef", "uint64_t term_cap", "uint8_t *coef", "uint64_t coef_cap", "uint64_t *nnz_out",
            "uint64_t *ncoef_out"]
    head = ["const bpg_r1cs_instance *inst", "const bpg_witness_program *program", "const bpg_witness_hints *hints"]
    outs = ["uint8_t *aL_out", "uint8_t *aR_out", "uint8_t *aO_out", "uint64_t *first_mismatch"]
    assert proto("bpg_test_template_repeat_inputs_instance") == head + ["uint64_t n_inputs", "uint64_t count", "const uint8_t *param_values", "const uint8_t *input_values"] + tail
    assert proto("bpg_test_template_eval_repeat_inputs") == head + ["const bpg_witness_checkpoints *checkpoints", "uint64_t n_inputs", "uint64_t count", "const uint8_t *v",
                                                                    "const uint8_t *ck_values", "const uint8_t *input_values"] + outs
    jhead = ["uint64_t n_parts", "const bpg_test_join_inputs_part *parts"]
    assert proto("bpg_test_template_join_inputs_instance") == jhead + ["const uint8_t *param_values", "const uint8_t *input_values"] + tail
    assert proto("bpg_test_template_eval_join_inputs") == jhead + ["const uint8_t *v", "const uint8_t *ck_values", "const uint8_t *input_values"] + outs
    fields = re.search(r"typedef struct \{([^}]*)\} bpg_test_join_inputs_part;", hdr).group(1)
    assert [" ".join(f.split()).split("*")[-1].split()[-1] for f in fields.split(";") if f.strip()] == [n for n, _ in bpg.TestJoinInputsPart._fields_]
    assert [n for n, _ in bpg.TestJoinInputsPart._fields_][:5] == [n for n, _ in bpg.TestJoinPart._fields_] and C.sizeof(bpg.TestJoinInputsPart) == 48
    assert all(hasattr(bpg.lib(), f) for f in ("bpg_r1cs_template_repeat_inputs", "bpg_r1cs_template_join_inputs", "bpg_r1cs_set_inputs",
                                               "bpg_test_template_repeat_inputs_instance", "bpg_test_template_eval_repeat_inputs",
                                               "bpg_test_template_join_inputs_instance", "bpg_test_template_eval_join_inputs"))
    assert all(hasattr(bpg.ResidentCircuit, f) for f in ("repeat_inputs", "set_inputs", "check_batch_inputs")) and hasattr(bpg.Context, "join_inputs")
