"""Random circuit templates against big-integer evaluation, without a GPU: the scheduler, the packer and every layout of the witness interpreter compiled for
the host, on shapes nobody drew by hand (tests/random_templates.py: m = 0, q = 0, n of 1, 2, 3, several sources and parameter rows per item, hint runs over
arbitrary linear combinations, zero coefficients, empty lists).

Two yardsticks, neither of them the code under test: the generator's MODEL (random_templates.evaluate: Python integers mod l read off the shape), and FRESH
HOST ASSEMBLIES - a separately built prover's instance() for every witness a template is evaluated on.  A template is always made from ONE item under value
seed 0 and evaluated under other value seeds.

SEEDS is the range every family runs over; test_generator_still_covers_the_edges keeps an edit of the generator from hollowing it."""
import random

import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import random_templates as RT
import template_inputs_cases as TC
from test_template_host import StubProver, check_invariant
from test_template_hints_host import schedule_hinted, check_against_host
from test_template_repeat_host import row_view
from test_template_checkpoints_host import eval_ck, schedule_ck
from test_template_inputs_host import eval_inputs, eval_batch_inputs, inputs_instance, meaning, meaning_of

L = bpg.L
SEEDS = range(200)
OTHERS = (1, 2, 3)              # the value seeds a template (value seed 0) is evaluated under
KS = (1, 2, 3, 5)
DENSITIES = (0.1, 0.5, 1.0)


def assemble(shape_seed, value_seeds, public=None):
    """ONE prover, the shape's items under the given value seeds one after the other -> (prover, [Item]); public: None, or as_inputs of the Public it makes"""
    p = StubProver(None, bpg.Transcript(b"RandomTemplate"))
    pub = None if public is None else TC.Public(p, public)
    return p, [RT.item(p, shape_seed, vs, pub) for vs in value_seeds]


def exported(p):
    prog, hints = p.witness_program(hints=True)
    return p.instance(), prog, hints


class Built:
    """shape `seed` assembled alone under value seed 0 (the template) and under OTHERS (the fresh host assemblies)"""
    def __init__(self, seed):
        self.seed = seed
        self.prover, (self.item,) = assemble(seed, [0])
        self.shape = self.item.shape
        self.template = exported(self.prover)
        self.others = [assemble(seed, [vs]) for vs in OTHERS]
        self.schedule = schedule_hinted(*self.template)


@pytest.fixture(scope="module")
def built():
    return {seed: Built(seed) for seed in SEEDS}


def test_plain_and_hinted(built):
    for seed, b in built.items():
        inst, prog, hints = b.template
        sh = b.shape
        assert (inst.n, inst.m, inst.q, len(hints), len(prog.param_rows)) == (sh.n, sh.m, sh.q, sh.hints, sh.rows), "shape %d" % seed
        assert list(hints.arg) == sh.hint_bits and prog.param_rows == b.item.rows, "shape %d" % seed
        assert (inst.aL, inst.aR, inst.aO) == b.item.witness(), "shape %d: the host assembly differs from the model" % seed
        check_invariant(inst, prog, b.schedule)
        for p, (it,) in b.others:
            o = p.instance()
            assert o.v == it.values and (o.aL, o.aR, o.aO) == it.witness(), "shape %d: the host assembly differs from the model" % seed
        try:
            check_against_host(b.template, [p for p, _ in b.others])          # `evaluate` of the hints module, the single and the batched interpreter
        except AssertionError as e:
            raise AssertionError("shape %d: %s" % (seed, e))


@pytest.mark.parametrize("K", KS)
def test_repeat(built, K):
    for seed, b in built.items():
        if (K == 3 and seed % 2 == 0) or (K == 5 and seed % 2 == 1):                     # the larger assemblies on every second shape: K = 3 on the odd seeds, K = 5 on the even ones
            continue
        tinst, prog, hints = b.template
        p, items = assemble(seed, [10 + k for k in range(K)])
        want = p.instance()
        params = [x for it in items for x in it.params]
        assert (want.n, want.q, want.m) == (K * tinst.n, K * tinst.q, K * tinst.m), "shape %d" % seed
        row_ptr, tv, tc, coef = bpg.test_template_repeat_instance(tinst, prog, hints, K, params)
        assert len(row_ptr) == want.q + 1 and int(row_ptr[-1]) == len(tv) == len(tc)
        for r in range(want.q):
            got, exp = row_view(row_ptr, tv, tc, coef, r), row_view(want.row_ptr, want.term_var, want.term_coef, want.coef, r)
            assert got == exp, "shape %d: row %d (row %d of item %d)" % (seed, r, r % tinst.q, r // tinst.q)
        wit = bpg.test_template_eval_repeat(tinst, prog, hints, K, want.v)
        assert wit == (want.aL, want.aR, want.aO), "shape %d: the repeat-layout interpreter differs from the K-fold host assembly" % seed
        assert wit == tuple(b"".join(it.witness()[k] for it in items) for k in range(3)), "shape %d: ... and from the model" % seed
        assert O.satisfied(O.FlatCircuit(want.n, want.m, *wit, row_ptr, tv, tc, coef), want.v), "shape %d: the oracle rejects the hook's instance" % seed


def join_parts(join_seed):
    """2-3 parts of random shapes with counts from {1, 2, 3}; a part carries a 0.5-density checkpoint set four times in ten"""
    R = random.Random("random-template-join-%d" % join_seed)
    parts = []
    for k in range(R.randint(2, 3)):
        seed = R.choice(SEEDS)
        cks = None
        if R.random() < 0.4:
            cks = RT.checkpoint_set(seed, 0.5, RT.mul_refs(RT.shape(seed).n))[0]
        parts.append((seed, R.choice((1, 2, 3)), cks))
    return parts


def join_assembly(parts, prover=None, value_base=100):
    """ONE prover, part by part, item by item -> (prover, [[Item] per part])"""
    p = prover or StubProver(None, bpg.Transcript(b"RandomJoin"))
    return p, [[RT.item(p, seed, value_base + 10 * k + i) for i in range(count)] for k, (seed, count, _) in enumerate(parts)]


def test_join(built):
    seen = set()
    for js in SEEDS:
        parts = join_parts(js)
        p, items = join_assembly(parts)
        want = p.instance()
        hp, ck_values = [], []
        for (seed, count, cks), its in zip(parts, items):
            b = built[seed]
            hp.append(b.template + (count, b.item.checkpoints(cks)[0] if cks else None))
            for it in its:
                ck_values += it.checkpoints(cks)[1] if cks else []
            seen |= {"m = 0"} if b.shape.m == 0 else set()
            seen |= {"no rows"} if b.shape.q == 0 else set()
            seen |= {"no parameters"} if b.shape.rows == 0 else set()
            seen |= {"hinted"} if b.shape.hints else set()
            seen |= {"checkpoints"} if cks else set()
            seen |= {"plain between checkpointed"} if len(parts) == 3 and parts[0][2] and parts[2][2] and not parts[1][2] else set()
        params = [x for its in items for it in its for x in it.params]
        row_ptr, tv, tc, coef = bpg.test_template_join_instance(hp, params)
        assert len(row_ptr) == want.q + 1 and int(row_ptr[-1]) == len(tv) == len(tc), "join %d" % js
        for r in range(want.q):
            (gt, gc), (wt, wc) = row_view(row_ptr, tv, tc, coef, r), row_view(want.row_ptr, want.term_var, want.term_coef, want.coef, r)
            assert (sorted(gt), gc) == (sorted(wt), wc), "join %d %r: row %d" % (js, parts, r)
        aL, aR, aO, first = bpg.test_template_eval_join(hp, want.v, ck_values or None)
        assert first is None, "join %d %r: checkpoint %d reported for true values" % (js, parts, first)
        assert (aL, aR, aO) == (want.aL, want.aR, want.aO), "join %d %r: the join-layout interpreter differs from the one-prover assembly" % (js, parts)
        assert (aL, aR, aO) == tuple(b"".join(it.witness()[k] for its in items for it in its) for k in range(3)), "join %d: ... and from the model" % js
        assert O.satisfied(O.FlatCircuit(want.n, want.m, aL, aR, aO, row_ptr, tv, tc, coef), want.v), "join %d: the oracle rejects the hook's instance" % js
        if ck_values:                                        # one wrong value: the flat index in the JOINED list, at or below the bumped one
            k = random.Random(js).randrange(len(ck_values))
            bad = list(ck_values); bad[k] = RT.sc(int.from_bytes(bad[k], "little") + 1)
            got = bpg.test_template_eval_join(hp, want.v, bad)[3]
            assert got is not None and got <= k, "join %d %r: checkpoint %d bumped, %r reported" % (js, parts, k, got)
    assert seen == {"m = 0", "no rows", "no parameters", "hinted", "checkpoints", "plain between checkpointed"}, seen


def test_checkpoints(built):
    """random subsets of all 3 n multiplier variables, shuffled: a_L / a_R of hinted multipliers and variables read through the register copy among them"""
    stats = {d: [0, 0, 0, 0, 0] for d in DENSITIES}          # per density: pairs, fell, rose, levels without (summed), levels with
    for seed, b in built.items():
        inst, prog, hints = b.template
        host, (it,) = b.others[0]
        want = host.instance()
        for density in DENSITIES:
            refs, R = RT.checkpoint_set(seed, density, b.item.mul_refs())
            ck_vars, ck_values = it.checkpoints(refs)
            where = "shape %d, density %s" % (seed, density)
            levels = schedule_ck(inst, prog, hints, ck_vars)["levels"]
            for i, x in enumerate((1, levels < b.schedule["levels"], levels > b.schedule["levels"], b.schedule["levels"], levels)):
                stats[density][i] += x
            aL, aR, aO, first = eval_ck(inst, prog, hints, ck_vars, ck_values, v=want.v)
            assert first is None, "%s: checkpoint %d reported for true values" % (where, first)
            assert (aL, aR, aO) == (want.aL, want.aR, want.aO), "%s: the checkpointed interpreter differs from the host assembly" % where
            k = R.randrange(len(refs))
            ints = [int.from_bytes(x, "little") for x in ck_values]
            ints[k] = (ints[k] + 1) % L
            got = eval_ck(inst, prog, hints, ck_vars, [RT.sc(x) for x in ints], v=want.v)[3]
            assert got is not None and got <= k, "%s: checkpoint %d bumped, %r reported" % (where, k, got)
            assert got == RT.first_mismatch(b.shape, it.v, (), refs, ints), "%s: checkpoint %d bumped: not the lowest one the model finds wrong" % (where, k)
    # a checkpointed term read in mid-segment cuts the segment, and later internal references become external: a set can DEEPEN the schedule
    for density, (pairs, fell, rose, without, with_) in stats.items():
        print("checkpoint sets of density %s over %d random shapes: the level count fell in %d, rose in %d, stayed in %d; levels with / without %d / %d" % (
            density, pairs, fell, rose, pairs - fell - rose, with_, without))
    assert sum(s[1] for s in stats.values()) and sum(s[2] for s in stats.values())


def test_public_inputs():
    for seed in SEEDS:
        p, (it0,) = assemble(seed, [0], public=True)
        inst, values = p.template_instance()
        prog, hints = p.witness_program(hints=True)
        tmpl = (inst, prog, hints, values)
        assert values == it0.inputs and prog.param_rows == it0.rows, "shape %d" % seed
        hosts, items = [], []
        for vs in OTHERS:
            hp, (it,) = assemble(seed, [vs], public=False)                   # the constants baked in: an assembly that knows nothing of inputs
            hosts.append(hp.instance()); items.append(it)
        for host, it in zip(hosts, items):
            assert (host.aL, host.aR, host.aO) == it.witness(), "shape %d: the host assembly differs from the model" % seed
            aL, aR, aO, first = eval_inputs(tmpl, host.v, it.inputs)
            assert first is None and (aL, aR, aO) == it.witness(), "shape %d: the interpreter differs from the assembly with constants" % seed
            assert meaning(*inputs_instance(tmpl, it.inputs, it.params)) == meaning_of(host), "shape %d: the resident rows do not mean the host's rows" % seed
        got = eval_batch_inputs(tmpl, [h.v for h in hosts], [it.inputs for it in items])
        assert got == [it.witness() for it in items], "shape %d: the batched interpreter, every item with inputs of its own" % seed


def test_generator_still_covers_the_edges(built):
    shapes = [b.shape for b in built.values()]
    levels = [b.schedule["levels"] for b in built.values()]
    segments = [b.schedule["segments"] for b in built.values()]
    total = len(shapes)
    assert sum(1 for s in shapes if s.hints) * 2 >= total, "at least half the shapes are hinted"
    assert sum(1 for x in levels if x >= 10) * 4 >= total, "at least a quarter have 10 levels or more"
    assert max(levels) >= 40 and max(segments) >= 100
    for what, have in (("m = 0", lambda s: s.m == 0), ("q = 0", lambda s: s.q == 0), ("n = 1", lambda s: s.n == 1), ("n = 2", lambda s: s.n == 2),
                       ("a sparse hint bit >= 200", lambda s: max(s.hint_bits, default=0) >= 200), ("a zero coefficient", lambda s: s.zero_coefs),
                       ("an empty linear combination", lambda s: s.empty_lcs), ("a right list that is the left list", lambda s: s.same_as_left)):
        assert any(have(s) for s in shapes), "no shape with " + what
    print("%d shapes: %d hinted, %d with >= 10 levels, at most %d levels and %d segments, %d with rows" % (
        total, sum(1 for s in shapes if s.hints), sum(1 for x in levels if x >= 10), max(levels), max(segments), sum(1 for s in shapes if s.q)))
