"""The R1CS check on the GPU (bpg_r1cs_check): the device's report - counters and rows - must equal the device-less mirror's (bpg_test_check_host, which
tests/test_check_host.py holds against the oracle and a restatement in Python integers), on circuits made through the Prover surface, on templates and on
repeats; and the call must leave every later proof as it was.

A synthetic row is a list of variable terms closed by ONE constant term, chosen so that the witness satisfies the row; `violate` adds one to that constant
through a coefficient slot of its own, so exactly the rows named break."""
import copy
import hashlib

import pytest
import bulletproofs_gadgets_amd as bpg
from test_template_host import StubProver
from test_template_repeat_host import assemble, bounds8_item, constant_term, sc

pytestmark = pytest.mark.gpu
L = bpg.L
SEED = hashlib.sha256(b"check").digest()
ONE = bpg.Variable.One()


def h(tag, i):
    return int.from_bytes(hashlib.sha512(b"check-gpu %s %d" % (tag, i)).digest(), "little") % L


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(16384)
    yield c
    c.close()


class Synth:
    """n free multipliers and m committed values through a device-less Prover; row(terms) constrains sum(terms) + c = 0 with c closing it"""
    def __init__(self, name, n, m, zero_left=()):
        self.p = StubProver(None, bpg.Transcript(b"check"))
        self.v = [h(name + b" v", j) for j in range(m)]
        self.vars = [[], [], [], []]
        if m:
            self.vars[3] = self.p.commit_many([sc(x) for x in self.v], [sc(h(name + b" vb", j)) for j in range(m)])[1]
        self.vals = [[], [], [], self.v]
        for i in range(n):
            a, b = (0 if i in zero_left else h(name + b" aL", i)), h(name + b" aR", i)
            for k, var in enumerate(self.p.allocate_multiplier((sc(a), sc(b)))):
                self.vars[k].append(var)
            self.vals[0].append(a); self.vals[1].append(b); self.vals[2].append(a * b % L)

    def row(self, terms, constant=None):
        """terms: [(kind, index, coefficient)]; constant None: the closing one"""
        total = sum(c * self.vals[k][i] for k, i, c in terms) % L
        lc = [(self.vars[k][i], sc(c)) for k, i, c in terms]
        c = (-total) % L if constant is None else constant
        self.p.constrain(bpg.LinearCombination(lc + [(ONE, sc(c))]))

    def instance(self):
        return self.p.instance()


def violate(inst, rows):
    """a copy of inst whose rows `rows` have their constant term (the last term of the row) raised by one, each through a coefficient slot of its own"""
    out = copy.copy(inst)
    out.term_coef = inst.term_coef.copy()
    coef = [inst.coef]
    for r in rows:
        t = int(inst.row_ptr[r + 1]) - 1
        assert int(inst.term_var[t]) >> 29 == 4
        k = int(inst.term_coef[t])
        coef.append(sc(int.from_bytes(inst.coef[32 * k:32 * k + 32], "little") + 1))
        out.term_coef[t] = inst.ncoef + len(coef) - 2
    out.coef = b"".join(coef)
    out.ncoef = inst.ncoef + len(rows)
    return out


def same(ctx, inst, max_rows=16):
    """check_flat against the mirror -> the report"""
    got, want = ctx.check_flat(inst, max_rows), bpg.test_check_host(inst, inst.v, max_rows)
    assert got == want, (got, want)
    return got


def test_smallest_circuits(ctx):
    s = Synth(b"one", 1, 0)                                 # n = 1, q = 1
    s.row([(0, 0, 3), (1, 0, 5), (2, 0, 7)])
    inst = s.instance()
    assert (inst.n, inst.q, inst.m) == (1, 1, 0) and same(ctx, inst).ok
    assert same(ctx, violate(inst, [0])).rows == [0]
    s = Synth(b"none", 0, 2)                                # n = 0, m = 2
    s.row([(3, 0, 11), (3, 1, 13)]); s.row([(3, 1, 17)])
    inst = s.instance()
    assert (inst.n, inst.q, inst.m) == (0, 2, 2) and same(ctx, inst).ok
    assert same(ctx, violate(inst, [1])).rows == [1]
    bad = copy.copy(inst); bad.v = sc(s.v[0] + 1) + inst.v[32:]
    assert same(ctx, bad).rows == [0]
    big = copy.copy(inst); big.v = b"".join((x + L).to_bytes(32, "little") for x in s.v)       # v + l: reduced mod l, as assign does
    assert same(ctx, big).ok
    s = Synth(b"norows", 2, 1)                              # q = 0
    inst = s.instance()
    assert (inst.n, inst.q) == (2, 0) and same(ctx, inst).ok
    bad = copy.copy(inst); bad.aO = sc(s.vals[2][0] + 1) + inst.aO[32:]
    r = same(ctx, bad)
    assert (r.bad_multipliers, r.first_bad_multiplier, r.bad_rows) == (1, 0, 0)


@pytest.fixture(scope="module")
def big():
    """n = 700, m = 3: row i touches a_L, a_R, a_O of multiplier i, a commitment and the constant (the shape of verify_cases.py)"""
    s = Synth(b"big", 700, 3)
    for i in range(700):
        s.row([(0, i, 1 + h(b"big l", i)), (1, i, 1 + h(b"big r", i)), (2, i, 1 + h(b"big o", i)), (3, i % 3, 1 + h(b"big v", i))])
    inst = s.instance()
    assert (inst.n, inst.q, inst.m, inst.nnz) == (700, 700, 3, 3500)
    return inst


BIG_ROWS = (0, 63, 64, 255, 256, 699)


@pytest.mark.parametrize("kind", range(5))
def test_one_coefficient_kind_at_a_time(ctx, big, kind):
    """the coefficient of the left, right, output, committed or constant term of rows 0, 63, 64, 255, 256 and 699, one row at a time and all six at once"""
    assert same(ctx, big).ok
    def broken(rows):
        out = copy.copy(big)
        for r in rows:
            t = int(big.row_ptr[r]) + kind
            assert int(big.term_var[t]) >> 29 == (kind if kind < 4 else 4)
            k = int(big.term_coef[t])
            assert list(big.term_coef).count(k) == 1, "a coefficient of its own"
            out.coef = out.coef[:32 * k] + sc(int.from_bytes(big.coef[32 * k:32 * k + 32], "little") + 1) + out.coef[32 * k + 32:]
        return out
    for r in BIG_ROWS:
        assert same(ctx, broken([r])).rows == [r]
    assert same(ctx, broken(BIG_ROWS)).rows == list(BIG_ROWS)


def test_more_violations_than_cap(ctx, big):
    rows = sorted({0, 63, 64, 699} | set(range(100, 396)))
    assert len(rows) == 300 and {0, 63, 64, 699} <= set(rows)
    bad = violate(big, rows)
    r = same(ctx, bad, 16)
    assert (r.bad_rows, r.first_bad_row, r.rows) == (300, 0, rows[:16])
    r = same(ctx, bad, 0)
    assert (r.bad_rows, r.first_bad_row, r.rows) == (300, 0, [])
    assert same(ctx, bad, 300).rows == rows and same(ctx, bad, 1000).rows == rows


def test_multiplier_violations(ctx, big):
    def bumped(idx):
        out = copy.copy(big)
        for i in idx:
            out.aO = out.aO[:32 * i] + sc(int.from_bytes(big.aO[32 * i:32 * i + 32], "little") + 1) + out.aO[32 * i + 32:]
        return out
    for i in (0, 63, 64, 699):
        r = same(ctx, bumped([i]))
        assert (r.bad_multipliers, r.first_bad_multiplier, r.rows) == (1, i, [i])       # row i reads a_O[i]
    r = same(ctx, bumped([0, 63, 64, 699]))
    assert (r.bad_multipliers, r.first_bad_multiplier, r.rows) == (4, 0, [0, 63, 64, 699])
    r = same(ctx, bumped([699]), 0)
    assert (r.bad_multipliers, r.first_bad_multiplier, r.bad_rows, r.rows) == (1, 699, 1, [])


@pytest.fixture(scope="module")
def lengths(ctx):
    """one circuit of n = 8,192, m = 3 with rows of every length the kernels tell apart (terms counted with the closing constant): the threshold is the
    context's own (bpg_profile_report's _schedule), not a copy"""
    T = ctx.schedule()["check_threshold"]
    assert T > 65, "the lengths below assume a threshold above a wave"
    n, m = 8192, 3
    s = Synth(b"len", n, m, zero_left={5})
    allvars = [(k, i) for k in range(3) for i in range(n)] + [(3, j) for j in range(m)]
    want = [1, 2, 63, 64, 65, T - 1, T, T + 1, 4097, 3 * n + m]
    s.p.constrain(bpg.LinearCombination([]))                                # row 0: empty
    s.p.constrain(bpg.LinearCombination([(ONE, sc(9))]))                    # row 1: a constant alone, not zero: violated as it stands
    s.p.constrain(bpg.LinearCombination([(s.vars[0][5], sc(77))]))          # row 2: one term, on a variable that is zero
    first = 3
    for length in want[1:]:                                                 # rows 3..: length - 1 variables and the closing constant
        off = h(b"len off", length) % len(allvars)
        s.row([allvars[(off + 31 * t) % len(allvars)] + (1 + h(b"len c %d" % length, t) % 1000,) for t in range(length - 1)])
    s.row([(k, i, 1 + (i + k) % 5) for k, i in allvars], constant=None)     # the row over ALL 3n + m variables (and the constant)
    inst = s.instance()
    got = [int(inst.row_ptr[r + 1] - inst.row_ptr[r]) for r in range(inst.q)]
    assert got == [0, 1, 1] + want[1:] + [3 * n + m + 1], got
    return inst, first


def test_row_lengths_around_every_boundary(ctx, lengths):
    inst, first = lengths
    r = same(ctx, inst)
    assert r.rows == [1] and r.bad_multipliers == 0         # every row holds but the non-zero constant
    for row in range(first, inst.q):                        # each row violated by its constant, alone
        assert same(ctx, violate(inst, [row])).rows == [1, row]
    r = same(ctx, violate(inst, list(range(first, inst.q))))
    assert r.rows == [1] + list(range(first, inst.q))
    zero = copy.copy(inst); zero.aL = inst.aL[:32 * 5] + sc(1) + inst.aL[32 * 6:]       # the one-term row, through its variable
    r = same(ctx, zero)
    assert 2 in r.rows and r.first_bad_multiplier == 5


def launches(ctx, fn):
    ctx.profile_set(2)
    try:
        res = fn()
        rep = ctx.profile_report()
    finally:
        ctx.profile_set(0)
    return res, {k: v["count"] for k, v in rep.items()}


VIEW_KERNELS = {"k_rowview_count", "k_rowview_fill", "k_rowview_long"}


def test_the_view_is_built_once_and_only_by_check(ctx, big):
    rc = ctx.upload(big)
    state = bpg.Transcript(b"check").state
    _, counts = launches(ctx, lambda: rc.prove(state, big.v_blinding, SEED))
    assert not VIEW_KERNELS & set(counts) and not any(k.startswith("k_check") for k in counts), counts
    r1, counts = launches(ctx, lambda: rc.check(big.v))
    assert VIEW_KERNELS <= set(counts) and counts["k_check_rows"] == counts["k_check_mul"] == counts["k_check_count"] == 1, counts
    r2, counts = launches(ctx, lambda: rc.check(big.v))
    assert not VIEW_KERNELS & set(counts) and "k_scan_apply" not in counts and counts["k_check_rows"] == 1, counts
    assert r1 == r2 and r1.ok
    rc.free()


def test_no_side_effect_on_proofs(ctx, big, monkeypatch):
    """BPG_MERGE=1: the first proof builds the equal-scalar sets; a check between two proofs changes no byte, and a second check agrees with the first"""
    monkeypatch.setenv("BPG_MERGE", "1")
    c2 = bpg.Context(0)
    try:
        c2.gens_ensure(1024)
        state = bpg.Transcript(b"check").state
        alone = c2.upload(big)
        want = [alone.prove(state, big.v_blinding, SEED) for _ in range(2)]
        alone.free()
        rc = c2.upload(big)
        assert rc.prove(state, big.v_blinding, SEED) == want[0]
        bad = bytes(32) + big.v[32:]
        first = rc.check(bad)
        assert not first.ok and first == bpg.test_check_host(big, bad) and rc.check(bad) == first
        assert rc.check(big.v).ok
        assert rc.prove(state, big.v_blinding, SEED) == want[1] == want[0]
        rc.free()
    finally:
        c2.close()


# ------------------------------------------------------------------------------------------------ templates and repeats
def bounds_values(k, bad):
    if bad:
        a = (1 << 8) + 5                                    # a + b = max - min holds, the 8-bit range proof of a does not
        return [sc(7), sc(a), sc(255 - a)]
    p, _, _ = assemble("bounds8", "chk-%d" % k, 1)
    v = p.instance().v
    return [v[0:32], v[32:64], v[64:96]]


def bounds_host(values):
    """the host assembly of one BoundsCheck item with these committed values"""
    p = StubProver(None, bpg.Transcript(b"BoundsCheck"))
    bounds8_item(p, "chk", 0, values)
    return p.instance()


def bounds_template(ctx):
    p, _, rows = assemble("bounds8", "tmpl", 1)
    return p.template(ctx, param_rows=rows), p.instance()


def test_bounds_check_template(ctx):
    tmpl, tinst = bounds_template(ctx)
    fresh = tmpl.repeat(1)
    with pytest.raises(bpg.BpgError) as e:                  # a template before its first assign
        fresh.check()
    assert e.value.status == 5
    fresh.free()
    good, bad = bounds_values(1, False), bounds_values(2, True)
    tmpl.assign(good)
    assert tmpl.check().ok and tmpl.check(b"".join(good)).ok
    tmpl.assign(bad)
    want = bpg.test_check_host(bounds_host(bad))
    got = tmpl.check()
    assert got == want and not got.ok and got.bad_multipliers == 0, (got, want)
    assert tmpl.check(b"".join(good)).bad_rows > 0          # the caller's values against the resident a_L, a_R, a_O of another witness
    tmpl.assign(good)                                       # a fresh assign: the check sees the new witness
    assert tmpl.check().ok
    tmpl.free()


def test_merkle_template_with_a_wrong_root(ctx):
    from bulletproofs_gadgets_amd import workloads
    a = workloads.merkle_full_tree(None, leaves=8, seed=1, prover_cls=StubProver)
    inst = a.prover.instance()
    row = inst.q - 1                                        # hash - root = 0: the last constraint
    tmpl = a.prover.template(ctx, param_rows=[row])
    root = constant_term(inst, row)
    tmpl.assign(inst.v, [root])
    assert tmpl.check().ok
    tmpl.assign(inst.v, [sc(int.from_bytes(root, "little") + 1)])
    r = tmpl.check()
    assert (r.bad_multipliers, r.bad_rows, r.rows) == (0, 1, [row])
    tmpl.free()


def test_repeat_names_the_bad_items(ctx):
    tmpl, tinst = bounds_template(ctx)
    K, bad = 130, (0, 64, 129)
    items = [bounds_values(k, k in bad) for k in range(K)]
    rep = tmpl.repeat(K)
    with pytest.raises(bpg.BpgError) as e:
        rep.check()
    assert e.value.status == 5
    rep.assign(b"".join(b"".join(v) for v in items))
    want = bpg.test_check_host(bounds_host(items[0])).rows   # the rows an out-of-range item breaks
    assert want
    r = rep.check(max_rows=1000)
    assert r.bad_multipliers == 0 and r.items(tinst.q) == [(k, j) for k in bad for j in want]
    assert sorted({k for k, _ in rep.check(max_rows=len(want) + 1).items(tinst.q)}) == [0, 64]
    rep.free()
    tmpl.assign(items[1])
    found = tmpl.check_batch([(v, b"") for v in items])
    assert [k for k, rows in enumerate(found) if rows] == list(bad) and all(found[k] == want[:16] for k in bad)
    assert tmpl.check().ok                                  # the template's own witness was left alone
    tmpl.free()
