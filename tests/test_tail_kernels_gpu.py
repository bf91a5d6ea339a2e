"""The table-driven kernels of the inner-product argument (hip/k_ipa.cuh) at chosen scalars, through bpg_test_tail and bpg_test_commit3 - the freeze step, the
per-round step and the commitment step of the prover, on the context's own generators: k_tt_bases, k_tt_multiples, k_tt_factors, k_tt_advance, k_tt_round,
k_tt_finish, the 8-bit k_tt_bases8 / k_tt_multiples8 / k_tt_round8, and k_tt_commit3 / k_tt_commit3_finish.

Inside a proof every scalar that reaches these kernels is a product of Fiat-Shamir challenges.  Here every case of the catalogue (tests/tail_cases.py: every
window at -8 or +7, at -128 or +127, those digits on both sides of each word edge, carries through all eight words, [2^252, l), all-zero vectors, one live
thread at each position of a block, <a_lo, b_hi> = 0, the scalar on B at each digit edge, challenges and y^-1 of 1, l - 1 and 2, the padding class on chosen
lanes) goes through one call, and the test compares, byte for byte,
  - every L_j and R_j with the textbook round on folded generator points (the CPU oracle's sums; plain integers for the scalars),
  - the folded a and b after the last challenge,
  - A_I, A_O and S with their defining sums,
and the evidence of the launch (round kernel, tables, M0, nblk, the block-sum layout) with what the shape predicts.  No case is skipped or sampled; the
parametrisation is by shape and tables with the cases looped inside, and a failure names the case, the round and the side.

The lockstep kernels k_bt_* (hip/k_batch.cuh) repeat the per-point code of these kernels for a wave of proofs; their wave is a separate structure and is not
run here."""
import ctypes as C
import hashlib

import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import tail_cases as T
from bulletproofs_gadgets_amd import workloads

pytestmark = pytest.mark.gpu

CAP = 128
SMALL = (1, 2, 4, 5, 6, 7)          # M0 = 2: 16 live threads; 4; 16: half a block; 32: one block, G and H meet at thread 128; 64: one block per side; 128


class Tables:
    """The generators of a context as lists of encodings, with the two Pedersen bases."""
    def __init__(self, c, count):
        g, h = c.gens_export(0, count)
        self.G, self.H = T.split_points(g), T.split_points(h)
        self.B, self.Bb = c.pedersen_bases()
        self.key = hashlib.sha256(g + h + self.B + self.Bb).digest()


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tabs(ctx):
    return Tables(ctx, CAP)


@pytest.fixture
def make_ctx(monkeypatch):
    """A fresh context with the given environment knobs (they are read once, at context creation)."""
    made = []

    def make(cap, **env):
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        c = bpg.Context(0)
        made.append(c)
        for k in env:
            monkeypatch.delenv(k)
        c.gens_ensure(cap)
        return c
    yield make
    for c in made:
        c.close()


_references = {}


def reference(tabs, case, lgM0, first, n, rounds, expanded=False):
    """T.tail_reference, computed once per (generators, case, shape) and shared by every table kind and layout that runs the same case."""
    key = (tabs.key, case, lgM0, first, n if first else 0, rounds)
    if key not in _references:
        f = T.tail_reference_expanded if expanded else T.tail_reference
        _references[key] = f(tabs.G, tabs.H, tabs.B, case, lgM0, first, n, rounds)
    return _references[key]


def run_tail(c, tabs, lgM0, tables, first, n, cases, rounds=None, quad=1, expanded=False):
    """One bpg_test_tail call per case, checked: every L_j, R_j and the folded a, b against the reference, the evidence against the shape."""
    M0 = 1 << lgM0
    rounds = lgM0 if rounds is None else rounds
    assert cases
    for case in cases:
        lr, a, b, ev = c.test_tail(lgM0, tables, first, n, [T.sc(s) for s in case.a], [T.sc(s) for s in case.b], T.sc(case.yinv), T.sc(case.u_ch), T.sc(case.gamma0),
                                   T.sc(case.eta0), T.sc(case.w), [T.sc(u) for u in case.u[:rounds]])
        where = "M0 = %d, tables %d, first %d, n %d, case %r" % (M0, tables, first, n, case.name)
        want_lr, want_a, want_b = reference(tabs, case, lgM0, first, n, rounds, expanded)
        for j in range(rounds):
            for side in (0, 1):
                assert lr[j][side] == want_lr[j][side], "%s: round %d, %s differs: %s, expected %s" % (where, j, "LR"[side], lr[j][side].hex(), want_lr[j][side].hex())
        assert a == [T.sc(s) for s in want_a], "%s: the folded a differs after %d rounds" % (where, rounds)
        assert b == [T.sc(s) for s in want_b], "%s: the folded b differs after %d rounds" % (where, rounds)
        assert ev == {"kernel": "k_tt_round8" if tables == 2 else "k_tt_round", "tables": tables, "M0": M0, "nblk": -(-M0 * 8 // 256), "quad": quad}, where


def shapes(lgM0):
    """(first, n) of one M0: a later round, and a first round with each of its n."""
    return [(0, 0)] + [(1, n) for n in T.first_ns(1 << lgM0)]


# ---------------------------------------------------------------------------------------------------- the tail on 4-bit tables
@pytest.mark.parametrize("tables", [0, 1])
@pytest.mark.parametrize("lgM0", SMALL)
def test_tail_on_4bit_tables(ctx, tabs, lgM0, tables):
    """All lgM0 sub-rounds of every case: on the context's tables of the original generators (0) and on tables built in the arena as for folded ones (1), in a later
    round and in a first round with the class boundary nowhere, everywhere, inside a block and (M0 = 128) on a multiple of 32."""
    for first, n in shapes(lgM0):
        run_tail(ctx, tabs, lgM0, tables, first, n, T.tail_cases(lgM0, first, n))


def test_one_live_thread_at_each_position_of_a_block(ctx, tabs):
    """M0 = 32 is exactly one block per sum, G on threads 0..127 and H on 128..255: one non-zero scalar with digits in one word lights one thread.  Every (vector,
    position, word): each thread of the block is the only live one once for L and once for R, the other sum and the term on B are the identity or zero."""
    cases = T.single_thread_cases(5)
    run_tail(ctx, tabs, 5, 0, 0, 0, cases, rounds=1)
    lit = {(j, side) for case in cases[:16] for j, pair in enumerate(reference(tabs, case, 5, 0, 0, 1)[0]) for side in (0, 1) if pair[side] != T.IDENTITY}
    assert lit == {(0, 1)} or lit == {(0, 0)}                  # a[0] alone: one of L, R, never both


# ---------------------------------------------------------------------------------------------------- the tail on 8-bit tables
@pytest.mark.parametrize("lgM0", [6, 7])
def test_tail_on_8bit_tables(make_ctx, lgM0):
    """k_tt_round8 on a fresh context whose budget admits the wide tables (64 and 128 MB of them): the evidence names the kernel, so a context that
    fell back to the 4-bit tables fails here instead of passing on them."""
    c = make_ctx(CAP, BPG_TT_WIDE_GB=1)
    t = Tables(c, CAP)
    for first, n in shapes(lgM0):
        run_tail(c, t, lgM0, 2, first, n, T.tail_cases(lgM0, first, n))
    with pytest.raises(bpg.BpgError) as e:                      # no 8-bit tables below 64 generators: refused, not run on the 4-bit ones
        one = T.sc(1)
        c.test_tail(5, 2, 0, 0, [one] * 32, [one] * 32, one, one, one, one, one, [one])
    assert e.value.status == 4


def test_8bit_tables_are_refused_without_a_budget(ctx):
    one = T.sc(1)
    with pytest.raises(bpg.BpgError) as e:                      # the one-shot profile keeps no 8-bit tables
        ctx.test_tail(6, 2, 0, 0, [one] * 64, [one] * 64, one, one, one, one, one, [one])
    assert e.value.status == 4 and "8-bit" in str(e.value)


# ---------------------------------------------------------------------------------------------------- the other block-sum layout
def test_tail_and_commitments_under_the_shared_device_layout(make_ctx):
    """BPG_FOLD_ADAPT=2 takes the block sums of a shared device in every call: quad = 0 in the evidence, the same bytes."""
    c = make_ctx(CAP, BPG_FOLD_ADAPT=2, BPG_TT_WIDE_GB=1)
    t = Tables(c, CAP)
    for lgM0 in (1, 5, 7):
        for first, n in shapes(lgM0)[:3]:
            for tables in (0, 1) + ((2,) if lgM0 == 7 else ()):
                run_tail(c, t, lgM0, tables, first, n, T.tail_cases(lgM0, first, n), quad=0)
    for lgM0, n in ((0, 1), (4, 9), (6, 64)):
        run_commit(c, t, lgM0, n, T.commit_cases(n), quad=0)


# ---------------------------------------------------------------------------------------------------- the commitments
_commit_references = {}


def run_commit(c, tabs, lgM0, n, cases, quad=1):
    M0 = 1 << lgM0
    assert cases
    for case in cases:
        got, ev = c.test_commit3(lgM0, n, *([T.sc(s) for s in v] for v in case[1:]))
        key = (tabs.key, case)
        if key not in _commit_references:
            _commit_references[key] = T.commit_reference(tabs.G, tabs.H, tabs.Bb, case)
        want = _commit_references[key]
        where = "M0 = %d, n = %d, case %r" % (M0, n, case.name)
        for k, name in enumerate(("A_I", "A_O", "S")):
            assert got[k] == want[k], "%s: %s differs: %s, expected %s" % (where, name, got[k].hex(), want[k].hex())
        if case.name == "all zero":
            assert got == [T.IDENTITY] * 3, where
        assert ev == {"M0": M0, "n": n, "nblk": -(-M0 * 16 // 256), "quad": quad}, where


def commit_ns(M0):
    """n = M0, M0/2 + 1, 1 and a value not divisible by 4 - without repeats, within 1..M0."""
    out = []
    for n in (M0, M0 // 2 + 1, 1, M0 - M0 // 4 - 1 if M0 >= 8 else M0 - 1):
        if 1 <= n <= M0 and n not in out:
            out.append(n)
    return out


@pytest.mark.parametrize("lgM0", [0, 1, 4, 6])
def test_commitments(ctx, tabs, lgM0):
    """k_tt_commit3 and its finish: every edge in every one of the five vectors, every blinding edge in each of the three sums, the all-zero case (three
    encodings of 32 zero bytes).  M0 = 1: 16 live threads, M0 = 16: one block, M0 = 64: four."""
    ns = commit_ns(1 << lgM0)
    assert lgM0 < 4 or any(n % 4 for n in ns)
    for n in ns:
        run_commit(ctx, tabs, lgM0, n, T.commit_cases(n))


# ---------------------------------------------------------------------------------------------------- the add branch of the finish kernels
@pytest.fixture(scope="module")
def big():
    c = bpg.Context(0)
    c.gens_ensure(8192)
    yield c, Tables(c, 8192)
    c.close()


def test_finish_adds_its_windows_to_a_partial_from_256_blocks_on(big):
    """M0 = 2^13: k_tt_round leaves 256 block partials per sum, so the 64 window threads of k_tt_finish (the last of the block) hold a partial and ADD the entry of
    B's table; below, they take it as it is.  Ordinary scalars, a first round, sub-rounds 0 and 1.  (1 GB of tables: what a default proof of 2^13 builds.)  The
    reference keeps each virtual generator as coefficients over the 2 * 8192 base points: one oracle sum per L_j, R_j."""
    c, t = big
    lgM0, n = 13, 6657
    cases = [case for case in T.tail_cases(lgM0, 1, n) if case.name == "padding: u_ch and every factor ordinary"]
    run_tail(c, t, lgM0, 0, 1, n, cases, rounds=2, expanded=True)


def test_commit3_finish_adds_its_windows_to_a_partial_from_256_blocks_on(big):
    """M0 = 2^12: 256 block partials per commitment (0.5 GB of tables).  Ordinary witness and blindings, n off a multiple of 4."""
    c, t = big
    n = 4096 - 1025
    W = [[T.ordinary(7000 * v + i) for i in range(n)] for v in range(5)]
    case = T.CommitCase("ordinary, 2^12", *(tuple(v) for v in W), (T.ordinary(1), T.ordinary(2), T.ordinary(3)))
    run_commit(c, t, 12, n, [case])
    assert -(-4096 * 16 // 256) == 256 and -(-8192 * 8 // 256) == 256


# ---------------------------------------------------------------------------------------------------- refusals, and the buffers handed back
def prove_and_compare(c, assembled):
    inst = assembled.prover.instance()
    c.gens_ensure(assembled.gens_capacity)
    res = c.upload(inst)
    seed = bytes(range(32))
    proof, st_after = res.prove(assembled.transcript.state, inst.v_blinding, seed, 0)
    oc = O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)
    rc, want, st_want = O.prove(O.Gens(assembled.gens_capacity), assembled.transcript.state, oc, inst.v_blinding, seed, O.FLAG_FAST_MSM)
    assert rc == 0 and proof == want and st_after == st_want
    res.free()


def test_refusals_leave_the_context_usable(make_ctx):
    """Each refused argument is INVALID_ARGUMENT (4) before any launch; a good call afterwards still matches the reference; proofs on the same context - which take
    the window tables, lv / rv, the factor and coefficient tables and the arena back from the hooks - are the oracle's, byte for byte, at N = the hook's M0 and at
    another N; and the hooks after the proofs still match."""
    c = make_ctx(512)
    t = Tables(c, 128)
    one, big, zero = T.sc(1), T.L.to_bytes(32, "little"), bytes(32)

    def refused(lgM0=7, tables=0, first=0, n=0, a="ok", b="ok", yinv=one, u_ch=one, gamma0=one, eta0=one, w=one, u="ok", count=None):
        M0 = 1 << (lgM0 if 0 <= lgM0 <= 14 else 0)
        a = [one] * M0 if a == "ok" else a
        b = [one] * M0 if b == "ok" else b
        u = [one] * min(max(lgM0, 1), 14) if u == "ok" else u
        with pytest.raises(bpg.BpgError) as e:
            c.test_tail(lgM0, tables, first, n, a, b, yinv, u_ch, gamma0, eta0, w, u)
        assert e.value.status == 4, e.value

    refused(a=None); refused(b=None); refused(yinv=None); refused(u_ch=None); refused(gamma0=None); refused(eta0=None); refused(w=None); refused(u=None)      # NULL
    refused(a=[one] * 127 + [big]); refused(b=[big] + [one] * 127); refused(a=[one] * 64 + [b"\xff" * 32] + [one] * 63)                                       # not canonical
    refused(yinv=big); refused(u_ch=big); refused(gamma0=big); refused(eta0=big); refused(w=big); refused(u=[one] * 6 + [big])
    refused(yinv=zero); refused(u=[one, zero, one]); refused(u=[zero])                                          # y^-1 = 0, a challenge of 0
    refused(lgM0=0); refused(lgM0=15); refused(lgM0=40); refused(lgM0=10, u=[one])                             # M0 out of range, M0 beyond the capacity (512)
    refused(tables=3); refused(tables=2)                                                                       # no such tables; no 8-bit tables in this profile
    refused(first=2, n=100); refused(first=1, n=64); refused(first=1, n=129); refused(first=1, n=0)             # n out of range
    refused(u=b""); refused(u=[one] * 8)                                                                       # rounds outside 1..lgM0

    def refused3(lgM0=6, n=64, vecs="ok", blind="ok", bad=None):
        count = n if 0 <= n <= 1 << 14 else 0
        v = [[one] * count for _ in range(5)] if vecs == "ok" else vecs
        if bad is not None:
            v[bad] = None if count == 0 else [one] * (count - 1) + [big]
        with pytest.raises(bpg.BpgError) as e:
            c.test_commit3(lgM0, n, *v, [one] * 3 if blind == "ok" else blind)
        assert e.value.status == 4, e.value

    for k in range(5):
        refused3(bad=k)
        refused3(vecs=[None if j == k else [one] * 64 for j in range(5)])
    refused3(blind=None); refused3(blind=[one, big, one]); refused3(blind=[one, one, b"\xff" * 32])
    refused3(n=0); refused3(n=65); refused3(lgM0=15, n=1); refused3(lgM0=10, n=1)
    # no context: as on a machine without a GPU
    lr, ab, ev, out = C.create_string_buffer(64), C.create_string_buffer(64), C.create_string_buffer(1024), C.create_string_buffer(96)
    assert bpg.lib().bpg_test_tail(None, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), one * 2, one * 2, one, one, one, one, one, C.c_uint32(1), one,
                                   lr, ab, ev, C.c_uint64(1024)) == 7
    assert bpg.lib().bpg_test_commit3(None, C.c_uint32(0), C.c_uint64(1), one, one, one, one, one, one * 3, out, ev, C.c_uint64(1024)) == 7

    def hooks():
        for tables in (0, 1):
            run_tail(c, t, 7, tables, 1, 105, T.tail_cases(7, 1, 105)[-4:])
        run_tail(c, t, 4, 0, 0, 0, T.tail_cases(4, 0, 0)[-3:])
        run_commit(c, t, 7, 105, T.commit_cases(105)[:2])
        run_commit(c, t, 4, 9, T.commit_cases(9)[-3:])

    hooks()
    prove_and_compare(c, workloads.bounds_check_64(c, seed=32))          # N = 128: the tables the hooks left are the proof's
    hooks()
    prove_and_compare(c, workloads.less_than_126(c, seed=32))            # N = 512: other tables
    prove_and_compare(c, workloads.bounds_check_64(c, seed=33))
    hooks()
