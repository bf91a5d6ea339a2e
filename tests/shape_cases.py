"""Circuit SHAPES at their edges: a catalogue of small satisfiable flat circuits chosen for the shape of their constraint matrix, and an integer model of
flattened_constraints(z) - a plain helper module (not a conftest) shared by test_shape_cases_host.py (which pins the catalogue, the model and the size rule of
the transposition workspace without a device) and test_shape_cases_gpu.py (which sends every case through every upload path, single and lockstep).

Every other circuit of the suite comes from a gadget (about two rows per multiplier), from script_cases.spec (one row per multiplier) or from a random
generator (at most two rows per multiplier, three terms per linear combination): q stays well below 3 n + m, no column is much longer than its neighbours,
and empty rows or an empty constant column appear by accident only.  The matrix-layout kernels (k_csc_count / _fill / _colptr between the two k_scan_* passes,
k_flatten, k_flatten_const, k_repeat_*, k_join_*, the block-diagonal transpose of the lockstep wave) therefore saw one family of shapes.  The catalogue:
  tall     more rows than variables (q > 3 n + m): n = 1 / q = 70, n = 3 (N = 4), m = 2 / q = 600, n = 1, m = 1 / q = 2100 (the row scan takes two blocks, the
           column scan one), n = 0, m = 2 / q = 300 (no multiplier: the single prover and the verifier only)
  wide     q = 0 (n = 5; n = 2 with m = 3) and q = 1 with n = 700 (3 n + m crosses a scan block: the column scan takes two, the row scan one)
  empty    the first row empty, the last row empty, 300 empty rows in a run that crosses a block of k_csc_count, every row empty (q = 10, nnz = 0)
  const    no constant term anywhere (rows that hold by cancellation or by zero coefficients), rows of constants only (they sum to zero), one row with forty
           constant terms, a matrix of constant terms only
  hot      q = 600 with a_L of multiplier 0 / committed value m - 1 in EVERY row and no other column of that kind in use
  dup      one variable five times in a row, terms of coefficient 0, terms of coefficient l - 1
  sect     no left / no right / no output / no committed term at all (m > 0): two section bounds of k_repeat_entries coincide
  edge     terms on multiplier 0 and n - 1 of each kind and on committed value 0 and m - 1, at n = 7 and n = 8
Each case is a verify_cases.Circuit: a witness a_L, a_R, a_O = a_L a_R, committed values with blindings - all from SHAKE - and rows closed with the constant
that makes them hold (VC._closed) unless the case is about not having one.  Each carries the PREDICATE that makes it that case, computed from its own n, m, q
and rows: no test writes a threshold.

model(circuit, z) is script_cases.weights: Python integers, nothing of the package's arithmetic."""
import collections
import functools
import hashlib

import numpy as np

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import script_cases as S
import verify_cases as VC

L = S.L
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
ONE = VC.var(KIND_ONE)
GENS_CAPACITY = 1024
SCAN_CHUNK = 2048            # keys per block of k_scan_blocksums / k_scan_apply (csrc/host/csc_work.hpp CSC_SCAN_CHUNK)
COUNT_BLOCK = 256            # rows per block of k_csc_count / k_csc_fill
LOCKSTEP_K = 8               # copies of one case in a wave of one shape
Z_VALUES = (("1", 1), ("2", 2), ("l-1", L - 1), ("filler", S.filler(b"shape z")))

Case = collections.namedtuple("Case", "name group circuit predicate after_run")


def le(x):
    return int(x).to_bytes(32, "little")


def filler(tag, k=0):
    """a fixed pseudo-random non-zero scalar"""
    x = int.from_bytes(hashlib.shake_256(b"shape-cases %s %d" % (tag, k)).digest(64), "little") % L
    assert x
    return x


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ what a predicate reads
def q_of(c): return len(c.rows)
def nvar_of(c): return 3 * c.n + c.m
def nnz_of(c): return sum(len(r) for r in c.rows)
def terms_of(c): return [t for r in c.rows for t in r]
def kind_count(c, kind): return sum(1 for pv, _ in terms_of(c) if pv >> 29 == kind)
def column_count(c, pv): return sum(1 for v, _ in terms_of(c) if v == pv)


def empty_runs(c):
    """[(first, last)] of the maximal runs of empty rows"""
    runs, start = [], None
    for r, row in enumerate(c.rows + [[None]]):
        if not row and start is None:
            start = r
        elif row and start is not None:
            runs.append((start, r - 1)); start = None
    return runs


def scan_blocks(keys):
    return cdiv(keys if keys else 1, SCAN_CHUNK)


def is_tall(c):
    return q_of(c) > nvar_of(c)


# ------------------------------------------------------------------------------------------------ the lockstep wave's old allocation
def al256(b):
    return (max(b, 1) + 255) & ~255


def wave_sizes(circuits):
    """(K N, qT, mT) of the block-diagonal instance a lockstep wave makes of these circuits (all of one padded size N)"""
    N = circuits[0].N
    assert all(c.N == N and c.n for c in circuits)
    return len(circuits) * N, sum(q_of(c) for c in circuits), sum(c.m for c in circuits)


def scan_scratch_overrun(circuits):
    """bytes by which the second scan of the transposition (qT keys, its scratch written into `counts`) ran past what the wave USED to lay out for `counts`:
    3 K N + mT + 2 words, rounded up to 256 bytes - what lay behind was `starts`, then `cursor`.  <= 0: it fitted."""
    KN, qT, mT = wave_sizes(circuits)
    return 4 * qT - al256(4 * (3 * KN + mT + 2))


# ------------------------------------------------------------------------------------------------ building blocks
def witness(n, m, tag):
    aL = [filler(tag + b" aL", i) for i in range(n)]
    aR = [filler(tag + b" aR", i) for i in range(n)]
    return {"n": n, "m": m, "aL": aL, "aR": aR, "aO": [a * b % L for a, b in zip(aL, aR)], "v": [filler(tag + b" v", j) for j in range(m)],
            "vb": [filler(tag + b" vb", j) for j in range(m)]}


def value_of(w):
    def val(pv):
        kind, idx = pv >> 29, pv & 0x1fffffff
        return 1 if kind == KIND_ONE else {KIND_L: w["aL"], KIND_R: w["aR"], KIND_O: w["aO"], KIND_V: w["v"]}[kind][idx]
    return val


def mixed_row(w, r, tag, kinds=(KIND_L, KIND_R, KIND_O, KIND_V)):
    """terms of row r over multipliers r, r + 1, r + 2 (mod n) of the three kinds and committed value r mod m - those of `kinds` the circuit has"""
    n, m, out = w["n"], w["m"], []
    for k in kinds:
        if k == KIND_V and m:
            out.append((VC.var(KIND_V, r % m), filler(tag + b" cv", r)))
        elif k != KIND_V and n:
            out.append((VC.var(k, (r + k) % n), filler(tag + b" c%d" % k, r)))
    return out


def circuit(name, w, rows, closed=True):
    """rows: lists of terms; closed: True (every row gets the constant that makes it hold), False (none does), or one flag per row"""
    flags = [closed] * len(rows) if isinstance(closed, bool) else list(closed)
    val = value_of(w)
    done = [VC._closed(t, val) if f else list(t) for t, f in zip(rows, flags)]
    return VC.Circuit(name, b"Shape " + name.encode(), w["n"], w["m"], w["aL"], w["aR"], w["aO"], done, w["v"], w["vb"])


# ------------------------------------------------------------------------------------------------ the catalogue
def _tall(name, n, m, q):
    w, tag = witness(n, m, name.encode()), name.encode()
    rows = []
    for r in range(q):
        row = [(VC.var(r % 3, r % n), filler(tag + b" c", r))] if n else []
        if m and (r % 2 or not n):
            row.append((VC.var(KIND_V, r % m), filler(tag + b" cv", r)))
        if n == 0 and r % 3 == 0:
            row.append((VC.var(KIND_V, (r + 1) % m), filler(tag + b" cw", r)))
        rows.append(row)
    return circuit(name, w, rows)


def _with_empty(name, q, empty):
    w, tag = witness(3, 1, name.encode()), name.encode()
    rows = [[] if r in empty else mixed_row(w, r, tag) for r in range(q)]
    return circuit(name, w, rows, [r not in empty for r in range(q)])


def _cancelling(name):
    """no constant term: even rows x c - x c over every kind in turn, odd rows of zero coefficients"""
    w, tag = witness(3, 1, name.encode()), name.encode()
    pool = [VC.var(k, i) for i in range(3) for k in (KIND_L, KIND_R, KIND_O)] + [VC.var(KIND_V, 0)]
    rows = []
    for r in range(8):
        x, c = pool[r % len(pool)], filler(tag + b" c", r)
        rows.append([(x, c), (x, L - c)] if r % 2 == 0 else [(x, 0), (pool[(r + 3) % len(pool)], 0)])
    return circuit(name, w, rows, False)


def _zero_sum(tag, r, count):
    cs = [filler(tag + b" k%d" % j, r) for j in range(count - 1)]
    return [(ONE, c) for c in cs] + [(ONE, (-sum(cs)) % L)]


def _constant_rows(name):
    w, tag = witness(3, 1, name.encode()), name.encode()
    only = (1, 3, 4)
    rows = [_zero_sum(tag, r, 3) if r in only else mixed_row(w, r, tag) for r in range(6)]
    return circuit(name, w, rows, [r not in only for r in range(6)])


def _forty(name):
    w, tag = witness(3, 1, name.encode()), name.encode()
    rows = [mixed_row(w, r, tag) + ([(ONE, filler(tag + b" k", j)) for j in range(39)] if r == 2 else []) for r in range(5)]
    return circuit(name, w, rows)


def _all_constants(name):
    w, tag = witness(2, 1, name.encode()), name.encode()
    return circuit(name, w, [_zero_sum(tag, r, 1 + r % 3) for r in range(5)], False)


def _hot(name, pv, other_kinds):
    w, tag = witness(3, 2, name.encode()), name.encode()
    rows = [[(pv, filler(tag + b" hot", r))] + mixed_row(w, r, tag, other_kinds[r % 2::2]) for r in range(600)]
    return circuit(name, w, rows)


def _dup(name, what):
    w, tag = witness(3, 1, name.encode()), name.encode()
    rows = [mixed_row(w, r, tag) for r in range(4)]
    if what == "five":
        rows[1] = [(VC.var(KIND_L, 1), filler(tag + b" d", j)) for j in range(5)]
    elif what == "zero":
        rows = [row[:1] + [(VC.var(KIND_R, r % 3), 0)] + row[1:] + [(VC.var(KIND_V, 0), 0)] for r, row in enumerate(rows)]
    else:
        rows = [[(pv, L - 1 if (r + j) % 2 == 0 else c) for j, (pv, c) in enumerate(row)] for r, row in enumerate(rows)]
    return circuit(name, w, rows)


def _without(name, kind):
    w, tag = witness(3, 2, name.encode()), name.encode()
    return circuit(name, w, [mixed_row(w, r, tag, tuple(k for k in (KIND_L, KIND_R, KIND_O, KIND_V) if k != kind)) for r in range(6)])


def _index_edges(name, n):
    w, tag, m = witness(n, 3, name.encode()), name.encode(), 3
    rows = [[(VC.var(k, 0), filler(tag + b" a", k)), (VC.var(k, n - 1), filler(tag + b" b", k))] for k in (KIND_L, KIND_R, KIND_O)]
    rows.append([(VC.var(KIND_V, 0), filler(tag + b" a", 3)), (VC.var(KIND_V, m - 1), filler(tag + b" b", 3))])
    rows.append([(VC.var(KIND_L, n - 1), filler(tag + b" e", 0)), (VC.var(KIND_O, 0), filler(tag + b" e", 1)), (VC.var(KIND_V, m - 1), filler(tag + b" e", 2))])
    return circuit(name, w, rows)


def _has_edges(c):
    used = {pv for pv, _ in terms_of(c)}
    return (all(VC.var(k, i) in used for k in (KIND_L, KIND_R, KIND_O) for i in (0, c.n - 1)) and all(VC.var(KIND_V, j) in used for j in (0, c.m - 1))
            and c.n > 1 and c.m > 1)


def _hot_predicate(pv):
    def p(c):
        kind = pv >> 29
        return (all(sum(1 for v, _ in row if v == pv) == 1 for row in c.rows) and column_count(c, pv) == q_of(c) == 600
                and kind_count(c, kind) == q_of(c) and (pv & 0x1fffffff) == (c.m - 1 if kind == KIND_V else 0))
    return p


def _run_crosses_a_count_block(c):
    return any(b - a + 1 >= 300 and a // COUNT_BLOCK != b // COUNT_BLOCK and a % COUNT_BLOCK and b + 1 < q_of(c) for a, b in empty_runs(c))


@functools.lru_cache(maxsize=None)
def catalogue():
    tall = lambda scans: (lambda c: is_tall(c) and (scan_blocks(q_of(c)), scan_blocks(nvar_of(c))) == scans)
    no_kind = lambda kind: (lambda c: kind_count(c, kind) == 0 and all(kind_count(c, k) for k in (KIND_L, KIND_R, KIND_O, KIND_V) if k != kind) and c.m > 0)
    cases = [
        ("tall/n1-q70", "tall", _tall("tall-n1-q70", 1, 0, 70), lambda c: is_tall(c) and (c.n, c.m, q_of(c)) == (1, 0, 70)),
        ("tall/n3-m2-q600", "tall", _tall("tall-n3-m2-q600", 3, 2, 600), lambda c: tall((1, 1))(c) and c.N == 4 > c.n and c.m == 2),
        ("tall/n1-m1-q2100", "tall", _tall("tall-n1-m1-q2100", 1, 1, 2100), tall((2, 1))),
        ("tall/n0-m2-q300", "tall", _tall("tall-n0-m2-q300", 0, 2, 300), lambda c: is_tall(c) and c.n == 0 and c.m == 2),
        ("wide/q0-n5", "wide", circuit("wide-q0-n5", witness(5, 0, b"wide-q0-n5"), []), lambda c: q_of(c) == 0 and c.m == 0 and c.n == 5),
        ("wide/q0-n2-m3", "wide", circuit("wide-q0-n2-m3", witness(2, 3, b"wide-q0-n2-m3"), []), lambda c: q_of(c) == 0 and c.m == 3 and c.n == 2),
        ("wide/q1-n700", "wide", circuit("wide-q1-n700", witness(700, 0, b"wide-q1-n700"),
                                         [[(VC.var(KIND_L, 0), filler(b"wide c", 0)), (VC.var(KIND_R, 699), filler(b"wide c", 1)), (VC.var(KIND_O, 350), filler(b"wide c", 2))]]),
         lambda c: q_of(c) == 1 and (scan_blocks(q_of(c)), scan_blocks(nvar_of(c))) == (1, 2)),
        ("empty/first", "empty", _with_empty("empty-first", 6, {0}), lambda c: empty_runs(c) == [(0, 0)]),
        ("empty/last", "empty", _with_empty("empty-last", 6, {5}), lambda c: empty_runs(c) == [(q_of(c) - 1, q_of(c) - 1)]),
        ("empty/run300", "empty", _with_empty("empty-run300", 530, set(range(200, 500))), _run_crosses_a_count_block),
        ("empty/all", "empty", circuit("empty-all", witness(2, 0, b"empty-all"), [[] for _ in range(10)], False), lambda c: q_of(c) == 10 and nnz_of(c) == 0),
        ("const/none", "const", _cancelling("const-none"), lambda c: kind_count(c, KIND_ONE) == 0 and nnz_of(c) > 0 and any(co == 0 for _, co in terms_of(c))),
        ("const/zero-sum-rows", "const", _constant_rows("const-zero-sum-rows"),
         lambda c: 0 < sum(1 for r in c.rows if r and all(pv == ONE for pv, _ in r)) < q_of(c) and all(len(r) > 1 for r in c.rows if all(pv == ONE for pv, _ in r))),
        ("const/forty", "const", _forty("const-forty"), lambda c: sorted(sum(1 for pv, _ in r if pv == ONE) for r in c.rows)[-2:] == [1, 40]),
        ("const/all", "const", _all_constants("const-all"), lambda c: kind_count(c, KIND_ONE) == nnz_of(c) > 0 and c.n > 0 and c.m > 0),
        ("hot/aL0", "hot", _hot("hot-aL0", VC.var(KIND_L, 0), (KIND_R, KIND_O, KIND_V)), _hot_predicate(VC.var(KIND_L, 0))),
        ("hot/v-last", "hot", _hot("hot-v-last", VC.var(KIND_V, 1), (KIND_L, KIND_R, KIND_O)), _hot_predicate(VC.var(KIND_V, 1))),
        ("dup/five", "dup", _dup("dup-five", "five"), lambda c: any(len(r) == 6 and len({pv for pv, _ in r[:5]}) == 1 and len({co for _, co in r[:5]}) == 5 for r in c.rows)),
        ("dup/zero-coef", "dup", _dup("dup-zero-coef", "zero"), lambda c: all(sum(1 for pv, co in r if co == 0 and pv != ONE) == 2 for r in c.rows)),
        ("dup/l-1", "dup", _dup("dup-l-1", "l-1"), lambda c: all(any(co == L - 1 and pv != ONE for pv, co in r) for r in c.rows)),
        ("sect/no-left", "sect", _without("sect-no-left", KIND_L), no_kind(KIND_L)),
        ("sect/no-right", "sect", _without("sect-no-right", KIND_R), no_kind(KIND_R)),
        ("sect/no-output", "sect", _without("sect-no-output", KIND_O), no_kind(KIND_O)),
        ("sect/no-committed", "sect", _without("sect-no-committed", KIND_V), no_kind(KIND_V)),
        ("edge/n7", "edge", _index_edges("edge-n7", 7), lambda c: _has_edges(c) and c.n == c.N - 1),
        ("edge/n8", "edge", _index_edges("edge-n8", 8), lambda c: _has_edges(c) and c.n == c.N),
    ]
    out = []
    for name, group, circ, pred in cases:
        runs = empty_runs(circ)
        after = next((b + 1 for a, b in runs if b + 1 < q_of(circ)), None)
        out.append(Case(name, group, circ, pred, after))
    return tuple(out)


def names():
    return [c.name for c in catalogue()]


def by_name(name):
    return {c.name: c for c in catalogue()}[name]


def lockstep_cases():
    """the cases a lockstep wave takes: a circuit without multipliers goes the single path"""
    return [c for c in catalogue() if c.circuit.n > 0]


# ------------------------------------------------------------------------------------------------ the model
def model(circ, z):
    """flattened_constraints(z) of the circuit's rows in integers: (w_L, w_R, w_O, w_V, w_c)"""
    return S.weights(circ.rows, circ.n, circ.m, z)


def model_bytes(circ, z):
    wL, wR, wO, wV, wc = model(circ, z)
    return [le(x) for x in wL], [le(x) for x in wR], [le(x) for x in wO], [le(x) for x in wV], le(wc)


def delta(circ, y, z):
    """<y^-n o w_R, w_L>"""
    wL, wR, _, _, _ = model(circ, z)
    yi, acc, p = S.inv(y), 0, 1
    for a, b in zip(wL, wR):
        acc, p = (acc + p * a * b) % L, p * yi % L
    return acc


# ------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def gens():
    return O.Gens(GENS_CAPACITY)


def seed(k):
    return hashlib.sha256(b"shape-cases seed %d" % k).digest()


def vb_of(circ):
    return b"".join(le(x) for x in circ.vb)


def v_of(circ):
    return b"".join(le(x) for x in circ.v)


@functools.lru_cache(maxsize=None)
def reference(name, k=0, flags=0):
    """(proof, transcript state after) of the oracle prover for the case under seed(k), computed once and shared"""
    circ = by_name(name).circuit
    rc, proof, after = O.prove(gens(), circ.state, S.oracle_circuit(circ), vb_of(circ), seed(k), flags | O.FLAG_FAST_MSM)
    assert rc == 0, name
    return proof, after


def oracle_verify(circ, proof, flags=0, rows=None):
    inst = circ.inst if rows is None else circ.instance(rows)
    return O.verify(gens(), circ.state, O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef), circ.V, proof,
                    S.SEED, flags)


# ------------------------------------------------------------------------------------------------ one row changed
def break_row(circ, r):
    """the rows with row r changed so that the witness no longer satisfies it: its (first) constant term plus one; a row without a constant: its first
    non-zero coefficient plus one (the variable's value is not zero).  An empty row cannot be broken: None"""
    row = list(circ.rows[r])
    if not row:
        return None
    at = next((k for k, (pv, _) in enumerate(row) if pv == ONE), None)
    if at is None:
        val = value_of({"aL": circ.aL, "aR": circ.aR, "aO": circ.aO, "v": circ.v})
        at = next(k for k, (pv, _) in enumerate(row) if val(pv) % L)
    row[at] = (row[at][0], (row[at][1] + 1) % L)
    return circ.rows[:r] + [row] + circ.rows[r + 1:]


def last_nonempty_row(circ):
    return next((r for r in range(q_of(circ) - 1, -1, -1) if circ.rows[r]), None)


def tampered_rows(circ):
    """THE pinned statement tamper of a case: break_row of its last non-empty row - the constant where there is one, which pins w_c on this shape.  A circuit
    without any term has no statement to tamper with: None"""
    r = last_nonempty_row(circ)
    return None if r is None else break_row(circ, r)


def rows_to_break(case):
    """row 0, row q - 1 and the row right after the (first) run of empty rows, where they hold a term"""
    c = case.circuit
    want = [r for r in (0, q_of(c) - 1, case.after_run) if r is not None and 0 <= r < q_of(c) and c.rows[r]]
    return sorted(set(want))


# ------------------------------------------------------------------------------------------------ templates
def template_parts(circ):
    """(FlatInstance, WitnessProgram) that make the circuit a template: multiplier i has a_L = aL_i * 1 and a_R = aR_i * 1 - one term on Variable One each, the
    values appended to the coefficient table behind those of the rows (which keep their indices).  The rows are the circuit's own, entry for entry."""
    import ctypes as C
    assert circ.n > 0
    base = circ.inst
    coefs = [int.from_bytes(base.coef[32 * k:32 * k + 32], "little") for k in range(base.ncoef)]
    index = {c: k for k, c in enumerate(coefs)}
    tv, tc = [], []
    for a, b in zip(circ.aL, circ.aR):
        for x in (a, b):
            if x not in index:
                index[x] = len(coefs); coefs.append(x)
            tv.append(ONE); tc.append(index[x])
    keep = [np.ascontiguousarray(base.row_ptr), np.ascontiguousarray(base.term_var), np.ascontiguousarray(base.term_coef),
            C.create_string_buffer(b"".join(le(c) for c in coefs), 32 * len(coefs) + 1)]
    wit = [C.create_string_buffer(x, len(x) + 1) for x in (base.aL, base.aR, base.aO)]
    view = bpg.R1CSInstance()
    view.n, view.q, view.m, view.nnz, view.ncoef = base.n, base.q, base.m, base.nnz, len(coefs)
    view.aL, view.aR, view.aO = [C.cast(w, C.c_void_p).value for w in wit]
    view.row_ptr, view.term_var, view.term_coef = keep[0].ctypes.data, keep[1].ctypes.data if base.nnz else None, keep[2].ctypes.data if base.nnz else None
    view.coef = C.cast(keep[3], C.c_void_p).value
    inst = bpg.FlatInstance(view, v=v_of(circ), v_blinding=vb_of(circ), commitments=circ.V)
    return inst, bpg.WitnessProgram(list(range(2 * circ.n + 1)), tv, tc)


def assembled(name, label, parts, flat):
    """the circuit a host-assembled repeat or join stands for: parts = [(circuit, count)] in order, flat = (row_ptr, term_var, term_coef, coef bytes) as
    bpg.test_template_repeat_instance / test_template_join_instance return them -> a verify_cases.Circuit over the concatenated witnesses"""
    row_ptr, tv, tc, coef = flat
    cs = [int.from_bytes(coef[32 * k:32 * k + 32], "little") for k in range(len(coef) // 32)]
    rows = [[(int(tv[e]), cs[int(tc[e])]) for e in range(int(row_ptr[r]), int(row_ptr[r + 1]))] for r in range(len(row_ptr) - 1)]
    cat = lambda f: [x for c, k in parts for _ in range(k) for x in f(c)]
    n, m = sum(c.n * k for c, k in parts), sum(c.m * k for c, k in parts)
    return VC.Circuit(name, label, n, m, cat(lambda c: c.aL), cat(lambda c: c.aR), cat(lambda c: c.aO), rows, cat(lambda c: c.v), cat(lambda c: c.vb))
