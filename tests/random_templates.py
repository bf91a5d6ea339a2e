"""Seeded random circuits for the template tests (tests/test_template_random_host.py, tests/test_template_random_gpu.py): the generator and the model.

An item is fully determined by (shape_seed, value_seed): ALL structure - how many committed values and multipliers, which terms every linear combination
names under which coefficients, where the bit hints and the parameter rows sit - comes from one random.Random stream, and all committed and public input
VALUES from another.  One shape can therefore be assembled with any number of witnesses: a template from one value seed, fresh witnesses from others.

`shape(shape_seed)` draws the structure as plain Python data (a Shape: a list of steps over symbolic references); `evaluate(shape, v, inputs)` is the MODEL:
Python integers mod l read straight off that data, with nothing from the code under test; `item(p, shape_seed, value_seed)` drives a prover through its
public surface (commit, multiply, allocate_bit, constrain, mark_param_row, input) and returns the model's numbers beside the variables the prover made.

What the shapes are made of (and what the gadget circuits of the other template tests never are):
  * m in 0..5 committed values; canonical values, three in ten from {0, 1, l - 1, 2^64 - 1, 2^252}
  * n from NS: 1, 2, 3, sizes just above a power of two, sizes of more than one wavefront of lanes
  * linear combinations of 0, 1, 1, 2, 3 or 6 terms (the empty one is the value 0); coefficients from {0, 1, -1, 2, -2} half of the time (zero is what the
    packer drops, +1 and -1 are its product-free classes), uniform otherwise; a term is One (15%), one of the last three variables made (45% of the rest:
    the interpreter's register copy of the previous multiplier) or any earlier variable (cross-segment reads, several new sources in one multiplier, diamonds)
  * in a fifth of the multipliers the right list IS the left list (WIT_SAME_AS_LEFT)
  * a fifth of the steps are hint runs over an arbitrary linear combination: bits 0..k-1 (k <= 8), or 1-4 sorted sparse bits anywhere in 0..255
  * after three steps in ten a row `lc - value(lc)`, marked as a parameter row: many parameter rows per item.  The value assign() takes for the row is the sum
    of ALL its One terms: the One terms lc itself drew, minus the value
  * with public=: 1-4 public inputs (template_inputs_cases.Public), which join the pool of variables and so appear in left and right lists, as hint
    sources and in rows, under general, +-1 and zero coefficients"""
import functools
import random

import bulletproofs_gadgets_amd as bpg
from bulletproofs_gadgets_amd import workloads

L = bpg.L
LC = bpg.LinearCombination
NS = [1, 2, 3, 5, 6, 8, 17, 33, 40, 64, 65, 100, 200]
EDGE_VALUES = [0, 1, L - 1, 2**64 - 1, 2**252]
EDGE_COEFS = [0, 1, L - 1, 2, L - 2]
TERM_COUNTS = [0, 1, 1, 2, 3, 6]
ONE = ("one", 0)


def sc(x):
    return (x % L).to_bytes(32, "little")


class Shape:
    """The structure of one item.  A reference is (kind, index): ("one", 0), ("v", i) committed value i, ("in", i) public input i, ("L" | "R" | "O", i) of
    multiplier i.  A linear combination is a list of (coefficient, reference).
    steps: ("mul", left, right)  right may BE left (the same list object)
           ("bit", source, bit)  a hinted multiplier: a_L = 1 - b, a_R = b, a_O = 0 with b = bit `bit` of the canonical value of source
           ("row", lc)           the parameter row lc - value(lc)"""
    def __init__(self, seed, n, m, n_inputs, steps):
        self.seed, self.n, self.m, self.n_inputs, self.steps = seed, n, m, n_inputs, steps
        self.rows = sum(1 for s in steps if s[0] == "row")
        self.hints = sum(1 for s in steps if s[0] == "bit")
        self.q = self.rows + 2 * (n - self.hints)             # multiply() constrains its two inputs; a hinted multiplier adds no row of its own
        self.hint_bits = [s[2] for s in steps if s[0] == "bit"]
        lcs = [x for s in steps for x in (s[1:3] if s[0] == "mul" else s[1:2])]
        self.empty_lcs = sum(1 for lc in lcs if not lc)
        self.zero_coefs = sum(1 for lc in lcs for c, _ in lc if c == 0)
        self.same_as_left = sum(1 for s in steps if s[0] == "mul" and s[1] is s[2])


@functools.lru_cache(maxsize=None)
def shape(shape_seed, public=False):
    """the structure of shape `shape_seed`, without (the default) or with public inputs - two different families: the inputs join the pool the terms are drawn from.  Drawn once and kept: nobody changes a Shape."""
    S = random.Random("random-template-shape-%d-%d" % (shape_seed, 1 if public else 0))
    m = S.randrange(6)
    n = S.choice(NS)
    n_inputs = S.randint(1, 4) if public else 0
    pool = [("v", i) for i in range(m)] + [("in", i) for i in range(n_inputs)]      # every variable made so far, in the order it was made

    def coef():
        return S.choice(EDGE_COEFS) if S.random() < 0.5 else S.randrange(L)

    def term():
        if not pool or S.random() < 0.15:
            return ONE
        if S.random() < 0.45:
            return S.choice(pool[-3:])
        return S.choice(pool)

    def lc():
        return [(coef(), term()) for _ in range(S.choice(TERM_COUNTS))]

    steps, made = [], 0
    while made < n:
        if S.random() < 0.2:
            src = lc()
            bits = list(range(S.randint(1, 8))) if S.random() < 0.5 else sorted(S.sample(range(256), S.randint(1, 4)))
            for b in bits[:n - made]:
                steps.append(("bit", src, b))
                pool += [("L", made), ("R", made), ("O", made)]
                made += 1
        else:
            left = lc()
            right = left if S.random() < 0.2 else lc()
            steps.append(("mul", left, right))
            pool += [("L", made), ("R", made), ("O", made)]
            made += 1
        if S.random() < 0.3:
            steps.append(("row", lc()))
    return Shape(shape_seed, n, m, n_inputs, steps)


def describe(sh):
    """the shape as text, one step a line: what to print beside the schedule JSON of a failing seed"""
    name = lambda ref: "1" if ref == ONE else "%s%d" % ref
    show = lambda lc: " + ".join("%s*%s" % (c if c < 1 << 16 else "(l-%d)" % (L - c) if L - c < 1 << 16 else "c", name(ref)) for c, ref in lc) or "0"
    lines, made = ["shape %d: n = %d, m = %d, q = %d, %d inputs, %d hinted, %d parameter rows" % (sh.seed, sh.n, sh.m, sh.q, sh.n_inputs, sh.hints, sh.rows)], 0
    for step in sh.steps:
        if step[0] == "row":
            lines.append("      row  %s - value" % show(step[1]))
        elif step[0] == "bit":
            lines.append("%4d  bit %d of  %s" % (made, step[2], show(step[1]))); made += 1
        else:
            lines.append("%4d  (%s) x (%s)" % (made, show(step[1]), "the same list" if step[2] is step[1] else show(step[2]))); made += 1
    return "\n".join(lines)


def values(sh, value_seed):
    """(the m committed values, the public input values) of witness `value_seed` of the shape: integers below l"""
    V = random.Random("random-template-values-%d" % value_seed)
    draw = lambda: V.choice(EDGE_VALUES) if V.random() < 0.3 else V.randrange(L)
    return [draw() for _ in range(sh.m)], [draw() for _ in range(sh.n_inputs)]


def evaluate(sh, v, inputs=(), given=None):
    """THE MODEL.  -> (a_L, a_R, a_O, the value of every row's linear combination, the value of every hinted multiplier's source): integers mod l.
    given: {(kind, index): value} - multiplier variables every READER takes from this table (the values a caller hands to a checkpointed template, right or
    wrong); what the multipliers themselves hold is still computed."""
    val = {"L": [], "R": [], "O": [], "v": list(v), "in": list(inputs), "one": [1]}
    given = given or {}

    def value(lc):
        return sum(c * (given[ref] if ref in given else val[ref[0]][ref[1]]) for c, ref in lc) % L

    rows, sources = [], []
    for step in sh.steps:
        if step[0] == "row":
            rows.append(value(step[1]))
            continue
        if step[0] == "bit":
            sources.append(value(step[1]))
            b = (sources[-1] >> step[2]) & 1
            left, right = 1 - b, b
        else:
            left = value(step[1])
            right = left if step[2] is step[1] else value(step[2])
        val["L"].append(left); val["R"].append(right); val["O"].append(left * right % L)
    return val["L"], val["R"], val["O"], rows, sources


def first_mismatch(sh, v, inputs, ck_refs, ck_values):
    """the lowest position in the checkpoint list whose given value is not what the circuit computes when every reader takes the GIVEN values; None: all hold"""
    aL, aR, aO = evaluate(sh, v, inputs, dict(zip(ck_refs, ck_values)))[:3]
    got = {"L": aL, "R": aR, "O": aO}
    for k, (ref, x) in enumerate(zip(ck_refs, ck_values)):
        if got[ref[0]][ref[1]] != x % L:
            return k
    return None


def checkpoint_set(shape_seed, density, refs):
    """a random subset of `refs` (each with probability `density`; 1.0: all; never empty unless refs is), shuffled -> (the subset, the stream that drew it)"""
    R = random.Random("random-template-checkpoints-%d-%s" % (shape_seed, density))
    cks = [r for r in refs if density >= 1.0 or R.random() < density]
    if refs and not cks:
        cks = [R.choice(refs)]
    R.shuffle(cks)
    return cks, R


def mul_refs(n):
    """all 3 n multiplier variables as references, multiplier by multiplier"""
    return [(k, i) for i in range(n) for k in "LRO"]


class Item:
    """one item as it stands in a prover: the model's a_L, a_R, a_O (integers), the parameter rows (indices in the prover) with the constants assign() takes for
    them, the public input values in input order, and the Variables the prover handed out"""
    def __init__(self, sh, v, inputs, aL, aR, aO, rows, params, var_of):
        self.shape, self.v, self.input_ints, self.aL, self.aR, self.aO, self.rows, self.params, self.var_of = sh, v, inputs, aL, aR, aO, rows, params, var_of
        self.inputs = [sc(x) for x in inputs]
        self.values = b"".join(sc(x) for x in v)

    def witness(self):
        return tuple(b"".join(sc(x) for x in a) for a in (self.aL, self.aR, self.aO))

    def mul_refs(self):
        return mul_refs(self.shape.n)

    def checkpoints(self, refs):
        """(the prover's Variables, the model's values as bytes) of the referenced multiplier variables"""
        at = {"L": self.aL, "R": self.aR, "O": self.aO}
        return [self.var_of[r] for r in refs], [sc(at[k][i]) for k, i in refs]


def item(p, shape_seed, value_seed, public=None, blind_tag=None):
    """Appends item (shape_seed, value_seed) to prover p: its commitments, its multipliers, its rows.
    public: None (the family without inputs), or a template_inputs_cases.Public over p - as_inputs=True names the public values as inputs (the template),
    as_inputs=False bakes them in as constants (the yardstick assembly)."""
    sh = shape(shape_seed, public is not None)
    v, inputs = values(sh, value_seed)
    aL, aR, aO, row_values, sources = evaluate(sh, v, inputs)
    tag = blind_tag or "random-template-%d-%d" % (shape_seed, value_seed)
    lcs = {ONE: LC.of(1)}
    var_of = {}
    for i, x in enumerate(v):
        var_of[("v", i)] = p.commit(sc(x), workloads.blinding(tag, i))[1]
        lcs[("v", i)] = LC.of(var_of[("v", i)])
    for i, x in enumerate(inputs):
        lcs[("in", i)] = public(sc(x))

    def build(lc):
        return LC([(var, sc(c * int.from_bytes(c0, "little"))) for c, ref in lc for var, c0 in lcs[ref].terms])

    rows, params, made, hinted = [], [], 0, 0
    for step in sh.steps:
        if step[0] == "row":
            lc = step[1]
            value = row_values[len(rows)]
            p.constrain(build(lc) - sc(value))
            row = p.num_constraints() - 1
            p.mark_param_row(row)
            rows.append(row)
            params.append(sc(sum(c for c, ref in lc if ref == ONE) - value))     # ALL the row's One terms, not just -value
            continue
        if step[0] == "bit":
            out = p.allocate_bit(build(step[1]), step[2], sc(sources[hinted]))
            hinted += 1
        else:
            left = build(step[1])
            out = p.multiply(left, left if step[2] is step[1] else build(step[2]))
        for k, var in zip("LRO", out):
            var_of[(k, made)] = var
            lcs[(k, made)] = LC.of(var)
        made += 1
    return Item(sh, v, inputs, aL, aR, aO, rows, params, var_of)
