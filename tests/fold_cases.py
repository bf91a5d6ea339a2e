"""The generator-fold kernels of the inner-product argument (csrc/hip/k_ipa.cuh) at CHOSEN scalars: the catalogue of cases and an integer model of the three
recodings that feed the kernels (csrc/host/fold_plan.hpp), shared by test_fold_cases_host.py (which pins the catalogue without a device) and
test_fold_kernels_gpu.py (which runs every case through bpg_test_fold).  Plain Python integers throughout; nothing here imports the package's recoders.

A case is (name, sG, sH, u_ch): the scalars of terms 1..nterms of the G side and of the H side, and the padding factor of a first group.  The case lists are
per recoding - bitmap_cases (k_fold_points, _reg, _quad, _split), steps_cases (k_fold_points_quadw, _regw), wnaf_cases (k_fold_points_wnaf) - and are
functions of the number of terms, because a fold group of r rounds has 2^r - 1 terms."""
import functools
import hashlib

L = 2**252 + 27742317777372353535851937790883648493

KERNELS = ("k_fold_points_wnaf", "k_fold_points_quadw", "k_fold_points_quad", "k_fold_points_split", "k_fold_points_regw", "k_fold_points_reg", "k_fold_points")
# (BPG_FOLD_WNAF, BPG_FOLD_PARTS) of the contexts k_fold_points_wnaf is run under: widths 3, 5, 8 by parts 1, 2, 8, and three more so that every width 3..8
# and every number of parts occurs
WNAF_PROFILES = ((3, 1), (3, 2), (3, 8), (5, 1), (5, 2), (5, 8), (8, 1), (8, 2), (8, 8), (4, 4), (6, 2), (7, 1))


def sc(v):
    assert 0 <= v < L, hex(v)
    return v.to_bytes(32, "little")


# ---------------------------------------------------------------------------------------------------- integer models of the recodings
def wnaf(s, w):
    """Width-w non-adjacent form of s >= 0: 256 digits, each 0 or odd with |d| < 2^(w-1), least significant first.  w = 2 is the plain NAF."""
    d = [0] * 256
    k, i = s, 0
    while k:
        if k & 1:
            dig = k & ((1 << w) - 1)
            if dig >= 1 << (w - 1):
                dig -= 1 << w
            d[i] = dig
            k -= dig
        k >>= 1
        i += 1
    return d


def naf(s):
    return wnaf(s, 2)


def top_of(d):
    """Position of the most significant non-zero digit, -1 for none."""
    return max((k for k, v in enumerate(d) if v), default=-1)


def value_of(d):
    return sum(v << k for k, v in enumerate(d))


def part_bits(parts):
    return (254 + parts - 1) // parts


def cut(s, parts):
    """s as `parts` pieces of L = ceil(254 / parts) bits, least significant piece first."""
    Lb = part_bits(parts)
    return [(s >> (p * Lb)) & ((1 << Lb) - 1) for p in range(parts)]


def step_list(scalars):
    """The width-4 step list of one class (fold_recode_steps): positions from the most significant down, the terms in order within a position, the doublings of
    the identity ahead of the first step skipped.  Returns ([(doublings before the addition, term, |digit|, negative)], tail = doublings after the last step)."""
    dg = [wnaf(s, 4) for s in scalars]
    top = max(top_of(d) for d in dg)
    steps, pending = [], 0
    for k in range(top, -1, -1):
        if steps:
            pending += 1
        for q, d in enumerate(dg):
            if d[k]:
                steps.append((pending, q, abs(d[k]), d[k] < 0))
                pending = 0
    return steps, pending


def class_scalars(case, first):
    """The scalars a launch recodes: sG, sH, and in a first group their products with u_ch (the class of the padding generators), whatever n is."""
    _, sG, sH, u = case
    out = [list(sG), list(sH)]
    if first:
        out += [[s * u % L for s in sG], [s * u % L for s in sH]]
    return out


def predict_bitmap(case, first):
    """Evidence of the bitmap kernels: top = the highest NAF digit position over every scalar recoded; and the non-zero digits (additions per lane of a class)."""
    digits = [naf(s) for cls in class_scalars(case, first) for s in cls]
    return {"top": max(top_of(d) for d in digits), "adds": sum(1 for d in digits for v in d if v)}


def predict_wnaf(case, first, w, parts):
    digits = [wnaf(p, w) for cls in class_scalars(case, first) for s in cls for p in cut(s, parts)]
    return {"top": max(top_of(d) for d in digits), "adds": sum(1 for d in digits for v in d if v), "wnaf": w, "parts": parts, "part_bits": part_bits(parts)}


def predict_steps(case):
    """Evidence of the step kernels, and what the lists hold: nsteps, tail per class (G, H); the largest doublings field; the additions."""
    _, sG, sH, _ = case
    lists = [step_list(sG), step_list(sH)]
    return {"nsteps": [len(st) for st, _ in lists], "tail": [tail for _, tail in lists],
            "max_doublings": max((s[0] for st, _ in lists for s in st), default=0), "adds": sum(len(st) for st, _ in lists)}


# ---------------------------------------------------------------------------------------------------- scalar builders
def named():
    """The named values: small ones, the ends of the range, its middle, the densest bit patterns, bits on both sides of the 32-bit word edges of the bitmaps."""
    v = {"0": 0, "1": 1, "2": 2, "3": 3, "l-1": L - 1, "l-2": L - 2, "(l-1)/2": (L - 1) // 2, "(l+1)/2": (L + 1) // 2,
         "2^252": 1 << 252, "2^252+1": (1 << 252) + 1, "2^252-1": (1 << 252) - 1,
         "0x0555..5": int("0" + "5" * 63, 16), "0x0aaa..a": int("0" + "a" * 63, 16),
         "2^31": 1 << 31, "2^32-1": (1 << 32) - 1, "2^32": 1 << 32, "2^223": 1 << 223, "2^224": 1 << 224, "7*2^200": 7 << 200}
    for s in v.values():
        assert 0 <= s < L
    return v


def width_extreme(w, pick):
    """sum_j pick(j) 2^(w j) with pick(j) odd and |pick(j)| < 2^(w-1): a digit every w positions, so the width-w NAF of the value is these digits.  The top
    digit (the last position not above 252) takes pick's value where that keeps 0 <= s < l, else the largest odd positive digit that does, else none."""
    half = 1 << (w - 1)
    J = 252 // w + 1
    for j in range(J):
        assert pick(j) & 1 and abs(pick(j)) < half
    low = sum(pick(j) << (w * j) for j in range(J - 1))
    for top in [pick(J - 1)] + list(range(half - 1, 0, -2)):
        s = low + (top << (w * (J - 1)))
        if 0 <= s < L:
            return s
    assert 0 <= low < L
    return low


def pick_max(w):
    return lambda j: (1 << (w - 1)) - 1


def pick_min(w):
    return lambda j: -((1 << (w - 1)) - 1)


def pick_alt(w, phase):
    return lambda j: ((1 << (w - 1)) - 1) * (1 if (j + phase) & 1 else -1)


def pick_turn(j):
    """width 4: every multiple and sign of the tables in turn"""
    return (1, -1, 3, -3, 5, -5, 7, -7)[j % 8]


def width_patterns(w):
    """(name, scalar): all +max, all -max, the two alternations, and for w = 4 every digit value in turn"""
    out = [("w%d+max" % w, width_extreme(w, pick_max(w))), ("w%d-max" % w, width_extreme(w, pick_min(w))),
           ("w%d+-" % w, width_extreme(w, pick_alt(w, 0))), ("w%d-+" % w, width_extreme(w, pick_alt(w, 1)))]
    if w == 4:
        out.append(("w4turn", width_extreme(4, pick_turn)))
    return out


def parts_extreme(w, parts, kind):
    """Scalars shaped for the cut into `parts` pieces of Lb bits that k_fold_points_wnaf uses.  low: only the lowest piece non-zero (digits +max every w
    positions); high: only the highest piece non-zero, the largest value l allows there; ones: one piece of 2^Lb - 1, whose recoding carries a digit into
    position Lb; every+ / every-: every piece at its extreme (+max digits every w positions / 2^Lb less those: a digit at Lb over -max digits), the top
    piece cut down to the bits below 2^252."""
    Lb, m = part_bits(parts), (1 << (w - 1)) - 1
    comb = sum(m << (w * j) for j in range((Lb - w + 1) // w + 1) if w * j + w - 1 <= Lb)          # < 2^Lb
    assert comb < 1 << Lb
    shift = (parts - 1) * Lb
    if kind == "low":
        s = comb if parts > 1 else comb & ((1 << 252) - 1)
    elif kind == "high":
        s = ((L - 1) >> shift) << shift
    elif kind == "ones":
        s = (1 << Lb) - 1 if parts > 1 else (1 << 252) - 1          # one piece: 2^254 - 1 is no scalar; the largest all-ones value below l
    elif kind in ("every+", "every-"):
        piece = comb if kind == "every+" else (1 << Lb) - comb
        assert 0 < piece < 1 << Lb
        s = sum(piece << (p * Lb) for p in range(parts)) & ((1 << 252) - 1)
    else:
        raise ValueError(kind)
    assert 0 <= s < L
    return s


PARTS_KINDS = ("low", "high", "ones", "every+", "every-")


def ordinary(k):
    """A fixed scalar with nothing special about it."""
    return int.from_bytes(hashlib.sha512(b"fold case %d" % k).digest(), "little") % L


# ---------------------------------------------------------------------------------------------------- case lists
def _fill(vals, nterms, rot=0):
    return [vals[(t + rot) % len(vals)] for t in range(nterms)]


def _named_cases(nterms):
    """One named value in every term of the G side, another in every term of the H side: each value comes up on both sides."""
    items = list(named().items())
    return [("named %s | %s" % (a[0], b[0]), [a[1]] * nterms, [b[1]] * nterms, 1) for a, b in zip(items, items[7:] + items[:7])]


def _mixed_cases(nterms, dense):
    v = named()
    tops = [1, L - 1, 0, 1 << 252, 2, 1 << 31, (1 << 252) + 1, 0, 3, 1 << 224, dense]
    return [("all zero", [0] * nterms, [0] * nterms, 1), ("all one", [1] * nterms, [1] * nterms, 1), ("all two", [2] * nterms, [2] * nterms, 1),
            ("mixed tops", _fill(tops, nterms), _fill(tops[::-1], nterms), 1),
            ("mixed tops, rotated", _fill(tops, nterms, 3), _fill(tops, nterms, 5), 1),
            ("one long term among zeros", [0] * (nterms - 1) + [L - 1], [v["2^252+1"]] + [0] * (nterms - 1), 1),
            ("G zero, H dense", [0] * nterms, [dense] * nterms, 1),
            ("G dense, H zero", [dense] * nterms, [0] * nterms, 1),
            ("G one, H dense", [1] * nterms, [dense] * nterms, 1),
            ("all different", [ordinary(t) for t in range(nterms)], [ordinary(100 + t) for t in range(nterms)], 1)]


def _class_b_cases(nterms):
    """Edges in the class of the padding generators of a first group: s is ordinary and u_ch = e / s, so that s * u_ch is the edge e."""
    v = named()
    s = ordinary(7)
    out = [("class B: s*u_ch = %s" % name, [s] * nterms, [s] * nterms, v[name] * pow(s, -1, L) % L)
           for name in ("0", "1", "2", "l-1", "2^252", "2^252+1", "0x0555..5", "2^32-1", "2^224")]
    out.append(("class B: u_ch = 1", [ordinary(t) for t in range(nterms)], [v["l-1"]] * nterms, 1))
    out.append(("class B: edges in class A, ordinary in B", [v["2^252"]] * nterms, [v["1"]] * nterms, ordinary(9)))
    return out


@functools.lru_cache(maxsize=None)
def bitmap_cases(nterms, first):
    """Cases of the plain-NAF kernels.  The densest NAF is 0x0555..5: a digit at every second position."""
    cases = _named_cases(nterms) + _mixed_cases(nterms, named()["0x0555..5"])
    if first:
        cases += _class_b_cases(nterms)
    return _checked(cases, nterms)


@functools.lru_cache(maxsize=None)
def steps_cases(nterms):
    """Cases of the width-4 step kernels (groups after the first only: u_ch is not used).  The densest list: a digit every four positions, 64 per term."""
    pats = width_patterns(4)
    dense = dict(pats)["w4-max"]
    cases = _named_cases(nterms) + _mixed_cases(nterms, dense)
    cases += [("%s | %s" % (a[0], b[0]), [a[1]] * nterms, [b[1]] * nterms, 1) for a, b in zip(pats, pats[2:] + pats[:2])]
    cases.append(("w4 patterns term by term", _fill([p[1] for p in pats], nterms), _fill([p[1] for p in pats], nterms, 2), 1))
    # every (multiple, sign) of the tables in a pattern one can read off: term t adds only the multiple 2 (t mod 4) + 1, sign by the side and the term
    one = lambda d: width_extreme(4, lambda j: d) if d > 0 else width_extreme(4, lambda j: d if j < 62 else 1)
    cases.append(("one multiple per term", [one((1, 3, 5, 7)[t % 4] * (1 if t & 4 else -1)) for t in range(nterms)],
                  [one((7, 5, 3, 1)[t % 4] * (-1 if t & 4 else 1)) for t in range(nterms)], 1))
    return _checked(cases, nterms)


@functools.lru_cache(maxsize=None)
def wnaf_cases(w, parts, nterms, first):
    """Cases of k_fold_points_wnaf under width w and the cut into `parts` pieces."""
    pats = width_patterns(w)
    cases = _named_cases(nterms) + _mixed_cases(nterms, dict(pats)["w%d-max" % w])
    cases += [("%s | %s" % (a[0], b[0]), [a[1]] * nterms, [b[1]] * nterms, 1) for a, b in zip(pats, pats[1:] + pats[:1])]
    px = [("parts %s" % k, parts_extreme(w, parts, k)) for k in PARTS_KINDS]
    cases += [("%s | %s" % (a[0], b[0]), [a[1]] * nterms, [b[1]] * nterms, 1) for a, b in zip(px, px[2:] + px[:2])]
    cases.append(("parts patterns term by term", _fill([p[1] for p in px], nterms), _fill([p[1] for p in px], nterms, 3), 1))
    if first:
        cases += _class_b_cases(nterms)
        s = ordinary(11)
        cases += [("class B: s*u_ch = %s" % name, [s] * nterms, [s] * nterms, e * pow(s, -1, L) % L) for name, e in (pats[1], px[2], px[4])]
    return _checked(cases, nterms)


def _checked(cases, nterms):
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names), names
    for name, sG, sH, u in cases:
        assert len(sG) == nterms and len(sH) == nterms, name
        assert all(0 <= s < L for s in sG + sH + [u]), name
    return tuple((name, tuple(sG), tuple(sH), u) for name, sG, sH, u in cases)


# ---------------------------------------------------------------------------------------------------- the reference
def padding(i, t, Mr, n, first):
    """Lane i takes term t (1..nterms) in class B: a padding generator of a first group."""
    return bool(first) and i + t * Mr >= n


def wave_classes(Mr, nterms, n, first, lanes_per_output=1):
    """How the waves of a launch with one lane (or four) per output see the classes: (waves whose lanes all agree on the side and on the class of every
    term, waves that do not) - the kernels take scalar digit loads in the former and per-lane ones in the latter."""
    per_wave = 64 // lanes_per_output
    uniform = mixed = 0
    for w0 in range(0, 2 * Mr, per_wave):
        keys = set()
        for t in range(w0, w0 + per_wave):
            t = min(t, 2 * Mr - 1)                                # idle lanes shadow the last output
            i = t % Mr
            keys.add((t >= Mr, tuple(padding(i, q, Mr, n, first) for q in range(1, nterms + 1))))
        uniform, mixed = uniform + (len(keys) == 1), mixed + (len(keys) > 1)
    return uniform, mixed


def reference(gens_G, gens_H, case, Mr, rounds, first, n):
    """out[i] = tab[i] + sum_t s'_t tab[i + t*Mr] for both tables, compressed: 2 * Mr encodings, G side then H side.  gens_G, gens_H: the compressed
    generators (32 bytes each, at least Mr * 2^rounds of them) as gens_export returns them; s'_t = s_t u_ch mod l exactly where first and i + t*Mr >= n.
    Every output is one multiscalar sum of the CPU oracle."""
    import oracle_lib as O
    _, sG, sH, u = case
    nterms = (1 << rounds) - 1
    assert len(sG) == nterms and len(gens_G) >= 32 * Mr * (nterms + 1) and len(gens_H) >= 32 * Mr * (nterms + 1)
    out = []
    for tab, ss in ((gens_G, sG), (gens_H, sH)):
        for i in range(Mr):
            scal, pts = [sc(1)], [tab[32 * i:32 * i + 32]]
            for t in range(1, nterms + 1):
                s = ss[t - 1] * u % L if padding(i, t, Mr, n, first) else ss[t - 1]
                if s:
                    scal.append(sc(s))
                    pts.append(tab[32 * (i + t * Mr):32 * (i + t * Mr) + 32])
            out.append(O.msm(b"".join(scal), b"".join(pts), 1))
    return out
