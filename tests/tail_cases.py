"""The table-driven kernels of the inner-product argument (csrc/hip/k_ipa.cuh: k_tt_factors, k_tt_advance, k_tt_round, k_tt_round8, k_tt_finish, k_tt_commit3,
k_tt_commit3_finish, on the tables of k_tt_bases / k_tt_multiples and their 8-bit siblings) at CHOSEN scalars: the catalogue of cases, an integer model of the
two signed-window recodings, and the textbook reference of a round.  Shared by test_tail_cases_host.py (which pins the catalogue without a device and compares
the model with the product's recoders compiled for the host) and test_tail_kernels_gpu.py (which runs every case through bpg_test_tail / bpg_test_commit3).
Plain Python integers for scalars, the CPU oracle for points; nothing here imports the package's recoders.

A tail case is a TailCase: a, b (M0 scalars each), yinv, u_ch, gamma0, eta0, w and one challenge per sub-round.  With yinv = gamma0 = eta0 = 1 (and u_ch = 1 or no
padding) the scalar that sub-round 0 puts on a base point is the caller's a[i] or b[i] itself: that is how a digit string reaches a kernel."""
import collections
import functools
import hashlib

import fold_cases as F

L = F.L
sc = F.sc
TailCase = collections.namedtuple("TailCase", "name a b yinv u_ch gamma0 eta0 w u")
CommitCase = collections.namedtuple("CommitCase", "name aL aR aO sL sR blind")
IDENTITY = bytes(32)                                    # the encoding of the neutral element


def inv(x):
    return pow(x, -1, L)


def ordinary(k):
    """A fixed non-zero scalar with nothing special about it."""
    return int.from_bytes(hashlib.sha512(b"tail case %d" % k).digest(), "little") % L or 1


# ---------------------------------------------------------------------------------------------------- integer model of the recodings
def signed_digits(s, bits):
    """The radix-2^bits digits of 0 <= s < 2^256 with every digit in [-2^(bits-1), 2^(bits-1) - 1], least significant first: 256 / bits of them.  The textbook
    recoding - take the residue, make it negative when it is in the upper half, carry - which is the only digit string with that digit set."""
    base, half = 1 << bits, 1 << (bits - 1)
    out = []
    for _ in range(256 // bits):
        d = s % base
        if d >= half:
            d -= base
        out.append(d)
        s = (s - d) // base
    assert s == 0
    return out


def digits4(s):
    return signed_digits(s, 4)


def digits8(s):
    return signed_digits(s, 8)


def from_digits(d, bits):
    return sum(v << (bits * k) for k, v in enumerate(d))


def word_carries(s, bits):
    """Which of the eight 32-bit words pass a carry upwards when the bias 0x88..8 (0x80..80) is added: the chain the kernels' recoders run through."""
    bias = int(("8" if bits == 4 else "80") * (64 if bits == 4 else 32), 16)
    out, carry = [], 0
    for k in range(8):
        t = ((s >> (32 * k)) & 0xffffffff) + ((bias >> (32 * k)) & 0xffffffff) + carry
        carry = t >> 32
        out.append(carry)
    return out


# ---------------------------------------------------------------------------------------------------- the digit edges
def _word_edges(bits, lo, hi, below_first):
    """Digits `below_first` / the other extreme on the two sides of each of the seven 32-bit word edges; a digit of 1 on top where the sum would be negative."""
    per = 32 // bits
    d = [0] * (256 // bits)
    for k in range(1, 8):
        d[per * k - 1], d[per * k] = (lo, hi) if below_first == lo else (hi, lo)
    if from_digits(d, bits) < 0:
        d[per * 7 + 2] = 1
    return from_digits(d, bits)


@functools.lru_cache(maxsize=None)
def edges():
    """name -> scalar: the named values of fold_cases, and the digit strings at which the two recodings can go wrong."""
    v = dict(F.named())
    v["4: every window -8"] = int("0" + "7" * 62 + "8", 16)                     # 0x0777..78: windows 0..62 are -8, each by a carry from below; window 63 is 1
    v["4: every window +7"] = int("0" + "7" * 63, 16)
    v["4: 0x0888..8"] = int("0" + "8" * 63, 16)                                 # -8, then -7 up to window 62, a carry into window 63
    v["8: every window -128"] = int("00" + "7f" * 30 + "80", 16)                # windows 0..30 are -128 by carries, window 31 is 1
    v["8: every window +127"] = int("00" + "7f" * 31, 16)
    v["8: +127 below the top byte of l"] = int("0f" + "7f" * 31, 16)
    v["4: -8 | +7 at the word edges"] = _word_edges(4, -8, 7, -8)
    v["4: +7 | -8 at the word edges"] = _word_edges(4, -8, 7, 7)
    v["8: -128 | +127 at the word edges"] = _word_edges(8, -128, 127, -128)
    v["8: +127 | -128 at the word edges"] = _word_edges(8, -128, 127, 127)
    v["carry through all words"] = int("0" + "f" * 63, 16) - (1 << 31)           # every word passes a carry upwards under both biases; no word is all ones
    v["l-1-2^128"] = L - 1 - (1 << 128)
    for name, s in v.items():
        assert 0 <= s < L, name
    return v


BLIND_EDGES = ("0", "1", "l-1", "4: every window -8", "4: every window +7", "4: 0x0888..8", "4: -8 | +7 at the word edges", "4: +7 | -8 at the word edges",
               "2^252", "2^252+1", "l-2", "carry through all words")          # what the 64 window threads of the finish kernels are given (4-bit tables only)


# ---------------------------------------------------------------------------------------------------- tail cases
def first_ns(M0):
    """The n of a first round: no padding; all the padding there is; a class boundary inside a block of 32 base points (and off any multiple of 8); one on a
    multiple of 32.  Only those with M0/2 < n <= M0, without repeats."""
    out = []
    for n in (M0, M0 // 2 + 1, M0 // 2 + M0 // 4 + M0 // 16 + 1 if M0 >= 16 else M0, (M0 // 2 // 32 + 1) * 32):
        if M0 // 2 < n <= M0 and n not in out:
            out.append(n)
    return out


def _vec(M0, k):
    return [ordinary(1000 * k + i) for i in range(M0)]


def _perp(M0):
    """a, b with <a_lo, b_hi> = <a_hi, b_lo> = 0 and neither vector zero: b_hi = (a_lo[1], -a_lo[0], a_lo[3], -a_lo[2], ..), likewise b_lo from a_hi."""
    h = M0 // 2
    a = _vec(M0, 7)
    if h == 1:
        return a, [0, 0]
    turn = lambda x: [x[i ^ 1] if i % 2 == 0 else (L - x[i ^ 1]) % L for i in range(len(x))]
    return a, turn(a[h:]) + turn(a[:h])


def _dot(x, y):
    return sum(p * q for p, q in zip(x, y)) % L


@functools.lru_cache(maxsize=None)
def tail_cases(lgM0, first, n):
    """The cases of one shape.  Every case has lgM0 challenges; a test may run fewer sub-rounds."""
    M0, h = 1 << lgM0, 1 << (lgM0 - 1)
    E = edges()
    items = list(E.items())
    one = [1] * lgM0
    us = [ordinary(50 + j) for j in range(lgM0)]
    A, B = _vec(M0, 1), _vec(M0, 2)
    pad = bool(first) and n < M0
    C = lambda name, a, b, yinv=1, u_ch=1, gamma0=1, eta0=1, w=ordinary(3), u=one: TailCase(name, tuple(a), tuple(b), yinv, u_ch, gamma0, eta0, w, tuple(u))
    cases = []
    if not pad or n == first_ns(M0)[min(2, len(first_ns(M0)) - 1)]:
        # digit strings: one edge in every position of a, another in every position of b - each comes up on both sides; all factors 1
        cases += [C("edge %s | %s" % (p[0], q[0]), [p[1]] * M0, [q[1]] * M0) for p, q in zip(items, items[5:] + items[:5])]
        cases.append(C("edges position by position", [items[i % len(items)][1] for i in range(M0)], [items[(3 * i + 1) % len(items)][1] for i in range(M0)]))
        cases.append(C("a and b all zero", [0] * M0, [0] * M0, ordinary(4), ordinary(5), ordinary(6), ordinary(7), ordinary(8), us))
        cases.append(C("a zero, b ordinary", [0] * M0, B, u=us))
        cases.append(C("a ordinary, b zero", A, [0] * M0, u=us))
        pa, pb = _perp(M0)
        cases.append(C("a perpendicular to b: cw = 0", pa, pb, u=one))
        cases.append(C("a perpendicular to b, ordinary factors", pa, pb, ordinary(4), ordinary(5), ordinary(6), ordinary(7), ordinary(8), us))
        cases.append(C("w = 0", A, B, w=0, u=us))
        # the scalar on B at sub-round 0 at each digit edge: w = e / <a_lo, b_hi> for L, e / <a_hi, b_lo> for R
        cL, cR = _dot(A[:h], B[h:]), _dot(A[h:], B[:h])
        assert cL and cR
        for name in BLIND_EDGES:
            cases.append(C("cw of L = %s" % name, A, B, w=E[name] * inv(cL) % L, u=us))
            cases.append(C("cw of R = %s" % name, A, B, w=E[name] * inv(cR) % L, u=us))
        for name, u in (("1", 1), ("l-1", L - 1), ("2", 2), ("ordinary", ordinary(9))):
            cases.append(C("every u = %s" % name, A, B, u=[u] * lgM0))
            cases.append(C("yinv = %s" % name, A, B, yinv=u, u=one))
        cases.append(C("u all different", A, B, u=us))
        cases.append(C("gamma0 and eta0 ordinary", A, B, gamma0=ordinary(6), eta0=ordinary(7), u=one))
        cases.append(C("every factor ordinary", A, B, ordinary(4), ordinary(5), ordinary(6), ordinary(7), ordinary(8), us))
    if first:
        # the class of the padding generators: u_ch ordinary and 1; digit strings there: s ordinary and u_ch = e / s, so that s * u_ch is the edge e
        cases.append(C("padding: u_ch = 1", A, B, u_ch=1, u=us))
        cases.append(C("padding: u_ch ordinary", A, B, u_ch=ordinary(5), u=us))
        cases.append(C("padding: u_ch and every factor ordinary", B, A, ordinary(14), ordinary(15), ordinary(16), ordinary(17), ordinary(18), us[::-1]))
        s = ordinary(11)
        for name in ("4: every window -8", "4: every window +7", "8: every window -128", "8: every window +127", "l-1", "2^252+1", "1"):
            cases.append(C("padding: s * u_ch = %s" % name, [s] * M0, [s] * M0, u_ch=E[name] * inv(s) % L))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert len(c.a) == M0 and len(c.b) == M0 and len(c.u) == lgM0
        assert all(0 <= s < L for s in c.a + c.b + c.u + (c.yinv, c.u_ch, c.gamma0, c.eta0, c.w)) and c.yinv and all(c.u)
    return tuple(cases)


def thread_scalar(g, wide=False):
    """A scalar whose non-zero digits all lie in 32-bit word g: one thread of the eight that share a base point adds, the other seven hold the identity."""
    s = (0x3d3a91c5 if g < 7 else 0x0d3a91c5) << (32 * g)
    assert 0 < s < L and [k for k in range(8) if any(digits4(s)[8 * k:8 * k + 8])] == [g] and [k for k in range(8) if any(digits8(s)[4 * k:4 * k + 4])] == [g]
    return s


@functools.lru_cache(maxsize=None)
def single_thread_cases(lgM0):
    """One non-zero scalar in all of a and b, with digits in one word: one live thread per launch, moved through every position of a block (and every block)."""
    M0 = 1 << lgM0
    out = []
    for side in "ab":
        for i in range(M0):
            for g in range(8):
                v = [0] * M0
                v[i] = thread_scalar(g)
                a, b = (v, [0] * M0) if side == "a" else ([0] * M0, v)
                out.append(TailCase("only %s[%d], word %d" % (side, i, g), tuple(a), tuple(b), 1, 1, 1, 1, ordinary(3), (ordinary(9),) * lgM0))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------- commitment cases
@functools.lru_cache(maxsize=None)
def commit_cases(n):
    E = edges()
    vals = list(E.values())
    cases = []
    rot = lambda k, r: [vals[(k * n + i + r) % len(vals)] for i in range(n)]
    for k in range(-(-len(vals) // n)):                     # every edge in every vector, n at a time
        cases.append(CommitCase("edges %d" % k, rot(k, 0), rot(k, 3), rot(k, 5), rot(k, 7), rot(k, 11), (ordinary(20 + k), ordinary(40 + k), ordinary(60 + k))))
    W = [[ordinary(100 * v + i) for i in range(n)] for v in range(5)]
    bl = [E[name] for name in BLIND_EDGES]
    for k in range(len(bl)):                                # each blinding edge in each of the three sums
        cases.append(CommitCase("blind %s" % BLIND_EDGES[k], *W, (bl[k], bl[(k + 1) % len(bl)], bl[(k + 2) % len(bl)])))
    cases.append(CommitCase("all zero", *[[0] * n] * 5, (0, 0, 0)))
    cases.append(CommitCase("witness zero, blinds ordinary", *[[0] * n] * 5, (ordinary(1), ordinary(2), ordinary(3))))
    cases.append(CommitCase("blinds zero, witness ordinary", *W, (0, 0, 0)))
    cases.append(CommitCase("only aO", [0] * n, [0] * n, W[2], [0] * n, [0] * n, (0, 1, 0)))
    cases.append(CommitCase("only aR and sR", [0] * n, W[1], [0] * n, [0] * n, W[4], (L - 1, 0, 1)))
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return tuple(CommitCase(c.name, *(tuple(v) for v in c[1:])) for c in cases)


# ---------------------------------------------------------------------------------------------------- the reference
def _msm(scalars, points):
    """sum s_i P_i by the CPU oracle; terms with a zero scalar left out; the empty sum is the identity."""
    import oracle_lib as O
    live = [(s, p) for s, p in zip(scalars, points) if s % L]
    if not live:
        return IDENTITY
    return O.msm(b"".join(sc(s % L) for s, _ in live), b"".join(p for _, p in live), 1)


def _factors(case, M0, first, n):
    fG = [case.u_ch if first and p >= n else 1 for p in range(M0)]
    return fG, [pow(case.yinv, p, L) * fG[p] % L for p in range(M0)]


_start_cache = {}
_fold_cache = {}


def _start(Gp, Hp, case, M0, first, n):
    """(a key, G0, H0): G0[p] = gamma0 fG[p] G_p, H0[p] = eta0 fH[p] H_p as points, shared by the cases with the same factors."""
    fG, fH = _factors(case, M0, first, n)
    key = (hashlib.sha256(b"".join(Gp[:M0] + Hp[:M0])).digest(), M0, tuple(fG), tuple(fH), case.gamma0, case.eta0)
    if key not in _start_cache:
        _start_cache[key] = ([_msm([case.gamma0 * fG[p]], [Gp[p]]) for p in range(M0)], [_msm([case.eta0 * fH[p]], [Hp[p]]) for p in range(M0)])
    return (key,) + _start_cache[key]


def _folded(key, G, H, us):
    """G'[i] = u^-1 G[i] + u G[h+i], H'[i] = u H[i] + u^-1 H[h+i] as points, shared by the cases with the same start and the same challenges so far."""
    key = (key, us)
    if key not in _fold_cache:
        u, ui, h = us[-1], inv(us[-1]), len(G) // 2
        _fold_cache[key] = ([_msm([ui, u], [G[i], G[h + i]]) for i in range(h)], [_msm([u, ui], [H[i], H[h + i]]) for i in range(h)])
    return _fold_cache[key]


def tail_reference(Gp, Hp, Bp, case, lgM0, first, n, rounds):
    """The textbook rounds on folded POINTS: ([(L_j, R_j)], a, b after the last challenge).  Gp, Hp: lists of compressed generators; Bp: the Pedersen base."""
    M0 = 1 << lgM0
    key, G, H = _start(Gp, Hp, case, M0, first, n)
    a, b = list(case.a), list(case.b)
    out = []
    for j in range(rounds):
        h = len(a) // 2
        out.append((_msm(a[:h] + b[h:] + [_dot(a[:h], b[h:]) * case.w], G[h:] + H[:h] + [Bp]), _msm(a[h:] + b[:h] + [_dot(a[h:], b[:h]) * case.w], G[:h] + H[h:] + [Bp])))
        u = case.u[j]
        ui = inv(u)
        a, b = [(a[i] * u + a[h + i] * ui) % L for i in range(h)], [(b[i] * ui + b[h + i] * u) % L for i in range(h)]
        if j + 1 < rounds:
            G, H = _folded(key, G, H, case.u[:j + 1])
    return out, a, b


def tail_reference_expanded(Gp, Hp, Bp, case, lgM0, first, n, rounds):
    """The same rounds with every virtual generator kept as its coefficients over the base points: G'[i] = u^-1 G[i] + u G[h+i] adds two coefficient vectors.  One
    multiscalar sum over the base points per L_j, R_j - for the shape too large to fold point by point."""
    M0 = 1 << lgM0
    fG, fH = _factors(case, M0, first, n)
    G = [{p: case.gamma0 * fG[p] % L} for p in range(M0)]
    H = [{p: case.eta0 * fH[p] % L} for p in range(M0)]
    a, b = list(case.a), list(case.b)

    def combine(x, X, y, Y):
        out = {p: x * c % L for p, c in X.items()}
        for p, c in Y.items():
            out[p] = (out.get(p, 0) + y * c) % L
        return out

    def total(sG, vG, sH, vH, cw):
        accG, accH = [0] * M0, [0] * M0
        for s, v in zip(sG, vG):
            for p, c in v.items():
                accG[p] = (accG[p] + s * c) % L
        for s, v in zip(sH, vH):
            for p, c in v.items():
                accH[p] = (accH[p] + s * c) % L
        return _msm(accG + accH + [cw], list(Gp[:M0]) + list(Hp[:M0]) + [Bp])

    out = []
    for j in range(rounds):
        h = len(a) // 2
        out.append((total(a[:h], G[h:], b[h:], H[:h], _dot(a[:h], b[h:]) * case.w), total(a[h:], G[:h], b[:h], H[h:], _dot(a[h:], b[:h]) * case.w)))
        u = case.u[j]
        ui = inv(u)
        a, b = [(a[i] * u + a[h + i] * ui) % L for i in range(h)], [(b[i] * ui + b[h + i] * u) % L for i in range(h)]
        if j + 1 < rounds:
            G, H = [combine(ui, G[i], u, G[h + i]) for i in range(h)], [combine(u, H[i], ui, H[h + i]) for i in range(h)]
    return out, a, b


def commit_reference(Gp, Hp, Bblind, case):
    """A_I = <aL, G> + <aR, H> + blind0 B_blinding, A_O = <aO, G> + blind1 B_blinding, S = <sL, G> + <sR, H> + blind2 B_blinding."""
    n = len(case.aL)
    G, H = list(Gp[:n]), list(Hp[:n])
    return [_msm(list(case.aL) + list(case.aR) + [case.blind[0]], G + H + [Bblind]), _msm(list(case.aO) + [case.blind[1]], G + [Bblind]),
            _msm(list(case.sL) + list(case.sR) + [case.blind[2]], G + H + [Bblind])]


def split_points(raw):
    return [raw[32 * i:32 * i + 32] for i in range(len(raw) // 32)]
