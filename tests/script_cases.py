"""Proofs under a scripted transcript: the catalogue of chosen challenges and an integer model of a proof's scalar skeleton - a plain helper module (not a
conftest) shared by test_script_cases_host.py (which pins the catalogue, the model and the scripted oracle without a device) and test_scripted_proofs_gpu.py
(which runs every case through bpg_test_prove_scripted, bpg_test_prove_batch_scripted, bpg_test_verify_scripted and bpg_test_verify_batch_scripted).

Inside a proof every challenge is a hash output, so the kernels that consume them see uniformly random 252-bit numbers only.  A script is the list
y, z, u, x, w, u_1 .. u_lgN that the transcript hands out INSTEAD of what it squeezed (its state evolves as always).  The catalogue:
  one     one script position at a time takes each value of V (and 0 where the position is not inverted), filler - a fixed scalar from SHAKE - everywhere else;
  all     every position is 1, then 2, then l - 1, at N = 1 (n = 1 and n = 0), 2, 8, 64, 512 (n = 300), 1024 (n = 700), in the dialects 0 and 3;
  cancel  exact cancellations the model solves for: w_O,i = y^i, l_1,i = 0, an addition in l(x) whose integer sum is exactly l, <a_lo, b_hi> = 0 in round 0,
          t_1 = 0, and l(x) = 0 through x = 0 - at N = 64 and N = 1024;
  witness a_L, a_R, a_O drawn from {0, 1, l - 1, 2^252} under all-1 and all-(l - 1) scripts.
The model (skeleton) is plain Python integers from the flat circuit, the witness, the TranscriptRng draws (O.rng_scalars: they do not depend on any challenge)
and the script; the points stay with the oracle.  Nothing here imports the package's arithmetic."""
import collections
import functools
import hashlib

import oracle_lib as O
import verify_cases as VC

L = 2**252 + 27742317777372353535851937790883648493
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
R_INV = pow(2, -256, L)                       # the scalar whose Montgomery form is 1; its negation has the form l - 1
V = (1, 2, 3, L - 1, L - 2, (L + 1) // 2, 2**252, 2**252 - 1, 2**128, R_INV, L - R_INV)
V_NAMES = ("1", "2", "3", "l-1", "l-2", "(l+1)/2", "2^252", "2^252-1", "2^128", "2^-256", "-2^-256")
POSITIONS = ("y", "z", "u", "x", "w")        # then u_1 .. u_lgN
MAY_BE_ZERO = ("z", "u", "x", "w")
SEED = bytes(range(32))
GENS_CAPACITY = 1024

Case = collections.namedtuple("Case", "name group circuit script flags seed")


def le(x):
    return int(x).to_bytes(32, "little")


def inv(x):
    return pow(x, -1, L)


def filler(tag, k=0):
    """a fixed pseudo-random non-zero scalar"""
    x = int.from_bytes(hashlib.shake_256(b"script-cases %s %d" % (tag, k)).digest(64), "little") % L
    assert x
    return x


def position_names(lgN):
    return POSITIONS + tuple("u_%d" % (k + 1) for k in range(lgN))


def filler_script(lgN, tag=b"script"):
    return [filler(tag + b" " + p.encode()) for p in position_names(lgN)]


def script_bytes(script):
    return [le(s) for s in script]


# ------------------------------------------------------------------------------------------------ circuits
def spec(n, m, tag):
    """random witness and rows WITHOUT their constant terms: row i holds a_L,i, a_R,i+1, a_O,i+2 and v_(i mod m), so a_O,k appears in row (k - 2) mod n alone"""
    s = {"n": n, "m": m, "tag": tag}
    s["aL"] = [filler(tag + b" aL", i) for i in range(n)]
    s["aR"] = [filler(tag + b" aR", i) for i in range(n)]
    s["aO"] = [a * b % L for a, b in zip(s["aL"], s["aR"])]
    s["v"] = [filler(tag + b" v", j) for j in range(m)]
    s["vb"] = [filler(tag + b" vb", j) for j in range(m)]
    c = lambda what, i: filler(tag + b" c" + what, i)
    s["terms"] = [[(VC.var(KIND_L, i), c(b"l", i)), (VC.var(KIND_R, (i + 1) % n), c(b"r", i)), (VC.var(KIND_O, (i + 2) % n), c(b"o", i))]
                  + ([(VC.var(KIND_V, i % m), c(b"v", i))] if m else []) for i in range(n)]
    return s


def spec_n0(tag):
    """the constraint-only circuit of test_constraint_only_circuit_n0: two commitments to one value, v_0 - v_1 = 0, no multiplier (N = 1)"""
    x = filler(tag + b" v")
    return {"n": 0, "m": 2, "tag": tag, "aL": [], "aR": [], "aO": [], "v": [x, x], "vb": [filler(tag + b" vb", 0), filler(tag + b" vb", 1)],
            "terms": [[(VC.var(KIND_V, 0), 1), (VC.var(KIND_V, 1), L - 1)]]}


def build(s, name):
    """the statement of a spec, every row closed with the constant that makes the witness satisfy it (the products a_L a_R = a_O are the spec's own affair)"""
    val = lambda pv: {KIND_L: s["aL"], KIND_R: s["aR"], KIND_O: s["aO"], KIND_V: s["v"]}[pv >> 29][pv & 0x1fffffff]
    rows = [VC._closed(t, val) for t in s["terms"]]
    return VC.Circuit(name, b"Scripted " + s["tag"], s["n"], s["m"], s["aL"], s["aR"], s["aO"], rows, s["v"], s["vb"])


def oracle_circuit(circ):
    i = circ.inst
    return O.FlatCircuit(i.n, i.m, i.aL, i.aR, i.aO, i.row_ptr, i.term_var, i.term_coef, i.coef)


def satisfied(circ):
    return O.satisfied(oracle_circuit(circ), b"".join(le(x) for x in circ.v))


# ------------------------------------------------------------------------------------------------ the model
@functools.lru_cache(maxsize=None)
def _draws(state, m, vb, seed, count):
    t = O.Transcript(state=state)
    t.append_u64(b"m", m)
    return tuple(int.from_bytes(b, "little") for b in O.rng_scalars(t.state, vb, seed, count))


def draws(circ, seed):
    """ib, ob, sb, s_L (n), s_R (n), tau_1, tau_3 .. tau_6: the TranscriptRng is built right after append_u64("m"), before any challenge"""
    return _draws(bytes(circ.state), circ.m, b"".join(le(x) for x in circ.vb), seed, 3 + 2 * circ.n + 5)


def weights(rows, n, m, z):
    """flattened_constraints(z): row j weighted by z^(j+1); committed and constant terms change side"""
    wL, wR, wO, wV, wc, ez = [0] * n, [0] * n, [0] * n, [0] * m, 0, z % L
    for row in rows:
        for pv, c in row:
            kind, idx, t = pv >> 29, pv & 0x1fffffff, ez * c % L
            if kind == KIND_L: wL[idx] = (wL[idx] + t) % L
            elif kind == KIND_R: wR[idx] = (wR[idx] + t) % L
            elif kind == KIND_O: wO[idx] = (wO[idx] + t) % L
            elif kind == KIND_V: wV[idx] = (wV[idx] - t) % L
            else: wc = (wc - t) % L
        ez = ez * z % L
    return wL, wR, wO, wV, wc


def ip(a, b):
    assert len(a) == len(b)
    return sum(x * y for x, y in zip(a, b)) % L


def skeleton(n, m, rows, aL, aR, aO, vb, d, script):
    """Every scalar of the proof that is not a point's: w_L .. w_V, the six vectors, t_1 .. t_6, t(x), its blinding, e_blinding, l(x), r(x), every round's
    <a_lo, b_hi>, <a_hi, b_lo> and folded vectors, the final a and b."""
    N = 1
    while N < n:
        N *= 2
    lgN = N.bit_length() - 1
    assert len(script) == 5 + lgN and len(d) == 3 + 2 * n + 5
    y, z, u, x, w = script[:5]
    ib, ob, sb = d[:3]
    sL, sR, tau = list(d[3:3 + n]), list(d[3 + n:3 + 2 * n]), dict(zip((1, 3, 4, 5, 6), d[3 + 2 * n:]))
    wL, wR, wO, wV, wc = weights(rows, n, m, z)
    yp, yip, yi = [1] * N, [1] * N, inv(y)
    for i in range(1, N):
        yp[i], yip[i] = yp[i - 1] * y % L, yip[i - 1] * yi % L
    l1 = [(aL[i] + yip[i] * wR[i]) % L for i in range(n)]
    l2, l3 = list(aO), sL
    r0 = [(wO[i] - yp[i]) % L for i in range(n)]
    r1 = [(yp[i] * aR[i] + wL[i]) % L for i in range(n)]
    r3 = [yp[i] * sR[i] % L for i in range(n)]
    t = [0, ip(l1, r0), (ip(l1, r1) + ip(l2, r0)) % L, (ip(l2, r1) + ip(l3, r0)) % L, (ip(l1, r3) + ip(l3, r1)) % L, ip(l2, r3), ip(l3, r3)]
    tau[2] = ip(wV, vb)
    t_x = sum(t[k] * pow(x, k, L) for k in range(1, 7)) % L
    t_x_blinding = sum(tau[k] * pow(x, k, L) for k in range(1, 7)) % L
    e_blinding = x * (ib + x * (ob + x * sb)) % L
    lx = [x * (l1[i] + x * (l2[i] + x * l3[i])) % L for i in range(n)] + [0] * (N - n)
    rx = [(r0[i] + x * (r1[i] + x * x * r3[i])) % L for i in range(n)] + [(-yp[i]) % L for i in range(n, N)]
    a, b, rounds = lx, rx, []
    for uk in script[5:]:
        h, ui = len(a) // 2, inv(uk)
        cL, cR = ip(a[:h], b[h:]), ip(a[h:], b[:h])
        a = [(a[i] * uk + ui * a[h + i]) % L for i in range(h)]
        b = [(b[i] * ui + uk * b[h + i]) % L for i in range(h)]
        rounds.append({"cL": cL, "cR": cR, "a": a, "b": b})
    return {"N": N, "wL": wL, "wR": wR, "wO": wO, "wV": wV, "wc": wc, "l1": l1, "l2": l2, "l3": l3, "r0": r0, "r1": r1, "r3": r3, "t": t, "tau": tau,
            "t_x": t_x, "t_x_blinding": t_x_blinding, "e_blinding": e_blinding, "lx": lx, "rx": rx, "rounds": rounds, "a": a[0], "b": b[0], "x": x,
            "sum_l2": [(l2[i], x * l3[i] % L) for i in range(n)]}


def case_skeleton(case):
    c = case.circuit
    return skeleton(c.n, c.m, c.rows, c.aL, c.aR, c.aO, c.vb, draws(c, case.seed), case.script)


def proof_scalars(proof, flags):
    """t_x, t_x_blinding, e_blinding, a, b of a proof's bytes"""
    at = (1 + 96 if flags & 1 else 192) + 160
    f = lambda o: int.from_bytes(proof[o:o + 32], "little")
    return {"t_x": f(at), "t_x_blinding": f(at + 32), "e_blinding": f(at + 64), "a": f(len(proof) - 64), "b": f(len(proof) - 32)}


# ------------------------------------------------------------------------------------------------ the catalogue
SIZES = (("N1", 1, 1), ("N1n0", 0, 2), ("N2", 2, 1), ("N8", 5, 2), ("N64", 40, 2), ("N512", 300, 2), ("N1024", 700, 3))      # (tag, n, m)


@functools.lru_cache(maxsize=None)
def base_spec(tag):
    n, m = {t: (n, m) for t, n, m in SIZES}[tag]
    return spec_n0(tag.encode()) if n == 0 else spec(n, m, tag.encode())


@functools.lru_cache(maxsize=None)
def base_circuit(tag):
    return build(base_spec(tag), tag)


def _one_position(tag, positions):
    c, out = base_circuit(tag), []
    names = position_names(c.lgN)
    for p in positions:
        k = names.index(p)
        for vname, value in zip(V_NAMES + ("0",), V + (0,)):
            if value == 0 and p not in MAY_BE_ZERO:
                continue
            script = filler_script(c.lgN)
            script[k] = value
            out.append(Case("one/%s/%s=%s" % (tag, p, vname), "one", c, script, 0, SEED))
    return out


def _all_at_once():
    out = []
    for tag, _, _ in SIZES:
        c = base_circuit(tag)
        for vname, value, flags in (("1", 1, 0), ("2", 2, 0), ("l-1", L - 1, 0), ("2", 2, 3), ("l-1", L - 1, 3)):
            out.append(Case("all/%s/%s/flags%d" % (tag, vname, flags), "all", c, [value] * (5 + c.lgN), flags, SEED))
    return out


def _solve(tag, kind):
    """the spec of `tag` changed so that, under the filler script, the named quantity cancels EXACTLY; whatever witness entry moves, a_O = a_L a_R is kept and
    the rows are closed again, so the witness still satisfies the circuit"""
    base = base_spec(tag)
    s = dict(base, aL=list(base["aL"]), aR=list(base["aR"]), aO=list(base["aO"]), terms=[list(t) for t in base["terms"]], tag=base["tag"] + b" " + kind.encode())
    n, m = s["n"], s["m"]
    script = filler_script((1 << (n - 1).bit_length()).bit_length() - 1)
    if kind == "x=0":
        script[3] = 0
        return s, script
    y, z, u, x, w = script[:5]
    d = _draws(bytes(build(s, "probe").state), m, b"".join(le(b) for b in s["vb"]), SEED, 3 + 2 * n + 5)       # (state: the label and V only)
    sL = d[3:3 + n]
    if kind == "wO=y^i":                        # r0_i = 0 at i = 0 and at the last real index: the one coefficient of a_O,i, in row j = (i - 2) mod n
        for i in (0, n - 1):
            j = (i - 2) % n
            s["terms"][j] = [(pv, pow(y, i, L) * inv(pow(z, j + 1, L)) % L if pv == VC.var(KIND_O, i) else c) for pv, c in s["terms"][j]]
        return s, script
    sk = lambda: skeleton(n, m, s["terms"], s["aL"], s["aR"], s["aO"], s["vb"], d, script)      # (constant terms weigh on w_c only: the verifier's)
    k0 = sk()
    if kind == "l1=0":                          # a_L,i = -y^-i w_R,i
        for i in (0, n - 1):
            s["aL"][i] = (-(k0["l1"][i] - s["aL"][i])) % L
    elif kind == "sum=l":                       # a_O,i + x s_L,i = l as integers, inside l(x)
        for i in (0, n - 1):
            s["aO"][i] = (-x * sL[i]) % L
            s["aL"][i] = s["aO"][i] * inv(s["aR"][i]) % L
    elif kind == "t1=0":                        # a_L,0 moves l_1,0 so that <l_1, r_0> = 0
        rest = ip(k0["l1"][1:], k0["r0"][1:])
        s["aL"][0] = (-rest * inv(k0["r0"][0]) - (k0["l1"][0] - s["aL"][0])) % L
    elif kind == "cL=0":                        # a_L,0 moves l(x)_0 so that <a_lo, b_hi> = 0 in round 0: l_0 = x (a_L,0 (1 + x a_R,0) + y^0 w_R,0 + x^2 s_L,0)
        h = k0["N"] // 2
        rest = ip(k0["lx"][1:h], k0["rx"][h + 1:])
        l0 = -rest * inv(k0["rx"][h]) % L
        s["aL"][0] = (l0 * inv(x) - k0["wR"][0] - x * x * sL[0]) * inv(1 + x * s["aR"][0]) % L
    else:
        raise KeyError(kind)
    for i in (0, n - 1):
        if kind != "sum=l":
            s["aO"][i] = s["aL"][i] * s["aR"][i] % L
    return s, script


CANCELLATIONS = ("wO=y^i", "l1=0", "sum=l", "cL=0", "t1=0", "x=0")


def _cancellations():
    out = []
    for tag in ("N64", "N1024"):
        for kind in CANCELLATIONS:
            s, script = _solve(tag, kind)
            out.append(Case("cancel/%s/%s" % (tag, kind), "cancel", build(s, "%s %s" % (tag, kind)), script, 0, SEED))
    return out


WITNESS_EDGES = (0, 1, L - 1, 2**252)


def _witness_edges():
    out = []
    for tag in ("N8", "N64"):
        base = base_spec(tag)
        pick = lambda what, i: WITNESS_EDGES[filler(b"edge " + what, i) % 4]
        s = dict(base, tag=base["tag"] + b" edges", aL=[pick(b"aL", i) for i in range(base["n"])], aR=[pick(b"aR", i) for i in range(base["n"])],
                 aO=[pick(b"aO", i) for i in range(base["n"])])
        c = build(s, tag + " edges")
        for vname, value in (("1", 1), ("l-1", L - 1)):
            out.append(Case("witness/%s/all=%s" % (tag, vname), "witness", c, [value] * (5 + c.lgN), 0, SEED))
    return out


@functools.lru_cache(maxsize=None)
def catalogue():
    cases = (_one_position("N8", position_names(3)) + _one_position("N64", ("y", "z", "x", "u_1", "u_6")) + _all_at_once() + _cancellations() + _witness_edges())
    assert len({c.name for c in cases}) == len(cases)
    return tuple(cases)


def by_name(name):
    return {c.name: c for c in catalogue()}[name]


# ------------------------------------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def gens():
    return O.Gens(GENS_CAPACITY)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(proof, transcript state after) of the scripted oracle prover, computed once per case and shared"""
    case = by_name(name)
    rc, proof, after = O.prove(gens(), case.circuit.state, oracle_circuit(case.circuit), b"".join(le(x) for x in case.circuit.vb), case.seed,
                               case.flags | O.FLAG_FAST_MSM, script=script_bytes(case.script))
    assert rc == 0, name
    return proof, after


@functools.lru_cache(maxsize=None)
def case_satisfied(name):
    return satisfied(by_name(name).circuit)


def oracle_verify(case, proof, script=None):
    return O.verify(gens(), case.circuit.state, oracle_circuit(case.circuit), case.circuit.V, proof, SEED, case.flags,
                    script=script_bytes(case.script if script is None else script))


# ------------------------------------------------------------------------------------------------ tampered proofs
TAMPER_BASES = ("one/N8/x=0", "one/N8/w=0", "one/N8/z=0", "one/N8/u_1=l-1", "all/N8/1/flags0", "all/N64/l-1/flags3", "cancel/N64/t1=0", "all/N1n0/2/flags0")
TAMPER_FIELDS = ("T_1", "t_x", "e_blinding", "a", "L_0")


def tamper(case, proof, field):
    """one field of the proof changed: T_1 and L_0 to another valid point (the Pedersen base B), a scalar to itself + 1; None where the proof has no such field"""
    at = (1 + 96 if case.flags & 1 else 192)
    where = {"T_1": at, "t_x": at + 160, "e_blinding": at + 224, "a": len(proof) - 64, "L_0": at + 256}[field]
    if field == "L_0" and case.circuit.lgN == 0:
        return None
    old = proof[where:where + 32]
    new = O.pedersen_bases()[0] if field in ("T_1", "L_0") else le((int.from_bytes(old, "little") + 1) % L)
    assert new != old
    return proof[:where] + new + proof[where + 32:]


def tampers():
    """[(name, case, tampered proof)]"""
    out = []
    for base in TAMPER_BASES:
        case = by_name(base)
        for field in TAMPER_FIELDS:
            p = tamper(case, reference(base)[0], field)
            if p is not None:
                out.append(("%s#%s" % (base, field), case, p))
    return out


def wrong_script(case):
    """the script of a case with another y"""
    s = list(case.script)
    s[0] = s[0] % (L - 1) + 1
    assert s[0] != case.script[0] and 0 < s[0] < L
    return s
