"""Malformed proofs for the verifier, with the CPU oracle's answer - a plain helper module (not a conftest) shared by
tests/test_verify_malformed_host.py and tests/test_verify_malformed_gpu.py.

corpus() builds, from fixed seeds and on the CPU alone:
  * base proofs: the oracle prover (O.prove) on six circuits in the four verifier dialects (flags 0..3);
  * mutants: records that differ from their base in exactly ONE way - one proof field, the framing, or the statement;
  * for every record the oracle verifier's status (orc_r1cs_verify, a serial restatement with its own decoder).
A record is (name, circuit, state, V, proof, seed, flags) plus what the tests need to file it: kind (which sort of field), cls (which mutation),
base, capacity (generator capacity the verifier has), status (the oracle's) and decided (must the host replay of the library decide it alone).

decoder_vectors() / check_decoder() are the vectors and the comparison of the RFC 9496 decoder (ge_decompress) with pyref.decompress, used
on the host build (hc_decompress) and on the device (bpg_test_decompress).

Three corners of the issue's matrix cannot exist and are left out by construction, not by taste:
  * a proof of the circuit without multipliers has t_x = 0, a = 0 and b = l - 1 (l(x) = 0, r(x) = -1 on the one padded index), so for these three
    fields "0" or "l - 1" is the base proof and two more classes coincide with an earlier one (0 + l = l, 0 - 1 = l - 1, (l - 1) + 1 = 0): each
    distinct value is kept once;
  * the second-phase points A_I2, A_O2, S2 of these circuits ARE the identity (no second phase), so "the identity" is the base proof itself and
    "its negation" p - 0 is the class "p"; both are skipped for kind A2 (and asserted to be the only holes);
  * the compact dialects carry no second-phase points, so kind A2 exists for flags 0 and 2 only.
"""
import collections
import ctypes as C
import functools
import hashlib
import numpy as np
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import pyref as R
import gen_proof_fixtures as G

P, L = R.P, R.L
KIND_L, KIND_R, KIND_O, KIND_V, KIND_ONE = 0, 1, 2, 3, 4
POINT_CLASSES = ("identity", "p", "bit255", "negation", "nonsquare", "negative_t", "p_minus_1", "other_point")
SCALAR_CLASSES = ("plus_l", "l", "all_ones", "plus_1", "minus_1", "zero", "l_minus_1")
NONCANONICAL_SCALARS = ("plus_l", "l", "all_ones")
SCALAR_FIELDS = ("t_x", "t_x_blinding", "e_blinding", "a", "b")
POINT_KINDS = ("A1", "A2", "T", "L", "R", "V")
IDENTITY_RULE_KINDS = ("A1", "T", "L", "R")          # validate_and_append_point / the inner-product argument's L, R: an identity encoding is refused on the host
FRAMING_CLASSES = ("len_minus_1", "len_plus_1", "len_minus_32", "len_plus_32", "empty", "lead_byte", "flags_other_length", "flags_same_length")
COEF_KINDS = {"left": KIND_L, "right": KIND_R, "output": KIND_O, "committed": KIND_V, "constant": KIND_ONE}
BIG_INDICES = (0, 255, 256, 511, 512, 699)            # the N = 1024 circuit: both ends of the first three blocks of k_verify_scalars, and n - 1

Record = collections.namedtuple("Record", "name circuit state V proof seed flags kind cls base capacity status decided")


def le(x):
    return int(x).to_bytes(32, "little")


def h_int(tag, i, mod=None):
    x = int.from_bytes(hashlib.sha512(b"verify-cases %s %d" % (tag, i)).digest(), "little")
    return x % mod if mod else x


# ------------------------------------------------------------------------------------------------ circuits
class Circuit:
    """A statement with its witness: rows = [[(variable, coefficient)]], each row constrained to zero (variable = kind << 29 | index)."""

    def __init__(self, name, label, n, m, aL, aR, aO, rows, v=(), vb=()):
        self.name, self.label, self.n, self.m = name, label, n, m
        self.aL, self.aR, self.aO, self.rows = list(aL), list(aR), list(aO), [list(r) for r in rows]
        self.v, self.vb = list(v), list(vb)
        self.V = b"".join(O.pedersen_commit(le(a), le(b)) for a, b in zip(self.v, self.vb))
        self.N = 1
        while self.N < n:
            self.N *= 2
        self.lgN = self.N.bit_length() - 1
        self.capacity = max(self.N, 8)
        self.inst = self.instance()
        self.state = self.transcript_state(self.label, self.V)

    @staticmethod
    def transcript_state(label, V):
        """Transcript::new(label), Verifier::new and every "V" append"""
        t = O.Transcript(label)
        t.append(b"dom-sep", b"r1cs v1")
        for j in range(len(V) // 32):
            t.append(b"V", V[32 * j:32 * j + 32])
        return t.state

    def instance(self, rows=None, witness=True):
        """the flattened instance of these (or other) rows as a bpg.FlatInstance, which both the library and - through G.to_oracle - the oracle take"""
        rows = self.rows if rows is None else rows
        coefs, tv, tc, rp = {}, [], [], [0]
        for row in rows:
            for var, c in row:
                tv.append(var)
                tc.append(coefs.setdefault(c % L, len(coefs)))
            rp.append(len(tv))
        keep = [np.asarray(rp, dtype=np.uint64), np.asarray(tv, dtype=np.uint32), np.asarray(tc, dtype=np.uint32),
                C.create_string_buffer(b"".join(le(c) for c in coefs), 32 * len(coefs) + 1)]
        wit = [C.create_string_buffer(b"".join(le(x) for x in a), 32 * self.n + 1) for a in (self.aL, self.aR, self.aO)]
        view = bpg.R1CSInstance()
        view.n, view.q, view.m, view.nnz, view.ncoef = self.n, len(rows), self.m, len(tv), len(coefs)
        if witness and self.n:
            view.aL, view.aR, view.aO = [C.cast(w, C.c_void_p).value for w in wit]
        view.row_ptr, view.term_var, view.term_coef = keep[0].ctypes.data, keep[1].ctypes.data if tv else None, keep[2].ctypes.data if tv else None
        view.coef = C.cast(keep[3], C.c_void_p).value
        return bpg.FlatInstance(view, v=b"".join(le(x) for x in self.v), v_blinding=b"".join(le(x) for x in self.vb), commitments=self.V)

    @classmethod
    def from_instance(cls, name, label, inst):
        """a commitment-free circuit assembled by the product's host code (gen_proof_fixtures)"""
        coef = [int.from_bytes(inst.coef[32 * k:32 * k + 32], "little") for k in range(inst.ncoef)]
        rows = [[(int(inst.term_var[k]), coef[int(inst.term_coef[k])]) for k in range(int(inst.row_ptr[j]), int(inst.row_ptr[j + 1]))] for j in range(inst.q)]
        ints = lambda b: [int.from_bytes(b[32 * k:32 * k + 32], "little") for k in range(inst.n)]
        assert inst.m == 0
        return cls(name, label, inst.n, 0, ints(inst.aL), ints(inst.aR), ints(inst.aO), rows)


def var(kind, index=0):
    return (kind << 29) | index


def _closed(terms, value_of):
    """the row sum(terms) + c = 0 with the constant chosen so that the witness satisfies it"""
    total = sum(c * value_of(v) for v, c in terms) % L
    return list(terms) + [(var(KIND_ONE), (-total) % L)]


def _random_circuit(name, label, n, m, row_terms):
    """n random multipliers, m random committed values; row_terms(i-th row) -> [(variable, coefficient)] without the constant term"""
    aL = [h_int(name + b" aL", i, L) for i in range(n)]
    aR = [h_int(name + b" aR", i, L) for i in range(n)]
    aO = [a * b % L for a, b in zip(aL, aR)]
    v = [h_int(name + b" v", j, L) for j in range(m)]
    vb = [h_int(name + b" vb", j, L) for j in range(m)]
    val = lambda pv: {KIND_L: aL, KIND_R: aR, KIND_O: aO, KIND_V: v}[pv >> 29][pv & 0x1fffffff]
    return Circuit(name.decode(), label, n, m, aL, aR, aO, [_closed(t, val) for t in row_terms], v, vb)


def circuits():
    c = lambda tag, i: 1 + h_int(tag, i, L - 1)                       # a non-zero coefficient
    out = []
    for name in ("range8", "range56"):
        inst, _, _ = G.build(name)
        out.append(Circuit.from_instance(name, b"RangeProof", inst))
    # n = 5, m = 2: pads 5 -> 8; every multiplier and both commitments appear
    out.append(_random_circuit(b"small5", b"Small5", 5, 2, [
        [(var(KIND_L, i), c(b"s5 l", i)), (var(KIND_R, (i + 1) % 5), c(b"s5 r", i)), (var(KIND_O, (i + 2) % 5), c(b"s5 o", i)), (var(KIND_V, i % 2), c(b"s5 v", i))]
        for i in range(5)]))
    # n = 1, m = 1: lg N = 0, a proof without L / R
    out.append(_random_circuit(b"one", b"One", 1, 1, [[(var(KIND_O, 0), 1), (var(KIND_V, 0), c(b"one v", 0))], [(var(KIND_L, 0), c(b"one l", 0)), (var(KIND_R, 0), c(b"one r", 0))]]))
    # n = 0: constraints over commitments alone
    out.append(_random_circuit(b"none", b"None", 0, 2, [[(var(KIND_V, 0), c(b"n0 a", 0)), (var(KIND_V, 1), c(b"n0 b", 0))], [(var(KIND_V, 1), c(b"n0 c", 0))]]))
    # n = 700 -> N = 1024, m = 3: four blocks of k_verify_scalars, real and padded indices in one block; row i touches all five kinds at multiplier i
    out.append(_random_circuit(b"big", b"Big", 700, 3, [
        [(var(KIND_L, i), c(b"big l", i)), (var(KIND_R, i), c(b"big r", i)), (var(KIND_O, i), c(b"big o", i)), (var(KIND_V, i % 3), c(b"big v", i))]
        for i in range(700)]))
    for k in out:
        assert O.satisfied(G.to_oracle(k.inst), b"".join(le(x) for x in k.v)), k.name
    return out


# ------------------------------------------------------------------------------------------------ encodings
def classify(b):
    """the RFC 9496 rejection rule an encoding falls under, in the order of the decoder, by the Python reference's arithmetic"""
    s = int.from_bytes(b, "little")
    if s >= P:
        return "noncanonical"
    if s & 1:
        return "negative_s"
    ss = s * s % P
    u1, u2 = (1 - ss) % P, (1 + ss) % P
    v = (-(R.D * u1 % P * u1) - u2 * u2) % P
    ok, inv = R.sqrt_ratio_m1(1, v * u2 % P * u2 % P)
    if not ok:
        return "nonsquare"
    den_x = inv * u2 % P
    x = R.fabs(2 * s * den_x)
    y = u1 * (inv * den_x % P * v % P) % P
    if R.is_neg(x * y):
        return "negative_t"
    if y == 0:
        return "y_zero"
    return "valid"


@functools.lru_cache(maxsize=None)
def hashed_encoding(cls, i=0, tag=b"enc"):
    """the i-th hashed even string below 2^255 that the reference files under cls"""
    k, seen = 0, -1
    while True:
        s = h_int(tag, k) % (1 << 255) & ~1
        k += 1
        if s < P and classify(le(s)) == cls:
            seen += 1
            if seen == i:
                return le(s)


RFC_BAD = ["00ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff",       # the four vectors of test_oracle_primitives.py (RFC 9496 A.2)
           "ffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffff7f",
           "0100000000000000000000000000000000000000000000000000000000000000",
           "26948d35ca62e643e26a83177332e6b6afeb9d08e4268b650f1f5bbd8d81d371"]


def decoder_vectors(golden, per_class=200):
    """[(class given by the reference, encoding)] - every edge the issue names, then hashed strings until valid, non-square and negative-t hold
    per_class each; the count is made not to be a multiple of 64 (the launch edge of k_decompress)"""
    vec = [le(0)] + [le(P + k) for k in range(19)] + [le(P - 1), le(1), le(2**255 - 1), le(2**256 - 1)]
    mult = [bytes.fromhex(x) for x in golden["ristretto_multiples"]]
    vec += mult + [bytes.fromhex(x) for x in RFC_BAD]
    valid = [m for m in mult if any(m)] + [hashed_encoding("valid", i) for i in range(8)]
    vec += [le(int.from_bytes(s, "little") | 1 << 255) for s in valid]                 # a valid encoding with bit 255 set
    vec += [le(P - int.from_bytes(s, "little")) for s in valid]                        # p - s for valid s
    have = collections.Counter()
    k = 0
    while min(have[c] for c in ("valid", "nonsquare", "negative_t")) < per_class:
        s = le(h_int(b"decoder", k) % (1 << 255) & ~1)
        k += 1
        have[classify(s)] += 1
        vec.append(s)
    if len(vec) % 64 == 0:
        vec.append(le(2))
    return [(classify(s), s) for s in vec]


def check_decoder(run, vectors):
    """run(list of encodings) -> (ok flags, [(x, y)]): the accept / reject decision of every vector against pyref.decompress; on accepted
    vectors x, y against it and the re-encoding against the input.  Returns the count per class."""
    encs = [s for _, s in vectors]
    assert len(encs) % 64 != 0
    ok, xy = run(encs)
    assert len(ok) == len(xy) == len(encs)
    counts = collections.Counter()
    for (cls, s), good, (x, y) in zip(vectors, ok, xy):
        want = R.decompress(s)
        assert (cls == "valid") == (want is not None)
        assert good in (0, 1) and bool(good) == (want is not None), (cls, s.hex(), good)
        if want is not None:
            assert (x, y) == (want.X, want.Y), (s.hex(), x, y)
            assert R.Point(x, y, 1, x * y).compress() == s, s.hex()
        counts[cls] += 1
    for s in (encs[0], encs[-1], le(P), hashed_encoding("valid"), hashed_encoding("negative_t")):        # n = 1: one lane of one wave
        ok1, xy1 = run([s])
        want = R.decompress(s)
        assert len(ok1) == 1 and bool(ok1[0]) == (want is not None), s.hex()
        if want is not None:
            assert xy1[0] == (want.X, want.Y)
    return counts


def check_decoder_counts(counts, per_class=200):
    """an empty class is a failure"""
    assert counts["valid"] >= per_class + 18 and counts["nonsquare"] >= per_class + 1 and counts["negative_t"] >= per_class, counts
    assert counts["noncanonical"] >= 19 + 2 + 24 + 2 and counts["negative_s"] >= 2 + 24 and counts["y_zero"] == 1, counts
    assert set(counts) == {"valid", "nonsquare", "negative_t", "noncanonical", "negative_s", "y_zero"}


# ------------------------------------------------------------------------------------------------ proofs and their fields
def oracle_verify(gens, state, inst, V, proof, seed, flags):
    """orc_r1cs_verify -> (status, transcript state after; the oracle returns early on a format or identity error and then leaves the state as given)"""
    ts = C.create_string_buffer(bytes(state), 203)
    cs = G.to_oracle(inst).cstruct()
    rc = O.lib().orc_r1cs_verify(gens.h, ts, C.byref(cs), V, proof, len(proof), seed, flags)
    return rc, ts.raw[:203]


def fields(circ, flags):
    """{field name: (kind, offset)} of a proof of circ in the dialect flags; V_j: offset into V"""
    out, o = collections.OrderedDict(), 0
    if flags & 1:
        o = 1
    for nm in ("A_I1", "A_O1", "S1"):
        out[nm] = ("A1", o); o += 32
    if not flags & 1:
        for nm in ("A_I2", "A_O2", "S2"):
            out[nm] = ("A2", o); o += 32
    for nm in ("T_1", "T_3", "T_4", "T_5", "T_6"):
        out[nm] = ("T", o); o += 32
    for nm in SCALAR_FIELDS[:3]:
        out[nm] = ("scalar", o); o += 32
    for k in range(circ.lgN):
        out["L_%d" % k] = ("L", o); o += 32
        out["R_%d" % k] = ("R", o); o += 32
    for nm in SCALAR_FIELDS[3:]:
        out[nm] = ("scalar", o); o += 32
    assert o == O.proof_size(circ.n, flags)
    for j in range(circ.m):
        out["V_%d" % j] = ("V", 32 * j)
    return out


def point_mutation(cls, cur, B):
    s = int.from_bytes(cur, "little")
    if cls == "identity":
        return le(0)
    if cls == "p":
        return le(P)
    if cls == "bit255":
        return le(s | 1 << 255)
    if cls == "negation":
        return le(P - s)
    if cls == "nonsquare":
        return hashed_encoding("nonsquare")
    if cls == "negative_t":
        return hashed_encoding("negative_t")
    if cls == "p_minus_1":
        return le(P - 1)
    if cls == "other_point":
        return O.point_add(cur, B)
    raise KeyError(cls)


def scalar_mutation(cls, cur):
    x = int.from_bytes(cur, "little")
    return le({"plus_l": x + L, "l": L, "all_ones": 2**256 - 1, "plus_1": (x + 1) % L, "minus_1": (x - 1) % L, "zero": 0, "l_minus_1": L - 1}[cls])


_CORPUS = None


def corpus():
    """(circuits by name, base records, mutant records); built once per process"""
    global _CORPUS
    if _CORPUS is None:
        _CORPUS = _build_corpus()
    return _CORPUS


def _build_corpus():
    B, _ = O.pedersen_bases()
    circs = collections.OrderedDict((c.name, c) for c in circuits())
    gens = {}

    def gens_of(cap):
        if cap not in gens:
            gens[cap] = O.Gens(cap)
        return gens[cap]

    bases, mutants = [], []

    def add(lst, name, circ, inst, state, V, proof, seed, flags, kind, cls, base, capacity=None, decided=False):
        capacity = circ.capacity if capacity is None else capacity
        status, _ = oracle_verify(gens_of(capacity), state, inst, V, proof, seed, flags)
        lst.append(Record(name, inst, state, V, proof, seed, flags, kind, cls, base, capacity, status, decided))

    proofs = {}
    for circ in circs.values():
        for flags in range(4):
            rc, proof, _ = O.prove(gens_of(circ.capacity), circ.state, G.to_oracle(circ.inst), circ.inst.v_blinding, hashlib.sha256(b"prove %s %d" % (circ.name.encode(), flags)).digest(),
                                   flags | O.FLAG_FAST_MSM)
            assert rc == 0 and len(proof) == O.proof_size(circ.n, flags)
            proofs[circ.name, flags] = proof

    for circ in circs.values():
        vinst = circ.instance(witness=False)                                      # the verifier's instance: no assignments
        for flags in range(4):
            proof = proofs[circ.name, flags]
            base = "%s/f%d" % (circ.name, flags)
            seed = hashlib.sha256(b"verify " + base.encode()).digest()
            put = lambda name, kind, cls, inst=vinst, state=circ.state, V=circ.V, proof=proof, flags=flags, **kw: \
                add(mutants, "%s/%s" % (base, name), circ, inst, state, V, proof, seed, flags, kind, cls, base, **kw)
            add(bases, base, circ, vinst, circ.state, circ.V, proof, seed, flags, "base", "base", base)
            # ---- every point field, every scalar field
            for nm, (kind, off) in fields(circ, flags).items():
                if kind == "scalar":
                    cur = proof[off:off + 32]
                    seen = {cur}
                    for cls in SCALAR_CLASSES:
                        new = scalar_mutation(cls, cur)
                        if new in seen:                                           # the module docstring's first hole
                            assert circ.n == 0 and nm in ("t_x", "a", "b")
                            continue
                        seen.add(new)
                        put("%s=%s" % (nm, cls), "scalar:" + nm, cls, proof=proof[:off] + new + proof[off + 32:], decided=cls in NONCANONICAL_SCALARS)
                    continue
                src = circ.V if kind == "V" else proof
                cur = src[off:off + 32]
                for cls in POINT_CLASSES:
                    if kind == "A2" and cls in ("identity", "negation"):
                        assert cur == bytes(32)                                   # the module docstring's two holes
                        continue
                    new = src[:off] + point_mutation(cls, cur, B) + src[off + 32:]
                    decided = cls == "identity" and kind in IDENTITY_RULE_KINDS
                    if kind == "V":
                        put("%s=%s" % (nm, cls), kind, cls, V=new)
                    else:
                        put("%s=%s" % (nm, cls), kind, cls, proof=new, decided=decided)
            # ---- framing
            put("len-1", "framing", "len_minus_1", proof=proof[:-1], decided=True)
            put("len+1", "framing", "len_plus_1", proof=proof + b"\x00", decided=True)
            put("len-32", "framing", "len_minus_32", proof=proof[:-32], decided=True)
            put("len+32", "framing", "len_plus_32", proof=proof + proof[-32:], decided=True)
            put("empty", "framing", "empty", proof=b"", decided=True)
            if flags & 1:
                put("lead=1", "framing", "lead_byte", proof=b"\x01" + proof[1:], decided=True)
                put("lead=255", "framing", "lead_byte", proof=b"\xff" + proof[1:], decided=True)
            for other in range(4):
                if other != flags:
                    same = (other & 1) == (flags & 1)
                    put("as-f%d" % other, "framing", "flags_same_length" if same else "flags_other_length", flags=other, decided=not same)
            # ---- statement
            rows = circ.rows
            if circ.name == "big":
                for i in BIG_INDICES:
                    for cname, ck in COEF_KINDS.items():
                        at = next(k for k, (pv, _) in enumerate(rows[i]) if pv >> 29 == ck)
                        changed = list(rows[i])
                        changed[at] = (changed[at][0], (changed[at][1] + 1) % L)
                        put("coef-%s@%d" % (cname, i), "statement", "coef_" + cname, inst=circ.instance(rows[:i] + [changed] + rows[i + 1:], witness=False))
            put("drop-row", "statement", "drop_row", inst=circ.instance(rows[:len(rows) // 2] + rows[len(rows) // 2 + 1:], witness=False))
            put("label", "statement", "label", state=Circuit.transcript_state(b"AnotherLabel", circ.V))
            if circ.m >= 2:
                sw = circ.V[32:64] + circ.V[:32] + circ.V[64:]
                put("swap-V", "statement", "swap_V", V=sw, state=Circuit.transcript_state(circ.label, sw))
            for j in range(circ.m):
                other = O.pedersen_commit(le(h_int(b"other v", j, L)), le(h_int(b"other vb", j, L)))
                rv = circ.V[:32 * j] + other + circ.V[32 * j + 32:]
                put("replace-V_%d" % j, "statement", "replace_V", V=rv, state=Circuit.transcript_state(circ.label, rv))
            if circ.N >= 8:
                put("capacity-4", "statement", "capacity", capacity=4, decided=True)
            if circ.name == "big":
                put("capacity-512", "statement", "capacity", capacity=512, decided=True)
    return circs, bases, mutants


def content_key(r):
    i = r.circuit
    return (i.n, i.m, i.row_ptr.tobytes(), i.term_var.tobytes(), i.term_coef.tobytes(), i.coef, r.state, r.V, r.proof, r.seed, r.flags, r.capacity)


def expected_status(r):
    """the status the documented order of checks gives (R1CSProof::from_bytes, then the capacity, then validate_and_append_point, then the one MSM)"""
    if r.kind == "base":
        return O.OK
    if r.kind == "framing":
        return O.ERR_VERIFY if r.cls == "flags_same_length" else O.ERR_FORMAT
    if r.kind.startswith("scalar:"):
        return O.ERR_FORMAT if r.cls in NONCANONICAL_SCALARS else O.ERR_VERIFY
    if r.cls == "capacity":
        return O.ERR_GENS_LENGTH
    return O.ERR_VERIFY
