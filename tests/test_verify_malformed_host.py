"""The malformed-proof corpus of tests/verify_cases.py without a GPU: the conditions the corpus itself must meet (the oracle accepts every base
proof and rejects EVERY mutant, with the status the documented order of checks gives; every cell of the matrix is filled; no two records are
equal), the library's own host-side decisions through bpg_test_verify_replay (verify_replay alone: no context, no launch), and the host build
of the device decoder (hc_decompress: csrc/hip/ge.cuh compiled by g++) against pyref.decompress.

Nothing here is skipped or expected to fail: a mutant the oracle accepts means the generator is wrong."""
import collections
import ctypes as C
import pathlib
import subprocess
import pytest
import bulletproofs_gadgets_amd as bpg
import oracle_lib as O
import verify_cases as VC

HERE = pathlib.Path(__file__).resolve().parent


@pytest.fixture(scope="module")
def corpus():
    return VC.corpus()


@pytest.fixture(scope="module")
def hc():
    so, src = HERE / "hostcheck" / "libhostcheck.so", HERE / "hostcheck" / "hostcheck.cpp"
    hdrs = list((HERE.parent / "bulletproofs_gadgets_amd" / "csrc" / "hip").glob("*.cuh")) + [HERE.parent / "bulletproofs_gadgets_amd" / "csrc" / "host" / "fe51.hpp"]
    if not so.exists() or any(p.stat().st_mtime > so.stat().st_mtime for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(src)])
    return C.CDLL(str(so))


def test_oracle_accepts_every_base_and_rejects_every_mutant(corpus):
    circs, bases, mutants = corpus
    assert len(bases) == 4 * len(circs) == 24 and [r.status for r in bases] == [0] * 24
    assert {r.flags for r in bases} == {0, 1, 2, 3}
    accepted = [r.name for r in mutants if r.status == 0]
    assert accepted == []
    print("verify corpus: %d base proofs, %d mutants, %d records" % (len(bases), len(mutants), len(bases) + len(mutants)))


def test_status_follows_the_documented_order_of_checks(corpus):
    """format error: every wrong length, wrong lead byte and non-canonical scalar; verification error: identity and undecodable points, canonical
    but wrong scalars, equal-length dialect mismatches, every statement mutant; generator-length error: a capacity below N"""
    _, bases, mutants = corpus
    wrong = [(r.name, r.status, VC.expected_status(r)) for r in bases + mutants if r.status != VC.expected_status(r)]
    assert wrong == []
    by = collections.Counter(r.status for r in mutants)
    assert set(by) == {O.ERR_GENS_LENGTH, O.ERR_FORMAT, O.ERR_VERIFY} and all(by.values())
    for r in mutants:
        if r.cls in ("len_minus_1", "len_plus_1", "len_minus_32", "len_plus_32", "empty", "lead_byte", "flags_other_length") or r.cls in VC.NONCANONICAL_SCALARS:
            assert r.status == O.ERR_FORMAT, r.name
        if r.cls == "capacity":
            assert r.status == O.ERR_GENS_LENGTH, r.name


def test_every_cell_of_the_matrix_is_filled(corpus):
    circs, bases, mutants = corpus
    cells = collections.Counter((r.kind, r.cls, r.flags) for r in mutants)
    want = set()
    for fl in range(4):
        for kind in VC.POINT_KINDS:
            if kind == "A2" and fl & 1:
                continue                                                   # the compact dialects carry no second-phase points
            for cls in VC.POINT_CLASSES:
                if kind == "A2" and cls in ("identity", "negation"):
                    continue                                               # the identity's identity and negation: see verify_cases
                want.add((kind, cls, fl))
        want |= {("scalar:" + nm, cls, fl) for nm in VC.SCALAR_FIELDS for cls in VC.SCALAR_CLASSES}
        want |= {("framing", cls, fl) for cls in VC.FRAMING_CLASSES if cls != "lead_byte" or fl & 1}
        want |= {("statement", cls, fl) for cls in ["coef_" + k for k in VC.COEF_KINDS] + ["drop_row", "label", "swap_V", "replace_V", "capacity"]}
    assert want - set(cells) == set() and set(cells) - want == set()
    # every field of every base by name, the coefficient changes at every index, and every circuit in every dialect
    names = {r.name for r in mutants}
    for b in bases:
        circ = circs[b.name.split("/")[0]]
        for nm, (kind, _) in VC.fields(circ, b.flags).items():
            classes = VC.SCALAR_CLASSES if kind == "scalar" else VC.POINT_CLASSES
            got = [c for c in classes if "%s/%s=%s" % (b.name, nm, c) in names]
            hole = 2 if kind == "A2" else {"t_x": 3, "a": 3, "b": 2}.get(nm, 0) if circ.n == 0 else 0      # the holes verify_cases explains
            assert len(got) == len(classes) - hole, (b.name, nm, got)
    for fl in range(4):
        for i in VC.BIG_INDICES:
            for k in VC.COEF_KINDS:
                assert "big/f%d/coef-%s@%d" % (fl, k, i) in names
    big = circs["big"]
    assert (big.n, big.N, big.m) == (700, 1024, 3) and VC.BIG_INDICES[-1] == big.n - 1
    touched = {kind: set() for kind in (VC.KIND_L, VC.KIND_R, VC.KIND_O)}
    for row in big.rows:
        for pv, c in row:
            if pv >> 29 in touched and c % VC.L:
                touched[pv >> 29].add(pv & 0x1fffffff)
    assert all(t == set(range(big.n)) for t in touched.values())         # a weight change at any index matters
    s5 = circs["small5"]
    assert (s5.n, s5.N, s5.m) == (5, 8, 2) and {pv & 0x1fffffff for row in s5.rows for pv, _ in row if pv >> 29 == VC.KIND_V} == {0, 1}
    assert (circs["one"].n, circs["one"].lgN, circs["one"].m) == (1, 0, 1) and circs["none"].n == 0


def test_no_two_records_are_equal(corpus):
    _, bases, mutants = corpus
    seen = {}
    for r in bases + mutants:
        k = VC.content_key(r)
        assert k not in seen, (r.name, seen[k])
        seen[k] = r.name
    assert len({r.name for r in bases + mutants}) == len(bases) + len(mutants)


def test_host_replay_decides_what_it_must_and_nothing_else(corpus):
    """bpg_test_verify_replay = verify_replay alone.  Decided there, with the oracle's status: every wrong length, wrong lead byte, non-canonical
    scalar, capacity below N, another dialect's flags when the lengths differ, and the identity in a field with an identity rule (A_I1, A_O1, S1,
    T_k, L_k, R_k - the second-phase points and V have none: upstream appends them unvalidated, and they fail in the MSM).  Everything else -
    every base proof included - comes back undecided with status 0."""
    _, bases, mutants = corpus
    decided = collections.Counter()
    for r in bases + mutants:
        status, dec = bpg.test_verify_replay(r.circuit.n, r.circuit.m, r.capacity, r.state, r.proof, r.seed, r.flags)
        assert dec == r.decided, r.name
        assert status == (r.status if r.decided else 0), (r.name, status, r.status)
        decided[r.kind.split(":")[0], r.cls] += dec
    assert not any(r.decided for r in bases)
    for cell in [("framing", c) for c in VC.FRAMING_CLASSES if c != "flags_same_length"] + [("scalar", c) for c in VC.NONCANONICAL_SCALARS] + \
                [(k, "identity") for k in VC.IDENTITY_RULE_KINDS] + [("statement", "capacity")]:
        assert decided[cell] > 0, cell
    assert decided["framing", "flags_same_length"] == 0 and decided["V", "identity"] == 0


def test_replay_hook_checks_its_arguments(corpus):
    _, bases, _ = corpus
    r = bases[0]
    lib = bpg.lib()
    st, dec = C.c_int32(77), C.c_int32(77)
    args = lambda **kw: [kw.get(k, d) for k, d in (("n", C.c_uint64(r.circuit.n)), ("m", C.c_uint64(0)), ("cap", C.c_uint64(8)), ("ts", r.state), ("proof", r.proof),
                                                   ("len", C.c_uint64(len(r.proof))), ("seed", r.seed), ("flags", C.c_uint32(r.flags)), ("st", C.byref(st)), ("dec", C.byref(dec)))]
    for bad in (dict(ts=None), dict(seed=None), dict(st=None), dict(dec=None), dict(proof=None), dict(n=C.c_uint64(2**33))):
        assert lib.bpg_test_verify_replay(*args(**bad)) == 4, bad
        assert (st.value, dec.value) == (77, 77)
    assert lib.bpg_test_verify_replay(*args()) == 0 and (st.value, dec.value) == (0, 0)
    assert lib.bpg_test_decompress(None, C.c_uint64(1), bytes(32), (C.c_uint32 * 1)(), C.create_string_buffer(64)) == 7      # no device context


def test_host_build_of_the_decoder_matches_the_python_reference(hc, golden):
    """ge_decompress of csrc/hip/ge.cuh compiled for the host, through the Niels conversion k_decompress applies: accept / reject on every vector,
    x and y on the accepted ones, and their re-encoding, against Python big integers"""
    def run(encs):
        n = len(encs)
        ok, xy = (C.c_uint32 * n)(), C.create_string_buffer(64 * n)
        hc.hc_decompress(C.c_uint32(n), b"".join(encs), ok, xy)
        return list(ok), [(int.from_bytes(xy.raw[64 * i:64 * i + 32], "little"), int.from_bytes(xy.raw[64 * i + 32:64 * i + 64], "little")) for i in range(n)]
    vectors = VC.decoder_vectors(golden)
    counts = VC.check_decoder(run, vectors)
    VC.check_decoder_counts(counts)
    print("decoder vectors: %d %s" % (len(vectors), dict(counts)))
