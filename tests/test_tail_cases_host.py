"""The catalogue of tests/tail_cases.py, pinned without a device: each case really has the digit string its name claims under the integer model of both
recodings, the model agrees with the product's recoders (csrc/hip/sc.cuh tt_biased_words / tt8_biased_words, compiled for the host by tests/hostcheck), and the
two forms of the reference - folded points, and coefficients over the base points - give the same bytes."""
import ctypes as C
import hashlib
import pathlib
import subprocess

import pytest

import oracle_lib as O
import tail_cases as T

L = T.L
HERE = pathlib.Path(__file__).resolve().parent
E = T.edges()


@pytest.fixture(scope="module")
def hc():
    so, src = HERE / "hostcheck" / "libhostcheck.so", HERE / "hostcheck" / "hostcheck.cpp"
    hdrs = list((HERE.parent / "bulletproofs_gadgets_amd" / "csrc" / "hip").glob("*.cuh")) + [HERE.parent / "bulletproofs_gadgets_amd" / "csrc" / "host" / "fe51.hpp"]
    if not so.exists() or any(p.stat().st_mtime > so.stat().st_mtime for p in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", str(so), str(src)])
    return C.CDLL(str(so))


def all_scalars():
    """Every scalar a kernel recodes at sub-round 0 of a case with unit factors, every cw the catalogue aims at, every blinding, and the edges themselves."""
    seen = set(E.values())
    for lgM0 in (1, 2, 4, 5):
        M0 = 1 << lgM0
        for first, n in [(0, 0)] + [(1, n) for n in T.first_ns(M0)]:
            for c in T.tail_cases(lgM0, first, n):
                if c.yinv == c.gamma0 == c.eta0 == 1:
                    seen.update(c.a, c.b)
                    seen.update(s * c.u_ch % L for s in c.a + c.b)
    for n in (1, 3, 16):
        for c in T.commit_cases(n):
            seen.update(c.aL, c.aR, c.aO, c.sL, c.sR, c.blind)
    seen.update(T.thread_scalar(g) for g in range(8))
    return sorted(seen)


def hashed(count):
    return [int.from_bytes(hashlib.sha512(b"tail digits %d" % i).digest(), "little") % L for i in range(count)]


def test_the_model_sums_back_and_stays_in_range():
    scalars = all_scalars() + hashed(400)
    assert len(scalars) > 500 and all(0 <= s < L for s in scalars)
    for s in scalars:
        d4, d8 = T.digits4(s), T.digits8(s)
        assert len(d4) == 64 and len(d8) == 32
        assert T.from_digits(d4, 4) == s and all(-8 <= v <= 7 for v in d4) and d4[63] in (0, 1)
        assert T.from_digits(d8, 8) == s and all(-128 <= v <= 127 for v in d8) and 0 <= d8[31] <= 16
        assert (d4[63] == 1) == (s >= (1 << 252) - int("8" * 63, 16))


def test_the_product_recoders_give_the_model_digits(hc):
    """tt_biased_words / tt8_biased_words as the kernels extract their windows, against the textbook recoding: for the catalogue and 400 hashed scalars."""
    out = (C.c_int32 * 64)()
    for s in all_scalars() + hashed(400):
        hc.hc_tt_digits(0, out, T.sc(s))
        assert list(out) == T.digits4(s), hex(s)
        hc.hc_tt_digits(1, out, T.sc(s))
        assert list(out)[:32] == T.digits8(s), hex(s)


def test_edges_have_the_digit_strings_their_names_claim():
    assert set(T.F.named()) <= set(E) and len(E) == 31
    assert T.digits4(E["4: every window -8"]) == [-8] * 63 + [1]
    assert T.digits4(E["4: every window +7"]) == [7] * 63 + [0]
    assert T.digits4(E["4: 0x0888..8"]) == [-8] + [-7] * 62 + [1]
    assert T.digits8(E["8: every window -128"]) == [-128] * 31 + [1]
    assert T.digits8(E["8: every window +127"]) == [127] * 31 + [0]
    assert T.digits8(E["8: +127 below the top byte of l"]) == [127] * 31 + [15]
    for name, below, above in (("4: -8 | +7 at the word edges", -8, 7), ("4: +7 | -8 at the word edges", 7, -8)):
        d = T.digits4(E[name])
        assert all((d[8 * k - 1], d[8 * k]) == (below, above) for k in range(1, 8)), name
    for name, below, above in (("8: -128 | +127 at the word edges", -128, 127), ("8: +127 | -128 at the word edges", 127, -128)):
        d = T.digits8(E[name])
        assert all((d[4 * k - 1], d[4 * k]) == (below, above) for k in range(1, 8)), name
    # the only scalars whose window 63 is non-zero without a carry from below: [2^252, l)
    for name in ("2^252", "2^252+1", "l-1", "l-2"):
        s = E[name]
        assert s >= 1 << 252 and T.digits4(s)[63] == 1 and T.word_carries(s, 4)[:7][-1] == 0 and T.digits8(s)[31] == 16
    # carries: through every word under both biases (the last word never carries out: s + bias < 2^256)
    for bits in (4, 8):
        assert T.word_carries(E["carry through all words"], bits) == [1] * 7 + [0]
        assert T.word_carries(0, bits) == [0] * 8
    assert T.word_carries(E["4: every window -8"], 4) == [1] * 7 + [0] and T.word_carries(E["8: every window -128"], 8) == [1] * 7 + [0]
    assert T.word_carries(E["4: every window +7"], 4) == [0] * 8
    # every digit value of both tables occurs somewhere in the catalogue, with both signs of the largest
    seen4 = {v for s in E.values() for v in T.digits4(s)}
    seen8 = {v for s in E.values() for v in T.digits8(s)}
    assert seen4 == set(range(-8, 8)) and {-128, 127, 0, 1, 15, 16} <= seen8


def test_thread_scalars_light_one_thread():
    for g in range(8):
        s = T.thread_scalar(g)
        assert all(v == 0 for k, v in enumerate(T.digits4(s)) if k // 8 != g) and sum(1 for v in T.digits4(s) if v) >= 6
        assert all(v == 0 for k, v in enumerate(T.digits8(s)) if k // 4 != g) and sum(1 for v in T.digits8(s) if v) == 4
    cases = T.single_thread_cases(5)
    assert len(cases) == 2 * 32 * 8
    assert {(i, g) for c in cases for i, v in enumerate(c.a) if v for g in range(8) if v == T.thread_scalar(g)} == {(i, g) for i in range(32) for g in range(8)}
    assert all(sum(1 for v in c.a + c.b if v) == 1 for c in cases)


@pytest.mark.parametrize("lgM0", [1, 2, 4, 5, 6, 7])
def test_tail_lists_hold_what_the_gpu_test_relies_on(lgM0):
    M0, h = 1 << lgM0, 1 << (lgM0 - 1)
    ns = T.first_ns(M0)
    assert ns[0] == M0 and all(M0 // 2 < n <= M0 for n in ns) and (M0 < 4 or M0 // 2 + 1 in ns)
    if M0 >= 16:
        assert any(n % 8 and n % 32 for n in ns[2:3]) and (M0 < 128 or any(n % 32 == 0 and n < M0 for n in ns))
    full = T.tail_cases(lgM0, 0, 0)
    by = {c.name: c for c in full}
    assert len(full) == 31 + 7 + 24 + 8 + 3                                         # pinned: 31 edge pairs, 7 degenerate, 24 cw edges, 8 u and yinv, 3 ordinary
    unit = [c for c in full if c.yinv == c.u_ch == c.gamma0 == c.eta0 == 1]
    assert set(E.values()) <= {s for c in unit for s in c.a} and set(E.values()) <= {s for c in unit for s in c.b}
    z = by["a and b all zero"]
    assert not any(z.a) and not any(z.b) and z.w and z.yinv != 1
    for name in ("a perpendicular to b: cw = 0", "a perpendicular to b, ordinary factors"):
        c = by[name]
        assert T._dot(c.a[:h], c.b[h:]) == 0 and T._dot(c.a[h:], c.b[:h]) == 0 and any(c.a) and (any(c.b) or M0 == 2)
    for name in T.BLIND_EDGES:
        c = by["cw of L = %s" % name]
        assert T._dot(c.a[:h], c.b[h:]) * c.w % L == E[name]
        c = by["cw of R = %s" % name]
        assert T._dot(c.a[h:], c.b[:h]) * c.w % L == E[name]
    assert {by["every u = %s" % k].u[0] for k in ("1", "l-1", "2", "ordinary")} >= {1, L - 1, 2}
    assert {by["yinv = %s" % k].yinv for k in ("1", "l-1", "2", "ordinary")} >= {1, L - 1, 2}
    assert len(set(by["u all different"].u)) == lgM0 and by["gamma0 and eta0 ordinary"].gamma0 not in (0, 1)
    for n in ns:
        cases = T.tail_cases(lgM0, 1, n)
        pad = [c for c in cases if c.name.startswith("padding")]
        assert len(pad) == 10 and {c.u_ch for c in pad} >= {1, T.ordinary(5)}
        assert {c.a[0] * c.u_ch % L for c in pad} >= {E["4: every window -8"], E["8: every window +127"], E["l-1"], 1}
        assert len(cases) == (83 if n == M0 or n == ns[min(2, len(ns) - 1)] else 10)      # the whole list where nothing is padded and at one padded n


def test_commit_lists_hold_their_edges():
    for n in (1, 2, 3, 9, 16, 33, 64):
        cases = T.commit_cases(n)
        for k in range(5):
            assert set(E.values()) <= {s for c in cases for s in c[1 + k]}, (n, k)
        for k in range(3):
            assert {E[name] for name in T.BLIND_EDGES} <= {c.blind[k] for c in cases}
        z = {c.name: c for c in cases}["all zero"]
        assert not any(z.aL + z.aR + z.aO + z.sL + z.sR + z.blind)
        assert all(len(v) == n for c in cases for v in c[1:6]) and all(0 <= s < L for c in cases for v in c[1:] for s in v)


@pytest.fixture(scope="module")
def gens():
    g, h = O.Gens(32).export(0, 32)
    return T.split_points(g), T.split_points(h), O.pedersen_bases()


@pytest.mark.parametrize("lgM0,first,n", [(1, 0, 0), (2, 1, 3), (4, 0, 0), (4, 1, 14), (5, 1, 27)])
def test_both_forms_of_the_reference_agree(gens, lgM0, first, n):
    """Folded points against coefficients over the base points, on the oracle's own generators; and the degenerate cases give the identity."""
    G, H, (B, _) = gens
    cases = {c.name: c for c in T.tail_cases(lgM0, first, n)}
    picked = [c for name, c in cases.items() if name in ("every factor ordinary", "padding: u_ch and every factor ordinary", "a and b all zero",
                                                         "a perpendicular to b, ordinary factors", "every u = l-1", "yinv = 2")]
    assert len(picked) >= 5
    for c in picked:
        want = T.tail_reference(G, H, B, c, lgM0, first, n, lgM0)
        assert T.tail_reference_expanded(G, H, B, c, lgM0, first, n, lgM0) == want, c.name
        assert len(want[0]) == lgM0 and len(want[1]) == len(want[2]) == 1
        if c.name == "a and b all zero":
            assert want == ([(T.IDENTITY, T.IDENTITY)] * lgM0, [0], [0])


def test_the_reference_round_is_the_provers_round(gens):
    """One round of the reference against the invariant the argument rests on: P' = u^2 L + P + u^-2 R for P = <a, G> + <b, H> + <a, b> w B, on the folded
    vectors and generators - no kernel and no recoder involved."""
    G, H, (B, _) = gens
    lgM0, M0 = 3, 8
    c = {c.name: c for c in T.tail_cases(lgM0, 0, 0)}["every factor ordinary"]
    _, G0, H0 = T._start(G, H, c, M0, 0, 0)
    commit = lambda a, b, Gv, Hv: T._msm(list(a) + list(b) + [T._dot(a, b) * c.w], list(Gv) + list(Hv) + [B])
    (Lp, Rp), = T.tail_reference(G, H, B, c, lgM0, 0, 0, 1)[0]
    u, ui, h = c.u[0], T.inv(c.u[0]), M0 // 2
    a1, b1 = T.tail_reference(G, H, B, c, lgM0, 0, 0, 1)[1:]
    G1, H1 = [T._msm([ui, u], [G0[i], G0[h + i]]) for i in range(h)], [T._msm([u, ui], [H0[i], H0[h + i]]) for i in range(h)]
    assert commit(a1, b1, G1, H1) == T._msm([u * u, 1, ui * ui], [Lp, commit(c.a, c.b, G0, H0), Rp])


def test_tail_hooks_without_device_fail_loudly():
    """bpg_test_tail and bpg_test_commit3 have no CPU path: without a context they are a DEVICE_ERROR, and nothing is written"""
    import bulletproofs_gadgets_amd as bpg
    one = T.sc(1)
    lr, ab, ev = (C.create_string_buffer(b"\x5a" * 64, 64) for _ in range(3))
    ev = C.create_string_buffer(b"\x5a" * 512, 512)
    rc = bpg.lib().bpg_test_tail(None, C.c_uint32(1), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), one * 2, one * 2, one, one, one, one, one, C.c_uint32(1), one,
                                 lr, ab, ev, C.c_uint64(512))
    assert rc == 7 and b"device" in bpg.lib().bpg_last_error()
    assert lr.raw == b"\x5a" * 64 and ab.raw == b"\x5a" * 64 and ev.raw == b"\x5a" * 512
    out = C.create_string_buffer(b"\x5a" * 96, 96)
    rc = bpg.lib().bpg_test_commit3(None, C.c_uint32(0), C.c_uint64(1), one, one, one, one, one, one * 3, out, ev, C.c_uint64(512))
    assert rc == 7 and b"device" in bpg.lib().bpg_last_error()
    assert out.raw == b"\x5a" * 96 and ev.raw == b"\x5a" * 512
