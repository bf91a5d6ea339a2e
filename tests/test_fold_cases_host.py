"""The catalogue of tests/fold_cases.py, pinned without a device: every scalar is canonical, the integer model of the recodings is sound, and the case lists
hold what test_fold_kernels_gpu.py relies on them to hold - each property derived from the lists by the model, never assumed from a case's name."""
import re

import pytest

import fold_cases as F
import oracle_lib as O

L = F.L
PLAN = (O.ROOT / "bulletproofs_gadgets_amd" / "csrc" / "host" / "fold_plan.hpp").read_text()
QW_MAXSTEPS = int(re.search(r"#define QW_MAXSTEPS (\d+)", PLAN).group(1))
MAX_DOUBLINGS = int(re.search(r"pending > (\d+)\) throw", PLAN).group(1))          # the 8-bit doublings field of a step

BITMAP_LISTS = {(nt, first): F.bitmap_cases(nt, first) for nt in (1, 3, 7, 15, 31) for first in (0, 1)}
STEP_LISTS = [F.steps_cases(nt) for nt in (1, 3, 7)]
WNAF_LISTS = {(w, parts, nt, first): F.wnaf_cases(w, parts, nt, first) for w, parts in F.WNAF_PROFILES for nt in (3, 7) for first in (0, 1)}


def all_scalars():
    seen = set()
    for cases in list(BITMAP_LISTS.values()) + STEP_LISTS + list(WNAF_LISTS.values()):
        for _, sG, sH, u in cases:
            seen.update(sG, sH, (u,))
            seen.update(s * u % L for s in sG + sH)
    return sorted(seen)


def test_constants_of_the_header():
    assert QW_MAXSTEPS == 1024 and MAX_DOUBLINGS == 255
    assert "doublings before the addition | term << 8 | multiple << 11 | sign << 13" in PLAN


def test_every_scalar_is_canonical_and_the_model_sums_back():
    scalars = all_scalars()
    assert len(scalars) > 150 and all(0 <= s < L for s in scalars)
    assert set(F.named().values()) <= set(scalars) and len(F.named()) == 19
    for s in scalars:
        for w in range(2, 9):
            d = F.wnaf(s, w)
            assert F.value_of(d) == s
            nz = [k for k, v in enumerate(d) if v]
            assert all(d[k] & 1 and abs(d[k]) < 1 << (w - 1) for k in nz)
            assert all(b - a >= w for a, b in zip(nz, nz[1:]))                 # at most one non-zero digit in any w consecutive positions
            assert F.top_of(d) == (nz[-1] if nz else -1) and F.top_of(d) <= 253
        for parts in (1, 2, 4, 8):
            Lb = F.part_bits(parts)
            pieces = F.cut(s, parts)
            assert sum(p << (k * Lb) for k, p in enumerate(pieces)) == s and all(0 <= p < 1 << Lb for p in pieces)
            assert all(F.top_of(F.wnaf(p, w)) <= Lb for p in pieces for w in (3, 8))


def test_width_extremes_are_the_digits_they_were_built_from():
    for w in range(3, 9):
        m, J = (1 << (w - 1)) - 1, 252 // w + 1
        for name, pick in (("+", F.pick_max(w)), ("-", F.pick_min(w)), ("+-", F.pick_alt(w, 0)), ("-+", F.pick_alt(w, 1))):
            d = F.wnaf(F.width_extreme(w, pick), w)
            assert all(d[w * j] == pick(j) for j in range(J - 1)), (w, name)
            assert all(v == 0 for k, v in enumerate(d) if k % w), (w, name)
        assert m in F.wnaf(F.width_extreme(w, F.pick_max(w)), w) and -m in F.wnaf(F.width_extreme(w, F.pick_min(w)), w)
    d = F.wnaf(F.width_extreme(4, F.pick_turn), 4)
    assert [d[4 * j] for j in range(8)] == [1, -1, 3, -3, 5, -5, 7, -7]
    # the densest width-4 scalar: a digit at every fourth position up to 252, which only a negative run below the top digit keeps below l
    assert sum(1 for v in F.wnaf(F.width_extreme(4, F.pick_min(4)), 4) if v) == 64


def test_the_step_model_replays_to_the_sum():
    """The step list of the model, replayed on integers: acc = sum_t s_t x_t, as tests/hostcheck/plans.cpp replays the recoder's."""
    for cases in STEP_LISTS:
        for name, sG, sH, _ in cases:
            for ss in (sG, sH):
                x = [F.ordinary(50 + t) for t in range(len(ss))]
                steps, tail = F.step_list(ss)
                acc = 0
                for k, (dbl, q, mag, neg) in enumerate(steps):
                    assert (dbl == 0 if k == 0 else dbl >= 0) and mag in (1, 3, 5, 7) and q < len(ss), name
                    acc = (acc << dbl) + (-mag if neg else mag) * x[q]
                assert (acc << tail) == sum(s * v for s, v in zip(ss, x)), name


def test_bitmap_lists_hold_their_edges():
    for (nterms, first), cases in BITMAP_LISTS.items():
        assert len(cases) == (40 if first else 29)                      # pinned: 19 named, 10 mixed, 11 in the padding class of a first group
        pred = [F.predict_bitmap(c, first) for c in cases]
        tops = [p["top"] for p in pred]
        assert {-1, 0, 1, 252} <= set(tops) and max(tops) == 252
        assert min(p["adds"] for p in pred) == 0 and max(p["adds"] for p in pred) >= 126 * nterms          # 0x0555..5: a digit at every second position
        words = set()                                                   # bits on both sides of the 32-bit word edges of the bitmaps
        for c in cases:
            for cls in F.class_scalars(c, first):
                for s in cls:
                    words.update(k for k, v in enumerate(F.naf(s)) if v)
        assert {0, 31, 32, 223, 224, 252} <= words
        # terms of one launch with very different tops: a scalar of top <= 1 beside one of top 252
        assert any({t for cls in F.class_scalars(c, first) for t in (F.top_of(F.naf(s)) for s in cls)} >= {-1, 0, 252} for c in cases) or nterms < 3
        if first:
            edges = {s * c[3] % L for c in cases for s in c[1] if c[3] != 1}
            v = F.named()
            assert {v["0"], v["1"], v["l-1"], v["2^252"], v["0x0555..5"]} <= edges and any(c[3] == 1 for c in cases[29:])


def test_step_lists_hold_their_edges():
    pairs = set()
    for cases in STEP_LISTS:
        nterms = len(cases[0][1])
        assert len(cases) == 36                                         # pinned: 19 named, 10 mixed, 5 patterns, 2 term by term
        pred = [F.predict_steps(c) for c in cases]
        assert max(p["max_doublings"] for p in pred) == 252 and max(p["max_doublings"] for p in pred) <= MAX_DOUBLINGS
        assert max(max(p["nsteps"]) for p in pred) == 64 * nterms <= QW_MAXSTEPS          # 448 at seven terms
        assert max(max(p["tail"]) for p in pred) >= 200 and max(max(p["tail"]) for p in pred) <= 252
        assert [0, 64 * nterms] in [p["nsteps"] for p in pred] and [64 * nterms, 0] in [p["nsteps"] for p in pred] and [0, 0] in [p["nsteps"] for p in pred]
        assert any(min(p["nsteps"]) == nterms and max(p["nsteps"]) == 64 * nterms for p in pred)          # G and H lists of very different length
        assert any(p["nsteps"][0] == nterms and p["tail"][0] == 252 for p in pred)                          # 2^252: one step per term, then 252 doublings
        for _, sG, sH, _ in cases:
            for ss in (sG, sH):
                pairs.update((mag, neg) for _, _, mag, neg in F.step_list(ss)[0])
    assert pairs == {(m, s) for m in (1, 3, 5, 7) for s in (False, True)}
    # the controlled pattern: every term of the G side of "one multiple per term" adds one multiple with one sign, below its top digit
    case = dict((c[0], c) for c in F.steps_cases(7))["one multiple per term"]
    for t, s in enumerate(case[1]):
        d = [v for v in F.wnaf(s, 4) if v]
        assert len(set(d[:-1])) == 1 and abs(d[0]) == (1, 3, 5, 7)[t % 4], t


def test_wnaf_lists_hold_their_edges():
    assert sorted({w for w, _ in F.WNAF_PROFILES}) == [3, 4, 5, 6, 7, 8] and sorted({p for _, p in F.WNAF_PROFILES}) == [1, 2, 4, 8]
    for (w, parts, nterms, first), cases in WNAF_LISTS.items():
        # pinned: 19 named, 10 mixed, 4 width patterns (5 at width 4), 6 part patterns, 14 in the padding class of a first group
        assert len(cases) == (53 if first else 39) + (w == 4), (w, parts)
        Lb, m = F.part_bits(parts), (1 << (w - 1)) - 1
        digits, tops, zero_part = set(), set(), False
        for c in cases:
            for cls in F.class_scalars(c, first):
                for s in cls:
                    pieces = F.cut(s, parts)
                    zero_part |= 0 in pieces
                    for p in pieces:
                        d = F.wnaf(p, w)
                        digits.update(d)
                        tops.add(F.top_of(d))
        assert m in digits and -m in digits, (w, parts)                 # the last table of odd multiples, with both signs
        assert zero_part and -1 in tops
        # a piece of 2^Lb - 1 carries a digit into position Lb.  One piece (Lb = 254) cannot: a scalar below l < 2^253 has no digit above 252, which it reaches
        assert max(tops) == (Lb if parts > 1 else 252), (w, parts)
        launch = [F.predict_wnaf(c, first, w, parts) for c in cases]
        assert {p["top"] for p in launch} >= {-1, 0, Lb if parts > 1 else 252}
        assert all(p["part_bits"] == Lb for p in launch)


@pytest.mark.parametrize("Mr,rounds,ns", [(64, 2, (256, 129, 213, 192)), (32, 3, (256, 129, 213, 192))])
def test_padding_shapes_take_both_kinds_of_wave(Mr, rounds, ns):
    """The four n of a first group: no padding, all the padding there is, a class boundary inside a wave, one on a multiple of 64."""
    g_M, nterms = Mr << rounds, (1 << rounds) - 1
    assert ns[0] == g_M and ns[1] == g_M // 2 + 1 and ns[3] % 64 == 0 and ns[2] % 64 and all(g_M // 2 < n <= g_M for n in ns)
    pads = [sum(F.padding(i, t, Mr, n, 1) for i in range(Mr) for t in range(1, nterms + 1)) for n in ns]
    assert pads == [g_M - n for n in ns]
    if Mr == 64:            # one wave per side with one lane per output: uniform unless the boundary falls inside it
        assert [F.wave_classes(Mr, nterms, n, 1) for n in ns] == [(2, 0), (0, 2), (0, 2), (2, 0)]
        assert F.wave_classes(Mr, nterms, 213, 1, 4) == (6, 2) and F.wave_classes(Mr, nterms, 192, 1, 4) == (8, 0)
    else:                   # G and H meet in one wave: per-lane throughout
        assert all(F.wave_classes(Mr, nterms, n, 1) == (0, 1) for n in ns)
    assert F.wave_classes(1, 1, 0, 0) == (0, 1) and F.wave_classes(16, 3, 0, 0) == (0, 1) and F.wave_classes(64, 3, 0, 0) == (2, 0)


def test_fold_hook_without_device_fails_loudly():
    """bpg_test_fold has no CPU path: without a context it is a DEVICE_ERROR, and nothing is written"""
    import ctypes as C
    import bulletproofs_gadgets_amd as bpg
    one = F.sc(1)
    out, ev = C.create_string_buffer(b"\x5a" * 64, 64), C.create_string_buffer(b"\x5a" * 512, 512)
    rc = bpg.lib().bpg_test_fold(None, C.c_int32(-1), C.c_uint32(0), C.c_uint32(1), C.c_uint32(0), C.c_uint64(0), one, one, one, out, ev, C.c_uint64(512))
    assert rc == 7 and b"device" in bpg.lib().bpg_last_error()
    assert out.raw == b"\x5a" * 64 and ev.raw == b"\x5a" * 512
