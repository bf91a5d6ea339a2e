"""The bucket-method MSM (hip/k_msm.cuh) branch by branch, at the sizes and skews that take each branch, through bpg_test_msm.

Every case compares the sum with the CPU oracle (O.msm over the terms the segment mapping selects, on the device's own generator table as
gens_export gives it), predicts every bucket's entry count from a model of the signed-digit recoding and compares it with the starts[] the
kernels left, predicts the heavy and medium lists of the combine step from those counts, and shows from that evidence - never from a threshold
written here - that the branch it exists for ran:
  k_msm_sort2                 a coarse bin (2^fb consecutive buckets) of at most sort2_regs entries is held in registers, of at most msm_stash
                              entries stashes its slots in LDS, a larger one takes its slots with LDS atomics a second time
  k_bucket_combine(_heavy)    a bucket over more than heavy_chunks + 1 chunks is heavy (more than heavy_blocks of them: the grid-stride loop
                              takes a second trip); in boundary mode one over 3 .. heavy_chunks + 1 chunks goes on the medium list
  plans                       up to 4 results, 16 segments, strided segments (lgblk), skip masks, empty results, segments beyond 2^20 (fb < 7)
"""
import functools

import numpy as np
import pytest

import bulletproofs_gadgets_amd as bpg
import oracle_lib as O

pytestmark = pytest.mark.gpu

L = bpg.L
CAP = 1 << 20          # generators of the module's context: the production plan's two 2^20 segments


def sc(x):
    return (x % L).to_bytes(32, "little")


def limbs(v):
    return np.frombuffer(sc(v), dtype="<u4")


def rand_scalars(n, seed):
    """n uniform scalars below 2^252 (< l), as an (n, 8) array of little-endian 32-bit limbs."""
    a = np.random.default_rng(seed).integers(0, 1 << 32, size=(n, 8), dtype=np.uint64).astype(np.uint32)
    a[:, 7] &= 0x0FFFFFFF
    return a


def seg(table, first, length, result, lgblk=31, skip=None):
    return {"table": table, "first": first, "len": length, "result": result, "lgblk": lgblk, "skip": skip}


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(CAP)
    yield c
    c.close()


@pytest.fixture(scope="module")
def table(ctx):
    """The device's generator table [G | H] as compressed points, (2, CAP, 32) uint8."""
    G, H = ctx.gens_export(0, CAP)
    return np.stack([np.frombuffer(G, np.uint8).reshape(CAP, 32), np.frombuffer(H, np.uint8).reshape(CAP, 32)])


@pytest.fixture
def make_ctx(monkeypatch):
    """A fresh context with the given environment knobs (they are read once, at context creation)."""
    made = []

    def make(cap=CAP, **env):
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


class Terms:
    """The terms of one call in global order (segments in order, elements in order): scalar limbs, result, generator, live (not skipped)."""

    def __init__(self, segments, S):
        self.segments, self.S = segments, S
        n = sum(g["len"] for g in segments)
        assert S.shape == (n, 8)
        self.res = np.empty(n, np.int64)
        self.tab = np.empty(n, np.int64)
        self.gen = np.empty(n, np.int64)
        self.live = np.ones(n, bool)
        t = 0
        for g in segments:
            e = np.arange(g["len"], dtype=np.int64)
            lg = g["lgblk"]
            self.res[t:t + g["len"]] = g["result"]
            self.tab[t:t + g["len"]] = 0 if g["table"] in ("G", 0) else 1
            self.gen[t:t + g["len"]] = g["first"] + (e if lg >= 31 else ((e >> lg) << (lg + 1)) | (e & ((1 << lg) - 1)))
            if g["skip"] is not None:
                w = np.array(g["skip"], dtype=np.uint32)
                self.live[t:t + g["len"]] = ((w[e >> 5] >> (e & 31).astype(np.uint32)) & 1) == 0
            t += g["len"]

    def scalar_bytes(self):
        return np.ascontiguousarray(self.S, dtype="<u4").tobytes()

    def oracle(self, nmsm, table):
        """O.msm of each result over its live terms with a non-zero scalar (the others add nothing); the identity encodes as 32 zero bytes."""
        nz = self.S.any(axis=1) & self.live
        out = []
        for m in range(nmsm):
            k = nz & (self.res == m)
            if not k.any():
                out.append(bytes(32))
                continue
            pts = table[self.tab[k], self.gen[k]]
            out.append(O.msm(np.ascontiguousarray(self.S[k]).tobytes(), np.ascontiguousarray(pts).tobytes(), 1))
        return out


def digits(S, off):
    """The recoding of k_msm_digits: bias = sum_j 2^(off(j+1) - 1) added once, digit j = field_j(s + bias) - 2^(wd(j) - 1).  (n, W) int64."""
    W = len(off) - 1
    bias = sum(1 << (off[j + 1] - 1) for j in range(W))
    X = np.zeros((S.shape[0], 9), np.uint64)
    carry = np.zeros(S.shape[0], np.uint64)
    for k in range(8):
        t = S[:, k].astype(np.uint64) + np.uint64((bias >> (32 * k)) & 0xFFFFFFFF) + carry
        X[:, k] = t & np.uint64(0xFFFFFFFF)
        carry = t >> np.uint64(32)
    assert not carry.any()
    D = np.empty((S.shape[0], W), np.int64)
    for j in range(W):
        o, wd = off[j], off[j + 1] - off[j]
        two = X[:, o >> 5] | (X[:, (o >> 5) + 1] << np.uint64(32))
        D[:, j] = ((two >> np.uint64(o & 31)) & np.uint64((1 << wd) - 1)).astype(np.int64) - (1 << (wd - 1))
    return D


def digits_of(v, off):
    return digits(limbs(v)[None, :], off)[0]


def predicted_counts(terms, ev):
    """Entries per bucket key (result * W + window) * nb + |digit| - 1 of the live terms with a non-zero digit."""
    W, nb = ev["W"], ev["nb"]
    counts = np.zeros(ev["nkeys"], np.int64)
    D = digits(terms.S, ev["off"])
    for j in range(W):
        d = D[:, j]
        k = terms.live & (d != 0)
        counts += np.bincount((terms.res[k] * W + j) * nb + np.abs(d[k]) - 1, minlength=ev["nkeys"])
    return counts


def spans(starts, CH):
    """For every non-empty bucket: c1 - c0, the chunk boundaries it crosses."""
    s0, s1 = starts[:-1], starts[1:]
    ne = s1 > s0
    return (s1[ne] - 1) // CH - s0[ne] // CH


def bins(starts, ev):
    """Entries of every coarse bin (2^fb consecutive buckets), and how many non-empty ones take each shape of k_msm_sort2."""
    b = np.diff(starts[::1 << ev["fb"]])
    assert b.size == ev["nmsm"] * ev["W"] * ev["CB"]
    shapes = {"regs": int(((b > 0) & (b <= ev["sort2_regs"])).sum()),
              "stash": int(((b > ev["sort2_regs"]) & (b <= ev["msm_stash"])).sum()),
              "atomic": int((b > ev["msm_stash"]).sum())}
    return b, shapes


def run(c, nmsm, segments, S, table, want=None):
    """One bpg_test_msm call, checked: the sums against the oracle (or `want`), every bucket count against the model, the combine lists
    against the prediction from those counts.  Returns the evidence with the starts as an array."""
    terms = Terms(segments, S)
    got, ev = c.test_msm(nmsm, segments, terms.scalar_bytes())
    starts = np.array(ev["starts"], dtype=np.int64)
    ev["starts"] = starts
    assert ev["nmsm"] == nmsm and starts.size == ev["nkeys"] + 1 == nmsm * ev["W"] * ev["nb"] + 1
    assert ev["nb"] == ev["CB"] << ev["fb"] and ev["off"][0] == 0 and ev["off"][-1] == 254
    assert ev["live"] == int(terms.live.sum()) and ev["skipped"] == terms.live.size - ev["live"]
    assert ev["window_sums"] == ("plain" if ev["shared"] else "quad")
    counts = predicted_counts(terms, ev)
    assert np.array_equal(starts, np.concatenate([[0], np.cumsum(counts)])), "bucket counts differ from the recoding model"
    sp = spans(starts, ev["CH"])
    assert starts[-1] <= ev["nchunks"] * ev["CH"]
    assert ev["heavy"] == int((sp > ev["heavy_chunks"]).sum()), "heavy list"
    if ev["combine"] == "boundary":
        assert ev["medium"] == int(((sp >= 2) & (sp <= ev["heavy_chunks"])).sum()), "medium list"
    else:
        assert ev["combine"] == "per_bucket" and ev["medium"] == 0
    if want is None:
        want = terms.oracle(nmsm, table)
    assert got == want, "MSM sums differ from the oracle"
    return ev


def probe(c, segments):
    """The plan a call of this shape takes (it depends on the term and skip counts, not on the scalars): the same call on zero scalars."""
    n = sum(g["len"] for g in segments)
    _, ev = c.test_msm(max(g["result"] for g in segments) + 1, segments, bytes(32 * n))
    assert not any(ev["starts"])
    return ev


def fill(n, groups, seed):
    """n terms: zero scalars, with groups = [(value, count), ...] of equal non-zero scalars spread over the range (every other term first)."""
    S = np.zeros((n, 8), np.uint32)
    order = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)])
    order = order[np.random.default_rng(seed).permutation(order.size)] if seed is not None else order
    t = 0
    for v, cnt in groups:
        S[order[t:t + cnt]] = limbs(v)
        t += cnt
    assert t <= n
    return S


def values(k, seed, off):
    """k distinct scalars below l whose digit is non-zero in every window of `off`, at least one of them negative."""
    out, rng = [], np.random.default_rng(seed)
    while len(out) < k:
        v = int.from_bytes(rng.bytes(32), "little") % L
        d = digits_of(v, off)
        if d.all() and (d < 0).any() and v not in out:
            out.append(v)
    return out


# ---------------------------------------------------------------------------------------------------- k_msm_sort2: the three shapes of a bin
TWO16 = [seg("G", 0, 1 << 16, 0), seg("H", 0, 1 << 16, 0)]          # 2^17 terms: 20 windows of 13 bits, 32 coarse bins of 128 buckets


@pytest.mark.parametrize("edge", ["regs", "regs+1", "stash", "stash+1", "atomic"])
def test_sort2_bin_shape_at_its_edge(ctx, table, edge):
    """n equal non-zero scalars among zeros: one bin per window holds exactly n entries.  n at both sides of each shape's limit."""
    ev0 = probe(ctx, TWO16)
    n = {"regs": ev0["sort2_regs"], "regs+1": ev0["sort2_regs"] + 1, "stash": ev0["msm_stash"], "stash+1": ev0["msm_stash"] + 1,
         "atomic": 60000}[edge]
    v, = values(1, 7, ev0["off"])
    ev = run(ctx, 1, TWO16, fill(1 << 17, [(v, n)], seed=1), table)
    assert ev["off"] == ev0["off"]
    b, shapes = bins(ev["starts"], ev)
    assert (b == n).sum() == ev["W"] and (b[b != n] == 0).all()
    shape = "regs" if n <= ev["sort2_regs"] else "stash" if n <= ev["msm_stash"] else "atomic"
    assert shapes[shape] == ev["W"], shapes


def test_sort2_all_three_shapes_in_one_launch(ctx, table):
    ev0 = probe(ctx, TWO16)
    r, s = ev0["sort2_regs"], ev0["msm_stash"]
    v = values(3, 8, ev0["off"])
    ev = run(ctx, 1, TWO16, fill(1 << 17, [(v[0], r // 2), (v[1], (r + s) // 2), (v[2], s + 4000)], seed=2), table)
    _, shapes = bins(ev["starts"], ev)
    assert shapes["regs"] >= 1 and shapes["stash"] >= 1 and shapes["atomic"] >= 1, shapes


# ---------------------------------------------------------------------------------------------------- the production plan
PROD = [seg("G", 0, 1 << 20, 0), seg("H", 0, 1 << 20, 0)]


@functools.lru_cache(maxsize=1)
def prod_terms():
    S = rand_scalars(1 << 21, 2020)
    S[::4099] = limbs(L - 1)
    terms = Terms(PROD, S)
    return S, terms


@pytest.fixture(scope="module")
def prod_want(table):
    _, terms = prod_terms()
    return terms.oracle(1, table)


def test_production_plan_alone(ctx, table, prod_want):
    """2^20 + 2^20 random terms, a proof alone on the device: 17 windows of (up to) 15 bits, 128 coarse bins, quad window sums; bins on both
    sides of msm_stash."""
    S, _ = prod_terms()
    ev = run(ctx, 1, PROD, S, table, want=prod_want)
    assert ev["W"] == 17 and max(np.diff(ev["off"])) == 15 and ev["CB"] == 128 and not ev["shared"]
    assert ev["window_sums"] == "quad" and ev["window_blocks"] >= 1
    _, shapes = bins(ev["starts"], ev)
    assert shapes["stash"] >= 1 and shapes["atomic"] >= 1, shapes


def test_production_plan_shared_variants(make_ctx, table, prod_want):
    """The same sum with the shared-device variants (BPG_FOLD_ADAPT=2): 16-bit windows, 64-entry chunks, plain window sums."""
    S, _ = prod_terms()
    ev = run(make_ctx(BPG_FOLD_ADAPT=2), 1, PROD, S, table, want=prod_want)
    assert ev["shared"] and ev["W"] == 16 and max(np.diff(ev["off"])) == 16 and ev["CH"] == 64
    assert ev["window_sums"] == "plain" and ev["window_threads"] >= 64
    _, shapes = bins(ev["starts"], ev)
    assert shapes["stash"] + shapes["atomic"] >= 1, shapes


# ---------------------------------------------------------------------------------------------------- heavy and medium lists
MODES = {"boundary": 6, "per_bucket": 2}           # BPG_LGCH: long chunks (CH * nkeys >= entries: boundary threads), short ones (per bucket)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("kind", ["many_heavy", "one_long", "medium_only"])
def test_combine_lists(make_ctx, table, mode, kind):
    c = make_ctx(BPG_LGCH=MODES[mode])
    ev0 = probe(c, TWO16)
    assert ev0["combine"] == mode
    CH, HC, W = ev0["CH"], ev0["heavy_chunks"], ev0["W"]
    if kind == "many_heavy":           # each value's bucket of every window is heavy: more of them than the heavy kernel has blocks
        nv = (ev0["heavy_blocks"] * 5 // 4) // W + 1
        groups = [(v, (HC + 2) * CH) for v in values(nv, 11, ev0["off"])]
    elif kind == "one_long":           # one bucket per window over thousands of chunks
        groups = [(values(1, 12, ev0["off"])[0], min(2000 * CH, 1 << 17))]
    else:                              # buckets over 8 or 9 chunks, and random terms
        groups = [(v, 8 * CH) for v in values(40, 13, ev0["off"])]
    S = fill(1 << 17, groups, seed=3)
    if kind == "medium_only":
        idx = np.flatnonzero(~S.any(axis=1))[:4096]
        S[idx] = rand_scalars(idx.size, 14)
    ev = run(c, 1, TWO16, S, table)
    assert ev["combine"] == mode and ev["CH"] == CH
    sp = spans(ev["starts"], CH)
    if kind == "many_heavy":
        assert ev["heavy"] > ev["heavy_blocks"], ev["heavy"]
    elif kind == "one_long":
        assert ev["heavy"] >= 1 and sp.max() + 1 >= 2000
    else:
        assert ev["heavy"] == 0
        assert ((sp >= 2) & (sp <= HC)).sum() >= 1
        if mode == "boundary":
            assert ev["medium"] >= 1


# ---------------------------------------------------------------------------------------------------- plans with several results and segments
def test_four_results_of_very_uneven_sizes(ctx, table):
    segments = [seg("G", 5, 1, 0), seg("H", 10, 3, 1), seg("G", 100, (1 << 12) + 1, 2), seg("G", 0, 1 << 16, 3), seg("H", 0, 1 << 16, 3)]
    n = sum(g["len"] for g in segments)
    S = rand_scalars(n, 21)
    S[0] = limbs(L - 1)
    ev = run(ctx, 4, segments, S, table)
    assert ev["tmax"] == 32


def test_empty_zero_and_skipped_results(ctx, table):
    """Result 1 has no segment, result 2 only zero scalars, result 3 only skipped terms: all three are the identity."""
    segments = [seg("G", 0, 5000, 0), seg("G", 7, 3000, 2), seg("H", 9, 1000, 2), seg("H", 0, 2000, 3, skip=[0xFFFFFFFF] * 63)]
    S = rand_scalars(11000, 22)
    S[5000:9000] = 0
    ev = run(ctx, 4, segments, S, table)
    assert ev["skipped"] == 2000


def test_sixteen_segments_with_length_one(ctx, table):
    lens = [1, 1, 700, 1, 5000, 33, 1, 4096, 4097, 1, 12, 1 << 15, 1, 300, 1, 9000]
    res = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2]
    segments = [seg("GH"[k & 1], (k * 997) % 50000, n, r) for k, (n, r) in enumerate(zip(lens, res))]
    S = rand_scalars(sum(lens), 23)
    S[::5] = limbs(12345)                  # equal scalars across segments and results
    S[1] = limbs(L - 1)
    ev = run(ctx, 3, segments, S, table)
    assert len(segments) == 16


def test_strided_segments(ctx, table):
    """lgblk 0..10, as the grouped inner-product rounds push them: every other block of 2^lgblk generators, from the first or the second block."""
    segments, r = [], 0
    for lg in range(11):
        segments.append(seg("GH"[lg & 1], (lg & 2) << lg >> 1, 3000 + 700 * lg, r))
        segments[-1]["lgblk"] = lg
        r += lg in (3, 7)
    S = rand_scalars(sum(g["len"] for g in segments), 24)
    ev = run(ctx, 3, segments, S, table)
    assert ev["nmsm"] == 3


def test_skip_masks(ctx, table):
    """Every other term, whole words and stray bits; bits beyond a segment's length are set and must be ignored."""
    n0, n1, n2 = 5000, 3000, 1001
    sk0 = [0x55555555] * ((n0 + 31) // 32)
    sk1 = [0xFFFFFFFF if w % 3 == 0 else 0x00010001 for w in range((n1 + 31) // 32)]
    sk2 = [0] * ((n2 + 31) // 32)
    sk2[-1] = 0xFFFFFFFE                   # element 1000 is live, the 31 bits past the end are not elements
    segments = [seg("G", 0, n0, 0, skip=sk0), seg("H", 0, n1, 0, skip=sk1), seg("G", 8000, n2, 1, skip=sk2)]
    S = rand_scalars(n0 + n1 + n2, 25)
    S[1:n0:2] = limbs(777)                 # live: equal; skipped: their values must not count
    ev = run(ctx, 2, segments, S, table)
    assert 0 < ev["skipped"] < n0 + n1


# ---------------------------------------------------------------------------------------------------- windows at their extremes
def extreme_scalar(off, want):
    """The scalar below l whose digit in window j < W-1 is want(j, wd) (-2^(wd-1) or 2^(wd-1) - 1): the top window takes what keeps it below l."""
    W = len(off) - 1
    X = sum((want(j, off[j + 1] - off[j]) + (1 << (off[j + 1] - off[j] - 1))) << off[j] for j in range(W - 1))
    low_bias = sum(1 << (off[j + 1] - 1) for j in range(W - 1))
    return (X - low_bias) % (1 << off[W - 1])


@pytest.mark.parametrize("cmin", [2, 11, 16])
def test_windows_at_their_extremes(make_ctx, table, cmin):
    c = make_ctx(BPG_MSM_CMIN=cmin, BPG_MSM_CMAX=16)
    n = 40 if cmin == 2 else 6000                  # a floor: 2-bit windows need a sum of at most 2^6 terms
    segments = [seg("G", 3, n // 2, 0), seg("H", 3, n // 2, 0)]
    ev0 = probe(c, segments)
    off = ev0["off"]
    assert max(np.diff(off)) == cmin
    lo = lambda j, wd: -(1 << (wd - 1))
    hi = lambda j, wd: (1 << (wd - 1)) - 1
    pats = [lo, hi, lambda j, wd: (lo, hi)[j & 1](j, wd), lambda j, wd: (hi, lo)[j & 1](j, wd)]
    vals = [extreme_scalar(off, p) for p in pats]
    for v, p in zip(vals, pats):
        assert v < L
        d = digits_of(v, off)
        assert all(d[j] == p(j, off[j + 1] - off[j]) for j in range(len(off) - 2))
    S = rand_scalars(n, 31 + cmin)
    q = n // len(vals)
    for k, v in enumerate(vals):
        S[k * q:(k + 1) * q:2] = limbs(v)
    ev = run(c, 1, segments, S, table)
    assert ev["off"] == off


# ---------------------------------------------------------------------------------------------------- a segment beyond 2^20 elements
def test_segment_of_2_21_elements(make_ctx):
    """The entry index then needs 21 bits: fb (and with it the coarse bin) shrinks so that 27 - fb bits hold it."""
    n = 1 << 21
    c = make_ctx(cap=n)
    G, H = c.gens_export(0, n)
    tab = np.stack([np.frombuffer(G, np.uint8).reshape(n, 32), np.frombuffer(H, np.uint8).reshape(n, 32)])
    segments = [seg("G", 0, n, 0)]
    S = np.zeros((n, 8), np.uint32)
    rng = np.random.default_rng(41)
    idx = np.unique(np.concatenate([np.arange(0, n, 97), np.arange(n - 3000, n), np.arange((1 << 20) - 500, (1 << 20) + 500),
                                    rng.integers(0, n, 20000)]))
    S[idx] = rand_scalars(idx.size, 42)
    ev = run(c, 1, segments, S, tab)
    assert ev["fb"] < 7 and 27 - ev["fb"] >= 21


# ---------------------------------------------------------------------------------------------------- refused arguments
def test_refused_arguments_and_recovery(ctx, table):
    good = [seg("G", 0, 100, 0), seg("H", 0, 100, 1)]
    S = rand_scalars(200, 51)
    sb = S.tobytes()
    bad = [
        (0, good, sb), (5, good, sb),                                                  # nmsm out of range
        (2, [seg("G", 0, 1, 0)] * 17, bytes(32 * 17)),                                 # 17 segments
        (2, [seg("G", 0, 100, 1), seg("H", 0, 100, 0)], sb),                           # results not ascending
        (2, [seg("G", 0, 100, 0), seg("H", 0, 100, 2)], sb),                           # result index beyond nmsm
        (2, [seg(2, 0, 100, 0), seg("H", 0, 100, 1)], sb),                             # no such table
        (1, [seg("G", CAP - 99, 100, 0), seg("H", 0, 100, 0)], sb),                    # one past the table
        (1, [seg("G", CAP, 1, 0)], bytes(32)),                                          # first beyond the table
        (1, [seg("G", 0, CAP // 2 + 1, 0, lgblk=0)], bytes(32 * (CAP // 2 + 1))),       # strided: the last point is CAP
        (1, [seg("G", 1 << 11, CAP // 2, 0, lgblk=10)], bytes(32 * (CAP // 2))),        # strided from the third block: the last point is CAP + 1023
        (1, [seg("G", 0, 100, 0, lgblk=32), seg("H", 0, 100, 0)], sb),                # lgblk beyond 31
        (1, good[:1] + [seg("H", 0, 100, 0)], sc(0) * 199 + L.to_bytes(32, "little")),   # l itself
        (1, good[:1] + [seg("H", 0, 100, 0)], b"\xff" * 32 + sc(1) * 199),               # 2^256 - 1
    ]
    for k, (nmsm, segments, scal) in enumerate(bad):
        with pytest.raises(bpg.BpgError) as e:
            ctx.test_msm(nmsm, segments, scal)
        assert e.value.status == 4, k
    # the edges themselves are accepted, and the context still computes
    run(ctx, 1, [seg("G", CAP - 100, 100, 0), seg("H", 0, 100, 0)], S, table)
    S2 = np.zeros((CAP // 2, 8), np.uint32)
    S2[:300], S2[-300:] = rand_scalars(300, 52), rand_scalars(300, 53)
    run(ctx, 1, [seg("H", 1, CAP // 2, 0, lgblk=0)], S2, table)                        # the last point is CAP - 1
    run(ctx, 1, [seg("G", 1 << 10, CAP // 2, 0, lgblk=10)], S2, table)                 # ... here too
    run(ctx, 2, good, S, table)
