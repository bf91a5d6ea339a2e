"""The seven generator-fold kernels of the inner-product argument (hip/k_ipa.cuh) at chosen scalars, edge by edge, through bpg_test_fold - the launch path
of the prover (kernel choice, recoding, upload, launch, normalisation) on the context's own generator tables.

Inside a proof the fold scalars are products of Fiat-Shamir challenges: uniformly random 252-bit numbers that no test can choose.  Here every case of the
catalogue (tests/fold_cases.py: zero, one and two, l - 1, 2^252 and its neighbours, the densest digit strings, every multiple and sign of the tables,
digits on both sides of the word edges, scalar parts of zero and of 2^L - 1, terms of very different length in one launch, edges in the class of the
padding generators) goes through one call, and the test compares
  - all 2 * Mr folded points, byte for byte, with out[i] = tab[i] + sum_t s_t tab[i + t*Mr] as the CPU oracle's multiscalar sum gives it, and
  - the evidence of the launch (kernel, top, nsteps, tail, wnaf, parts, part_bits) with the integer model's prediction.
No case is skipped or sampled; the parametrisation is by kernel and shape with the cases looped inside.  The shapes are the smallest at which each kernel
can still go wrong: whole waves and blocks on each side (Mr = 64; 256 for the one-lane step kernel), fewer outputs than a wave (Mr = 1, 16: idle lanes
shadow the last output, G and H meet in one wave and take the per-lane path), and a first group with its class boundary nowhere, everywhere, inside a wave
and on a wave's edge."""
import ctypes as C
import hashlib

import pytest

import bulletproofs_gadgets_amd as bpg
import fold_cases as F
import oracle_lib as O
from bulletproofs_gadgets_amd import workloads

pytestmark = pytest.mark.gpu

CAP = 2048
WNAF, QUADW, QUAD, SPLIT, REGW, REG, MEM = F.KERNELS
PADDING_NS = {256: (256, 129, 213, 192)}          # g_M -> no padding, all there is, a class boundary inside a wave, one on a multiple of 64


@pytest.fixture(scope="module")
def ctx():
    c = bpg.Context(0)
    c.gens_ensure(CAP)
    yield c
    c.close()


@pytest.fixture
def make_ctx(monkeypatch):
    """A fresh context with the given environment knobs (they are read once, at context creation)."""
    made = []

    def make(cap, **env):
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


_references = {}


def reference(gens, case, Mr, rounds, first, n):
    """F.reference, computed once per (tables, scalars, shape) and shared by every kernel and context that folds the same."""
    g_M = Mr << rounds
    G, H = gens[0][:32 * g_M], gens[1][:32 * g_M]
    key = (hashlib.sha256(G + H).digest(), case[1], case[2], case[3] if first else 1, Mr, rounds, first, n if first else 0)
    if key not in _references:
        _references[key] = tuple(F.reference(G, H, case, Mr, rounds, first, n))
    return _references[key]


EVIDENCE = ("top", "nsteps", "tail", "wnaf", "parts", "part_bits")          # what a launch reports beside its kernel and shape, where the model predicts it


def run_cases(c, gens, kernel, lgMr, rounds, first, n, cases, predict):
    """One bpg_test_fold call per case, checked: every folded point against the oracle, the evidence against the model."""
    Mr, nterms = 1 << lgMr, (1 << rounds) - 1
    assert cases and all(len(case[1]) == nterms for case in cases)
    for case in cases:
        got, ev = c.test_fold(kernel, lgMr, rounds, first, n, [F.sc(s) for s in case[1]], [F.sc(s) for s in case[2]], F.sc(case[3]))
        want = reference(gens, case, Mr, rounds, first, n)
        wrong = [i for i in range(2 * Mr) if got[i] != want[i]]
        assert not wrong, "%s, case %r: %d of %d outputs differ, first at %d (%s side)" % (kernel, case[0], len(wrong), 2 * Mr, wrong[0], "GH"[wrong[0] >= Mr])
        expect = dict({k: v for k, v in predict(case).items() if k in EVIDENCE}, kernel=kernel, Mr=Mr, nterms=nterms, first=first, n=n)
        assert ev == expect, "%s, case %r" % (kernel, case[0])


def bitmap_evidence(first):
    return lambda case: F.predict_bitmap(case, first)


steps_evidence = F.predict_steps


@pytest.fixture(scope="module")
def gens(ctx):
    return ctx.gens_export(0, CAP)


# ---------------------------------------------------------------------------------------------------- plain NAF bitmaps: k_fold_points, _reg<NT>, _quad, _split
BITMAP_ROUNDS = [(REG, r) for r in (1, 2, 3, 4)] + [(QUAD, r) for r in (1, 2, 3)] + [(SPLIT, r) for r in (2, 3, 4)] + [(MEM, r) for r in (1, 3, 5)]


@pytest.mark.parametrize("lgMr", [6, 0, 4])
@pytest.mark.parametrize("kernel,rounds", BITMAP_ROUNDS)
def test_bitmap_kernels_after_the_first_group(ctx, gens, kernel, rounds, lgMr):
    """Mr = 64: one whole wave per side (four with four lanes per output), every wave uniform.  Mr = 1, 16: fewer outputs than a wave."""
    Mr, nterms = 1 << lgMr, (1 << rounds) - 1
    lanes = 4 if kernel == QUAD else 1
    uniform, mixed = F.wave_classes(Mr, nterms, 0, 0, lanes)
    assert mixed == 0 if Mr % (64 // lanes) == 0 else uniform == 0             # whole waves on each side, or G and H in one wave
    run_cases(ctx, gens, kernel, lgMr, rounds, 0, 0, F.bitmap_cases(nterms, 0), bitmap_evidence(0))


@pytest.mark.parametrize("n", PADDING_NS[256])
@pytest.mark.parametrize("kernel", [REG, QUAD, SPLIT, MEM])
def test_bitmap_kernels_in_a_first_group(ctx, gens, kernel, n):
    """Mr = 64, two rounds: the lanes with i + t*Mr >= n take s_t * u_ch.  n = 256 and 192 leave every wave uniform, 129 and 213 put the class boundary
    inside the waves (one lane per output: both waves; four lanes per output: one wave per side)."""
    kinds = [F.wave_classes(64, 3, m, 1) for m in PADDING_NS[256]]
    assert kinds == [(2, 0), (0, 2), (0, 2), (2, 0)]
    run_cases(ctx, gens, kernel, 6, 2, 1, n, F.bitmap_cases(3, 1), bitmap_evidence(1))


# ---------------------------------------------------------------------------------------------------- width-4 step lists: k_fold_points_quadw, _regw
@pytest.mark.parametrize("kernel,lgMr,rounds", [(QUADW, 6, 1), (QUADW, 6, 2), (QUADW, 6, 3), (REGW, 8, 1), (REGW, 8, 3)])
def test_step_kernels(ctx, gens, kernel, lgMr, rounds):
    """A block of the step kernels lies in G or in H: Mr = 64 with four lanes per output, Mr = 256 with one."""
    run_cases(ctx, gens, kernel, lgMr, rounds, 0, 0, F.steps_cases((1 << rounds) - 1), steps_evidence)


# ---------------------------------------------------------------------------------------------------- width-w digits per part: k_fold_points_wnaf
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("w,parts", F.WNAF_PROFILES)
def test_wnaf_kernel(make_ctx, w, parts, first):
    """A fresh context of 256 generators per (width, parts): its tables of odd multiples are a few MB.  Mr = 32 with three rounds (G and H meet in one wave:
    per-lane digits) and Mr = 64 with two (one wave per side: the wave's digits, scalar branches), a first group with each of the four n.  The evidence
    shows the width and the parts asked for: a context that settled on a smaller profile fails here instead of passing on other tables."""
    c = make_ctx(256, BPG_FOLD_WNAF=w, BPG_FOLD_PARTS=parts)
    g = c.gens_export(0, 256)
    for lgMr, rounds in ((5, 3), (6, 2)):
        nterms = (1 << rounds) - 1
        cases = F.wnaf_cases(w, parts, nterms, first)
        for n in (PADDING_NS[256] if first else (0,)):
            run_cases(c, g, WNAF, lgMr, rounds, first, n, cases, lambda case: F.predict_wnaf(case, first, w, parts))


# ---------------------------------------------------------------------------------------------------- the chooser's kernel
def chosen(Mr, nterms, first, wnaf=5, split_max=65536, quad=True, quad_w=True, reg_w=True, shared=False, original=True, tables=True):
    """The seven rules of choose_fold as host/fold_plan.hpp documents them: the first that holds decides."""
    outputs = 2 * Mr
    regs = nterms in (1, 3, 7, 15)
    small = outputs <= (0 if regs and shared else split_max)
    if wnaf >= 3 and original and outputs > split_max and tables:
        return WNAF
    if small and 1 <= nterms <= 7 and quad and quad_w and not first and Mr % 64 == 0:
        return QUADW
    if small and 1 <= nterms <= 7 and quad:
        return QUAD
    if small and 3 <= nterms <= 15:
        return SPLIT
    if not small and reg_w and not first and 1 <= nterms <= 7 and Mr % 256 == 0:
        return REGW
    return REG if regs else MEM


@pytest.mark.parametrize("env,knobs", [({}, {}), ({"BPG_FOLD_QUAD_W": "0"}, {"quad_w": False}), ({"BPG_FOLD_ADAPT": "2"}, {"shared": True}),
                                        ({"BPG_FOLD_ADAPT": "2", "BPG_FOLD_REG_W": "0"}, {"shared": True, "reg_w": False}),
                                        ({"BPG_FOLD_QUAD": "0"}, {"quad": False}), ({"BPG_FOLD_SPLIT": "64"}, {"split_max": 64})])
def test_the_hook_runs_the_kernel_the_chooser_names(make_ctx, env, knobs):
    """kernel = -1 under the knob settings of test_small_folds_on_multiples_the_kernel_makes_itself (and two more: no quads; a split bound of 64 outputs, above
    which the original generators fold on their odd multiples): the hook reports what the seven rules give for the shape, and folds right."""
    c = make_ctx(CAP, BPG_TT_LG=0, **env)
    g = c.gens_export(0, CAP)
    seen = set()
    for lgMr, rounds, first in ((6, 1, 0), (6, 2, 0), (6, 3, 0), (6, 4, 0), (6, 5, 0), (8, 3, 0), (8, 2, 0), (4, 3, 0), (4, 2, 0), (6, 2, 1), (4, 3, 1), (6, 4, 1)):
        Mr, nterms = 1 << lgMr, (1 << rounds) - 1
        want = chosen(Mr, nterms, first, **knobs)
        seen.add(want)
        case = ("chooser", tuple(F.ordinary(20 + t) for t in range(nterms)), tuple(F.ordinary(60 + t) for t in range(nterms)), F.ordinary(99))
        n = (Mr << rounds) - Mr // 2 - 5 if first else 0
        got, ev = c.test_fold(-1, lgMr, rounds, first, n, [F.sc(s) for s in case[1]], [F.sc(s) for s in case[2]], F.sc(case[3]))
        assert ev["kernel"] == want, (env, Mr, nterms, first)
        assert tuple(got) == reference(g, case, Mr, rounds, first, n), (env, Mr, nterms, first)
    assert len(seen) >= 2, seen


# ---------------------------------------------------------------------------------------------------- refusals, and the borrowed buffers handed back
def test_refusals_leave_the_context_usable(make_ctx):
    """Each refused argument is INVALID_ARGUMENT (4) before any launch; a good call afterwards still matches the reference, and a proof on the same context -
    which takes scratch_ext, the digit and step buffers and the arena back from the hook - is the oracle's, byte for byte."""
    c = make_ctx(CAP, BPG_FOLD_WNAF=0)
    g = c.gens_export(0, CAP)
    one, big = F.sc(1), (F.L).to_bytes(32, "little")

    def refused(kernel=MEM, lgMr=6, rounds=2, first=0, n=0, sG="ok", sH="ok", u=one):
        nterms = (1 << min(max(rounds, 1), 5)) - 1
        sG = [one] * nterms if sG == "ok" else sG
        sH = [one] * nterms if sH == "ok" else sH
        with pytest.raises(bpg.BpgError) as e:
            c.test_fold(kernel, lgMr, rounds, first, n, sG, sH, u)
        assert e.value.status == 4, e.value

    refused(sG=None); refused(sH=None); refused(u=None)                                     # a NULL pointer
    refused(sG=[one, big, one]); refused(sH=[one, one, big]); refused(u=big)                # a non-canonical scalar
    refused(sG=[one, (2**256 - 1).to_bytes(32, "little"), one])
    refused(rounds=0); refused(rounds=6)                                                    # rounds outside 1..5
    refused(lgMr=10, rounds=2); refused(lgMr=11, rounds=1); refused(lgMr=31, rounds=1); refused(lgMr=40, rounds=1)      # g_M beyond the capacity
    refused(first=1, n=128); refused(first=1, n=257); refused(first=1, n=0); refused(first=2, n=200)                     # n out of range
    refused(kernel=-2); refused(kernel=7)
    refused(kernel=QUADW, first=1, n=256); refused(kernel=QUADW, lgMr=5); refused(kernel=QUADW, rounds=4)               # a forced kernel outside its conditions
    refused(kernel=REGW, lgMr=8, rounds=2, first=1, n=1024); refused(kernel=REGW, lgMr=6); refused(kernel=REGW, lgMr=7, rounds=4)
    refused(kernel=QUAD, rounds=4); refused(kernel=SPLIT, rounds=1); refused(kernel=SPLIT, rounds=5); refused(kernel=REG, rounds=5)
    refused(kernel=WNAF)                                                                    # BPG_FOLD_WNAF = 0: the chooser never names it
    out, ev = C.create_string_buffer(32 * 128), C.create_string_buffer(1024)                # no context: as on a machine without a GPU
    assert bpg.lib().bpg_test_fold(None, C.c_int32(6), C.c_uint32(6), C.c_uint32(2), C.c_uint32(0), C.c_uint64(0), one * 3, one * 3, one, out, ev, C.c_uint64(1024)) == 7
    for kernel, lgMr, rounds, first, n, cases, predict in ((QUADW, 6, 3, 0, 0, F.steps_cases(7)[-4:], steps_evidence), (REGW, 8, 3, 0, 0, F.steps_cases(7)[-2:], steps_evidence),
                                                           (SPLIT, 6, 2, 1, 213, F.bitmap_cases(3, 1)[-3:], bitmap_evidence(1))):
        run_cases(c, g, kernel, lgMr, rounds, first, n, cases, predict)
    a = workloads.mimc_preimage(c, nbytes=100, seed=32, label=b"MiMCHash")
    inst = a.prover.instance()
    c.gens_ensure(a.gens_capacity)
    res = c.upload(inst)
    seed = bytes(range(32))
    proof, st_after = res.prove(a.transcript.state, inst.v_blinding, seed, 0)
    oc = O.FlatCircuit(inst.n, inst.m, inst.aL, inst.aR, inst.aO, inst.row_ptr, inst.term_var, inst.term_coef, inst.coef)
    rc, want, st_want = O.prove(O.Gens(a.gens_capacity), a.transcript.state, oc, inst.v_blinding, seed, O.FLAG_FAST_MSM)
    assert rc == 0 and proof == want and st_after == st_want
    res.free()
    run_cases(c, c.gens_export(0, CAP), QUAD, 6, 3, 0, 0, F.bitmap_cases(7, 0)[:3], bitmap_evidence(0))       # and the hook after the proof
