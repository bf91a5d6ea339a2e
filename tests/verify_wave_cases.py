"""Lockstep verification (bpg_r1cs_verify_resident_batch, csrc/hip/k_vwave.cuh): the items, the chosen challenge sets and a Python big-integer model of
the wave kernels - a plain helper module (not a conftest) shared by tests/test_verify_wave_host.py and tests/test_verify_wave_gpu.py.

The model restates what one call computes between the challenge records and the one MSM, in integers mod l and nothing of the package's arithmetic:
per item the s vector, g_i and h_i with the padding rule (lanes i >= n carry no weights and the factor u), w_c (over the rows the item's constants
stand in) and delta; then the rho-weighted sums over the items.  The weights and delta are shape_cases.model / shape_cases.delta, which
test_shape_cases_host.py ties to oracle proofs.

A challenge record is the dict {yinv, z, x, u, a, b, rho, uk, ukinv}; record_bytes() lays it out as the hook takes it."""
import hashlib

import shape_cases as SC
import script_cases as S
import template_inputs_cases as TI          # noqa: F401  (the circuits with a public side; the GPU test builds its items from them)
import verify_cases as VC

L = S.L
SET_NAMES = ("hashed", "edges", "zero")
K_MODEL = 3


def le(x):
    return int(x).to_bytes(32, "little")


def filler(tag, k=0):
    x = int.from_bytes(hashlib.shake_256(b"verify-wave %s %d" % (tag, k)).digest(64), "little") % L
    assert x
    return x


# ------------------------------------------------------------------------------------------------ challenge records
def hashed_record(lgN, tag, k):
    r = {name: filler(tag + b" " + name.encode(), k) for name in ("yinv", "z", "x", "u", "a", "b", "rho")}
    r["uk"] = [filler(tag + b" u%d" % j, k) for j in range(lgN)]
    r["ukinv"] = [S.inv(u) for u in r["uk"]]
    return r


def _with(rec, **changes):
    out = dict(rec)
    out.update(changes)
    if "uk" in changes:
        out["ukinv"] = [S.inv(u) for u in out["uk"]]
    return out


def challenge_set(name, lgN, K, tag=b""):
    """K records of the named set.  hashed: every entry a hashed non-zero scalar.  edges: y^-1 = 1, z = 1, z = 0, x = l - 1, rho = 1, rho = l - 1 and a
    self-inverse u_k = l - 1, spread over the items in a cycle of three.  zero: rho = 0, a = b = 0, and both, in a cycle of three."""
    assert name in SET_NAMES
    out = []
    for k in range(K):
        r = hashed_record(lgN, tag + name.encode(), k)
        if name == "edges":
            if k % 3 == 0:
                r = _with(r, yinv=1, z=1, x=L - 1, rho=1, uk=([L - 1] + r["uk"][1:])[:lgN])
            elif k % 3 == 1:
                r = _with(r, z=0, rho=L - 1, uk=[L - 1] * lgN)
            else:
                r = _with(r, yinv=1, x=L - 1, rho=L - 1, uk=r["uk"][:-1] + [L - 1] if lgN else [])
        elif name == "zero":
            r = _with(r, **({"rho": 0} if k % 3 == 0 else {"a": 0, "b": 0} if k % 3 == 1 else {"rho": 0, "a": 0, "b": 0}))
        out.append(r)
    return out


def record_bytes(r):
    return [le(r[k]) for k in ("yinv", "z", "x", "u", "a", "b", "rho")] + [le(u) for u in r["uk"]] + [le(u) for u in r["ukinv"]]


# ------------------------------------------------------------------------------------------------ the model
def s_vector(r, N):
    lgN = len(r["uk"])
    assert 1 << lgN == N
    out = []
    for i in range(N):
        acc = 1
        for k in range(lgN):
            acc = acc * (r["uk"][k] if (i >> (lgN - 1 - k)) & 1 else r["ukinv"][k]) % L
        out.append(acc)
    return out


def item(circ, r):
    """(g, h, slot) of one item, unweighted by rho: g_i = x y^-i w_R,i - a s_i, h_i = y^-i (x w_L,i + w_O,i - b s_{N-1-i}) - 1 on the lanes i < n; on the
    padding lanes the weights are absent and both carry the factor u.  slot = [w_V (m) | w_c | delta]"""
    n, N = circ.n, circ.N
    wL, wR, wO, wV, wc = SC.model(circ, r["z"])
    s = s_vector(r, N)
    g, h, yi = [], [], 1
    for i in range(N):
        real = i < n
        gi = ((r["x"] * yi * wR[i] if real else 0) - r["a"] * s[i]) % L
        t = ((r["x"] * wL[i] + wO[i] if real else 0) - r["b"] * s[N - 1 - i]) % L
        hi = (yi * t - 1) % L
        if not real:
            gi, hi = gi * r["u"] % L, hi * r["u"] % L
        g.append(gi); h.append(hi)
        yi = yi * r["yinv"] % L
    return g, h, list(wV) + [wc, SC.delta(circ, S.inv(r["yinv"]), r["z"])]


def wave(circs, records):
    """the accumulators and the slots of a call: circs[k] is the circuit item k is judged on (the same rows for all, unless items bring constants)"""
    N = circs[0].N
    g, h, slots = [0] * N, [0] * N, []
    for circ, r in zip(circs, records):
        gk, hk, slot = item(circ, r)
        for i in range(N):
            g[i] = (g[i] + r["rho"] * gk[i]) % L
            h[i] = (h[i] + r["rho"] * hk[i]) % L
        slots.append(slot)
    return g, h, slots


def wave_bytes(circs, records):
    g, h, slots = wave(circs, records)
    return [le(x) for x in g], [le(x) for x in h], [[le(x) for x in s] for s in slots]


# ------------------------------------------------------------------------------------------------ the circuits
def model_circuits(with_n0=False):
    """[(name, verify_cases.Circuit)] the kernels are held against the model on: the lockstep cases of shape_cases and the circuits of verify_cases - with_n0:
    all six; else the five with multipliers (the n = 0 circuit has no wave: the call serves it item by item)"""
    out = [(c.name, c.circuit) for c in SC.lockstep_cases()]
    out += [("verify/" + c.name, c) for c in VC.corpus()[0].values() if with_n0 or c.n]
    return out


def rows_of(inst):
    """the rows of a bpg.FlatInstance as [[(variable, coefficient)]]"""
    coef = [int.from_bytes(inst.coef[32 * k:32 * k + 32], "little") for k in range(inst.ncoef)]
    return [[(int(inst.term_var[k]), coef[int(inst.term_coef[k])]) for k in range(int(inst.row_ptr[j]), int(inst.row_ptr[j + 1]))] for j in range(inst.q)]


class Rows:
    """what the model reads of a circuit, for statements that exist as instances only (a template with the item's constants baked in)"""
    def __init__(self, inst):
        self.n, self.m, self.rows = inst.n, inst.m, rows_of(inst)
        self.N = 1
        while self.N < self.n:
            self.N *= 2
