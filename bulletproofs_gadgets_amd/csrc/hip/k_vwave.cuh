// lockstep verification: K proofs of ONE resident circuit per launch (Engine::verify_resident_batch; include/bpg.h bpg_r1cs_verify_resident_batch) - part of
// kernels.cuh (included from there, in this order; see its header for the kernel map and the data layout).  Launch shapes: host/verify_wave_plan.hpp.
// Every vector of a wave is item-major, vec[k * len + i] with a 64-bit k * len; everything is canonical Montgomery form, as in k_verify.cuh.
// The per-lane arithmetic sits in BPG_HD functions, which also compile for the host alone (tests/hostcheck/verify_wave_lanes.cpp).
#pragma once
#include <cstddef>
#include "k_witness.cuh"      // witness_input_slot: what a derived coefficient slot holds

namespace bpg {

// One record per item, uploaded once per call: VW_CH_FIXED scalars, then u_k (lg N of them), then u_k^-1.  u_ch is the replay's `u`, the factor of the
// padding generators; rho the item's weight in the batch.
enum { VW_YINV = 0, VW_Z = 1, VW_X = 2, VW_UCH = 3, VW_A = 4, VW_B = 5, VW_RHO = 6, VW_CH_FIXED = 7 };
// what an item brings of its own (flags[k]): parameter values, public inputs
enum { VW_HAS_PARAMS = 1u, VW_HAS_INPUTS = 2u };

// base^t and base^T (T = 2^lgT): where thread t of a power table starts and what it multiplies by, as k_exp_table
BPG_HD void vw_pow_start(const scm &base, uint32_t t, uint32_t lgT, scm &cur, scm &step) {
    cur = SC_R1(); step = base;
    for (uint32_t b = 0; b < lgT; b++) {
        if ((t >> b) & 1u) cur = sc_mont_mul(cur, step);
        step = sc_mont_mul(step, step);
    }
}
// s_i = prod_k (bit_{lgN-1-k}(i) ? u_k : u_k^-1) and s_{N-1-i}, whose every factor is the other one of the pair: 2 lg N products, no s vector in memory
BPG_HD void vw_s_pair(const scm *u, const scm *uinv, uint32_t lgN, uint32_t i, scm &s_i, scm &s_rev) {
    s_i = SC_R1(); s_rev = SC_R1();
    for (uint32_t k = 0; k < lgN; k++) {
        const bool bit = (i >> (lgN - 1 - k)) & 1u;
        s_i = sc_mont_mul(s_i, bit ? u[k] : uinv[k]);
        s_rev = sc_mont_mul(s_rev, bit ? uinv[k] : u[k]);
    }
}
// rho-weighted g_i, h_i of one item by the expressions of k_verify_scalars_acc: real = i < n, the - 1, rho * u_ch on the padding lanes.
// ch: the item's record; wL, wR, wO: its weights at i (read only when real)
BPG_HD void vw_weighted_gh(const scm *ch, bool real, const scm &yi, const scm &wL, const scm &wR, const scm &wO, const scm &s_i, const scm &s_rev, scm &g, scm &h) {
    const scm x = ch[VW_X], rho = ch[VW_RHO];
    const scm ywr = real ? sc_mont_mul(yi, wR) : sc_zero();
    const scm gi = sc_sub(sc_mont_mul(x, ywr), sc_mont_mul(ch[VW_A], s_i));
    scm t = sc_neg(sc_mont_mul(ch[VW_B], s_rev));
    if (real) t = sc_add(t, sc_add(sc_mont_mul(x, wL), wO));
    const scm hi = sc_sub(sc_mont_mul(yi, t), SC_R1());
    const scm wgt = real ? rho : sc_mont_mul(rho, ch[VW_UCH]);
    g = sc_mont_mul(wgt, gi); h = sc_mont_mul(wgt, hi);
}
// entry j of an item's coefficient tail [parameter slots (n_params) | derived slots (n_slots)]: the item's own value where it brings one, else the
// circuit's standing one.  raw: the item's n_params + n_in values as bytes (any 256-bit value, reduced as assign reduces them); slots: (input,
// coefficient index) per derived slot, the index below the tail: the shared table
BPG_HD scm vw_tail_entry(uint32_t j, uint32_t flags, uint32_t n_params, const uint32_t *raw, const uint32_t *slots, const scm *coef, const scm *standing) {
    if (j < n_params) return (flags & VW_HAS_PARAMS) ? sc_from_words(raw + 8 * (size_t)j) : standing[j];
    if (!(flags & VW_HAS_INPUTS)) return standing[j];
    const uint32_t *sl = slots + 2 * (size_t)(j - n_params);              // host/template.hpp InputSlot: (p, ci)
    return witness_input_slot(coef[sl[1]], sc_from_words(raw + 8 * ((size_t)n_params + sl[0])));
}

#if defined(__HIPCC__)
// y^-i (i < N) and z^j (j < nz) of every item of a wave: blockIdx.z = item, blockIdx.y = table, thread t walks t, t + T, .. as k_exp_table does
__global__ void __launch_bounds__(256) k_vw_exp(const scm *__restrict__ ch, uint32_t ch_len, scm *__restrict__ ypow, uint32_t N, uint32_t lgTy,
                                                scm *__restrict__ zpow, uint32_t nz, uint32_t lgTz) {
    const uint64_t k = blockIdx.z;
    const bool isz = blockIdx.y != 0;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lgT = isz ? lgTz : lgTy, T = 1u << lgT, count = isz ? nz : N;
    if (t >= T) return;
    scm *__restrict__ out = (isz ? zpow : ypow) + k * count;
    scm cur, step;
    vw_pow_start(ch[k * ch_len + (isz ? VW_Z : VW_YINV)], t, lgT, cur, step);
    for (uint32_t i = t; i < count; i += T) { out[i] = cur; cur = sc_mont_mul(cur, step); }
}
// every item's coefficient tail: a lane per (item, entry)
__global__ void __launch_bounds__(256) k_vw_tails(const uint32_t *__restrict__ flags, const uint32_t *__restrict__ raw, uint32_t n_raw, const uint32_t *__restrict__ slots,
                                                  const scm *__restrict__ coef, const scm *__restrict__ standing, uint32_t n_params, uint32_t n_tail, uint64_t total,
                                                  scm *__restrict__ tails) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t k = t / n_tail;
    const uint32_t j = (uint32_t)(t - k * n_tail);
    tails[t] = vw_tail_entry(j, flags[k], n_params, raw + 8 * k * n_raw, slots, coef, standing);
}
// flattened_constraints(z_k) of every item: a lane per (item, column c < ncols = 3 n + m), columns >= first_neg_col negated, exactly as k_flatten.  Variable
// columns of a template WITHOUT gates never name a parameter or derived slot (host/template.hpp makes those constant terms): tails == nullptr, the shared
// table throughout.  With gates a column entry may sit on a derived slot (coefficient * input): an index at or above tail_first then comes from the item's
// tail, as in k_vw_small.  The engine passes tails only for a circuit with gates whose items bring constants
__global__ void __launch_bounds__(256) k_vw_flatten(const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row, const uint32_t *__restrict__ ent_coef,
                                                    const scm *__restrict__ coef, const scm *__restrict__ tails, uint32_t tail_first, uint32_t n_tail,
                                                    const scm *__restrict__ zpow, uint32_t nz, scm *__restrict__ w, uint32_t ncols,
                                                    uint32_t first_neg_col, uint64_t total) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t k = t / ncols;
    const uint32_t c = (uint32_t)(t - k * ncols);
    const scm *__restrict__ zp = zpow + k * nz;
    const scm *__restrict__ tk = tails ? tails + k * n_tail : nullptr;
    scm acc = sc_zero();
    for (uint64_t e = col_ptr[c]; e < col_ptr[c + 1]; e++) {
        const uint32_t ci = ent_coef[e];
        const scm cf = (tk && ci >= tail_first) ? tk[ci - tail_first] : coef[ci];
        acc = sc_add(acc, sc_mont_mul(cf, zp[ent_row[e] + 1]));
    }
    w[t] = (c >= first_neg_col) ? sc_neg(acc) : acc;
}
// a block per item: w_c = - sum over the constant column [e0, e1) of coef * z^(row + 1) - a coefficient below tail_first from the shared table, one at or
// above it from the item's tail (tails == nullptr: no item brings constants, the shared table throughout) - and delta = sum_{i<n} y^-i wR_i wL_i, straight into
// the item's slot [w_V (m) | w_c | delta], the w_V part copied from columns 3 n .. 3 n + m - 1
__global__ void __launch_bounds__(256) k_vw_small(const uint32_t *__restrict__ ent_row, const uint32_t *__restrict__ ent_coef, const scm *__restrict__ coef,
                                                  const scm *__restrict__ tails, uint32_t tail_first, uint32_t n_tail, uint64_t e0, uint64_t e1,
                                                  const scm *__restrict__ zpow, uint32_t nz, const scm *__restrict__ ypow, const scm *__restrict__ w, uint32_t n, uint32_t m,
                                                  uint32_t N, scm *__restrict__ small) {
    __shared__ scm lds[256];
    const uint64_t k = blockIdx.x;
    const scm *__restrict__ zp = zpow + k * nz, *__restrict__ yp = ypow + k * N, *__restrict__ wk = w + k * (3 * (uint64_t)n + m);
    const scm *__restrict__ tk = tails ? tails + k * n_tail : nullptr;
    scm *__restrict__ sl = small + k * ((uint64_t)m + 2);
    scm acc = sc_zero();
    for (uint64_t e = e0 + threadIdx.x; e < e1; e += 256) {
        const uint32_t ci = ent_coef[e];
        const scm cf = (tk && ci >= tail_first) ? tk[ci - tail_first] : coef[ci];
        acc = sc_add(acc, sc_mont_mul(cf, zp[ent_row[e] + 1]));
    }
    scm r = block_sum_256(acc, lds);
    if (threadIdx.x == 0) sl[m] = sc_neg(r);
    scm delta = sc_zero();
    for (uint32_t i = threadIdx.x; i < n; i += 256) delta = sc_add(delta, sc_mont_mul(sc_mont_mul(yp[i], wk[n + i]), wk[i]));
    r = block_sum_256(delta, lds);
    if (threadIdx.x == 0) sl[m + 1] = r;
    for (uint32_t j = threadIdx.x; j < m; j += 256) sl[j] = wk[3 * (uint64_t)n + j];
}
// grid (cdiv(N, 256), chunks): lane i walks items [chunk * per_chunk, min(items, (chunk + 1) * per_chunk)) of the wave, sums their rho-weighted g_i and h_i in
// registers and writes part[chunk][0][i], part[chunk][1][i] once
__global__ void __launch_bounds__(256) k_vw_scalars(const scm *__restrict__ ch, uint32_t ch_len, const scm *__restrict__ w, const scm *__restrict__ ypow, uint32_t n, uint32_t m,
                                                    uint32_t N, uint32_t lgN, uint64_t items, uint64_t per_chunk, scm *__restrict__ part) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint64_t k0 = blockIdx.y * per_chunk, k1 = k0 + per_chunk < items ? k0 + per_chunk : items, ncols = 3 * (uint64_t)n + m;
    const bool real = i < n;
    scm gs = sc_zero(), hs = sc_zero();
    for (uint64_t k = k0; k < k1; k++) {
        const scm *__restrict__ c = ch + k * ch_len, *__restrict__ wk = w + k * ncols;
        scm s_i, s_rev, g, h;
        vw_s_pair(c + VW_CH_FIXED, c + VW_CH_FIXED + lgN, lgN, i, s_i, s_rev);
        const scm zero = sc_zero();
        vw_weighted_gh(c, real, ypow[k * N + i], real ? wk[i] : zero, real ? wk[n + i] : zero, real ? wk[2 * (uint64_t)n + i] : zero, s_i, s_rev, g, h);
        gs = sc_add(gs, g); hs = sc_add(hs, h);
    }
    scm *__restrict__ p = part + (uint64_t)blockIdx.y * 2 * N;
    p[i] = gs; p[(uint64_t)N + i] = hs;
}
// lane i adds the chunks' partial sums into the call's accumulators (zeroed once per call; later waves add to them)
__global__ void __launch_bounds__(256) k_vw_reduce(const scm *__restrict__ part, uint32_t chunks, uint32_t N, scm *__restrict__ g_acc, scm *__restrict__ h_acc) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    scm g = g_acc[i], h = h_acc[i];
    for (uint32_t c = 0; c < chunks; c++) {
        const scm *__restrict__ p = part + (uint64_t)c * 2 * N;
        g = sc_add(g, p[i]); h = sc_add(h, p[(uint64_t)N + i]);
    }
    g_acc[i] = g; h_acc[i] = h;
}
#endif

}  // namespace bpg
