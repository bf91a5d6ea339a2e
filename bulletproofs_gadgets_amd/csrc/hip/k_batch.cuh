// lockstep batch proving (Engine::prove_batch): the table-driven prove path of a circuit with N <= 2^tt_orig_lg, for K proofs of the same padded
// size N at once - part of kernels.cuh (included from there, in this order; see its header for the kernel map and the data layout).
// Layout of a wave: item k's vectors of length N live at [k*N, (k+1)*N) (a_L, a_R, a_O, s_L, s_R, y^i, y^-i, l, r, the flattened weights of each
// of the L, R, O column blocks); blockIdx.z (or .y) is the item.  The window tables are those of the original generators, built for M0T >= N
// generators (G at rows [0, M0T), H at [M0T, 2*M0T)); an item of N < M0T uses the first N rows of each half.  Per-item scalars sit in bsc[k * BSC + j].
// Same thread layouts and the same per-point arithmetic as the single-proof kernels of k_ipa.cuh, so every point and scalar is the same.
#pragma once

namespace bpg {

#define BSC 8                   // per-item device scalars: ib, ob, sb, x, u_ch, w, u, u^-1
#define BSC_X 3
#define BSC_UCH 4
#define BSC_W 5
#define BSC_U 6
#define BSC_UINV 7

// A_I, A_O, S of every item (k_tt_commit3 per item): blockIdx.y = class, blockIdx.z = item; partial[(item * 3 + class) * gridDim.x + block]
__global__ void __launch_bounds__(256) k_bt_commit3(const ge_pniels *__restrict__ table, uint32_t M0T, const scm *__restrict__ aL, const scm *__restrict__ aR,
                                                    const scm *__restrict__ aO, const scm *__restrict__ sL, const scm *__restrict__ sR,
                                                    const uint32_t *__restrict__ nk, uint32_t lgN, ge_ext *__restrict__ partial, uint32_t quad) {
    __shared__ ge_ext lds[256];
    const uint32_t cls = blockIdx.y, item = blockIdx.z, tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t N = 1u << lgN, e = tid >> 3, g = tid & 7u, n = nk[item];
    const size_t base = (size_t)item << lgN;
    ge_ext acc = ge_identity();
    const bool isH = e >= N;
    const uint32_t p = isH ? e - N : e;
    if (e < 2 * N && p < n && !(cls == 1 && isH)) {
        const size_t q = base + p;
        const scm s = cls == 0 ? (isH ? aR[q] : aL[q]) : (cls == 1 ? aO[q] : (isH ? sR[q] : sL[q]));
        uint32_t w[8]; tt_biased_words(w, s);
        const ge_pniels *tbl = table + ((size_t)(isH ? M0T : 0u) + p) * (TT_WINDOWS * TT_MULTS) + (size_t)g * 8 * TT_MULTS;
        const uint32_t word = w[g];
#pragma unroll 1
        for (uint32_t k = 0; k < 8; k++) {
            const int32_t d = (int32_t)((word >> (4 * k)) & 15u) - 8;
            if (d == 0) continue;
            const uint32_t neg = d < 0, mag = neg ? (uint32_t)(-d) : (uint32_t)d;
            acc = ge_add_pniels_signed(acc, tbl[k * TT_MULTS + mag - 1], neg);
        }
    }
    ge_block_sum_store(acc, lds, quad, partial + ((size_t)item * 3 + cls) * gridDim.x + blockIdx.x);
}
// block (class, item): out[item * 3 + class] = sum of its partials + bsc[item][class] * B_blinding (k_tt_commit3_finish per item)
__global__ void __launch_bounds__(256) k_bt_commit3_finish(const ge_ext *__restrict__ partial, uint32_t nblk, const scm *__restrict__ bsc,
                                                           const ge_pniels *__restrict__ tableX, ge_ext *__restrict__ out, uint32_t quad) {
    __shared__ ge_ext lds[256];
    const uint32_t cls = blockIdx.x, item = blockIdx.y;
    const ge_ext *part = partial + ((size_t)item * 3 + cls) * nblk;
    ge_ext acc = ge_identity();
    uint32_t s0 = threadIdx.x;
    if (s0 < nblk) { acc = part[s0]; s0 += 256; }
    for (; s0 < nblk; s0 += 256) acc = ge_add(acc, part[s0]);
    const uint32_t win = 255u - threadIdx.x;
    if (win < TT_WINDOWS) {
        uint32_t w[8]; tt_biased_words(w, bsc[(size_t)item * BSC + cls]);
        const int32_t d = (int32_t)((w[win >> 3] >> (4 * (win & 7u))) & 15u) - 8;
        if (d != 0) {
            const uint32_t neg = d < 0, mag = neg ? (uint32_t)(-d) : (uint32_t)d;
            const ge_pniels q = tableX[win * TT_MULTS + mag - 1];
            acc = threadIdx.x >= nblk ? ge_from_pniels_signed(q, neg) : ge_add_pniels_signed(acc, q, neg);
        }
    }
    ge_block_sum_store(acc, lds, quad, out + (size_t)item * 3 + cls);
}
// The Pedersen commitments of a wave's committed values (bpg_r1cs_prove_template_batch_commit): out[c] = compress(v[c] * B + r[c] * B_blinding) for the
// `count` = K m commitments of the wave, from the window tables k_pedersen reads.  v is the wave's device block of REDUCED values in Montgomery form
// (what the witness evaluation reads: B has order l, so the reduced value gives the same point), r the reduced blindings as plain little-endian
// words.  Both are below l < 2^253, so the digits come from the biased form (tt_biased_words: nibble - 8 in [-8, 7], no carry chain) instead of
// ped_digit's serial recoding - another signed representation of the same integer, and the encoding of a point does not depend on how it was summed.
// Layout: a block of four waves makes 4 * cpw commitments (cpw in 1..4).  Wave w makes commitments first + w * cpw + i one after the other (lane =
// window: the first table entry is taken as it is, the second added), the 64 partial sums meet in the wave's own LDS region as four lanes per point
// (three additions through LDS, four shuffle levels: seven quad_add of ~750 instructions where k_pedersen's binary tree does six ge_add of ~1,650 -
// that tree was measured here too and lost at every cpw) and the sum is parked in LDS.  The encodings, the longest chain by far
// (~250 dependent squarings each), are then made SIDE BY SIDE in the lanes of the block's first wave: 4 * cpw encodings for the instructions of
// one, where k_pedersen spends a wave per encoding.
// Precondition: count >= 1 (the caller launches nothing for a wave without commitments; count - 1 below would wrap).  The tail of the launch computes
// commitment count - 1 again in the lanes past the end (every lane reaches every barrier; at most 4 * cpw - 1 redundant sums) and keeps its stores.
__global__ void __launch_bounds__(256) k_bt_commit_v(const scm *__restrict__ v, const uint32_t *__restrict__ r, const ge_pniels *__restrict__ table /* [2][64][8] */,
                                                     uint8_t *__restrict__ out, uint32_t count, uint32_t cpw) {
    __shared__ ge_ext lds[256];
    __shared__ ge_ext sums[16];
    const uint32_t wv = threadIdx.x >> 6, win = threadIdx.x & 63u, per = 4u * cpw, first = blockIdx.x * per;
    ge_ext *L = lds + 64 * wv;
    for (uint32_t i = 0; i < cpw; i++) {
        const uint32_t c = min(first + wv * cpw + i, count - 1u);
        uint32_t vw[8], rw[8];
        tt_biased_words(vw, v[c]);
        {
            uint64_t carry = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) { const uint64_t t = (uint64_t)r[8 * (size_t)c + k] + 0x88888888ull + carry; rw[k] = (uint32_t)t; carry = t >> 32; }
        }
        const int32_t dv = (int32_t)((vw[win >> 3] >> (4 * (win & 7u))) & 15u) - 8, dr = (int32_t)((rw[win >> 3] >> (4 * (win & 7u))) & 15u) - 8;
        ge_ext acc = ge_identity();
        if (dv != 0) acc = ge_from_pniels_signed(table[(size_t)win * TT_MULTS + (dv < 0 ? -dv : dv) - 1], dv < 0);
        if (dr != 0) {
            const ge_pniels q = table[(size_t)(TT_WINDOWS + win) * TT_MULTS + (dr < 0 ? -dr : dr) - 1];
            acc = dv != 0 ? ge_add_pniels_signed(acc, q, dr < 0) : ge_from_pniels_signed(q, dr < 0);
        }
        L[win] = acc;
        __syncthreads();
        const uint32_t cr = win & 3u, slot = win >> 2;
        const fe *F = reinterpret_cast<const fe *>(L);
        fe s = F[(4 * slot + 0) * 4 + cr];
#pragma unroll 1
        for (uint32_t k = 1; k < 4; k++) s = quad_add(s, F[(4 * slot + k) * 4 + cr], cr);
        for (uint32_t d = 8; d > 0; d >>= 1) { const fe o = fe_shfl_down(s, 4u * d); s = quad_add(s, o, cr); }
        if (slot == 0) reinterpret_cast<fe *>(sums + wv * cpw + i)[cr] = s;
        __syncthreads();                                            // the wave's region is written again by its next commitment
    }
    // (the last barrier of the loop has published sums[0 .. per))
    if (wv == 0 && win < per && first + win < count) ge_compress(out + 32 * (size_t)(first + win), sums[win]);
}
// extended points -> 32-byte encodings, one thread per point (what the host's h51::pt_compress gives)
__global__ void __launch_bounds__(64) k_bt_compress(const ge_ext *__restrict__ in, uint8_t *__restrict__ out, uint32_t count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    ge_compress(out + 32 * (size_t)i, in[i]);
}
// powers of every item, one launch: blockIdx.y = 0: y^i -> ypow[k*N + i], 1: y^-i -> yinvpow[k*N + i] (i < N), 2: z^(r+1) -> zcat[rbase[k] + 1 + r]
// (r < q_k: the flattened weights index z by GLOBAL row + 1).  bases[k * 3 + table]; thread t of a table walks t, t + T, ... (T = 2^lgT) as k_exp_table does
__global__ void __launch_bounds__(256) k_bt_exp(const scm *__restrict__ bases, const uint32_t *__restrict__ qk, const uint32_t *__restrict__ rbase, uint32_t lgN,
                                                uint32_t lgT, scm *__restrict__ ypow, scm *__restrict__ yinvpow, scm *__restrict__ zcat) {
    const uint32_t tab = blockIdx.y, item = blockIdx.z;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, T = 1u << lgT;
    if (t >= T) return;
    const uint32_t count = tab == 2 ? qk[item] : (1u << lgN);
    scm *__restrict__ out = tab == 0 ? ypow + ((size_t)item << lgN) : (tab == 1 ? yinvpow + ((size_t)item << lgN) : zcat + rbase[item] + 1);
    const scm base = bases[(size_t)item * 3 + tab];
    scm cur = SC_R1(), sq = base;
    for (uint32_t b = 0; b < lgT; b++) {
        if ((t >> b) & 1u) cur = sc_mont_mul(cur, sq);
        sq = sc_mont_mul(sq, sq);
    }
    if (tab == 2) cur = sc_mont_mul(cur, base);                 // z^(i+1)
    for (uint32_t i = t; i < count; i += T) { out[i] = cur; cur = sc_mont_mul(cur, sq); }
}
// t1..t6 partial sums of every item (k_poly_t per item): blockIdx.y = item; partial[block * 6K + item * 6 + j]
__global__ void __launch_bounds__(256) k_bt_poly_t(const scm *__restrict__ aL, const scm *__restrict__ aR, const scm *__restrict__ aO,
                                                   const scm *__restrict__ sL, const scm *__restrict__ sR,
                                                   const scm *__restrict__ wL, const scm *__restrict__ wR, const scm *__restrict__ wO,
                                                   const scm *__restrict__ ypow, const scm *__restrict__ yinvpow, const uint32_t *__restrict__ nk, uint32_t lgN,
                                                   scm *__restrict__ partial) {
    __shared__ scm lds[256];
    const uint32_t item = blockIdx.y, n = nk[item], K = gridDim.y;
    const size_t o = (size_t)item << lgN;
    scm t1 = sc_zero(), t2 = t1, t3 = t1, t4 = t1, t5 = t1, t6 = t1;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const size_t q = o + i;
        scm y = ypow[q];
        scm l1 = sc_add(aL[q], sc_mont_mul(yinvpow[q], wR[q]));
        scm l2 = aO[q], l3 = sL[q];
        scm r0 = sc_sub(wO[q], y);
        scm r1 = sc_add(sc_mont_mul(y, aR[q]), wL[q]);
        scm r3 = sc_mont_mul(y, sR[q]);
        t1 = sc_add(t1, sc_mont_mul(l1, r0));
        t2 = sc_add(t2, sc_add(sc_mont_mul(l1, r1), sc_mont_mul(l2, r0)));
        t3 = sc_add(t3, sc_add(sc_mont_mul(l2, r1), sc_mont_mul(l3, r0)));
        t4 = sc_add(t4, sc_add(sc_mont_mul(l1, r3), sc_mont_mul(l3, r1)));
        t5 = sc_add(t5, sc_mont_mul(l2, r3));
        t6 = sc_add(t6, sc_mont_mul(l3, r3));
    }
    scm *dst = partial + (size_t)blockIdx.x * 6 * K + (size_t)item * 6;
    scm r;
    r = block_sum_256(t1, lds); if (threadIdx.x == 0) dst[0] = r;
    r = block_sum_256(t2, lds); if (threadIdx.x == 0) dst[1] = r;
    r = block_sum_256(t3, lds); if (threadIdx.x == 0) dst[2] = r;
    r = block_sum_256(t4, lds); if (threadIdx.x == 0) dst[3] = r;
    r = block_sum_256(t5, lds); if (threadIdx.x == 0) dst[4] = r;
    r = block_sum_256(t6, lds); if (threadIdx.x == 0) dst[5] = r;
}
// l(x), r(x) of every item (k_poly_eval per item, x = bsc[item][BSC_X]): blockIdx.y = item
__global__ void __launch_bounds__(256) k_bt_poly_eval(const scm *__restrict__ aL, const scm *__restrict__ aR, const scm *__restrict__ aO,
                                                      const scm *__restrict__ sL, const scm *__restrict__ sR,
                                                      const scm *__restrict__ wL, const scm *__restrict__ wR, const scm *__restrict__ wO,
                                                      const scm *__restrict__ ypow, const scm *__restrict__ yinvpow, const scm *__restrict__ bsc,
                                                      const uint32_t *__restrict__ nk, uint32_t lgN, scm *__restrict__ lv, scm *__restrict__ rv) {
    const uint32_t item = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << lgN)) return;
    const size_t q = ((size_t)item << lgN) + i;
    scm y = ypow[q];
    if (i >= nk[item]) { lv[q] = sc_zero(); rv[q] = sc_neg(y); return; }
    const scm x = bsc[(size_t)item * BSC + BSC_X];
    scm l1 = sc_add(aL[q], sc_mont_mul(yinvpow[q], wR[q]));
    scm r0 = sc_sub(wO[q], y);
    scm r1 = sc_add(sc_mont_mul(y, aR[q]), wL[q]);
    scm r3 = sc_mont_mul(y, sR[q]);
    lv[q] = sc_mont_mul(x, sc_add(l1, sc_mont_mul(x, sc_add(aO[q], sc_mont_mul(x, sL[q])))));
    rv[q] = sc_add(r0, sc_mont_mul(x, sc_add(r1, sc_mont_mul(x, sc_mont_mul(x, r3)))));
}
// per-base-point factors of every item (k_tt_factors at round 0 with Gamma = Eta = 1): fG, fH at [k*N, (k+1)*N); coefficient tables c at k * 4N
// (two halves of 2N for the ping-pong, G coefficients at +0 and H coefficients at +N of each half)
__global__ void __launch_bounds__(256) k_bt_factors(const scm *__restrict__ yinvpow, const scm *__restrict__ bsc, const uint32_t *__restrict__ nk, uint32_t lgN,
                                                    scm *__restrict__ fG, scm *__restrict__ fH, scm *__restrict__ c) {
    const uint32_t item = blockIdx.y, p = blockIdx.x * blockDim.x + threadIdx.x, N = 1u << lgN;
    if (p == 0) { scm *c0 = c + (size_t)item * 4 * N; c0[0] = SC_R1(); c0[N] = SC_R1(); }
    if (p >= N) return;
    const size_t q = ((size_t)item << lgN) + p;
    const bool pad = p >= nk[item];
    const scm u_ch = bsc[(size_t)item * BSC + BSC_UCH];
    fG[q] = pad ? u_ch : SC_R1();
    fH[q] = pad ? sc_mont_mul(yinvpow[q], u_ch) : yinvpow[q];
}
// k_tt_advance of every item with its own u, u^-1: half `cur` of its coefficient tables -> half cur ^ 1
__global__ void __launch_bounds__(256) k_bt_advance(scm *__restrict__ a, scm *__restrict__ b, const scm *__restrict__ bsc, uint32_t h, scm *__restrict__ c,
                                                    uint32_t cur, uint32_t cnt, uint32_t lgN) {
    const uint32_t item = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x, N = 1u << lgN;
    const scm u = bsc[(size_t)item * BSC + BSC_U], uinv = bsc[(size_t)item * BSC + BSC_UINV];
    if (i < h) {
        scm *ai = a + ((size_t)item << lgN), *bi = b + ((size_t)item << lgN);
        ai[i] = sc_add(sc_mont_mul(ai[i], u), sc_mont_mul(uinv, ai[h + i]));
        bi[i] = sc_add(sc_mont_mul(bi[i], uinv), sc_mont_mul(u, bi[h + i]));
    }
    if (i < cnt) {
        const scm *cprev = c + (size_t)item * 4 * N + (size_t)cur * 2 * N;
        scm *cnext = c + (size_t)item * 4 * N + (size_t)(cur ^ 1u) * 2 * N;
        const scm g = cprev[i], e = cprev[N + i];
        cnext[2 * i] = sc_mont_mul(g, uinv); cnext[2 * i + 1] = sc_mont_mul(g, u);
        cnext[N + 2 * i] = sc_mont_mul(e, u); cnext[N + 2 * i + 1] = sc_mont_mul(e, uinv);
    }
}
// sub-round j of every item's tail (k_tt_round per item): blockIdx.y = 0 L, 1 R; blockIdx.z = item; partial[(item * 2 + class) * gridDim.x + block]
__global__ void __launch_bounds__(256) k_bt_round(const ge_pniels *__restrict__ table, uint32_t M0T, const scm *__restrict__ a, const scm *__restrict__ b,
                                                  const scm *__restrict__ fG, const scm *__restrict__ fH, const scm *__restrict__ c, uint32_t cur,
                                                  uint32_t lgN, uint32_t j, ge_ext *__restrict__ partial, uint32_t quad) {
    __shared__ ge_ext lds[256];
    const uint32_t cls = blockIdx.y, item = blockIdx.z, tid = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t N = 1u << lgN, e = tid >> 3, g = tid & 7u;
    const size_t o = (size_t)item << lgN;
    ge_ext acc = ge_identity();
    if (e < N) {
        const bool isH = e >= (N >> 1);
        const uint32_t e2 = isH ? e - (N >> 1) : e;
        const uint32_t lgh = lgN - j - 1, h = 1u << lgh;
        const uint32_t t = e2 >> lgh, i = e2 & (h - 1);
        const bool hi = (cls == 0) != isH;                         // L: G_hi and H_lo;  R: G_lo and H_hi
        const uint32_t p = (t << (lgh + 1)) | (hi ? h : 0u) | i;
        const uint32_t sidx = hi ? i : (h | i);                    // the scalar of the opposite half
        scm s = isH ? b[o + sidx] : a[o + sidx];
        s = sc_mont_mul(s, isH ? fH[o + p] : fG[o + p]);
        s = sc_mont_mul(s, c[(size_t)item * 4 * N + (size_t)cur * 2 * N + (isH ? N : 0u) + t]);
        uint32_t w[8]; tt_biased_words(w, s);
        const ge_pniels *tbl = table + ((size_t)(isH ? M0T : 0u) + p) * (TT_WINDOWS * TT_MULTS) + (size_t)g * 8 * TT_MULTS;
        const uint32_t word = w[g];
#pragma unroll 1
        for (uint32_t k = 0; k < 8; k++) {
            const int32_t d = (int32_t)((word >> (4 * k)) & 15u) - 8;
            if (d == 0) continue;
            const uint32_t neg = d < 0, mag = neg ? (uint32_t)(-d) : (uint32_t)d;
            acc = ge_add_pniels_signed(acc, tbl[k * TT_MULTS + mag - 1], neg);
        }
    }
    ge_block_sum_store(acc, lds, quad, partial + ((size_t)item * 2 + cls) * gridDim.x + blockIdx.x);
}
// block (class, item) -> L or R of that item (k_tt_finish per item, w = bsc[item][BSC_W]); out[item * 2 + class]
__global__ void __launch_bounds__(256) k_bt_finish(const ge_ext *__restrict__ partial, uint32_t nblk, const scm *__restrict__ a, const scm *__restrict__ b,
                                                   uint32_t h, uint32_t lgN, const scm *__restrict__ bsc, const ge_pniels *__restrict__ tableB,
                                                   ge_ext *__restrict__ out, uint32_t quad) {
    __shared__ ge_ext lds[256];
    __shared__ scm slds[256];
    const uint32_t cls = blockIdx.x, item = blockIdx.y;
    const scm *ai = a + ((size_t)item << lgN), *bi = b + ((size_t)item << lgN);
    scm ip = sc_zero();
    for (uint32_t i = threadIdx.x; i < h; i += 256) ip = sc_add(ip, cls == 0 ? sc_mont_mul(ai[i], bi[h + i]) : sc_mont_mul(ai[h + i], bi[i]));
    const scm cw = sc_mont_mul(block_sum_256(ip, slds), bsc[(size_t)item * BSC + BSC_W]);
    const ge_ext *part = partial + ((size_t)item * 2 + cls) * nblk;
    ge_ext acc = ge_identity();
    uint32_t s0 = threadIdx.x;
    if (s0 < nblk) { acc = part[s0]; s0 += 256; }
    for (; s0 < nblk; s0 += 256) acc = ge_add(acc, part[s0]);
    const uint32_t win = 255u - threadIdx.x;
    if (win < TT_WINDOWS) {
        uint32_t w[8]; tt_biased_words(w, cw);
        const int32_t d = (int32_t)((w[win >> 3] >> (4 * (win & 7u))) & 15u) - 8;
        if (d != 0) {
            const uint32_t neg = d < 0, mag = neg ? (uint32_t)(-d) : (uint32_t)d;
            const ge_pniels q = tableB[win * TT_MULTS + mag - 1];
            acc = threadIdx.x >= nblk ? ge_from_pniels_signed(q, neg) : ge_add_pniels_signed(acc, q, neg);
        }
    }
    ge_block_sum_store(acc, lds, quad, out + (size_t)item * 2 + cls);
}
// the last round's scalar fold of every item (k_ipa_fold_scalars per item), then a[k*N], b[k*N] -> ab[2k], ab[2k+1]
__global__ void __launch_bounds__(256) k_bt_fold_scalars(scm *__restrict__ a, scm *__restrict__ b, const scm *__restrict__ bsc, uint32_t lgN,
                                                         scm *__restrict__ ab, uint32_t count) {
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= count) return;
    scm *ai = a + ((size_t)item << lgN), *bi = b + ((size_t)item << lgN);
    if (lgN) {      // h = 1: the fold has one output per item
        const scm u = bsc[(size_t)item * BSC + BSC_U], uinv = bsc[(size_t)item * BSC + BSC_UINV];
        ai[0] = sc_add(sc_mont_mul(ai[0], u), sc_mont_mul(uinv, ai[1]));
        bi[0] = sc_add(sc_mont_mul(bi[0], uinv), sc_mont_mul(u, bi[1]));
    }
    ab[2 * (size_t)item] = ai[0]; ab[2 * (size_t)item + 1] = bi[0];
}

}  // namespace bpg
