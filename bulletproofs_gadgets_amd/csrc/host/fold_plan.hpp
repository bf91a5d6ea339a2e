// The generator fold of one group of rounds of the inner-product argument, decided and recoded before anything is launched: the group scalars, which
// of the seven fold kernels of hip/k_ipa.cuh takes the fold (choose_fold), and the scalars in the format that kernel reads (plain NAF bitmaps,
// width-w NAF digits per part, width-4 step lists).  No HIP and no device here: tests/hostcheck/plans.cpp checks the chooser row by row and the
// recoders against integer arithmetic on the CPU; Engine::Impl::fold_launch() uploads what the recoders wrote and launches what the chooser named, for
// inner_product() and for the test hook bpg_test_fold alike.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "r1cs_error.hpp"
#include "scalar.hpp"

namespace bpg {

// Kernel arguments of the fold kernels (hip/k_ipa.cuh; passed by value, filled here)
struct FoldGroup { uint32_t Mr, nterms, first_group, n; int32_t top; };                             // k_fold_points, _reg<NT>, _split, _quad
struct FoldWnaf { uint32_t Mr, nterms, first_group, n, cap; int32_t top; uint32_t parts, NM; };     // k_fold_points_wnaf
#define QW_MAXSTEPS 1024
struct FoldQuadW { uint32_t Mr, nterms, nsteps[2], tail[2]; };                                      // k_fold_points_quadw, _regw

// non-adjacent form of a canonical scalar; returns index of the top non-zero digit (-1 for zero)
inline int32_t naf256(const Scalar &s, int8_t d[256]) {
    uint64_t k[5] = {s.w[0], s.w[1], s.w[2], s.w[3], 0};
    std::memset(d, 0, 256);
    int32_t top = -1;
    for (int i = 0; i < 256; i++) {
        if ((k[0] | k[1] | k[2] | k[3] | k[4]) == 0) break;
        if (k[0] & 1) {
            int dig = 2 - (int)(k[0] & 3);           // +1 or -1
            d[i] = (int8_t)dig; top = i;
            if (dig == 1) k[0] -= 1;                  // low bit set, no borrow
            else { for (int j = 0; j < 5; j++) { if (++k[j] != 0) break; } }
        }
        for (int j = 0; j < 4; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 63);
        k[4] >>= 1;
    }
    return top;
}

// width-w non-adjacent form of a canonical scalar: odd digits in (-2^(w-1), 2^(w-1)), at most one non-zero in any w consecutive positions;
// returns the index of the top non-zero digit (-1 for zero).  Scalars are < 2^253, so position 255 is never reached.
inline int32_t wnaf256(const Scalar &s, uint32_t w, int8_t d[256]) {
    uint64_t k[5] = {s.w[0], s.w[1], s.w[2], s.w[3], 0};
    std::memset(d, 0, 256);
    int32_t top = -1;
    const int64_t full = 1ll << w, half = 1ll << (w - 1);
    for (int i = 0; i < 256; i++) {
        if ((k[0] | k[1] | k[2] | k[3] | k[4]) == 0) break;
        if (k[0] & 1) {
            int64_t dig = (int64_t)(k[0] & (uint64_t)(full - 1));
            if (dig >= half) dig -= full;
            d[i] = (int8_t)dig; top = i;
            if (dig > 0) { k[0] -= (uint64_t)dig; }                                                   // low bits cleared, no borrow
            else { uint64_t add = (uint64_t)(-dig); for (int j = 0; j < 5; j++) { uint64_t t = k[j] + add; add = t < add ? 1 : 0; k[j] = t; if (!add) break; } }
        }
        for (int j = 0; j < 4; j++) k[j] = (k[j] >> 1) | (k[j + 1] << 63);
        k[4] >>= 1;
    }
    return top;
}

// bits [from, from + count) of a canonical scalar as a scalar of its own (count <= 128)
inline Scalar scalar_bits(const Scalar &s, uint32_t from, uint32_t count) {
    Scalar r = Scalar::zero();
    for (uint32_t k = 0; k < count && from + k < 256; k++) {
        const uint32_t b = from + k;
        if ((s.w[b >> 6] >> (b & 63)) & 1ull) r.w[k >> 6] |= 1ull << (k & 63);
    }
    return r;
}

// The scalars of the fold of a group of g_r rounds on tables of size g_M with challenges us[0 .. g_r): Gst'[i] = Gst[i] + sum_{t>=1} sG_t Gst[i + t*Mr], same
// for H, with sG_t = prod_k (u_k^2)^bit_k(t), sH_t = prod_k (u_k^-2 y^-(g_M/2^k))^bit_k(t), bit_k(t) = bit (g_r - k) of t.  yinv_pow2[j] = y^-(2^j).
// Term t is entry t - 1 of sG, sH (2^g_r - 1 entries each).
inline void fold_group_scalars(const std::vector<Scalar> &us, const std::vector<Scalar> &yinv_pow2, uint64_t g_M, uint32_t g_r, std::vector<Scalar> &sG, std::vector<Scalar> &sH) {
    std::vector<Scalar> fG(g_r), fH(g_r);
    for (uint32_t k = 1; k <= g_r; k++) {
        const Scalar &uk = us[k - 1]; const Scalar ukinv = uk.invert();
        fG[k - 1] = uk * uk; fH[k - 1] = ukinv * ukinv * yinv_pow2[ceil_log2(g_M >> k)];
    }
    const uint32_t nterms = (1u << g_r) - 1u;
    sG.assign(nterms, Scalar::one()); sH.assign(nterms, Scalar::one());
    for (uint32_t t = 1; t <= nterms; t++)
        for (uint32_t k = 1; k <= g_r; k++) if ((t >> (g_r - k)) & 1u) { sG[t - 1] = sG[t - 1] * fG[k - 1]; sH[t - 1] = sH[t - 1] * fH[k - 1]; }
}

// lanes of term t that are padding generators (first group only): i + t*Mr >= n
inline uint64_t fold_padding_lanes(uint32_t t, uint32_t Mr, uint64_t n, bool first) {
    const uint64_t lo = (uint64_t)t * Mr;
    return !first ? 0 : (lo >= n ? Mr : (lo + Mr > n ? lo + Mr - n : 0));
}

// What a recoder reports: the top digit position over every scalar it wrote (the length of the doubling chain; for the step lists the mean of the two
// classes' doublings, as the roofline bookkeeping counts them), the field multiplications of the fold's additions, and the doublings of the step lists.
struct FoldRecode { int32_t top = -1; double adds_fm = 0, dbls_w = 0; };

// Plain NAF as two 256-bit masks per (class, term): out[4][nterms][16] words, non-zero digits at +0, negative ones at +8; class = 2*isH + isB, the B classes
// (scalar * u_ch, for the padding generators) only in the first group.
inline size_t fold_naf_words(uint32_t nterms) { return (size_t)4 * nterms * 16; }
inline FoldRecode fold_recode_naf(const std::vector<Scalar> &sG, const std::vector<Scalar> &sH, const Scalar &u_ch, uint32_t Mr, uint64_t n, bool first, uint32_t *out) {
    const uint32_t nterms = (uint32_t)sG.size();
    std::memset(out, 0, fold_naf_words(nterms) * 4);
    FoldRecode r;
    for (uint32_t q = 0; q < nterms; q++) {
        const Scalar cls_s[4] = {sG[q], sG[q] * u_ch, sH[q], sH[q] * u_ch};
        const uint64_t nB = fold_padding_lanes(q + 1, Mr, n, first);
        for (int cls = 0; cls < 4; cls++) {
            if ((cls & 1) && !first) continue;
            int8_t dg[256]; const int32_t tp = naf256(cls_s[cls], dg);
            if (tp > r.top) r.top = tp;
            uint32_t *d = out + ((size_t)cls * nterms + q) * 16; int adds = 0;
            for (int k = 0; k < 256; k++) { if (dg[k]) { d[k >> 5] |= 1u << (k & 31); adds++; } if (dg[k] < 0) d[8 + (k >> 5)] |= 1u << (k & 31); }
            r.adds_fm += 7.0 * adds * ((cls & 1) ? (double)nB : (double)(Mr - nB));
        }
    }
    return r;
}

// Width-w NAF digits of the scalars cut into `parts` pieces of L bits (k_fold_points_wnaf): out[4 classes][parts * nterms][256] signed odd digits, entry
// part * nterms + q holding part `part` of term q's scalar.
inline size_t fold_wnaf_bytes(uint32_t nterms, uint32_t parts) { return (size_t)4 * nterms * parts * 256; }
inline FoldRecode fold_recode_wnaf(const std::vector<Scalar> &sG, const std::vector<Scalar> &sH, const Scalar &u_ch, uint32_t Mr, uint64_t n, bool first,
                                   uint32_t w, uint32_t parts, uint32_t L, int8_t *out) {
    const uint32_t nterms = (uint32_t)sG.size(), nq = nterms * parts;
    std::memset(out, 0, fold_wnaf_bytes(nterms, parts));
    FoldRecode r;
    for (uint32_t q = 0; q < nterms; q++) {
        const Scalar cls_s[4] = {sG[q], sG[q] * u_ch, sH[q], sH[q] * u_ch};
        const uint64_t nB = fold_padding_lanes(q + 1, Mr, n, first);
        for (int cls = 0; cls < 4; cls++) {
            if ((cls & 1) && !first) continue;
            for (uint32_t part = 0; part < parts; part++) {
                int8_t *d = out + ((size_t)cls * nq + (size_t)part * nterms + q) * 256;
                const int32_t tp = wnaf256(scalar_bits(cls_s[cls], part * L, L), w, d);
                if (tp > r.top) r.top = tp;
                int adds = 0; for (int k = 0; k < 256; k++) adds += d[k] != 0;
                r.adds_fm += 7.0 * adds * ((cls & 1) ? (double)nB : (double)(Mr - nB));
            }
        }
    }
    return r;
}

// Width-4 NAF steps against odd multiples that the fold kernel makes itself (k_fold_points_quadw / _regw): one list of steps per class (G, H) in
// steps[2][QW_MAXSTEPS], step = doublings before the addition | term << 8 | multiple << 11 | sign << 13; fq.nsteps, fq.tail (doublings after the last
// addition) per class.  Doubling the identity ahead of the first addition is skipped.  Groups after the first only (no padding class).
inline FoldRecode fold_recode_steps(const std::vector<Scalar> &sG, const std::vector<Scalar> &sH, uint32_t Mr, uint32_t *steps, FoldQuadW &fq) {
    const uint32_t nterms = (uint32_t)sG.size();
    std::memset(&fq, 0, sizeof fq); fq.Mr = Mr; fq.nterms = nterms;
    double adds_w = 0, dbls_w = 0;
    for (uint32_t cls = 0; cls < 2; cls++) {
        std::vector<std::array<int8_t, 256>> dg(nterms);
        int32_t tp = -1;
        for (uint32_t q = 0; q < nterms; q++) tp = std::max(tp, wnaf256(cls ? sH[q] : sG[q], 4, dg[q].data()));
        uint32_t ns = 0, pending = 0;
        for (int32_t k = tp; k >= 0; k--) {
            if (ns) pending++;
            for (uint32_t q = 0; q < nterms; q++) {
                const int d = dg[q][k];
                if (!d) continue;
                if (ns >= QW_MAXSTEPS || pending > 255) throw std::logic_error("fold: step list overflow");
                const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
                steps[cls * QW_MAXSTEPS + ns++] = pending | (q << 8) | ((mag >> 1) << 11) | ((d < 0 ? 1u : 0u) << 13);
                dbls_w += pending; pending = 0;
            }
        }
        fq.nsteps[cls] = ns; fq.tail[cls] = pending; adds_w += ns; dbls_w += pending;
    }
    // field multiplications of the whole launch (8 per addition against a projective multiple; P, 2P, 3P, 5P, 7P and three conversions per term)
    FoldRecode r;
    r.adds_fm = (adds_w * 8.0 + nterms * 2.0 * (7.0 + 8.0 + 7.0 + 2 * 9.0 + 3.0)) * Mr; r.dbls_w = dbls_w; r.top = (int32_t)(dbls_w / 2.0) - 1;
    return r;
}

// ------------------------------------------------------------------------------------------------ which kernel folds
enum class FoldKernel {
    Wnaf,    // k_fold_points_wnaf: the original generators against their precomputed odd multiples
    QuadW,   // k_fold_points_quadw: four lanes per output, width-4 steps
    Quad,    // k_fold_points_quad: four lanes per output, plain NAF
    Split,   // k_fold_points_split: the four-wave latency variant
    RegW,    // k_fold_points_regw: one lane per output, width-4 steps, every operand from memory
    Reg,     // k_fold_points_reg<nterms>: addends in registers (groups of 1..4 rounds)
    Mem      // k_fold_points: addends from memory (groups of 5)
};
struct FoldKnobs {       // Engine::Impl: BPG_FOLD_WNAF, BPG_FOLD_SPLIT, BPG_FOLD_QUAD, BPG_FOLD_QUAD_W, BPG_FOLD_REG_W; shared: the proof takes the shared-device variants
    uint32_t fold_wnaf = 5, fold_split_max = 65536;
    bool fold_quad = true, fold_quad_w = true, fold_reg_w = true, shared = false;
};
struct FoldShape {
    uint32_t Mr, nterms;     // outputs per side, terms per output (2^r - 1)
    bool first;              // the first group of the proof (padding classes)
    bool original;           // the group-start tables are the context's own generator tables
};
// Rule 1 of choose_fold as far as the host can tell: the fold would take the precomputed odd multiples if they are there (the caller then asks for them,
// which may build them).  The raw knobs on purpose: a shared device does not switch the width-w NAF fold off.
inline bool fold_wants_tables(const FoldShape &s, const FoldKnobs &k) { return k.fold_wnaf >= 3 && s.original && 2 * (uint64_t)s.Mr > k.fold_split_max; }
// Seven rules in order, the first that holds decides.  tables: the odd multiples are available (asked for only when fold_wants_tables).
inline FoldKernel choose_fold(const FoldShape &s, const FoldKnobs &k, bool tables) {
    const uint32_t nterms = s.nterms;
    const uint64_t outputs = 2 * (uint64_t)s.Mr;
    const bool regs = nterms == 1 || nterms == 3 || nterms == 7 || nterms == 15;        // the group size has a register instantiation (r = 1..4)
    const uint32_t split_max = (regs && k.shared) ? 0 : k.fold_split_max;                // other proofs fill the device: fewest instructions
    if (fold_wants_tables(s, k) && tables) return FoldKernel::Wnaf;
    if (outputs <= split_max && nterms >= 1 && nterms <= 7 && k.fold_quad && k.fold_quad_w && !s.first && s.Mr % 64 == 0) return FoldKernel::QuadW;
    if (outputs <= split_max && nterms >= 1 && nterms <= 7 && k.fold_quad) return FoldKernel::Quad;
    if (outputs <= split_max && nterms >= 3 && nterms <= 15) return FoldKernel::Split;
    if (outputs > split_max && k.fold_reg_w && !s.first && nterms >= 1 && nterms <= 7 && s.Mr % 256 == 0) return FoldKernel::RegW;
    if (regs) return FoldKernel::Reg;
    return FoldKernel::Mem;
}

}  // namespace bpg
