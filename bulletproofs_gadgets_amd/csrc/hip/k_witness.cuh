// Circuit templates: a_L, a_R, a_O of a resident circuit computed on the device from the committed values (Engine::assign).
// The kernel INTERPRETS the packed witness program (record format: host/witness_record.hpp, written by host/template.hpp); nothing here knows a gadget.
//   one launch per level of the schedule, one lane per segment of that level; the lane walks its multipliers in order:
//   left = sum of its terms, right likewise (or the same value when the record says the two lists are one), output = left * right.
// Everything a lane reads was written by an EARLIER launch (lower level) or by the lane itself: there is no flag, no spin and no wait on another lane.
// Values are Montgomery form, canonical - what upload() leaves in aL / aR / aO (k_sc_from_bytes) - so a proof cannot tell which of the two filled them.
// A lane is a latency chain (a MiMC block: 972 dependent products); the last multiplier's three values stay in registers because the programs the
// gadgets record read them back at once (a MiMC round reads the previous output, then the square's left value).
// A HINTED record (a range proof's bit: WIT_HINT_BIT_PAIR) is no product: the lane evaluates the record's source, takes it out of Montgomery form once, and
// keeps the eight canonical words in registers for the records that follow with WIT_HINT_SAME_SOURCE - a 64-bit range costs one reduction and 64 bit
// extractions.  Which branch a record takes is a property of the RECORD (the same for every lane that walks it); the bit itself, the only thing that differs
// between the items of a batch, selects by mask.
// A term of kind WIT_KIND_CHECKPOINT reads `ck`, the values the caller handed to assign (Engine::assign_checkpointed), by its position in the checkpoint
// list - never a_L, a_R, a_O and never the register copy of the last multiplier, whoever computes that variable.  So a level still reads only what an earlier
// launch, the lane itself or the caller wrote.  k_witness_ck_verify, after the last level, compares every checkpoint with what the circuit computed for it.
// A term of kind WIT_KIND_INPUT reads `in`, the public inputs the caller handed to assign (Engine::assign_inputs), by the input's index - a word of the record,
// the same for every lane that walks it, so the items of a batch stay convergent: only the value differs.  The ROWS of the matrix never name an input: their
// input terms are constant terms on derived coefficient slots, which k_input_slots fills per item before anything reads constant terms (a repeat or join
// with inputs: k_input_slots_join of k_join.cuh, a lane per (part, item, slot)).
// A GATED term (class WIT_COEF_GATED, two term slots: host/witness_record.hpp) is coefficient * in[p] * x: x is fetched as for any term - the previous
// multiplier's registers, aL / aR / aO, v or ck -, multiplied by the input the first slot names, and the second slot's class decides as before whether a
// product with the coefficient follows.  One product under +-1, two under a general coefficient; which branch is taken is again a word of the record.
#pragma once
#include "sc.cuh"
#include "../host/witness_record.hpp"

namespace bpg {

struct WitPrev { scm l, r, o; uint32_t idx; };

// sum of `count` terms at t[0 .. 2 count): (packed variable, class << 30 | coefficient index)
BPG_HD scm witness_eval_lc(const uint32_t *t, uint32_t count, const WitPrev &prev, const scm *coef, const scm *v, const scm *aL, const scm *aR, const scm *aO,
                           const scm *ck, const scm *in) {
    scm acc = sc_zero();
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t var = t[2 * k], cw = t[2 * k + 1];
        const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
        uint32_t cls = cw >> WIT_CLASS_SHIFT, ci = cw & WIT_COEF_INDEX_MASK;
        if (kind == 4) {                                            // the constant One: the coefficient itself, no product
            acc = sc_add(acc, cls == WIT_COEF_PLUS_ONE ? SC_R1() : cls == WIT_COEF_MINUS_ONE ? sc_neg(SC_R1()) : coef[ci]);
            continue;
        }
        scm x;
        if (kind <= 2 && idx == prev.idx) x = kind == 0 ? prev.l : kind == 1 ? prev.r : prev.o;
        else x = (kind == 0 ? aL : kind == 1 ? aR : kind == 2 ? aO : kind == WIT_KIND_CHECKPOINT ? ck : kind == WIT_KIND_INPUT ? in : v)[idx];
        if (cls == WIT_COEF_GATED) {                                // coefficient * in[p] * x: p stands where the coefficient index does, the term's own
            x = sc_mont_mul(in[ci], x);                             // class and index in the next slot (a word of the record: the same for every lane)
            k++;
            const uint32_t cw2 = t[2 * k + 1];
            cls = cw2 >> WIT_CLASS_SHIFT; ci = cw2 & WIT_COEF_INDEX_MASK;
        }
        if (cls == WIT_COEF_PLUS_ONE) acc = sc_add(acc, x);
        else if (cls == WIT_COEF_MINUS_ONE) acc = sc_sub(acc, x);
        else acc = sc_add(acc, sc_mont_mul(coef[ci], x));
    }
    return acc;
}

// bit `bit` (0..255) of the little-endian words w[0..8): the word is picked by compares, not by an indexed read of a register array
BPG_HD uint32_t witness_bit(const uint32_t *w, uint32_t bit) {
    const uint32_t k = bit >> 5;
    uint32_t x = w[0];
    BPG_UNROLL for (uint32_t j = 1; j < 8; j++) x = k == j ? w[j] : x;
    return (x >> (bit & 31u)) & 1u;
}

// multipliers [first, first + count) from the records at `rec`; ck: the checkpoint values (null for a program without checkpoints: no term names one);
// in: the item's public inputs, canonical Montgomery form (null for a program without inputs, likewise)
BPG_HD void witness_eval_segment(uint32_t first, uint32_t count, const uint32_t *rec, const scm *coef, const scm *v, scm *aL, scm *aR, scm *aO,
                                 const scm *ck = nullptr, const scm *in = nullptr) {
    WitPrev prev; prev.l = prev.r = prev.o = sc_zero(); prev.idx = 0xffffffffu;
    uint32_t src[8];                                                // canonical words of the last hint source (the packer never shares across segments)
    BPG_UNROLL for (int k = 0; k < 8; k++) src[k] = 0;
    for (uint32_t i = first; i < first + count; i++) {
        const uint32_t nl = rec[0], w1 = rec[1];
        if (w1 & WIT_HINT_BIT_PAIR) {
            if (!(w1 & WIT_HINT_SAME_SOURCE)) sc_to_words(src, witness_eval_lc(rec + 2, nl, prev, coef, v, aL, aR, aO, ck, in));
            const uint32_t set = 0u - witness_bit(src, w1 & WIT_HINT_ARG_MASK);     // all ones when the bit is set
            const scm one = SC_R1();
            scm l, r;
            BPG_UNROLL for (int k = 0; k < 8; k++) { l.v[k] = one.v[k] & ~set; r.v[k] = one.v[k] & set; }
            aL[i] = l; aR[i] = r; aO[i] = sc_zero();
            prev.l = l; prev.r = r; prev.o = sc_zero(); prev.idx = i;
            rec += 2 + 2 * nl;
            continue;
        }
        const uint32_t same = w1 & WIT_SAME_AS_LEFT, nr = w1 & WIT_RIGHT_COUNT_MASK;
        const scm l = witness_eval_lc(rec + 2, nl, prev, coef, v, aL, aR, aO, ck, in);
        const scm r = same ? l : witness_eval_lc(rec + 2 + 2 * nl, nr, prev, coef, v, aL, aR, aO, ck, in);
        const scm o = sc_mont_mul(l, r);
        aL[i] = l; aR[i] = r; aO[i] = o;
        prev.l = l; prev.r = r; prev.o = o; prev.idx = i;
        rec += 2 + 2 * (nl + nr);
    }
}

// Does checkpoint k of an item hold?  var = ck_var[k]; aL, aR, aO and ck are the ITEM's (both sides canonical Montgomery form: equal values, equal words)
BPG_HD bool witness_ck_holds(uint32_t var, const scm &given, const scm *aL, const scm *aR, const scm *aO) {
    const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
    const scm x = (kind == 0 ? aL : kind == 1 ? aR : aO)[idx];
    uint32_t diff = 0;
    BPG_UNROLL for (int j = 0; j < 8; j++) diff |= x.v[j] ^ given.v[j];
    return diff == 0;
}

// what a derived coefficient slot of a template with public inputs holds: coef[ci] * x_p, both canonical Montgomery form (k_input_slots; the host hook
// bpg_test_template_inputs_instance calls the same function)
BPG_HD scm witness_input_slot(const scm &c, const scm &x) { return sc_mont_mul(c, x); }

#if defined(__HIPCC__)     // the kernels; everything above also compiles for the host alone (tests/hostcheck/template_repeat.cpp)
// segs: (first multiplier, count, first record word, -) per segment of ONE level.  Blocks are small (the engine spreads a level's few hundred lanes
// over many waves: a lane alone in its wave reads one cache line per load, 64 lanes read 64).
__global__ void __launch_bounds__(64) k_witness_eval(const uint4 *__restrict__ segs, uint32_t nseg, const uint32_t *__restrict__ stream,
                                                     const scm *__restrict__ coef, const scm *__restrict__ v, const scm *__restrict__ ck,
                                                     const scm *__restrict__ in, scm *aL, scm *aR, scm *aO) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg) return;
    const uint4 sd = segs[s];
    witness_eval_segment(sd.x, sd.y, stream + sd.z, coef, v, aL, aR, aO, ck, in);
}

// The derived coefficient slots of a template with public inputs (host/template.hpp with_parameter_slots): one lane per (item, slot), flat index t = item * n_slots
// + s.  slots[s] = (input p, coefficient index ci); the slot holds coef[ci] * x_p.  Item k's table starts at coef + k * stride (assign: one item; a lockstep
// wave: the items' ranges of the wave's table), its slots at slot_first in it, its inputs at in + k * n_in.  Both factors are canonical Montgomery form and so
// is the product.  A slot is never a factor (ci names the caller's table, below the parameter slots), so no lane reads what another writes.
__global__ void __launch_bounds__(256) k_input_slots(const uint2 *__restrict__ slots, uint32_t n_slots, uint32_t slot_first, uint32_t stride, uint32_t n_in,
                                                     uint64_t total, const scm *__restrict__ in, scm *coef) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t item = t / n_slots;
    const uint32_t s = (uint32_t)(t - item * n_slots);
    const uint2 sl = slots[s];
    scm *tab = coef + (size_t)item * stride;
    tab[slot_first + s] = witness_input_slot(tab[sl.y], in[(size_t)item * n_in + sl.x]);
}

// After the last level of a checkpointed assign: one lane per (item, checkpoint), flat index t = item * n_ck + k; item's vectors at item * n (a plain template:
// one item).  The lowest flat index whose value differs from what the circuit computed goes to *first (64-bit atomicMin; the host set it to all ones).
__global__ void __launch_bounds__(256) k_witness_ck_verify(const uint32_t *__restrict__ ck_var, uint32_t n_ck, uint64_t total, uint32_t n, const scm *__restrict__ ck,
                                                           const scm *__restrict__ aL, const scm *__restrict__ aR, const scm *__restrict__ aO, unsigned long long *first) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t item = t / n_ck;
    const uint32_t k = (uint32_t)(t - item * n_ck);
    const size_t b = (size_t)item * n;
    if (!witness_ck_holds(ck_var[k], ck[t], aL + b, aR + b, aO + b)) atomicMin(first, (unsigned long long)t);
}

// K witnesses of ONE template in the wave layout of a lockstep batch (k_batch.cuh: item k's vectors of length N live at [k*N, (k+1)*N)); item k's
// committed values at v[k*m .. (k+1)*m).  One launch per level: blockIdx.y = segment of the level, x = item, so the 64 lanes of a wave are consecutive
// ITEMS of one segment.  They walk the same records - same term counts, same classes, no divergence - and segment, record words and coefficients are
// wave-uniform loads; only the values differ.  (Consecutive segments of one item, the map of k_witness_eval, diverge on record length and leave each lane
// alone in its cache lines.)  The stream and the coefficient table are the template's own: a program reads no parameter slot.
// ck: item k's n_ck checkpoint values at ck[k * n_ck ..) (a checkpointed template; n_ck = 0: none, ck is not read).  The position a term names is a word of the
// record - wave-uniform like everything else the lanes walk; only the values differ.
// in: item k's n_in public inputs at in[k * n_in ..) (n_in = 0: none, in is not read); the index a term names is again a word of the record.
__global__ void __launch_bounds__(64) k_witness_eval_batch(const uint4 *__restrict__ segs, const uint32_t *__restrict__ stream, const scm *__restrict__ coef,
                                                           const scm *__restrict__ v, const scm *__restrict__ ck, uint32_t n_ck, const scm *__restrict__ in,
                                                           uint32_t n_in, uint32_t m, uint32_t lgN, uint32_t K, scm *aL, scm *aR, scm *aO) {
    const uint32_t item = blockIdx.x * blockDim.x + threadIdx.x;
    if (item >= K) return;
    const uint4 sd = segs[blockIdx.y];
    const size_t b = (size_t)item << lgN;
    witness_eval_segment(sd.x, sd.y, stream + sd.z, coef, v + (size_t)item * m, aL + b, aR + b, aO + b, n_ck ? ck + (size_t)item * n_ck : nullptr,
                         n_in ? in + (size_t)item * n_in : nullptr);
}

// After the last level of a checkpointed wave: one lane per (item, checkpoint), flat index t = item * n_ck + k, item's vectors at item << lgN.  The lowest
// checkpoint of an item whose value differs from what the circuit computed goes to first[item] (32-bit atomicMin; the wave set the K words to all ones).
__global__ void __launch_bounds__(256) k_witness_ck_verify_batch(const uint32_t *__restrict__ ck_var, uint32_t n_ck, uint64_t total, uint32_t lgN,
                                                                 const scm *__restrict__ ck, const scm *__restrict__ aL, const scm *__restrict__ aR,
                                                                 const scm *__restrict__ aO, uint32_t *first) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const uint64_t item = t / n_ck;
    const uint32_t k = (uint32_t)(t - item * n_ck);
    const size_t b = (size_t)item << lgN;
    if (!witness_ck_holds(ck_var[k], ck[t], aL + b, aR + b, aO + b)) atomicMin(first + item, k);
}
#endif  // __HIPCC__

}  // namespace bpg
