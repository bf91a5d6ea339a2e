// A circuit template repeated K times on the device (Engine::repeat_template): the circuit a host gets by assembling the template's gadget code K times in
// a row into one prover.  Copy k of the template lives at
//   multiplier i -> k n + i        committed value j -> k m + j        constraint row r -> k q + r
//   parameter slot param_first + p -> param_first + k n_params + p     One and every other coefficient -> itself
//   derived slot param_first + n_params + s of a source with public inputs -> param_first + K n_params + k n_slots + s (behind ALL parameter slots), and item k
//   reads its own n_in inputs at k n_in: the table is [shared | K n_params parameter slots | K n_slots derived slots]
// (repeat_map below: the ONE place that knows this, shared by the kernels, the host hooks of engine.hip and tests/hostcheck/template_repeat.cpp).
// The resident matrix is column-major (k_scalars.cuh: columns left | right | output | committed | constants, entries = (row, coefficient slot)), so the
// replication works on columns: the five SECTIONS of the source's entry list are each written K times, copy after copy, which keeps every column's entries
// together and the columns of a section in index order - exactly the layout upload() gives the repeated rows, up to the order of entries within a column
// (a sum of exact field elements: no proof can tell).
// The witness of the repeat is evaluated by the SOURCE's packed program: one lane per (segment, item), item k reading and writing a_L, a_R, a_O at k n and
// its committed values at k m (the wave layout of k_witness_eval_batch has k << lg N there, which is another place whenever n is no power of two).
#pragma once
#include <cstddef>
#include "k_witness.cuh"

namespace bpg {

// of the SOURCE template; its coefficient table is [0, param_first) shared | n_params slots | n_slots derived slots (public inputs; 0: none, and count is not read)
struct RepeatDims { uint32_t n, m, q, param_first, n_params, n_slots, count; };

// copy k of (packed variable, coefficient slot, row) of the source
BPG_HD void repeat_map(const RepeatDims &d, uint32_t k, uint32_t var, uint32_t coef, uint32_t row, uint32_t &var_out, uint32_t &coef_out, uint32_t &row_out) {
    const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
    var_out = kind <= 2 ? (kind << 29 | (k * d.n + idx)) : kind == 3 ? (kind << 29 | (k * d.m + idx)) : var;
    if (d.n_slots && coef >= d.param_first + d.n_params) coef_out = coef + (d.count - 1) * d.n_params + k * d.n_slots;      // a derived slot: behind every item's parameters
    else coef_out = coef >= d.param_first ? coef + k * d.n_params : coef;     // (only constant terms name a slot)
    row_out = k * d.q + row;
}
// column of a packed variable in a matrix over n multipliers and m committed values (csc_col of k_scalars.cuh), and the packed variable of a column
BPG_HD uint32_t repeat_col_of(uint32_t var, uint32_t n, uint32_t m) {
    const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
    return kind <= 2 ? kind * n + idx : (kind == 3 ? 3 * n + idx : 3 * n + m);
}
BPG_HD uint32_t repeat_var_of(uint32_t col, uint32_t n, uint32_t m) {
    return col < 3 * n ? ((col / n) << 29 | (col % n)) : col < 3 * n + m ? (3u << 29 | (col - 3 * n)) : 4u << 29;
}
// where entry e of the source's section [s0, s1) goes in copy k: the section is written K times in a row, behind K copies of everything before it
BPG_HD uint64_t repeat_entry_pos(uint64_t K, uint64_t k, uint64_t s0, uint64_t s1, uint64_t e) { return K * s0 + k * (s1 - s0) + (e - s0); }

// one lane of the repeat evaluation: segment sd = (first, count, stream word) of the source for item k
// (ck, n_ck: the checkpoint values of a checkpointed source, item k's at ck + k n_ck; null, 0 otherwise.  in, n_in: the public inputs likewise, item k's at in + k n_in)
BPG_HD void witness_eval_repeat_lane(uint32_t first, uint32_t count, const uint32_t *rec, const scm *coef, const scm *v, uint32_t n, uint32_t m, uint64_t k,
                                     scm *aL, scm *aR, scm *aO, const scm *ck = nullptr, uint32_t n_ck = 0, const scm *in = nullptr, uint32_t n_in = 0) {
    const size_t b = (size_t)k * n;
    witness_eval_segment(first, count, rec, coef, v + (size_t)k * m, aL + b, aR + b, aO + b, ck ? ck + (size_t)k * n_ck : nullptr, in ? in + (size_t)k * n_in : nullptr);
}

#if defined(__HIPCC__)
// col_ptr of the repeat: thread = (source column c in [0, 3n + m], copies k = y, y + gridDim.y, ...).  The constant column is ONE column of the repeat as well: copy 0 writes its
// start and the total.
__global__ void __launch_bounds__(256) k_repeat_colptr(const uint64_t *__restrict__ cp, RepeatDims d, uint32_t K, uint64_t *__restrict__ out) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, ncol = 3 * d.n + d.m;
    if (c > ncol) return;
    if (c == ncol) {
        if (blockIdx.y == 0) { out[3 * K * d.n + K * d.m] = (uint64_t)K * cp[ncol]; out[3 * K * d.n + K * d.m + 1] = (uint64_t)K * cp[ncol + 1]; }
        return;
    }
    const uint32_t sec = c < 3 * d.n ? c / d.n : 3u;                                   // left, right, output, committed
    const uint32_t c0 = sec * d.n, c1 = sec < 3 ? c0 + d.n : c0 + d.m;
    const uint64_t s0 = cp[c0], s1 = cp[c1], e = cp[c];
    for (uint32_t k = blockIdx.y; k < K; k += gridDim.y) {
        uint32_t var, coef, row;
        repeat_map(d, k, repeat_var_of(c, d.n, d.m), 0, 0, var, coef, row);
        out[repeat_col_of(var, K * d.n, K * d.m)] = repeat_entry_pos(K, k, s0, s1, e);
    }
}
// the entries: thread = (source entry e, copies k = y, y + gridDim.y, ...); the section of e follows from the four column pointers that separate the five sections
__global__ void __launch_bounds__(256) k_repeat_entries(const uint64_t *__restrict__ cp, const uint32_t *__restrict__ ent_row, const uint32_t *__restrict__ ent_coef,
                                                        RepeatDims d, uint32_t K, uint64_t nnz, uint32_t *__restrict__ row_out, uint32_t *__restrict__ coef_out) {
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const uint64_t b1 = cp[d.n], b2 = cp[2 * d.n], b3 = cp[3 * d.n], b4 = cp[3 * d.n + d.m];
    const uint64_t s0 = e < b1 ? 0 : e < b2 ? b1 : e < b3 ? b2 : e < b4 ? b3 : b4;
    const uint64_t s1 = e < b1 ? b1 : e < b2 ? b2 : e < b3 ? b3 : e < b4 ? b4 : nnz;
    const uint32_t r = ent_row[e], ci = ent_coef[e];
    for (uint32_t k = blockIdx.y; k < K; k += gridDim.y) {
        uint32_t var, coef, row;
        repeat_map(d, k, 4u << 29, ci, r, var, coef, row);                          // (an entry carries no variable: its column does)
        const uint64_t pos = repeat_entry_pos(K, k, s0, s1, e);
        row_out[pos] = row; coef_out[pos] = coef;
    }
}
// the coefficient table: the shared part once, the source's parameter slots (as they stand) once per copy, then its derived slots (as they stand) once per copy
__global__ void __launch_bounds__(256) k_repeat_coef(const scm *__restrict__ coef, RepeatDims d, uint32_t K, scm *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, par_end = (uint64_t)d.param_first + (uint64_t)K * d.n_params;
    if (i >= par_end + (uint64_t)K * d.n_slots) return;
    out[i] = coef[i < d.param_first ? i : i < par_end ? d.param_first + (i - d.param_first) % d.n_params : d.param_first + d.n_params + (i - par_end) % d.n_slots];
}
// One launch per schedule level of the SOURCE; segs = that level's segments.  A block holds 64 consecutive ITEMS of one segment, the lane
// map of k_witness_eval_batch: same records, same classes, no divergence; blocks_per_seg = ceil(K / 64) blocks per segment, segment-major in x.
__global__ void __launch_bounds__(64) k_witness_eval_repeat(const uint4 *__restrict__ segs, uint32_t nseg, uint32_t blocks_per_seg, const uint32_t *__restrict__ stream,
                                                            const scm *__restrict__ coef, const scm *__restrict__ v, const scm *__restrict__ ck, uint32_t n_ck,
                                                            const scm *__restrict__ in, uint32_t n_in, uint32_t n, uint32_t m, uint32_t K, scm *aL, scm *aR, scm *aO) {
    const uint32_t s = blockIdx.x / blocks_per_seg, item = (blockIdx.x % blocks_per_seg) * blockDim.x + threadIdx.x;
    if (s >= nseg || item >= K) return;
    const uint4 sd = segs[s];
    witness_eval_repeat_lane(sd.x, sd.y, stream + sd.z, coef, v, n, m, item, aL, aR, aO, ck, n_ck, in, n_in);
}
#endif  // __HIPCC__

}  // namespace bpg
