// Circuit templates joined on the device (Engine::join_templates): the circuit a host gets by assembling, in ONE prover, part 0's gadget code count_0 times,
// then part 1's count_1 times, and so on - "these k1 values are in range AND these k2 leaves are in the tree" as one statement, one proof.  A repeat
// (k_repeat.cuh) is the join of one part.  With B^x_p = sum over the parts before p of count x (that part's x), copy k of part p lives at
//   multiplier i -> B^n_p + k n_p + i         committed value j -> B^m_p + k m_p + j         constraint row r -> B^q_p + k q_p + r
//   parameter slot s -> B^par_p + k n_params_p + s                                         checkpoint c -> B^ck_p + k n_ck_p + c
// part-major, then item-major (join_map below: the ONE place that knows this, shared by the kernels, the host hooks of engine.hip and
// tests/hostcheck/template_join.cpp).  The coefficient table is [shared of part 0 | shared of part 1 | ... | slots of part 0 | slots of part 1 | ...]: the
// parameter slots stay one contiguous range behind the sum of the shared parts, which is all assign() and the verifier know of them.  Parts with PUBLIC
// INPUTS (bpg_r1cs_template_join_inputs) add a third range behind it, the derived slots, part-major then item-major like everything else:
//   derived slot s -> B^ds_p + k n_slots_p + s        input x -> B^in_p + k n_in_p + x        (a part without inputs contributes nothing to either)
// k_input_slots_join fills the range from the joined inputs in one launch per assign, before anything reads a constant term.
// The resident matrix is column-major (k_scalars.cuh: columns left | right | output | committed | constants).  Each of the five SECTIONS of the joined entry
// list holds part 0's count_0 copies of its section, then part 1's, and so on: the columns of a section stay in index order, and the constants column stays
// ONE column whose entries are in ascending row order (rows are part-major, item-major as well), which the row view of the check (k_check.cuh) relies on.
// The witness is evaluated by the PARTS' packed programs, one launch per level for all parts together: a block is 64 consecutive items of one segment of
// one part (the lane map of k_witness_eval_repeat), and a per-level block table says which.  A level of a hash part - one latency chain per lane - then runs
// beside the lanes of the other parts instead of after them.
#pragma once
#include <cstddef>
#include "k_repeat.cuh"

namespace bpg {

// One part of a join.  The first line is the part's template, the second where its copies start in the join, the third where its program lives in the
// join's concatenated program buffers; sec: the five sections of the template's OWN entry list ([sec[s], sec[s + 1])), sec_base[s]: where the part's
// count copies of section s start in the joined list.
struct JoinPart {
    uint32_t n, m, q, shared, n_params, n_ck, count;            // (the template's coefficient table: [0, shared) shared | n_params slots)
    uint32_t base_n, base_m, base_q, base_shared, base_slot, base_ck;      // base_slot: an index into the joined table (its shared parts included)
    uint32_t seg_first, stream_first, ck_var_first;
    uint64_t sec[6], sec_base[5];
    // public inputs (all zero: the part has none): the template takes n_in values and has n_slots derived coefficient slots behind its parameter slots; its
    // items' inputs start at base_in of the joined input list, their derived slots at base_dslot of the joined table (behind ALL parameter slots), and its
    // (input, coefficient index) pairs at slot_list_first of the joined pair list
    uint32_t n_in, n_slots, base_in, base_dslot, slot_list_first, reserved_;
};
struct JoinTotals { uint64_t n, m, q, nnz, shared, n_params, n_ck, n_in, n_slots; };

// the bases of every part from the dims, counts and sections of all of them (the caller has checked the totals against the instance format)
inline JoinTotals join_fill_bases(JoinPart *parts, size_t n_parts) {
    JoinTotals T{0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t pairs = 0;
    for (size_t p = 0; p < n_parts; p++) {
        JoinPart &P = parts[p];
        P.base_n = (uint32_t)T.n; P.base_m = (uint32_t)T.m; P.base_q = (uint32_t)T.q; P.base_shared = (uint32_t)T.shared; P.base_ck = (uint32_t)T.n_ck;
        P.base_slot = (uint32_t)T.n_params;                      // (the shared total is added below)
        P.base_in = (uint32_t)T.n_in; P.base_dslot = (uint32_t)T.n_slots; P.slot_list_first = pairs;      // (shared and parameter totals are added below)
        T.n += (uint64_t)P.count * P.n; T.m += (uint64_t)P.count * P.m; T.q += (uint64_t)P.count * P.q; T.nnz += (uint64_t)P.count * P.sec[5];
        T.shared += P.shared; T.n_params += (uint64_t)P.count * P.n_params; T.n_ck += (uint64_t)P.count * P.n_ck;
        T.n_in += (uint64_t)P.count * P.n_in; T.n_slots += (uint64_t)P.count * P.n_slots; pairs += P.n_slots;
    }
    uint64_t at = 0;
    for (int s = 0; s < 5; s++)
        for (size_t p = 0; p < n_parts; p++) { parts[p].sec_base[s] = at; at += (uint64_t)parts[p].count * (parts[p].sec[s + 1] - parts[p].sec[s]); }
    for (size_t p = 0; p < n_parts; p++) { parts[p].base_slot += (uint32_t)T.shared; parts[p].base_dslot += (uint32_t)(T.shared + T.n_params); }
    return T;
}

// copy k of (packed variable, coefficient slot, row) of part p's template
BPG_HD void join_map(const JoinPart *parts, uint32_t p, uint32_t k, uint32_t var, uint32_t coef, uint32_t row, uint32_t &var_out, uint32_t &coef_out, uint32_t &row_out) {
    const JoinPart &P = parts[p];
    const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
    var_out = kind <= 2 ? (kind << 29 | (P.base_n + k * P.n + idx)) : kind == 3 ? (kind << 29 | (P.base_m + k * P.m + idx)) : var;
    if (P.n_slots && coef >= P.shared + P.n_params) coef_out = P.base_dslot + k * P.n_slots + (coef - P.shared - P.n_params);     // a derived slot of a part with inputs
    else coef_out = coef >= P.shared ? P.base_slot + k * P.n_params + (coef - P.shared) : P.base_shared + coef;
    row_out = P.base_q + k * P.q + row;
}
// flat derived-slot index t of the join (part-major, item-major: slot t lives at parts[0].base_dslot + t of the joined table) -> (part, item, slot of the part's template)
BPG_HD void join_slot_place(const JoinPart *parts, uint32_t n_parts, uint64_t t, uint32_t &p, uint32_t &item, uint32_t &s) {
    const uint64_t at = parts[0].base_dslot + t;
    p = 0;
    while (p + 1 < n_parts && at >= parts[p + 1].base_dslot) p++;     // (a part without slots shares its base with the next one and is passed over)
    const uint64_t local = at - parts[p].base_dslot;
    item = (uint32_t)(local / parts[p].n_slots); s = (uint32_t)(local % parts[p].n_slots);
}
// One lane of the slot kernel below: derived slot t of the join.  pairs: the parts' (input, coefficient index) lists one after the other (x = input, y = index
// into the part's shared table); in: the joined inputs; coef: the joined table.  The factor comes from the ONE shared table of the part, whichever item asks.
BPG_HD void join_input_slot_lane(const JoinPart *parts, uint32_t n_parts, uint64_t t, const uint32_t *pairs, const scm *in, scm *coef) {
    uint32_t p, item, s;
    join_slot_place(parts, n_parts, t, p, item, s);
    const JoinPart &P = parts[p];
    const uint32_t ip = pairs[2 * ((size_t)P.slot_list_first + s)], ci = pairs[2 * ((size_t)P.slot_list_first + s) + 1];
    coef[(size_t)P.base_dslot + (size_t)item * P.n_slots + s] = witness_input_slot(coef[(size_t)P.base_shared + ci], in[(size_t)P.base_in + (size_t)item * P.n_in + ip]);
}
// the section (0 left .. 4 constants) of entry e of a part's own entry list
BPG_HD uint32_t join_section_of(const JoinPart &P, uint64_t e) { return e < P.sec[1] ? 0u : e < P.sec[2] ? 1u : e < P.sec[3] ? 2u : e < P.sec[4] ? 3u : 4u; }
// where entry e of section s of the part's template goes in copy k (repeat_entry_pos with the part's place in the section in front)
BPG_HD uint64_t join_entry_pos(const JoinPart &P, uint32_t s, uint64_t k, uint64_t e) { return P.sec_base[s] + k * (P.sec[s + 1] - P.sec[s]) + (e - P.sec[s]); }
// flat checkpoint index t of the join -> (part, item, checkpoint of the part's template)
BPG_HD void join_ck_place(const JoinPart *parts, uint32_t n_parts, uint64_t t, uint32_t &p, uint32_t &item, uint32_t &c) {
    p = 0;
    while (p + 1 < n_parts && t >= parts[p + 1].base_ck) p++;     // (a part without checkpoints shares its base with the next one and is passed over)
    const uint64_t local = t - parts[p].base_ck;
    item = (uint32_t)(local / parts[p].n_ck); c = (uint32_t)(local % parts[p].n_ck);
}

// one lane of the joined evaluation: segment (first, count, records) of part P's program for the part's item k.  coef, v, ck and the vectors are the JOIN's:
// a program reads no parameter slot, so its coefficient indices are those of the part's shared table.  in: the JOIN's public inputs (null: no part has any).
BPG_HD void witness_eval_join_lane(const JoinPart &P, uint32_t first, uint32_t count, const uint32_t *rec, const scm *coef, const scm *v, uint64_t k,
                                   scm *aL, scm *aR, scm *aO, const scm *ck, const scm *in = nullptr) {
    const size_t b = (size_t)P.base_n + (size_t)k * P.n;
    witness_eval_segment(first, count, rec, coef + P.base_shared, v + P.base_m + (size_t)k * P.m, aL + b, aR + b, aO + b,
                         ck ? ck + P.base_ck + (size_t)k * P.n_ck : nullptr, in ? in + P.base_in + (size_t)k * P.n_in : nullptr);
}

#if defined(__HIPCC__)
// col_ptr of the join, one launch per part: thread = (column c in [0, 3n + m] of the part's template, copies k = y, y + gridDim.y, ...).  The constants column is
// ONE column of the join: part 0 writes its start and the total.
__global__ void __launch_bounds__(256) k_join_colptr(const uint64_t *__restrict__ cp, const JoinPart *__restrict__ parts, uint32_t p, uint32_t n_tot, uint32_t m_tot,
                                                     uint64_t nnz_tot, uint64_t *__restrict__ out) {
    const JoinPart P = parts[p];
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x, ncol = 3 * P.n + P.m;
    if (c > ncol) return;
    if (c == ncol) {
        if (p == 0 && blockIdx.y == 0) { out[(size_t)3 * n_tot + m_tot] = P.sec_base[4]; out[(size_t)3 * n_tot + m_tot + 1] = nnz_tot; }
        return;
    }
    const uint32_t sec = c < 3 * P.n ? c / P.n : 3u;                                   // left, right, output, committed
    const uint64_t e = cp[c];
    for (uint32_t k = blockIdx.y; k < P.count; k += gridDim.y) {
        uint32_t var, coef, row;
        join_map(parts, p, k, repeat_var_of(c, P.n, P.m), 0, 0, var, coef, row);
        out[repeat_col_of(var, n_tot, m_tot)] = join_entry_pos(P, sec, k, e);
    }
}
// the entries of one part: thread = (entry e of the part's template, copies k = y, y + gridDim.y, ...)
__global__ void __launch_bounds__(256) k_join_entries(const uint32_t *__restrict__ ent_row, const uint32_t *__restrict__ ent_coef, const JoinPart *__restrict__ parts,
                                                      uint32_t p, uint32_t *__restrict__ row_out, uint32_t *__restrict__ coef_out) {
    const JoinPart P = parts[p];
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P.sec[5]) return;
    const uint32_t sec = join_section_of(P, e), r = ent_row[e], ci = ent_coef[e];
    for (uint32_t k = blockIdx.y; k < P.count; k += gridDim.y) {
        uint32_t var, coef, row;
        join_map(parts, p, k, 4u << 29, ci, r, var, coef, row);                         // (an entry carries no variable: its column does)
        const uint64_t pos = join_entry_pos(P, sec, k, e);
        row_out[pos] = row; coef_out[pos] = coef;
    }
}
// the coefficients of one part: its shared table once, its parameter slots (as they stand) once per copy, then its derived slots (as they stand) once per copy
__global__ void __launch_bounds__(256) k_join_coef(const scm *__restrict__ coef, const JoinPart *__restrict__ parts, uint32_t p, scm *__restrict__ out) {
    const JoinPart P = parts[p];
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, par_end = (uint64_t)P.shared + (uint64_t)P.count * P.n_params;
    if (i >= par_end + (uint64_t)P.count * P.n_slots) return;
    if (i < P.shared) out[P.base_shared + i] = coef[i];
    else if (i < par_end) out[(uint64_t)P.base_slot + (i - P.shared)] = coef[P.shared + (i - P.shared) % P.n_params];
    else out[(uint64_t)P.base_dslot + (i - par_end)] = coef[P.shared + P.n_params + (i - par_end) % P.n_slots];
}
// The derived coefficient slots of a repeat or join with public inputs: one lane per (part, item, slot), ONE launch per assign or set_inputs whatever the number
// of parts (a repeat: one part).  k_input_slots cannot serve: its per-item stride moves the factor with the item, and here every item of a part multiplies from the
// part's one shared table.  A slot is never a factor (ci names a shared table, below every slot), so no lane reads what another writes.
__global__ void __launch_bounds__(256) k_input_slots_join(const JoinPart *__restrict__ parts, uint32_t n_parts, uint64_t total, const uint32_t *__restrict__ pairs,
                                                          const scm *__restrict__ in, scm *coef) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    join_input_slot_lane(parts, n_parts, t, pairs, in, coef);
}
// One launch per level of the JOIN (levels 0 .. the most any part has).  blocks = that level's table: (part, segment in the joined segment list, first item);
// a block holds 64 consecutive ITEMS of one segment of one part, so a wave walks one record stream: same records, same classes, no divergence.
__global__ void __launch_bounds__(64) k_witness_eval_join(const uint4 *__restrict__ blocks, const JoinPart *__restrict__ parts, const uint4 *__restrict__ segs,
                                                          const uint32_t *__restrict__ stream, const scm *__restrict__ coef, const scm *__restrict__ v,
                                                          const scm *__restrict__ ck, const scm *__restrict__ in, scm *aL, scm *aR, scm *aO) {
    const uint4 b = blocks[blockIdx.x];
    const JoinPart &P = parts[b.x];
    const uint32_t item = b.z + threadIdx.x;
    if (item >= P.count) return;
    const uint4 sd = segs[b.y];
    witness_eval_join_lane(P, sd.x, sd.y, stream + P.stream_first + sd.z, coef, v, item, aL, aR, aO, ck, in);
}
// k_witness_ck_verify for a join: one lane per (part, item, checkpoint), flat index t in the joined checkpoint list; the lowest one whose value differs from what
// the circuit computed goes to *first (64-bit atomicMin; the host set it to all ones).  ck_var: the parts' checkpoint variables, part after part.
__global__ void __launch_bounds__(256) k_witness_ck_verify_join(const uint32_t *__restrict__ ck_var, const JoinPart *__restrict__ parts, uint32_t n_parts, uint64_t total,
                                                                const scm *__restrict__ ck, const scm *__restrict__ aL, const scm *__restrict__ aR,
                                                                const scm *__restrict__ aO, unsigned long long *first) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    uint32_t p, item, c;
    join_ck_place(parts, n_parts, t, p, item, c);
    const JoinPart &P = parts[p];
    const size_t b = (size_t)P.base_n + (size_t)item * P.n;
    if (!witness_ck_holds(ck_var[P.ck_var_first + c], ck[t], aL + b, aR + b, aO + b)) atomicMin(first, (unsigned long long)t);
}
#endif  // __HIPCC__

}  // namespace bpg
