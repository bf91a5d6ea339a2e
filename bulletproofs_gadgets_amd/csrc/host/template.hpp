// Circuit templates, host side: the checks on a witness program, its schedule, and the packed form the device interprets (hip/k_witness.cuh).
//
// A witness program (r1cs.hpp WitnessProgram) says how a_L[i], a_R[i] follow from committed values and EARLIER multipliers; a_O[i] is their product.
// The schedule cuts [0, n) into SEGMENTS of consecutive multipliers - one GPU lane walks a segment in order - and gives each a LEVEL such that everything
// a segment reads from another segment lies at a lower level (committed values: level -1).  One kernel launch per level, so no lane ever waits for another.
// Cutting rule: walk the multipliers in order; a multiplier that names a committed value, or a multiplier outside the current segment, which the segment
// has not named before opens a new segment.  (A MiMC sponge names the block it absorbs in every round of that block and nothing else from outside: one
// segment per absorbed block; a Merkle node absorbs two children: two segments per node, the second one level above the first.)
// A HINTED multiplier (a bit of a source, WitnessProgramView::hint_*) reads its source's terms under the same rules, and one more: a hinted multiplier whose
// source is not the source of the hinted multiplier right before it opens a segment.  A run of bit hints over one source - a range proof - is thus a lane of
// its own that reduces the source once (WIT_HINT_SAME_SOURCE), one level above whatever made the source, and is never hung onto the end of a 972-product
// chain.  (A 64-bit range proof over one committed value: one segment at level 0.)
// A CHECKPOINTED multiplier variable (WitnessProgramView::ck_var) is a value the caller hands to assign beside the committed ones.  It is WRITTEN like any
// multiplier and READ like a committed value: a multiplier that names a checkpoint its segment has not named before opens a new segment (also when the named
// multiplier lies inside the current segment), and the read adds nothing to the segment's level.  The packer writes every term that names it - left lists,
// right lists, hint sources - with the packed kind WIT_KIND_CHECKPOINT and the position in the checkpoint list, so the reader takes the caller's value and
// never another lane's.  (A sponge whose block states are checkpointed: every block a segment at level 0.  A Merkle path whose node hashes are: two levels.)
// Whether the caller's values ARE what the circuit computes is checked on the device after the last level (k_witness_ck_verify).  No checkpoints: the
// schedule and the stream are bit for bit what they were.
// A PUBLIC INPUT (Variable::Input, WitnessProgramView::n_inputs) is a value the caller hands to assign and nothing in the circuit computes.  It is read like a
// committed value: a level-0 source, and a multiplier that names an input its segment has not named opens a segment.  (LessThan against a public bound: the
// 4 segments on 1 level of LessThan against a constant; a hint run whose source is one input term is a lane of its own.)  The packer writes such a term with
// the packed kind WIT_KIND_INPUT.  In the ROWS a term (input p, coefficient index ci) becomes a constant term on a DERIVED coefficient slot that every assign
// fills with coef[ci] * x_p (with_parameter_slots, k_input_slots).  No inputs: schedule, stream and slot layout are bit for bit what they were.
// A GATED term (Variable::Gated, WitnessProgramView::n_gates) is coefficient * input p_k * variable var_k for entry k of the gate table.  To the schedule it is
// two reads: var_k under that variable's rules (committed, outside multiplier, checkpoint) and input p_k under the input's.  The packer writes it on two term
// slots (witness_record.hpp).  In the ROWS the term (gate k, ci) becomes (var_k, derived slot of the pair (p_k, ci)) - the slot list, order rule and
// de-duplication map of the constant input terms, so a pair a constant term and a gated term both use has ONE slot, and everything that fills slots
// (k_input_slots, the tails of a verify wave, the per-item ranges of a proving wave) stays as it is.  No gates: schedule, stream and slots are bit for bit what they were.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>
#include "r1cs.hpp"
#include "witness_record.hpp"

namespace bpg {

// A launch per level: a circuit that is one long chain of dependent segments is no GPU job.  A 512-leaf Merkle tree has 18 levels, a 1 MB MiMC preimage
// 32,768 (refused: assemble it on the host); 4,096 launches of a few microseconds each stay below the 0.3 s blinding chain the evaluation runs beside.
constexpr uint32_t WITNESS_MAX_LEVELS = 4096;

struct WitnessSchedule {
    std::vector<uint32_t> seg_first;    // nseg + 1: segment s = multipliers [seg_first[s], seg_first[s + 1])
    std::vector<uint32_t> seg_level;    // nseg
    std::vector<uint32_t> order;        // segments sorted by level (stable); level l = order[level_ptr[l] .. level_ptr[l + 1])
    std::vector<uint32_t> level_ptr;    // levels + 1
    uint32_t levels() const { return (uint32_t)level_ptr.size() - 1; }
    uint32_t segments() const { return (uint32_t)seg_level.size(); }
};

// Every check on a program against its instance (shape, index ranges, forward references, parameter rows): std::invalid_argument, no device work.
// the gate table against the instance's sizes (before anything indexes it)
inline void check_gate_table(const FlatView &c, const WitnessProgramView &p) {
    if (!p.n_gates) return;
    if (!p.gate_var || !p.gate_input) throw std::invalid_argument("template: n_gates without gate_var / gate_input");
    if (p.n_gates >= (1ull << 29)) throw std::invalid_argument("template: too many gates (the variable index has 29 bits)");
    for (uint64_t k = 0; k < p.n_gates; k++) {
        const uint32_t kind = p.gate_var[k] >> 29, idx = p.gate_var[k] & 0x1fffffffu;
        if (kind > 3) throw std::invalid_argument("template: gate " + std::to_string(k) + " gates a variable of kind " + std::to_string(kind) + " (a gate takes a multiplier variable or a committed value)");
        if (kind == 3 ? idx >= c.m : idx >= c.n) throw std::invalid_argument("template: gate " + std::to_string(k) + " gates a variable out of range");
        if (p.gate_input[k] >= p.n_inputs) throw std::invalid_argument("template: gate " + std::to_string(k) + " names public input " + std::to_string(p.gate_input[k]) + " (the template takes " + std::to_string(p.n_inputs) + ")");
    }
}
inline void check_witness_program(const FlatView &c, const WitnessProgramView &p) {
    if (c.n == 0) throw std::invalid_argument("template: the circuit has no multipliers");
    check_gate_table(c, p);
    if (!p.lc_ptr) throw std::invalid_argument("template: the witness program has no lc_ptr");
    if (p.lc_ptr[0] != 0) throw std::invalid_argument("template: lc_ptr[0] must be 0");
    for (uint64_t k = 0; k < 2 * c.n; k++) if (p.lc_ptr[k] > p.lc_ptr[k + 1]) throw std::invalid_argument("template: lc_ptr must not decrease");
    const uint64_t nterms = p.lc_ptr[2 * c.n];
    if (nterms && (!p.term_var || !p.term_coef)) throw std::invalid_argument("template: the witness program has no term arrays");
    if (nterms >= (1ull << 31)) throw std::invalid_argument("template: witness program too large");
    for (uint64_t i = 0; i < c.n; i++)
        for (uint64_t k = p.lc_ptr[2 * i]; k < p.lc_ptr[2 * i + 2]; k++) {
            const uint32_t kind = p.term_var[k] >> 29, idx = p.term_var[k] & 0x1fffffffu;
            if (p.term_coef[k] >= c.ncoef) throw std::invalid_argument("template: coefficient index out of range in the witness program");
            if (kind <= 2) { if (idx >= i) throw std::invalid_argument("template: multiplier " + std::to_string(i) + " refers to multiplier " + std::to_string(idx) + " (a multiplier may read only earlier multipliers and committed values)"); }
            else if (kind == 3) { if (idx >= c.m) throw std::invalid_argument("template: committed index out of range in the witness program"); }
            else if (kind == Variable::Input && p.n_inputs) {
                if (idx >= p.n_inputs) throw std::invalid_argument("template: multiplier " + std::to_string(i) + " names public input " + std::to_string(idx) + " (the template takes " + std::to_string(p.n_inputs) + ")");
            }
            else if (kind == Variable::Gated && p.n_gates) {
                if (idx >= p.n_gates) throw std::invalid_argument("template: multiplier " + std::to_string(i) + " names gate " + std::to_string(idx) + " (the template has " + std::to_string(p.n_gates) + ")");
                const uint32_t gk = p.gate_var[idx] >> 29, gi = p.gate_var[idx] & 0x1fffffffu;
                if (gk <= 2 && gi >= i) throw std::invalid_argument("template: multiplier " + std::to_string(i) + " refers to multiplier " + std::to_string(gi) + " through gate " + std::to_string(idx) + " (a multiplier may read only earlier multipliers and committed values)");
            }
            else if (kind != 4) throw std::invalid_argument("template: bad variable kind in the witness program (term " + std::to_string(k) + ", of multiplier " + std::to_string(i) + ", has kind " + std::to_string(kind) +
                                                            (kind == Variable::Input ? ": a public input, which only bpg_r1cs_upload_template_inputs takes)" :
                                                             kind == Variable::Gated ? ": a gated variable, which only bpg_r1cs_upload_template_gated takes)" : ")"));
        }
    if (p.n_hints && (!p.hint_mul || !p.hint_kind || !p.hint_arg)) throw std::invalid_argument("template: n_hints without hint arrays");
    for (uint64_t k = 0; k < p.n_hints; k++) {
        const uint64_t i = p.hint_mul[k];
        if (i >= c.n) throw std::invalid_argument("template: hint " + std::to_string(k) + " names multiplier " + std::to_string(i) + " (out of range)");
        if (k && p.hint_mul[k - 1] >= i) throw std::invalid_argument("template: hinted multipliers must be strictly ascending");
        if (p.hint_kind[k] != WITNESS_HINT_BIT_PAIR) throw std::invalid_argument("template: unknown hint kind " + std::to_string(p.hint_kind[k]));
        if (p.hint_arg[k] >= 256) throw std::invalid_argument("template: hint bit " + std::to_string(p.hint_arg[k]) + " (a scalar has 256 bits)");
        if (p.lc_ptr[2 * i + 1] != p.lc_ptr[2 * i + 2])
            throw std::invalid_argument("template: hinted multiplier " + std::to_string(i) + " has a right list" + ((p.term_var[p.lc_ptr[2 * i + 1]] >> 29) == Variable::Input ? " that names a public input" : "") +
                                        " (its left list is the source, the right list is empty)");
    }
    if (p.n_params && !p.param_rows) throw std::invalid_argument("template: n_params without param_rows");
    for (uint64_t k = 0; k < p.n_params; k++) {
        if (p.param_rows[k] >= c.q) throw std::invalid_argument("template: parameter row out of range");
        for (uint64_t j = 0; j < k; j++) if (p.param_rows[j] == p.param_rows[k]) throw std::invalid_argument("template: parameter row named twice");
    }
    if (p.n_ck && !p.ck_var) throw std::invalid_argument("template: n_checkpoints without vars");
    if (p.n_ck > 3 * c.n) throw std::invalid_argument("template: more checkpoints than multiplier variables (a variable is named twice)");
    std::unordered_map<uint32_t, uint32_t> seen;
    for (uint64_t k = 0; k < p.n_ck; k++) {
        const uint32_t kind = p.ck_var[k] >> 29, idx = p.ck_var[k] & 0x1fffffffu;
        if (kind > 2) throw std::invalid_argument("template: checkpoint " + std::to_string(k) + " is no multiplier variable (kind " + std::to_string(kind) + "; a checkpoint is a_L, a_R or a_O of a multiplier)");
        if (idx >= c.n) throw std::invalid_argument("template: checkpoint " + std::to_string(k) + " names multiplier " + std::to_string(idx) + " (out of range)");
        if (!seen.emplace(p.ck_var[k], (uint32_t)k).second) throw std::invalid_argument("template: checkpoint " + std::to_string(k) + " names a variable that checkpoint " + std::to_string(seen[p.ck_var[k]]) + " names already");
    }
}

// packed variable -> position in the checkpoint list (empty without checkpoints)
inline std::unordered_map<uint32_t, uint32_t> checkpoint_index(const WitnessProgramView &p) {
    std::unordered_map<uint32_t, uint32_t> at;
    at.reserve(p.n_ck);
    for (uint64_t k = 0; k < p.n_ck; k++) at.emplace(p.ck_var[k], (uint32_t)k);
    return at;
}

// hint k reads the source of hint k - 1, which sits on the multiplier right before: the same terms in the same order
inline bool hint_same_source(const WitnessProgramView &p, uint64_t k) {
    if (k == 0 || p.hint_mul[k - 1] + 1 != p.hint_mul[k]) return false;
    const uint64_t a = p.lc_ptr[2 * (uint64_t)p.hint_mul[k - 1]], b = p.lc_ptr[2 * (uint64_t)p.hint_mul[k]], cnt = p.lc_ptr[2 * (uint64_t)p.hint_mul[k] + 1] - b;
    if (b - a != cnt) return false;
    for (uint64_t t = 0; t < cnt; t++) if (p.term_var[a + t] != p.term_var[b + t] || p.term_coef[a + t] != p.term_coef[b + t]) return false;
    return true;
}

// (a checked program) -> schedule; refuses more than WITNESS_MAX_LEVELS levels
inline WitnessSchedule build_witness_schedule(uint64_t n, uint64_t m, const WitnessProgramView &p) {
    WitnessSchedule S;
    const uint32_t NONE = UINT32_MAX;
    std::vector<uint32_t> seg_of(n), seen_mul(n, NONE), seen_v(m, NONE), seen_ck(p.n_ck, NONE), seen_in(p.n_inputs, NONE);    // seen_*: the last segment that named this value from outside
    const std::unordered_map<uint32_t, uint32_t> ck_at = checkpoint_index(p);
    auto ck_of = [&](uint32_t var) { if (ck_at.empty()) return NONE; const auto it = ck_at.find(var); return it == ck_at.end() ? NONE : it->second; };
    uint32_t seg = NONE, first = 0;
    uint64_t h = 0;                                                          // next hint
    for (uint64_t i = 0; i < n; i++) {
        bool cut = (seg == NONE);
        if (h < p.n_hints && p.hint_mul[h] == i) { cut = cut || !hint_same_source(p, h); h++; }
        for (uint64_t k = p.lc_ptr[2 * i]; k < p.lc_ptr[2 * i + 2] && !cut; k++) {
            uint32_t var = p.term_var[k];
            if ((var >> 29) == Variable::Gated) {                                    // two reads: the input, then the gated variable under its own rules
                cut = seen_in[p.gate_input[var & 0x1fffffffu]] != seg;
                if (cut) break;
                var = p.gate_var[var & 0x1fffffffu];
            }
            const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
            const uint32_t ck = kind <= 2 ? ck_of(var) : NONE;
            if (kind == 3) cut = seen_v[idx] != seg;
            else if (kind == Variable::Input) cut = seen_in[idx] != seg;
            else if (ck != NONE) cut = seen_ck[ck] != seg;
            else if (kind <= 2 && idx < first) cut = seen_mul[idx] != seg;
        }
        if (cut) { seg = (uint32_t)S.seg_first.size(); first = (uint32_t)i; S.seg_first.push_back(first); S.seg_level.push_back(0); }
        seg_of[i] = seg;
        for (uint64_t k = p.lc_ptr[2 * i]; k < p.lc_ptr[2 * i + 2]; k++) {
            uint32_t var = p.term_var[k];
            if ((var >> 29) == Variable::Gated) { seen_in[p.gate_input[var & 0x1fffffffu]] = seg; var = p.gate_var[var & 0x1fffffffu]; }
            const uint32_t kind = var >> 29, idx = var & 0x1fffffffu;
            const uint32_t ck = kind <= 2 ? ck_of(var) : NONE;
            if (kind == 3) seen_v[idx] = seg;
            else if (kind == Variable::Input) seen_in[idx] = seg;                    // the caller's value: a level-0 source
            else if (ck != NONE) seen_ck[ck] = seg;                                  // the caller's value: no level, whoever computes it
            else if (kind <= 2 && idx < first) { seen_mul[idx] = seg; S.seg_level[seg] = std::max(S.seg_level[seg], S.seg_level[seg_of[idx]] + 1); }
        }
    }
    S.seg_first.push_back((uint32_t)n);
    uint32_t levels = 0;
    for (uint32_t l : S.seg_level) levels = std::max(levels, l + 1);
    if (levels > WITNESS_MAX_LEVELS)
        throw std::invalid_argument("template: the witness program is a chain of " + std::to_string(levels) + " dependent levels (at most " + std::to_string(WITNESS_MAX_LEVELS) + ": one launch per level)");
    S.level_ptr.assign(levels + 1, 0);
    for (uint32_t l : S.seg_level) S.level_ptr[l + 1]++;
    for (uint32_t l = 0; l < levels; l++) S.level_ptr[l + 1] += S.level_ptr[l];
    S.order.resize(S.seg_level.size());
    std::vector<uint32_t> at(S.level_ptr.begin(), S.level_ptr.end() - 1);
    for (uint32_t s = 0; s < S.seg_level.size(); s++) S.order[at[S.seg_level[s]]++] = s;
    return S;
}

inline std::string witness_schedule_json(const WitnessSchedule &S) {
    std::string j = "{\"levels\": " + std::to_string(S.levels()) + ", \"segments\": " + std::to_string(S.segments()) + ", \"max_levels\": " + std::to_string(WITNESS_MAX_LEVELS) + ", \"seg_first\": [";
    for (size_t i = 0; i < S.seg_first.size(); i++) { if (i) j += ","; j += std::to_string(S.seg_first[i]); }
    j += "], \"seg_level\": [";
    for (size_t i = 0; i < S.seg_level.size(); i++) { if (i) j += ","; j += std::to_string(S.seg_level[i]); }
    j += "], \"level_segments\": [";
    for (uint32_t l = 0; l < S.levels(); l++) { if (l) j += ","; j += std::to_string(S.level_ptr[l + 1] - S.level_ptr[l]); }
    return j + "]}";
}

// The packed program the device walks: record format in witness_record.hpp.
struct WitnessSegment { uint32_t first, count, stream, pad; };     // multipliers [first, first + count), records from word `stream`

struct PackedWitnessProgram {
    std::vector<uint32_t> stream;
    std::vector<WitnessSegment> segs;       // in WitnessSchedule::order
};
// share_sources = false (a measurement switch, BPG_WIT_HINT_SHARE=0): every hinted record carries its source and the reader reduces it again
inline PackedWitnessProgram pack_witness_program(const FlatView &c, const WitnessProgramView &p, const WitnessSchedule &S, bool share_sources = true) {
    static const uint8_t MINUS_ONE[32] = {0xec, 0xd3, 0xf5, 0x5c, 0x1a, 0x63, 0x12, 0x58, 0xd6, 0x9c, 0xf7, 0xa2, 0xde, 0xf9, 0xde, 0x14,
                                          0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x10};
    std::vector<uint8_t> cls(c.ncoef);      // 0 general, 1 plus one, 2 minus one, 3 zero
    for (uint64_t k = 0; k < c.ncoef; k++) {
        const Scalar s = Scalar::from_bytes_mod_order(c.coef + 32 * k);
        uint8_t b[32]; s.to_bytes(b);
        bool zero = true, one = b[0] == 1, minus = true;
        for (int i = 0; i < 32; i++) { zero = zero && b[i] == 0; one = one && (i == 0 || b[i] == 0); minus = minus && b[i] == MINUS_ONE[i]; }
        cls[k] = zero ? 3 : one ? WIT_COEF_PLUS_ONE : minus ? WIT_COEF_MINUS_ONE : WIT_COEF_GENERAL;
    }
    PackedWitnessProgram P;
    const std::unordered_map<uint32_t, uint32_t> ck_at = checkpoint_index(p);
    auto packed_var = [&](uint32_t var) {
        if ((var >> 29) == Variable::Input) return WIT_KIND_INPUT << 29 | (var & 0x1fffffffu);
        if (ck_at.empty()) return var;
        const auto it = ck_at.find(var);
        return it == ck_at.end() ? var : (WIT_KIND_CHECKPOINT << 29 | it->second);
    };
    std::vector<uint64_t> rec_at(c.n);
    P.stream.reserve(2 * c.n + 2 * p.lc_ptr[2 * c.n]);
    auto emit = [&](uint64_t a, uint64_t b) {
        uint32_t cnt = 0;
        for (uint64_t k = a; k < b; k++) {
            const uint32_t cl = cls[p.term_coef[k]];
            if (cl == 3) continue;
            if ((p.term_var[k] >> 29) == Variable::Gated) {                          // two slots: (variable, GATED | input), (-, class | coefficient index)
                const uint32_t g = p.term_var[k] & 0x1fffffffu;
                P.stream.push_back(packed_var(p.gate_var[g])); P.stream.push_back(WIT_COEF_GATED << WIT_CLASS_SHIFT | p.gate_input[g]);
                P.stream.push_back(0); P.stream.push_back(cl << WIT_CLASS_SHIFT | p.term_coef[k]); cnt += 2;
                continue;
            }
            P.stream.push_back(packed_var(p.term_var[k])); P.stream.push_back(cl << WIT_CLASS_SHIFT | p.term_coef[k]); cnt++;
        }
        return cnt;
    };
    std::vector<uint8_t> seg_start(c.n, 0);
    for (uint32_t s = 0; s < S.segments(); s++) seg_start[S.seg_first[s]] = 1;
    uint64_t hk = 0;                                                         // next hint
    for (uint64_t i = 0; i < c.n; i++) {
        const uint64_t l0 = p.lc_ptr[2 * i], l1 = p.lc_ptr[2 * i + 1], r1 = p.lc_ptr[2 * i + 2];
        rec_at[i] = P.stream.size();
        P.stream.push_back(0); P.stream.push_back(0);
        const uint64_t h = rec_at[i];
        if (hk < p.n_hints && p.hint_mul[hk] == i) {
            const bool shared = share_sources && !seg_start[i] && hint_same_source(p, hk);     // the reader starts every segment with no source held
            const uint32_t ns = shared ? 0u : emit(l0, l1);
            P.stream[h] = ns; P.stream[h + 1] = WIT_HINT_BIT_PAIR | (shared ? WIT_HINT_SAME_SOURCE : 0u) | (p.hint_arg[hk] & WIT_HINT_ARG_MASK);
            hk++;
            continue;
        }
        bool same = (l1 - l0 == r1 - l1);
        for (uint64_t k = 0; same && k < l1 - l0; k++) same = p.term_var[l0 + k] == p.term_var[l1 + k] && p.term_coef[l0 + k] == p.term_coef[l1 + k];
        if (2 * (r1 - l1) > WIT_RIGHT_COUNT_MASK) throw std::invalid_argument("template: witness program too large");
        const uint32_t nl = emit(l0, l1);
        const uint32_t nr = same ? 0u : emit(l1, r1);
        P.stream[h] = nl; P.stream[h + 1] = same ? WIT_SAME_AS_LEFT : nr;
    }
    if (c.ncoef > WIT_COEF_INDEX_MASK || P.stream.size() >= (1ull << 32)) throw std::invalid_argument("template: witness program too large");
    P.segs.resize(S.segments());
    for (uint32_t k = 0; k < S.segments(); k++) {
        const uint32_t s = S.order[k];
        P.segs[k] = WitnessSegment{S.seg_first[s], S.seg_first[s + 1] - S.seg_first[s], (uint32_t)rec_at[S.seg_first[s]], 0};
    }
    return P;
}

// Parameter rows (bpg_witness_program.param_rows): row r's constant terms become ONE term on a coefficient slot of its own, ncoef + k for parameter k, which
// starts at the sum of the constants it replaces (zero when the row had none) and is overwritten by every assign().  The other terms keep their order.
// Input terms (bpg_r1cs_upload_template_inputs): a term (input p, coefficient index ci) of a row becomes a constant term on a DERIVED slot, one per distinct pair
// (p, ci) in the order the rows name them, laid out behind the parameter slots: slot s is coefficient ncoef + n_params + s and holds coef[ci] * x_p, which
// every assign writes (k_input_slots).  derived (out): the pairs, slot by slot.  input_values (n_inputs x 32, may be null): what the slots start with.
struct InputSlot { uint32_t p, ci; };
inline FlatCircuit with_parameter_slots(const FlatView &c, const WitnessProgramView &p, std::vector<InputSlot> *derived = nullptr, const uint8_t *input_values = nullptr) {
    if (p.n_inputs) {
        if (!derived) throw std::logic_error("template: input slots without a list to keep them in");
        // the parameter pass first, over the caller's table: it folds the constants of a parameter row and keeps every other term, input terms among them, as
        // it is - an input term beside a parameter slot stays a term of its own
        WitnessProgramView q = p; q.n_inputs = 0;
        FlatCircuit f = with_parameter_slots(c, q);
        const uint64_t first = c.ncoef + p.n_params, room = (uint64_t)WIT_COEF_INDEX_MASK + 1 - std::min<uint64_t>(first, WIT_COEF_INDEX_MASK);
        std::unordered_map<uint64_t, uint32_t> slot_of;
        for (size_t k = 0; k < f.term_var.size(); k++) {
            const uint32_t tk = f.term_var[k] >> 29;
            if (tk != Variable::Input && tk != Variable::Gated) continue;
            uint32_t ip = f.term_var[k] & 0x1fffffffu, to = Variable::one().packed();
            const uint32_t ci = f.term_coef[k];
            if (tk == Variable::Gated) {            // (gate g, ci) -> (var_g, slot of (p_g, ci)): the pair's slot, whoever named the pair first
                if (ip >= p.n_gates) throw std::invalid_argument("template: a constraint names gate " + std::to_string(ip) + " (the template has " + std::to_string(p.n_gates) + ")");
                to = p.gate_var[ip]; ip = p.gate_input[ip];
            }
            if (ip >= p.n_inputs) throw std::invalid_argument("template: a constraint names public input " + std::to_string(ip) + " (the template takes " + std::to_string(p.n_inputs) + ")");
            const auto at = slot_of.emplace((uint64_t)ip << 32 | ci, (uint32_t)derived->size());
            if (at.second) {
                if (derived->size() >= room) throw std::invalid_argument("template: the derived coefficient slots of the public inputs are too many");
                derived->push_back(InputSlot{ip, ci});
            }
            f.term_var[k] = to; f.term_coef[k] = (uint32_t)(first + at.first->second);
        }
        f.coef.resize(32 * (first + derived->size()));
        for (size_t s = 0; s < derived->size() && input_values; s++) {
            const Scalar x = Scalar::from_bytes_mod_order(c.coef + 32 * (size_t)(*derived)[s].ci) * Scalar::from_bytes_mod_order(input_values + 32 * (size_t)(*derived)[s].p);
            x.to_bytes(&f.coef[32 * (first + s)]);
        }
        return f;
    }
    FlatCircuit f; f.n = c.n; f.m = c.m;
    std::vector<int64_t> param_of(c.q, -1);
    for (uint64_t k = 0; k < p.n_params; k++) param_of[p.param_rows[k]] = (int64_t)k;
    f.coef.assign(c.coef, c.coef + 32 * c.ncoef);
    f.coef.resize(32 * (c.ncoef + p.n_params));
    f.term_var.reserve(c.nnz + p.n_params); f.term_coef.reserve(c.nnz + p.n_params);
    f.row_ptr.reserve(c.q + 1);
    for (uint64_t r = 0; r < c.q; r++) {
        Scalar sum;
        for (uint64_t k = c.row_ptr[r]; k < c.row_ptr[r + 1]; k++) {
            if (param_of[r] >= 0 && (c.term_var[k] >> 29) == Variable::One) { sum += Scalar::from_bytes_mod_order(c.coef + 32 * c.term_coef[k]); continue; }
            f.term_var.push_back(c.term_var[k]); f.term_coef.push_back(c.term_coef[k]);
        }
        if (param_of[r] >= 0) {
            f.term_var.push_back(Variable::one().packed()); f.term_coef.push_back((uint32_t)(c.ncoef + param_of[r]));
            (sum.is_canonical() ? sum : sum.reduced()).to_bytes(&f.coef[32 * (c.ncoef + param_of[r])]);
        }
        f.row_ptr.push_back(f.term_var.size());
    }
    return f;
}

// Everything upload_template needs from the host, made in ONE pass over the program (checks first): Engine::plan_template
struct TemplatePlan {
    WitnessSchedule schedule;
    PackedWitnessProgram packed;
    FlatCircuit slotted;            // the instance's rows with parameter slots (no witness)
    uint64_t n_params = 0, param_first = 0;
    std::vector<uint32_t> ck_var;   // the checkpointed variables, in the caller's order (empty: none)
    // public inputs: how many values assign takes, and the derived coefficient slots [slot_first, slot_first + in_slots.size()) of the rows, kept resident
    uint64_t n_inputs = 0, slot_first = 0;
    std::vector<InputSlot> in_slots;
    uint64_t n_gates = 0;           // gates of the program and the rows (0: none; a template with gates is refused by repeat, join and check_batch)
};

}  // namespace bpg
