// TEST HARNESS, stand-alone: gated variables through the host compiler - Prover::gate, the checks, the schedule, the packer and the derived slots of
// csrc/host/template.hpp, and the interpreter of csrc/hip/k_witness.cuh (its BPG_HD half).  tests/test_gates_sanitized_host.py builds it with
// -fsanitize=address,undefined and expects "ok" on the last line.
//   1. A hand-made circuit of 9 multipliers (gates over a committed value, over the previous output, over an earlier segment, under +1, -1 and a general
//      coefficient, two inputs on one variable, a pair shared with a constant input term, a plain row, a hint run over a gated source): ONE template, made
//      from the first input vector, is evaluated under every vector (0, 1, l - 1 and 2^252 + 9 among the values) and must give the witness a fresh assembly
//      of that vector computes; every slotted row must vanish on that witness.
//   2. The depth-2 Merkle path (MerklePath256): the template of index 0 under the inputs of every index, against the assembly of that index.
// Streams and coefficient tables are heap blocks of exactly the sizes the plan gives: an overrun is an ASan report.
#include "../../bulletproofs_gadgets_amd/csrc/host/gadgets.hpp"
#include "../../bulletproofs_gadgets_amd/csrc/host/template.hpp"
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_witness.cuh"
#include <cstdio>
#include <cstring>
using namespace bpg;

namespace bpg {
// the two pieces of the host mirror this program needs and csrc/capi.hip defines (it is not linked here)
const std::vector<Scalar> &mimc_round_constants() {
    static const uint64_t RC[486][4] = {
#include "../../bulletproofs_gadgets_amd/csrc/host/mimc_rc769.inc"
    };
    static const std::vector<Scalar> v = [] {
        std::vector<Scalar> out(486);
        for (int i = 0; i < 486; i++) out[i] = Scalar::from_bits(reinterpret_cast<const uint8_t *>(RC[i]));
        return out;
    }();
    return v;
}
Variable Prover::commit_precomputed(const Scalar &v, const Scalar &v_blinding, const uint8_t com[32]) {
    const uint32_t idx = (uint32_t)v_.size();
    v_.push_back(v); vb_.push_back(v_blinding);
    V_.insert(V_.end(), com, com + 32);
    t_->append_point("V", com);
    flushed_ = v_.size();
    return Variable{Variable::Committed, idx};
}
}  // namespace bpg

static int fail(const char *what, int at = -1) { std::printf("FAILED: %s (%d)\n", what, at); return 1; }
static Scalar S(uint64_t x) { return Scalar::from_u64(x); }
static Scalar big() { uint8_t b[32] = {9}; b[31] = 0x10; return Scalar::from_bits(b); }          // 2^252 + 9
static Scalar red(const Scalar &s) { return s.is_canonical() ? s : s.reduced(); }
static scm to_scm(const Scalar &s) { uint8_t b[32]; red(s).to_bytes(b); uint32_t w[8]; std::memcpy(w, b, 32); return sc_from_words(w); }
static Scalar from_scm(const scm &x) { uint32_t w[8]; sc_to_words(w, x); uint8_t b[32]; std::memcpy(b, w, 32); return Scalar::from_bytes_mod_order(b); }
static LinearCombination operator*(const Variable &v, const Scalar &s) { return LinearCombination(v) * s; }

struct Assembly {
    Transcript t{std::string("gates")};
    Prover p{nullptr, &t};
    std::vector<Variable> v;
    void commit(const std::vector<Scalar> &values) { const uint8_t com[32] = {7}; for (auto &x : values) v.push_back(p.commit_precomputed(red(x), S(1), com)); }
};

static void hand(Assembly &a, const std::vector<Scalar> &in, const std::vector<Scalar> &values) {
    Prover &p = a.p;
    a.commit(values);
    std::vector<Variable> X;
    for (auto &x : in) X.push_back(p.input(x));
    auto G = [&](int k, const Variable &var) { return p.gate(X[k], var); };
    const Scalar m1 = -Scalar::one();
    MulVars m0 = p.multiply(LinearCombination(G(0, a.v[0])) + a.v[1], LinearCombination(a.v[0]) + X[1]);
    MulVars q1 = p.multiply(G(1, m0.o) * m1 + LinearCombination(Scalar::one()), LinearCombination(m0.l));
    MulVars q2 = p.multiply(G(2, q1.o) * S(5) + G(3, q1.o) * S(7), LinearCombination(a.v[1]) + q1.r);
    MulVars q3 = p.multiply(LinearCombination(a.v[0]) + X[2] * S(5), G(2, a.v[1]) * S(5) + q2.o);
    MulVars q4 = p.multiply(G(0, m0.l) * big() + a.v[0], LinearCombination(G(3, q3.o)) + LinearCombination(S(3)));
    const LinearCombination src = LinearCombination(G(3, q3.o)) + a.v[1];
    const OptScalar src_value(red(p.eval(src)));
    for (uint32_t bit = 0; bit < 3; bit++) p.allocate_bit(src, bit, src_value);
    MulVars q8 = p.multiply(LinearCombination(G(2, q4.r)) + q3.o, LinearCombination(q4.o) + X[0] * m1);
    p.constrain(G(2, q4.r) * S(9) + q3.o * S(9) - q8.l * S(9));
}

static void path(Assembly &a, uint64_t index, const Scalar &leaf, const std::vector<Scalar> &sib, const Scalar &root) {
    a.commit({leaf});
    std::vector<Variable> X;
    for (auto &x : merkle_path_inputs(index, sib, root)) X.push_back(a.p.input(x));
    std::vector<MerklePath256::Level> lv;
    for (size_t j = 0; j < sib.size(); j++) lv.push_back({X[4 * j], X[4 * j + 1], X[4 * j + 2], X[4 * j + 3]});
    MerklePath256(LinearCombination(X[4 * sib.size()]), a.v[0], lv).assemble(a.p, {}, {});
}

// the template of `tmpl` evaluated under the inputs and committed values of `other`: the interpreter's witness against other's own, and every slotted row on it
static int check(Assembly &tmpl, Assembly &other, bool with_ck, const char *what, int at) {
    FlatCircuit f = tmpl.p.flatten(true);
    WitnessProgram w = tmpl.p.witness_program(true);
    std::vector<uint32_t> gv, gi, ck;
    for (auto &g : tmpl.p.gates()) { gv.push_back(g.first); gi.push_back(g.second); }
    if (with_ck) for (size_t k = 0; k < tmpl.p.noted_vars().size(); k++) if (tmpl.p.noted_tags()[k] & MimcHash256::NOTE_LAST_BLOCK) ck.push_back(tmpl.p.noted_vars()[k]);
    FlatView c(f); c.aL = c.aR = c.aO = nullptr;
    WitnessProgramView p(w);
    p.n_inputs = tmpl.p.inputs().size(); p.n_gates = gv.size(); p.gate_var = gv.data(); p.gate_input = gi.data();
    p.n_ck = ck.size(); p.ck_var = ck.data();
    check_witness_program(c, p);
    const WitnessSchedule sched = build_witness_schedule(c.n, c.m, p);
    const PackedWitnessProgram P = pack_witness_program(c, p, sched);
    std::vector<InputSlot> slots;
    const FlatCircuit rows = with_parameter_slots(c, p, &slots);
    for (uint32_t v : rows.term_var) if ((v >> 29) > 4) return fail("a slotted row names an input or a gate", at);
    for (uint32_t v : f.term_var) if ((v >> 29) == Variable::Gated) goto kept;
    return fail("the template instance lost its gated terms", at);
kept:
    // exact-size heap blocks for everything the interpreter reads
    const FlatCircuit own = other.p.flatten();
    const size_t n = c.n;
    std::vector<uint32_t> stream(P.stream);
    std::vector<scm> coef(c.ncoef), vv(c.m), in(p.n_inputs), ckv(ck.size()), aL(n), aR(n), aO(n);
    for (size_t k = 0; k < c.ncoef; k++) coef[k] = to_scm(Scalar::from_bytes_mod_order(c.coef + 32 * k));
    for (size_t k = 0; k < c.m; k++) vv[k] = to_scm(other.p.v()[k]);
    for (size_t k = 0; k < p.n_inputs; k++) in[k] = to_scm(other.p.inputs()[k]);
    auto own_value = [&](uint32_t var) { const std::vector<uint8_t> &vec = (var >> 29) == 0 ? own.aL : (var >> 29) == 1 ? own.aR : own.aO; return Scalar::from_bytes_mod_order(&vec[32 * (var & 0x1fffffffu)]); };
    for (size_t k = 0; k < ck.size(); k++) ckv[k] = to_scm(own_value(ck[k]));
    const std::vector<uint32_t> &lp = sched.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l + 1]; s-- > lp[l];)
            witness_eval_segment(P.segs[s].first, P.segs[s].count, stream.data() + P.segs[s].stream, coef.data(), vv.data(), aL.data(), aR.data(), aO.data(),
                                 ck.empty() ? nullptr : ckv.data(), in.data());
    for (size_t i = 0; i < n; i++) {
        uint8_t b[3][32];
        from_scm(aL[i]).to_bytes(b[0]); from_scm(aR[i]).to_bytes(b[1]); from_scm(aO[i]).to_bytes(b[2]);
        if (std::memcmp(b[0], &own.aL[32 * i], 32) || std::memcmp(b[1], &own.aR[32 * i], 32) || std::memcmp(b[2], &own.aO[32 * i], 32)) { std::printf("%s: multiplier %zu\n", what, i); return fail("the interpreter's witness differs from the assembly's", at); }
    }
    for (size_t k = 0; k < ck.size(); k++) if (!witness_ck_holds(ck[k], ckv[k], aL.data(), aR.data(), aO.data())) return fail("a true checkpoint does not hold", at);
    // the rows with their slots filled as k_input_slots fills them
    std::vector<Scalar> table(rows.coef.size() / 32);
    for (size_t k = 0; k < table.size(); k++) table[k] = Scalar::from_bytes_mod_order(&rows.coef[32 * k]);
    const size_t first = c.ncoef + p.n_params;
    if (table.size() != first + slots.size()) return fail("slot table size", at);
    for (size_t s = 0; s < slots.size(); s++) table[first + s] = from_scm(witness_input_slot(coef[slots[s].ci], in[slots[s].p]));
    for (size_t r = 0; r + 1 < rows.row_ptr.size(); r++) {
        Scalar acc;
        for (uint64_t k = rows.row_ptr[r]; k < rows.row_ptr[r + 1]; k++) {
            const uint32_t var = rows.term_var[k], kind = var >> 29;
            acc += table[rows.term_coef[k]] * (kind == 4 ? Scalar::one() : kind == 3 ? other.p.v()[var & 0x1fffffffu] : own_value(var));
        }
        if (!(red(acc) == Scalar::zero())) { std::printf("%s: row %zu\n", what, r); return fail("a slotted row does not vanish on the witness", at); }
    }
    return 0;
}

int main() {
    const Scalar lm1 = -Scalar::one();
    const std::vector<std::vector<Scalar>> ins = {{S(0), S(1), lm1, big()}, {S(1), S(0), S(5), S(7)}, {big(), lm1, S(0), S(1)}, {S(3), S(11), big() * S(3), lm1 - S(1)}};
    const std::vector<std::vector<Scalar>> vals = {{S(3), S(4)}, {big(), lm1 - S(1)}, {S(0), S(9)}, {S(6), big() + S(5)}};
    {
        Assembly t; hand(t, ins[0], vals[0]);
        if (t.p.get_num_multiplications() != 9 || t.p.gates().size() < 9) return fail("hand circuit shape");
        for (int k = 0; k < 4; k++) { Assembly o; hand(o, ins[k], vals[k]); if (check(t, o, false, "hand", k)) return 1; }
        // the refusals of gate()
        const Variable x = Variable{Variable::Input, 0}, c0 = t.v[0];
        const std::pair<Variable, Variable> bad[] = {{c0, c0}, {Variable{Variable::Input, 4}, c0}, {x, Variable::one()}, {x, x}, {x, Variable{Variable::Gated, 0}},
                                                     {x, Variable{Variable::Committed, 2}}, {x, Variable{Variable::MultiplierOutput, 9}}};
        for (auto &b : bad) { try { t.p.gate(b.first, b.second); return fail("gate accepted a bad argument"); } catch (const std::invalid_argument &) {} }
        OpBuffer buf(0, true);
        try { buf.constrain(LinearCombination(Variable{Variable::Gated, 0})); return fail("a buffer took a gate"); } catch (const std::invalid_argument &) {}
        try { buf.gate(x, c0); return fail("a buffer made a gate"); } catch (const std::invalid_argument &) {}
    }
    {
        const std::vector<Scalar> &rc = mimc_round_constants();
        std::vector<Scalar> leaf = {S(11), big(), lm1, S(0)};
        const Scalar n0 = mimc_sponge_1({leaf[0], leaf[1]}, rc), n1 = mimc_sponge_1({leaf[2], leaf[3]}, rc), root = mimc_sponge_1({n0, n1}, rc);
        Assembly t; path(t, 0, leaf[0], {leaf[1], n1}, root);
        if (t.p.get_num_multiplications() != 2 * 1944 || t.p.inputs().size() != 9 || t.p.gates().size() != 4) return fail("path shape");
        for (uint64_t i = 0; i < 4; i++) {
            Assembly o; path(o, i, leaf[i], {leaf[i ^ 1], i < 2 ? n1 : n0}, root);
            if (check(t, o, false, "path", (int)i) || check(t, o, true, "checkpointed path", (int)i)) return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
