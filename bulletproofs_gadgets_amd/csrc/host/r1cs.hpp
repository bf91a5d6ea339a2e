// Host-side constraint-system surface (product code, C++), mirroring bulletproofs::r1cs as the reference uses it:
//   Variable / LinearCombination                       src/bin/prover.rs:8,245 ; src/conversions.rs:49-64
//   trait ConstraintSystem {multiply, allocate, allocate_multiplier, constrain}   src/cs_buffer.rs:89-113
//   Prover::{new, commit, num_constraints, get_num_multiplications, prove}        src/bin/prover.rs:54,89,92-93
//   Verifier::{new, commit, get_num_vars}                                         src/bin/verifier.rs:51-53,89
// Assembly (witness synthesis, LC evaluation, constraint list) stays on the host exactly as in the reference; only
// commit() and prove() cross the C ABI into the HIP engine.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>
#include "scalar.hpp"
#include "merlin.hpp"
#include "r1cs_error.hpp"

namespace bpg {

struct Variable {
    // Input: public value idx of THIS proof (Prover::input / Verifier::input) - a constant to the proof system, a variable to a circuit template
    // Gated: entry idx of THIS assembly's gate table (Prover::gate / Verifier::gate): the product of a public input and a variable of kind 0..3
    enum Kind : uint32_t { MultiplierLeft = 0, MultiplierRight = 1, MultiplierOutput = 2, Committed = 3, One = 4, Input = 5, Gated = 6 };
    Kind kind; uint32_t idx;
    static Variable one() { return Variable{One, 0}; }
    uint32_t packed() const { return (static_cast<uint32_t>(kind) << 29) | idx; }
    static Variable unpack(uint32_t p) { return Variable{static_cast<Kind>(p >> 29), p & 0x1fffffffu}; }
};

// Terms of a linear combination.  Nearly every combination the gadgets build has one to four terms (a MiMC round makes seven of them per
// multiplier pair), so the first four live inside the object and nothing is allocated; longer ones move to the heap.
class TermVec {
public:
    using value_type = std::pair<Variable, Scalar>;
    using iterator = value_type *;
    using const_iterator = const value_type *;
    TermVec() {}
    TermVec(const TermVec &o) { append(o.begin(), o.end()); }
    TermVec(TermVec &&o) noexcept { take(o); }
    TermVec &operator=(const TermVec &o) { if (this != &o) { n_ = 0; append(o.begin(), o.end()); } return *this; }
    TermVec &operator=(TermVec &&o) noexcept { if (this != &o) { n_ = 0; heap_.clear(); take(o); } return *this; }
    size_t size() const { return n_; }
    bool empty() const { return n_ == 0; }
    iterator begin() { return data(); }
    iterator end() { return data() + n_; }
    const_iterator begin() const { return data(); }
    const_iterator end() const { return data() + n_; }
    value_type &operator[](size_t i) { return data()[i]; }
    const value_type &operator[](size_t i) const { return data()[i]; }
    void push_back(const value_type &t) { reserve(n_ + 1); data()[n_++] = t; }
    void emplace_back(const Variable &v, const Scalar &s) { push_back(value_type(v, s)); }
    template <class It> void insert(const_iterator at, It first, It last) {       // appending only (what LinearCombination needs)
        if (at != end()) throw std::logic_error("TermVec::insert: only at end()");
        append(first, last);
    }
    void reserve(size_t need) {
        const size_t cap = heap_.empty() ? INLINE : heap_.size();
        if (need <= cap) return;
        std::vector<value_type> h(std::max(need, 2 * cap));
        std::copy(begin(), end(), h.begin());
        heap_.swap(h);
    }
private:
    static constexpr size_t INLINE = 4;
    template <class It> void append(It first, It last) { for (; first != last; ++first) push_back(*first); }
    void take(TermVec &o) {
        if (!o.heap_.empty()) heap_.swap(o.heap_); else std::copy(o.inl_, o.inl_ + o.n_, inl_);
        n_ = o.n_; o.n_ = 0; o.heap_.clear();
    }
    value_type *data() { return heap_.empty() ? inl_ : heap_.data(); }
    const value_type *data() const { return heap_.empty() ? inl_ : heap_.data(); }
    value_type inl_[INLINE];
    std::vector<value_type> heap_;
    size_t n_ = 0;
};

struct LinearCombination {
    TermVec terms;
    LinearCombination() {}
    LinearCombination(const Variable &v) { terms.emplace_back(v, Scalar::one()); }          // From<Variable>
    LinearCombination(const Scalar &s) { terms.emplace_back(Variable::one(), s); }           // From<Scalar>
    LinearCombination operator+(const LinearCombination &o) const { LinearCombination r = *this; r.terms.insert(r.terms.end(), o.terms.begin(), o.terms.end()); return r; }
    LinearCombination operator-(const LinearCombination &o) const { LinearCombination r = *this; for (auto &t : o.terms) r.terms.emplace_back(t.first, -t.second); return r; }
    LinearCombination operator-() const { LinearCombination r; for (auto &t : terms) r.terms.emplace_back(t.first, -t.second); return r; }
    LinearCombination operator*(const Scalar &s) const { LinearCombination r; for (auto &t : terms) r.terms.emplace_back(t.first, t.second * s); return r; }
};

struct OptScalar { bool some; Scalar v; OptScalar() : some(false) {} OptScalar(const Scalar &s) : some(true), v(s) {} };
struct MulVars { Variable l, r, o; };

class ConstraintSystem {
public:
    virtual ~ConstraintSystem() {}
    virtual MulVars multiply(LinearCombination left, LinearCombination right) = 0;
    virtual Variable allocate(const OptScalar &assignment) = 0;
    virtual MulVars allocate_multiplier(bool some, const Scalar &l, const Scalar &r) = 0;
    virtual void constrain(const LinearCombination &lc) = 0;
    // The multiplier a range proof makes for bit `bit` (0..255) of `source`: a_L = 1 - b, a_R = b, with b read off the little-endian bytes of the value
    // the caller assigns to the source (utils.rs:9-21).  To a verifier and to a recording buffer it is allocate_multiplier and nothing more; a Prover also
    // notes WHERE the bit comes from, so that the circuit stays a template (bpg_witness_hints).  `source` is constrained by the caller, not here.
    virtual MulVars allocate_bit(const LinearCombination &source, uint32_t bit, const OptScalar &source_assignment) {
        (void)source;
        if (bit >= 256) throw std::invalid_argument("allocate_bit: a scalar has 256 bits");
        Scalar l, r;
        if (source_assignment.some) {
            const uint32_t b = (source_assignment.v.as_bytes()[bit / 8] >> (bit % 8)) & 1u;
            l = Scalar::from_u64(1u - b); r = Scalar::from_u64(b);
        }
        return allocate_multiplier(source_assignment.some, l, r);
    }
    // "The value of `lc` is one a caller may know without this circuit" (a sponge state after an absorbed block, a Merkle node): a Prover remembers the
    // variable as a candidate CHECKPOINT of a circuit template (bpg_witness_checkpoints); to everybody else it is nothing.  It adds no multiplier, no
    // constraint and no transcript byte.
    virtual void note_value(const LinearCombination &lc, uint32_t tag) { (void)lc; (void)tag; }
    // x * var as a variable (Variable::Gated): x a public input of the assembly, var a multiplier variable or a committed value.  A Prover and a Verifier keep
    // a gate table; a recording buffer has none and refuses
    virtual Variable gate(const Variable &x, const Variable &var) { (void)x; (void)var; throw std::invalid_argument("gate: this constraint system keeps no gate table (gates belong to a prover or a verifier)"); }
};

// Flattened instance handed to the engine / exported for the oracle (layout of include/bpg.h bpg_r1cs_upload)
struct FlatCircuit {
    uint64_t n = 0, m = 0;
    std::vector<uint8_t> aL, aR, aO;             // n*32 each (empty on the verifier side)
    std::vector<uint64_t> row_ptr{0};
    std::vector<uint32_t> term_var, term_coef;
    std::vector<uint8_t> coef;                   // ncoef*32, deduplicated coefficient table
};

// non-owning view of the same (what crosses the C ABI: bpg_r1cs_instance); witness pointers may be null on the verifier side
struct FlatView {
    uint64_t n = 0, m = 0, q = 0, nnz = 0, ncoef = 0;
    const uint8_t *aL = nullptr, *aR = nullptr, *aO = nullptr;
    const uint64_t *row_ptr = nullptr;
    const uint32_t *term_var = nullptr, *term_coef = nullptr;
    const uint8_t *coef = nullptr;
    FlatView() {}
    explicit FlatView(const FlatCircuit &f)
        : n(f.n), m(f.m), q(f.row_ptr.size() - 1), nnz(f.term_var.size()), ncoef(f.coef.size() / 32),
          aL(f.aL.empty() ? nullptr : f.aL.data()), aR(f.aR.empty() ? nullptr : f.aR.data()), aO(f.aO.empty() ? nullptr : f.aO.data()),
          row_ptr(f.row_ptr.data()), term_var(f.term_var.data()), term_coef(f.term_coef.data()), coef(f.coef.data()) {}
};

// Witness program of a circuit whose every multiplier came from multiply(left, right) (include/bpg.h bpg_witness_program): multiplier i has
// left = terms [lc_ptr[2i], lc_ptr[2i+1]) and right = terms [lc_ptr[2i+1], lc_ptr[2i+2]); a term is (packed variable, index into the instance's coefficient table)
// and may name committed values, the constant One and multipliers BELOW i only.  param_rows: constraint rows whose constant term is assigned per witness.
// Hints (bpg_witness_hints): multiplier hint_mul[k] (strictly ascending) is no product of two linear combinations; its left list is the SOURCE of the hint,
// its right list is empty, and hint_kind / hint_arg say what to take from the source's value (WITNESS_HINT_BIT_PAIR: a_L = 1 - b, a_R = b, b = bit arg).
constexpr uint32_t WITNESS_HINT_BIT_PAIR = 1;
struct WitnessProgram {
    std::vector<uint64_t> lc_ptr{0};
    std::vector<uint32_t> term_var, term_coef;
    std::vector<uint64_t> param_rows;
    std::vector<uint32_t> hint_mul, hint_kind, hint_arg;
};
struct WitnessProgramView {
    const uint64_t *lc_ptr = nullptr;
    const uint32_t *term_var = nullptr, *term_coef = nullptr;
    uint64_t n_params = 0;
    const uint64_t *param_rows = nullptr;
    uint64_t n_hints = 0;
    const uint32_t *hint_mul = nullptr, *hint_kind = nullptr, *hint_arg = nullptr;
    // Checkpoints (bpg_witness_checkpoints): ck_var[k] is a multiplier variable (kind 0..2, index < n, each named once) whose value the caller hands to
    // assign; every term that names it reads the caller's value (host/template.hpp), and the device compares it with what the circuit computed
    uint64_t n_ck = 0;
    const uint32_t *ck_var = nullptr;
    // Public inputs (bpg_r1cs_upload_template_inputs): terms of kind Variable::Input name inputs [0, n_inputs); 0: the program may hold no such term
    uint64_t n_inputs = 0;
    // Gates (bpg_r1cs_upload_template_gated): a term of kind Variable::Gated names gate k < n_gates, the product of input gate_input[k] and the variable
    // gate_var[k] (kind 0..3); the ROWS of the instance name the same table.  0: neither may hold such a term
    uint64_t n_gates = 0;
    const uint32_t *gate_var = nullptr, *gate_input = nullptr;
    WitnessProgramView() {}
    explicit WitnessProgramView(const WitnessProgram &w)
        : lc_ptr(w.lc_ptr.data()), term_var(w.term_var.data()), term_coef(w.term_coef.data()), n_params(w.param_rows.size()), param_rows(w.param_rows.data()),
          n_hints(w.hint_mul.size()), hint_mul(w.hint_mul.data()), hint_kind(w.hint_kind.data()), hint_arg(w.hint_arg.data()) {}
};

// Shared bookkeeping of Prover and Verifier: constraint rows with a coefficient dictionary.
class CircuitCore {
protected:
    struct KeyHash { size_t operator()(const Scalar &s) const { return (size_t)(s.w[0] * 0x9e3779b97f4a7c15ULL ^ s.w[1] ^ (s.w[2] << 1) ^ (s.w[3] >> 3)); } };
    std::vector<uint64_t> row_ptr_{0};
    std::vector<uint32_t> term_var_, term_coef_;
    std::vector<Scalar> coef_;
    std::unordered_map<Scalar, uint32_t, KeyHash> coef_index_;
    std::pair<Scalar, uint32_t> last_[2] = {{Scalar(), UINT32_MAX}, {Scalar(), UINT32_MAX}};
    // index of a coefficient in the dictionary (appended when new)
    uint32_t intern(const Scalar &s) {
        Scalar c = s.is_canonical() ? s : s.reduced();
        uint32_t id;
        if (last_[0].second != UINT32_MAX && c == last_[0].first) id = last_[0].second;           // two-entry memo in front of the hash map
        else if (last_[1].second != UINT32_MAX && c == last_[1].first) { id = last_[1].second; std::swap(last_[0], last_[1]); }
        else {
            auto it = coef_index_.find(c);
            if (it == coef_index_.end()) { id = (uint32_t)coef_.size(); coef_.push_back(c); coef_index_.emplace(c, id); } else id = it->second;
            last_[1] = last_[0]; last_[0] = {c, id};
        }
        return id;
    }
    void push_row(const LinearCombination &lc) {
        for (auto &t : lc.terms) { term_var_.push_back(t.first.packed()); term_coef_.push_back(intern(t.second)); }
        row_ptr_.push_back(term_var_.size());
    }
    // Public inputs (Variable::Input): the values of this assembly, in the order input() made them
    std::vector<Scalar> inputs_;
    // resolve (every export but a template's): a term (Input p, c) leaves as the constant term (One, c * x_p), its product in the table behind the
    // dictionary's own entries - so nothing that reads an instance ever meets an input, and an assembly without inputs exports what it always did
    void export_rows(FlatCircuit &f, bool resolve = true) const {
        f.row_ptr = row_ptr_; f.term_var = term_var_; f.term_coef = term_coef_;
        f.coef.resize(coef_.size() * 32);
        for (size_t i = 0; i < coef_.size(); i++) coef_[i].to_bytes(&f.coef[32 * i]);
        if (inputs_.empty()) {
            for (uint32_t v : f.term_var) if ((v >> 29) == Variable::Input) throw std::invalid_argument("a constraint names public input " + std::to_string(v & 0x1fffffffu) + ", and this assembly has made none");
                                          else if ((v >> 29) == Variable::Gated) throw std::invalid_argument("a constraint names gate " + std::to_string(v & 0x1fffffffu) + ", and this assembly has made none");
            return;
        }
        std::unordered_map<Scalar, uint32_t, KeyHash> derived;
        for (size_t k = 0; k < f.term_var.size(); k++) {
            const uint32_t kind = f.term_var[k] >> 29;
            if (kind != Variable::Input && kind != Variable::Gated) continue;
            uint32_t p = f.term_var[k] & 0x1fffffffu, to = Variable::one().packed();
            if (kind == Variable::Gated) {          // (gate g, c) leaves as (var_g, c * x_p): the same products, the same table
                if (p >= gates_.size()) throw std::invalid_argument("a constraint names gate " + std::to_string(p) + " of " + std::to_string(gates_.size()));
                to = gates_[p].first; p = gates_[p].second;
            }
            if (p >= inputs_.size()) throw std::invalid_argument("a constraint names public input " + std::to_string(p) + " of " + std::to_string(inputs_.size()));
            if (!resolve) continue;
            const Scalar c = coef_[f.term_coef[k]] * inputs_[p];
            uint32_t id;
            const auto own = coef_index_.find(c);
            if (own != coef_index_.end()) id = own->second;
            else {
                const auto it = derived.find(c);
                if (it != derived.end()) id = it->second;
                else { id = (uint32_t)(f.coef.size() / 32); f.coef.resize(f.coef.size() + 32); c.to_bytes(&f.coef[32 * (size_t)id]); derived.emplace(c, id); }
            }
            f.term_var[k] = to; f.term_coef[k] = id;
        }
    }
    // Gates (Variable::Gated): (packed variable of kind 0..3, input index) per gate, in the order gate() made them
    std::vector<std::pair<uint32_t, uint32_t>> gates_;
    // n_mul, n_committed: what the assembly has allocated so far (a gate names what exists)
    Variable make_gate(const Variable &x, const Variable &var, size_t n_mul, size_t n_committed) {
        if (x.kind != Variable::Input) throw std::invalid_argument("gate: x is no public input (kind " + std::to_string((uint32_t)x.kind) + "; a gate is input * variable)");
        if (x.idx >= inputs_.size()) throw std::invalid_argument("gate: x names public input " + std::to_string(x.idx) + " of " + std::to_string(inputs_.size()) + " (an input of another assembly?)");
        if (var.kind > Variable::Committed)
            throw std::invalid_argument(std::string("gate: the gated variable is ") + (var.kind == Variable::One ? "the constant One (name the input itself)" : var.kind == Variable::Input ? "a public input (a product of two inputs is no linear term)" :
                                        var.kind == Variable::Gated ? "a gate (gates do not nest)" : "of an unknown kind") + "; a gate takes a multiplier variable or a committed value");
        if (var.kind == Variable::Committed ? var.idx >= n_committed : var.idx >= n_mul)
            throw std::invalid_argument("gate: the gated variable's index " + std::to_string(var.idx) + " is out of range (" + std::to_string(var.kind == Variable::Committed ? n_committed : n_mul) + " allocated)");
        if (gates_.size() >= 0x1fffffffu) throw std::invalid_argument("gate: too many gates");
        gates_.emplace_back(var.packed(), x.idx);
        return Variable{Variable::Gated, (uint32_t)(gates_.size() - 1)};
    }
public:
    size_t num_constraints() const { return row_ptr_.size() - 1; }
    // A public input of this proof: a scalar prover and verifier both know, named in linear combinations like any variable.  To the proof it is the constant
    // c * x wherever a term (input, c) stands; a circuit template keeps the term and takes x with every assign (include/bpg.h bpg_prover_input).
    Variable input(const Scalar &x) {
        if (inputs_.size() >= 0x1fffffffu) throw std::invalid_argument("input: too many public inputs");
        inputs_.push_back(x.is_canonical() ? x : x.reduced());
        return Variable{Variable::Input, (uint32_t)(inputs_.size() - 1)};
    }
    const std::vector<Scalar> &inputs() const { return inputs_; }
    const std::vector<std::pair<uint32_t, uint32_t>> &gates() const { return gates_; }
};

class Engine;   // engine.hip

class Prover : public ConstraintSystem, public CircuitCore {
public:
    // Prover::new(&pc_gens, &mut transcript): the transcript is borrowed for the prover's lifetime
    Prover(Engine *engine, Transcript *transcript) : engine_(engine), t_(transcript) { t_->r1cs_domain_sep(); }

    // Prover::commit(v, v_blinding) -> (CompressedRistretto, Variable)
    std::pair<std::vector<uint8_t>, Variable> commit(const Scalar &v, const Scalar &v_blinding);
    // batched form of the same call sequence (identical transcript effect, one kernel launch)
    std::vector<Variable> commit_many(const std::vector<Scalar> &v, const std::vector<Scalar> &blind, std::vector<uint8_t> &coms_out);
    // the same for a commitment computed by the caller (no device context needed): registers the variable, appends "V"
    Variable commit_precomputed(const Scalar &v, const Scalar &v_blinding, const uint8_t com[32]);
    // extension (include/bpg.h bpg_prover_defer_commitments): while on, commit / commit_many register their variables and return zero bytes;
    // flush_commitments() makes every pending commitment in ONE kernel launch and appends them to the transcript in the order they were made -
    // the transcript of the per-call path.  prove(), start_blinding() and commit_precomputed() flush first.
    void defer_commitments(bool on) { if (!on) flush_commitments(); deferred_ = on; }
    void flush_commitments();
    // TEST HOOK (include/bpg.h bpg_test_prover_stub_commitments): commitments become 32 hash bytes of (v, blinding) made on the host - NOT group
    // elements - so that the file drivers' parsers and the gadget assembly can be fuzzed under sanitizers without a device; prove() stays refused
    void test_stub_commitments() {
        if (engine_) throw std::invalid_argument("stub commitments are for device-less provers only (a prover with an engine makes real Pedersen commitments)");
        stub_commitments_ = true;
    }
    size_t num_flushed() const { return flushed_; }
    const uint8_t *commitment(size_t i) const { return &V_[32 * i]; }

    MulVars multiply(LinearCombination left, LinearCombination right) override {
        Scalar l = eval(left), r = eval(right), o = l * r;
        uint32_t i = (uint32_t)aL_.size();
        MulVars mv{{Variable::MultiplierLeft, i}, {Variable::MultiplierRight, i}, {Variable::MultiplierOutput, i}};
        aL_.push_back(l); aR_.push_back(r); aO_.push_back(o);
        made_by_.push_back(num_constraints());
        left.terms.emplace_back(mv.l, -Scalar::one());
        right.terms.emplace_back(mv.r, -Scalar::one());
        constrain(left); constrain(right);
        return mv;
    }
    Variable allocate(const OptScalar &a) override {
        if (!a.some) throw R1CSException(R1CSError::MissingAssignment, "missing assignment");
        if (pending_ < 0) {
            uint32_t i = (uint32_t)aL_.size(); pending_ = i;
            aL_.push_back(a.v); aR_.push_back(Scalar::zero()); aO_.push_back(Scalar::zero());
            made_by_.push_back(FREE_MULTIPLIER);
            return Variable{Variable::MultiplierLeft, i};
        }
        uint32_t i = (uint32_t)pending_; pending_ = -1;
        aR_[i] = a.v; aO_[i] = aL_[i] * aR_[i];
        return Variable{Variable::MultiplierRight, i};
    }
    MulVars allocate_multiplier(bool some, const Scalar &l, const Scalar &r) override {
        if (!some) throw R1CSException(R1CSError::MissingAssignment, "missing assignment");
        uint32_t i = (uint32_t)aL_.size();
        aL_.push_back(l); aR_.push_back(r); aO_.push_back(l * r);
        made_by_.push_back(FREE_MULTIPLIER);
        return MulVars{{Variable::MultiplierLeft, i}, {Variable::MultiplierRight, i}, {Variable::MultiplierOutput, i}};
    }
    // the base multiplier, plus the record of its source: the terms are kept as given and enter the coefficient dictionary only when the instance or the
    // program is exported (resolve_hints) - a range proof constrains its source afterwards, so its coefficients are in the dictionary by then and neither the
    // table nor its order differs from an assembly that records nothing
    MulVars allocate_bit(const LinearCombination &source, uint32_t bit, const OptScalar &source_assignment) override {
        const MulVars mv = ConstraintSystem::allocate_bit(source, bit, source_assignment);
        Hint h; h.bit = bit;
        bool same = !hints_.empty() && hints_.back().t1 - hints_.back().t0 == source.terms.size();
        for (size_t k = 0; same && k < source.terms.size(); k++)
            same = hint_terms_[hints_.back().t0 + k].first.packed() == source.terms[k].first.packed() && hint_terms_[hints_.back().t0 + k].second == source.terms[k].second;
        if (same) { h.t0 = hints_.back().t0; h.t1 = hints_.back().t1; }         // the bits of one range share one copy of their source
        else { h.t0 = hint_terms_.size(); hint_terms_.insert(hint_terms_.end(), source.terms.begin(), source.terms.end()); h.t1 = hint_terms_.size(); }
        made_by_.back() = HINT_MULTIPLIER | hints_.size();
        hints_.push_back(h);
        return mv;
    }
    void constrain(const LinearCombination &lc) override { push_row(lc); }
    // recorded when lc is exactly ONE multiplier variable with coefficient one plus constants that sum to zero (a sponge state is `cube.o + 0`); else ignored
    // (a committed term or a public input beside it: ignored - the value is then no multiplier's own)
    void note_value(const LinearCombination &lc, uint32_t tag) override {
        const Variable *var = nullptr;
        Scalar constant;
        for (auto &t : lc.terms) {
            if (t.first.kind == Variable::One) { constant += t.second; continue; }
            if (var || t.first.kind > Variable::MultiplierOutput || !(red(t.second) == Scalar::one())) return;
            var = &t.first;
        }
        if (!var || !(red(constant) == Scalar::zero())) return;
        noted_var_.push_back(var->packed()); noted_tag_.push_back(tag);
    }
    const std::vector<uint32_t> &noted_vars() const { return noted_var_; }
    const std::vector<uint32_t> &noted_tags() const { return noted_tag_; }

    size_t get_num_multiplications() const { return aL_.size(); }
    size_t num_committed() const { return v_.size(); }
    const std::vector<Scalar> &v() const { return v_; }
    const std::vector<Scalar> &v_blinding() const { return vb_; }
    Transcript *transcript() { return t_; }

    // g = gate(x, var): the variable whose value is x * var - x a public input of this prover, var a multiplier variable or a committed value.  Named in
    // linear combinations like any variable; a resolved export shows (var, c * x), a template keeps the term and takes x with every assign
    Variable gate(const Variable &x, const Variable &var) override { return make_gate(x, var, aL_.size(), v_.size()); }

    Scalar eval(const LinearCombination &lc) const {
        Scalar acc;
        for (auto &t : lc.terms) {
            if (t.first.kind == Variable::One) { acc += t.second; continue; }     // a constant term: c * 1 (round constants, keys) without the product
            static const Scalar ONE = Scalar::one();
            if (t.first.kind == Variable::Gated) {                                  // c * x_p * value
                if (t.first.idx >= gates_.size()) throw std::invalid_argument("linear combination refers to a gate this prover has not made");
                const auto &g = gates_[t.first.idx];
                acc += t.second * inputs_[g.second] * value_of(Variable::unpack(g.first));
                continue;
            }
            const Scalar *x = &value_of(t.first);
            static const Scalar MINUS_ONE = -Scalar::one();
            if (t.second == ONE) acc += *x;                          // most coefficients of the gadgets are +-1: skip the multiplication
            else if (t.second == MINUS_ONE) acc -= *x;
            else acc += t.second * *x;
        }
        return acc;
    }
    // a stale or foreign variable (another prover's, a packed value from the C ABI) must not index past the vectors: dalek panics here
    const Scalar &value_of(const Variable &var) const {
        const size_t idx = var.idx;
        switch (var.kind) {
        case Variable::MultiplierLeft: if (idx >= aL_.size()) throw std::invalid_argument("linear combination refers to an unallocated multiplier"); return aL_[idx];
        case Variable::MultiplierRight: if (idx >= aR_.size()) throw std::invalid_argument("linear combination refers to an unallocated multiplier"); return aR_[idx];
        case Variable::MultiplierOutput: if (idx >= aO_.size()) throw std::invalid_argument("linear combination refers to an unallocated multiplier"); return aO_[idx];
        case Variable::Committed: if (idx >= v_.size()) throw std::invalid_argument("linear combination refers to an uncommitted variable"); return v_[idx];
        case Variable::Input: if (idx >= inputs_.size()) throw std::invalid_argument("linear combination refers to a public input this prover has not made"); return inputs_[idx];
        default: throw std::invalid_argument("linear combination holds an unknown variable kind");
        }
    }

    // keep_inputs (bpg_prover_template_instance): the rows keep their input terms, for a template; else they leave as constants (export_rows)
    FlatCircuit flatten(bool keep_inputs = false) {
        resolve_hints();
        FlatCircuit f; f.n = aL_.size(); f.m = v_.size();
        f.aL.resize(f.n * 32); f.aR.resize(f.n * 32); f.aO.resize(f.n * 32);
        for (size_t i = 0; i < f.n; i++) { red(aL_[i]).to_bytes(&f.aL[32 * i]); red(aR_[i]).to_bytes(&f.aR[32 * i]); red(aO_[i]).to_bytes(&f.aO[32 * i]); }
        export_rows(f, !keep_inputs);
        return f;
    }

    // The witness program (include/bpg.h bpg_witness_program): how each multiplier's assignment follows from earlier variables.  Recording is ALWAYS ON and costs
    // one 8-byte push per multiplier: multiply() notes the constraint row it is about to make (its two rows ARE the program: left - a_L[i], right - a_R[i], so
    // the linear combinations as they were before those terms are the rows without their last term); allocate() / allocate_multiplier() note a free multiplier,
    // whose assignment is no function of linear combinations.  Nothing the prover exports today (instance, transcript, proof) reads the record.
    // Throws std::invalid_argument when the circuit has a free multiplier or none at all.
    // with_hints (bpg_prover_witness_program_hinted): a multiplier made by allocate_bit is exported as a hint - its left list is the source, its right list
    // empty; without, it is refused like any free multiplier.
    WitnessProgram witness_program(bool with_hints = false) {
        if (aL_.empty()) throw std::invalid_argument("witness program: the circuit has no multipliers");
        if (with_hints) resolve_hints();
        WitnessProgram w;
        w.lc_ptr.reserve(2 * aL_.size() + 1);
        for (size_t i = 0; i < made_by_.size(); i++) {
            if (made_by_[i] == FREE_MULTIPLIER || (!with_hints && (made_by_[i] & HINT_MULTIPLIER)))
                throw std::invalid_argument("witness program: multiplier " + std::to_string(i) + " is a free multiplier (allocate / allocate_multiplier: its assignment is a hint, not a function of linear combinations)");
            if (made_by_[i] & HINT_MULTIPLIER) {
                const Hint &h = hints_[made_by_[i] & ~HINT_MULTIPLIER];
                for (uint64_t k = h.t0; k < h.t1; k++) { w.term_var.push_back(hint_terms_[k].first.packed()); w.term_coef.push_back(hint_coef_[k]); }
                w.lc_ptr.push_back(w.term_var.size()); w.lc_ptr.push_back(w.term_var.size());
                w.hint_mul.push_back((uint32_t)i); w.hint_kind.push_back(WITNESS_HINT_BIT_PAIR); w.hint_arg.push_back(h.bit);
                continue;
            }
            for (uint64_t r = made_by_[i]; r < made_by_[i] + 2; r++) {
                w.term_var.insert(w.term_var.end(), term_var_.begin() + row_ptr_[r], term_var_.begin() + row_ptr_[r + 1] - 1);
                w.term_coef.insert(w.term_coef.end(), term_coef_.begin() + row_ptr_[r], term_coef_.begin() + row_ptr_[r + 1] - 1);
                w.lc_ptr.push_back(w.term_var.size());
            }
        }
        w.param_rows = param_rows_;
        return w;
    }
    // the constant term of constraint row `row` is assigned per witness (bpg_r1cs_assign); the row a constrain() call made is num_constraints() - 1 right after it
    void mark_param_row(uint64_t row) {
        if (row >= num_constraints()) throw std::invalid_argument("mark_param_row: no such constraint row");
        if (std::find(param_rows_.begin(), param_rows_.end(), row) != param_rows_.end()) throw std::invalid_argument("mark_param_row: the row is marked already");
        param_rows_.push_back(row);
    }

    // Prover::prove(&bp_gens) -> R1CSProof::to_bytes(). rng_seed replaces thread_rng() (32 external bytes).
    std::vector<uint8_t> prove(uint64_t gens_capacity, const uint8_t rng_seed[32], uint32_t flags);
    // extension: start drawing prove()'s blinding scalars now (all commitments made), while the constraints are still being assembled
    void start_blinding(const uint8_t rng_seed[32], uint64_t max_multipliers);

private:
    static Scalar red(const Scalar &s) { return s.is_canonical() ? s : s.reduced(); }
    Engine *engine_;
    Transcript *t_;
    std::vector<Scalar> aL_, aR_, aO_, v_, vb_;
    std::vector<uint8_t> V_;            // the commitments, 32 bytes each (zero until flushed)
    bool deferred_ = false; size_t flushed_ = 0;
    bool stub_commitments_ = false;
    int64_t pending_ = -1;
    static constexpr uint64_t FREE_MULTIPLIER = ~0ull, HINT_MULTIPLIER = 1ull << 63;
    std::vector<uint64_t> made_by_;     // per multiplier: the first of the two constraint rows multiply() made for it, FREE_MULTIPLIER, or HINT_MULTIPLIER | index into hints_
    struct Hint { uint32_t bit; uint64_t t0, t1; };                     // allocate_bit: bit `bit` of the source hint_terms_[t0, t1)
    std::vector<Hint> hints_;
    std::vector<std::pair<Variable, Scalar>> hint_terms_;
    std::vector<uint32_t> hint_coef_;   // dictionary index per hint term, filled by resolve_hints
    void resolve_hints() { while (hint_coef_.size() < hint_terms_.size()) hint_coef_.push_back(intern(hint_terms_[hint_coef_.size()].second)); }
    std::vector<uint64_t> param_rows_;
    std::vector<uint32_t> noted_var_, noted_tag_;     // note_value: packed variable and the caller's tag, in call order
};

class Verifier : public ConstraintSystem, public CircuitCore {
public:
    explicit Verifier(Transcript *transcript) : t_(transcript) { t_->r1cs_domain_sep(); }
    // Verifier::commit(CompressedRistretto) -> Variable
    Variable commit(const uint8_t com[32]) {
        uint32_t i = (uint32_t)(V_.size() / 32);
        V_.insert(V_.end(), com, com + 32);
        t_->append_point("V", com);
        return Variable{Variable::Committed, i};
    }
    MulVars multiply(LinearCombination left, LinearCombination right) override {
        uint32_t i = (uint32_t)num_vars_++;
        MulVars mv{{Variable::MultiplierLeft, i}, {Variable::MultiplierRight, i}, {Variable::MultiplierOutput, i}};
        left.terms.emplace_back(mv.l, -Scalar::one());
        right.terms.emplace_back(mv.r, -Scalar::one());
        constrain(left); constrain(right);
        return mv;
    }
    Variable allocate(const OptScalar &) override {
        if (pending_ < 0) { pending_ = (int64_t)num_vars_++; return Variable{Variable::MultiplierLeft, (uint32_t)pending_}; }
        uint32_t i = (uint32_t)pending_; pending_ = -1; return Variable{Variable::MultiplierRight, i};
    }
    MulVars allocate_multiplier(bool, const Scalar &, const Scalar &) override {
        uint32_t i = (uint32_t)num_vars_++;
        return MulVars{{Variable::MultiplierLeft, i}, {Variable::MultiplierRight, i}, {Variable::MultiplierOutput, i}};
    }
    void constrain(const LinearCombination &lc) override { push_row(lc); }
    // the verifier's side of Prover::gate: the same gates in the same order
    Variable gate(const Variable &x, const Variable &var) override { return make_gate(x, var, num_vars_, V_.size() / 32); }
    size_t get_num_vars() const { return num_vars_; }
    const std::vector<uint8_t> &commitments() const { return V_; }
    Transcript *transcript() { return t_; }
    FlatCircuit flatten() const { FlatCircuit f; f.n = num_vars_; f.m = V_.size() / 32; export_rows(f); return f; }
private:
    Transcript *t_;
    std::vector<uint8_t> V_;
    size_t num_vars_ = 0;
    int64_t pending_ = -1;
};

}  // namespace bpg
