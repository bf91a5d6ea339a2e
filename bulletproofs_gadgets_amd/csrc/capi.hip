// extern "C" surface declared in include/bpg.h.  Translates C handles to the C++ host mirror (host/*.hpp) and the
// HIP engine (engine.hip); every exception is mapped to a bpg_status and a thread-local message.
#include <algorithm>
#include <chrono>
#include <atomic>
#include <cstring>
#include <thread>
#include <memory>
#include <string>
#include "../../include/bpg.h"
#include "engine.hpp"
#include "host/gadgets.hpp"

using namespace bpg;

// ---------------------------------------------------------------------------------------- pieces of the host mirror
namespace bpg {

const std::vector<Scalar> &mimc_round_constants() {
    static const uint64_t RC[486][4] = {
#include "host/mimc_rc769.inc"
    };
    static const std::vector<Scalar> v = [] {
        std::vector<Scalar> out(486);
        for (int i = 0; i < 486; i++) out[i] = Scalar::from_bits(reinterpret_cast<const uint8_t *>(RC[i]));   // Scalar::from_bits(*constant), mimc.rs:69-71
        return out;
    }();
    return v;
}

std::pair<std::vector<uint8_t>, Variable> Prover::commit(const Scalar &v, const Scalar &v_blinding) {
    std::vector<uint8_t> com;
    std::vector<Variable> vars = commit_many({v}, {v_blinding}, com);
    return {com, vars[0]};
}

std::vector<Variable> Prover::commit_many(const std::vector<Scalar> &v, const std::vector<Scalar> &blind, std::vector<uint8_t> &coms_out) {
    if (v.size() != blind.size()) throw std::invalid_argument("commit_many: size mismatch");
    const size_t k = v.size();
    coms_out.assign(k * 32, 0);
    std::vector<Variable> vars;
    if (!k) return vars;
    if (!engine_ && !stub_commitments_) throw DeviceError("this prover has no device context: Pedersen commitments need the GPU engine");
    for (size_t i = 0; i < k; i++) {
        const uint32_t idx = (uint32_t)v_.size();
        v_.push_back(v[i]); vb_.push_back(blind[i].is_canonical() ? blind[i] : blind[i].reduced());
        vars.push_back(Variable{Variable::Committed, idx});
    }
    V_.resize(v_.size() * 32, 0);
    if (!deferred_) {
        const size_t before = v_.size() - k;
        try { flush_commitments(); }
        catch (...) { if (flushed_ <= before) { v_.resize(before); vb_.resize(before); V_.resize(before * 32); } throw; }     // a failed call registers nothing
        std::memcpy(coms_out.data(), &V_[32 * before], k * 32);
    }
    return vars;
}

// every commitment registered since the last flush: one k_pedersen launch, then the "V" appends in order (the per-call path's transcript)
void Prover::flush_commitments() {
    const size_t k = v_.size() - flushed_;
    if (!k) return;
    if (!engine_ && !stub_commitments_) throw DeviceError("this prover has no device context: Pedersen commitments need the GPU engine");
    std::vector<uint8_t> vb(k * 32), bb(k * 32);
    for (size_t i = 0; i < k; i++) { v_[flushed_ + i].to_bytes(&vb[32 * i]); vb_[flushed_ + i].to_bytes(&bb[32 * i]); }
    V_.resize(v_.size() * 32, 0);
    if (stub_commitments_) {      // test hook: hash bytes in place of group elements (sanitizer fuzzing of the drivers without a device)
        for (size_t i = 0; i < k; i++) {
            Shake256 sh; sh.absorb(reinterpret_cast<const uint8_t *>("bpg stub commitment"), 19); sh.absorb(&vb[32 * i], 32); sh.absorb(&bb[32 * i], 32);
            sh.squeeze(&V_[32 * (flushed_ + i)], 32);
        }
    } else
    engine_->pedersen_commit(k, vb.data(), bb.data(), &V_[32 * flushed_]);
    for (size_t i = 0; i < k; i++) t_->append_point("V", &V_[32 * (flushed_ + i)]);
    flushed_ = v_.size();
}

Variable Prover::commit_precomputed(const Scalar &v, const Scalar &v_blinding, const uint8_t com[32]) {
    flush_commitments();
    const uint32_t idx = (uint32_t)v_.size();
    v_.push_back(v); vb_.push_back(v_blinding.is_canonical() ? v_blinding : v_blinding.reduced());
    V_.insert(V_.end(), com, com + 32);
    t_->append_point("V", com);
    flushed_ = v_.size();
    return Variable{Variable::Committed, idx};
}

std::vector<uint8_t> Prover::prove(uint64_t gens_capacity, const uint8_t rng_seed[32], uint32_t flags) {
    if (!engine_) throw DeviceError("this prover has no device context: prove() needs the GPU engine");
    if (stub_commitments_) throw DeviceError("this prover holds stub (hash) commitments: prove() is refused");      // (test hook; cannot be set on a prover with an engine)
    flush_commitments();
    engine_->gens_ensure(gens_capacity);
    require_gens_capacity(gens_capacity, aL_.size());
    FlatCircuit f = flatten();
    DeviceCircuit *dc = engine_->upload(f);
    try {
        std::vector<uint8_t> proof = engine_->prove(dc, *t_, vb_, rng_seed, flags, nullptr);
        engine_->free_circuit(dc);
        return proof;
    } catch (...) { engine_->free_circuit(dc); throw; }
}

void Prover::start_blinding(const uint8_t rng_seed[32], uint64_t max_multipliers) {
    if (!engine_) throw DeviceError("this prover has no device context: start_blinding() needs the GPU engine");
    flush_commitments();
    engine_->blinding_begin(*t_, vb_, rng_seed, max_multipliers);
}

}  // namespace bpg

// ---------------------------------------------------------------------------------------- handles
struct bpg_ctx { Engine *engine; };
struct bpg_merkle { DeviceMerkle *t; };
struct bpg_circuit { DeviceCircuit *dc; uint64_t n, m; bool is_template = false; uint64_t n_params = 0; uint64_t n_ck = 0; uint64_t n_in = 0; uint64_t n_gates = 0; };     // dc == nullptr: bpg_test_circuit_handle
struct bpg_transcript { Transcript t; };
struct bpg_prover { Prover *p; FlatCircuit flat; std::vector<uint8_t> v_bytes, vb_bytes, in_bytes; WitnessProgram program; std::vector<uint32_t> gate_var, gate_input; };
struct bpg_verifier { Verifier *v; FlatCircuit flat; };
struct bpg_gadget { std::unique_ptr<Gadget> g; };
struct bpg_buffer { OpBuffer b; };

static thread_local std::string g_last_error;

template <class F> static bpg_status guard(F &&f) {
    try { f(); g_last_error.clear(); return BPG_OK; }
    catch (const R1CSException &e) { g_last_error = e.what(); return (bpg_status)e.code; }
    catch (const DeviceError &e) { g_last_error = e.what(); return BPG_ERR_DEVICE; }
    catch (const std::invalid_argument &e) { g_last_error = e.what(); return BPG_ERR_INVALID_ARGUMENT; }
    catch (const std::out_of_range &e) { g_last_error = e.what(); return BPG_ERR_INVALID_ARGUMENT; }
    catch (const std::bad_alloc &) { g_last_error = "out of host memory"; return BPG_ERR_INTERNAL; }
    catch (const std::exception &e) { g_last_error = e.what(); return BPG_ERR_INTERNAL; }
    catch (...) { g_last_error = "unknown error"; return BPG_ERR_INTERNAL; }
}
#define REQUIRE(cond) do { if (!(cond)) throw std::invalid_argument("null or invalid argument: " #cond); } while (0)

static LinearCombination lc_from(const bpg_lc *lc) {
    REQUIRE(lc && (lc->n == 0 || lc->terms));
    LinearCombination out;
    for (uint64_t i = 0; i < lc->n; i++) {
        if ((lc->terms[i].var >> 29) > BPG_VAR_GATED) throw std::invalid_argument("linear combination holds an unknown variable kind");
        out.terms.emplace_back(Variable::unpack(lc->terms[i].var), Scalar::from_bits(lc->terms[i].coeff));
    }
    return out;
}
static void view(const FlatCircuit &f, bpg_r1cs_instance *o) {
    o->n = f.n; o->m = f.m; o->q = f.row_ptr.size() - 1; o->nnz = f.term_var.size(); o->ncoef = f.coef.size() / 32;
    o->aL = f.aL.empty() ? nullptr : f.aL.data(); o->aR = f.aR.empty() ? nullptr : f.aR.data(); o->aO = f.aO.empty() ? nullptr : f.aO.data();
    o->row_ptr = f.row_ptr.data(); o->term_var = f.term_var.data(); o->term_coef = f.term_coef.data(); o->coef = f.coef.data();
}
static FlatView as_view(const bpg_r1cs_instance *i, bool need_witness, bool drop_witness = false) {
    REQUIRE(i && i->row_ptr && (i->nnz == 0 || (i->term_var && i->term_coef)) && (i->ncoef == 0 || i->coef));
    const bool has_w = i->aL && i->aR && i->aO;
    REQUIRE(i->n == 0 || has_w || !need_witness);
    FlatView v; v.n = i->n; v.m = i->m; v.q = i->q; v.nnz = i->nnz; v.ncoef = i->ncoef;
    if (has_w && !drop_witness) { v.aL = i->aL; v.aR = i->aR; v.aO = i->aO; }
    v.row_ptr = i->row_ptr; v.term_var = i->term_var; v.term_coef = i->term_coef; v.coef = i->coef;
    return v;
}
extern "C" {

const char *bpg_strerror(bpg_status s) {
    switch (s) {
    case BPG_OK: return "ok";
    case BPG_ERR_INVALID_GENERATORS_LENGTH: return "invalid generators length";
    case BPG_ERR_FORMAT: return "format error";
    case BPG_ERR_VERIFICATION: return "verification error";
    case BPG_ERR_INVALID_ARGUMENT: return "invalid argument";
    case BPG_ERR_MISSING_ASSIGNMENT: return "missing assignment";
    case BPG_ERR_GADGET: return "gadget error";
    case BPG_ERR_DEVICE: return "device error";
    case BPG_ERR_CHECKPOINT_MISMATCH: return "checkpoint mismatch";
    default: return "internal error";
    }
}
const char *bpg_last_error(void) { return g_last_error.c_str(); }
uint32_t bpg_abi_version(void) { return BPG_ABI_VERSION; }

static EngineConfig engine_config(const bpg_config *c) {
    EngineConfig e;
    if (!c) return e;
    // struct_size tells which fields the caller's header knows; the layout only ever grows at the end
    // a field is read when the caller's struct holds ALL of it (offset + size <= struct_size)
    const size_t sz = c->struct_size;
#define BPG_CFG_HAS(field) (sz >= offsetof(bpg_config, field) + sizeof(c->field))
    if (!BPG_CFG_HAS(profile)) throw std::invalid_argument("bpg_config.struct_size not set");
    e.profile = c->profile;
    if (BPG_CFG_HAS(table_budget_gb)) e.table_budget_gb = c->table_budget_gb;
    if (BPG_CFG_HAS(chain_workers)) e.chain_workers = c->chain_workers;
    if (BPG_CFG_HAS(chain_lanes)) e.chain_lanes = c->chain_lanes;
    if (BPG_CFG_HAS(blocking_sync)) e.blocking_sync = c->blocking_sync;
    if (BPG_CFG_HAS(gens_cache_dir) && c->gens_cache_dir) e.gens_cache_dir = c->gens_cache_dir;
#undef BPG_CFG_HAS
    return e;
}
bpg_status bpg_ctx_create_ex(int32_t device, const bpg_config *config, bpg_ctx **out) {
    return guard([&] { REQUIRE(out); *out = nullptr; Engine *e = new Engine(device, engine_config(config)); *out = new bpg_ctx{e}; });
}
bpg_status bpg_ctx_create(int32_t device, bpg_ctx **out) { return bpg_ctx_create_ex(device, nullptr, out); }
int32_t bpg_device_count(void) { return Engine::device_count(); }
bpg_status bpg_test_fail_next_upload(bpg_ctx *ctx) { return guard([&] { REQUIRE(ctx); ctx->engine->test_fail_next_upload(); }); }
bpg_status bpg_test_drop_next_upload(bpg_ctx *ctx) { return guard([&] { REQUIRE(ctx); ctx->engine->test_drop_next_upload(); }); }
bpg_status bpg_test_live_resources(uint64_t out[6]) { return guard([&] { REQUIRE(out); live_resources(out); }); }
uint64_t bpg_table_bytes(bpg_ctx *ctx) { return ctx ? ctx->engine->table_bytes() : 0; }
int32_t bpg_ctx_last_shared_variants(bpg_ctx *ctx) { return ctx && ctx->engine->last_shared_variants() ? 1 : 0; }
void bpg_ctx_destroy(bpg_ctx *ctx) { if (ctx) { delete ctx->engine; delete ctx; } }
bpg_status bpg_pedersen_bases(bpg_ctx *ctx, uint8_t B[32], uint8_t Bb[32]) { return guard([&] { REQUIRE(ctx && B && Bb); ctx->engine->pedersen_bases(B, Bb); }); }
bpg_status bpg_gens_ensure(bpg_ctx *ctx, uint64_t capacity) { return guard([&] { REQUIRE(ctx); ctx->engine->gens_ensure(capacity); }); }
bpg_status bpg_gens_export(bpg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *G, uint8_t *H) {
    return guard([&] { REQUIRE(ctx && (count == 0 || (G && H))); ctx->engine->gens_export(first, count, G, H); });
}
bpg_status bpg_pedersen_commit(bpg_ctx *ctx, uint64_t k, const uint8_t *v, const uint8_t *blind, uint8_t *out) {
    return guard([&] { REQUIRE(ctx && (k == 0 || (v && blind && out))); ctx->engine->pedersen_commit(k, v, blind, out); });
}
bpg_status bpg_test_fe_ops(bpg_ctx *ctx, int32_t op, uint64_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
    return guard([&] { REQUIRE(ctx && op >= 0 && op <= 10 && (n == 0 || (a && b && out))); ctx->engine->test_fe_ops(op, n, a, b, out); });
}
bpg_status bpg_msm_gens(bpg_ctx *ctx, uint64_t first, uint64_t count, const uint8_t *s, const uint8_t *t, uint8_t out[32]) {
    return guard([&] { REQUIRE(ctx && out && (count == 0 || (s && t))); ctx->engine->msm_gens(first, count, s, t, out); });
}
bpg_status bpg_test_msm(bpg_ctx *ctx, uint32_t nmsm, uint32_t nseg, const bpg_msm_seg *segs, const uint8_t *scalars, uint8_t *out,
                        char *evidence, uint64_t cap) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_msm: no device context (the MSM runs on the GPU only)");
        REQUIRE(out && evidence && cap);
        if (nseg > 16) throw std::invalid_argument("test_msm: at most 16 segments");
        if (nseg && !segs) throw std::invalid_argument("test_msm: no segment array");
        std::vector<Engine::MsmSegSpec> sp(nseg);
        for (uint32_t k = 0; k < nseg; k++) sp[k] = {segs[k].table, segs[k].result, segs[k].first, segs[k].len, segs[k].lgblk, segs[k].skip};
        const std::string r = ctx->engine->test_msm(nmsm, nseg, sp.data(), scalars, out);
        if (r.size() + 1 > cap) throw std::invalid_argument("test_msm: evidence buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(evidence, r.c_str(), r.size() + 1);
    });
}

bpg_status bpg_test_fold(bpg_ctx *ctx, int32_t kernel, uint32_t lgMr, uint32_t rounds, uint32_t first, uint64_t n, const uint8_t *sG, const uint8_t *sH,
                         const uint8_t u_ch[32], uint8_t *out, char *evidence, uint64_t cap) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_fold: no device context (the fold runs on the GPU only)");
        REQUIRE(sG && sH && u_ch && out && evidence && cap >= 512);
        const std::string r = ctx->engine->test_fold(kernel, lgMr, rounds, first, n, sG, sH, u_ch, out);
        if (r.size() + 1 > cap) throw std::invalid_argument("test_fold: evidence buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(evidence, r.c_str(), r.size() + 1);
    });
}

bpg_status bpg_test_tail(bpg_ctx *ctx, uint32_t lgM0, uint32_t tables, uint32_t first, uint64_t n, const uint8_t *a, const uint8_t *b, const uint8_t yinv[32],
                         const uint8_t u_ch[32], const uint8_t gamma0[32], const uint8_t eta0[32], const uint8_t w[32], uint32_t rounds, const uint8_t *u,
                         uint8_t *lr_out, uint8_t *ab_out, char *evidence, uint64_t cap) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_tail: no device context (the tail runs on the GPU only)");
        REQUIRE(a && b && yinv && u_ch && gamma0 && eta0 && w && u && lr_out && ab_out && evidence && cap >= 512);
        const std::string r = ctx->engine->test_tail(lgM0, tables, first, n, a, b, yinv, u_ch, gamma0, eta0, w, rounds, u, lr_out, ab_out);
        if (r.size() + 1 > cap) throw std::invalid_argument("test_tail: evidence buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(evidence, r.c_str(), r.size() + 1);
    });
}

bpg_status bpg_test_commit3(bpg_ctx *ctx, uint32_t lgM0, uint64_t n, const uint8_t *aL, const uint8_t *aR, const uint8_t *aO, const uint8_t *sL, const uint8_t *sR,
                            const uint8_t blind[96], uint8_t out[96], char *evidence, uint64_t cap) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_commit3: no device context (the commitments run on the GPU only)");
        REQUIRE(aL && aR && aO && sL && sR && blind && out && evidence && cap >= 512);
        const std::string r = ctx->engine->test_commit3(lgM0, n, aL, aR, aO, sL, sR, blind, out);
        if (r.size() + 1 > cap) throw std::invalid_argument("test_commit3: evidence buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(evidence, r.c_str(), r.size() + 1);
    });
}

bpg_status bpg_test_weights(bpg_ctx *ctx, bpg_circuit *c, const uint8_t z[32], uint8_t *out) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_weights: no device context (the weights are flattened on the GPU only)");
        REQUIRE(c && z && out);
        if (!c->dc) throw std::invalid_argument("test_weights: the handle has no device state (bpg_test_circuit_handle)");
        ctx->engine->test_weights(c->dc, z, out);
    });
}

bpg_status bpg_test_decompress(bpg_ctx *ctx, uint64_t n, const uint8_t *in, uint32_t *ok_out, uint8_t *xy_out) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_decompress: no device context (k_decompress runs on the GPU only)");
        REQUIRE(n == 0 || (in && ok_out && xy_out));
        if (n > (1ull << 24)) throw std::invalid_argument("test_decompress: at most 2^24 encodings");
        ctx->engine->test_decompress(n, in, ok_out, xy_out);
    });
}
bpg_status bpg_test_verify_replay(uint64_t n, uint64_t m, uint64_t gens_capacity, const uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], const uint8_t *proof,
                                  uint64_t proof_len, const uint8_t seed[32], uint32_t flags, bpg_status *status_out, int32_t *decided_out) {
    return guard([&] {
        REQUIRE(ts && seed && status_out && decided_out && (proof_len == 0 || proof));
        if (n > (1ull << 32)) throw std::invalid_argument("test_verify_replay: n above 2^32");
        Transcript T = Transcript::from_state(ts);
        static const uint8_t none = 0;
        const R1CSError e = Engine::test_verify_replay(n, m, gens_capacity, T, proof ? proof : &none, proof_len, seed, flags);
        *status_out = (bpg_status)e; *decided_out = e != R1CSError::None;
    });
}
bpg_status bpg_test_verify_replay_scripted(uint64_t n, uint64_t m, uint64_t gens_capacity, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], const uint8_t *proof,
                                           uint64_t proof_len, const uint8_t seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len,
                                           bpg_status *status_out, uint8_t *challenges_out, uint64_t *consumed_out) {
    return guard([&] {
        REQUIRE(ts && seed && status_out && challenges_out && consumed_out && (proof_len == 0 || proof));
        if (n > (1ull << 32)) throw std::invalid_argument("test_verify_replay_scripted: n above 2^32");
        Transcript T = Transcript::from_state(ts);
        if (script) Engine::script_transcript(T, n, script, script_len);
        std::memset(challenges_out, 0, 32 * (5 + (size_t)ceil_log2(padded_size(n))));
        static const uint8_t none = 0;
        const R1CSError e = Engine::test_verify_replay_scripted(n, m, gens_capacity, T, proof ? proof : &none, proof_len, seed, flags, challenges_out, consumed_out);
        T.export_state(ts);
        *status_out = (bpg_status)e;
    });
}
bpg_status bpg_profile_set(bpg_ctx *ctx, int32_t mode) { return guard([&] { REQUIRE(ctx && mode >= 0 && mode <= 2); ctx->engine->profile_set(mode); }); }
bpg_status bpg_profile_report(bpg_ctx *ctx, char *out, uint64_t cap) {
    return guard([&] { REQUIRE(ctx && out && cap); std::string r = ctx->engine->profile_report(); if (r.size() + 1 > cap) throw std::invalid_argument("profile_report: buffer too small"); std::memcpy(out, r.c_str(), r.size() + 1); });
}
bpg_status bpg_bench_fe_mul(bpg_ctx *ctx, uint32_t iters, double *out) { return guard([&] { REQUIRE(ctx && out && iters); *out = ctx->engine->bench_fe_mul(iters); }); }

uint64_t bpg_proof_size(uint64_t n, uint32_t flags) {
    return ((flags & BPG_FLAG_COMPACT_1PHASE) ? 1 + 11 * 32 : 14 * 32) + (2 * (uint64_t)ceil_log2(n) + 2) * 32;
}

bpg_status bpg_r1cs_upload(bpg_ctx *ctx, const bpg_r1cs_instance *inst, bpg_circuit **out) {
    return guard([&] {
        REQUIRE(ctx && out); *out = nullptr;
        const FlatView f = as_view(inst, true);                  // no host copy: the instance goes to the device as it is
        Engine::check_instance(f);                               // (a public input among its terms: refused here, before the context is touched)
        DeviceCircuit *dc = ctx->engine->upload(f);
        *out = new bpg_circuit{dc, f.n, f.m};
    });
}
void bpg_r1cs_free(bpg_ctx *ctx, bpg_circuit *c) {
    if (!c || (c->dc && !ctx)) return;
    if (c->dc) ctx->engine->free_circuit(c->dc);
    delete c;
}

static WitnessProgramView program_view(const bpg_witness_program *w, const bpg_witness_hints *h = nullptr, const bpg_witness_checkpoints *k = nullptr) {
    REQUIRE(w);
    WitnessProgramView v; v.lc_ptr = w->lc_ptr; v.term_var = w->term_var; v.term_coef = w->term_coef; v.n_params = w->n_params; v.param_rows = w->param_rows;
    if (h) { v.n_hints = h->n_hints; v.hint_mul = h->hint_mul; v.hint_kind = h->hint_kind; v.hint_arg = h->hint_arg; }
    if (k) { v.n_ck = k->n_checkpoints; v.ck_var = k->vars; }
    return v;
}
static WitnessProgramView program_view_inputs(const bpg_witness_program *w, const bpg_witness_hints *h, const bpg_witness_checkpoints *k, uint64_t n_inputs,
                                              const bpg_witness_gates *g);
bpg_status bpg_r1cs_upload_template(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, bpg_circuit **out) {
    return bpg_r1cs_upload_template_hinted(ctx, inst, program, nullptr, out);
}
bpg_status bpg_r1cs_upload_template_hinted(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           bpg_circuit **out) {
    return bpg_r1cs_upload_template_checkpointed(ctx, inst, program, hints, nullptr, out);
}
bpg_status bpg_r1cs_upload_template_checkpointed(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                 const bpg_witness_checkpoints *checkpoints, bpg_circuit **out) {
    return bpg_r1cs_upload_template_inputs(ctx, inst, program, hints, checkpoints, 0, nullptr, out);
}
bpg_status bpg_r1cs_upload_template_inputs(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *input_values, bpg_circuit **out) {
    return bpg_r1cs_upload_template_gated(ctx, inst, program, hints, checkpoints, n_inputs, input_values, nullptr, out);
}
bpg_status bpg_r1cs_upload_template_gated(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *input_values,
                                          const bpg_witness_gates *gates, bpg_circuit **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(ctx && inst && program);
        const FlatView f = as_view(inst, false);
        const WitnessProgramView w = program_view_inputs(program, hints, checkpoints, n_inputs, gates);
        const TemplatePlan plan = Engine::plan_template(f, w, input_values);      // every check, the level cap included, before the context is touched
        DeviceCircuit *dc = ctx->engine->upload_template(f, plan);
        bpg_circuit *c = new bpg_circuit{dc, f.n, f.m}; c->is_template = true; c->n_params = w.n_params; c->n_ck = w.n_ck; c->n_in = n_inputs; c->n_gates = w.n_gates;
        *out = c;
    });
}
// the argument checks the two assign calls share
static void assign_checks(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values) {
    REQUIRE(ctx && c);
    if (!c->is_template) throw std::invalid_argument("assign: the circuit is not a template (bpg_r1cs_upload_template)");
    if (m != c->m) throw std::invalid_argument("assign: m does not match the template");
    if (n_params != c->n_params) throw std::invalid_argument("assign: n_params does not match the template");
    REQUIRE((m == 0 || v) && (n_params == 0 || param_values));
}
bpg_status bpg_r1cs_assign(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values) {
    return guard([&] {
        assign_checks(ctx, c, m, v, n_params, param_values);
        if (c->n_in) throw std::invalid_argument("assign: the template has public inputs and needs their values (bpg_r1cs_assign_inputs)");
        if (c->n_ck) throw std::invalid_argument("assign: the template was uploaded with checkpoints and needs their values (bpg_r1cs_assign_checkpointed)");
        if (!c->dc) throw std::invalid_argument("assign: the handle has no device state (bpg_test_circuit_handle)");
        ctx->engine->assign(c->dc, v, param_values);
    });
}
bpg_status bpg_r1cs_assign_checkpointed(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values,
                                        uint64_t n_ck, const uint8_t *ck_values, uint64_t *first_mismatch) {
    if (c && c->is_template && c->n_in) {       // its arguments carry no input values: refused as plain assign refuses a checkpointed template
        if (first_mismatch) *first_mismatch = UINT64_MAX;
        return guard([&] { throw std::invalid_argument("assign: the template has public inputs and needs their values (bpg_r1cs_assign_inputs)"); });
    }
    return bpg_r1cs_assign_inputs(ctx, c, m, v, n_params, param_values, n_ck, ck_values, first_mismatch, 0, nullptr);
}
bpg_status bpg_r1cs_assign_inputs(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values,
                                  uint64_t n_ck, const uint8_t *ck_values, uint64_t *first_mismatch, uint64_t n_inputs, const uint8_t *input_values) {
    if (first_mismatch) *first_mismatch = UINT64_MAX;
    uint64_t first = Engine::CHECKPOINTS_HOLD;
    const bpg_status st = guard([&] {
        assign_checks(ctx, c, m, v, n_params, param_values);
        if (n_ck != c->n_ck) throw std::invalid_argument("assign: n_ck does not match the template (" + std::to_string(c->n_ck) + " checkpoint values)");
        REQUIRE(n_ck == 0 || ck_values);
        if (n_inputs != c->n_in) throw std::invalid_argument("assign: n_inputs does not match the template (" + std::to_string(c->n_in) + " public inputs)");
        if (n_inputs && !input_values) throw std::invalid_argument("assign: the template has " + std::to_string(n_inputs) + " public inputs and input_values is null");
        if (!c->dc) throw std::invalid_argument("assign: the handle has no device state (bpg_test_circuit_handle)");
        first = ctx->engine->assign_inputs(c->dc, v, param_values, ck_values, input_values);
    });
    if (st != BPG_OK || first == Engine::CHECKPOINTS_HOLD) return st;
    if (first_mismatch) *first_mismatch = first;
    const uint64_t per = Engine::checkpoints_per_item(c->dc);
    uint64_t jp = 0, ji = 0, jc = 0;
    if (Engine::join_checkpoint_place(c->dc, first, &jp, &ji, &jc)) {     // a join: `per` is its total, no divisor
        g_last_error = "assign: checkpoint " + std::to_string(jc) + " of item " + std::to_string(ji) + " of part " + std::to_string(jp) +
                       " (flat index " + std::to_string(first) + ") is not the value the circuit computes; the circuit holds no witness";
    } else {
        g_last_error = "assign: checkpoint " + std::to_string(first % per) + (per != c->n_ck ? " of item " + std::to_string(first / per) : std::string()) +
                       " (flat index " + std::to_string(first) + ") is not the value the circuit computes; the circuit holds no witness";
    }
    return BPG_ERR_CHECKPOINT_MISMATCH;
}
bpg_status bpg_test_template_schedule(const bpg_r1cs_instance *inst, const bpg_witness_program *program, char *out, uint64_t cap) {
    return bpg_test_template_schedule_hinted(inst, program, nullptr, out, cap);
}
bpg_status bpg_test_template_schedule_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, char *out, uint64_t cap) {
    return bpg_test_template_schedule_checkpointed(inst, program, hints, nullptr, out, cap);
}
bpg_status bpg_test_template_schedule_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                   const bpg_witness_checkpoints *checkpoints, char *out, uint64_t cap) {
    return guard([&] {
        REQUIRE(inst && program && out && cap);
        const std::string r = witness_schedule_json(Engine::plan_template(as_view(inst, false), program_view(program, hints, checkpoints)).schedule);
        if (r.size() + 1 > cap) throw std::invalid_argument("template_schedule: buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(out, r.c_str(), r.size() + 1);
    });
}
static WitnessProgramView program_view_inputs(const bpg_witness_program *w, const bpg_witness_hints *h, const bpg_witness_checkpoints *k, uint64_t n_inputs,
                                              const bpg_witness_gates *g) {
    WitnessProgramView v = program_view(w, h, k);
    if (n_inputs >= (1ull << 29)) throw std::invalid_argument("template: too many public inputs (the variable index has 29 bits)");
    v.n_inputs = n_inputs;
    if (g && g->n_gates) {
        if (!g->gate_var || !g->gate_input) throw std::invalid_argument("template: n_gates without gate_var / gate_input");
        if (!n_inputs) throw std::invalid_argument("template: gates without public inputs (a gate is input * variable)");
        v.n_gates = g->n_gates; v.gate_var = g->gate_var; v.gate_input = g->gate_input;
    }
    return v;
}
bpg_status bpg_test_template_schedule_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                             const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, char *out, uint64_t cap) {
    return guard([&] {
        REQUIRE(inst && program && out && cap);
        const std::string r = witness_schedule_json(Engine::plan_template(as_view(inst, false, true), program_view_inputs(program, hints, checkpoints, n_inputs, gates)).schedule);
        if (r.size() + 1 > cap) throw std::invalid_argument("template_schedule: buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(out, r.c_str(), r.size() + 1);
    });
}
bpg_status bpg_test_template_schedule_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                             const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, char *out, uint64_t cap) {
    return bpg_test_template_schedule_gated(inst, program, hints, checkpoints, n_inputs, nullptr, out, cap);
}
bpg_status bpg_test_template_packed_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, uint32_t *stream_out, uint64_t cap, uint64_t *words_out) {
    return guard([&] {
        REQUIRE(inst && program && words_out && (cap == 0 || stream_out));
        const TemplatePlan T = Engine::plan_template(as_view(inst, false, true), program_view_inputs(program, hints, checkpoints, n_inputs, gates));
        *words_out = T.packed.stream.size();
        if (cap < T.packed.stream.size()) { if (cap) throw std::invalid_argument("template_packed: buffer too small (" + std::to_string(T.packed.stream.size()) + " words needed)"); return; }
        std::memcpy(stream_out, T.packed.stream.data(), T.packed.stream.size() * 4);
    });
}
bpg_status bpg_test_template_packed_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint32_t *stream_out, uint64_t cap, uint64_t *words_out) {
    return bpg_test_template_packed_gated(inst, program, hints, checkpoints, n_inputs, nullptr, stream_out, cap, words_out);
}
bpg_status bpg_test_template_eval_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                         const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, const uint8_t *v, const uint8_t *ck_values,
                                         const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && first_mismatch && (inst->m == 0 || v));
        REQUIRE(!checkpoints || checkpoints->n_checkpoints == 0 || ck_values);
        if (n_inputs && !input_values) throw std::invalid_argument("template_eval: the program has " + std::to_string(n_inputs) + " public inputs and input_values is null");
        *first_mismatch = Engine::template_eval_checkpointed_host(as_view(inst, false), program_view_inputs(program, hints, checkpoints, n_inputs, gates), v, ck_values, aL, aR, aO, input_values);
    });
}
bpg_status bpg_test_template_eval_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                         const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *v, const uint8_t *ck_values,
                                         const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return bpg_test_template_eval_gated(inst, program, hints, checkpoints, n_inputs, nullptr, v, ck_values, input_values, aL, aR, aO, first_mismatch);
}
bpg_status bpg_test_template_eval_batch_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                               const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, uint64_t count, const uint8_t *v,
                                               const uint8_t *ck_values, const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                               uint64_t *first_mismatch_out) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && (inst->m == 0 || count == 0 || v) && (count == 0 || first_mismatch_out));
        REQUIRE(!checkpoints || checkpoints->n_checkpoints == 0 || count == 0 || ck_values);
        if (n_inputs && count && !input_values) throw std::invalid_argument("template_eval_batch: the program has " + std::to_string(n_inputs) + " public inputs and input_values is null");
        Engine::template_eval_batch_checkpointed_host(as_view(inst, false), program_view_inputs(program, hints, checkpoints, n_inputs, gates), count, v, ck_values, aL, aR, aO,
                                                      first_mismatch_out, input_values);
    });
}
bpg_status bpg_test_template_eval_batch_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                               const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint64_t count, const uint8_t *v,
                                               const uint8_t *ck_values, const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                               uint64_t *first_mismatch_out) {
    return bpg_test_template_eval_batch_gated(inst, program, hints, checkpoints, n_inputs, nullptr, count, v, ck_values, input_values, aL, aR, aO, first_mismatch_out);
}
bpg_status bpg_test_template_gated_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs, const bpg_witness_gates *gates,
                                             const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var,
                                             uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out) {
    return guard([&] {
        REQUIRE(inst && program && row_ptr && nnz_out && ncoef_out);
        const FlatCircuit f = Engine::template_inputs_instance_host(as_view(inst, false), program_view_inputs(program, hints, nullptr, n_inputs, gates), param_values, input_values);
        const uint64_t nnz = f.term_var.size(), ncoef = f.coef.size() / 32;
        if (row_cap < f.row_ptr.size()) throw std::invalid_argument("template_inputs_instance: row_ptr too short (" + std::to_string(f.row_ptr.size()) + " entries needed)");
        if (term_cap < nnz || (nnz && (!term_var || !term_coef))) throw std::invalid_argument("template_inputs_instance: term_var / term_coef too short (" + std::to_string(nnz) + " entries needed)");
        if (coef_cap < ncoef || (ncoef && !coef)) throw std::invalid_argument("template_inputs_instance: coef too short (" + std::to_string(ncoef) + " scalars needed)");
        std::memcpy(row_ptr, f.row_ptr.data(), f.row_ptr.size() * 8);
        if (nnz) { std::memcpy(term_var, f.term_var.data(), nnz * 4); std::memcpy(term_coef, f.term_coef.data(), nnz * 4); }
        if (ncoef) std::memcpy(coef, f.coef.data(), ncoef * 32);
        *nnz_out = nnz; *ncoef_out = ncoef;
    });
}
bpg_status bpg_test_template_inputs_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs,
                                             const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var,
                                             uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out) {
    return bpg_test_template_gated_instance(inst, program, hints, n_inputs, nullptr, param_values, input_values, row_ptr, row_cap, term_var, term_coef, term_cap, coef, coef_cap, nnz_out, ncoef_out);
}
bpg_status bpg_test_circuit_handle_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, bpg_circuit **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(inst && program);
        const FlatView f = as_view(inst, false, true);
        const WitnessProgramView w = program_view_inputs(program, hints, checkpoints, n_inputs, gates);
        (void)Engine::plan_template(f, w);
        bpg_circuit *c = new bpg_circuit{nullptr, f.n, f.m}; c->is_template = true; c->n_params = w.n_params; c->n_ck = w.n_ck; c->n_in = n_inputs; c->n_gates = w.n_gates;
        *out = c;
    });
}
bpg_status bpg_test_circuit_handle_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, bpg_circuit **out) {
    return bpg_test_circuit_handle_gated(inst, program, hints, checkpoints, n_inputs, nullptr, out);
}
bpg_status bpg_test_template_eval_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                               const bpg_witness_checkpoints *checkpoints, const uint8_t *v, const uint8_t *ck_values,
                                               uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && first_mismatch && (inst->m == 0 || v));
        REQUIRE(!checkpoints || checkpoints->n_checkpoints == 0 || ck_values);
        *first_mismatch = Engine::template_eval_checkpointed_host(as_view(inst, false), program_view(program, hints, checkpoints), v, ck_values, aL, aR, aO);
    });
}
bpg_status bpg_test_template_packed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                    const bpg_witness_checkpoints *checkpoints, uint32_t *stream_out, uint64_t cap, uint64_t *words_out) {
    return guard([&] {
        REQUIRE(inst && program && words_out && (cap == 0 || stream_out));
        const TemplatePlan T = Engine::plan_template(as_view(inst, false), program_view(program, hints, checkpoints));
        *words_out = T.packed.stream.size();
        if (cap < T.packed.stream.size()) { if (cap) throw std::invalid_argument("template_packed: buffer too small (" + std::to_string(T.packed.stream.size()) + " words needed)"); return; }
        std::memcpy(stream_out, T.packed.stream.data(), T.packed.stream.size() * 4);
    });
}
bpg_status bpg_test_template_eval(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO) {
    return bpg_test_template_eval_hinted(inst, program, nullptr, v, aL, aR, aO);
}
bpg_status bpg_test_template_eval_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, const uint8_t *v,
                                         uint8_t *aL, uint8_t *aR, uint8_t *aO) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && (inst->m == 0 || v));
        Engine::template_eval_host(as_view(inst, false), program_view(program, hints), v, aL, aR, aO);
    });
}
bpg_status bpg_test_template_eval_batch(const bpg_r1cs_instance *inst, const bpg_witness_program *program, uint64_t count, const uint8_t *v,
                                        uint8_t *aL, uint8_t *aR, uint8_t *aO) {
    return bpg_test_template_eval_batch_hinted(inst, program, nullptr, count, v, aL, aR, aO);
}
bpg_status bpg_test_template_eval_batch_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                               const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && (inst->m == 0 || count == 0 || v));
        Engine::template_eval_batch_host(as_view(inst, false), program_view(program, hints), count, v, aL, aR, aO);
    });
}
bpg_status bpg_test_template_eval_batch_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                     const bpg_witness_checkpoints *checkpoints, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                     uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch_out) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && (inst->m == 0 || count == 0 || v) && (count == 0 || first_mismatch_out));
        REQUIRE(!checkpoints || checkpoints->n_checkpoints == 0 || count == 0 || ck_values);
        Engine::template_eval_batch_checkpointed_host(as_view(inst, false), program_view(program, hints, checkpoints), count, v, ck_values, aL, aR, aO, first_mismatch_out);
    });
}
bpg_status bpg_test_circuit_handle(const bpg_r1cs_instance *inst, const bpg_witness_program *program, bpg_circuit **out) {
    return bpg_test_circuit_handle_hinted(inst, program, nullptr, out);
}
bpg_status bpg_test_circuit_handle_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, bpg_circuit **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        const FlatView f = as_view(inst, false);
        if (program) (void)Engine::plan_template(f, program_view(program, hints)); else Engine::check_instance(f);
        bpg_circuit *c = new bpg_circuit{nullptr, f.n, f.m}; c->is_template = program != nullptr; c->n_params = program ? program->n_params : 0;
        *out = c;
    });
}
// bpg_r1cs_template_repeat and bpg_r1cs_template_repeat_inputs: the second serves a source with public inputs, the first refuses it
static bpg_status template_repeat(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, bpg_circuit **out, bool with_inputs) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(ctx && tmpl);
        if (count == 0) throw std::invalid_argument("template_repeat: count must be at least 1");
        if (!tmpl->is_template) throw std::invalid_argument("template_repeat: the circuit is not a template (bpg_r1cs_upload_template)");
        if (tmpl->n_gates) throw std::invalid_argument("template_repeat: the template has gated variables (a repeat carries none yet: prove its items in a batch, bpg_r1cs_prove_template_batch_inputs)");
        if (tmpl->n_in && !with_inputs) throw std::invalid_argument("template_repeat: the template has public inputs (a repeat carries none: prove its items in a batch, bpg_r1cs_prove_template_batch_inputs)");
        if (!tmpl->dc) throw std::invalid_argument("template_repeat: the handle has no device state (bpg_test_circuit_handle)");
        if (Engine::is_join(tmpl->dc)) throw std::invalid_argument("template_repeat: the circuit is a join (join its parts with larger counts instead)");
        DeviceCircuit *dc = ctx->engine->repeat_template(tmpl->dc, count, with_inputs);          // count 0, a repeat, sizes: refused there, before any device work
        bpg_circuit *c = new bpg_circuit{dc, count * tmpl->n, count * tmpl->m}; c->is_template = true; c->n_params = count * tmpl->n_params; c->n_ck = count * tmpl->n_ck;
        c->n_in = count * tmpl->n_in;
        *out = c;
    });
}
bpg_status bpg_r1cs_template_repeat(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, bpg_circuit **out) { return template_repeat(ctx, tmpl, count, out, false); }
bpg_status bpg_r1cs_template_repeat_inputs(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, bpg_circuit **out) { return template_repeat(ctx, tmpl, count, out, true); }
bpg_status bpg_r1cs_set_inputs(bpg_ctx *ctx, bpg_circuit *c, uint64_t n_inputs, const uint8_t *input_values) {
    return guard([&] {
        REQUIRE(ctx && c);
        if (!c->is_template || !c->n_in) throw std::invalid_argument("set_inputs: the circuit is not a template with public inputs (bpg_r1cs_upload_template_inputs)");
        if (n_inputs != c->n_in) throw std::invalid_argument("set_inputs: n_inputs does not match the template (" + std::to_string(c->n_in) + " public inputs)");
        if (!input_values) throw std::invalid_argument("set_inputs: the template has " + std::to_string(n_inputs) + " public inputs and input_values is null");
        if (!c->dc) throw std::invalid_argument("set_inputs: the handle has no device state (bpg_test_circuit_handle)");
        ctx->engine->set_inputs(c->dc, input_values);
    });
}
static bpg_status template_join(bpg_ctx *ctx, uint64_t n_parts, const bpg_template_part *parts, bpg_circuit **out, bool with_inputs) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(ctx && parts);
        if (n_parts == 0) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
        if (n_parts > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(n_parts) + "; at most 256)");
        std::vector<std::pair<DeviceCircuit *, uint64_t>> src;
        for (uint64_t p = 0; p < n_parts; p++) {
            const bpg_circuit *t = parts[p].tmpl;
            const std::string at = "template_join: part " + std::to_string(p) + ": ";
            if (!t) throw std::invalid_argument(at + "null template");
            if (parts[p].count == 0) throw std::invalid_argument(at + "count must be at least 1");
            if (!t->is_template) throw std::invalid_argument(at + "the circuit is not a template (bpg_r1cs_upload_template)");
            if (t->n_gates) throw std::invalid_argument(at + "the template has gated variables (a join carries none yet)");
            if (t->n_in && !with_inputs) throw std::invalid_argument(at + "the template has public inputs (a join carries none)");
            if (!t->dc) throw std::invalid_argument(at + "the handle has no device state (bpg_test_circuit_handle)");
            src.emplace_back(t->dc, parts[p].count);
        }
        DeviceCircuit *dc = ctx->engine->join_templates(src, with_inputs);          // a repeat, a join, another device, sizes: refused there, before any device work
        bpg_circuit *c = new bpg_circuit{dc, 0, 0}; c->is_template = true;
        for (uint64_t p = 0; p < n_parts; p++) {
            const bpg_circuit *t = parts[p].tmpl;
            c->n += parts[p].count * t->n; c->m += parts[p].count * t->m; c->n_params += parts[p].count * t->n_params; c->n_ck += parts[p].count * t->n_ck;
            c->n_in += parts[p].count * t->n_in;
        }
        *out = c;
    });
}
bpg_status bpg_r1cs_template_join(bpg_ctx *ctx, uint64_t n_parts, const bpg_template_part *parts, bpg_circuit **out) { return template_join(ctx, n_parts, parts, out, false); }
bpg_status bpg_r1cs_template_join_inputs(bpg_ctx *ctx, uint64_t n_parts, const bpg_template_part *parts, bpg_circuit **out) { return template_join(ctx, n_parts, parts, out, true); }
static std::vector<Engine::JoinSource> join_sources(uint64_t n_parts, const bpg_test_join_part *parts) {
    if (n_parts == 0) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
    if (n_parts > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(n_parts) + "; at most 256)");
    std::vector<Engine::JoinSource> src;
    for (uint64_t p = 0; p < n_parts; p++) {
        if (!parts[p].inst || !parts[p].program) throw std::invalid_argument("template_join: part " + std::to_string(p) + ": null instance or program");
        src.push_back({as_view(parts[p].inst, false), program_view(parts[p].program, parts[p].hints, parts[p].checkpoints), parts[p].count});
    }
    return src;
}
bpg_status bpg_test_template_join_instance(uint64_t n_parts, const bpg_test_join_part *parts, const uint8_t *param_values, uint64_t *row_ptr, uint64_t row_cap,
                                           uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out,
                                           uint64_t *ncoef_out) {
    return guard([&] {
        REQUIRE(parts && row_ptr && nnz_out && ncoef_out);
        const FlatCircuit f = Engine::template_join_instance_host(join_sources(n_parts, parts), param_values);
        const uint64_t nnz = f.term_var.size(), ncoef = f.coef.size() / 32;
        if (row_cap < f.row_ptr.size()) throw std::invalid_argument("template_join_instance: row_ptr too short (" + std::to_string(f.row_ptr.size()) + " entries needed)");
        if (term_cap < nnz || (nnz && (!term_var || !term_coef))) throw std::invalid_argument("template_join_instance: term_var / term_coef too short (" + std::to_string(nnz) + " entries needed)");
        if (coef_cap < ncoef || (ncoef && !coef)) throw std::invalid_argument("template_join_instance: coef too short (" + std::to_string(ncoef) + " scalars needed)");
        std::memcpy(row_ptr, f.row_ptr.data(), f.row_ptr.size() * 8);
        if (nnz) { std::memcpy(term_var, f.term_var.data(), nnz * 4); std::memcpy(term_coef, f.term_coef.data(), nnz * 4); }
        if (ncoef) std::memcpy(coef, f.coef.data(), ncoef * 32);
        *nnz_out = nnz; *ncoef_out = ncoef;
    });
}
bpg_status bpg_test_template_eval_join(uint64_t n_parts, const bpg_test_join_part *parts, const uint8_t *v, const uint8_t *ck_values, uint8_t *aL,
                                       uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return guard([&] {
        REQUIRE(parts && aL && aR && aO && first_mismatch);
        const std::vector<Engine::JoinSource> src = join_sources(n_parts, parts);
        uint64_t m = 0;
        for (const Engine::JoinSource &s : src) m += s.c.m;
        REQUIRE(m == 0 || v);
        *first_mismatch = Engine::template_eval_join_host(src, v, ck_values, aL, aR, aO);
    });
}
static std::vector<Engine::JoinSource> join_sources_inputs(uint64_t n_parts, const bpg_test_join_inputs_part *parts) {
    if (n_parts == 0) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
    if (n_parts > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(n_parts) + "; at most 256)");
    std::vector<Engine::JoinSource> src;
    for (uint64_t p = 0; p < n_parts; p++) {
        if (!parts[p].inst || !parts[p].program) throw std::invalid_argument("template_join: part " + std::to_string(p) + ": null instance or program");
        src.push_back({as_view(parts[p].inst, false, true), program_view_inputs(parts[p].program, parts[p].hints, parts[p].checkpoints, parts[p].n_inputs, nullptr), parts[p].count});
    }
    return src;
}
// the outputs of an instance hook, after its sizes were checked against the caller's capacities
static void instance_out(const FlatCircuit &f, uint64_t *row_ptr, uint32_t *term_var, uint32_t *term_coef, uint8_t *coef, uint64_t *nnz_out, uint64_t *ncoef_out) {
    const uint64_t nnz = f.term_var.size(), ncoef = f.coef.size() / 32;
    std::memcpy(row_ptr, f.row_ptr.data(), f.row_ptr.size() * 8);
    if (nnz) { std::memcpy(term_var, f.term_var.data(), nnz * 4); std::memcpy(term_coef, f.term_coef.data(), nnz * 4); }
    if (ncoef) std::memcpy(coef, f.coef.data(), ncoef * 32);
    *nnz_out = nnz; *ncoef_out = ncoef;
}
bpg_status bpg_test_template_join_inputs_instance(uint64_t n_parts, const bpg_test_join_inputs_part *parts, const uint8_t *param_values, const uint8_t *input_values,
                                                  uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef,
                                                  uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out) {
    return guard([&] {
        REQUIRE(parts && row_ptr && nnz_out && ncoef_out);
        const uint64_t caps[3] = {row_cap, (term_var && term_coef) ? term_cap : 0, coef ? coef_cap : 0};       // every size is known before a row is made: refused, nothing written
        const FlatCircuit f = Engine::template_join_instance_host(join_sources_inputs(n_parts, parts), param_values, input_values, caps);
        instance_out(f, row_ptr, term_var, term_coef, coef, nnz_out, ncoef_out);
    });
}
bpg_status bpg_test_template_eval_join_inputs(uint64_t n_parts, const bpg_test_join_inputs_part *parts, const uint8_t *v, const uint8_t *ck_values,
                                              const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return guard([&] {
        REQUIRE(parts && aL && aR && aO && first_mismatch);
        const std::vector<Engine::JoinSource> src = join_sources_inputs(n_parts, parts);
        uint64_t m = 0;
        for (const Engine::JoinSource &s : src) m += s.c.m;
        REQUIRE(m == 0 || v);
        *first_mismatch = Engine::template_eval_join_host(src, v, ck_values, aL, aR, aO, input_values);
    });
}
bpg_status bpg_test_template_repeat_inputs_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs,
                                                    uint64_t count, const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr, uint64_t row_cap,
                                                    uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out,
                                                    uint64_t *ncoef_out) {
    return guard([&] {
        REQUIRE(inst && program && row_ptr && nnz_out && ncoef_out);
        const uint64_t caps[3] = {row_cap, (term_var && term_coef) ? term_cap : 0, coef ? coef_cap : 0};
        const FlatCircuit f = Engine::template_repeat_inputs_instance_host(as_view(inst, false, true), program_view_inputs(program, hints, nullptr, n_inputs, nullptr), count, param_values,
                                                                           input_values, caps);
        instance_out(f, row_ptr, term_var, term_coef, coef, nnz_out, ncoef_out);
    });
}
bpg_status bpg_test_template_eval_repeat_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && first_mismatch && (inst->m == 0 || count == 0 || v));
        REQUIRE(!checkpoints || checkpoints->n_checkpoints == 0 || count == 0 || ck_values);
        *first_mismatch = Engine::template_eval_repeat_inputs_host(as_view(inst, false, true), program_view_inputs(program, hints, checkpoints, n_inputs, nullptr), count, v, ck_values,
                                                                   input_values, aL, aR, aO);
    });
}
bpg_status bpg_r1cs_check(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out, bpg_check_report *report) {
    return guard([&] {
        REQUIRE(ctx && c && n_rows_out && report);
        if (cap && !rows_out) throw std::invalid_argument("check: rows_out is null with cap > 0");
        if (m != c->m) throw std::invalid_argument("check: m does not match the circuit");
        if (!v && m && !c->is_template) throw std::invalid_argument("check: a plain upload does not keep its committed values: pass v");
        if (!c->dc) throw std::invalid_argument("check: the handle has no device state (bpg_test_circuit_handle)");
        uint64_t have = 0;
        const CheckReport r = ctx->engine->check(c->dc, v, cap, rows_out, &have);        // no witness: refused there, before any device work
        *n_rows_out = have;
        report->bad_multipliers = r.bad_multipliers; report->first_bad_multiplier = r.first_bad_multiplier; report->bad_rows = r.bad_rows; report->first_bad_row = r.first_bad_row;
    });
}
bpg_status bpg_test_check_host(const bpg_r1cs_instance *inst, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out, bpg_check_report *report) {
    return guard([&] {
        REQUIRE(inst && n_rows_out && report);
        const FlatView f = as_view(inst, false);
        Engine::check_instance(f);
        if (f.n && !f.aL) throw R1CSException(R1CSError::MissingAssignment, "check: the instance carries no witness");
        if (!v && f.m) throw std::invalid_argument("check: v is null with m > 0");
        if (cap && !rows_out) throw std::invalid_argument("check: rows_out is null with cap > 0");
        uint64_t have = 0;
        const CheckReport r = check_host(f, v, cap, rows_out, &have);
        *n_rows_out = have;
        report->bad_multipliers = r.bad_multipliers; report->first_bad_multiplier = r.first_bad_multiplier; report->bad_rows = r.bad_rows; report->first_bad_row = r.first_bad_row;
    });
}
bpg_status bpg_test_template_repeat_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                             const uint8_t *param_values, uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var, uint32_t *term_coef,
                                             uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out) {
    return guard([&] {
        REQUIRE(inst && program && row_ptr && nnz_out && ncoef_out);
        const FlatCircuit f = Engine::template_repeat_instance_host(as_view(inst, false), program_view(program, hints), count, param_values);
        const uint64_t nnz = f.term_var.size(), ncoef = f.coef.size() / 32;
        if (row_cap < f.row_ptr.size()) throw std::invalid_argument("template_repeat_instance: row_ptr too short (" + std::to_string(f.row_ptr.size()) + " entries needed)");
        if (term_cap < nnz || (nnz && (!term_var || !term_coef))) throw std::invalid_argument("template_repeat_instance: term_var / term_coef too short (" + std::to_string(nnz) + " entries needed)");
        if (coef_cap < ncoef || (ncoef && !coef)) throw std::invalid_argument("template_repeat_instance: coef too short (" + std::to_string(ncoef) + " scalars needed)");
        std::memcpy(row_ptr, f.row_ptr.data(), f.row_ptr.size() * 8);
        if (nnz) { std::memcpy(term_var, f.term_var.data(), nnz * 4); std::memcpy(term_coef, f.term_coef.data(), nnz * 4); }
        if (ncoef) std::memcpy(coef, f.coef.data(), ncoef * 32);
        *nnz_out = nnz; *ncoef_out = ncoef;
    });
}
bpg_status bpg_test_template_eval_repeat(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                         const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO) {
    return guard([&] {
        REQUIRE(inst && program && aL && aR && aO && (inst->m == 0 || count == 0 || v));
        Engine::template_eval_repeat_host(as_view(inst, false), program_view(program, hints), count, v, aL, aR, aO);
    });
}

static void copy_timings(const ProveTimings &t, bpg_timings *o) {
    if (!o) return;
    o->rng_host = t.rng_host; o->msm_aiao = t.msm_aiao; o->msm_s = t.msm_s; o->poly = t.poly; o->ipa = t.ipa; o->total = t.total;
    o->ipa_msm = t.ipa_msm; o->ipa_fold = t.ipa_fold; o->ipa_sync = t.ipa_sync;
}

// script: null everywhere but in the bpg_test_*_scripted hooks, which run the same body on a transcript that hands out the challenges their caller chose
static bpg_status prove_resident(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *v_blinding, const uint8_t seed[32],
                                 uint32_t flags, uint8_t *proof_out, uint64_t *proof_len, bpg_timings *timings, const uint8_t *script, uint64_t script_len) {
    return guard([&] {
        REQUIRE(ctx && c && c->dc && ts && seed && proof_out && proof_len && (m == 0 || v_blinding));
        if (m != c->m) throw std::invalid_argument("prove: m does not match the uploaded circuit");
        if (*proof_len < bpg_proof_size(c->n, flags)) throw std::invalid_argument("prove: proof buffer too small");
        require_gens_capacity(ctx->engine->gens_capacity(), c->n, " (call bpg_gens_ensure)");
        Transcript T = Transcript::from_state(ts);
        if (script) Engine::script_transcript(T, c->n, script, script_len);
        std::vector<Scalar> vb(m);
        for (uint64_t i = 0; i < m; i++) vb[i] = Scalar::from_bytes_mod_order(v_blinding + 32 * i);
        ProveTimings tm;
        std::vector<uint8_t> proof = ctx->engine->prove(c->dc, T, vb, seed, flags, timings ? &tm : nullptr);
        std::memcpy(proof_out, proof.data(), proof.size()); *proof_len = proof.size();
        T.export_state(ts);
        copy_timings(tm, timings);
    });
}
bpg_status bpg_r1cs_prove_resident(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *v_blinding,
                                   const uint8_t seed[32], uint32_t flags, uint8_t *proof_out, uint64_t *proof_len, bpg_timings *timings) {
    return prove_resident(ctx, c, ts, m, v_blinding, seed, flags, proof_out, proof_len, timings, nullptr, 0);
}
bpg_status bpg_test_prove_scripted(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *v_blinding, const uint8_t seed[32],
                                   uint32_t flags, const uint8_t *script, uint64_t script_len, uint8_t *proof_out, uint64_t *proof_len) {
    if (!script) { g_last_error = "null or invalid argument: script"; return BPG_ERR_INVALID_ARGUMENT; }
    return prove_resident(ctx, c, ts, m, v_blinding, seed, flags, proof_out, proof_len, nullptr, script, script_len);
}

bpg_status bpg_r1cs_prove(bpg_ctx *ctx, const bpg_r1cs_instance *inst, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *v_blinding,
                          const uint8_t seed[32], uint32_t flags, uint8_t *proof_out, uint64_t *proof_len) {
    bpg_circuit *c = nullptr;
    bpg_status s = bpg_r1cs_upload(ctx, inst, &c);
    if (s != BPG_OK) return s;
    s = bpg_r1cs_prove_resident(ctx, c, ts, m, v_blinding, seed, flags, proof_out, proof_len, nullptr);
    std::string keep = g_last_error;
    bpg_r1cs_free(ctx, c);
    g_last_error = keep;
    return s;
}

// what a batch call returns: every item's status, and the first failure with its message as the call's own
static bpg_status batch_status(const std::vector<bpg_status> &st, const std::vector<std::string> &msg, bpg_status *status_out) {
    bpg_status first = BPG_OK;
    g_last_error.clear();
    for (size_t k = 0; k < st.size(); k++) {
        status_out[k] = st[k];
        if (first == BPG_OK && st[k] != BPG_OK) { first = st[k]; g_last_error = "item " + std::to_string(k) + ": " + msg[k]; }
    }
    return first;
}

// scripts: null everywhere but in bpg_test_prove_batch_scripted - one script per item, every item through Engine::prove_batch (an item that would take the
// single path is refused), and a bad script refuses the whole call before anything is launched
static bpg_status prove_batch(bpg_ctx *ctx, uint64_t count, const bpg_batch_item *items, bpg_status *status_out, const uint8_t *const *scripts, const uint64_t *script_lens) {
    if (!ctx || (count && (!items || !status_out))) { g_last_error = "null or invalid argument: ctx, items and status_out"; return BPG_ERR_INVALID_ARGUMENT; }
    if (!count) { g_last_error.clear(); return BPG_OK; }
    if (scripts) {
        const bpg_status s = guard([&] {
            for (uint64_t k = 0; k < count; k++) {
                REQUIRE(items[k].inst && scripts[k]);
                Transcript probe;
                Engine::script_transcript(probe, items[k].inst->n, scripts[k], script_lens[k]);
                if (!ctx->engine->lockstep_eligible(items[k].inst->n, items[k].flags)) throw std::invalid_argument("prove_batch_scripted: item " + std::to_string(k) + " is not lockstep-eligible");
            }
        });
        if (s != BPG_OK) return s;
    }
    std::vector<bpg_status> st(count, BPG_OK);
    std::vector<std::string> msg(count);
    std::vector<FlatView> views(count);
    std::vector<Transcript> T(count);
    std::vector<std::vector<Scalar>> vb(count);
    std::vector<Engine::ProveItem> lock;
    std::vector<uint64_t> lock_at, single_at;
    for (uint64_t k = 0; k < count; k++) {
        const bpg_batch_item &it = items[k];
        // the checks of bpg_r1cs_prove (upload, then bpg_r1cs_prove_resident), in its order: an item fails alone, with that call's status
        st[k] = guard([&] {
            const FlatView f = as_view(it.inst, true);
            Engine::check_instance(f);
            REQUIRE(it.transcript_state && it.rng_seed && it.proof_out && it.proof_len && (it.m == 0 || it.v_blinding));
            if (it.m != f.m) throw std::invalid_argument("prove: m does not match the uploaded circuit");
            if (*it.proof_len < bpg_proof_size(f.n, it.flags)) throw std::invalid_argument("prove: proof buffer too small");
            require_gens_capacity(ctx->engine->gens_capacity(), f.n, " (call bpg_gens_ensure)");
            views[k] = f;
        });
        if (st[k] != BPG_OK) { msg[k] = g_last_error; continue; }
        if (!ctx->engine->lockstep_eligible(views[k].n, it.flags)) { single_at.push_back(k); continue; }
        T[k] = Transcript::from_state(it.transcript_state);
        if (scripts) Engine::script_transcript(T[k], views[k].n, scripts[k], script_lens[k]);       // (checked above: does not throw)
        vb[k].resize(it.m);
        for (uint64_t i = 0; i < it.m; i++) vb[k][i] = Scalar::from_bytes_mod_order(it.v_blinding + 32 * i);
        Engine::ProveItem p; p.flat = &views[k]; p.T = &T[k]; p.vb = &vb[k]; p.seed = it.rng_seed; p.flags = it.flags;
        lock.push_back(std::move(p)); lock_at.push_back(k);
    }
    if (!lock.empty()) {
        const bpg_status s = guard([&] { ctx->engine->prove_batch(lock.size(), lock.data()); });
        const std::string why = g_last_error;
        for (size_t j = 0; j < lock.size(); j++) {
            const uint64_t k = lock_at[j];
            st[k] = s;
            if (s != BPG_OK) { msg[k] = why; continue; }
            std::memcpy(items[k].proof_out, lock[j].proof.data(), lock[j].proof.size()); *items[k].proof_len = lock[j].proof.size();
            T[k].export_state(items[k].transcript_state);
        }
    }
    for (uint64_t k : single_at) {      // larger circuits and expanded blinding: the single path, same bytes
        const bpg_batch_item &it = items[k];
        st[k] = bpg_r1cs_prove(ctx, it.inst, it.transcript_state, it.m, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len);
        if (st[k] != BPG_OK) msg[k] = g_last_error;
    }
    return batch_status(st, msg, status_out);
}
bpg_status bpg_r1cs_prove_batch(bpg_ctx *ctx, uint64_t count, const bpg_batch_item *items, bpg_status *status_out) {
    return prove_batch(ctx, count, items, status_out, nullptr, nullptr);
}
bpg_status bpg_test_prove_batch_scripted(bpg_ctx *ctx, uint64_t count, const bpg_batch_item *items, const uint8_t *const *scripts, const uint64_t *script_lens,
                                         bpg_status *status_out) {
    if (count && (!scripts || !script_lens)) { g_last_error = "null or invalid argument: scripts and script_lens"; return BPG_ERR_INVALID_ARGUMENT; }
    return prove_batch(ctx, count, items, status_out, count ? scripts : nullptr, script_lens);
}

// the whole call is refused before anything is written or launched; a handle without device state first, whatever else was passed
// (checkpointed: bpg_r1cs_prove_template_batch_checkpointed, whose items carry the values the two frozen calls have no place for)
static bpg_status template_batch_refusal(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const void *items, bpg_status *status_out, bool checkpointed = false,
                                         bool with_inputs = false) {
    // (a template with public inputs handed to a call whose items carry none: the one refusal that comes before the handle's, so that it can be seen without a device)
    if (tmpl && tmpl->is_template && tmpl->n_in && !with_inputs) { g_last_error = "prove_template_batch: the template has public inputs, and a batch item carries no values for them (bpg_r1cs_prove_template_batch_inputs, or bpg_r1cs_assign_inputs + bpg_r1cs_prove_resident)"; return BPG_ERR_INVALID_ARGUMENT; }
    if (tmpl && !tmpl->dc) { g_last_error = "prove_template_batch: the handle has no device state (bpg_test_circuit_handle)"; return BPG_ERR_INVALID_ARGUMENT; }
    if (!ctx || !tmpl || (count && (!items || !status_out))) { g_last_error = "null or invalid argument: ctx, tmpl, items and status_out"; return BPG_ERR_INVALID_ARGUMENT; }
    if (!tmpl->is_template) { g_last_error = "prove_template_batch: the circuit is not a template (bpg_r1cs_upload_template)"; return BPG_ERR_INVALID_ARGUMENT; }
    if (tmpl->n_ck && !checkpointed) { g_last_error = "prove_template_batch: the template has checkpoints, and a batch item carries no values for them (bpg_r1cs_prove_template_batch_checkpointed, or bpg_r1cs_assign_checkpointed + bpg_r1cs_prove_resident)"; return BPG_ERR_INVALID_ARGUMENT; }
    return BPG_OK;
}
// items that passed template_batch_refusal (none: BPG_OK, nothing touched).  coms == nullptr: bpg_r1cs_prove_template_batch.  Else bpg_r1cs_prove_template_batch_commit: the
// transcript states are those BEFORE the "V" appends and coms[k] receives item k's m encodings (the caller checked m > 0).
// cks != nullptr: bpg_r1cs_prove_template_batch_checkpointed on a template with checkpoints - cks[k] item k's n_ck values, firsts[k] (null allowed) where its
// lowest mismatch goes.  A mismatching item fails alone on either path, with nothing of it written.
// ins != nullptr: bpg_r1cs_prove_template_batch_inputs on a template with public inputs - ins[k] item k's n_inputs values
static bpg_status template_batch(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_item *items, uint8_t *const *coms, bpg_status *status_out,
                                 const uint8_t *const *cks = nullptr, uint64_t *const *firsts = nullptr, const uint8_t *const *ins = nullptr) {
    if (!count) { g_last_error.clear(); return BPG_OK; }
    const uint64_t m = tmpl->m, n = tmpl->n, n_params = tmpl->n_params, n_ck = cks ? tmpl->n_ck : 0, n_in = ins ? tmpl->n_in : 0;
    for (uint64_t k = 0; k < count && firsts; k++) if (firsts[k]) *firsts[k] = UINT64_MAX;
    std::vector<bpg_status> st(count, BPG_OK);
    std::vector<std::string> msg(count);
    std::vector<Transcript> T(count);
    std::vector<std::vector<Scalar>> vb(count);
    std::vector<Engine::ProveItem> lock;
    std::vector<uint64_t> lock_at;
    std::vector<uint8_t> route(count, 0);       // 0 failed its checks, 1 lockstep, 2 assign + prove_resident
    const bool host_copy = Engine::template_lockstep(tmpl->dc);
    for (uint64_t k = 0; k < count; k++) {
        const bpg_template_item &it = items[k];
        // the checks of bpg_r1cs_assign, then those of bpg_r1cs_prove_resident, in their order: an item fails alone, with that call's status
        st[k] = guard([&] {
            REQUIRE((m == 0 || it.v) && (n_params == 0 || it.param_values));
            REQUIRE(it.transcript_state && it.rng_seed && it.proof_out && it.proof_len && (m == 0 || it.v_blinding));
            if (coms && !coms[k]) throw std::invalid_argument("prove_template_batch_commit: an item without a commitment buffer");
            if (n_ck && !cks[k]) throw std::invalid_argument("prove_template_batch_checkpointed: an item without checkpoint values (the template takes " + std::to_string(n_ck) + ")");
            if (n_in && !ins[k]) throw std::invalid_argument("prove_template_batch_inputs: an item without input values (the template takes " + std::to_string(n_in) + ")");
            if (*it.proof_len < bpg_proof_size(n, it.flags)) throw std::invalid_argument("prove: proof buffer too small");
            require_gens_capacity(ctx->engine->gens_capacity(), n, " (call bpg_gens_ensure)");
        });
        if (st[k] != BPG_OK) { msg[k] = g_last_error; continue; }
        if (!host_copy || !ctx->engine->lockstep_eligible(n, it.flags)) { route[k] = 2; continue; }
        route[k] = 1;
        T[k] = Transcript::from_state(it.transcript_state);
        vb[k].resize(m);
        for (uint64_t i = 0; i < m; i++) vb[k][i] = Scalar::from_bytes_mod_order(it.v_blinding + 32 * i);
        Engine::ProveItem p; p.T = &T[k]; p.vb = &vb[k]; p.seed = it.rng_seed; p.flags = it.flags; p.values = it.v; p.params = it.param_values;
        if (n_ck) p.ck = cks[k];
        if (n_in) p.inputs = ins[k];
        lock.push_back(std::move(p)); lock_at.push_back(k);
    }
    if (!lock.empty()) {
        const bpg_status s = guard([&] { ctx->engine->prove_template_batch(tmpl->dc, lock.size(), lock.data(), coms != nullptr, cks != nullptr); });
        const std::string why = g_last_error;
        for (size_t j = 0; j < lock.size(); j++) {
            const uint64_t k = lock_at[j];
            st[k] = s;
            if (s != BPG_OK) { msg[k] = why; continue; }
            if (lock[j].ck_first != Engine::CHECKPOINTS_HOLD) {       // its wave went on without it mattering: no proof, no commitments, the state as given
                st[k] = BPG_ERR_CHECKPOINT_MISMATCH;
                msg[k] = "checkpoint " + std::to_string(lock[j].ck_first) + " is not the value the circuit computes; no proof was made for the item";
                if (firsts && firsts[k]) *firsts[k] = lock[j].ck_first;
                continue;
            }
            std::memcpy(items[k].proof_out, lock[j].proof.data(), lock[j].proof.size()); *items[k].proof_len = lock[j].proof.size();
            T[k].export_state(items[k].transcript_state);
            if (coms) std::memcpy(coms[k], lock[j].commitments.data(), 32 * m);
        }
    }
    // larger templates, BPG_TT_ORIG_LG=0 and expanded blinding: assign + the single path, one at a time, same bytes.  Their commitments (coms) are made
    // up front, ALL of them in one Pedersen launch, and appended to a copy of each transcript: an item that fails keeps its state and its buffer
    std::vector<uint64_t> single_at;
    for (uint64_t k = 0; k < count; k++) if (route[k] == 2) single_at.push_back(k);
    std::vector<uint8_t> scom;
    if (coms && !single_at.empty()) {
        std::vector<uint8_t> sv(single_at.size() * m * 32), sb(sv.size());
        for (size_t j = 0; j < single_at.size(); j++) {
            std::memcpy(&sv[j * m * 32], items[single_at[j]].v, m * 32); std::memcpy(&sb[j * m * 32], items[single_at[j]].v_blinding, m * 32);
        }
        scom.resize(sv.size());
        const bpg_status s = guard([&] { ctx->engine->pedersen_commit(single_at.size() * m, sv.data(), sb.data(), scom.data()); });
        if (s != BPG_OK) { for (uint64_t k : single_at) { st[k] = s; msg[k] = g_last_error; } single_at.clear(); }
    }
    for (size_t j = 0; j < single_at.size(); j++) {
        const uint64_t k = single_at[j];
        const bpg_template_item &it = items[k];
        uint8_t state[BPG_TRANSCRIPT_STATE_BYTES];
        if (coms) {
            Transcript t = Transcript::from_state(it.transcript_state);
            for (uint64_t i = 0; i < m; i++) t.append_point("V", &scom[(j * m + i) * 32]);
            t.export_state(state);
        }
        st[k] = n_in ? bpg_r1cs_assign_inputs(ctx, tmpl, m, it.v, n_params, it.param_values, n_ck, n_ck ? cks[k] : nullptr, firsts ? firsts[k] : nullptr, n_in, ins[k])
                : n_ck ? bpg_r1cs_assign_checkpointed(ctx, tmpl, m, it.v, n_params, it.param_values, n_ck, cks[k], firsts ? firsts[k] : nullptr)
                       : bpg_r1cs_assign(ctx, tmpl, m, it.v, n_params, it.param_values);
        if (st[k] == BPG_OK) st[k] = bpg_r1cs_prove_resident(ctx, tmpl, coms ? state : it.transcript_state, m, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len, nullptr);
        if (st[k] != BPG_OK) { msg[k] = g_last_error; continue; }
        if (coms) { std::memcpy(it.transcript_state, state, sizeof state); std::memcpy(coms[k], &scom[j * m * 32], m * 32); }
    }
    Engine::drop_witness(tmpl->dc);             // on either path: a caller never depends on which one its items took
    return batch_status(st, msg, status_out);
}

bpg_status bpg_r1cs_prove_template_batch(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_item *items, bpg_status *status_out) {
    const bpg_status s = template_batch_refusal(ctx, tmpl, count, items, status_out);
    if (s != BPG_OK) return s;
    return template_batch(ctx, tmpl, count, items, nullptr, status_out);
}

bpg_status bpg_r1cs_prove_template_batch_commit(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_commit_item *items, bpg_status *status_out) {
    const bpg_status s = template_batch_refusal(ctx, tmpl, count, items, status_out);
    if (s != BPG_OK) return s;
    std::vector<bpg_template_item> plain(count);
    std::vector<uint8_t *> coms(count);
    for (uint64_t k = 0; k < count; k++) {
        const bpg_template_commit_item &it = items[k];
        plain[k] = bpg_template_item{it.v, it.param_values, it.transcript_state, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len};
        coms[k] = it.commitments_out;
    }
    return template_batch(ctx, tmpl, count, plain.data(), tmpl->m ? coms.data() : nullptr, status_out);      // nothing to commit to: the existing call
}

bpg_status bpg_r1cs_prove_template_batch_checkpointed(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_ck_item *items, int32_t commit,
                                                      bpg_status *status_out) {
    const bpg_status s = template_batch_refusal(ctx, tmpl, count, items, status_out, true);
    if (s != BPG_OK) return s;
    std::vector<bpg_template_item> plain(count);
    std::vector<uint8_t *> coms(count);
    std::vector<const uint8_t *> cks(count);
    std::vector<uint64_t *> firsts(count);
    for (uint64_t k = 0; k < count; k++) {
        const bpg_template_ck_item &it = items[k];
        plain[k] = bpg_template_item{it.v, it.param_values, it.transcript_state, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len};
        coms[k] = it.commitments_out; cks[k] = it.ck_values; firsts[k] = it.first_mismatch;
    }
    // a template without checkpoints: exactly the frozen call `commit` selects (ck_values is not looked at; *first_mismatch, where given, reads UINT64_MAX)
    return template_batch(ctx, tmpl, count, plain.data(), commit && tmpl->m ? coms.data() : nullptr, status_out, tmpl->n_ck ? cks.data() : nullptr, firsts.data());
}

bpg_status bpg_r1cs_prove_template_batch_inputs(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_in_item *items, int32_t commit,
                                                bpg_status *status_out) {
    const bpg_status s = template_batch_refusal(ctx, tmpl, count, items, status_out, true, true);
    if (s != BPG_OK) return s;
    std::vector<bpg_template_item> plain(count);
    std::vector<uint8_t *> coms(count);
    std::vector<const uint8_t *> cks(count), ins(count);
    std::vector<uint64_t *> firsts(count);
    for (uint64_t k = 0; k < count; k++) {
        const bpg_template_in_item &it = items[k];
        plain[k] = bpg_template_item{it.v, it.param_values, it.transcript_state, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len};
        coms[k] = it.commitments_out; cks[k] = it.ck_values; firsts[k] = it.first_mismatch; ins[k] = it.input_values;
    }
    // a template without inputs: exactly bpg_r1cs_prove_template_batch_checkpointed, byte for byte (input_values is not looked at)
    return template_batch(ctx, tmpl, count, plain.data(), commit && tmpl->m ? coms.data() : nullptr, status_out, tmpl->n_ck ? cks.data() : nullptr, firsts.data(),
                          tmpl->n_in ? ins.data() : nullptr);
}

bpg_status bpg_test_append_commitments(const uint8_t state_in[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *coms, uint8_t state_out[BPG_TRANSCRIPT_STATE_BYTES]) {
    return guard([&] {
        REQUIRE(state_in && state_out && (m == 0 || coms));
        Transcript t = Transcript::from_state(state_in);
        for (uint64_t i = 0; i < m; i++) t.append_point("V", coms + 32 * i);
        t.export_state(state_out);
    });
}

bpg_status bpg_r1cs_verify(bpg_ctx *ctx, const bpg_r1cs_instance *inst, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *V,
                           const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags) {
    return guard([&] {
        REQUIRE(ctx && ts && proof && seed && (m == 0 || V));
        const FlatView f = as_view(inst, false, true);           // verifier side: no assignments
        if (f.m != m) throw std::invalid_argument("verify: m does not match the instance");
        Engine::check_instance(f);
        DeviceCircuit *dc = ctx->engine->upload(f);
        Transcript T = Transcript::from_state(ts);
        R1CSError e;
        try { e = ctx->engine->verify(dc, T, V, proof, proof_len, seed, flags); } catch (...) { ctx->engine->free_circuit(dc); throw; }
        ctx->engine->free_circuit(dc);
        T.export_state(ts);
        if (e != R1CSError::None) throw R1CSException(e, e == R1CSError::VerificationError ? "proof rejected" : e == R1CSError::FormatError ? "malformed proof" : "generator capacity below padded circuit size");
    });
}

static bpg_status verify_resident(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *V, const uint8_t *proof,
                                  uint64_t proof_len, const uint8_t seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len) {
    return guard([&] {
        REQUIRE(ctx && c && c->dc && ts && proof && seed && (m == 0 || V));
        if (m != c->m) throw std::invalid_argument("verify: m does not match the uploaded circuit");
        Transcript T = Transcript::from_state(ts);
        if (script) Engine::script_transcript(T, c->n, script, script_len);
        const R1CSError e = ctx->engine->verify(c->dc, T, V, proof, proof_len, seed, flags);
        T.export_state(ts);
        if (e != R1CSError::None) throw R1CSException(e, e == R1CSError::VerificationError ? "proof rejected" : e == R1CSError::FormatError ? "malformed proof" : "generator capacity below padded circuit size");
    });
}

bpg_status bpg_r1cs_verify_resident(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *V,
                                    const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags) {
    return verify_resident(ctx, c, ts, m, V, proof, proof_len, seed, flags, nullptr, 0);
}
bpg_status bpg_test_verify_scripted(bpg_ctx *ctx, bpg_circuit *c, uint8_t ts[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *V, const uint8_t *proof,
                                    uint64_t proof_len, const uint8_t seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len) {
    if (!script) { g_last_error = "null or invalid argument: script"; return BPG_ERR_INVALID_ARGUMENT; }
    return verify_resident(ctx, c, ts, m, V, proof, proof_len, seed, flags, script, script_len);
}

static bpg_status verify_batch(bpg_ctx *ctx, uint64_t count, const bpg_verify_item *items, const uint8_t batch_seed[32], bpg_status *status_out,
                               const uint8_t *const *scripts, const uint64_t *script_lens) {
    return guard([&] {
        REQUIRE(ctx);
        if (!count) return;
        REQUIRE(items && status_out && batch_seed);
        // every argument first: a refused call launches nothing and touches no transcript state
        std::vector<FlatView> views(count);
        std::vector<Transcript> T(count);
        std::vector<Engine::VerifyItem> ei(count);
        for (uint64_t k = 0; k < count; k++) {
            const bpg_verify_item &it = items[k];
            const std::string who = "verify_batch: item " + std::to_string(k);
            if ((it.inst != nullptr) == (it.circuit != nullptr)) throw std::invalid_argument(who + ": exactly one of inst and circuit must be set");
            if (!it.transcript_state || !it.proof || !it.seed || (it.m && !it.V)) throw std::invalid_argument(who + ": null argument");
            Engine::VerifyItem &e = ei[k];
            if (it.inst) {
                views[k] = as_view(it.inst, false, true);               // verifier side: no assignments
                if (views[k].m != it.m) throw std::invalid_argument(who + ": m does not match the instance");
                Engine::check_instance(views[k]);
                e.flat = &views[k];
            } else {
                if (it.m != it.circuit->m) throw std::invalid_argument(who + ": m does not match the uploaded circuit");
                if (!it.circuit->dc) throw std::invalid_argument(who + ": the circuit handle has no device state");
                e.dc = it.circuit->dc;
            }
            T[k] = Transcript::from_state(it.transcript_state);
            if (scripts) { REQUIRE(scripts[k]); Engine::script_transcript(T[k], it.inst ? views[k].n : it.circuit->n, scripts[k], script_lens[k]); }
            e.T = &T[k]; e.V = it.V; e.proof = it.proof; e.proof_len = it.proof_len; e.seed = it.seed; e.flags = it.flags;
        }
        std::vector<R1CSError> st(count);
        ctx->engine->verify_batch(count, ei.data(), batch_seed, st.data());
        uint64_t first = count;
        for (uint64_t k = 0; k < count; k++) {
            T[k].export_state(items[k].transcript_state);
            status_out[k] = (bpg_status)st[k];
            if (first == count && st[k] != R1CSError::None) first = k;
        }
        if (first < count) {
            const R1CSError e = st[first];
            throw R1CSException(e, "item " + std::to_string(first) + ": " + (e == R1CSError::VerificationError ? "proof rejected" : e == R1CSError::FormatError ? "malformed proof" : "generator capacity below padded circuit size"));
        }
    });
}
bpg_status bpg_r1cs_verify_batch(bpg_ctx *ctx, uint64_t count, const bpg_verify_item *items, const uint8_t batch_seed[32], bpg_status *status_out) {
    return verify_batch(ctx, count, items, batch_seed, status_out, nullptr, nullptr);
}
bpg_status bpg_test_verify_batch_scripted(bpg_ctx *ctx, uint64_t count, const bpg_verify_item *items, const uint8_t *const *scripts, const uint64_t *script_lens,
                                          const uint8_t batch_seed[32], bpg_status *status_out) {
    if (count && (!scripts || !script_lens)) { g_last_error = "null or invalid argument: scripts and script_lens"; return BPG_ERR_INVALID_ARGUMENT; }
    return verify_batch(ctx, count, items, batch_seed, status_out, count ? scripts : nullptr, script_lens);
}

// K proofs of ONE resident circuit in lockstep launches (Engine::verify_resident_batch).  Every argument first: a refused call launches nothing and touches
// neither status_out nor a transcript state
bpg_status bpg_r1cs_verify_resident_batch(bpg_ctx *ctx, bpg_circuit *c, uint64_t count, const bpg_verify_resident_item *items, const uint8_t batch_seed[32],
                                          bpg_status *status_out) {
    return guard([&] {
        const std::string fn = "verify_resident_batch: ";
        if (!c) throw std::invalid_argument(fn + "null circuit");
        if (count && (!items || !status_out || !batch_seed)) throw std::invalid_argument(fn + "null items, status_out or batch_seed with count > 0");
        if (count > (1ull << 32)) throw std::invalid_argument(fn + "more than 2^32 items");
        for (uint64_t k = 0; k < count; k++) {
            const bpg_verify_resident_item &it = items[k];
            const char *what = !it.transcript_state ? "transcript_state" : !it.proof ? "proof" : !it.seed ? "seed" : (c->m && !it.V) ? "V" : nullptr;
            if (what) throw std::invalid_argument(fn + "item " + std::to_string(k) + ": null " + what);
        }
        if (!c->dc) throw std::invalid_argument(fn + "the handle has no device state (bpg_test_circuit_handle)");
        REQUIRE(ctx);
        std::vector<Transcript> T(count);
        std::vector<Engine::ResidentVerifyItem> ei(count);
        for (uint64_t k = 0; k < count; k++) {
            const bpg_verify_resident_item &it = items[k];
            Engine::ResidentVerifyItem &e = ei[k];
            e.V = it.V; e.proof = it.proof; e.proof_len = it.proof_len; e.seed = it.seed; e.flags = it.flags; e.params = it.param_values; e.inputs = it.input_values;
        }
        ctx->engine->check_resident_batch(c->dc, count, ei.data());            // another context or device, constants the circuit cannot take
        if (!count) return;
        for (uint64_t k = 0; k < count; k++) { T[k] = Transcript::from_state(items[k].transcript_state); ei[k].T = &T[k]; }
        std::vector<R1CSError> st(count);
        ctx->engine->verify_resident_batch(c->dc, count, ei.data(), batch_seed, st.data());
        uint64_t first = count;
        for (uint64_t k = 0; k < count; k++) {
            T[k].export_state(items[k].transcript_state);
            status_out[k] = (bpg_status)st[k];
            if (first == count && st[k] != R1CSError::None) first = k;
        }
        if (first < count) {
            const R1CSError e = st[first];
            throw R1CSException(e, "item " + std::to_string(first) + ": " + (e == R1CSError::VerificationError ? "proof rejected" : e == R1CSError::FormatError ? "malformed proof" : "generator capacity below padded circuit size"));
        }
    });
}
bpg_status bpg_test_verify_wave_scalars(bpg_ctx *ctx, bpg_circuit *c, uint64_t count, const uint8_t *challenges, const uint8_t *param_values, const uint8_t *input_values,
                                        uint8_t *g_out, uint8_t *h_out, uint8_t *small_out, char *evidence, uint64_t cap) {
    return guard([&] {
        if (!ctx) throw DeviceError("test_verify_wave_scalars: no device context (the wave runs on the GPU only)");
        REQUIRE(c && challenges && g_out && h_out && small_out && evidence);
        if (!c->dc) throw std::invalid_argument("test_verify_wave_scalars: the handle has no device state (bpg_test_circuit_handle)");
        if (cap < 1024) throw std::invalid_argument("test_verify_wave_scalars: evidence buffer too small (1024 bytes needed)");
        const std::string r = ctx->engine->test_verify_wave_scalars(c->dc, count, challenges, param_values, input_values, g_out, h_out, small_out);
        if (r.size() + 1 > cap) throw std::invalid_argument("test_verify_wave_scalars: evidence buffer too small (" + std::to_string(r.size() + 1) + " bytes needed)");
        std::memcpy(evidence, r.c_str(), r.size() + 1);
    });
}

// ---------------------------------------------------------------------------------------- batch pool
struct bpg_pool { std::vector<bpg_ctx *> ctxs; };
bpg_status bpg_pool_create(int32_t device, uint32_t workers, uint64_t gens_capacity, bpg_pool **out) { return bpg_pool_create_ex(device, workers, gens_capacity, nullptr, out); }
bpg_status bpg_pool_create_ex(int32_t device, uint32_t workers, uint64_t gens_capacity, const bpg_config *config, bpg_pool **out) {
    if (!out) return BPG_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    if (workers < 1 || workers > 64) { g_last_error = "pool: 1..64 workers"; return BPG_ERR_INVALID_ARGUMENT; }
    bpg_pool *pool = new bpg_pool();
    for (uint32_t k = 0; k < workers; k++) {
        bpg_ctx *c = nullptr;
        bpg_status s = bpg_ctx_create_ex(device, config, &c);
        if (s == BPG_OK && gens_capacity) s = bpg_gens_ensure(c, gens_capacity);
        if (s != BPG_OK) { std::string keep = g_last_error; if (c) bpg_ctx_destroy(c); bpg_pool_destroy(pool); g_last_error = keep; return s; }
        pool->ctxs.push_back(c);
    }
    *out = pool;
    return BPG_OK;
}
void bpg_pool_destroy(bpg_pool *pool) {
    if (!pool) return;
    for (bpg_ctx *c : pool->ctxs) bpg_ctx_destroy(c);
    delete pool;
}
bpg_status bpg_pool_prove(bpg_pool *pool, uint64_t count, const bpg_batch_item *items, bpg_status *status_out) {
    if (!pool || (count && !items)) return BPG_ERR_INVALID_ARGUMENT;
    std::atomic<uint64_t> next(0);
    std::vector<bpg_status> st(count, BPG_OK);
    std::vector<std::string> msg(count);
    auto work = [&](bpg_ctx *ctx) {
        for (;;) {
            const uint64_t i = next.fetch_add(1);
            if (i >= count) return;
            const bpg_batch_item &it = items[i];
            st[i] = (it.inst && it.transcript_state && it.rng_seed && it.proof_out && it.proof_len)
                        ? bpg_r1cs_prove(ctx, it.inst, it.transcript_state, it.m, it.v_blinding, it.rng_seed, it.flags, it.proof_out, it.proof_len)
                        : BPG_ERR_INVALID_ARGUMENT;
            if (st[i] != BPG_OK) msg[i] = g_last_error;            // g_last_error is per thread
        }
    };
    std::vector<std::thread> th;
    const size_t nthreads = std::min<uint64_t>(pool->ctxs.size(), count);
    for (size_t k = 1; k < nthreads; k++) th.emplace_back(work, pool->ctxs[k]);
    if (nthreads) work(pool->ctxs[0]);
    for (std::thread &t : th) t.join();
    bpg_status first = BPG_OK;
    for (uint64_t i = 0; i < count; i++) {
        if (status_out) status_out[i] = st[i];
        if (first == BPG_OK && st[i] != BPG_OK) { first = st[i]; g_last_error = "item " + std::to_string(i) + ": " + msg[i]; }
    }
    return first;
}

// ---------------------------------------------------------------------------------------- transcript
bpg_status bpg_transcript_new(const uint8_t *label, uint64_t len, bpg_transcript **out) {
    return guard([&] { REQUIRE(out && (len == 0 || label)); *out = new bpg_transcript{Transcript(label, len)}; });
}
void bpg_transcript_free(bpg_transcript *t) { delete t; }
bpg_status bpg_transcript_append_message(bpg_transcript *t, const char *label, const uint8_t *msg, uint64_t len) {
    return guard([&] { REQUIRE(t && label && (len == 0 || msg)); t->t.append_message(label, msg, len); });
}
bpg_status bpg_transcript_challenge_bytes(bpg_transcript *t, const char *label, uint8_t *out, uint64_t len) {
    return guard([&] { REQUIRE(t && label && out); t->t.challenge_bytes(label, out, len); });
}
bpg_status bpg_transcript_state(const bpg_transcript *t, uint8_t out[BPG_TRANSCRIPT_STATE_BYTES]) { return guard([&] { REQUIRE(t && out); t->t.export_state(out); }); }

// ---------------------------------------------------------------------------------------- prover / verifier
bpg_status bpg_prover_new(bpg_ctx *ctx, bpg_transcript *t, bpg_prover **out) {
    // ctx may be NULL: an assembly-only prover (multiply / constrain / witness synthesis); commit() and prove() then fail with BPG_ERR_DEVICE
    return guard([&] { REQUIRE(t && out); bpg_prover *p = new bpg_prover(); p->p = new Prover(ctx ? ctx->engine : nullptr, &t->t); *out = p; });
}
void bpg_prover_free(bpg_prover *p) { if (p) { delete p->p; delete p; } }
bpg_status bpg_test_prover_stub_commitments(bpg_prover *p) { return guard([&] { REQUIRE(p); p->p->test_stub_commitments(); }); }
bpg_status bpg_prover_commit(bpg_prover *p, const uint8_t v[32], const uint8_t blind[32], uint8_t com_out[32], uint32_t *var_out) {
    return bpg_prover_commit_many(p, 1, v, blind, com_out, var_out);
}
bpg_status bpg_prover_commit_many(bpg_prover *p, uint64_t k, const uint8_t *v, const uint8_t *blind, uint8_t *coms_out, uint32_t *vars_out) {
    return guard([&] {
        REQUIRE(p && (k == 0 || (v && blind && coms_out)));
        std::vector<Scalar> vs(k), bs(k);
        for (uint64_t i = 0; i < k; i++) { vs[i] = Scalar::from_bits(v + 32 * i); bs[i] = Scalar::from_bytes_mod_order(blind + 32 * i); }
        std::vector<uint8_t> coms;
        std::vector<Variable> vars = p->p->commit_many(vs, bs, coms);
        if (k) std::memcpy(coms_out, coms.data(), k * 32);
        if (vars_out) for (uint64_t i = 0; i < k; i++) vars_out[i] = vars[i].packed();
    });
}
bpg_status bpg_prover_defer_commitments(bpg_prover *p, int32_t on) { return guard([&] { REQUIRE(p); p->p->defer_commitments(on != 0); }); }
bpg_status bpg_prover_flush_commitments(bpg_prover *p) { return guard([&] { REQUIRE(p); p->p->flush_commitments(); }); }
bpg_status bpg_prover_commitment(bpg_prover *p, uint64_t index, uint8_t out[32]) {
    return guard([&] {
        REQUIRE(p && out);
        if (index >= p->p->num_flushed()) throw std::invalid_argument("commitment: no such committed variable (or its commitment is still deferred)");
        std::memcpy(out, p->p->commitment(index), 32);
    });
}
bpg_status bpg_prover_commit_precomputed(bpg_prover *p, const uint8_t v[32], const uint8_t blind[32], const uint8_t com[32], uint32_t *var_out) {
    return guard([&] {
        REQUIRE(p && v && blind && com);
        const Variable var = p->p->commit_precomputed(Scalar::from_bits(v), Scalar::from_bytes_mod_order(blind), com);
        if (var_out) *var_out = var.packed();
    });
}
uint64_t bpg_prover_num_constraints(const bpg_prover *p) { return p ? p->p->num_constraints() : 0; }
uint64_t bpg_prover_num_multiplications(const bpg_prover *p) { return p ? p->p->get_num_multiplications() : 0; }
uint64_t bpg_prover_num_committed(const bpg_prover *p) { return p ? p->p->num_committed() : 0; }

static void put_vars(const MulVars &mv, uint32_t out[3]) { if (out) { out[0] = mv.l.packed(); out[1] = mv.r.packed(); out[2] = mv.o.packed(); } }
bpg_status bpg_prover_multiply(bpg_prover *p, const bpg_lc *left, const bpg_lc *right, uint32_t vars_out[3]) {
    return guard([&] { REQUIRE(p); put_vars(p->p->multiply(lc_from(left), lc_from(right)), vars_out); });
}
bpg_status bpg_prover_allocate_multiplier(bpg_prover *p, int32_t has, const uint8_t l[32], const uint8_t r[32], uint32_t vars_out[3]) {
    return guard([&] {
        REQUIRE(p && (!has || (l && r)));
        Scalar a, b; if (has) { a = Scalar::from_bits(l); b = Scalar::from_bits(r); }
        put_vars(p->p->allocate_multiplier(has != 0, a, b), vars_out);
    });
}
bpg_status bpg_prover_allocate(bpg_prover *p, int32_t has, const uint8_t s[32], uint32_t *var_out) {
    return guard([&] { REQUIRE(p && (!has || s)); Variable v = p->p->allocate(has ? OptScalar(Scalar::from_bits(s)) : OptScalar()); if (var_out) *var_out = v.packed(); });
}
bpg_status bpg_prover_constrain(bpg_prover *p, const bpg_lc *lc) { return guard([&] { REQUIRE(p); p->p->constrain(lc_from(lc)); }); }

bpg_status bpg_prover_instance(bpg_prover *p, bpg_r1cs_instance *out, const uint8_t **v_out, const uint8_t **vb_out) {
    return guard([&] {
        REQUIRE(p && out);
        p->p->flush_commitments();
        p->flat = p->p->flatten();
        view(p->flat, out);
        const size_t m = p->p->num_committed();
        p->v_bytes.resize(m * 32 + 1); p->vb_bytes.resize(m * 32 + 1);
        for (size_t i = 0; i < m; i++) { p->p->v()[i].to_bytes(&p->v_bytes[32 * i]); p->p->v_blinding()[i].to_bytes(&p->vb_bytes[32 * i]); }
        if (v_out) *v_out = p->v_bytes.data();
        if (vb_out) *vb_out = p->vb_bytes.data();
    });
}

bpg_status bpg_prover_input(bpg_prover *p, const uint8_t value[32], uint32_t *var_out) {
    return guard([&] { REQUIRE(p && value); const Variable x = p->p->input(Scalar::from_bits(value)); if (var_out) *var_out = x.packed(); });
}
bpg_status bpg_prover_gate(bpg_prover *p, uint32_t x, uint32_t var, uint32_t *var_out) {
    return guard([&] { REQUIRE(p); const Variable g = p->p->gate(Variable::unpack(x), Variable::unpack(var)); if (var_out) *var_out = g.packed(); });
}
bpg_status bpg_prover_gates(bpg_prover *p, bpg_witness_gates *out) {
    return guard([&] {
        REQUIRE(p && out);
        p->gate_var.clear(); p->gate_input.clear();
        for (auto &g : p->p->gates()) { p->gate_var.push_back(g.first); p->gate_input.push_back(g.second); }
        p->gate_var.push_back(0); p->gate_input.push_back(0);       // (never a null pointer)
        out->n_gates = p->p->gates().size(); out->gate_var = p->gate_var.data(); out->gate_input = p->gate_input.data();
    });
}
bpg_status bpg_prover_template_instance(bpg_prover *p, bpg_r1cs_instance *out, const uint8_t **v_out, const uint8_t **vb_out, uint64_t *n_inputs_out,
                                        const uint8_t **inputs_out) {
    return guard([&] {
        REQUIRE(p && out && n_inputs_out && inputs_out);
        p->p->flush_commitments();
        p->flat = p->p->flatten(true);
        view(p->flat, out);
        const size_t m = p->p->num_committed(), ni = p->p->inputs().size();
        p->v_bytes.resize(m * 32 + 1); p->vb_bytes.resize(m * 32 + 1); p->in_bytes.resize(ni * 32 + 1);
        for (size_t i = 0; i < m; i++) { p->p->v()[i].to_bytes(&p->v_bytes[32 * i]); p->p->v_blinding()[i].to_bytes(&p->vb_bytes[32 * i]); }
        for (size_t i = 0; i < ni; i++) p->p->inputs()[i].to_bytes(&p->in_bytes[32 * i]);
        if (v_out) *v_out = p->v_bytes.data();
        if (vb_out) *vb_out = p->vb_bytes.data();
        *n_inputs_out = ni; *inputs_out = p->in_bytes.data();
    });
}

static void put_program(const WitnessProgram &w, bpg_witness_program *out) {
    out->lc_ptr = w.lc_ptr.data(); out->term_var = w.term_var.data(); out->term_coef = w.term_coef.data();
    out->n_params = w.param_rows.size(); out->param_rows = w.param_rows.data();
}
bpg_status bpg_prover_witness_program(bpg_prover *p, bpg_witness_program *out) {
    return guard([&] {
        REQUIRE(p && out);
        p->program = p->p->witness_program();
        put_program(p->program, out);
    });
}
bpg_status bpg_prover_witness_program_hinted(bpg_prover *p, bpg_witness_program *program_out, bpg_witness_hints *hints_out) {
    return guard([&] {
        REQUIRE(p && program_out && hints_out);
        p->program = p->p->witness_program(true);
        put_program(p->program, program_out);
        hints_out->n_hints = p->program.hint_mul.size(); hints_out->hint_mul = p->program.hint_mul.data();
        hints_out->hint_kind = p->program.hint_kind.data(); hints_out->hint_arg = p->program.hint_arg.data();
    });
}
bpg_status bpg_prover_noted(bpg_prover *p, uint32_t *vars_out, uint32_t *tags_out, uint64_t cap, uint64_t *n_out) {
    return guard([&] {
        REQUIRE(p && n_out);
        const std::vector<uint32_t> &vars = p->p->noted_vars(), &tags = p->p->noted_tags();
        *n_out = vars.size();
        REQUIRE(cap == 0 || (vars_out && tags_out));
        const uint64_t k = std::min<uint64_t>(cap, vars.size());
        if (k) { std::memcpy(vars_out, vars.data(), k * 4); std::memcpy(tags_out, tags.data(), k * 4); }
    });
}
bpg_status bpg_prover_allocate_bit(bpg_prover *p, const bpg_lc *source, uint32_t bit, const uint8_t source_value[32], uint32_t vars_out[3]) {
    return guard([&] { REQUIRE(p && source_value && bit < 256); put_vars(p->p->allocate_bit(lc_from(source), bit, OptScalar(Scalar::from_bits(source_value))), vars_out); });
}
bpg_status bpg_prover_mark_param_row(bpg_prover *p, uint64_t row) { return guard([&] { REQUIRE(p); p->p->mark_param_row(row); }); }

bpg_status bpg_prover_start_blinding(bpg_prover *p, const uint8_t seed[32], uint64_t max_multipliers) {
    return guard([&] { REQUIRE(p && seed); p->p->start_blinding(seed, max_multipliers); });
}

bpg_status bpg_blinding_begin(bpg_ctx *ctx, const uint8_t transcript_state[203], uint64_t m, const uint8_t *v_blinding, const uint8_t seed[32], uint64_t max_multipliers) {
    return guard([&] {
        REQUIRE(ctx && transcript_state && seed && (v_blinding || m == 0));
        std::vector<Scalar> vb(m);
        for (uint64_t i = 0; i < m; i++) vb[i] = Scalar::from_bytes_mod_order(v_blinding + 32 * i);
        ctx->engine->blinding_begin(Transcript::from_state(transcript_state), vb, seed, max_multipliers);
    });
}

bpg_status bpg_ctx_set_chain_workers(bpg_ctx *ctx, uint32_t workers) { return guard([&] { REQUIRE(ctx); ctx->engine->set_chain_workers(workers); }); }
bpg_status bpg_ctx_set_chain_lanes(bpg_ctx *ctx, uint32_t lanes) { return guard([&] { REQUIRE(ctx); ctx->engine->set_chain_lanes(lanes); }); }
int32_t bpg_chain_cpu(bpg_ctx *ctx) { return ctx ? ctx->engine->chain_cpu() : -1; }
struct bpg_chain_pool { ChainPool *pool; };
bpg_status bpg_chain_pool_create(uint32_t threads, const uint32_t *lanes, bpg_chain_pool **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(threads >= 1 && threads <= 256);
        std::vector<uint32_t> l(threads, 1u);
        if (lanes) l.assign(lanes, lanes + threads);
        *out = new bpg_chain_pool{new ChainPool(l)};
    });
}
void bpg_chain_pool_destroy(bpg_chain_pool *pool) { if (pool) { delete pool->pool; delete pool; } }
bpg_status bpg_ctx_attach_chain_pool(bpg_ctx *ctx, bpg_chain_pool *pool, uint32_t max_streams) {
    return guard([&] { REQUIRE(ctx); ctx->engine->attach_chain_pool(pool ? pool->pool : nullptr, pool ? max_streams : 1u); });
}

bpg_status bpg_prover_prove(bpg_prover *p, uint64_t gens_capacity, const uint8_t seed[32], uint32_t flags, uint8_t *proof_out, uint64_t *proof_len, bpg_timings *timings) {
    return guard([&] {
        REQUIRE(p && seed && proof_out && proof_len);
        if (*proof_len < bpg_proof_size(p->p->get_num_multiplications(), flags)) throw std::invalid_argument("prove: proof buffer too small");
        (void)timings;
        std::vector<uint8_t> proof = p->p->prove(gens_capacity, seed, flags);
        std::memcpy(proof_out, proof.data(), proof.size()); *proof_len = proof.size();
    });
}

bpg_status bpg_verifier_new(bpg_transcript *t, bpg_verifier **out) {
    return guard([&] { REQUIRE(t && out); bpg_verifier *v = new bpg_verifier(); v->v = new Verifier(&t->t); *out = v; });
}
void bpg_verifier_free(bpg_verifier *v) { if (v) { delete v->v; delete v; } }
bpg_status bpg_verifier_commit(bpg_verifier *v, const uint8_t com[32], uint32_t *var_out) {
    return guard([&] { REQUIRE(v && com); Variable x = v->v->commit(com); if (var_out) *var_out = x.packed(); });
}
bpg_status bpg_verifier_input(bpg_verifier *v, const uint8_t value[32], uint32_t *var_out) {
    return guard([&] { REQUIRE(v && value); const Variable x = v->v->input(Scalar::from_bits(value)); if (var_out) *var_out = x.packed(); });
}
bpg_status bpg_verifier_gate(bpg_verifier *v, uint32_t x, uint32_t var, uint32_t *var_out) {
    return guard([&] { REQUIRE(v); const Variable g = v->v->gate(Variable::unpack(x), Variable::unpack(var)); if (var_out) *var_out = g.packed(); });
}
uint64_t bpg_verifier_num_vars(const bpg_verifier *v) { return v ? v->v->get_num_vars() : 0; }
bpg_status bpg_verifier_instance(bpg_verifier *v, bpg_r1cs_instance *out, const uint8_t **commitments_out) {
    return guard([&] { REQUIRE(v && out); v->flat = v->v->flatten(); view(v->flat, out); if (commitments_out) *commitments_out = v->v->commitments().data(); });
}

bpg_status bpg_verifier_verify(bpg_verifier *v, bpg_ctx *ctx, uint64_t gens_capacity, const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags) {
    return guard([&] {
        REQUIRE(v && ctx && proof && seed);
        ctx->engine->gens_ensure(gens_capacity);
        require_gens_capacity(gens_capacity, v->v->get_num_vars());
        FlatCircuit f = v->v->flatten();
        DeviceCircuit *dc = ctx->engine->upload(f);
        R1CSError e;
        try { e = ctx->engine->verify(dc, *v->v->transcript(), v->v->commitments().data(), proof, proof_len, seed, flags); } catch (...) { ctx->engine->free_circuit(dc); throw; }
        ctx->engine->free_circuit(dc);
        if (e != R1CSError::None) throw R1CSException(e, e == R1CSError::VerificationError ? "proof rejected" : e == R1CSError::FormatError ? "malformed proof" : "generator capacity below padded circuit size");
    });
}

// ---------------------------------------------------------------------------------------- gadgets
bpg_status bpg_bounds_check_new(const uint8_t *min_be, uint64_t min_len, const uint8_t *max_be, uint64_t max_len, bpg_gadget **out) {
    return guard([&] {
        REQUIRE(out && min_be && max_be);
        if (min_len > 32 || max_len > 32) throw std::invalid_argument("the given vector is longer than 32 bytes");
        *out = new bpg_gadget{std::unique_ptr<Gadget>(new BoundsCheck(Bytes(min_be, min_be + min_len), Bytes(max_be, max_be + max_len)))};
    });
}
bpg_status bpg_mimc_hash256_new(const bpg_lc *image, bpg_gadget **out) {
    return guard([&] { REQUIRE(out); *out = new bpg_gadget{std::unique_ptr<Gadget>(new MimcHash256(lc_from(image)))}; });
}
bpg_status bpg_merkle_tree256_new(const bpg_lc *root, const bpg_lc *inst, uint64_t n_inst, const bpg_lc *wit, uint64_t n_wit, const char *pattern, bpg_gadget **out) {
    return guard([&] {
        REQUIRE(out && pattern && (n_inst == 0 || inst) && (n_wit == 0 || wit));
        std::vector<LinearCombination> iv, wv;
        for (uint64_t i = 0; i < n_inst; i++) iv.push_back(lc_from(&inst[i]));
        for (uint64_t i = 0; i < n_wit; i++) wv.push_back(lc_from(&wit[i]));
        *out = new bpg_gadget{std::unique_ptr<Gadget>(new MerkleTree256(lc_from(root), iv, wv, Pattern::parse(pattern)))};
    });
}
bpg_status bpg_merkle_path256_new(const bpg_lc *root, uint32_t leaf, const uint32_t *levels, uint64_t depth, bpg_gadget **out) {
    return guard([&] {
        REQUIRE(out && (depth == 0 || levels));
        if (depth > Pattern::MAX_DEPTH) throw std::invalid_argument("MerklePath256: deeper than 64 levels");
        std::vector<MerklePath256::Level> lv;
        for (uint64_t j = 0; j < depth; j++)
            lv.push_back({Variable::unpack(levels[4 * j]), Variable::unpack(levels[4 * j + 1]), Variable::unpack(levels[4 * j + 2]), Variable::unpack(levels[4 * j + 3])});
        *out = new bpg_gadget{std::unique_ptr<Gadget>(new MerklePath256(lc_from(root), Variable::unpack(leaf), lv))};
    });
}
bpg_status bpg_merkle_path_inputs(uint64_t index, const uint8_t *siblings, uint64_t depth, const uint8_t root[32], uint8_t *inputs_out) {
    return guard([&] {
        REQUIRE(root && inputs_out && (depth == 0 || siblings));
        if (depth > Pattern::MAX_DEPTH) throw std::invalid_argument("merkle_path_inputs: deeper than 64 levels");
        std::vector<Scalar> sib(depth);
        for (uint64_t j = 0; j < depth; j++) sib[j] = Scalar::from_bits(siblings + 32 * j);
        const std::vector<Scalar> in = merkle_path_inputs(index, sib, Scalar::from_bits(root));
        for (size_t k = 0; k < in.size(); k++) std::memcpy(inputs_out + 32 * k, in[k].as_bytes(), 32);
    });
}
static std::vector<LinearCombination> lcs_from(const bpg_lc *a, uint64_t n) { std::vector<LinearCombination> o; for (uint64_t i = 0; i < n; i++) o.push_back(lc_from(&a[i])); return o; }
static std::vector<Scalar> scalars_from(const uint8_t *p, uint64_t n) { std::vector<Scalar> o; if (p) for (uint64_t i = 0; i < n; i++) o.push_back(Scalar::from_bits(p + 32 * i)); return o; }
bpg_status bpg_equality_new(const bpg_lc *right, uint64_t n, bpg_gadget **out) {
    return guard([&] { REQUIRE(out && (n == 0 || right)); *out = new bpg_gadget{std::unique_ptr<Gadget>(new Equality(lcs_from(right, n)))}; });
}
bpg_status bpg_inequality_new(const bpg_lc *right, uint64_t n, const uint8_t *ra, bpg_gadget **out) {
    return guard([&] { REQUIRE(out && (n == 0 || right)); *out = new bpg_gadget{std::unique_ptr<Gadget>(new Inequality(lcs_from(right, n), ra != nullptr, scalars_from(ra, n)))}; });
}
bpg_status bpg_less_than_new(const bpg_lc *left, const uint8_t *la, const bpg_lc *right, const uint8_t *ra, bpg_gadget **out) {
    return guard([&] {
        REQUIRE(out);
        *out = new bpg_gadget{std::unique_ptr<Gadget>(new LessThan(lc_from(left), la ? OptScalar(Scalar::from_bits(la)) : OptScalar(), lc_from(right),
                                                                   ra ? OptScalar(Scalar::from_bits(ra)) : OptScalar()))};
    });
}
bpg_status bpg_set_membership_new(const bpg_lc *value, const uint8_t *va, const bpg_lc *inst, uint64_t n_inst, const uint8_t *ia, bpg_gadget **out) {
    return guard([&] {
        REQUIRE(out && (n_inst == 0 || inst));
        *out = new bpg_gadget{std::unique_ptr<Gadget>(new SetMembership(lc_from(value), va ? OptScalar(Scalar::from_bits(va)) : OptScalar(), lcs_from(inst, n_inst),
                                                                        ia != nullptr || n_inst == 0, scalars_from(ia, n_inst)))};
    });
}
void bpg_gadget_free(bpg_gadget *g) { delete g; }

bpg_status bpg_gadget_setup(bpg_gadget *g, bpg_prover *p, const uint8_t *wit, uint64_t n_wit, const uint8_t *blind, uint64_t n_blind,
                            uint8_t *coms_out, uint8_t *derived_scalars_out, uint32_t *derived_vars_out, uint64_t *n_derived) {
    return guard([&] {
        REQUIRE(g && p && n_derived && (n_wit == 0 || wit) && (n_blind == 0 || blind));
        std::vector<Scalar> w(n_wit), b(n_blind);
        for (uint64_t i = 0; i < n_wit; i++) w[i] = Scalar::from_bits(wit + 32 * i);
        for (uint64_t i = 0; i < n_blind; i++) b[i] = Scalar::from_bytes_mod_order(blind + 32 * i);
        if (g->g->preprocess(w).size() > *n_derived) throw std::invalid_argument("setup: output capacity too small");
        auto r = g->g->setup(*p->p, w, b);
        const size_t k = r.second.size();
        if (k) { REQUIRE(coms_out && derived_scalars_out && derived_vars_out); std::memcpy(coms_out, r.first.data(), k * 32); }
        for (size_t i = 0; i < k; i++) { r.second[i].first.v.to_bytes(derived_scalars_out + 32 * i); derived_vars_out[i] = r.second[i].second.packed(); }
        *n_derived = k;
    });
}
bpg_status bpg_gadget_preprocess(bpg_gadget *g, const uint8_t *wit, uint64_t n_wit, uint8_t *derived_scalars_out, uint64_t *n_derived) {
    return guard([&] {
        REQUIRE(g && n_derived && (n_wit == 0 || wit));
        std::vector<Scalar> w(n_wit);
        for (uint64_t i = 0; i < n_wit; i++) w[i] = Scalar::from_bits(wit + 32 * i);
        const std::vector<Scalar> d = g->g->preprocess(w);
        if (d.size() > *n_derived) throw std::invalid_argument("preprocess: output capacity too small");
        if (!d.empty()) REQUIRE(derived_scalars_out);
        for (size_t i = 0; i < d.size(); i++) d[i].to_bytes(derived_scalars_out + 32 * i);
        *n_derived = d.size();
    });
}
static std::vector<Variable> unpack_vars(const uint32_t *v, uint64_t n) { std::vector<Variable> o; for (uint64_t i = 0; i < n; i++) o.push_back(Variable::unpack(v[i])); return o; }
bpg_status bpg_gadget_prove(bpg_gadget *g, bpg_prover *p, const uint32_t *vars, uint64_t n_vars, const uint8_t *dsc, const uint32_t *dvars, uint64_t n_derived) {
    return guard([&] {
        REQUIRE(g && p && (n_vars == 0 || vars) && (n_derived == 0 || (dsc && dvars)));
        Derived d;
        for (uint64_t i = 0; i < n_derived; i++) d.emplace_back(OptScalar(Scalar::from_bits(dsc + 32 * i)), Variable::unpack(dvars[i]));
        g->g->prove(*p->p, unpack_vars(vars, n_vars), d);
    });
}
bpg_status bpg_gadget_verify(bpg_gadget *g, bpg_verifier *v, const uint32_t *vars, uint64_t n_vars, const uint32_t *dvars, uint64_t n_derived) {
    return guard([&] {
        REQUIRE(g && v && (n_vars == 0 || vars) && (n_derived == 0 || dvars));
        g->g->verify(*v->v, unpack_vars(vars, n_vars), unpack_vars(dvars, n_derived));
    });
}
bpg_status bpg_buffer_new(uint64_t first, int32_t prover_side, bpg_buffer **out) { return guard([&] { REQUIRE(out); *out = new bpg_buffer{OpBuffer(first, prover_side != 0)}; }); }
void bpg_buffer_free(bpg_buffer *b) { delete b; }
bpg_status bpg_buffer_rewind(bpg_buffer *b) { return guard([&] { REQUIRE(b); b->b.rewind(); }); }
uint64_t bpg_buffer_next_multiplier(const bpg_buffer *b) { return b ? b->b.next_multiplier() : 0; }
bpg_status bpg_gadget_prove_buffered(bpg_gadget *g, bpg_buffer *b, const uint32_t *vars, uint64_t n_vars, const uint8_t *dsc, const uint32_t *dvars, uint64_t n_derived) {
    return guard([&] {
        REQUIRE(g && b && (n_vars == 0 || vars) && (n_derived == 0 || (dsc && dvars)));
        Derived d;
        for (uint64_t i = 0; i < n_derived; i++) d.emplace_back(OptScalar(Scalar::from_bits(dsc + 32 * i)), Variable::unpack(dvars[i]));
        g->g->prove(b->b, unpack_vars(vars, n_vars), d);
    });
}
bpg_status bpg_gadget_verify_buffered(bpg_gadget *g, bpg_buffer *b, const uint32_t *vars, uint64_t n_vars, const uint32_t *dvars, uint64_t n_derived) {
    return guard([&] { REQUIRE(g && b && (n_vars == 0 || vars) && (n_derived == 0 || dvars)); g->g->verify(b->b, unpack_vars(vars, n_vars), unpack_vars(dvars, n_derived)); });
}
bpg_status bpg_or_prover(bpg_prover *main, const bpg_buffer *b) { return guard([&] { REQUIRE(main && b); or_conjunction(*main->p, b->b); }); }
bpg_status bpg_or_verifier(bpg_verifier *main, const bpg_buffer *b) { return guard([&] { REQUIRE(main && b); or_conjunction(*main->v, b->b); }); }
bpg_status bpg_or_buffer(bpg_buffer *parent, const bpg_buffer *b) { return guard([&] { REQUIRE(parent && b); or_conjunction(parent->b, b->b); }); }
bpg_status bpg_range_proof_prove(bpg_prover *p, const bpg_lc *x, uint32_t n_bits, const uint8_t a[32]) {
    return guard([&] { REQUIRE(p && a && n_bits <= 255); range_proof(*p->p, lc_from(x), (uint8_t)n_bits, OptScalar(Scalar::from_bits(a))); });
}
bpg_status bpg_range_proof_verify(bpg_verifier *v, const bpg_lc *x, uint32_t n_bits) {
    return guard([&] { REQUIRE(v && n_bits <= 255); range_proof(*v->v, lc_from(x), (uint8_t)n_bits, OptScalar()); });
}
bpg_status bpg_mimc_hash(const uint8_t *pre, uint64_t len, uint8_t out[32]) {
    return guard([&] { REQUIRE(pre && out && len > 0); mimc_hash(Bytes(pre, pre + len)).to_bytes(out); });
}
bpg_status bpg_mimc_sponge(const uint8_t *blocks, uint64_t n_blocks, uint8_t out[32]) {
    return guard([&] {
        REQUIRE(blocks && out && n_blocks > 0);
        std::vector<Scalar> pre(n_blocks);
        for (uint64_t i = 0; i < n_blocks; i++) std::memcpy(pre[i].w, blocks + 32 * i, 32);     // all 256 bits: `state += b` reduces them
        mimc_sponge_1(pre, mimc_round_constants()).to_bytes(out);
    });
}
bpg_status bpg_mimc_sponge_states(const uint8_t *blocks, uint64_t n_blocks, uint8_t *out) {
    return guard([&] {
        REQUIRE(blocks && out && n_blocks > 0);
        const std::vector<Scalar> &rc = mimc_round_constants();
        Scalar state;
        for (uint64_t i = 0; i < n_blocks; i++) {                 // mimc_sponge_1, keeping the state after every block
            Scalar b; std::memcpy(b.w, blocks + 32 * i, 32);
            state += b; state = mimc_encryption(state, Scalar::zero(), rc);
            state.to_bytes(out + 32 * i);
        }
    });
}
// ---- MiMC Merkle trees on the device: the arguments that need no tree are checked here, the rest by the engine, all of it before the device is touched
bpg_status bpg_mimc_sponge_many(bpg_ctx *ctx, uint64_t count, uint64_t blocks_per_item, const uint8_t *in, uint8_t *out) {
    return guard([&] { REQUIRE(count > 0 && blocks_per_item > 0 && blocks_per_item <= (1ull << 22) && in && out && ctx); ctx->engine->mimc_sponge_many(count, blocks_per_item, in, out); });
}
bpg_status bpg_merkle_build(bpg_ctx *ctx, uint32_t depth, const uint8_t *leaves, bpg_merkle **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(depth >= 1 && depth <= 24 && leaves && ctx);
        std::unique_ptr<bpg_merkle> h(new bpg_merkle{nullptr});
        h->t = ctx->engine->merkle_build(depth, leaves);
        *out = h.release();
    });
}
bpg_status bpg_merkle_build_partial(bpg_ctx *ctx, uint32_t depth, uint64_t size, const uint8_t *leaves, const uint8_t empty[32], bpg_merkle **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(depth >= 1 && depth <= 24 && size <= (1ull << depth) && (leaves || size == 0));       // the arguments first: each is refused whatever the context
        REQUIRE(ctx);
        std::unique_ptr<bpg_merkle> h(new bpg_merkle{nullptr});
        h->t = ctx->engine->merkle_build_partial(depth, size, leaves, empty);
        *out = h.release();
    });
}
bpg_status bpg_merkle_build_prefix(bpg_ctx *ctx, uint32_t depth, uint64_t reserve, uint64_t size, const uint8_t *leaves, const uint8_t empty[32], bpg_merkle **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(depth >= 1 && depth <= 32 && reserve >= 1 && reserve <= (1ull << 24) && reserve <= (1ull << depth) && size <= reserve && (leaves || size == 0));
        REQUIRE(ctx);
        std::unique_ptr<bpg_merkle> h(new bpg_merkle{nullptr});
        h->t = ctx->engine->merkle_build_prefix(depth, reserve, size, leaves, empty);
        *out = h.release();
    });
}
bpg_status bpg_merkle_reserve(bpg_ctx *ctx, bpg_merkle *t, uint64_t leaves) {
    return guard([&] { REQUIRE(leaves <= (1ull << 24)); REQUIRE(ctx && t); ctx->engine->merkle_reserve(t->t, leaves); });
}
bpg_status bpg_merkle_reserved(bpg_ctx *ctx, bpg_merkle *t, uint64_t *reserve_out, uint64_t *bytes_out) {
    return guard([&] { REQUIRE(reserve_out || bytes_out); REQUIRE(ctx && t); ctx->engine->merkle_reserved(t->t, reserve_out, bytes_out); });
}
bpg_status bpg_merkle_append(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint8_t *leaves, uint64_t *first_index_out, uint8_t root_out[32]) {
    return guard([&] { REQUIRE(leaves || count == 0); REQUIRE(ctx && t); ctx->engine->merkle_append(t->t, count, leaves, first_index_out, root_out); });
}
bpg_status bpg_merkle_size(bpg_ctx *ctx, bpg_merkle *t, uint64_t *size_out, uint32_t *depth_out) {
    return guard([&] { REQUIRE(size_out || depth_out); REQUIRE(ctx && t); ctx->engine->merkle_size(t->t, size_out, depth_out); });
}
bpg_status bpg_merkle_empty_nodes(bpg_ctx *ctx, bpg_merkle *t, uint8_t *out) {
    return guard([&] { REQUIRE(out); REQUIRE(ctx && t); ctx->engine->merkle_empty_nodes(t->t, out); });
}
bpg_status bpg_merkle_root(bpg_ctx *ctx, bpg_merkle *t, uint8_t out[32]) { return guard([&] { REQUIRE(ctx && t && out); ctx->engine->merkle_nodes(t->t, 0, 0, 1, out); }); }
bpg_status bpg_merkle_nodes(bpg_ctx *ctx, bpg_merkle *t, uint32_t level, uint64_t first, uint64_t count, uint8_t *out) {
    return guard([&] { REQUIRE(ctx && t && (out || count == 0)); ctx->engine->merkle_nodes(t->t, level, first, count, out); });
}
bpg_status bpg_merkle_paths(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, uint8_t *siblings_out) {
    return guard([&] { REQUIRE(ctx && t && (count == 0 || (indices && siblings_out))); ctx->engine->merkle_paths(t->t, count, indices, siblings_out); });
}
bpg_status bpg_merkle_path_nodes(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, uint8_t *out) {
    return guard([&] { REQUIRE(ctx && t && (count == 0 || (indices && out))); ctx->engine->merkle_paths(t->t, count, indices, out, true); });
}
bpg_status bpg_merkle_update(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, const uint8_t *leaves) {
    return guard([&] { REQUIRE(ctx && t && (count == 0 || (indices && leaves))); ctx->engine->merkle_update(t->t, count, indices, leaves); });
}
// ---- keyed trees: depth, pointers, key range, duplicates and the 2^24 bound are checked (and the keys sorted) before the context or the tree is looked at
bpg_status bpg_merkle_build_keyed(bpg_ctx *ctx, uint32_t depth, uint64_t count, const uint64_t *keys, const uint8_t *leaves, const uint8_t empty[32], bpg_merkle **out) {
    return guard([&] {
        REQUIRE(out); *out = nullptr;
        REQUIRE(depth >= 1 && depth <= 32 && count <= (1ull << 24) && count <= (1ull << depth) && ((keys && leaves) || count == 0));
        const std::vector<uint32_t> order = Engine::merkle_key_order(depth, count, keys);
        REQUIRE(ctx);
        std::unique_ptr<bpg_merkle> h(new bpg_merkle{nullptr});
        h->t = ctx->engine->merkle_build_keyed(depth, count, keys, leaves, empty, &order);
        *out = h.release();
    });
}
bpg_status bpg_merkle_put(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *keys, const uint8_t *leaves, uint64_t *inserted_out, uint8_t root_out[32]) {
    return guard([&] {
        REQUIRE(count <= (1ull << 24) && ((keys && leaves) || count == 0));
        const std::vector<uint32_t> order = Engine::merkle_key_order(32, count, keys);         // the tree's own depth is checked once the tree is known to be one
        REQUIRE(ctx && t);
        ctx->engine->merkle_put(t->t, count, keys, leaves, inserted_out, root_out, false, &order);
    });
}
bpg_status bpg_merkle_get(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *keys, uint8_t *leaves_out, uint8_t *held_out) {
    return guard([&] { REQUIRE((keys && leaves_out) || count == 0); REQUIRE(ctx && t); ctx->engine->merkle_get(t->t, count, keys, leaves_out, held_out); });
}
bpg_status bpg_merkle_keys(bpg_ctx *ctx, bpg_merkle *t, uint64_t first, uint64_t count, uint64_t *keys_out) {
    return guard([&] { REQUIRE(keys_out || count == 0); REQUIRE(first <= (1ull << 24) && count <= (1ull << 24)); REQUIRE(ctx && t); ctx->engine->merkle_keys(t->t, first, count, keys_out); });
}
bpg_status bpg_merkle_node_counts(bpg_ctx *ctx, bpg_merkle *t, uint64_t *counts_out, uint64_t *bytes_out) {
    return guard([&] { REQUIRE(counts_out || bytes_out); REQUIRE(ctx && t); ctx->engine->merkle_node_counts(t->t, counts_out, bytes_out); });
}
void bpg_merkle_free(bpg_ctx *ctx, bpg_merkle *t) {
    (void)ctx;                      // the tree knows its context: its memory is released there whatever is passed here
    if (!t) return;
    Engine::merkle_free(t->t);
    delete t;
}
bpg_status bpg_be_to_scalars(const uint8_t *be, uint64_t len, uint8_t *out, uint64_t *n_out) {
    return guard([&] {
        REQUIRE(n_out && (len == 0 || be));
        std::vector<Scalar> s = be_to_scalars(Bytes(be, be + len));
        if (s.size() > *n_out) throw std::invalid_argument("be_to_scalars: output capacity too small");
        for (size_t i = 0; i < s.size(); i++) s[i].to_bytes(out + 32 * i);
        *n_out = s.size();
    });
}
bpg_status bpg_rng_draws(const uint8_t transcript_state[203], uint64_t m, const uint8_t *v_blinding, const uint8_t rng_seed[32],
                         uint64_t skip, uint64_t count, int32_t bulk, uint8_t *out) {
    return guard([&] {
        REQUIRE(transcript_state && rng_seed && out && (m == 0 || v_blinding));
        Transcript t = Transcript::from_state(transcript_state);
        std::vector<Scalar> vb(m);
        for (uint64_t i = 0; i < m; i++) std::memcpy(vb[i].w, v_blinding + 32 * i, 32);
        TranscriptRng rng = t.build_rng(vb, rng_seed);
        uint8_t tmp[64];
        for (uint64_t i = 0; i < skip; i++) rng.fill_bytes(tmp, 64);
        if (bulk) rng.fill_draws64(out, count);
        else for (uint64_t i = 0; i < count; i++) rng.fill_bytes(out + 64 * i, 64);
    });
}
bpg_status bpg_rng_draws_multi(const uint8_t transcript_state[203], uint64_t m, const uint8_t *v_blinding, uint32_t lanes, const uint8_t *rng_seeds,
                               const uint64_t *skip, uint64_t count, uint8_t *out) {
    return guard([&] {
        REQUIRE(transcript_state && rng_seeds && skip && out && lanes >= 1 && lanes <= 8 && (m == 0 || v_blinding));
        Transcript t = Transcript::from_state(transcript_state);
        std::vector<Scalar> vb(m);
        for (uint64_t i = 0; i < m; i++) std::memcpy(vb[i].w, v_blinding + 32 * i, 32);
        std::vector<TranscriptRng> rngs;
        for (uint32_t v = 0; v < lanes; v++) {
            rngs.push_back(t.build_rng(vb, rng_seeds + 32 * v));
            uint8_t tmp[64];
            for (uint64_t i = 0; i < skip[v]; i++) rngs.back().fill_bytes(tmp, 64);
        }
        TranscriptRng *r[8]; uint8_t *dst[8];
        for (uint32_t v = 0; v < lanes; v++) { r[v] = &rngs[v]; dst[v] = out + (size_t)v * 64 * count; }
        // in two calls, so that the second starts from the state the first left behind
        const uint64_t first = count / 3;
        TranscriptRng::fill_draws64_multi(r, dst, lanes, first);
        for (uint32_t v = 0; v < lanes; v++) dst[v] += 64 * first;
        TranscriptRng::fill_draws64_multi(r, dst, lanes, count - first);
    });
}
bpg_status bpg_keccak_selftest(uint64_t seed, uint32_t rounds, int32_t *impl_out, double *ns_out) {
    return guard([&] {
        uint64_t a[25], b[25], c[25], d[25];
        for (int i = 0; i < 25; i++) a[i] = b[i] = c[i] = d[i] = seed * 0x9e3779b97f4a7c15ULL + (uint64_t)i * 0xd1342543de82ef95ULL + (seed >> (i & 31));
#if defined(__x86_64__)
        const bool vec = __builtin_cpu_supports("avx512f") && __builtin_cpu_supports("avx512vl");
#else
        const bool vec = false;
#endif
        for (uint32_t r = 0; r < rounds; r++) {
            keccak_f1600_scalar(a); keccak_f1600_host(b);
            if (std::memcmp(a, b, sizeof a) != 0) throw std::runtime_error("keccak: active and scalar implementations disagree");
#if defined(__x86_64__)
            if (vec) {
                keccak_f1600_avx512(c); keccak_f1600_xmm(d);
                if (std::memcmp(a, c, sizeof a) != 0) throw std::runtime_error("keccak: planes-in-ZMM and scalar implementations disagree");
                if (std::memcmp(a, d, sizeof a) != 0) throw std::runtime_error("keccak: lanes-in-XMM and scalar implementations disagree");
            }
#endif
            a[r % 25] ^= r; b[r % 25] ^= r; c[r % 25] ^= r; d[r % 25] ^= r;
        }
        if (impl_out) *impl_out = keccak_impl();
        if (ns_out) {
            auto t0 = std::chrono::steady_clock::now();
            for (int r = 0; r < 200000; r++) keccak_f1600_host(b);
            *ns_out = std::chrono::duration<double, std::nano>(std::chrono::steady_clock::now() - t0).count() / 200000.0 + (b[0] == 1 ? 1e-9 : 0);
        }
    });
}
bpg_status bpg_scalar_op(int32_t op, const uint8_t *a, const uint8_t *b, uint8_t out[32]) {
    return guard([&] {
        REQUIRE(a && out);
        Scalar r;
        if (op == 5) r = Scalar::from_wide(a);
        else {
            Scalar x; std::memcpy(x.w, a, 32);
            Scalar y; if (b) std::memcpy(y.w, b, 32);
            switch (op) { case 0: r = x + y; break; case 1: r = x - y; break; case 2: r = x * y; break; case 3: r = x.invert(); break; case 4: r = x.reduced(); break; default: throw std::invalid_argument("bad op"); }
        }
        r.to_bytes(out);
    });
}

}  // extern "C"
