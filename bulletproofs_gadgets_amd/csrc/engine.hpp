// HIP engine behind the C ABI (include/bpg.h): owns the device, the generator tables resident in HBM, the MSM
// workspace and the prove pipeline.  There is NO CPU execution path: construction throws when no GPU is present.
#pragma once
#include <cstdint>
#include <string>
#include <utility>
#include <vector>
#include "host/scalar.hpp"
#include "host/merlin.hpp"
#include "host/r1cs.hpp"
#include "host/template.hpp"
#include "host/check.hpp"

namespace bpg {

struct DeviceError : std::runtime_error { explicit DeviceError(const std::string &m) : std::runtime_error(m) {} };

struct ProveTimings {       // milliseconds, host wall clock around each phase (stream synchronised at phase ends)
    double rng_host = 0, msm_aiao = 0, msm_s = 0, poly = 0, ipa = 0, total = 0;
    double ipa_msm = 0, ipa_fold = 0, ipa_sync = 0;
    uint32_t shared_variants = 0;   // 1: this proof took the shared-device kernel variants (decided once, when prove() was entered)
};

// What the process holds from the HIP runtime at this moment, all contexts and all devices together (include/bpg.h bpg_test_live_resources; counted in
// hip_handles.hpp): device buffers, their bytes, pinned buffers, their bytes, streams, events.  Reads six counters: no device work.
void live_resources(uint64_t out[6]);

struct DeviceCircuit;       // HBM-resident flattened R1CS instance
struct DeviceMerkle;        // HBM-resident MiMC Merkle tree

// What a host chooses at context creation (include/bpg.h bpg_config).  A field left at its "unset" value falls back to the environment
// variable named beside it, then to the profile's default.
struct EngineConfig {
    uint32_t profile = 0;           // 0 unset (BPG_PROFILE, else one-shot), 1 one-shot, 2 serving
    double table_budget_gb = 0;     // cumulative HBM the precomputed generator multiples of this device may take (BPG_TABLE_GB); 0 unset
    uint32_t chain_workers = 0;     // 0 unset (BPG_CHAIN_WORKERS, else 1)
    uint32_t chain_lanes = 0;       // 0 unset (BPG_CHAIN_LANES, else 1)
    int32_t blocking_sync = -1;     // -1 unset (BPG_SYNC_BLOCKING=1/0, else spin), 1 blocking waits, 0 (or 2) spin waits
    std::string gens_cache_dir;     // empty unset (BPG_GENS_CACHE_DIR, else no cache)
};

// Chain threads shared by several contexts (include/bpg.h bpg_chain_pool_*): thread k draws up to lanes_per_thread[k] queued blinding streams in
// lockstep, whichever attached context queued them.  Must outlive the contexts attached to it.
class ChainPool {
public:
    explicit ChainPool(const std::vector<uint32_t> &lanes_per_thread);
    ~ChainPool();
    ChainPool(const ChainPool &) = delete;
    ChainPool &operator=(const ChainPool &) = delete;
    uint32_t capacity() const { return capacity_; }          // chains the pool draws side by side
    struct Impl;
private:
    friend class Engine;
    Impl *impl_;
    uint32_t capacity_ = 0;
};

class Engine {
public:
    explicit Engine(int device, const EngineConfig &cfg = EngineConfig());
    ~Engine();
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;

    int device() const { return device_; }
    static int device_count();      // AMD GPUs visible to the process (0 when there is none)
    // BulletproofGens::new(capacity, 1): derive (or extend) the G/H tables in HBM; capacity must be a power of two
    void gens_ensure(uint64_t capacity);
    uint64_t gens_capacity() const { return gens_cap_; }
    void gens_export(uint64_t first, uint64_t count, uint8_t *G_out, uint8_t *H_out);
    void pedersen_bases(uint8_t B[32], uint8_t B_blinding[32]);
    // k Pedersen commitments v_i*B + r_i*B_blinding (compressed). v may be unreduced (< 2^255); r any 256-bit value.
    void pedersen_commit(size_t k, const uint8_t *v, const uint8_t *blind, uint8_t *out);
    // multiscalar multiplication over generator-table slices, for tests: sum s_i * G[first+i] + t_i * H[first+i]
    void msm_gens(uint64_t first, uint64_t count, const uint8_t *s, const uint8_t *t, uint8_t out[32]);
    // the same kernels on any plan the prove path builds (include/bpg.h bpg_test_msm): nmsm compressed results, and a JSON text of the plan the
    // call took and the device state it left (starts[] of every bucket, the heavy and medium list counts)
    struct MsmSegSpec { uint32_t table, result; uint64_t first; uint32_t len, lgblk; const uint32_t *skip; };
    std::string test_msm(uint32_t nmsm, uint32_t nseg, const MsmSegSpec *segs, const uint8_t *scalars, uint8_t *out);
    // the generator fold of one group of the inner-product argument on scalars the caller chose (include/bpg.h bpg_test_fold): the launch path of the prover
    // on the context's own tables (G at 0, H at capacity; 2^(lgMr + rounds) points each), kernel = -1 (the chooser's) or a FoldKernel; out = 2 * 2^lgMr
    // compressed points, G side first; returns a JSON text of what was launched
    std::string test_fold(int32_t kernel, uint32_t lgMr, uint32_t rounds, uint32_t first, uint64_t n, const uint8_t *sG, const uint8_t *sH, const uint8_t u_ch[32],
                          uint8_t *out);
    // the table-driven tail of the inner-product argument on scalars the caller chose (include/bpg.h bpg_test_tail): the freeze and `rounds` sub-rounds as
    // inner_product() runs them, on G[0, M0), H[0, M0) and B of the context; lr_out = 2 * rounds encodings (L_0, R_0, L_1, ..), ab_out = the folded a then the
    // folded b (M0 >> rounds canonical scalars each); returns a JSON text of what was launched
    std::string test_tail(uint32_t lgM0, uint32_t tables, uint32_t first, uint64_t n, const uint8_t *a, const uint8_t *b, const uint8_t yinv[32], const uint8_t u_ch[32],
                          const uint8_t gamma0[32], const uint8_t eta0[32], const uint8_t w[32], uint32_t rounds, const uint8_t *u, uint8_t *lr_out, uint8_t *ab_out);
    // A_I, A_O, S from the window tables of the original generators on scalars the caller chose (include/bpg.h bpg_test_commit3): n values per vector,
    // blind = the three blindings; out = the three encodings; returns a JSON text of what was launched
    std::string test_commit3(uint32_t lgM0, uint64_t n, const uint8_t *aL, const uint8_t *aR, const uint8_t *aO, const uint8_t *sL, const uint8_t *sR,
                             const uint8_t *blind, uint8_t out[96]);
    // the verifier's flattened weights of a resident circuit at a z the caller chose (include/bpg.h bpg_test_weights): the powers of z, k_flatten and the
    // k_flatten_const reduction as verify() runs them; out = 3 n + m + 1 canonical scalars w_L | w_R | w_O | w_V | w_c.  Refused before any launch
    // (std::invalid_argument): a null pointer, a non-canonical z, a circuit of another device
    void test_weights(DeviceCircuit *c, const uint8_t z[32], uint8_t *out);

    DeviceCircuit *upload(const FlatView &c);
    DeviceCircuit *upload(const FlatCircuit &c) { return upload(FlatView(c)); }
    void free_circuit(DeviceCircuit *c);
    // Circuit template (include/bpg.h bpg_r1cs_upload_template): upload() plus the witness program, packed and scheduled (host/template.hpp), in HBM.  The
    // witness arrays are allocated either way; a witness in `c` is uploaded as upload() does, so the first proof needs no assign().  Each parameter row's
    // constant terms become one coefficient slot of its own.  Constants that flow into multiplications are part of the program and stay fixed - unless they
    // are PUBLIC INPUTS (p.n_inputs > 0, include/bpg.h bpg_r1cs_upload_template_inputs): terms of kind Variable::Input in the rows and in the program, whose
    // values every assign brings.  input_values (n_inputs x 32): those of the witness `c` carries (needed then; null: the derived slots start at zero).
    // plan_template: every host-side check (instance and program: std::invalid_argument) and the schedule, packed program and parameter slots, no device work.
    static TemplatePlan plan_template(const FlatView &c, const WitnessProgramView &p, const uint8_t *input_values = nullptr);
    DeviceCircuit *upload_template(const FlatView &c, const TemplatePlan &plan);
    // A fresh witness for a template: m committed values (32 bytes each, any 256-bit value: reduced mod l on the device) and the constant term of every
    // parameter row; a_L, a_R, a_O are computed on the device (k_witness_eval, one launch per schedule level), everything cached for the previous witness
    // (the equal-scalar merge sets) is dropped.  Returns once the witness is in place.
    void assign(DeviceCircuit *c, const uint8_t *v, const uint8_t *param_values);
    // The same for a template uploaded with checkpoints (include/bpg.h bpg_r1cs_assign_checkpointed; WitnessProgramView::ck_var): ck_values are the values of the
    // checkpointed variables (32 bytes each, reduced mod l on the device; a repeat: count x n_ck, item-major).  The levels read them wherever the program names a
    // checkpoint; one more launch (k_witness_ck_verify) then compares each with what the circuit computed.  Returns CHECKPOINTS_HOLD, or the lowest flat index
    // (item * n_ck + k) that differs - the circuit then holds NO witness.  A template without checkpoints takes null ck_values and is plain assign().
    // Plain assign() on a checkpointed template: std::invalid_argument.
    static constexpr uint64_t CHECKPOINTS_HOLD = ~0ull;
    uint64_t assign_checkpointed(DeviceCircuit *c, const uint8_t *v, const uint8_t *param_values, const uint8_t *ck_values);
    static uint64_t checkpoints_per_item(const DeviceCircuit *c);   // n_ck of the template (a repeat: of its source; it takes count x n_ck values)
    // The same for a template with public inputs (include/bpg.h bpg_r1cs_assign_inputs): input_values are its n_inputs values (32 bytes each, reduced mod l on the
    // device).  They go up as v does; k_input_slots writes coef[ci] * x_p into every derived slot before a level runs, and the levels read the inputs wherever the
    // program names one.  A template without inputs takes null and is assign_checkpointed().  assign() / assign_checkpointed() on a template with inputs:
    // std::invalid_argument.
    uint64_t assign_inputs(DeviceCircuit *c, const uint8_t *v, const uint8_t *param_values, const uint8_t *ck_values, const uint8_t *input_values);
    // The verifier's half of it (include/bpg.h bpg_r1cs_set_inputs): the n_inputs values go up and the derived slots are filled - one launch - and nothing else; the
    // circuit is left without a witness.  Any template with inputs: single, repeat or join.  Refused (std::invalid_argument): no inputs, null values.
    void set_inputs(DeviceCircuit *c, const uint8_t *input_values);
    // Which multiplier, which constraint row does the resident witness break (include/bpg.h bpg_r1cs_check; hip/k_check.cuh): a_L * a_R against a_O per multiplier, and
    // every row of the matrix over the operand vector [a_L | a_R | a_O | v | 1].  v: m x 32 bytes (reduced mod l on the device), or null on a template: the values
    // of its last assign().  rows_out receives the lowest min(cap, bad_rows) bad rows, ascending.  The first check of a circuit derives a row-major view of its
    // matrix on the device and keeps it in the circuit.  Refused before any device work: no witness (R1CSException MissingAssignment), null v where the circuit keeps
    // no values, null rows_out with cap > 0 (std::invalid_argument).  Leaves the witness, the equal-scalar sets and every proof that follows as they were.
    CheckReport check(DeviceCircuit *c, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out);
    static void template_eval_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO);   // test hook
    // test hook (bpg_test_template_eval_batch): the BATCHED interpreter (k_witness_eval_batch) compiled for the host - level by level, every item of a
    // segment side by side, into the wave layout (count x N x 32 bytes per vector, item-major, N = padded size, padding rows zero); v: count x m x 32
    // test hook (bpg_test_template_eval_checkpointed): template_eval_host for a program with checkpoints, made to show what in-order execution on one thread
    // hides - a_L, a_R, a_O start as a poison value, the segments of every level run in REVERSE order, then the verify step; returns the first mismatch
    // input_values (bpg_test_template_eval_inputs): the n_inputs public inputs of a program with inputs, reduced as assign_inputs reduces them
    static uint64_t template_eval_checkpointed_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *v, const uint8_t *ck_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                                    const uint8_t *input_values = nullptr);
    static void template_eval_batch_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO);
    // test hook (bpg_test_template_eval_batch_checkpointed): the two combined - the batched interpreter with count x n_ck checkpoint values (item-major) under
    // the poison / reverse-order discipline, then the step of k_witness_ck_verify_batch: first_out[k] = item k's lowest mismatch, or CHECKPOINTS_HOLD
    static void template_eval_batch_checkpointed_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                      uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_out, const uint8_t *input_values = nullptr);
    // test hook (bpg_test_template_inputs_instance): the resident rows of a template with inputs as an assign of input_values leaves them - every input term a
    // constant term on its derived slot, the slot holding what k_input_slots writes (the same product, compiled for the host)
    static FlatCircuit template_inputs_instance_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *param_values, const uint8_t *input_values);
    // A template repeated `count` times (include/bpg.h bpg_r1cs_template_repeat; hip/k_repeat.cuh): a new resident template of count x (n, q, m, n_params), built on
    // the device from the source's resident matrix - copy k at multipliers k n.., committed values k m.., rows k q.., parameter slots k n_params.., everything else
    // shared.  It owns copies of all it needs, holds no witness and no host rows; assign() evaluates it with the source's program, a lane per (segment, item).
    // Refused (std::invalid_argument, before any device work): not a template, a repeat, count 0, sizes beyond the instance format.
    // with_inputs (bpg_r1cs_template_repeat_inputs): a source with public inputs is served - count x n_inputs values, item-major, and count x n_slots derived
    // coefficient slots behind ALL parameter slots, filled per item by k_input_slots_join; false: such a source is refused, as the frozen call refuses it.
    DeviceCircuit *repeat_template(DeviceCircuit *tmpl, uint64_t count, bool with_inputs = false);
    static bool is_repeat(const DeviceCircuit *c);
    // test hooks (bpg_test_template_repeat_instance, bpg_test_template_eval_repeat): the repeated rows as k_repeat_* leave them, and the repeat-layout interpreter
    // (k_witness_eval_repeat) compiled for the host; no device
    static FlatCircuit template_repeat_instance_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *param_values);
    static void template_eval_repeat_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, uint8_t *aL, uint8_t *aR, uint8_t *aO);
    // the same two for a source with public inputs and / or checkpoints (bpg_test_template_repeat_inputs_instance, bpg_test_template_eval_repeat_inputs): the derived
    // slots as k_input_slots_join fills them; the interpreter from poisoned vectors, segments and items in reverse order, then the comparison step.  caps: row_ptr,
    // term and coef capacities of the caller, checked against the size formulas before anything is built (null: not checked)
    static FlatCircuit template_repeat_inputs_instance_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *param_values,
                                                            const uint8_t *input_values, const uint64_t caps[3] = nullptr);
    static uint64_t template_eval_repeat_inputs_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                     const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO);
    // Templates joined (include/bpg.h bpg_r1cs_template_join; hip/k_join.cuh): a new resident template that holds count_0 copies of part 0, then count_1 of part 1,
    // and so on - the circuit of ONE host assembly of the parts' gadget code in that order - built on the device from the parts' resident matrices.  It owns copies
    // of all it needs, holds no witness and no host rows; assign() evaluates every part's program in ONE launch per level (the most levels any part has).
    // Refused (std::invalid_argument that names the part, before any device work): no part or more than 256, a null part, count 0, not a template, a repeat or a
    // join, a part on another device, totals beyond the instance format.
    // with_inputs (bpg_r1cs_template_join_inputs): parts with public inputs are served - inputs and derived slots part-major, then item-major; false: refused.
    DeviceCircuit *join_templates(const std::vector<std::pair<DeviceCircuit *, uint64_t>> &parts, bool with_inputs = false);
    static bool is_join(const DeviceCircuit *c);
    // flat index of the joined checkpoint list -> (part, item, checkpoint of the part's template); false: not a join, or no such index
    static bool join_checkpoint_place(const DeviceCircuit *c, uint64_t flat, uint64_t *part, uint64_t *item, uint64_t *ck);
    // test hooks (bpg_test_template_join_instance, bpg_test_template_eval_join): the joined rows as k_join_* leave them, and the join-layout interpreter
    // (k_witness_eval_join, k_witness_ck_verify_join) compiled for the host; no device
    struct JoinSource { FlatView c; WitnessProgramView p; uint64_t count; };
    // input_values (bpg_test_template_join_inputs_instance, bpg_test_template_eval_join_inputs): the joined public inputs when a part's program has any; caps as above
    static FlatCircuit template_join_instance_host(const std::vector<JoinSource> &parts, const uint8_t *param_values, const uint8_t *input_values = nullptr,
                                                   const uint64_t *caps = nullptr);
    static uint64_t template_eval_join_host(const std::vector<JoinSource> &parts, const uint8_t *v, const uint8_t *ck_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                            const uint8_t *input_values = nullptr);
    // Prover::prove on a resident circuit. transcript: state after Prover::new + every "V" append (updated in place).
    std::vector<uint8_t> prove(DeviceCircuit *c, Transcript &transcript, const std::vector<Scalar> &v_blinding,
                               const uint8_t rng_seed[32], uint32_t flags, ProveTimings *timings = nullptr);
    // Speculative start of prove()'s TranscriptRng on a host thread (extension; include/bpg.h bpg_blinding_begin): the draws depend on the
    // transcript after the last commitment, v_blinding and the seed only.  prove() uses the stream iff all three still match, else discards it.
    void blinding_begin(const Transcript &after_commitments, const std::vector<Scalar> &v_blinding, const uint8_t seed[32], uint64_t max_multipliers);
    void blinding_cancel();
    // threads of the context's chain worker: that many queued streams are drawn side by side, workers + 1 may be alive (default 1)
    void set_chain_workers(uint32_t n);
    // draw this context's blinding streams on a shared pool instead of its own worker (nullptr: back to its own); max_streams of them may be alive
    void attach_chain_pool(ChainPool *pool, uint32_t max_streams);
    void set_chain_lanes(uint32_t n);        // streams each chain thread draws in lockstep (1..8; eight sponges in the lanes of ZMM registers)
    void test_fail_next_upload();   // test hook (bpg_test_fail_next_upload)
    void test_drop_next_upload();   // test hook (bpg_test_drop_next_upload): the copies of the next stream are skipped without an error
    uint64_t table_bytes() const;   // precomputed generator multiples held on this device by the process
    bool last_shared_variants() const;   // did the last prove()/verify() on this context take the shared-device kernel variants
    int chain_cpu() const;      // host core the chain worker last drew a stream on (-1: none yet); diagnostics for bench.py
    void test_fe_ops(int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out);   // unit-test hook (k_test_fe)
    // unit-test hook (bpg_test_decompress): k_decompress on n encodings; ok flags and canonical affine x || y (from the halved Niels form) of every entry
    void test_decompress(size_t n, const uint8_t *in, uint32_t *ok_out, uint8_t *xy_out);
    // unit-test hook (bpg_test_verify_replay): R1CSProof::from_bytes and the Fiat-Shamir replay alone - None means "left to the device"; no device work
    static R1CSError test_verify_replay(uint64_t n, uint64_t m, uint64_t gens_cap, Transcript &T, const uint8_t *proof, size_t proof_len,
                                        const uint8_t seed[32], uint32_t flags);
    // test seam (include/bpg.h bpg_test_prove_scripted and its siblings): attach to T a script of challenges y, z, u, x, w, u_1 .. u_lgN for a circuit of n
    // multipliers (host/merlin.hpp Transcript::attach_script), after which prove(), prove_batch(), verify() and verify_batch() run on T as on any transcript.
    // Refused (std::invalid_argument): a length other than 5 + lg N, a non-canonical entry, y or a u_k of zero.  No device work.
    static void script_transcript(Transcript &T, uint64_t n, const uint8_t *script, uint64_t script_len);
    // unit-test hook (bpg_test_verify_replay_scripted): test_verify_replay, plus the challenges the replay drew (challenges_out: (5 + lg N) x 32, zero where it
    // did not get) and the number of script entries T gave out
    static R1CSError test_verify_replay_scripted(uint64_t n, uint64_t m, uint64_t gens_cap, Transcript &T, const uint8_t *proof, size_t proof_len,
                                                 const uint8_t seed[32], uint32_t flags, uint8_t *challenges_out, uint64_t *consumed_out);
    // Verifier::verify on a resident (assignment-free) circuit. transcript: state after Verifier::new + every "V" append.
    R1CSError verify(DeviceCircuit *c, Transcript &transcript, const uint8_t *V, const uint8_t *proof, size_t proof_len,
                     const uint8_t seed[32], uint32_t flags);
    // One proof of a batch (include/bpg.h bpg_r1cs_verify_batch): a resident circuit (dc) or a verifier-side instance (flat) that is uploaded,
    // used and freed inside the call; T is updated in place exactly as verify() updates it.
    struct VerifyItem {
        DeviceCircuit *dc = nullptr; const FlatView *flat = nullptr;
        Transcript *T = nullptr; const uint8_t *V = nullptr; const uint8_t *proof = nullptr; size_t proof_len = 0;
        const uint8_t *seed = nullptr; uint32_t flags = 0;
    };
    // Every proof's verification equation weighted by a random rho_k, all of them in ONE multiscalar multiplication; status_out[k] is what verify()
    // returns for item k alone (a rejected batch is re-verified item by item).
    void verify_batch(size_t count, const VerifyItem *items, const uint8_t batch_seed[32], R1CSError *status_out);
    // One proof of a lockstep verification (include/bpg.h bpg_r1cs_verify_resident_batch): the arguments of verify() on the call's ONE resident circuit, plus the
    // item's own parameter values (n_params x 32) and public inputs (n_inputs x 32), either null: the circuit's standing slots.
    struct ResidentVerifyItem {
        Transcript *T = nullptr; const uint8_t *V = nullptr; const uint8_t *proof = nullptr; size_t proof_len = 0; const uint8_t *seed = nullptr; uint32_t flags = 0;
        const uint8_t *params = nullptr, *inputs = nullptr;
    };
    // K proofs of one resident circuit, weighted as verify_batch weighs them, with a constant number of launches per wave of items (hip/k_vwave.cuh,
    // host/verify_wave_plan.hpp) and the replays on the host threads of the proving waves; status_out[k] is what verify() returns for item k alone with its
    // constants standing.  The circuit's coefficient table holds afterwards what it held before; a resident witness is neither read nor dropped.
    // check_resident_batch: what the call refuses before any device work (std::invalid_argument): a null circuit, one of another context or device, per-item
    // constants on anything but a single template, parameter values without parameter rows, inputs without public inputs.
    void check_resident_batch(const DeviceCircuit *c, size_t count, const ResidentVerifyItem *items) const;
    void verify_resident_batch(DeviceCircuit *c, size_t count, const ResidentVerifyItem *items, const uint8_t batch_seed[32], R1CSError *status_out);
    // test hook (bpg_test_verify_wave_scalars): the device side of verify_resident_batch from k_vw_exp to k_vw_reduce, through the function the call runs, on
    // challenge records the caller chose (count x (7 + 2 lg N) canonical scalars: y^-1, z, x, u, a, b, rho, u_k, u_k^-1); param_values / input_values: null or
    // one set per item.  g_out, h_out: the accumulators (N canonical scalars each); small_out: count slots [w_V (m) | w_c | delta]; returns a JSON text of the
    // plan it took.  Refused before a launch (std::invalid_argument): a non-canonical entry, y^-1 or a u_k of zero, a u_k^-1 that is not the inverse
    std::string test_verify_wave_scalars(DeviceCircuit *c, uint64_t count, const uint8_t *challenges, const uint8_t *param_values, const uint8_t *input_values,
                                         uint8_t *g_out, uint8_t *h_out, uint8_t *small_out);
    // One proof of a lockstep batch (include/bpg.h bpg_r1cs_prove_batch): an instance with its witness that passed the checks of bpg_r1cs_prove and
    // lockstep_eligible(); T is updated in place and proof filled exactly as prove() does for the item alone.  An item of prove_template_batch has no
    // instance of its own: its witness source is the template plus `values` (m x 32 committed values) and `params` (n_params x 32), and flat is left null.
    struct ProveItem {
        const FlatView *flat = nullptr; Transcript *T = nullptr; const std::vector<Scalar> *vb = nullptr; const uint8_t *seed = nullptr; uint32_t flags = 0;
        const uint8_t *values = nullptr, *params = nullptr;
        std::vector<uint8_t> proof;
        std::vector<uint8_t> commitments;       // prove_template_batch(commit = true): the m encodings this item's wave made and appended to T as "V"
        // prove_template_batch(checkpointed = true): in, the template's n_ck checkpoint values (n_ck x 32, as assign_checkpointed takes them); out, the lowest
        // checkpoint that is not the circuit's own value, or CHECKPOINTS_HOLD.  An item that reports one rode its wave to the end and leaves with an EMPTY
        // proof and no commitments; its T is spent (the caller proves on a copy and exports it on success only)
        const uint8_t *ck = nullptr; uint64_t ck_first = ~0ull;
        const uint8_t *inputs = nullptr;        // a template with public inputs: the item's n_inputs values (n_inputs x 32, as assign_inputs takes them)
    };
    // does a proof of n multipliers with these flags take the lockstep path (0 < n, padded N <= 2^tt_orig_lg, no expanded blinding)
    bool lockstep_eligible(uint64_t n, uint32_t flags) const;
    // every item proved in lockstep: grouped by lg N, each group in waves of at most BPG_BATCH_WAVE_MB of device state, one launch per stage per wave
    void prove_batch(size_t count, ProveItem *items) { prove_batch(count, items, nullptr); }
    // K fresh witnesses of ONE template in lockstep (include/bpg.h bpg_r1cs_prove_template_batch): prove_batch with the witness of every item computed
    // on the device, all items of a wave in one launch per schedule level (k_witness_eval_batch), straight into the wave's a_L, a_R, a_O.  The template
    // must be lockstep-eligible with every item's flags (template_lockstep()).  Whatever happens, the template holds no witness afterwards.
    // commit (include/bpg.h bpg_r1cs_prove_template_batch_commit): T is the transcript BEFORE the "V" appends; each wave makes the commitments
    // values[j] * B + vb[j] * B_blinding of its items in one launch (k_bt_commit_v) from the values it uploaded for the witness evaluation, fills
    // `commitments` and appends them to T before anything is drawn from it.  Nothing after that point differs.
    // checkpointed (include/bpg.h bpg_r1cs_prove_template_batch_checkpointed): every item brings ProveItem::ck; a wave evaluates the CHECKPOINTED schedule
    // (a preimage: one level, a Merkle path: two) and one more launch (k_witness_ck_verify_batch) compares, per item; the result comes back with the copy of
    // A_I, A_O, S.  Without it a template with checkpoints is refused (std::invalid_argument), as the frozen batch calls document.
    void prove_template_batch(DeviceCircuit *tmpl, size_t count, ProveItem *items, bool commit = false, bool checkpointed = false);
    // the template kept the host copy of its rows that the lockstep packer needs (padded N <= 2^14)
    static bool template_lockstep(const DeviceCircuit *tmpl);
    // what a template batch leaves behind on either path: no witness, no equal-scalar sets
    static void drop_witness(DeviceCircuit *tmpl);
    // the host-side checks of an instance (CSR shape, index ranges, sizes), which upload() and plan_template() start with: std::invalid_argument, no device work
    // n_inputs: terms of kind Variable::Input that name inputs [0, n_inputs) are legal (a template with inputs); 0, every other caller: the kind is refused
    static void check_instance(const FlatView &c, uint64_t n_inputs = 0, uint64_t n_gates = 0);
    // MiMC sponges and Merkle trees on the device (include/bpg.h, "MiMC Merkle trees"; hip/k_mimc.cuh).  Every argument is checked before the device is touched
    // (std::invalid_argument); the calls run on the context's stream and return synchronised.
    // mimc_sponge_1 of count items of `blocks` 32-byte blocks each (any 256-bit value, taken mod l) -> count canonical scalars
    void mimc_sponge_many(uint64_t count, uint64_t blocks, const uint8_t *in, uint8_t *out);
    // the full tree over 2^depth leaves (depth 1..24; a leaf is any 256-bit value, taken mod l): node = sponge(left, right), resident in Montgomery form
    DeviceMerkle *merkle_build(uint32_t depth, const uint8_t *leaves);
    void merkle_nodes(DeviceMerkle *t, uint32_t level, uint64_t first, uint64_t count, uint8_t *out);      // level 0 = the root, level depth = the leaves
    // count x depth x 32, the leaf's sibling first; ancestors (bpg_merkle_path_nodes): the nodes ON each path instead, the leaf's parent first, the root last
    void merkle_paths(DeviceMerkle *t, uint64_t count, const uint64_t *indices, uint8_t *siblings_out, bool ancestors = false);
    void merkle_update(DeviceMerkle *t, uint64_t count, const uint64_t *indices, const uint8_t *leaves);   // distinct indices below the tree's size; only their ancestors are recomputed
    // A tree that grows: capacity 2^depth, `size` leaves, the rest `empty` (NULL = zero) - node for node the full tree over leaves || empty x (2^depth - size).
    // The empty subtrees are constants the host computes and k_merkle_fill_empty writes; only the ancestors of real leaves are hashed, by the launches of
    // host/merkle_plan.hpp and by nothing else.  append puts leaves at [size, size + count) and recomputes exactly their ancestors, each once.
    DeviceMerkle *merkle_build_partial(uint32_t depth, uint64_t size, const uint8_t *leaves, const uint8_t *empty);
    void merkle_append(DeviceMerkle *t, uint64_t count, const uint8_t *leaves, uint64_t *first_index_out, uint8_t *root_out);
    void merkle_size(DeviceMerkle *t, uint64_t *size_out, uint32_t *depth_out);
    void merkle_empty_nodes(DeviceMerkle *t, uint8_t *out);         // (depth + 1) x 32: out[k] = an empty subtree k levels above the leaves; host only
    static void merkle_free(DeviceMerkle *t);       // on the tree's own context; a tree that outlived its context lost its memory then and is only deleted
    // The prefix layout (host/merkle_prefix_plan.hpp; hip/k_merkle_prefix.cuh): depth 1..32, room for `reserve` <= min(2^depth, 2^24) leaves, only the occupied
    // prefix of every level stored and everything else read as an empty-subtree constant - node for node the tree merkle_build_partial builds, in
    // 32 x (sum of the stored widths + depth + 1) bytes.  Every call above serves such a tree; append grows the reserve when the tree outgrows it.
    DeviceMerkle *merkle_build_prefix(uint32_t depth, uint64_t reserve, uint64_t size, const uint8_t *leaves, const uint8_t *empty);
    void merkle_reserve(DeviceMerkle *t, uint64_t leaves);          // room for at least `leaves`: a new buffer, one relayout launch, the old buffer released; a dense tree is refused
    void merkle_reserved(DeviceMerkle *t, uint64_t *reserve_out, uint64_t *bytes_out);     // a dense tree: 2^depth and its array; a keyed tree: the keys held and its bytes
    // The keyed layout (host/merkle_keyed_plan.hpp; hip/k_merkle_keyed.cuh): depth 1..32, up to 2^24 distinct keys below 2^depth, one leaf per key and `empty`
    // everywhere else - node for node the tree merkle_build builds over that 2^depth-entry list.  Height s stores the nodes with a held key below them as
    // sorted positions beside their values; everything else reads as an empty-subtree constant.  Every read call above serves such a tree; update takes held
    // keys only; append and reserve refuse it.  put replaces the leaf of a held key and inserts a key that is not held (held_only: refuses the latter).
    // merkle_key_order: the permutation that sorts the keys of one call (refuses a key beyond 2^depth and a key given twice; no device); build and put take
    // one that the caller made already instead of sorting again.
    static std::vector<uint32_t> merkle_key_order(uint32_t depth, uint64_t count, const uint64_t *keys);
    DeviceMerkle *merkle_build_keyed(uint32_t depth, uint64_t count, const uint64_t *keys, const uint8_t *leaves, const uint8_t *empty, const std::vector<uint32_t> *sorted_order = nullptr);
    void merkle_put(DeviceMerkle *t, uint64_t count, const uint64_t *keys, const uint8_t *leaves, uint64_t *inserted_out, uint8_t *root_out, bool held_only = false,
                    const std::vector<uint32_t> *sorted_order = nullptr);
    void merkle_get(DeviceMerkle *t, uint64_t count, const uint64_t *keys, uint8_t *leaves_out, uint8_t *held_out);       // any layout: dense and prefix hold index < size
    void merkle_keys(DeviceMerkle *t, uint64_t first, uint64_t count, uint64_t *keys_out);                                 // held keys, ascending; dense and prefix: key i = i
    void merkle_node_counts(DeviceMerkle *t, uint64_t *counts_out, uint64_t *bytes_out);                                   // depth + 1 stored-node counts, height 0 first; keyed trees only
private:
    void merkle_append_prefix(DeviceMerkle *t, uint64_t count, const uint8_t *leaves, uint64_t *first_index_out, uint8_t *root_out);
public:
    void synchronize();
    // HIP-event profile on the engine's own stream: mode 0 off, 1 = dominant kernel (k_fold_points) only, 2 = all kernels
    void profile_set(int mode);
    std::string profile_report();          // JSON: {kernel: {count, total_ms, alg_bytes, device_bytes, field_mults}}
    double bench_fe_mul(uint32_t iters);   // measured field-multiplication throughput (integer-VALU roofline)
    void *stream_handle() const { return stream_; }
    // names of the kernels launched by the last prove(), with counts (diagnostics for bench.py)
    struct Impl;
private:
    int device_;
    void *stream_ = nullptr;
    uint64_t gens_cap_ = 0;
    Impl *impl_ = nullptr;
    void prove_batch(size_t count, ProveItem *items, DeviceCircuit *tmpl, bool commit = false);
    void init_device();             // second half of the constructor: everything that touches the GPU
};

}  // namespace bpg
