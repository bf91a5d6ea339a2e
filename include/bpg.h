/* bpg.h - C ABI of the MI355X-native Bulletproofs R1CS prove path (libbpg_hip.so).
 *
 * Drop-in boundary for MarcKloter/bulletproofs_gadgets: the reference reaches this path through Rust crates
 * (bulletproofs fork, curve25519-dalek, merlin; reference Cargo.toml:8-20) that have no FFI today.  A Rust host
 * keeps the mini-language parser and the R1CS assembly and binds the functions of PART 1 (see INTEGRATION.md for
 * the `extern "C"` block); PART 2 is the same assembly surface offered natively (C++ inside the library) for hosts
 * without a Rust toolchain - the repo's Python harness, tests and bench.py drive it through ctypes.
 *
 * Conventions: scalars and compressed points are 32-byte little-endian encodings; the caller allocates every
 * output; every function returns a bpg_status (0 = ok) and never unwinds across the boundary; a context (and the
 * objects created from it) is used by one host thread at a time, different contexts are independent.
 * There is NO CPU fallback: bpg_ctx_create fails with BPG_ERR_DEVICE when no AMD GPU is visible.
 *
 * SIDE CHANNELS - read before proving with secrets on shared hardware.  Upstream computes A_I, A_O, S, T_k and every Pedersen commitment with
 * a CONSTANT-TIME multiscalar multiplication (Straus, fixed table lookups) because their scalars are secret: the witness a_L, a_R, a_O, the
 * blinding vectors s_L, s_R and the blinding factors.  This library does not: those scalars go through the bucket method (digit-indexed
 * scatter and gather) and, in the table-driven paths, through digit-indexed table reads with zero digits skipped; the host's Horner
 * recombination and the scalar arithmetic of host/scalar.hpp are variable-time as well.  Memory access pattern and running time therefore depend
 * on secret data.  The proof bytes are the same; the posture is that of a prover on a machine its operator trusts.
 * The witness evaluation of a circuit template (bpg_r1cs_assign) is variable-time in the same sense: it skips products by coefficients +1 / -1 and reduces
 * with data-dependent selects.  The batched evaluation of bpg_r1cs_prove_template_batch runs the same interpreter and is variable-time in the same sense.
 * The bit hints of a range-proof template (bpg_witness_hints) are read by that interpreter too: no claim of constant time is made for them either.
 */
#ifndef BPG_H
#define BPG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t bpg_status;
#define BPG_OK 0
#define BPG_ERR_INVALID_GENERATORS_LENGTH 1   /* R1CSError::InvalidGeneratorsLength */
#define BPG_ERR_FORMAT 2                      /* R1CSError::FormatError */
#define BPG_ERR_VERIFICATION 3                /* R1CSError::VerificationError */
#define BPG_ERR_INVALID_ARGUMENT 4
#define BPG_ERR_MISSING_ASSIGNMENT 5          /* R1CSError::MissingAssignment (reference src/cs_buffer.rs:104) */
#define BPG_ERR_GADGET 6                      /* R1CSError::GadgetError        (reference src/cs_buffer.rs:100) */
#define BPG_ERR_DEVICE 7
#define BPG_ERR_INTERNAL 8
#define BPG_ERR_CHECKPOINT_MISMATCH 9         /* bpg_r1cs_assign_checkpointed: a checkpoint value is not what the circuit computes */

/* dialect flags of the proof encoding / transcript (the fork's revision is unpinned) */
#define BPG_FLAG_COMPACT_1PHASE 1u            /* v2.0.0 encoding: version byte 0x00 + 11 points */
#define BPG_FLAG_NO_1PHASE_DOMSEP 2u          /* omit the "r1cs-1phase" domain separator */
/* Prover-only, opt-in, NOT upstream's derivation (off by default; never used for the headline benchmark): the 2n blinding scalars
 * s_L || s_R are expanded on the GPU instead of being drawn one by one from Merlin's serial TranscriptRng (which is 87 % of a
 * 2^20 proof).  After the three blinding scalars of A_I, A_O, S one more 64-byte block K is drawn from the TranscriptRng; scalar j is
 * from_bytes_mod_order_wide(SHAKE256("bpg blinding v1" || K || le64(j))[0..64)).  K depends on the transcript, the witness blindings
 * and the external 32 random bytes exactly as every upstream draw does.  The proof is an ordinary proof for any verifier. */
#define BPG_FLAG_EXPANDED_BLINDING 4u

/* variable encoding inside constraint terms: kind << 29 | index   (bulletproofs::r1cs::Variable) */
#define BPG_VAR_MULTIPLIER_LEFT 0u
#define BPG_VAR_MULTIPLIER_RIGHT 1u
#define BPG_VAR_MULTIPLIER_OUTPUT 2u
#define BPG_VAR_COMMITTED 3u
#define BPG_VAR_ONE 4u
/* A PUBLIC INPUT of the proof (bpg_prover_input / bpg_verifier_input; "Public inputs in circuit templates" below): legal in term_var of an instance and of a
 * witness program ONLY for bpg_r1cs_upload_template_inputs.  Every other entry point that takes an instance or a program - bpg_r1cs_upload, bpg_r1cs_prove,
 * bpg_r1cs_verify, bpg_r1cs_verify_batch, bpg_r1cs_prove_batch, the pool, the older template uploads - refuses the kind before any device work with
 * BPG_ERR_INVALID_ARGUMENT, and bpg_last_error names the term.  (bpg_prover_instance and bpg_verifier_instance never export it: see below.) */
#define BPG_VAR_INPUT 5u
#define BPG_TRANSCRIPT_STATE_BYTES 203        /* STROBE-128: 200 state bytes, pos, pos_begin, cur_flags */

typedef struct bpg_ctx bpg_ctx;
typedef struct bpg_circuit bpg_circuit;

/* Flattened R1CS instance = the state a bulletproofs::r1cs::Prover holds when prove() is called:
 * a_L, a_R, a_O (n x 32 B, reduced mod l) and the constraint list in CSR form with a de-duplicated coefficient table. */
typedef struct {
    uint64_t n, q, m, nnz, ncoef;
    const uint8_t *aL, *aR, *aO;
    const uint64_t *row_ptr;      /* q + 1 */
    const uint32_t *term_var;     /* nnz : kind << 29 | index */
    const uint32_t *term_coef;    /* nnz : index into coef */
    const uint8_t *coef;          /* ncoef x 32 */
} bpg_r1cs_instance;

/* milliseconds; filled when a non-NULL pointer is passed to a prove call.  FROZEN at nine doubles (72 bytes): the library writes exactly these and
 * the struct never grows (a caller-owned struct without a size field cannot).  Whether a proof took the shared-device kernel variants is reported by
 * bpg_ctx_last_shared_variants() and in bpg_profile_report's "_schedule". */
typedef struct {
    double rng_host, msm_aiao, msm_s, poly, ipa, total, ipa_msm, ipa_fold, ipa_sync;
} bpg_timings;

/* ---------------------------------------------------------------------------------------------------- PART 1: hot path */
/* ABI version of this header.  Rules: structs the CALLER allocates either carry a struct_size (bpg_config: fields are only ever added at the end and
 * read when struct_size covers them) or are frozen (bpg_timings, bpg_r1cs_instance, bpg_batch_item, bpg_template_item, bpg_template_commit_item, bpg_template_ck_item, bpg_template_in_item, bpg_witness_program, bpg_witness_hints, bpg_witness_checkpoints, bpg_check_report, bpg_term, bpg_lc); a field never changes type or
 * meaning.  BPG_ABI_VERSION grows when something a version-7 host relies on is extended (a new field, a new flag value); functions ADDED since
 * version 7 (bpg_r1cs_prove_batch, the circuit-template calls) did not raise it: a host that needs one looks the symbol up (dlsym) and treats its
 * absence as "not supported".  A host checks bpg_abi_version() >= the BPG_ABI_VERSION it was compiled against. */
#define BPG_ABI_VERSION 7u
uint32_t bpg_abi_version(void);
const char *bpg_strerror(bpg_status s);
const char *bpg_last_error(void);                                /* message of the calling thread's last failure */

/* replaces PedersenGens::default() + device selection            (reference src/bin/prover.rs:53).
 * bpg_ctx_create(device, out) = bpg_ctx_create_ex(device, NULL, out): the ONE-SHOT profile - what a process that proves once and exits wants
 * (the reference's prover binary, src/bin/prover.rs:47-100): at most 4 GB of precomputed tables beside the generators (3.0 GB at 2^20, 7 ms).
 * bpg_ctx_create_ex takes the choices a host has: a zeroed bpg_config with struct_size set means "defaults"; a field left at 0 / NULL falls
 * back to the environment variable named beside it, then to the profile's default.  Every setting gives the same proof bytes. */
#define BPG_PROFILE_DEFAULT 0u   /* BPG_PROFILE=oneshot|serving if set, else one-shot */
#define BPG_PROFILE_ONESHOT 1u   /* first generator fold on width-5 NAF tables of scalars cut in two (15 tables: 3.0 GB at 2^20); no 8-bit tail tables; table budget 4 GB */
#define BPG_PROFILE_SERVING 2u   /* a long-lived prover: width-8 NAF on scalars cut in four (51.5 GB of tables at 2^20, built once per device in 0.12 s,
                                    shared by the contexts of the process: -2.4 ms per 2^20 proof), 8-bit tail tables for circuits up to 2^14
                                    multipliers (17.2 GB); table budget 96 GB */
typedef struct {
    uint32_t struct_size;        /* size of this struct in bytes as the caller compiled it: lets the struct grow */
    uint32_t profile;            /* BPG_PROFILE_* */
    double table_budget_gb;      /* cumulative HBM all precomputed generator multiples of this process on the device may take (BPG_TABLE_GB); what does
                                    not fit is replaced by the next smaller table set, in the end by kernels that need none; 0 = profile default */
    uint32_t chain_workers;      /* bpg_ctx_set_chain_workers at creation (BPG_CHAIN_WORKERS); 0 = default 1 */
    uint32_t chain_lanes;        /* bpg_ctx_set_chain_lanes at creation (BPG_CHAIN_LANES); 0 = default 1 */
    int32_t blocking_sync;       /* 1: host threads sleep in stream waits (hipDeviceScheduleBlockingSync; device-wide, first context of the process
                                    decides) - for hosts that run many proving threads beside their chain threads; 0 (and 2, which one revision of this
                                    header used for it): spin; -1 = BPG_SYNC_BLOCKING (1 / 0) if set, else spin.  A zeroed struct therefore spins, which
                                    is also what an unset environment gives */
    const char *gens_cache_dir;  /* directory of the on-disk generator cache (BPG_GENS_CACHE_DIR); NULL = no cache */
} bpg_config;
int32_t bpg_device_count(void);          /* AMD GPUs visible to the process (0: none - every bpg_ctx_create then fails with BPG_ERR_DEVICE) */
bpg_status bpg_ctx_create(int32_t device, bpg_ctx **out);
bpg_status bpg_ctx_create_ex(int32_t device, const bpg_config *config /* NULL = defaults */, bpg_ctx **out);
void bpg_ctx_destroy(bpg_ctx *ctx);
bpg_status bpg_pedersen_bases(bpg_ctx *ctx, uint8_t B[32], uint8_t B_blinding[32]);

/* replaces BulletproofGens::new(capacity, 1)                     (reference src/bin/prover.rs:92); tables stay in HBM.
   Contexts of one process on one device share the tables of a capacity (derived once, immutable, freed with the last context using them). */
bpg_status bpg_gens_ensure(bpg_ctx *ctx, uint64_t capacity);
bpg_status bpg_gens_export(bpg_ctx *ctx, uint64_t first, uint64_t count, uint8_t *G_out, uint8_t *H_out);

/* replaces the point part of Prover::commit(v, v_blinding)       (reference src/gadget.rs:31, src/commitments.rs:27,39):
 * out[i] = compress(v[i]*B + blind[i]*B_blinding); v may be an unreduced Scalar::from_bits value */
bpg_status bpg_pedersen_commit(bpg_ctx *ctx, uint64_t k, const uint8_t *v, const uint8_t *blind, uint8_t *out);

/* replaces Prover::prove(&bp_gens) + R1CSProof::to_bytes()        (reference src/bin/prover.rs:93,97).
 * transcript_state: Merlin state after Transcript::new(label), Prover::new and every "V" append; updated in place.
 * rng_seed replaces the 32 bytes upstream draws from thread_rng(). proof_len: in = capacity, out = bytes written. */
bpg_status bpg_r1cs_upload(bpg_ctx *ctx, const bpg_r1cs_instance *inst, bpg_circuit **out);
void bpg_r1cs_free(bpg_ctx *ctx, bpg_circuit *c);
bpg_status bpg_r1cs_prove_resident(bpg_ctx *ctx, bpg_circuit *c, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES],
                                   uint64_t m, const uint8_t *v_blinding, const uint8_t rng_seed[32], uint32_t flags,
                                   uint8_t *proof_out, uint64_t *proof_len, bpg_timings *timings);
bpg_status bpg_r1cs_prove(bpg_ctx *ctx, const bpg_r1cs_instance *inst, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES],
                          uint64_t m, const uint8_t *v_blinding, const uint8_t rng_seed[32], uint32_t flags,
                          uint8_t *proof_out, uint64_t *proof_len);
uint64_t bpg_proof_size(uint64_t n_multipliers, uint32_t flags);

/* replaces R1CSProof::from_bytes + Verifier::verify(&proof, &pc_gens, &bp_gens)   (reference src/bin/verifier.rs:64,89-90).
 * inst: the verifier-side instance (aL/aR/aO NULL, constraints as assembled with None assignments); transcript_state: Merlin
 * state after Verifier::new and every "V" append (updated in place); V: the m commitments; seed replaces the verifier's
 * thread_rng() draw. Returns BPG_OK, BPG_ERR_VERIFICATION, BPG_ERR_FORMAT or BPG_ERR_INVALID_GENERATORS_LENGTH. */
bpg_status bpg_r1cs_verify(bpg_ctx *ctx, const bpg_r1cs_instance *inst, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES],
                           uint64_t m, const uint8_t *V, const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags);

/* the same on an uploaded circuit (prover-side or verifier-side upload): a verifier that checks many proofs of one circuit
 * keeps the constraint matrix in HBM. */
bpg_status bpg_r1cs_verify_resident(bpg_ctx *ctx, bpg_circuit *circuit, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES],
                                    uint64_t m, const uint8_t *V, const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags);

/* Batch verification: many proofs in ONE multiscalar multiplication.  Each item is the argument list of bpg_r1cs_verify (inst) or of
 * bpg_r1cs_verify_resident (circuit, uploaded on this ctx): exactly one of the two is non-NULL.  Items may differ in circuit, n, m and flags.
 * Every item's verification equation is multiplied by an independent random weight rho_k and all of them are summed into one MSM of about
 * 2 N_max + sum_k (npts_k + 2) terms; the batch is accepted iff that sum is the identity.  If it is not, every item is verified alone.
 *   status_out[i] = exactly what bpg_r1cs_verify / bpg_r1cs_verify_resident returns for item i with the same seed (BPG_OK, BPG_ERR_VERIFICATION,
 *                   BPG_ERR_FORMAT or BPG_ERR_INVALID_GENERATORS_LENGTH); transcript_state is left as that call leaves it.
 *   return value  = BPG_OK when every item is accepted, else the status of the first failing item (as bpg_pool_prove).
 * Every argument is checked before any device work: a NULL ctx, NULL items / status_out / batch_seed with count > 0, an item with both or neither of
 * inst / circuit, an m that does not match the item's instance or circuit, or a malformed instance refuse the whole call with BPG_ERR_INVALID_ARGUMENT
 * (no launch, no transcript state touched).  count == 0 returns BPG_OK.
 * The weights rho_k come from a Merlin transcript "bpg-verify-batch-v1" over count, every proof and its replayed transcript state, finalised
 * with batch_seed.  batch_seed MUST be fresh randomness in production, just as each item's seed: a prover who can predict the weights can make
 * two invalid proofs whose errors cancel.  Flat items are uploaded, used and freed one at a time (peak HBM: one flat circuit + 2 N_max scalars). */
typedef struct {
    const bpg_r1cs_instance *inst;   /* verifier-side instance ... */
    bpg_circuit *circuit;            /* ... or a circuit uploaded on this ctx: exactly one of the two is non-NULL */
    uint8_t *transcript_state;       /* 203 B, state after Verifier::new + every "V" append; updated in place as bpg_r1cs_verify does */
    uint64_t m; const uint8_t *V;    /* the m commitments */
    const uint8_t *proof; uint64_t proof_len;
    const uint8_t *seed;             /* 32 B: this item's verifier thread_rng draw, as in bpg_r1cs_verify */
    uint32_t flags;                  /* dialect flags of this item (BPG_FLAG_COMPACT_1PHASE / BPG_FLAG_NO_1PHASE_DOMSEP) */
} bpg_verify_item;
bpg_status bpg_r1cs_verify_batch(bpg_ctx *ctx, uint64_t count, const bpg_verify_item *items, const uint8_t batch_seed[32], bpg_status *status_out);

/* Lockstep verification: K proofs of ONE resident circuit with a constant number of launches per wave of items.  bpg_r1cs_verify_batch gives every item a
 * replay on one host thread and at least seven stream operations of its own; a service that checks many proofs of one shape keeps the circuit resident and
 * calls this instead.  The replays run on the host threads the proving waves use; all live items' points are decoded in one launch; then, per wave of at
 * most BPG_BATCH_WAVE_MB of device state (0: one item per wave), at most six launches whatever K and N compute every item's y^-i and z^j, its flattened
 * weights, w_c and delta, and the rho-weighted G / H scalars of all items into two accumulators; the K small slots come back in one copy, and ONE multiscalar
 * multiplication of 2 N + K (npts + 2) terms decides.  Three host synchronisations.  A rejected sum re-verifies every live item alone, as
 * bpg_r1cs_verify_batch does.
 *   status_out[k] = exactly what bpg_r1cs_verify_resident returns for item k alone on this circuit with that item's constants standing - after
 *                   bpg_r1cs_set_inputs(input_values) and / or a write of param_values into the parameter slots, where the item gives them;
 *                   transcript_state is left as that call leaves it.
 *   return value  = BPG_OK when every item is accepted, else the status of the first failing item.
 * THE CIRCUIT IS NEVER CHANGED: per-item constants live in the call's own buffers, and after the call, accepted or rejected, the coefficient table holds
 * what it held before (the item-by-item pass of a rejected sum writes an item's constants into the table and puts the standing parameter and derived
 * slots back).  A resident witness is neither read nor dropped.
 * Served: any handle with device state (plain upload, template, repeat, join) when every item leaves param_values and input_values NULL; per-item
 * param_values / input_values on a SINGLE template only.  A circuit without multipliers (n = 0) is served inside the call item by item.
 * The whole call is refused with BPG_ERR_INVALID_ARGUMENT - nothing launched, status_out and every transcript state untouched, bpg_last_error names the
 * item and the reason - for: a NULL circuit; NULL items, status_out or batch_seed with count > 0; a NULL transcript_state, proof or seed, or a NULL V with
 * m > 0, in any item; a handle without device state (bpg_test_circuit_handle); a NULL ctx (as bpg_r1cs_verify_batch); a circuit of another context or
 * device; per-item constants on a repeat or a join; param_values on a circuit without parameter rows; input_values on a circuit without public inputs.
 * These checks come first, in this order; count == 0 then returns BPG_OK with nothing launched.
 * The weights are bpg_r1cs_verify_batch's: a Merlin transcript "bpg-verify-batch-v1" over count, every proof and its replayed state, finalised with
 * batch_seed (fresh randomness in production, as there); an item that brings constants has their bytes absorbed behind its state under the labels
 * "params" / "inputs", so a call without per-item constants draws the very weights bpg_r1cs_verify_batch draws for the same items.
 * (An addition to ABI version 7: look the symbol up.) */
typedef struct {                       /* frozen */
    uint8_t *transcript_state;         /* 203 B in/out, as bpg_r1cs_verify_resident */
    const uint8_t *V;                  /* m x 32 (m is the circuit's) */
    const uint8_t *proof; uint64_t proof_len;
    const uint8_t *seed;               /* 32 B */
    uint32_t flags;                    /* dialect flags of this item */
    const uint8_t *param_values;       /* NULL: the circuit's standing parameter slots; else n_params x 32, as bpg_r1cs_assign takes them */
    const uint8_t *input_values;       /* NULL: the standing derived slots; else n_inputs x 32, as bpg_r1cs_set_inputs takes them */
} bpg_verify_resident_item;
bpg_status bpg_r1cs_verify_resident_batch(bpg_ctx *ctx, bpg_circuit *circuit, uint64_t count, const bpg_verify_resident_item *items,
                                          const uint8_t batch_seed[32], bpg_status *status_out);

/* A batch of INDEPENDENT proofs on one GPU.  One proof keeps the device busy for ~45 ms of 340 (the rest is the host's serial Merlin
 * TranscriptRng chain, upstream-exact), so a pool of `workers` engine contexts + host threads proves items concurrently: the chain of
 * one proof overlaps the kernels of the others (8 workers: ~5x the single-proof rate on a 2^20 circuit).  Each item is what
 * bpg_r1cs_prove takes; items are independent (own transcript, witness, seed); results are byte-identical to proving them one by
 * one.  status_out[i] receives the bpg_status of item i; the call returns BPG_OK when every item succeeded, else the first failure. */
typedef struct bpg_pool bpg_pool;
typedef struct {
    const bpg_r1cs_instance *inst;
    uint8_t *transcript_state;            /* 203 B, updated in place */
    uint64_t m; const uint8_t *v_blinding;
    const uint8_t *rng_seed;              /* 32 B */
    uint32_t flags;
    uint8_t *proof_out; uint64_t *proof_len;   /* in = capacity, out = bytes written */
} bpg_batch_item;
bpg_status bpg_pool_create(int32_t device, uint32_t workers, uint64_t gens_capacity, bpg_pool **out);
bpg_status bpg_pool_create_ex(int32_t device, uint32_t workers, uint64_t gens_capacity, const bpg_config *config /* of every context; NULL = defaults */, bpg_pool **out);
void bpg_pool_destroy(bpg_pool *pool);
bpg_status bpg_pool_prove(bpg_pool *pool, uint64_t count, const bpg_batch_item *items, bpg_status *status_out);
/* Many SMALL proofs in lockstep on one context: the proofs of a batch share every launch of the prove pipeline (one per stage for all of them),
 * and their Fiat-Shamir steps run between the stages on up to 16 host threads (the cores the process may use, capped by its CPU quota).
 * proof_out, *proof_len, transcript_state and status_out[i] of each item are exactly what bpg_r1cs_prove(ctx, item...) gives for it alone,
 * byte for byte, whatever the batch around it.  Lockstep: items with 0 < n and padded N <= 2^14 (BPG_TT_ORIG_LG), dialect flags 1 and 2 included;
 * every other item - larger circuits, n = 0, BPG_TT_ORIG_LG=0, and BPG_FLAG_EXPANDED_BLINDING, which always takes this path - is proved by
 * bpg_r1cs_prove inside the same call.  Items are grouped by lg N and each group runs in waves of at most BPG_BATCH_WAVE_MB (default 512;
 * 0 = one proof per wave) of device state (about 30 N x 32 B per proof).
 * A NULL ctx, or NULL items / status_out with count > 0, refuses the whole call (BPG_ERR_INVALID_ARGUMENT, nothing launched or written);
 * count == 0 returns BPG_OK.  Anything else fails per item with bpg_r1cs_prove's status while the other items are proved (NULL pointers in the
 * item, a malformed instance, an m mismatch, a proof buffer below bpg_proof_size, a generator capacity below N).  Returns BPG_OK when every item
 * succeeded, else the status of the first failing item; bpg_last_error names it.  (An addition to ABI version 7.) */
bpg_status bpg_r1cs_prove_batch(bpg_ctx *ctx, uint64_t count, const bpg_batch_item *items, bpg_status *status_out);

/* Circuit templates: assemble once, assign fresh witnesses on the device.  (Additions to ABI version 7, like bpg_r1cs_prove_batch: a host that needs them
 * looks the symbols up.)
 * The shape of a circuit - constraints and wiring - does not depend on the witness.  When every multiplier came from multiply(left, right), its three
 * values are functions of committed values and earlier multipliers, and the device can compute a_L, a_R, a_O itself: a further proof of the same shape
 * needs the m committed values (and the public constants that changed), not a host assembly and a 96 MB upload.
 *
 * The frozen struct bpg_witness_program says how: multiplier i has left = terms [lc_ptr[2i], lc_ptr[2i+1]) and right = [lc_ptr[2i+1], lc_ptr[2i+2]) - the linear
 * combinations handed to multiply(), WITHOUT the -a_L[i] / -a_R[i] terms the constraint rows carry.  A term may name committed values, the constant One
 * and multipliers below i.  param_rows names constraint rows whose CONSTANT TERM changes with the witness (the root in `hash - root = 0`, the image of a
 * preimage proof, the right-hand side of an equality): each such row's constant terms are replaced by one term on a coefficient slot of its own, which
 * starts at their sum (zero for a row without one) and is overwritten by every bpg_r1cs_assign.  Constants that flow INTO MULTIPLICATIONS are part of
 * the program.  Those the gadget code itself brings - MiMC keys, round constants - stay fixed for the life of the template.  The instance values of a
 * statement - the public bound of LessThan, the right-hand side of Inequality, an instance set, the instance siblings of a Merkle pattern - need not:
 * assemble them as PUBLIC INPUTS (bpg_prover_input, below) and every assign brings their values.
 *
 * bpg_r1cs_upload_template = bpg_r1cs_upload plus the program: the witness of `inst`, if it carries one, is uploaded as usual (the first proof needs no
 * assign); with aL = aR = aO = NULL the circuit has no witness until the first bpg_r1cs_assign (proving it before: BPG_ERR_MISSING_ASSIGNMENT).
 * Refused with BPG_ERR_INVALID_ARGUMENT, before any device work, bpg_last_error naming the reason: NULL arguments, n = 0, a malformed instance or program,
 * a term index out of range or naming a multiplier >= i, a parameter row >= q or named twice, and a program whose schedule has more than 4096 levels
 * (the device runs one launch per level of dependent segments; a circuit that is one long dependent chain is assembled on the host).  A circuit with
 * FREE multipliers (allocate / allocate_multiplier) has no program: bpg_prover_witness_program refuses it.  Of the gadgets only range_proof - BoundsCheck,
 * LessThan - allocates multipliers of its own (Inequality and SetMembership use multiply() alone, their derived values are committed), and what it
 * allocates is a function of earlier values after all: see the HINTS below, which make those circuits templates.  An OR block replays its clauses through
 * a recording buffer that keeps the two scalars only: range proofs inside OR blocks stay free multipliers.
 *
 * bpg_r1cs_assign: m committed values (32 bytes each; any value below 2^255 as Scalar::from_bits admits, reduced mod l on the device) and n_params
 * constant terms in the order of param_rows (for `hash - root = 0` the constant term is -root mod l).  m and n_params must match the template, v and
 * param_values must be non-NULL when their count is not zero, the circuit must be a template: else BPG_ERR_INVALID_ARGUMENT, nothing launched.  On
 * return the witness is resident - exactly the scalars a host assembly of the same values uploads - and everything kept for the previous witness (the
 * equal-scalar sets of BPG_MERGE) is dropped.  The circuit is then proved with bpg_r1cs_prove_resident; the caller makes the commitments
 * (bpg_pedersen_commit) and the transcript state itself, as for any resident proof.  bpg_r1cs_verify_resident on a template checks against the constant
 * terms of the last assign. */
typedef struct {
    const uint64_t *lc_ptr;      /* 2n + 1 */
    const uint32_t *term_var;    /* kind << 29 | index, as in bpg_r1cs_instance */
    const uint32_t *term_coef;   /* index into the instance's coef table */
    uint64_t n_params;
    const uint64_t *param_rows;  /* n_params constraint rows whose constant term is assigned per witness */
} bpg_witness_program;
bpg_status bpg_r1cs_upload_template(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, bpg_circuit **out);
/* HINTS: templates for circuits with range proofs.  (Additions to ABI version 7; bpg_witness_program itself is unchanged.)  utils::range_proof allocates,
 * for bit j of a linear combination x, a multiplier with a_L = 1 - b, a_R = b, a_O = 0.  The frozen struct bpg_witness_hints names such multipliers: for a
 * hinted multiplier i the program's LEFT list [lc_ptr[2i], lc_ptr[2i+1]) is the SOURCE x and its right list is empty.
 * SEMANTICS: the device takes bit `arg` of the CANONICAL representative (mod l) of the source's value.  The host's range_proof reads the raw little-endian
 * bytes of the assignment it was handed.  The two agree whenever that assignment is canonical - everything Gadget::setup derives is, and so is every source
 * that is not one single unreduced committed value - and byte identity of proofs with a host assembly is promised for canonical source values only.  Bits
 * above a range's width are ignored on both sides: an out-of-range value gives the same (unsatisfying) witness, and the same proof bytes, as the host.
 * bpg_r1cs_upload_template_hinted: hints == NULL or n_hints == 0 makes it bpg_r1cs_upload_template.  Refused besides, before any device work, with
 * BPG_ERR_INVALID_ARGUMENT and bpg_last_error naming the reason: NULL arrays with n_hints > 0, an index >= n or indices not strictly ascending, an unknown
 * kind, arg >= 256, a hinted multiplier with a non-empty right list, a source naming a multiplier >= i.  bpg_r1cs_assign, bpg_r1cs_prove_resident,
 * bpg_r1cs_verify_resident and bpg_r1cs_prove_template_batch serve a hinted template exactly as they are documented for any template.  In the schedule a
 * run of hints over one source is a segment of its own, one level above what made the source; the source is reduced once per run. */
#define BPG_HINT_BIT_PAIR 1u      /* a_L = 1 - b, a_R = b, a_O = 0; b = bit `arg` (0..255) of the canonical value of the source */
typedef struct {                  /* frozen */
    uint64_t n_hints;
    const uint32_t *hint_mul;     /* strictly ascending multiplier indices */
    const uint32_t *hint_kind;    /* BPG_HINT_* */
    const uint32_t *hint_arg;
} bpg_witness_hints;
bpg_status bpg_r1cs_upload_template_hinted(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, bpg_circuit **out);
bpg_status bpg_r1cs_assign(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values);
/* CHECKPOINTS: known intermediate values flatten bpg_r1cs_assign.  (Additions to ABI version 7; no struct changes.)  The device runs one launch per level of
 * dependent segments, and a hash chain - a preimage of many blocks, a Merkle path - is nothing but dependent segments.  Often the caller knows the values that
 * link them: the sponge states of a preimage (bpg_mimc_sponge_states, microseconds per block on the host), the nodes of a resident tree
 * (bpg_merkle_path_nodes, bpg_merkle_nodes).  The frozen struct bpg_witness_checkpoints names such values: an ordered list of distinct multiplier variables
 * (kind 0, 1 or 2, index below n; bpg_prover_noted lists the candidates a gadget pointed out).  A checkpointed variable is computed like any other, but every term
 * of the program that names it reads the caller's value: the segments stop depending on each other (a preimage: one level; a Merkle path or tree: two), and
 * one more launch compares each value with what the circuit computed for it.
 * bpg_r1cs_upload_template_checkpointed: checkpoints == NULL or n_checkpoints == 0 makes it bpg_r1cs_upload_template_hinted (same schedule, same program bits).
 * Refused besides, before any device work, with BPG_ERR_INVALID_ARGUMENT and bpg_last_error naming the reason: NULL vars, an index >= n, a kind that is no
 * multiplier kind (committed, One), a variable named twice.
 * bpg_r1cs_assign_checkpointed: bpg_r1cs_assign plus the n_ck checkpoint values in the order of vars (32 bytes each, any value below 2^255, reduced mod l on
 * the device as v is).  n_ck must match the template; ck_values non-NULL when n_ck > 0.  When every value is the circuit's own, the resident witness is
 * exactly what bpg_r1cs_assign leaves on a template of the same circuit without checkpoints, and the call returns BPG_OK with *first_mismatch = UINT64_MAX.
 * Otherwise it returns BPG_ERR_CHECKPOINT_MISMATCH, *first_mismatch (NULL allowed) is the lowest flat index item * n_ck + k that differs, bpg_last_error names
 * it, and the circuit is left WITHOUT a witness (bpg_r1cs_prove_resident: BPG_ERR_MISSING_ASSIGNMENT) - an inconsistent witness is never provable.  Either way
 * the equal-scalar sets of the previous witness are dropped, and the call returns synchronised: the host reads the 8-byte result of the comparison back.
 * On a template with checkpoints: bpg_r1cs_template_repeat(K) gives a repeat whose bpg_r1cs_assign_checkpointed takes K x n_ck values, item-major; plain
 * bpg_r1cs_assign, bpg_r1cs_prove_template_batch and bpg_r1cs_prove_template_batch_commit are refused with BPG_ERR_INVALID_ARGUMENT before any work (their
 * frozen arguments carry no checkpoint values: bpg_r1cs_prove_template_batch_checkpointed is the lockstep batch that does); bpg_r1cs_check, bpg_r1cs_prove_resident and bpg_r1cs_verify_resident serve it unchanged.  On a template
 * without checkpoints bpg_r1cs_assign_checkpointed with n_ck = 0 is bpg_r1cs_assign. */
typedef struct {                  /* frozen */
    uint64_t n_checkpoints;
    const uint32_t *vars;         /* kind << 29 | index: distinct multiplier variables (kind 0..2) */
} bpg_witness_checkpoints;
bpg_status bpg_r1cs_upload_template_checkpointed(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                 const bpg_witness_checkpoints *checkpoints, bpg_circuit **out);
bpg_status bpg_r1cs_assign_checkpointed(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values,
                                        uint64_t n_ck, const uint8_t *ck_values /* n_ck x 32 */, uint64_t *first_mismatch);
/* K fresh witnesses of ONE template proved in lockstep: bpg_r1cs_prove_batch without the host assembly and without the witness upload.  Each item brings
 * what bpg_r1cs_assign takes (v: m committed values, any value below 2^255; param_values: n_params constant terms in the order of param_rows) and what
 * bpg_r1cs_prove_resident takes (transcript state after every "V" append, m blindings, the seed, flags, the proof buffer).  proof_out, *proof_len,
 * transcript_state and status_out[k] of item k are exactly what bpg_r1cs_assign(ctx, tmpl, m, v, n_params, param_values) followed by
 * bpg_r1cs_prove_resident(ctx, tmpl, ...) gives for it alone, byte for byte, whatever the batch around it and however it is cut into waves.
 * Lockstep: a template with padded N <= 2^14 (BPG_TT_ORIG_LG), dialect flags 1 and 2 included.  The witnesses of a wave are computed on the device in
 * one launch per schedule level for ALL its items (a lane per segment and item), straight into the wave's a_L, a_R, a_O; every later stage is shared
 * as in bpg_r1cs_prove_batch, in waves of at most BPG_BATCH_WAVE_MB (same rule).  Every other item - a template with N > 2^14, BPG_TT_ORIG_LG=0, and
 * BPG_FLAG_EXPANDED_BLINDING - is proved inside the call by bpg_r1cs_assign + bpg_r1cs_prove_resident, one at a time, in item order.
 * The whole call is refused with BPG_ERR_INVALID_ARGUMENT, nothing launched and nothing written, for a NULL ctx or tmpl, a circuit that is not a
 * template, a handle without device state (bpg_test_circuit_handle), and NULL items / status_out with count > 0; count == 0 returns BPG_OK.
 * Anything else fails per item while the other items are proved: a NULL v with m > 0, a NULL param_values with n_params > 0, a NULL transcript,
 * blinding, seed, proof or length pointer and a proof buffer below bpg_proof_size (BPG_ERR_INVALID_ARGUMENT), a generator capacity below N
 * (BPG_ERR_INVALID_GENERATORS_LENGTH).  Returns BPG_OK when every item succeeded, else the status of the first failing item; bpg_last_error names it.
 * AFTERWARDS (count > 0, whole-call checks passed, on either path) the template holds NO witness: bpg_r1cs_prove_resident returns
 * BPG_ERR_MISSING_ASSIGNMENT until the next bpg_r1cs_assign, the equal-scalar sets of BPG_MERGE are dropped, and the parameter slots are unspecified
 * (assign before bpg_r1cs_verify_resident).  (An addition to ABI version 7.) */
typedef struct {
    const uint8_t *v;                     /* m x 32: committed values, as bpg_r1cs_assign takes them */
    const uint8_t *param_values;          /* n_params x 32, in the order of param_rows */
    uint8_t *transcript_state;            /* 203 B, after every "V" append; updated in place */
    const uint8_t *v_blinding;            /* m x 32 */
    const uint8_t *rng_seed;              /* 32 B */
    uint32_t flags;
    uint8_t *proof_out; uint64_t *proof_len;   /* in = capacity, out = bytes written */
} bpg_template_item;
bpg_status bpg_r1cs_prove_template_batch(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_item *items, bpg_status *status_out);
/* The same batch MAKING ITS OWN PEDERSEN COMMITMENTS: from (values, blindings, transcript before the commitments) to (commitments, proofs, transcripts) in
 * one call, where bpg_r1cs_prove_template_batch has the caller create a transcript and a prover per item, commit m times (a launch and a round trip each)
 * and append.  The frozen struct bpg_template_commit_item has the fields of bpg_template_item, with two differences: transcript_state comes IN as the state
 * BEFORE the "V" appends - as Prover::new leaves it - and goes OUT as the state after the proof; commitments_out receives the item's m commitments (m x 32
 * bytes, RFC 9496 encodings, in commit order).  Commitment j of item k is what bpg_pedersen_commit(ctx, 1, v + 32 j, v_blinding + 32 j, ...) writes: v with
 * Scalar::from_bits semantics (any value below 2^255), the blinding reduced mod l.  The library appends the m encodings to the item's transcript in order, as
 * append_point(b"V", ...), exactly as Prover::commit does; proof_out, *proof_len, the out-state and status_out[k] are then byte for byte those of
 * bpg_r1cs_prove_template_batch given that post-commit state, whatever the batch around the item and however it is cut into waves.
 * A caller that interleaves OTHER transcript appends between its commits (or commits in another order than v lists them) cannot use this call: all m
 * appends happen back to back on the state handed in.  Such a caller commits itself and calls bpg_r1cs_prove_template_batch.
 * Lockstep (the rule of bpg_r1cs_prove_template_batch): a wave's commitments are made in ONE launch from the values the wave has uploaded for its witness
 * evaluation and read back with one copy; the witness evaluation runs while the host appends.  The other items (a template with N > 2^14, BPG_TT_ORIG_LG=0,
 * BPG_FLAG_EXPANDED_BLINDING) get all their commitments from one Pedersen launch up front and are then proved one at a time as before.
 * Whole-call and per-item refusals are those of bpg_r1cs_prove_template_batch, and a NULL commitments_out with m > 0 fails that item alone
 * (BPG_ERR_INVALID_ARGUMENT).  For an item that fails, no commitment is written and its transcript is untouched; the other items are proved.  m = 0: the
 * existing call (commitments_out is not looked at).  The template AFTERWARDS: as documented above.  (An addition to ABI version 7: look the symbol up.) */
typedef struct {
    const uint8_t *v;                     /* m x 32: committed values, as bpg_r1cs_assign takes them */
    const uint8_t *param_values;          /* n_params x 32, in the order of param_rows */
    uint8_t *transcript_state;            /* 203 B, in: BEFORE the "V" appends; out: after the proof */
    const uint8_t *v_blinding;            /* m x 32 */
    const uint8_t *rng_seed;              /* 32 B */
    uint32_t flags;
    uint8_t *proof_out; uint64_t *proof_len;   /* in = capacity, out = bytes written */
    uint8_t *commitments_out;             /* m x 32: the commitments, in commit order */
} bpg_template_commit_item;
bpg_status bpg_r1cs_prove_template_batch_commit(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_commit_item *items, bpg_status *status_out);
/* The same batches for a CHECKPOINTED template: K hash-chain proofs - preimages, Merkle paths against a resident tree - whose witnesses a wave evaluates in
 * the one or two levels of the checkpointed schedule where the template without checkpoints runs one launch per dependent block.  The frozen struct
 * bpg_template_ck_item has the nine fields of bpg_template_commit_item, same order and meaning, then ck_values - what bpg_r1cs_assign_checkpointed takes for
 * this template, n_ck x 32 bytes, any value below 2^255 - and first_mismatch.  commit == 0: the semantics of bpg_r1cs_prove_template_batch (transcript_state
 * comes in AFTER the "V" appends, commitments_out is not looked at); commit != 0: those of bpg_r1cs_prove_template_batch_commit (the state comes in BEFORE
 * the commitments; the library commits and appends).
 * For an item whose checkpoint values are the circuit's own, proof_out, *proof_len, the out-state, commitments_out and status_out[k] are byte for byte what
 * bpg_r1cs_assign_checkpointed followed by bpg_r1cs_prove_resident gives for that item alone (with bpg_pedersen_commit and the "V" appends first when commit
 * is set), whatever the batch around it and however it is cut into waves; *first_mismatch (NULL allowed) reads UINT64_MAX.
 * An item with a value that is NOT the circuit's own fails alone with BPG_ERR_CHECKPOINT_MISMATCH: nothing of it is written - no proof, no commitment, its
 * transcript state as given - *first_mismatch receives its lowest bad checkpoint (on a repeat or join: the flat index bpg_r1cs_assign_checkpointed reports),
 * bpg_last_error names the item and the checkpoint when it is the first failure, and every other item is proved.  In a lockstep wave such an item rides to
 * the wave's end - the comparison (k_witness_ck_verify_batch, one launch per wave) comes back with the copy of A_I, A_O, S the wave makes anyway - and what it
 * made is thrown away: an inconsistent witness never leaves the call as a proof.
 * Whole-call and per-item refusals are those of the two calls above; a NULL ck_values with n_ck > 0 fails that item alone (BPG_ERR_INVALID_ARGUMENT).
 * Lockstep: the rule of bpg_r1cs_prove_template_batch.  Every other item - a template with N > 2^14, BPG_TT_ORIG_LG=0, BPG_FLAG_EXPANDED_BLINDING, and a
 * repeat or join, which keep no host copy of their rows - runs bpg_r1cs_assign_checkpointed + bpg_r1cs_prove_resident in item order (with commit set, all
 * their commitments come from one Pedersen launch up front), and a mismatch is reported in the same way.  On a template WITHOUT checkpoints the call is
 * exactly the call above that `commit` selects, byte for byte (ck_values is not looked at).  The template AFTERWARDS: as documented above - no witness.
 * (An addition to ABI version 7: look the symbol up.) */
typedef struct {                          /* frozen */
    const uint8_t *v;                     /* m x 32: committed values, as bpg_r1cs_assign takes them */
    const uint8_t *param_values;          /* n_params x 32, in the order of param_rows */
    uint8_t *transcript_state;            /* 203 B, in: commit == 0 after every "V" append, else BEFORE them; out: after the proof */
    const uint8_t *v_blinding;            /* m x 32 */
    const uint8_t *rng_seed;              /* 32 B */
    uint32_t flags;
    uint8_t *proof_out; uint64_t *proof_len;   /* in = capacity, out = bytes written */
    uint8_t *commitments_out;             /* commit != 0: m x 32, the commitments in commit order */
    const uint8_t *ck_values;             /* n_ck x 32, what bpg_r1cs_assign_checkpointed takes for this template */
    uint64_t *first_mismatch;             /* NULL allowed; out: UINT64_MAX, or the lowest mismatching checkpoint of THIS item */
} bpg_template_ck_item;
bpg_status bpg_r1cs_prove_template_batch_checkpointed(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_ck_item *items, int32_t commit,
                                                      bpg_status *status_out);
/* PUBLIC INPUTS in circuit templates: instance values that change per proof.  (Additions to ABI version 7; the frozen structs are unchanged.)
 * A public input is a scalar x_p known to prover and verifier.  bpg_prover_input / bpg_verifier_input hand its value over and return a variable of kind
 * BPG_VAR_INPUT, index p counting from 0, which is named in linear combinations like any variable: a caller passes it wherever it passed a constant before
 * (right_hand of LessThan and Inequality, instance_vars of SetMembership and MerkleTree256, root, image).  Gadget code does not change.  To the proof system
 * a term (input p, c) IS the constant c x_p: a proof made from a template with inputs X is byte for byte the proof of a fresh host assembly with those constants
 * (the transcript holds no constraint, the prover reads no constant term).
 * RESOLVED EXPORT: bpg_prover_instance, bpg_verifier_instance and everything built on them (bpg_prover_prove, bpg_verifier_verify, the oracle) fold every such
 * term into a constant term on the product c x_p (new products behind the table's own entries); they never show kind 5, and an assembly without inputs
 * exports bit for bit what it always did.  TEMPLATE EXPORT: bpg_prover_template_instance keeps the terms (coefficients interned as for any term), returns the
 * n_inputs values in input order, and bpg_prover_witness_program(_hinted) on such a prover keeps them in the program too, hint sources included.
 * bpg_r1cs_upload_template_inputs: bpg_r1cs_upload_template_checkpointed for such an instance and program.  n_inputs == 0 makes it that call (same schedule,
 * same record stream).  input_values (n_inputs x 32): the inputs of the witness `inst` carries; NULL only when it carries none.  An input is read like a
 * committed value: a level-0 source of the schedule (LessThan against a public bound: the 4 segments on 1 level of LessThan against a constant).  In the rows
 * a term (input p, coefficient index ci) becomes a constant term on a DERIVED coefficient slot, one per distinct pair, behind the parameter slots; every assign
 * fills it with coef[ci] x_p on the device (k_input_slots) before anything reads a constant term.  Refused besides, with BPG_ERR_INVALID_ARGUMENT before any
 * device work and bpg_last_error naming the reason: an input index >= n_inputs (in a row or in the program), an input term in a hint's right list (which is
 * empty), NULL input_values for an instance with a witness, more derived slots than the coefficient index holds (2^30 with the table and the parameters).
 * bpg_r1cs_assign_inputs: bpg_r1cs_assign_checkpointed plus the n_inputs values (32 bytes each, any value below 2^255, reduced mod l on the device as v is).
 * n_inputs must match the template; input_values non-NULL when n_inputs > 0.  CANONICAL INPUTS ONLY: as for the bit hints above, byte identity with a host
 * assembly is promised when the value handed over is canonical (below l) - the host's range_proof reads the raw bytes of the assignment it was handed, the
 * device the canonical representative.  A refused or mismatching call leaves the circuit without a witness; the equal-scalar sets are dropped as by every assign.
 * bpg_r1cs_prove_template_batch_inputs: bpg_r1cs_prove_template_batch_checkpointed with the frozen struct bpg_template_in_item - the eleven fields of
 * bpg_template_ck_item, same order and meaning, then input_values, what bpg_r1cs_assign_inputs takes for this template.  Each item is byte for byte
 * bpg_r1cs_assign_inputs + bpg_r1cs_prove_resident for it alone (commitments first when commit is set).  A NULL input_values with n_inputs > 0 fails that item
 * alone.  In a lockstep wave the inputs travel beside the checkpoint values, the witness evaluation reads item k's inputs, and one launch of k_input_slots
 * writes every item's derived slots into its range of the wave's coefficient table.  Items off the lockstep path (N > 2^14, BPG_TT_ORIG_LG=0, expanded
 * blinding) run bpg_r1cs_assign_inputs + bpg_r1cs_prove_resident in item order.  On a template WITHOUT inputs it is that call, byte for byte.
 * On a template WITH inputs: bpg_r1cs_assign, bpg_r1cs_assign_checkpointed, bpg_r1cs_prove_template_batch, _commit and _checkpointed are refused with
 * BPG_ERR_INVALID_ARGUMENT before any work (their arguments carry no input values), as the frozen calls refuse a checkpointed template;
 * bpg_r1cs_template_repeat and bpg_r1cs_template_join refuse it as a source, and with them the repeat-based batch check of the Python layer
 * (bpg_r1cs_template_repeat_inputs and bpg_r1cs_template_join_inputs below serve it, with per-item inputs); bpg_r1cs_prove_resident, bpg_r1cs_verify_resident and bpg_r1cs_check serve it as any template -
 * bpg_r1cs_verify_resident checks against the inputs of the last assign. */
typedef struct {                          /* frozen */
    const uint8_t *v;                     /* m x 32: committed values, as bpg_r1cs_assign takes them */
    const uint8_t *param_values;          /* n_params x 32, in the order of param_rows */
    uint8_t *transcript_state;            /* 203 B, in: commit == 0 after every "V" append, else BEFORE them; out: after the proof */
    const uint8_t *v_blinding;            /* m x 32 */
    const uint8_t *rng_seed;              /* 32 B */
    uint32_t flags;
    uint8_t *proof_out; uint64_t *proof_len;   /* in = capacity, out = bytes written */
    uint8_t *commitments_out;             /* commit != 0: m x 32, the commitments in commit order */
    const uint8_t *ck_values;             /* n_ck x 32, what bpg_r1cs_assign_checkpointed takes for this template */
    uint64_t *first_mismatch;             /* NULL allowed; out: UINT64_MAX, or the lowest mismatching checkpoint of THIS item */
    const uint8_t *input_values;          /* n_inputs x 32, what bpg_r1cs_assign_inputs takes for this template */
} bpg_template_in_item;
bpg_status bpg_r1cs_upload_template_inputs(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *input_values /* n_inputs x 32 */,
                                           bpg_circuit **out);
bpg_status bpg_r1cs_assign_inputs(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t n_params, const uint8_t *param_values,
                                  uint64_t n_ck, const uint8_t *ck_values, uint64_t *first_mismatch, uint64_t n_inputs, const uint8_t *input_values /* n_inputs x 32 */);
bpg_status bpg_r1cs_prove_template_batch_inputs(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, const bpg_template_in_item *items, int32_t commit,
                                                bpg_status *status_out);
/* The hooks below for a program with public inputs (no device): n_inputs as bpg_r1cs_upload_template_inputs takes it, input_values n_inputs x 32 (the batch
 * hook: count x n_inputs x 32, item-major).  The eval hooks are their _checkpointed siblings - the same interpreter compiled for the host, the same poison of
 * a_L, a_R, a_O, the same reverse segment order within a level.  bpg_test_template_inputs_instance: the resident rows, row-major, as an assign of param_values
 * and input_values leaves them (the counterpart of bpg_test_template_repeat_instance: every input term a constant term on its derived slot).
 * bpg_test_circuit_handle_inputs: bpg_test_circuit_handle_hinted for such a program. */
bpg_status bpg_test_template_schedule_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                             const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, char *out, uint64_t cap);
bpg_status bpg_test_template_packed_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                           const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint32_t *stream_out, uint64_t cap, uint64_t *words_out);
bpg_status bpg_test_template_eval_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                         const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *v, const uint8_t *ck_values,
                                         const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch);
bpg_status bpg_test_template_eval_batch_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                               const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint64_t count, const uint8_t *v,
                                               const uint8_t *ck_values, const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                               uint64_t *first_mismatch_out);
bpg_status bpg_test_template_inputs_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs,
                                             const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var,
                                             uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out);
bpg_status bpg_test_circuit_handle_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, bpg_circuit **out);
/* ---- Gated variables: a term whose coefficient is a public input of the proof (an addition to ABI version 7).
 *
 * g = bpg_prover_gate(x, var) / bpg_verifier_gate(x, var): a new variable of kind BPG_VAR_GATED whose value is x * var.  x is a variable of kind
 * BPG_VAR_INPUT made by THIS prover or verifier, var a variable of kind 0..3 (a multiplier variable or a committed value) that exists already; the index of g
 * is the gate's position in the object's gate table of (var, input) pairs, in call order.  g is named in linear combinations like any variable, under any
 * coefficient (the bpg_lc layout does not change).  Refused with BPG_ERR_INVALID_ARGUMENT: an x that is no input of this object, a var of kind One, Input or
 * Gated, an index out of range.  Constraint buffers (bpg_buffer, bpg_or_*) offer no gates and refuse a combination that names one.
 *
 * Every RESOLVED export - bpg_prover_instance, bpg_prover_prove, bpg_verifier_verify, bpg_verifier_instance - treats a term (gate k, c) as (var_k, c * x_p),
 * the product in the coefficient table behind the table's own entries exactly as an input's product is: no such export shows kind 6, and with the values
 * bpg_merkle_path_inputs makes a gated circuit IS the ungated circuit of those values.  bpg_prover_template_instance and bpg_prover_witness_program(_hinted)
 * KEEP gated terms (hint sources included); bpg_prover_gates exports the table beside them (pointers valid until the next call on the prover).
 *
 * bpg_r1cs_upload_template_gated: bpg_r1cs_upload_template_inputs plus the gate table; gates == NULL or n_gates == 0 makes it that call (same schedule, record
 * stream and slot layout, bit for bit).  In the rows a term (gate k, ci) becomes (var_k, derived slot of the pair (p_k, ci)): the slot list of the constant
 * input terms, one slot per distinct pair whoever names it.  The resulting template is served by bpg_r1cs_assign_inputs (with checkpoints: a gate over a
 * checkpointed variable reads the caller's value), bpg_r1cs_prove_resident, bpg_r1cs_verify_resident, bpg_r1cs_set_inputs, bpg_r1cs_check,
 * bpg_r1cs_prove_template_batch_inputs and bpg_r1cs_verify_resident_batch with per-item input_values.  bpg_r1cs_template_repeat(_inputs) and
 * bpg_r1cs_template_join(_inputs) refuse it (BPG_ERR_INVALID_ARGUMENT, before any device work).  Kind 6 in an instance or program handed to any other entry
 * point is refused the way kind 5 is.
 *
 * bpg_merkle_path256_new: the Merkle path gadget whose leaf index is a public input - `levels` holds 4 variables of kind BPG_VAR_INPUT per level, bottom level
 * first: (nb, b, c1, c2); the node above running hash h absorbs gate(nb, h) + c1, then gate(b, h) + c2; `leaf` is a variable of kind 0..3.  It makes gates, so
 * it is assembled with bpg_gadget_prove / bpg_gadget_verify only.  bpg_merkle_path_inputs: the 4 * depth + 1 input values for leaf `index` (bit j of it: b_j;
 * nb_j = 1 - b_j; the sibling in c1_j where b_j = 1, in c2_j where it is 0, zero in the other; then the root).  A verifier MUST build its inputs with this
 * call from an index and siblings: arbitrary input values state something else than membership. */
#define BPG_VAR_GATED 6u
typedef struct {
    uint64_t n_gates;
    const uint32_t *gate_var;             /* n_gates: packed variable of kind 0..3 */
    const uint32_t *gate_input;           /* n_gates: index of the public input */
} bpg_witness_gates;
bpg_status bpg_r1cs_upload_template_gated(bpg_ctx *ctx, const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const uint8_t *input_values /* n_inputs x 32 */,
                                          const bpg_witness_gates *gates, bpg_circuit **out);
bpg_status bpg_merkle_path_inputs(uint64_t index, const uint8_t *siblings /* depth x 32 */, uint64_t depth, const uint8_t root[32],
                                  uint8_t *inputs_out /* (4 * depth + 1) x 32 */);
/* the _inputs hooks above for a program with gates: the same calls with the gate table (NULL: the _inputs hook itself) */
bpg_status bpg_test_template_schedule_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                            const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, char *out, uint64_t cap);
bpg_status bpg_test_template_packed_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                          const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, uint32_t *stream_out,
                                          uint64_t cap, uint64_t *words_out);
bpg_status bpg_test_template_eval_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                        const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, const uint8_t *v,
                                        const uint8_t *ck_values, const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch);
bpg_status bpg_test_template_eval_batch_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                              const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, uint64_t count,
                                              const uint8_t *v, const uint8_t *ck_values, const uint8_t *input_values, uint8_t *aL, uint8_t *aR, uint8_t *aO,
                                              uint64_t *first_mismatch_out);
bpg_status bpg_test_template_gated_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs,
                                            const bpg_witness_gates *gates, const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr,
                                            uint64_t row_cap, uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap,
                                            uint64_t *nnz_out, uint64_t *ncoef_out);
bpg_status bpg_test_circuit_handle_gated(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                         const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, const bpg_witness_gates *gates, bpg_circuit **out);
/* TEST HOOKS, no device needed.  bpg_test_template_schedule: the checks of bpg_r1cs_upload_template and the schedule as JSON {"levels", "segments",
 * "max_levels", "seg_first": [segments + 1], "seg_level": [...], "level_segments": [...]}: segment s is multipliers [seg_first[s], seg_first[s+1]), one
 * device lane walks it in order, and everything it reads from another segment lies at a lower level.  bpg_test_template_eval: the device's interpreter
 * compiled for the host over the same packed program (a_L, a_R, a_O out, n x 32 bytes each).  bpg_test_template_eval_batch: the BATCHED interpreter
 * likewise, `count` witnesses (v: count x m x 32) into the wave layout of a lockstep batch: count x N x 32 bytes per vector, item-major, N = n padded to a
 * power of two, rows [n, N) of every item zero.  bpg_test_circuit_handle: a handle WITHOUT device state for
 * the argument checks of bpg_r1cs_assign (program NULL: a plain circuit); every call that needs the device refuses it, bpg_r1cs_free(NULL, c) frees it.
 * Any function added later that takes a bpg_circuit must refuse such a handle (its device state is NULL) before it touches the device. */
bpg_status bpg_test_template_schedule(const bpg_r1cs_instance *inst, const bpg_witness_program *program, char *out, uint64_t cap);
bpg_status bpg_test_template_eval(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out);
bpg_status bpg_test_template_eval_batch(const bpg_r1cs_instance *inst, const bpg_witness_program *program, uint64_t count, const uint8_t *v,
                                        uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out);
bpg_status bpg_test_circuit_handle(const bpg_r1cs_instance *inst, const bpg_witness_program *program, bpg_circuit **out);
/* the append step of bpg_r1cs_prove_template_batch_commit alone: state_out = state_in after append_point(b"V", coms + 32 j) for j = 0 .. m - 1 */
bpg_status bpg_test_append_commitments(const uint8_t state_in[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *coms, uint8_t state_out[BPG_TRANSCRIPT_STATE_BYTES]);
/* the same four for a program with hints (hints == NULL: the calls above) */
bpg_status bpg_test_template_schedule_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, char *out, uint64_t cap);
bpg_status bpg_test_template_eval_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, const uint8_t *v,
                                         uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out);
bpg_status bpg_test_template_eval_batch_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                               const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out);
/* The same hooks for a program with checkpoints (no device).  bpg_test_template_eval_checkpointed shows what one thread running the segments in order would hide -
 * a term the packer did not redirect to the caller's value, which reads another lane of the same level: a_L, a_R, a_O start as a poison value, the segments of every
 * level run in REVERSE order, then the comparison step; *first_mismatch as bpg_r1cs_assign_checkpointed reports it.  bpg_test_template_packed: the packed record
 * stream (host/witness_record.hpp) - *words_out its length; cap = 0 only asks for the length. */
bpg_status bpg_test_template_schedule_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                   const bpg_witness_checkpoints *checkpoints, char *out, uint64_t cap);
bpg_status bpg_test_template_eval_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                               const bpg_witness_checkpoints *checkpoints, const uint8_t *v, const uint8_t *ck_values,
                                               uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch);
bpg_status bpg_test_template_packed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                    const bpg_witness_checkpoints *checkpoints, uint32_t *stream_out, uint64_t cap, uint64_t *words_out);
/* bpg_test_template_eval_batch_hinted for a program with checkpoints, as a wave of bpg_r1cs_prove_template_batch_checkpointed evaluates it: ck_values holds
 * count x n_ck x 32 bytes, item-major; rows [0, n) of every item start as the poison value and the segments of every level run in reverse order (the discipline
 * of bpg_test_template_eval_checkpointed), rows [n, N) are zero; then the comparison step per item: first_mismatch_out[k] (count of them) = UINT64_MAX, or the
 * lowest checkpoint of item k whose value is not the circuit's own. */
bpg_status bpg_test_template_eval_batch_checkpointed(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                     const bpg_witness_checkpoints *checkpoints, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                     uint8_t *aL, uint8_t *aR, uint8_t *aO, uint64_t *first_mismatch_out);
bpg_status bpg_test_circuit_handle_hinted(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, bpg_circuit **out);
/* A TEMPLATE REPEATED K TIMES ON THE DEVICE: one proof for K witnesses of one circuit shape.  bpg_r1cs_template_repeat makes a new resident TEMPLATE from a
 * template uploaded with bpg_r1cs_upload_template(_hinted): the circuit a host gets by assembling the template's gadget code `count` times in a row into ONE
 * prover, each time with fresh variables.  Sizes: n' = count n, q' = count q, m' = count m, n_params' = count n_params.  Copy k of the template:
 * multiplier i -> k n + i, committed value j -> k m + j, constraint row r -> k q + r, parameter row p -> parameter k n_params + p (item-major); the
 * constant One and every coefficient that is no parameter slot are shared.  The matrix is replicated on the device from the template's resident copy; the
 * host never sees a row, so a template of any size can be repeated.  The proof of the repeat has bpg_proof_size(count n, flags) bytes - it grows with
 * log(count n), where count separate proofs grow with count - and is checked by ONE verification.
 * The result is a template like any other: bpg_r1cs_assign takes count m values and count n_params constants, both item-major, and evaluates every item
 * with the source's witness program, one launch per schedule level of the SOURCE and a lane per (segment, item), hinted segments included;
 * bpg_r1cs_prove_resident, bpg_r1cs_verify_resident, bpg_r1cs_verify_batch and bpg_r1cs_free serve it as documented for templates.  It starts WITHOUT a
 * witness, whatever the source holds (its parameter slots start as the source's stand), owns copies of everything it needs - the source may be freed
 * first, the two are used independently - and keeps no host copy of its rows: bpg_r1cs_prove_template_batch(_commit) prove its items one at a time.
 * The caller makes the count m commitments itself (one bpg_pedersen_commit launch) and appends them to the transcript in item order.
 * Refused with BPG_ERR_INVALID_ARGUMENT before any device work (bpg_last_error names the reason): a NULL ctx, tmpl or out; count == 0; a circuit that
 * is not a template; a handle without device state (bpg_test_circuit_handle); a circuit that is itself a repeat or a join (bpg_r1cs_template_join: join
 * its parts with larger counts instead); count n >= 2^27, count m >= 2^29,
 * count q or count nnz >= 2^32, 3 count n + count m + 1 >= 2^32, or 2^30 and more coefficient slots.  The generator capacity is checked when the repeat
 * is proved or verified, as for every circuit.  (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_r1cs_template_repeat(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, bpg_circuit **out);
/* TEST HOOKS, no device needed (hints may be NULL).  bpg_test_template_repeat_instance: the repeated instance, row-major, as it stands after a
 * bpg_r1cs_assign with param_values (count x n_params x 32, item-major; NULL: the slots keep the constants the template's rows carry).  Every parameter
 * row's constant terms are ONE term on a slot of its own, the last of its row (as in the resident template).  row_ptr: count q + 1 entries (row_cap);
 * term_var / term_coef: *nnz_out entries, at most count (nnz + n_params) (term_cap); coef: *ncoef_out = ncoef + count n_params scalars (coef_cap, in
 * scalars).  A buffer that is too short is refused and named.  bpg_test_template_eval_repeat: the repeat-layout interpreter of bpg_r1cs_assign compiled for
 * the host: v = count x m x 32 in, count x n x 32 bytes per vector out. */
bpg_status bpg_test_template_repeat_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                             const uint8_t *param_values, uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var, uint32_t *term_coef,
                                             uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out);
bpg_status bpg_test_template_eval_repeat(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t count,
                                         const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out);
/* TEMPLATES JOINED ON THE DEVICE: one proof for a mixed statement - "these k1 values are in range AND these k2 leaves are in the tree AND this preimage
 * hashes to that image".  bpg_r1cs_template_join makes a new resident TEMPLATE from n_parts pairs (template, count): the circuit a host gets by assembling, in
 * ONE prover, part 0's gadget code count_0 times, then part 1's count_1 times, and so on, each time with fresh variables.  bpg_r1cs_template_repeat(K) is the
 * join of one part.  Write n_p, m_p, q_p, n_params_p, n_ck_p, K_p for part p and B^x_p for the sum of K x over the parts before p.  Copy k of part p:
 * multiplier i -> B^n_p + k n_p + i, committed value j -> B^m_p + k m_p + j, constraint row r -> B^q_p + k q_p + r, parameter s -> B^par_p + k n_params_p + s,
 * checkpoint c -> B^ck_p + k n_ck_p + c: part-major, then item-major.  The coefficient table is [shared of part 0 | shared of part 1 | ... | the parameter
 * slots in the order above]; shared coefficients are not merged across parts (no proof byte can tell).  The matrices are replicated on the device from the
 * parts' resident copies - no host assembly per (k1, k2), no template cache per shape; the same template may be named by several parts.
 * The result is a template like any other: bpg_r1cs_assign takes the sum of K_p m_p values and the sum of K_p n_params_p constants in the order above and
 * evaluates every part with its own witness program in ONE launch per level - as many launches as the part with the most levels has, so a level of a hash
 * part runs beside the other parts' lanes, not after them.  When any part has checkpoints, plain bpg_r1cs_assign is refused and
 * bpg_r1cs_assign_checkpointed takes the sum of K_p n_ck_p values; *first_mismatch is the flat index in that joined list and bpg_last_error names (part,
 * item, checkpoint).  bpg_r1cs_prove_resident, bpg_r1cs_verify_resident, bpg_r1cs_verify_batch, bpg_r1cs_check and bpg_r1cs_free serve it as documented for
 * templates.  It starts WITHOUT a witness (its parameter slots start as the sources' stand), owns copies of everything it needs - any source may be freed
 * first - and keeps no host copy of its rows: bpg_r1cs_prove_template_batch(_commit) prove its items one at a time.
 * Refused with BPG_ERR_INVALID_ARGUMENT before any device work (bpg_last_error names the part and the reason): a NULL ctx, parts or out; n_parts == 0 or
 * above 256; a NULL part or count == 0; a part that is no template, has no device state (bpg_test_circuit_handle), is itself a repeat or a join (name the
 * source template and a count instead), or lives on another context's device; totals beyond the limits of bpg_r1cs_template_repeat (n' >= 2^27,
 * m' >= 2^29, q' or nnz' >= 2^32, columns, coefficient slots).  (An addition to ABI version 7: look the symbol up.) */
typedef struct { bpg_circuit *tmpl; uint64_t count; } bpg_template_part;      /* frozen */
bpg_status bpg_r1cs_template_join(bpg_ctx *ctx, uint64_t n_parts, const bpg_template_part *parts, bpg_circuit **out);
/* TEST HOOKS, no device needed.  A part of a join for them: the template's instance, program, hints and checkpoints (either may be NULL) and its count.
 * bpg_test_template_join_instance: the joined instance, row-major, in the form bpg_test_template_repeat_instance returns, as it stands after a
 * bpg_r1cs_assign with param_values (the joined parameters x 32; NULL: the slots keep the constants the parts' rows carry).  row_ptr: q' + 1 entries;
 * term_var / term_coef: *nnz_out entries; coef: *ncoef_out scalars.  A buffer that is too short is refused and named.
 * bpg_test_template_eval_join: the join-layout interpreter of bpg_r1cs_assign(_checkpointed) compiled for the host, in the order that shows what in-order
 * execution would hide: the vectors start as a poison value, the levels run in order and within a level the parts and their segments in REVERSE order, then
 * the checkpoints are compared.  v = m' x 32, ck_values = n_ck' x 32 (NULL when no part has checkpoints) in; n' x 32 bytes per vector and the first
 * mismatching flat checkpoint index (UINT64_MAX: none) out. */
typedef struct { const bpg_r1cs_instance *inst; const bpg_witness_program *program; const bpg_witness_hints *hints; const bpg_witness_checkpoints *checkpoints;
                 uint64_t count; } bpg_test_join_part;
bpg_status bpg_test_template_join_instance(uint64_t n_parts, const bpg_test_join_part *parts, const uint8_t *param_values, uint64_t *row_ptr, uint64_t row_cap,
                                           uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out,
                                           uint64_t *ncoef_out);
bpg_status bpg_test_template_eval_join(uint64_t n_parts, const bpg_test_join_part *parts, const uint8_t *v, const uint8_t *ck_values, uint8_t *aL_out,
                                       uint8_t *aR_out, uint8_t *aO_out, uint64_t *first_mismatch);
/* PUBLIC INPUTS THROUGH REPEAT AND JOIN: K statements against K different public values - bounds, sets, roots, sibling lists - as ONE proof.  The frozen calls
 * above keep refusing a template with public inputs; the capability comes through the entry points below.  On a template WITHOUT inputs each is its older
 * sibling byte for byte.  (Additions to ABI version 7: look the symbols up.)
 * bpg_r1cs_template_repeat_inputs: bpg_r1cs_template_repeat for a template uploaded with bpg_r1cs_upload_template_inputs.  Sizes as for the repeat, plus
 * n_inputs' = count n_inputs, item-major.  With n_slots derived slots in the source (one per distinct (input, coefficient) pair of its rows) the coefficient
 * table becomes [shared | count n_params parameter slots | count n_slots derived slots]: item k's derived slot s sits at param_first + count n_params +
 * k n_slots + s, and item k's copies of the rows name item k's slots.  The result starts without a witness, its derived slots stand as the source's, and it
 * owns copies of everything it needs, the source's (input, coefficient index) list included.  Refused as bpg_r1cs_template_repeat refuses, and besides:
 * shared + count (n_params + n_slots) >= 2^30 coefficient indices, count n_inputs >= 2^29 - before any device work, named in bpg_last_error.
 * bpg_r1cs_template_join_inputs: bpg_r1cs_template_join where any part may have inputs, over the same frozen bpg_template_part.  Inputs are ordered part-major,
 * then item-major - the order of values, parameters and checkpoints.  The table is [shared of each part | parameter slots as in the join | derived slots,
 * part-major, item-major]; a part without inputs contributes nothing to either new range; the same template may be named by several parts.
 * bpg_r1cs_assign_inputs on such a repeat or join takes the n_inputs' values in that order, with its usual semantics (canonical values for byte identity; a
 * refused or mismatching call leaves no witness; the equal-scalar sets are dropped).  ONE launch (k_input_slots_join, a lane per (part, item, slot)) writes
 * coef[shared_p + ci] x_(p, k, input) into every derived slot before anything reads a constant term, and the levels hand every item its own inputs: as many
 * launches as the repeat or join has without inputs.  bpg_r1cs_assign and bpg_r1cs_assign_checkpointed refuse it as they refuse a single template with inputs.
 * bpg_r1cs_prove_resident, bpg_r1cs_verify_resident, bpg_r1cs_verify_batch (as one item), bpg_r1cs_check and bpg_r1cs_free serve it as any template;
 * bpg_r1cs_prove_template_batch_inputs proves its items one at a time, as for every repeat; it is no source of a further repeat or join.
 * bpg_r1cs_set_inputs: the VERIFIER's half of bpg_r1cs_assign_inputs, on any template with inputs (single, repeat or join).  It uploads and reduces the
 * n_inputs values and fills the derived slots - one small launch - and does nothing else.  The circuit is left WITHOUT a witness: bpg_r1cs_prove_resident and
 * bpg_r1cs_check then return BPG_ERR_MISSING_ASSIGNMENT, bpg_r1cs_verify_resident checks against these inputs.  The derived slots are sticky state of the
 * circuit: they stand as the last bpg_r1cs_assign_inputs or bpg_r1cs_set_inputs left them.  Refused with BPG_ERR_INVALID_ARGUMENT before any device work: a
 * wrong n_inputs, NULL input_values, a circuit without inputs, a handle without device state.  A verifying service uploads the shape once - from an instance
 * without a witness, which bpg_r1cs_upload_template_inputs accepts - repeats it, and checks the one proof of K statements after this one call. */
bpg_status bpg_r1cs_template_repeat_inputs(bpg_ctx *ctx, bpg_circuit *tmpl, uint64_t count, bpg_circuit **out);
bpg_status bpg_r1cs_template_join_inputs(bpg_ctx *ctx, uint64_t n_parts, const bpg_template_part *parts, bpg_circuit **out);
bpg_status bpg_r1cs_set_inputs(bpg_ctx *ctx, bpg_circuit *c, uint64_t n_inputs, const uint8_t *input_values /* n_inputs x 32 */);
/* TEST HOOKS, no device needed: the four repeat and join hooks above for programs with public inputs (n_inputs per template; input_values: the n_inputs' values
 * in the order bpg_r1cs_assign_inputs takes them; hints and checkpoints may be NULL).  The instance hooks give the rows as an assign of param_values (NULL: the
 * constants of the templates' rows) and input_values leaves them: row-major, every input term a constant term on its derived slot, the slot filled by the lane
 * function of k_input_slots_join compiled for the host.  coef: *ncoef_out = shared + n_params' + n_slots' scalars.  Every size is known before a row is made: a
 * buffer that is one entry short is refused, named, and nothing is written.  The eval hooks are the repeat- and join-layout interpreters compiled for the host
 * from poisoned vectors: levels in order, within a level parts, segments and items in REVERSE order, then the comparison step (*first_mismatch: the lowest
 * mismatching flat checkpoint index, UINT64_MAX: none).  A join part for them is a new struct: bpg_test_join_part is frozen. */
typedef struct { const bpg_r1cs_instance *inst; const bpg_witness_program *program; const bpg_witness_hints *hints; const bpg_witness_checkpoints *checkpoints;
                 uint64_t count; uint64_t n_inputs; } bpg_test_join_inputs_part;
bpg_status bpg_test_template_repeat_inputs_instance(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints, uint64_t n_inputs,
                                                    uint64_t count, const uint8_t *param_values, const uint8_t *input_values, uint64_t *row_ptr, uint64_t row_cap,
                                                    uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef, uint64_t coef_cap, uint64_t *nnz_out,
                                                    uint64_t *ncoef_out);
bpg_status bpg_test_template_eval_repeat_inputs(const bpg_r1cs_instance *inst, const bpg_witness_program *program, const bpg_witness_hints *hints,
                                                const bpg_witness_checkpoints *checkpoints, uint64_t n_inputs, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                const uint8_t *input_values, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out, uint64_t *first_mismatch);
bpg_status bpg_test_template_join_inputs_instance(uint64_t n_parts, const bpg_test_join_inputs_part *parts, const uint8_t *param_values, const uint8_t *input_values,
                                                  uint64_t *row_ptr, uint64_t row_cap, uint32_t *term_var, uint32_t *term_coef, uint64_t term_cap, uint8_t *coef,
                                                  uint64_t coef_cap, uint64_t *nnz_out, uint64_t *ncoef_out);
bpg_status bpg_test_template_eval_join_inputs(uint64_t n_parts, const bpg_test_join_inputs_part *parts, const uint8_t *v, const uint8_t *ck_values,
                                              const uint8_t *input_values, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out, uint64_t *first_mismatch);

/* R1CS CHECK ON THE DEVICE: is the resident witness satisfying, and if not, where does it fail.  (An addition to ABI version 7: look the symbol up.)
 * The witness of a template never visits the host (bpg_r1cs_assign, bpg_r1cs_template_repeat), and a proof of an unsatisfying witness is made all the same - the
 * host learns from the verifier that it is worthless, never which item or constraint was wrong.  bpg_r1cs_check evaluates, on the device, every multiplier
 * (a_L[i] * a_R[i] against a_O[i]) and every constraint row (its linear combination over a_L, a_R, a_O, the committed values and the constant One, mod l) of a
 * resident circuit.  Row j is the j-th constrain() call, as in bpg_r1cs_instance; on a repeat, row k q + j is constraint j of copy k.
 * v: the m committed values (32 bytes each, reduced mod l as bpg_r1cs_assign reduces them).  A plain upload does not keep them: the caller passes them.  A
 * template or a repeat may pass NULL: the values and the parameter slots stand as the last bpg_r1cs_assign left them (a template uploaded WITH a witness and
 * never assigned has no values: pass v).  m = 0: v is not looked at.
 * rows_out receives the lowest min(cap, bad_rows) violated row indices in ascending order, *n_rows_out how many - the same list whatever the launch order; the
 * frozen struct bpg_check_report the exact counts.  A satisfying witness: BPG_OK, zero counts.  An unsatisfying one is NOT an error: BPG_OK, counts above 0.
 * Refused before any device work: a NULL ctx, c, n_rows_out or report, a NULL rows_out with cap > 0, an m that does not match the circuit's, a NULL v where the
 * circuit keeps no values, a handle without device state (BPG_ERR_INVALID_ARGUMENT); a circuit without a witness - a verifier's upload, a template before its
 * first bpg_r1cs_assign or after a template batch (BPG_ERR_MISSING_ASSIGNMENT).
 * The first check of a circuit derives a row-major view of its matrix on the device (8 bytes per term and 8 per row, kept until bpg_r1cs_free; no part of the
 * table budget); no other call builds it.  The call changes nothing a later bpg_r1cs_prove_resident or bpg_r1cs_verify_resident sees: same proof bytes.  A host
 * may call it before it proves.  Variable-time, like every witness computation here (see SIDE CHANNELS above). */
typedef struct {                      /* frozen, like bpg_timings */
    uint64_t bad_multipliers;         /* i in [0,n) with a_L[i]*a_R[i] != a_O[i] */
    uint64_t first_bad_multiplier;    /* UINT64_MAX when none */
    uint64_t bad_rows;                /* constraints j in [0,q) whose linear combination is not 0 */
    uint64_t first_bad_row;           /* UINT64_MAX when none */
} bpg_check_report;
bpg_status bpg_r1cs_check(bpg_ctx *ctx, bpg_circuit *c, uint64_t m, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out, bpg_check_report *report);
/* TEST HOOK, no device and no context needed: the same definition in host C++ (csrc/host/check.hpp) on an instance WITH its witness.  Refused with
 * BPG_ERR_INVALID_ARGUMENT: NULL inst, n_rows_out or report, a malformed instance, a NULL v with m > 0, a NULL rows_out with cap > 0; an instance without a_L,
 * a_R, a_O (n > 0): BPG_ERR_MISSING_ASSIGNMENT. */
bpg_status bpg_test_check_host(const bpg_r1cs_instance *inst, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out, bpg_check_report *report);

/* measurement hooks (bench.py): HIP events on the engine's own stream. mode 0 off, 1 = dominant kernel only, 2 = all kernels;
 * report = JSON text {kernel: {count, total_ms, alg_bytes, device_bytes, field_mults}} accumulated since the last set. */
bpg_status bpg_profile_set(bpg_ctx *ctx, int32_t mode);
bpg_status bpg_profile_report(bpg_ctx *ctx, char *out, uint64_t cap);
bpg_status bpg_bench_fe_mul(bpg_ctx *ctx, uint32_t iters, double *mults_per_second);

/* test hook: device field arithmetic on n pairs of raw 256-bit values; op 0 mul, 1 sq, 2 add, 3 sub, 4 invert, 5 mixed chain; canonical output;
 * op 6: the scalar-field Montgomery product a b / 2^256 mod l of the device (one operand below l), eight raw words out;
 * op 7 a + b, 8 a - b, 9 -a mod l (operands below l) and 10 a / 2^256 mod l: the device code of the other scalar operations, eight raw words out */
bpg_status bpg_test_fe_ops(bpg_ctx *ctx, int32_t op, uint64_t n, const uint8_t *a, const uint8_t *b, uint8_t *out);
/* test hook: the next blinding stream started on ctx (bpg_blinding_begin) records a failed upload of its first block, as a failing hipMemcpyAsync
 * would: the prove that adopts it must fail with BPG_ERR_DEVICE instead of reading a stale device slab */
bpg_status bpg_test_fail_next_upload(bpg_ctx *ctx);
/* test hook: the copies of the next blinding stream started on ctx are skipped WITHOUT an error (a dropped DMA): the device slab keeps the pattern its
 * blocks were marked with when the slab changed owner, the conversion kernel notices, and the prove that adopts the stream fails with BPG_ERR_DEVICE */
bpg_status bpg_test_drop_next_upload(bpg_ctx *ctx);
/* test hook: what the whole process holds from the HIP runtime at this moment, every context and device together - out = device buffers, their bytes, pinned
 * buffers, their bytes, streams, events.  No context and no device work: six counters are read.  All zero once every context, circuit and tree is freed. */
bpg_status bpg_test_live_resources(uint64_t out[6]);
/* diagnostics: bytes of precomputed generator multiples (fold tables + wide tail tables) this process holds on the context's device */
uint64_t bpg_table_bytes(bpg_ctx *ctx);
/* diagnostics: 1 when the last bpg_r1cs_prove* / bpg_prover_prove on ctx took the kernel variants for a shared device (another prove() was in flight on the
 * device when it was entered; decided once per proof), else 0 - replay a failing proof with BPG_FOLD_ADAPT=2 (always) or 0 (never) */
int32_t bpg_ctx_last_shared_variants(bpg_ctx *ctx);
/* test hook: compress(sum s_i*G[first+i] + t_i*H[first+i]) through the bucket-method MSM kernels */
bpg_status bpg_msm_gens(bpg_ctx *ctx, uint64_t first, uint64_t count, const uint8_t *s, const uint8_t *t, uint8_t out[32]);
/* test hook: the bucket-method MSM on any plan the prove path builds.  A segment (frozen struct) is `len` terms on generator table `table`
 * (0 = G, 1 = H) from generator `first`; lgblk 31 = contiguous, else element e is point first + ((e >> lgblk) << (lgblk+1)) | (e & (2^lgblk - 1));
 * skip = NULL or (len + 31) / 32 words, bit e set = element e takes no part.  Segments are grouped by ascending result (< nmsm <= 4), at most 16 of
 * them; `scalars` holds the canonical 32-byte scalars of all segments in order.  out = nmsm compressed results.  evidence = JSON text of the plan
 * the call took (W, off[], nb, fb, CB, lgTile, tmax, CH, nchunks, shared-device variants, combine and window-sum variants), the thresholds the
 * sort and the combine compare against, and the device state it left: starts[0..nkeys] of every bucket, the heavy and medium list counts.
 * Every argument is checked before a launch (BPG_ERR_INVALID_ARGUMENT); a NULL ctx is BPG_ERR_DEVICE, as on a machine without a GPU. */
typedef struct {
    uint32_t table, result;
    uint64_t first;
    uint32_t len, lgblk;
    const uint32_t *skip;
} bpg_msm_seg;
bpg_status bpg_test_msm(bpg_ctx *ctx, uint32_t nmsm, uint32_t nseg, const bpg_msm_seg *segs, const uint8_t *scalars, uint8_t *out,
                        char *evidence, uint64_t cap);

/* test hook: the generator fold of one group of rounds of the inner-product argument, on scalars the caller chooses, through the launch path of the prover
 * (kernel choice, recoding, upload, launch, normalisation).  The group-start tables are the context's own generator tables, G from generator 0 and H from
 * generator 0, g_M = 2^(lgMr + rounds) <= capacity points each; Mr = 2^lgMr, nterms = 2^rounds - 1 with rounds 1..5.  sG, sH: nterms canonical 32-byte
 * scalars each - the scalars of terms 1..nterms themselves, not challenges: out[i] = G[i] + sum_t sG_t G[i + t*Mr], out[Mr + i] the same on H with sH.  first = 1:
 * the lanes with i + t*Mr >= n take s_t * u_ch (the padding generators of a first group), and g_M/2 < n <= g_M; first = 0: n and u_ch are not used.
 * kernel: -1 = what the chooser picks under the context's knobs; 0..6 force k_fold_points_wnaf, _quadw, _quad, _split, _regw, _reg, k_fold_points - accepted
 * exactly where the chooser could name that kernel under some setting of the knobs (quadw: first = 0, Mr % 64 == 0, nterms <= 7; regw: first = 0,
 * Mr % 256 == 0, nterms <= 7; quad: nterms <= 7; split: 3..15 terms; reg: 1, 3, 7 or 15 terms; wnaf: BPG_FOLD_WNAF >= 3 and a table of odd multiples fits).
 * out = 2 * Mr compressed points, G side then H side, normalised as the prover normalises them.  evidence (cap >= 512) = JSON text: the kernel's name, Mr,
 * nterms, first, n; top (the length of the doubling chain less one) for the bitmap and width-w kernels; nsteps[2], tail[2] for the step kernels; wnaf, parts,
 * part_bits as settled for k_fold_points_wnaf.  Every argument is checked before a launch (BPG_ERR_INVALID_ARGUMENT: a NULL pointer, a non-canonical scalar,
 * rounds outside 1..5, g_M beyond the capacity, n out of range, a forced kernel outside its conditions); a NULL ctx is BPG_ERR_DEVICE.
 * (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_test_fold(bpg_ctx *ctx, int32_t kernel, uint32_t lgMr, uint32_t rounds, uint32_t first, uint64_t n, const uint8_t *sG, const uint8_t *sH,
                         const uint8_t u_ch[32], uint8_t *out, char *evidence, uint64_t cap);

/* test hook: the table-driven tail of the inner-product argument (k_tt_bases, k_tt_multiples, k_tt_factors, k_tt_advance, k_tt_round or k_tt_round8, k_tt_finish)
 * on scalars the caller chooses, through the freeze and per-round steps of the prover, on the context's own generators G[0, M0), H[0, M0) (M0 = 2^lgM0, 2 .. 2^14,
 * at most the capacity) and the Pedersen base B.  tables: 0 = the context's 4-bit window tables of the original generators (they stay with the context, as after
 * a proof of M0 multipliers), 1 = 4-bit tables built in the arena, as for folded generators, 2 = the 8-bit tables of the original generators - refused where the
 * prover would fall back to the 4-bit ones (M0 < 64, or the table budget: BPG_TT_WIDE_GB), so that no case passes on other tables than it names.  a, b: M0
 * canonical scalars each.  The virtual generators start as G0[p] = gamma0 * fG[p] * G_p, H0[p] = eta0 * yinv^p * fG[p] * H_p with fG[p] = u_ch where first = 1
 * and p >= n (then M0/2 < n <= M0; first = 0: n and u_ch are not used), else 1.  Sub-round j (h = M0 >> (j+1)) gives
 *     L_j = sum_{i<h} a[i] Gj[h+i] + b[h+i] Hj[i] + <a_lo, b_hi> w B,   R_j = sum_{i<h} a[h+i] Gj[i] + b[i] Hj[h+i] + <a_hi, b_lo> w B
 * and then folds with u = u[j]: a'[i] = a[i] u + a[h+i] / u, b'[i] = b[i] / u + b[h+i] u, G'[i] = G[i] / u + u G[h+i], H'[i] = u H[i] + H[h+i] / u.
 * rounds: 1 .. lgM0 sub-rounds.  lr_out = 2 * rounds encodings L_0, R_0, L_1, ..; ab_out = the folded a, then the folded b, after the last challenge
 * (M0 >> rounds canonical scalars each).  evidence (cap >= 512) = JSON text: kernel (k_tt_round or k_tt_round8), tables, M0, nblk (blocks per sum of the round
 * kernel: k_tt_finish adds its B windows to a partial from 256 on, else takes them as they are), quad (the block-sum layout: 1 for a proof alone).  Every
 * argument is checked before a launch (BPG_ERR_INVALID_ARGUMENT: a NULL pointer, a non-canonical scalar, yinv = 0, a challenge of 0, lgM0, tables, first, n or
 * rounds out of range); a NULL ctx is BPG_ERR_DEVICE.  (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_test_tail(bpg_ctx *ctx, uint32_t lgM0, uint32_t tables, uint32_t first, uint64_t n, const uint8_t *a, const uint8_t *b, const uint8_t yinv[32],
                         const uint8_t u_ch[32], const uint8_t gamma0[32], const uint8_t eta0[32], const uint8_t w[32], uint32_t rounds, const uint8_t *u,
                         uint8_t *lr_out, uint8_t *ab_out, char *evidence, uint64_t cap);
/* test hook: A_I = <aL, G> + <aR, H> + blind[0] B_blinding, A_O = <aO, G> + blind[1] B_blinding, S = <sL, G> + <sR, H> + blind[2] B_blinding from the context's
 * window tables of the original generators G[0, M0), H[0, M0) (k_tt_commit3, k_tt_commit3_finish, as a proof of at most 2^14 multipliers computes them):
 * M0 = 2^lgM0 (1 .. 2^14, at most the capacity), n = 1 .. M0 canonical scalars per vector, blind = three canonical scalars.  out = the three encodings;
 * evidence (cap >= 512) = JSON text: M0, n, nblk (blocks per sum: the finish kernel adds its blinding windows to a partial from 256 on), quad.  Arguments are
 * checked before a launch (BPG_ERR_INVALID_ARGUMENT); a NULL ctx is BPG_ERR_DEVICE.  (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_test_commit3(bpg_ctx *ctx, uint32_t lgM0, uint64_t n, const uint8_t *aL, const uint8_t *aR, const uint8_t *aO, const uint8_t *sL, const uint8_t *sR,
                            const uint8_t blind[96], uint8_t out[96], char *evidence, uint64_t cap);
/* test hook: the verifier's flattened weights of a resident circuit (any handle with device state: a plain upload, a template, a repeat, a join) at a z the
 * caller chooses - the powers of z (k_exp_table), k_flatten over the variable columns and the k_flatten_const / k_reduce_partials reduction over the constant
 * column, through the one function bpg_r1cs_verify_resident calls for them.  out = 3 n + m + 1 canonical scalars of 32 bytes: w_L (n) | w_R (n) | w_O (n) |
 * w_V (m) | w_c, where row j weighs z^(j+1) and committed and constant terms change side (w_V and w_c come out negated).  The witness, if any, is not read.
 * Checked before a launch (BPG_ERR_INVALID_ARGUMENT: a NULL pointer, a non-canonical z, a handle without device state or of another device); a NULL ctx is
 * BPG_ERR_DEVICE and writes nothing.  (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_test_weights(bpg_ctx *ctx, bpg_circuit *circuit, const uint8_t z[32], uint8_t *out);
/* test hook: the device side of bpg_r1cs_verify_resident_batch from k_vw_exp to k_vw_reduce, through the function the call runs, on challenge records the
 * caller chooses.  challenges = count records of 7 + 2 lg N canonical scalars of 32 bytes: y^-1, z, x, u (the factor of the padding generators), a, b, rho,
 * then u_1 .. u_lgN, then their inverses (N = n padded to a power of two).  param_values / input_values: NULL (the standing slots) or one set per item
 * (count x n_params x 32, count x n_inputs x 32), on a single template.  g_out, h_out = the two accumulators, N canonical scalars each: sum_k rho_k g_k,i
 * and sum_k rho_k h_k,i with the padding lanes times u; small_out = count slots [w_V (m) | w_c | delta].  evidence (cap >= 1024) = JSON text of the plan
 * the call took: n, N, count, n_tail, item_bytes, waves, items_per_wave, chunks, items_per_chunk, the last wave's figures, target_blocks, wave_bytes and
 * launches per kernel.  Refused before a launch (BPG_ERR_INVALID_ARGUMENT): a NULL pointer, count = 0 or above 2^20, a circuit without multipliers or of
 * another context, a non-canonical entry, y^-1 = 0 or a u_k = 0, a u_k^-1 that is not the inverse of u_k, constants the circuit cannot take; a NULL ctx
 * is BPG_ERR_DEVICE and writes nothing.  (An addition to ABI version 7: look the symbol up.) */
bpg_status bpg_test_verify_wave_scalars(bpg_ctx *ctx, bpg_circuit *circuit, uint64_t count, const uint8_t *challenges, const uint8_t *param_values,
                                        const uint8_t *input_values, uint8_t *g_out, uint8_t *h_out, uint8_t *small_out, char *evidence, uint64_t cap);

/* test hook: k_decompress, the verifier's RFC 9496 decoder, on n encodings of 32 bytes, launched as bpg_r1cs_verify launches it.  ok_out[i] = 1 when
 * encoding i is accepted; xy_out holds, for EVERY entry, the affine x || y (32 + 32 bytes, canonical) the kernel wrote, recovered on the host from
 * its halved Niels form (x = ypx - ymx, y = ypx + ymx) - meaningful where ok_out[i] = 1.  Arguments are checked before any launch
 * (BPG_ERR_INVALID_ARGUMENT: a NULL pointer with n > 0, n above 2^24); a NULL ctx is BPG_ERR_DEVICE; n = 0 returns BPG_OK.  (An addition to ABI version 7.) */
bpg_status bpg_test_decompress(bpg_ctx *ctx, uint64_t n, const uint8_t *in, uint32_t *ok_out, uint8_t *xy_out);
/* test hook, no device needed: the host half of bpg_r1cs_verify alone - R1CSProof::from_bytes and the Fiat-Shamir replay - for a circuit of n multipliers
 * and m commitments on a context of gens_capacity generators.  *decided_out = 1 and *status_out = BPG_ERR_FORMAT, BPG_ERR_INVALID_GENERATORS_LENGTH or
 * BPG_ERR_VERIFICATION when the replay refuses the proof itself (length, lead byte, non-canonical scalar, capacity, an identity encoding where upstream
 * validates one); *decided_out = 0 and *status_out = BPG_OK when the decision is left to the device (decompression and the one MSM).  transcript_state is
 * not written.  (An addition to ABI version 7.) */
bpg_status bpg_test_verify_replay(uint64_t n, uint64_t m, uint64_t gens_capacity, const uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES],
                                  const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags, bpg_status *status_out, int32_t *decided_out);

/* test hooks: proofs under a SCRIPTED transcript.  Each call runs exactly what its production sibling runs - bpg_r1cs_prove_resident, bpg_r1cs_prove_batch (the
 * lockstep path only), bpg_r1cs_verify_resident, bpg_r1cs_verify_batch - on a transcript that absorbs and squeezes as always, so that its 203-byte state evolves
 * as in the sibling, but whose challenge_scalar RETURNS the next entry of `script` instead of the squeezed value.  script = 5 + lg N canonical scalars of 32
 * bytes in the order y, z, u, x, w, u_1 .. u_lgN (N = n padded to a power of two); the batch calls take one script per item (scripts[k], script_lens[k]), and
 * the weights of bpg_test_verify_batch_scripted stay the real ones.  Outputs are the sibling's: proof bytes, the transcript state after, the status.
 * THE RESULT OF A SCRIPTED CALL IS NOT A SOUND PROOF, and an accepted scripted verification says nothing about a statement: whoever chooses the challenges
 * can forge.  The script lives in the call's own transcript object and never crosses the ABI: no production entry point can end up with one.
 * Refused before any launch (BPG_ERR_INVALID_ARGUMENT; a batch call as a whole): a NULL script, script_len != 5 + lg N, a non-canonical entry, y = 0 or a
 * u_k = 0 (both are inverted; z, u, x, w may be 0); in bpg_test_prove_batch_scripted also an item that bpg_r1cs_prove_batch would prove on the single path.
 * bpg_test_verify_replay_scripted needs no device: bpg_test_verify_replay on a scripted transcript (script NULL: on a plain one), which also writes the state
 * after into transcript_state, the challenges the replay drew into challenges_out ((5 + lg N) x 32 bytes, zero where it did not get) and the number of script
 * entries it took into *consumed_out.  (Additions to ABI version 7: look the symbols up.) */
bpg_status bpg_test_prove_scripted(bpg_ctx *ctx, bpg_circuit *circuit, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *v_blinding,
                                   const uint8_t rng_seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len, uint8_t *proof_out, uint64_t *proof_len);
bpg_status bpg_test_prove_batch_scripted(bpg_ctx *ctx, uint64_t count, const bpg_batch_item *items, const uint8_t *const *scripts, const uint64_t *script_lens,
                                         bpg_status *status_out);
bpg_status bpg_test_verify_scripted(bpg_ctx *ctx, bpg_circuit *circuit, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES], uint64_t m, const uint8_t *V,
                                    const uint8_t *proof, uint64_t proof_len, const uint8_t seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len);
bpg_status bpg_test_verify_batch_scripted(bpg_ctx *ctx, uint64_t count, const bpg_verify_item *items, const uint8_t *const *scripts, const uint64_t *script_lens,
                                          const uint8_t batch_seed[32], bpg_status *status_out);
bpg_status bpg_test_verify_replay_scripted(uint64_t n, uint64_t m, uint64_t gens_capacity, uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES], const uint8_t *proof,
                                           uint64_t proof_len, const uint8_t seed[32], uint32_t flags, const uint8_t *script, uint64_t script_len,
                                           bpg_status *status_out, uint8_t *challenges_out, uint64_t *consumed_out);

/* ---------------------------------------------------------------------------------------------------- PART 2: host mirror
 * merlin::Transcript, bulletproofs::r1cs::{Prover, Verifier}, and the reference's Gadget trait with BoundsCheck,
 * MimcHash256 and MerkleTree256 (reference src/gadget.rs:6-59 and the gadget modules), implemented in C++. */
typedef struct bpg_transcript bpg_transcript;
typedef struct bpg_prover bpg_prover;
typedef struct bpg_verifier bpg_verifier;
typedef struct bpg_gadget bpg_gadget;
typedef struct { uint32_t var; uint8_t coeff[32]; } bpg_term;       /* (Variable, Scalar); var = kind << 29 | index */
typedef struct { const bpg_term *terms; uint64_t n; } bpg_lc;        /* bulletproofs::r1cs::LinearCombination */

bpg_status bpg_transcript_new(const uint8_t *label, uint64_t len, bpg_transcript **out);        /* Transcript::new */
void bpg_transcript_free(bpg_transcript *t);
bpg_status bpg_transcript_append_message(bpg_transcript *t, const char *label, const uint8_t *msg, uint64_t len);
bpg_status bpg_transcript_challenge_bytes(bpg_transcript *t, const char *label, uint8_t *out, uint64_t len);
bpg_status bpg_transcript_state(const bpg_transcript *t, uint8_t out[BPG_TRANSCRIPT_STATE_BYTES]);

bpg_status bpg_prover_new(bpg_ctx *ctx, bpg_transcript *t, bpg_prover **out);                   /* Prover::new */
void bpg_prover_free(bpg_prover *p);
/* test hook: from now on the commitments of p are 32 hash bytes of (value, blinding) made on the host - NOT group elements - so that a device-less
 * prover (bpg_prover_new with ctx = NULL) can run a file driver's parsing and gadget assembly under sanitizers / a fuzzer; bpg_prover_prove stays
 * refused (BPG_ERR_DEVICE).  Refused with BPG_ERR_INVALID_ARGUMENT on a prover that HAS a device context: such a prover never hands out anything
 * but Pedersen commitments */
bpg_status bpg_test_prover_stub_commitments(bpg_prover *p);
bpg_status bpg_prover_commit(bpg_prover *p, const uint8_t v[32], const uint8_t blind[32], uint8_t com_out[32], uint32_t *var_out);
bpg_status bpg_prover_commit_many(bpg_prover *p, uint64_t k, const uint8_t *v, const uint8_t *blind, uint8_t *coms_out, uint32_t *vars_out);
/* Prover::commit for a host that computes its Pedersen commitments elsewhere (its own PedersenGens, or a prover created without a device
 * context): registers (v, blind) as the next committed variable and appends the given 32-byte commitment to the transcript as "V". */
bpg_status bpg_prover_commit_precomputed(bpg_prover *p, const uint8_t v[32], const uint8_t blind[32], const uint8_t com[32], uint32_t *var_out);
/* Extension - every commitment of a prover in ONE kernel launch (the reference commits one value at a time, src/gadget.rs:27-35,
 * src/lalrpop/assignment_parser.rs:152-169; a 512-leaf tree makes a thousand of them).  While deferral is on, the commit calls above and
 * Gadget::setup register their variables and return ALL-ZERO commitment bytes; the flush computes every pending commitment at once and
 * appends them to the transcript in the order they were made, which is the transcript the per-call path gives.  Prove, the start of the
 * blinding chain and the instance export flush first; a host that reads the transcript itself flushes before it does.  The commitment
 * of committed variable `index` (0-based, in commit order) can be read once it has been flushed. */
bpg_status bpg_prover_defer_commitments(bpg_prover *p, int32_t on);     /* turning it off flushes */
bpg_status bpg_prover_flush_commitments(bpg_prover *p);
bpg_status bpg_prover_commitment(bpg_prover *p, uint64_t index, uint8_t out[32]);
uint64_t bpg_prover_num_constraints(const bpg_prover *p);                                       /* fork getter, prover.rs:89 */
uint64_t bpg_prover_num_multiplications(const bpg_prover *p);                                   /* fork getter, prover.rs:92 */
uint64_t bpg_prover_num_committed(const bpg_prover *p);
/* ConstraintSystem methods (trait visible at reference src/cs_buffer.rs:89-113) */
bpg_status bpg_prover_multiply(bpg_prover *p, const bpg_lc *left, const bpg_lc *right, uint32_t vars_out[3]);
bpg_status bpg_prover_allocate_multiplier(bpg_prover *p, int32_t has_assignment, const uint8_t l[32], const uint8_t r[32], uint32_t vars_out[3]);
bpg_status bpg_prover_allocate(bpg_prover *p, int32_t has_assignment, const uint8_t s[32], uint32_t *var_out);
bpg_status bpg_prover_constrain(bpg_prover *p, const bpg_lc *lc);
/* borrowed view of the assembled instance (valid until the prover is next mutated or freed) */
bpg_status bpg_prover_instance(bpg_prover *p, bpg_r1cs_instance *out, const uint8_t **v_out, const uint8_t **v_blinding_out);
/* Circuit templates (PART 1, bpg_r1cs_upload_template) for hosts of this mirror.  The prover records, for every multiplier, how it was made - always, at
 * the cost of eight bytes per multiplier; nothing else it exports changes.  bpg_prover_witness_program: borrowed view of the program (valid until the
 * prover is next mutated or freed; term_coef indexes the coefficient table of bpg_prover_instance); BPG_ERR_INVALID_ARGUMENT when the circuit has a free
 * multiplier (allocate / allocate_multiplier) or no multiplier at all.  bpg_prover_mark_param_row: the constant term of constraint `row` is assigned per
 * witness; the row a bpg_prover_constrain call made is bpg_prover_num_constraints(p) - 1 right after it (a gadget's closing constraint likewise). */
bpg_status bpg_prover_witness_program(bpg_prover *p, bpg_witness_program *out);
/* The same with hints: succeeds when every multiplier came from multiply() or from a range proof (bpg_range_proof_prove, BoundsCheck, LessThan,
 * bpg_prover_allocate_bit), else the "free multiplier" refusal above.  Both views are borrowed under the same rule and replace those of an earlier export
 * call on this prover; export the instance (bpg_prover_instance) AFTER the last bpg_prover_allocate_bit.  bpg_prover_witness_program itself still refuses a
 * circuit with a hinted multiplier.
 * bpg_prover_allocate_bit: ConstraintSystem::allocate_bit for hosts that drive the mirror directly - the multiplier range_proof makes for bit `bit` (0..255)
 * of `source`, whose assigned value is source_value (raw little-endian bytes, as range_proof reads them): a_L = 1 - b, a_R = b.  It adds no constraint. */
bpg_status bpg_prover_witness_program_hinted(bpg_prover *p, bpg_witness_program *program_out, bpg_witness_hints *hints_out);
/* Public inputs ("Public inputs in circuit templates" above).  bpg_prover_input: a new input with this value (Scalar::from_bits semantics, kept reduced mod l),
 * *var_out = BPG_VAR_INPUT << 29 | p.  bpg_prover_template_instance: bpg_prover_instance with the input terms KEPT in the rows (kind 5), for
 * bpg_r1cs_upload_template_inputs; *n_inputs_out and *inputs_out (n_inputs x 32, input order) are this prover's inputs.  The pointers stay valid until the
 * prover is next mutated or freed.  Without inputs it exports what bpg_prover_instance exports. */
bpg_status bpg_prover_input(bpg_prover *p, const uint8_t value[32], uint32_t *var_out);
bpg_status bpg_prover_template_instance(bpg_prover *p, bpg_r1cs_instance *inst_out, const uint8_t **v_out, const uint8_t **v_blinding_out, uint64_t *n_inputs_out,
                                        const uint8_t **inputs_out);
/* Checkpoint candidates (bpg_witness_checkpoints).  A gadget that computes a value its caller may know anyway says so through ConstraintSystem::note_value;
 * MimcHash256 - and MerkleTree256 through it - notes the sponge state after every absorbed block, tag = the block index, bit 31 set on the sponge's last block
 * (its digest: a Merkle node).  A prover keeps the note when the value is exactly one multiplier variable; it costs no multiplier, constraint or transcript byte.
 * bpg_prover_noted: *n_out = how many notes there are; the first min(cap, *n_out) go to vars_out / tags_out, in the order they were made. */
bpg_status bpg_prover_noted(bpg_prover *p, uint32_t *vars_out, uint32_t *tags_out, uint64_t cap, uint64_t *n_out);
bpg_status bpg_prover_allocate_bit(bpg_prover *p, const bpg_lc *source, uint32_t bit, const uint8_t source_value[32], uint32_t vars_out[3]);
bpg_status bpg_prover_mark_param_row(bpg_prover *p, uint64_t row);
/* Extension (no upstream counterpart; the proof bytes do not change): start drawing the blinding scalars of the coming prove() now.
 * Upstream's Prover::prove builds its TranscriptRng from the transcript after the last commitment (+ the "m" suffix), the commitment
 * blindings and thread_rng() - not from the constraints - and then draws 2n + 3 scalars serially (0.30 s of a 0.34 s proof at n = 2^20).
 * Called once every commitment has been made, this starts that chain on a host thread while the caller keeps assembling constraints;
 * bpg_prover_prove / bpg_r1cs_prove(_resident) on the same context use the stream iff transcript state, blindings and rng_seed are still
 * the same and n <= max_multipliers, and silently draw afresh otherwise (another commitment, another seed, BPG_FLAG_EXPANDED_BLINDING).
 * Streams of one context are drawn in the order of the calls by the context's chain worker - ONE AT A TIME with its single default thread
 * (bpg_ctx_set_chain_workers adds threads); workers + 1 are alive at most (one more call retires the oldest), so a sequence of proofs can have the chain of proof i+1 drawn while the kernels of proof i
 * run: call bpg_blinding_begin for proof i+1, then prove proof i.  max_multipliers sizes a pinned host buffer of 128 bytes per multiplier.
 * A deterministic rng_seed is for tests and benchmarks; production callers pass 32 fresh random bytes per proof (upstream: thread_rng()). */
bpg_status bpg_prover_start_blinding(bpg_prover *p, const uint8_t rng_seed[32], uint64_t max_multipliers);
bpg_status bpg_blinding_begin(bpg_ctx *ctx, const uint8_t transcript_state[BPG_TRANSCRIPT_STATE_BYTES] /* after every "V" append */, uint64_t m,
                              const uint8_t *v_blinding /* m x 32 */, const uint8_t rng_seed[32], uint64_t max_multipliers);
/* Threads of the context's chain worker (default 1, or BPG_CHAIN_WORKERS): with `workers` threads that many queued blinding streams are drawn
 * side by side and workers + 1 may be alive, so a host that proves a SEQUENCE of independent proofs keeps bpg_blinding_begin `workers` proofs
 * ahead of the proof it is proving and the GPU, not one host core's Keccak chain, sets the pace.  Streams in flight are dropped by the call.
 * Each alive stream pins 128 bytes per multiplier of host memory. */
bpg_status bpg_ctx_set_chain_workers(bpg_ctx *ctx, uint32_t workers);
/* streams EACH chain thread draws in lockstep, 1..8 (default 1): with AVX-512 the sponges of up to eight queued streams sit in the 64-bit lanes of ZMM
 * registers and cost one core about what one costs it (EPYC 9575F: 193 ns per draw of all eight against 152 ns for one), so one thread keeps
 * up to eight chains going - a chain alone gets ~25 % slower, a core's chain throughput six times higher; workers * lanes + 1 streams may be alive.
 * Streams in flight are dropped by this call, like bpg_ctx_set_chain_workers. */
bpg_status bpg_ctx_set_chain_lanes(bpg_ctx *ctx, uint32_t lanes);
/* A chain pool: host threads that draw the blinding chains of EVERY context attached to it, thread k up to lanes[k] (1..8) of them in lockstep.  A
 * host that proves on several contexts of a GPU (proving streams) sizes ONE pool for its cores instead of a worker per context: e.g. 14 threads with
 * one lane (a chain alone takes 0.30 s at 2^20) and one thread with 6 lanes (0.38 s each) draw twenty chains at once on 15 cores.  An attached
 * context may have max_streams blinding streams alive (bpg_blinding_begin retires the oldest beyond that); bpg_ctx_set_chain_workers / _lanes detach.
 * The pool should outlive its contexts' use of it: detach (pool = NULL) or destroy the contexts first.  (bpg_chain_pool_destroy lets the pool finish
 * what is queued; a context that is still attached afterwards goes back to its own chain worker at its next bpg_blinding_begin.) */
typedef struct bpg_chain_pool bpg_chain_pool;
bpg_status bpg_chain_pool_create(uint32_t threads, const uint32_t *lanes /* threads entries, NULL = 1 each */, bpg_chain_pool **out);
void bpg_chain_pool_destroy(bpg_chain_pool *pool);
bpg_status bpg_ctx_attach_chain_pool(bpg_ctx *ctx, bpg_chain_pool *pool /* NULL = detach */, uint32_t max_streams);
int32_t bpg_chain_cpu(bpg_ctx *ctx);   /* diagnostics: host core the chain worker last ran on, -1 = no stream drawn yet */
bpg_status bpg_prover_prove(bpg_prover *p, uint64_t gens_capacity, const uint8_t rng_seed[32], uint32_t flags,
                            uint8_t *proof_out, uint64_t *proof_len, bpg_timings *timings);

bpg_status bpg_verifier_new(bpg_transcript *t, bpg_verifier **out);                             /* Verifier::new */
void bpg_verifier_free(bpg_verifier *v);
bpg_status bpg_verifier_commit(bpg_verifier *v, const uint8_t com[32], uint32_t *var_out);       /* Verifier::commit */
bpg_status bpg_verifier_input(bpg_verifier *v, const uint8_t value[32], uint32_t *var_out);      /* the verifier's side of bpg_prover_input */
/* Gated variables ("Gated variables" above): x of kind BPG_VAR_INPUT, var of kind 0..3, *var_out = BPG_VAR_GATED << 29 | position in the gate table */
bpg_status bpg_prover_gate(bpg_prover *p, uint32_t x, uint32_t var, uint32_t *var_out);
bpg_status bpg_verifier_gate(bpg_verifier *v, uint32_t x, uint32_t var, uint32_t *var_out);
bpg_status bpg_prover_gates(bpg_prover *p, bpg_witness_gates *out);
bpg_status bpg_merkle_path256_new(const bpg_lc *root, uint32_t leaf, const uint32_t *levels /* 4 x depth */, uint64_t depth, bpg_gadget **out);
uint64_t bpg_verifier_num_vars(const bpg_verifier *v);                                          /* fork getter, verifier.rs:89 */
bpg_status bpg_verifier_instance(bpg_verifier *v, bpg_r1cs_instance *out, const uint8_t **commitments_out);
/* Verifier::verify(&proof, &pc_gens, &bp_gens) on the GPU of ctx */
bpg_status bpg_verifier_verify(bpg_verifier *v, bpg_ctx *ctx, uint64_t gens_capacity, const uint8_t *proof, uint64_t proof_len,
                               const uint8_t seed[32], uint32_t flags);

bpg_status bpg_bounds_check_new(const uint8_t *min_be, uint64_t min_len, const uint8_t *max_be, uint64_t max_len, bpg_gadget **out);
bpg_status bpg_mimc_hash256_new(const bpg_lc *image, bpg_gadget **out);
/* pattern: the tree syntax of the .gadgets grammar with W / I leaves, e.g. "((W I) (I W))"; at most 64 levels of nesting (BPG_ERR_INVALID_ARGUMENT beyond) */
bpg_status bpg_merkle_tree256_new(const bpg_lc *root, const bpg_lc *instance_vars, uint64_t n_inst, const bpg_lc *witness_vars,
                                  uint64_t n_wit, const char *pattern, bpg_gadget **out);
/* the remaining gadgets of the reference; assignment pointers may be NULL on the verifier side */
bpg_status bpg_equality_new(const bpg_lc *right_hand, uint64_t n, bpg_gadget **out);
bpg_status bpg_inequality_new(const bpg_lc *right_hand, uint64_t n, const uint8_t *right_assignment /* n x 32 or NULL */, bpg_gadget **out);
bpg_status bpg_less_than_new(const bpg_lc *left, const uint8_t *left_assignment, const bpg_lc *right, const uint8_t *right_assignment, bpg_gadget **out);
bpg_status bpg_set_membership_new(const bpg_lc *value, const uint8_t *value_assignment, const bpg_lc *instance_vars, uint64_t n_inst,
                                  const uint8_t *instance_assignments /* n_inst x 32 or NULL */, bpg_gadget **out);
void bpg_gadget_free(bpg_gadget *g);
/* Gadget::setup: derived = preprocess(witnesses); one commitment each. *n_derived: in = capacity, out = count */
bpg_status bpg_gadget_setup(bpg_gadget *g, bpg_prover *p, const uint8_t *witness_scalars, uint64_t n_wit, const uint8_t *blindings,
                            uint64_t n_blind, uint8_t *coms_out, uint8_t *derived_scalars_out, uint32_t *derived_vars_out, uint64_t *n_derived);
/* Gadget::preprocess alone: the derived scalars a host commits itself (bpg_prover_commit / bpg_prover_commit_precomputed), in order */
bpg_status bpg_gadget_preprocess(bpg_gadget *g, const uint8_t *witness_scalars, uint64_t n_wit, uint8_t *derived_scalars_out, uint64_t *n_derived);
bpg_status bpg_gadget_prove(bpg_gadget *g, bpg_prover *p, const uint32_t *vars, uint64_t n_vars, const uint8_t *derived_scalars,
                            const uint32_t *derived_vars, uint64_t n_derived);
bpg_status bpg_gadget_verify(bpg_gadget *g, bpg_verifier *v, const uint32_t *vars, uint64_t n_vars, const uint32_t *derived_vars, uint64_t n_derived);
/* OR blocks (reference src/cs_buffer.rs, src/or/or_conjunction.rs): a recording constraint system whose multiplier numbering
 * starts at the parent's current multiplier count; rewind() closes a clause; bpg_or_* replays the clauses into the parent. */
typedef struct bpg_buffer bpg_buffer;
bpg_status bpg_buffer_new(uint64_t first_multiplier, int32_t prover_side, bpg_buffer **out);
void bpg_buffer_free(bpg_buffer *b);
bpg_status bpg_buffer_rewind(bpg_buffer *b);
uint64_t bpg_buffer_next_multiplier(const bpg_buffer *b);
bpg_status bpg_gadget_prove_buffered(bpg_gadget *g, bpg_buffer *b, const uint32_t *vars, uint64_t n_vars, const uint8_t *derived_scalars,
                                     const uint32_t *derived_vars, uint64_t n_derived);
bpg_status bpg_gadget_verify_buffered(bpg_gadget *g, bpg_buffer *b, const uint32_t *vars, uint64_t n_vars, const uint32_t *derived_vars, uint64_t n_derived);
bpg_status bpg_or_prover(bpg_prover *main, const bpg_buffer *b);
bpg_status bpg_or_verifier(bpg_verifier *main, const bpg_buffer *b);
bpg_status bpg_or_buffer(bpg_buffer *parent, const bpg_buffer *b);
/* utils::range_proof(cs, x, n, x_assignment) on a prover (assignment given) or a verifier (none) */
bpg_status bpg_range_proof_prove(bpg_prover *p, const bpg_lc *x, uint32_t n_bits, const uint8_t assignment[32]);
bpg_status bpg_range_proof_verify(bpg_verifier *v, const bpg_lc *x, uint32_t n_bits);
/* mimc::mimc_hash(preimage) -> Scalar bytes (little-endian); conversions */
bpg_status bpg_mimc_hash(const uint8_t *preimage, uint64_t len, uint8_t out[32]);
bpg_status bpg_be_to_scalars(const uint8_t *be, uint64_t len, uint8_t *out, uint64_t *n_out);   /* conversions::be_to_scalars */
/* MiMC Merkle trees: the native hash in front of Prover::commit - the root a verifier takes as its public input, the sibling lists that become the committed
 * values of a path proof, and both again after an insertion.  bpg_mimc_sponge is mimc::mimc_sponge_1 on the host (no context): n_blocks blocks of 32
 * little-endian bytes, each any 256-bit value (taken mod l, as the sponge's `state += block` takes it), canonical output.  The other calls run on the GPU of ctx:
 *   bpg_mimc_sponge_many   count sponges of blocks_per_item blocks each (in: count x blocks_per_item x 32, out: count x 32), one lane per item; at most 2^22
 *                          blocks per item (BPG_ERR_INVALID_ARGUMENT beyond).
 *   bpg_merkle_build       the full binary tree over 2^depth leaves, depth 1..24 (depth 24 holds 1 GB of device memory; the size is checked against the free
 *                          memory of the device first: BPG_ERR_DEVICE).  A node is sponge(left, right) over its children AS THEY ARE - leaves are not hashed
 *                          first - which is what MerkleTree256 constrains for a "(W W)" node.  The tree stays resident until bpg_merkle_free.
 *   bpg_merkle_root        the root; bpg_merkle_nodes: `count` nodes of `level` from node `first` (level 0 = the root, level depth = the leaves, 2^level nodes).
 *   bpg_merkle_paths       for each leaf index its `depth` siblings from the leaf level upward (siblings_out[i][0] is the sibling of leaf indices[i]); an index
 *                          may be given more than once.
 *   bpg_merkle_update      replaces leaf indices[i] by leaves[i] and recomputes only the ancestors of the replaced leaves, level by level, each once.  The indices
 *                          of one call are distinct: a repeated index is refused (there is no "last one wins"), and a refused call leaves the tree as it was.
 *                          An index at or above the tree's size (below) is refused; for a tree of bpg_merkle_build that is 2^depth.
 * Trees that grow - an accumulator of fixed depth (the path circuit is a template of one depth) whose n leaves arrive over time:
 *   bpg_merkle_build_partial  a tree of capacity 2^depth (depth 1..24, the memory check of bpg_merkle_build) holding `size` <= 2^depth leaves; every leaf from
 *                          `size` on holds `empty` (any 256-bit value taken mod l, as a leaf is; NULL = zero).  The layout rule: every node of the resident
 *                          array equals the node of bpg_merkle_build over leaves || empty x (2^depth - size), so root, nodes, paths and path_nodes serve
 *                          it unchanged and no circuit, template or verifier can tell.  A subtree without a leaf is one of depth + 1 constants, E_0 = empty,
 *                          E_{k+1} = node(E_k, E_k), computed on the host and written by one bandwidth-bound kernel; only the ancestors of real leaves
 *                          are hashed.  size may be 0 (leaves may then be NULL): the root is E_depth and no node function runs on the device.
 *   bpg_merkle_append      puts `count` leaves at [size, size + count) and recomputes exactly the ancestors of the new leaves, each once: one launch per
 *                          level whose dirty range holds more than 256 parents, then ONE launch from there to the root.  *first_index_out = the old size,
 *                          root_out = the new root (either may be NULL).  count == 0 is BPG_OK and only fills the outputs.  A tree of bpg_merkle_build
 *                          has size 2^depth: it takes no append.
 *   bpg_merkle_size        the number of leaves and the depth (either output may be NULL, not both).
 *   bpg_merkle_empty_nodes E_0 .. E_depth as (depth + 1) x 32 canonical bytes: out[k] = an empty subtree k levels above the leaves - the sibling a path meets
 *                          wherever it borders the empty region.  Works on every tree (bpg_merkle_build: empty = 0, computed at the first call); no device work.
 * Deep trees - the prefix layout, a second layout behind the same handle: a tree that only grows by append occupies a prefix of every level, and everything
 * right of the prefix is one of the constants E_k, so only the prefix is stored and depth stops being a memory question:
 *   bpg_merkle_build_prefix  a tree of capacity 2^depth, depth 1..32, with room for `reserve` leaves (1 <= reserve <= min(2^depth, 2^24)) holding `size` <=
 *                          reserve of them; `empty` as above.  Height s above the leaves stores max(1, ceil(reserve / 2^s)) nodes, so the tree holds
 *                          32 x (the sum of those widths over s = 0..depth, plus the depth + 1 constants) bytes of device memory - about 64 bytes per
 *                          reserved leaf: depth 32 with reserve 2^20 is 64 MB (the memory check applies to that count).  Node for node it is the tree
 *                          bpg_merkle_build_partial would build: root, nodes, paths, path_nodes, update, append, size, empty_nodes and free serve both
 *                          layouts under the same argument rules - any level, any node of a level, any leaf index below 2^depth; what is not stored
 *                          reads as its constant - and no circuit, template or verifier can tell.  update still reaches the leaves below `size` only.
 *   bpg_merkle_reserve     room for at least `leaves` leaves: a new buffer, ONE launch that moves every stored node and fills the new slots with their
 *                          constants, then the old buffer is released (both exist for that moment).  A no-op when the reserve is enough already; a
 *                          reserve never shrinks.  Refused: a tree of the dense layout (bpg_merkle_build, _build_partial), `leaves` > min(2^depth, 2^24).
 *   bpg_merkle_reserved    the reserve and the device bytes the tree holds (either output may be NULL, not both).  A dense tree reports 2^depth and the
 *                          32 x 2^(depth+1) bytes of its array.
 *   bpg_merkle_append on such a tree takes size + count <= min(2^depth, 2^24); a tree that outgrows its reserve first reserves min(that limit,
 *                          max(2 x reserve, size + count)) and then grows as above (wide launches, then one that climbs through up to 32 levels).  A
 *                          refused append leaves the tree and its reserve as they were.
 * Keyed trees - the third layout behind the same handle: leaves at any key, for a set addressed by an arbitrary 32-bit key (a revocation list, a nullifier
 * set, an allow-list keyed by account number).  A tree of depth 1..32 holds n <= 2^24 distinct keys below 2^depth, one leaf per key; every other leaf holds
 * `empty`.  Node for node it is the tree bpg_merkle_build would build over the 2^depth-entry list that is `empty` everywhere but at the keys: root, nodes,
 * paths, path_nodes, path inputs, circuits, templates and verifiers cannot tell the layouts apart, and a path of an absent key proves `empty` there.
 * Height s above the leaves stores exactly the nodes with a held key below them (the distinct values key >> s, ascending, beside their 32-byte values); what
 * is not stored reads as E_s.  Memory follows the sum of those counts - for random keys about n x (depth - lg n + 2) nodes of 36 bytes - plus the slack of
 * a doubling policy per height (csrc/host/merkle_keyed_plan.hpp).
 *   bpg_merkle_build_keyed the empty tree, then bpg_merkle_put of the `count` keys (any order) and their leaves; `empty` as above.
 *   bpg_merkle_put         replaces the leaf of a held key and inserts a key that is not held; *inserted_out = how many were inserted, root_out = the new
 *                          root.  The host sorts the keys; the device classifies them, merges brand-new positions into the arrays of every height
 *                          (reallocating a height that outgrows its room), and hashes exactly the proper ancestors of the put keys, each once.  count == 0
 *                          is BPG_OK and only fills the outputs.  A leaf equal to `empty` keeps its key held (no root or path differs from the absent key's).
 *   bpg_merkle_get         the leaves at `count` keys (any key below 2^depth; `empty`, reduced, where none is held) and held_out[i] = 1 or 0.  On a dense
 *                          or prefix tree: held = index < size.
 *   bpg_merkle_keys        held keys in ascending order, the run [first, first + count) of them (first + count <= the keys held).  Dense and prefix: key i = i.
 *   bpg_merkle_node_counts the stored nodes per height, height 0 first (depth + 1 counts), and the device bytes held (either may be NULL, not both).
 * On a keyed tree bpg_merkle_size gives the keys held, bpg_merkle_reserved (keys held, bytes held), bpg_merkle_update takes held keys only (a key that is not
 * held is BPG_ERR_INVALID_ARGUMENT and nothing changes); bpg_merkle_append and bpg_merkle_reserve refuse it.  bpg_merkle_put and bpg_merkle_node_counts
 * refuse dense and prefix trees.  Refused before the device is touched: depth 0 or above 32, a NULL pointer with a non-zero count, a key >= 2^depth, a key
 * given twice in one call, more than 2^24 keys in one call; a put that would make the tree hold more than 2^24 keys, or outgrow the device's free memory,
 * is refused before the first store to the tree.  A refused build sets *out to NULL.
 * size > 2^depth, size + count > 2^depth and a NULL `leaves` with a non-zero count are BPG_ERR_INVALID_ARGUMENT like the rest below; a refused
 * bpg_merkle_build_partial sets *out to NULL, and a refused call leaves the tree as it was and writes no output.
 * A depth of 0 or above 24 (bpg_merkle_build_prefix: above 32; a reserve of 0, above 2^depth or above 2^24; size > reserve), a NULL pointer, an index >= 2^depth, a level above depth, nodes beyond a level and count x blocks_per_item == 0 are
 * BPG_ERR_INVALID_ARGUMENT before the device is touched.  The calls run on the context's stream and return synchronised; a tree belongs to the context that built
 * it (another context's tree is BPG_ERR_INVALID_ARGUMENT); like every call on a context they are not re-entrant.  bpg_merkle_free releases the tree on the context
 * that built it, whatever ctx is passed (NULL included).  Destroying a context releases the device memory of the trees it still holds: their handles stay valid
 * for bpg_merkle_free alone, and every other call on them is BPG_ERR_INVALID_ARGUMENT.
 * Out of scope: more than 2^24 leaves or keys held, shrinking a reserve, removing keys from a keyed tree and reclaiming their storage, keys wider than
 * 32 bits, sorting incoming keys on the device, hashing records into keys, going under the latency floor of a narrow level (a
 * level narrower than the device still costs one node's 1,944 dependent products: an append of a few leaves is `depth` such floors in one launch), hashing
 * records into leaves on the device, the byte-preimage padding of mimc_hash on the device (pad on the host with bpg_be_to_scalars / bpg_mimc_hash's rules
 * and hand the blocks over), flags of the file drivers, and a tree spread over more than one GPU.  (Additions to ABI version 7: no struct changes.) */
typedef struct bpg_merkle bpg_merkle;
bpg_status bpg_mimc_sponge(const uint8_t *blocks, uint64_t n_blocks, uint8_t out[32]);
bpg_status bpg_mimc_sponge_many(bpg_ctx *ctx, uint64_t count, uint64_t blocks_per_item, const uint8_t *in, uint8_t *out);
bpg_status bpg_merkle_build(bpg_ctx *ctx, uint32_t depth, const uint8_t *leaves /* 2^depth x 32 */, bpg_merkle **out);
bpg_status bpg_merkle_build_partial(bpg_ctx *ctx, uint32_t depth, uint64_t size, const uint8_t *leaves /* size x 32; NULL allowed when size == 0 */,
                                    const uint8_t empty[32] /* NULL = zero */, bpg_merkle **out);
bpg_status bpg_merkle_append(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint8_t *leaves /* count x 32 */,
                             uint64_t *first_index_out /* NULL allowed */, uint8_t root_out[32] /* NULL allowed */);
bpg_status bpg_merkle_build_prefix(bpg_ctx *ctx, uint32_t depth, uint64_t reserve, uint64_t size, const uint8_t *leaves /* size x 32; NULL allowed when size == 0 */,
                                   const uint8_t empty[32] /* NULL = zero */, bpg_merkle **out);
bpg_status bpg_merkle_reserve(bpg_ctx *ctx, bpg_merkle *t, uint64_t leaves);
bpg_status bpg_merkle_reserved(bpg_ctx *ctx, bpg_merkle *t, uint64_t *reserve_out, uint64_t *bytes_out /* either may be NULL, not both */);
bpg_status bpg_merkle_size(bpg_ctx *ctx, bpg_merkle *t, uint64_t *size_out, uint32_t *depth_out /* either may be NULL, not both */);
bpg_status bpg_merkle_empty_nodes(bpg_ctx *ctx, bpg_merkle *t, uint8_t *out /* (depth + 1) x 32: out[k] = an empty subtree k levels above the leaves */);
bpg_status bpg_merkle_root(bpg_ctx *ctx, bpg_merkle *t, uint8_t out[32]);
bpg_status bpg_merkle_nodes(bpg_ctx *ctx, bpg_merkle *t, uint32_t level, uint64_t first, uint64_t count, uint8_t *out);
bpg_status bpg_merkle_paths(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, uint8_t *siblings_out /* count x depth x 32 */);
/* What a checkpointed template wants from these: bpg_mimc_sponge_states is bpg_mimc_sponge returning the state after EVERY block (out: n_blocks x 32; the last
 * entry is the digest); bpg_merkle_path_nodes gives for each leaf index the `depth` nodes ON its path, from the leaf's parent upward, the root last - the same
 * bytes bpg_merkle_nodes gives node by node - under the argument rules of bpg_merkle_paths. */
bpg_status bpg_mimc_sponge_states(const uint8_t *blocks, uint64_t n_blocks, uint8_t *out /* n_blocks x 32 */);
bpg_status bpg_merkle_path_nodes(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, uint8_t *out /* count x depth x 32 */);
bpg_status bpg_merkle_update(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *indices, const uint8_t *leaves /* count x 32 */);
bpg_status bpg_merkle_build_keyed(bpg_ctx *ctx, uint32_t depth, uint64_t count, const uint64_t *keys, const uint8_t *leaves /* count x 32; both NULL allowed when count == 0 */,
                                  const uint8_t empty[32] /* NULL = zero */, bpg_merkle **out);
bpg_status bpg_merkle_put(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *keys, const uint8_t *leaves /* count x 32 */, uint64_t *inserted_out /* NULL allowed */,
                          uint8_t root_out[32] /* NULL allowed */);
bpg_status bpg_merkle_get(bpg_ctx *ctx, bpg_merkle *t, uint64_t count, const uint64_t *keys, uint8_t *leaves_out /* count x 32 */, uint8_t *held_out /* count bytes, NULL allowed */);
bpg_status bpg_merkle_keys(bpg_ctx *ctx, bpg_merkle *t, uint64_t first, uint64_t count, uint64_t *keys_out);   /* held keys in ascending order, run [first, first + count) */
bpg_status bpg_merkle_node_counts(bpg_ctx *ctx, bpg_merkle *t, uint64_t *counts_out /* depth + 1, height 0 first; NULL allowed */, uint64_t *bytes_out /* NULL allowed, not both */);
void bpg_merkle_free(bpg_ctx *ctx, bpg_merkle *t);
/* test hook: `count` 64-byte TranscriptRng draws (merlin build_rng().rekey_with_witness_bytes("v_blinding")*.finalize(seed)), after
 * `skip` draws through the generic STROBE operations; bulk != 0 uses the prover's in-register bulk path. Same bytes either way. */
bpg_status bpg_rng_draws(const uint8_t transcript_state[203], uint64_t m, const uint8_t *v_blinding, const uint8_t rng_seed[32],
                         uint64_t skip, uint64_t count, int32_t bulk, uint8_t *out);
/* the same for `lanes` (1..8) generators with seeds rng_seeds[lanes][32] drawn in lockstep (csrc/host/merlin.hpp: eight sponges in the lanes of ZMM
   registers); lane v skips skip[v] draws first; out = [lanes][count][64] */
bpg_status bpg_rng_draws_multi(const uint8_t transcript_state[203], uint64_t m, const uint8_t *v_blinding, uint32_t lanes, const uint8_t *rng_seeds,
                               const uint64_t *skip, uint64_t count, uint8_t *out);
/* host Keccak-f[1600] self-check: runs the scalar and (when the CPU has AVX-512F+VL) both vector implementations on `rounds` chained
 * states derived from seed; *impl_out = the active one (0 scalar, 1 planes-in-ZMM, 2 lanes-in-XMM; chosen by a start-up calibration).
 * Fails with BPG_ERR_INTERNAL on a mismatch. */
bpg_status bpg_keccak_selftest(uint64_t seed, uint32_t rounds, int32_t *impl_out, double *ns_per_permutation);
/* host scalar arithmetic (curve25519_dalek::Scalar semantics), exposed for tests: op 0 add, 1 sub, 2 mul, 3 invert, 4 reduce, 5 from_wide(a = 64 B) */
bpg_status bpg_scalar_op(int32_t op, const uint8_t *a, const uint8_t *b, uint8_t out[32]);

#ifdef __cplusplus
}
#endif
#endif
