// Engine implementation: device buffers, generator derivation, the bucket-method MSM pipeline and the prove
// pipeline (dalek bulletproofs r1cs/prover.rs::prove + inner_product_proof.rs::create re-designed for one GPU;
// reference call site src/bin/prover.rs:92-93).  Fiat-Shamir stays on the host (merlin.hpp); every challenge is a
// 32..96-byte device->host copy followed by a few hundred bytes host->device.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <array>
#include <chrono>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <sched.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include "engine.hpp"
#include "hip_handles.hpp"
#include "host/fe51.hpp"
#include "host/chain.hpp"
#include "host/fiat_shamir.hpp"
#include "host/csc_work.hpp"
#include "host/verify_wave_plan.hpp"
#include "host/merkle_plan.hpp"
#include "host/merkle_prefix_plan.hpp"
#include "hip/kernels.cuh"

namespace bpg {

// launch on the engine stream, bracketed by HIP events when the profile asks for this kernel
#define BPG_LAUNCH_ID(I, id, kernel, grid, block, ...) do { (I).prof_begin(id); hipLaunchKernelGGL(kernel, grid, block, 0, (I).st, __VA_ARGS__); (I).prof_end(id); } while (0)
#define BPG_LAUNCH(I, kernel, grid, block, ...) BPG_LAUNCH_ID(I, KID_##kernel, kernel, grid, block, __VA_ARGS__)
#define BPG_LAUNCH_LDS(I, id, kernel, grid, block, lds, ...) do { (I).prof_begin(id); hipLaunchKernelGGL(kernel, grid, block, lds, (I).st, __VA_ARGS__); (I).prof_end(id); } while (0)

namespace {

// Generator tables of one (device, capacity), shared by every context of the process on that device: the affine-Niels table [G | H] and, built on
// first use, the odd multiples for the width-w NAF fold (one set per w).  Immutable once published, so contexts on different streams read them
// freely; two proving streams then gather from ONE 201 MB table that the Infinity Cache holds, instead of two that evict each other.  A context that
// needs a larger capacity moves to another generation; a generation is freed with its last context.
// Bytes of precomputed multiples (fold tables + wide tail tables) held on each device by ALL generations of this process: what the table budget
// of a context (bpg_config.table_budget_gb) is compared with, so that a process serving mixed circuit sizes cannot pin more than it was given.
static std::mutex g_table_bytes_mutex;
static std::map<int, uint64_t> g_table_bytes;
static uint64_t table_bytes_held(int device) { std::lock_guard<std::mutex> lk(g_table_bytes_mutex); return g_table_bytes[device]; }
static void table_bytes_add(int device, int64_t delta) { std::lock_guard<std::mutex> lk(g_table_bytes_mutex); g_table_bytes[device] = (uint64_t)((int64_t)g_table_bytes[device] + delta); }
// Proofs this process has in flight per device.  Some steps come in two variants with the same results: one that finishes soonest on an idle
// device (four lanes per output in the small folds, sweep chunks fitted to whole rounds of resident blocks, 15-bit windows) and one with the
// fewest instructions (one lane per output, 64-entry chunks, 16-bit windows); a proof that shares the device with others takes the second
// (Impl::shared_variants; measured at 2^20, profiles/r03_tail_start.txt: 1.9 ms per proof sustained, and 1.7 ms more for a proof alone).
// BPG_FOLD_ADAPT=0 pins the first set, 2 the second.
static std::atomic<int> g_proving[64];
struct ProvingGuard {
    std::atomic<int> &c;
    explicit ProvingGuard(int device) : c(g_proving[(unsigned)device & 63u]) { c.fetch_add(1, std::memory_order_relaxed); }
    ~ProvingGuard() { c.fetch_sub(1, std::memory_order_relaxed); }
};
static bool device_shared(int device) { return g_proving[(unsigned)device & 63u].load(std::memory_order_relaxed) > 1; }
struct SharedTables {
    int device = 0; uint64_t cap = 0;
    DevBuf gens;
    std::mutex m;                                   // guards odd, wide, refused (construction on first use)
    std::map<uint32_t, DevBuf> wide;                // M0 -> 8-bit window tables of G[0..M0), H[0..M0) for a tail that starts on the original generators (k_tt_round8)
    std::map<uint32_t, DevBuf> odd;                 // (w | parts << 8) -> [parts * 2^(w-2) - 1][2*cap] Niels points: (2m+1) * 2^(j*L) * P, see FoldWnaf
    std::map<uint64_t, uint64_t> refused;           // table key (odd: w | parts << 8; wide: 1 << 32 | M0) -> bytes held on the device when its allocation failed:
                                                    // not tried again until the device holds less (no failing 50 GB hipMalloc per proof)
    ~SharedTables() {       // on the tables' device, and their share of the table budget given back; the members then free themselves
        (void)hipSetDevice(device);
        uint64_t held = 0;
        for (auto &kv : odd) held += kv.second.cap;
        for (auto &kv : wide) held += kv.second.cap;
        table_bytes_add(device, -(int64_t)held);
    }
};
// The 486 MiMC round constants in Montgomery form, once per device: contexts created on one device share the buffer, and it goes with the last of them.
struct MimcConstants {
    int device = 0; DevBuf rc;
    ~MimcConstants() { (void)hipSetDevice(device); }
};
static std::mutex g_mimc_mutex;
void merkle_orphan(DeviceMerkle *t);                // (defined with DeviceMerkle, below) releases the device memory of a tree whose context is being destroyed
static std::map<int, std::weak_ptr<MimcConstants>> g_mimc;
static std::mutex g_tables_mutex;                   // held across a derivation: contexts created side by side derive once
static std::map<std::pair<int, uint64_t>, std::weak_ptr<SharedTables>> g_tables;

inline uint32_t cdiv(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// host Scalar (plain, canonical) <-> device Montgomery form
const Scalar &R1_plain() { static Scalar r = [] { Scalar s; s.w[0] = 0xd6ec31748d98951dULL; s.w[1] = 0xc6ef5bf4737dcf70ULL; s.w[2] = 0xfffffffffffffffeULL; s.w[3] = 0x0fffffffffffffffULL; return s; }(); return r; }
const Scalar &Rinv_plain() { static Scalar r = R1_plain().invert(); return r; }
scm to_scm(const Scalar &s) { Scalar m = s * R1_plain(); scm o; std::memcpy(o.v, m.w, 32); return o; }
Scalar from_scm(const scm &m) { Scalar s; std::memcpy(s.w, m.v, 32); return s * Rinv_plain(); }

// One msm() call: the segments (a kernel argument, layout fixed) and, beside them, what only the host needs to know about them.  The counts travel with
// the segments they describe, so no call can be sized by what was pushed for another.
struct MsmJob {
    MsmSegs S;
    uint32_t skipped;        // terms whose skip bit is set (they make no entries): the window width and the entry lists are sized for the rest
    uint32_t alg_discount;   // terms that are not terms of the sum the call computes (merged-point terms stand in for terms that were skipped): roofline bookkeeping only
};
MsmJob job_new() { MsmJob J; std::memset(&J, 0, sizeof J); return J; }
void seg_push(MsmJob &J, const scm *sc, const ge_niels *pts, uint32_t len, uint32_t msm, uint32_t lgblk = 31, const uint32_t *skip = nullptr) {
    if (!len) return;
    MsmSegs &S = J.S;
    if (S.nseg >= BPG_MAX_SEGS) throw std::logic_error("too many MSM segments");
    uint32_t k = S.nseg++;
    S.sc[k] = sc; S.pts[k] = pts; S.len[k] = len; S.msm[k] = msm; S.lgblk[k] = lgblk; S.skip[k] = skip;
    S.start[k + 1] = S.start[k] + len;
}
// the segment of merged points (hip/k_merge.cuh): `groups` terms that stand in for the `skipped` terms whose skip bits the other segments of the job carry
void seg_push_merged(MsmJob &J, const scm *sc, const ge_niels *pts, uint32_t groups, uint32_t msm, uint32_t skipped) {
    seg_push(J, sc, pts, groups, msm);
    J.alg_discount += groups; J.skipped += skipped;
}
static_assert(sizeof(ge_ext) == MSM_POINT_BYTES, "host/msm_plan.hpp sizes the MSM workspace in extended points");

constexpr uint32_t TEMPLATE_HOST_COPY_LG = 14;     // templates up to this padded size keep a host copy of their rows (the widest lockstep proof: BPG_TT_ORIG_LG <= 14)

// On-disk cache of the generator tables (reference src/bin/prover.rs:92 re-derives them on every run).  Opt-in:
// BPG_GENS_CACHE_DIR names a directory; the file gens_<capacity>.bpg holds a header and the affine Niels table [G | H] exactly as it lives
// in HBM.  A file is used only if its header, length and checksum agree AND a sample of its points equals freshly derived ones.  The checksum
// catches corruption, not an adversary: whoever can write the file chooses the generators (a table with known discrete-log relations lets
// verify() accept forged proofs), so the cache trusts the FILE SYSTEM: directory and file must belong to the calling user and be writable by
// nobody else (gens_cache_trusted), files are written through an O_EXCL | O_NOFOLLOW temporary and renamed.
struct GensCacheHeader { char magic[8]; uint64_t version, capacity, bytes, checksum; };
static const char kGensMagic[8] = {'B', 'P', 'G', 'G', 'E', 'N', 'S', '1'};
uint64_t gens_checksum(const uint8_t *p, size_t n) {            // four interleaved multiply-rotate lanes over 8-byte words (about 10 GB/s): corruption, not adversaries
    uint64_t h[4] = {0x9e3779b97f4a7c15ull, 0xc2b2ae3d27d4eb4full, 0x165667b19e3779f9ull, 0x27d4eb2f165667c5ull};
    size_t i = 0;
    for (; i + 32 <= n; i += 32) for (int k = 0; k < 4; k++) { uint64_t w; std::memcpy(&w, p + i + 8 * k, 8); h[k] = (h[k] ^ w) * 0x100000001b3ull; h[k] = (h[k] << 29) | (h[k] >> 35); }
    for (; i < n; i++) h[0] = (h[0] ^ p[i]) * 0x100000001b3ull;
    return h[0] ^ (h[1] * 3) ^ (h[2] * 5) ^ (h[3] * 7) ^ (uint64_t)n;
}
// the cache directory (and, when it exists, the file) is owned by this user and not writable by group or others
bool gens_cache_trusted(const std::string &dir, const std::string &file) {
    struct stat st;
    if (::stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode) || st.st_uid != ::geteuid() || (st.st_mode & (S_IWGRP | S_IWOTH))) return false;
    if (::lstat(file.c_str(), &st) != 0) return true;                       // nothing there yet
    return S_ISREG(st.st_mode) && st.st_uid == ::geteuid() && !(st.st_mode & (S_IWGRP | S_IWOTH));
}
std::string gens_cache_path(const std::string &dir, uint64_t cap) {
    if (dir.empty()) return std::string();
    return dir + "/gens_" + std::to_string(cap) + ".bpg";
}

}  // namespace

struct DeviceCircuit {
    uint64_t n = 0, m = 0, q = 0, ncols = 0, nnz = 0;
    bool has_witness = false;
    uint64_t const_begin = 0;      // first entry of the constant-terms column (the last one)
    DevBuf aL, aR, aO, col_ptr, ent_row, ent_coef, coef;
    // equal-scalar merging of A_I and A_O (hip/k_merge.cuh), built at the first prove() of this witness: terms of <a_L, G> + <a_R, H> (of <a_O, G>) that carry
    // the same scalar -> one term on the sum of their generators (pts, affine Niels) with that scalar (sc); skipA / skipB mark the terms that were merged away
    // (one bit per multiplier: a_L and a_R for A_I, a_O for A_O)
    struct MergeSet { uint32_t groups = 0, skipped = 0; DevBuf skipA, skipB, sc, pts; };
    bool merge_tried = false;
    MergeSet mI, mO;
    // circuit template (upload_template): the packed witness program and its schedule in HBM, the committed values of the last assign(), and where the
    // per-witness constant terms live in `coef` (slots [param_first, param_first + n_params))
    bool is_template = false;
    DevBuf wit_stream, wit_segs, wit_v;
    // checkpoints (WitnessProgramView::ck_var): the variables, and the values of the last assign_checkpointed (a repeat: rep_count x n_ck of them)
    uint64_t n_ck = 0;
    DevBuf wit_ck_var, wit_ck;
    // public inputs (WitnessProgramView::n_inputs): the values of the last assign_inputs, and the derived coefficient slots [slot_first, slot_first + n_slots) of
    // `coef` with the (input, coefficient index) pair of each (host/template.hpp InputSlot), which k_input_slots reads
    // A repeat or join WITH inputs (repeat_template / join_templates, with_inputs): n_in and n_slots are the totals over all items, in_slots the sources' pair lists
    // one after the other, and k_input_slots_join fills the slots from slot_parts descriptors in join_desc (a repeat: one, made for this kernel alone; 0: a
    // single template, k_input_slots).  The derived slots are STICKY state of the circuit: they stand as the last assign_inputs or set_inputs left them.
    uint64_t n_in = 0, slot_first = 0, n_slots = 0;
    // gates (WitnessProgramView::n_gates): with any, variable columns of the matrix name derived slots too (host/template.hpp); repeat, join and check_batch refuse
    uint64_t n_gates = 0;
    uint32_t slot_parts = 0;
    DevBuf wit_in, in_slots;
    bool wit_v_set = false;                 // wit_v holds the values of an assign() (a template uploaded WITH its witness has a_L, a_R, a_O and no values yet)
    std::vector<uint32_t> wit_level_ptr;    // level l = segments [wit_level_ptr[l], wit_level_ptr[l + 1]) of wit_segs
    uint64_t n_params = 0, param_first = 0;
    // host copy of the rows with their parameter slots (TemplatePlan::slotted), which the lockstep packer of prove_template_batch reads: kept only for
    // padded N <= 2^14 - a larger template never takes the lockstep path, and a 2^20 one would hold hundreds of MB of host memory for nothing
    bool has_host = false;
    FlatCircuit host;
    FlatView host_view;
    // a template repeated on the device (repeat_template, hip/k_repeat.cuh): rep_count copies of a source template of rep_n multipliers and rep_m committed
    // values, whose packed program (wit_stream, wit_segs, wit_level_ptr: copies of the source's) assign() walks once per (segment, item).  0: not a repeat.
    uint64_t rep_count = 0, rep_n = 0, rep_m = 0, rep_in = 0;       // rep_in: the public inputs of ONE item (n_in = rep_count x rep_in)
    // templates joined on the device (join_templates, hip/k_join.cuh): the descriptors of the parts (host copy and device array), the parts' programs one after
    // the other in wit_stream / wit_segs / wit_ck_var, and the block table of assign(): level l = blocks [join_level_ptr[l], join_level_ptr[l + 1]) of join_blocks.
    // n_ck is the total over all parts and items.  No part: not a join.
    std::vector<JoinPart> join_parts;
    DevBuf join_desc, join_blocks;
    std::vector<uint32_t> join_level_ptr;
    int device = 0;                         // the device the buffers live on
    const void *owner = nullptr;            // the Engine that made the circuit (verify_resident_batch refuses a circuit of another context)
    // row-major view of the matrix for check() (hip/k_check.cuh), derived from the column-major one at the first check and kept until the circuit is freed (the
    // matrix never changes; parameter values live in `coef`, which the view indexes): rv_ptr = q + 1 row starts, rv_ent = nnz pairs (column, coefficient slot),
    // rv_long = [count | the rows of more than rv_threshold terms].  Plain device memory: no part of the table budget.
    bool rv_built = false;
    uint32_t rv_threshold = 0;
    DevBuf rv_ptr, rv_ent, rv_long;
};

// kernel ids for the optional HIP-event profile (bpg_profile_*)
#define BPG_KERNELS(X) X(k_gens_derive) X(k_normalize_niels) X(k_compress_niels) X(k_pedersen) X(k_sc_from_bytes) \
    X(k_sc_from_wide) X(k_blind_poison) X(k_exp_table) X(k_reduce_partials) X(k_flatten) X(k_flatten_const) X(k_poly_t) X(k_poly_eval) X(k_ipa_prep) \
    X(k_ipa_fold_scalars) X(k_fold_points) X(k_fold_points_reg) X(k_fold_points_split) X(k_fold_points_wnaf) X(k_fold_points_quad) X(k_fold_points_quadw) X(k_fold_points_regw) X(k_odd_start) X(k_odd_start_ext) X(k_dbl_times) X(k_odd_step) X(k_msm_digits) X(k_msm_scatter1) X(k_msm_sort2) X(k_scan_blocksums) \
    X(k_scan_apply) X(k_bucket_chunks) X(k_bucket_combine) X(k_bucket_combine_heavy) X(k_bucket_reduce) X(k_window_sums) X(k_window_sums_quad) X(k_decompress) X(k_ipa_s) X(k_verify_scalars) X(k_verify_scalars_acc) X(k_bench_fe_mul) \
    X(k_tt_bases) X(k_tt_multiples) X(k_tt_bases8) X(k_tt_multiples8) X(k_tt_round8) X(k_tt_factors) X(k_tt_advance) X(k_tt_round) X(k_tt_finish) X(k_blind_expand) X(k_tt_commit3) X(k_tt_commit3_finish) X(k_csc_count) X(k_csc_fill) X(k_csc_colptr) X(k_merge_insert) X(k_merge_plan) X(k_merge_groups) X(k_merge_members) X(k_merge_sum) \
    X(k_bt_commit3) X(k_bt_commit3_finish) X(k_bt_compress) X(k_bt_exp) X(k_bt_poly_t) X(k_bt_poly_eval) X(k_bt_factors) X(k_bt_advance) X(k_bt_round) \
    X(k_bt_finish) X(k_bt_fold_scalars) X(k_witness_eval) X(k_witness_eval_batch) X(k_bt_commit_v) X(k_repeat_colptr) X(k_repeat_entries) X(k_repeat_coef) X(k_witness_eval_repeat) X(k_witness_ck_verify) X(k_witness_ck_verify_batch) \
    X(k_join_colptr) X(k_join_entries) X(k_join_coef) X(k_witness_eval_join) X(k_witness_ck_verify_join) X(k_input_slots) X(k_input_slots_join) \
    X(k_mimc_sponge) X(k_merkle_leaves) X(k_merkle_level) X(k_merkle_top) X(k_merkle_level_list) X(k_merkle_set_leaves) X(k_merkle_paths) X(k_merkle_export) X(k_merkle_fill_empty) X(k_merkle_level_range) X(k_merkle_climb) \
    X(k_mpx_fill) X(k_mpx_range) X(k_mpx_climb) X(k_mpx_list) X(k_mpx_set_leaves) X(k_mpx_paths) X(k_mpx_export) X(k_mpx_relayout) \
    X(k_mkx_classify) X(k_mkx_scan_sums) X(k_mkx_scan_top) X(k_mkx_scatter) X(k_mkx_merge) X(k_mkx_set_leaves) X(k_mkx_level) X(k_mkx_climb) X(k_mkx_paths) X(k_mkx_export) X(k_mkx_get) X(k_mkx_keys) X(k_mkx_gather) \
    X(k_rowview_count) X(k_rowview_fill) X(k_rowview_long) X(k_check_mul) X(k_check_rows) X(k_check_rows_long) X(k_check_count) \
    X(k_vw_exp) X(k_vw_tails) X(k_vw_flatten) X(k_vw_small) X(k_vw_scalars) X(k_vw_reduce)
enum KernelId {
#define X(n) KID_##n,
    BPG_KERNELS(X)
#undef X
    KID_COUNT
};
static const char *const kKernelNames[KID_COUNT] = {
#define X(n) #n,
    BPG_KERNELS(X)
#undef X
};

struct Engine::Impl {
    Stream st;                                  // the first member: destroyed last, after every buffer, event and copy stream below
    int device = 0;
    ~Impl();                                    // waits for the context's work, then the members free themselves (defined below the constructor)
    // profiling: mode 0 off, 1 = the generator-fold kernels and the bucket sweep only (a few launches per proof: cheap enough for
    // timed regions), 2 = every kernel
    int prof_mode = 0;
    struct ProfRec { int id; Event a, b; };
    std::vector<ProfRec> prof_open;
    std::vector<Event> prof_pool;
    double prof_ms[KID_COUNT] = {0};
    std::vector<float> prof_wit_ms;     // the first 1024 k_witness_eval / k_witness_eval_repeat / k_witness_eval_join launches since the last reset, in launch order (a launch = a level of an assign)
    std::vector<std::pair<int, float>> prof_merkle_ms;   // the first 512 launches of the tree-hashing kernels (k_merkle_level, _top, _level_list, _level_range, _climb, k_mpx_range, _climb, _list, k_mkx_level, _climb) since the last reset, in launch order
    uint64_t prof_count[KID_COUNT] = {0};
    double prof_alg_bytes[KID_COUNT] = {0}, prof_act_bytes[KID_COUNT] = {0}, prof_fm[KID_COUNT] = {0};
    bool prof_on(int id) const { return prof_mode == 2 || (prof_mode == 1 && (id == KID_k_fold_points || id == KID_k_fold_points_reg || id == KID_k_fold_points_split || id == KID_k_fold_points_wnaf || id == KID_k_fold_points_quad || id == KID_k_fold_points_quadw || id == KID_k_fold_points_regw || id == KID_k_bucket_chunks)); }
    Event prof_event() { if (prof_pool.empty()) return Event::timed(); Event e = std::move(prof_pool.back()); prof_pool.pop_back(); return e; }
    void prof_begin(int id) { if (!prof_on(id)) return; ProfRec r{id, prof_event(), prof_event()}; HIPCHK(hipEventRecord(r.a, st)); prof_open.push_back(std::move(r)); }
    void prof_end(int id) { if (!prof_on(id)) return; HIPCHK(hipEventRecord(prof_open.back().b, st)); }
    void prof_note(int id, double alg_bytes, double act_bytes, double fm) { if (!prof_on(id)) return; prof_alg_bytes[id] += alg_bytes; prof_act_bytes[id] += act_bytes; prof_fm[id] += fm; }
    void prof_collect() {
        if (prof_open.empty()) return;
        HIPCHK(hipStreamSynchronize(st));
        for (ProfRec &r : prof_open) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, r.a, r.b)); prof_ms[r.id] += ms; prof_count[r.id]++; if ((r.id == KID_k_witness_eval || r.id == KID_k_witness_eval_repeat || r.id == KID_k_witness_eval_join) && prof_wit_ms.size() < 1024) prof_wit_ms.push_back(ms); if ((r.id == KID_k_merkle_level || r.id == KID_k_merkle_top || r.id == KID_k_merkle_level_list || r.id == KID_k_merkle_level_range || r.id == KID_k_merkle_climb || r.id == KID_k_mpx_range || r.id == KID_k_mpx_climb || r.id == KID_k_mpx_list || r.id == KID_k_mkx_level || r.id == KID_k_mkx_climb) && prof_merkle_ms.size() < 512) prof_merkle_ms.emplace_back(r.id, ms); prof_pool.push_back(std::move(r.a)); prof_pool.push_back(std::move(r.b)); }
        prof_open.clear();
    }
    void prof_reset() { prof_collect(); for (int i = 0; i < KID_COUNT; i++) { prof_ms[i] = 0; prof_count[i] = 0; prof_alg_bytes[i] = prof_act_bytes[i] = prof_fm[i] = 0; } prof_wit_ms.clear(); prof_merkle_ms.clear(); }
    std::shared_ptr<SharedTables> shared;       // the generation of generator tables this context works on
    const ge_niels *gens = nullptr;             // shared->gens, [G | H]: a view, the generation owns the table
    DevBuf bases, scratch_ext, comp, small_in, small_sc;
    // MiMC sponges and Merkle trees (hip/k_mimc.cuh): the round constants of this device (shared by its contexts), the staging buffers of the calls, and the trees
    // this context built and has not freed (the destructor releases their device memory; bpg_merkle_free then only deletes the handle)
    std::shared_ptr<MimcConstants> mimc;
    DevBuf mk_in, mk_out;
    DevBuf mkx_dirty, mkx_fresh, mkx_flags, mkx_sums, mkx_totals, mkx_merge;    // a put into a keyed tree (hip/k_merkle_keyed.cuh): dirty lists, brand-new positions, scan scratch, a merge in place
    std::vector<DeviceMerkle *> trees;
    // check() (hip/k_check.cuh): the caller's committed values of a plain upload, the violation bitmap (a bit per row), the four counters of the report
    DevBuf chk_v, chk_bitmap, chk_report;
    DevBuf ck_first;                            // assign_checkpointed: the lowest mismatching checkpoint (8 bytes)
    uint32_t check_threshold = CHECK_ROW_THRESHOLD;     // rows of more terms get a wave each (BPG_CHECK_THRESHOLD)
    void rowview_build(DeviceCircuit *c);
    void fill_input_slots(DeviceCircuit *c);    // assign_inputs, set_inputs: the derived coefficient slots from the resident inputs, one launch
    // One arena for the large per-stream buffers whose lifetimes never overlap in stream order (round 5: 20 proving streams held 2.9 GB each):
    //   an MSM:        [digits | entries1] (dead once k_msm_sort2 has run) overlaid by the sweep's partial sums (slots); entries behind them
    //   poly phase:    flattened weights, powers of z and y (between the S sums and the first round of the inner-product argument)
    //   IPA tail:      the window tables of the folded generators (0.54 GB; no MSM runs once the tail has started)
    // Everything is queued on ONE stream, so a later phase's kernels start after the earlier phase's have finished.  Growing the arena frees it first
    // (hipFree synchronises the device), exactly as growing any DevBuf does.
    DevBuf arena;
    uint8_t *arena_at(size_t off) const { return arena.as<uint8_t>() + off; }
    // Waiting for the stream inside a proof (a round of the inner-product argument ends with one: the host needs L, R for the transcript).  With blocking waits
    // (bpg_config.blocking_sync = 1: a host with many proving threads beside its chain threads) a wake-up costs tens of microseconds, twenty-odd times per
    // proof; a proof that has the device to ITSELF has a core to spare, so it polls first (a proof alone: 1.5 ms; the mix never polls) and blocks only
    // when the work is long.
    bool blocking_waits = false;
    void wait_stream() {
        if (blocking_waits && !shared_now) {
            const double until = now_ms() + 3.0;
            do {
                const hipError_t e = hipStreamQuery(st);
                if (e == hipSuccess) return;
                if (e != hipErrorNotReady) HIPCHK(e);
                for (int k = 0; k < 64; k++) __builtin_ia32_pause();
            } while (now_ms() < until);
        }
        HIPCHK(hipStreamSynchronize(st));
    }
    static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
    // MSM workspace
    DevBuf counts, starts, cursor, blocksum, buckets, partial, msm_result, open_keys, medium, wsums, wq_stage, wq_tickets, tile_hist, heavy, plain, starts1;   // tile_hist, plain: workspace of upload(); digits, the entry lists and the sweep's partial sums live in the arena
    uint32_t sweep_blocks_resident = 1024;   // blocks of k_bucket_chunks the device holds at once: 4 per CU of the device the context is created on (BPG_SWEEP_RESIDENT overrides)
    uint32_t msm_cmax = 15;         // widest window of a proof ALONE on the device (BPG_MSM_CMAX sets both caps)
    uint32_t msm_cmax_shared = 16;  // ... and while other proofs share the device: 16 windows instead of 17 per term, twice the buckets (digits are 16-bit)
    uint32_t rseg = 8;              // buckets per thread of k_bucket_reduce, a power of two (BPG_RSEG)
    uint32_t lgch = 0;              // BPG_LGCH: pins the sweep's chunk length to 2^lgch entries (0 = fitted, see msm())
    bool gens_share = true;         // BPG_GENS_SHARE=0: this context derives (or loads) and keeps generator tables of its own
    uint32_t profile = 1;           // 1 one-shot, 2 serving (what bpg_config / BPG_PROFILE settled on)
    bool shared_now = false;        // sampled ONCE per prove()/verify(): does this call take the shared-device variants (shared_variants())
    uint32_t msm_cmin = 2;          // BPG_MSM_CMIN: narrowest window (tests: wide windows on small sums)
    uint32_t wit_waves = 1024;      // waves k_witness_eval spreads a level's lanes over: one per SIMD of the device the context is created on
    uint32_t merge_equal = 1;       // BPG_MERGE: 0 A_I and A_O term by term; 1 equal scalars grouped once per uploaded witness (at its first proof); 2 grouped afresh in EVERY
                                    // proof (what a host that proves each witness once pays: the measurement behind bench.py's `merge_per_proof`); same bytes
    uint32_t merged_last = 0, merged_skipped_last = 0;   // witness of the last prove(): groups of equal scalars in A_I and A_O, and the terms they replace (0: none, or the table-driven path)
    void merge_witness(DeviceCircuit *c, const ge_niels *Gtab, const ge_niels *Htab);
    void merge_build(DeviceCircuit::MergeSet &M, const scm *A, const ge_niels *PA, uint32_t nA, const scm *B, const ge_niels *PB, uint32_t nB);
    double merge_ms_last = 0;       // host wall time of the last merge_witness() that did something (BPG_MERGE=1: to the end of its kernels; 2: to the end of the group count's read-back)
    // prove buffers
    DevBuf sLR, yinvpow, lv, rv, red_partial, red_out, raw_rng, extras;      // (y^i, z^j and the flattened weights: in the arena)
    DevBuf stale_flag;              // one word, zero unless k_sc_from_wide met a poisoned (never uploaded) draw: checked before a proof leaves prove()
    DevBuf ipa_s, ipa_tabA, ipa_tabB, naf, qsteps, vfy_in, vfy_pts, vfy_ok, vfy_sc, vfy_ch;
    DevBuf vfy_small;               // verify_batch: per proof [w_V (m) | w_c | delta]
    // verify_resident_batch (hip/k_vwave.cuh): the items' own parameter and input values as bytes, what each brings (flags), the circuit's standing tail
    // (copied before the first wave; the item-by-item pass of a rejected batch restores the table from it), one item's tail for that pass
    DevBuf vw_raw, vw_flags, vw_standing, vw_tail1;
    uint32_t cu_count = 256;        // compute units of the device the context is created on: the block target of k_vw_scalars (host/verify_wave_plan.hpp)
    // table-driven IPA tail (kernels.cuh k_tt_*): frozen-generator window tables, per-point factors, coefficient tables
    DevBuf tt_bases, tt_table, tt_f, tt_c, tt_partial, grp_c, ped_table, s_parts;
    // tt_table holds the tables of the ORIGINAL generators G[0..M0), H[0..M0) when tt_orig_M0 != 0: they survive across proofs (a circuit
    // with N <= 2^tt_orig_lg freezes its generators at round 0) and also serve A_I, A_O, S (k_tt_commit3)
    uint32_t tt_orig_M0 = 0; const void *tt_orig_gens = nullptr;
    ge_pniels *tt_table_p = nullptr;            // the window tables in use: tt_table (original generators) or the arena (folded ones), set by tt_build
    void tt_build(const ge_niels *G, const ge_niels *H, const ge_niels *B, uint32_t M0, bool original) {
        const uint32_t npts = 2 * M0 + 1;
        if (original && tt_orig_M0 == M0 && tt_orig_gens == gens) { tt_table_p = tt_table.as<ge_pniels>(); return; }
        const size_t bb = al256((size_t)npts * TT_WINDOWS * sizeof(ge_ext)), tb = (size_t)npts * TT_WINDOWS * TT_MULTS * sizeof(ge_pniels);
        ge_ext *basesp;
        if (original) {     // tables of the ORIGINAL generators outlive the proof (and serve A_I, A_O, S of the next one): buffers of their own
            tt_orig_M0 = 0;                             // (tables of folded generators live in the arena and leave these alone)
            tt_bases.ensure(bb); tt_table.ensure(tb);
            basesp = tt_bases.as<ge_ext>(); tt_table_p = tt_table.as<ge_pniels>();
        } else {            // tables of FOLDED generators live for the tail of one proof: in the arena, where the MSM workspace of the rounds before was
            arena.ensure(bb + tb);
            basesp = reinterpret_cast<ge_ext *>(arena_at(0)); tt_table_p = reinterpret_cast<ge_pniels *>(arena_at(bb));
        }
        tt_partial.ensure((size_t)3 * cdiv((uint64_t)M0 * 16, 256) * sizeof(ge_ext));
        BPG_LAUNCH((*this), k_tt_bases, dim3(cdiv(npts, 64)), dim3(256), G, H, B, basesp, M0);
        BPG_LAUNCH((*this), k_tt_multiples, dim3(cdiv((uint64_t)npts * TT_WINDOWS, 256)), dim3(256), basesp, tt_table_p, npts * TT_WINDOWS);
        if (original) { tt_orig_M0 = M0; tt_orig_gens = gens; }
    }
    // 8-bit window tables of the original generators (kernels.cuh k_tt_round8): shared per device like the fold tables, built on first use
    // Budgets.  table_budget bounds the CUMULATIVE bytes of precomputed multiples (fold tables + wide tail tables, every capacity) this process
    // holds on the device (bpg_config.table_budget_gb / BPG_TABLE_GB; profile default: one-shot 4 GB, serving 96 GB); the two per-kind caps are
    // diagnostics (BPG_TT_WIDE_GB, BPG_FOLD_TABLE_GB).
    uint64_t table_budget = 4ull << 30;
    uint64_t tt_wide_budget = 0;                // widest single 8-bit tail table (17.2 GB at M0 = 2^14); 0 = never (the one-shot profile)
    std::string gens_cache_dir;                 // bpg_config.gens_cache_dir / BPG_GENS_CACHE_DIR
    // Reserve `bytes` of the device's table budget (shared->m held).  Check and reservation happen under ONE lock of the per-device byte count, so
    // two generations of different capacity (each under its own shared->m) cannot both pass the check and overshoot the budget together; the
    // caller gives the bytes back (table_bytes_add(-bytes)) when its allocation fails.
    bool table_reserve(uint64_t key, uint64_t bytes) const {
        std::lock_guard<std::mutex> lk(g_table_bytes_mutex);
        uint64_t &held = g_table_bytes[shared->device];
        auto it = shared->refused.find(key);
        if (it != shared->refused.end() && held >= it->second) return false;      // failed with this much (or less) held: do not try again
        if (held + bytes > table_budget) return false;
        held += bytes;
        return true;
    }
    const ge_pniels *wide_ensure(uint32_t M0) {
        const uint64_t bytes = (uint64_t)2 * M0 * TT8_WINDOWS * TT8_MULTS * sizeof(ge_pniels);
        if (M0 < 64 || bytes > tt_wide_budget) return nullptr;
        std::lock_guard<std::mutex> lk(shared->m);
        auto it = shared->wide.find(M0);
        if (it != shared->wide.end()) return it->second.as<ge_pniels>();
        const uint64_t key = (1ull << 32) | M0;
        if (!table_reserve(key, bytes)) return nullptr;                          // the 4-bit tables of the context do
        DevBuf table, bases8;
        try { table.ensure(bytes); bases8.ensure((size_t)2 * M0 * TT8_WINDOWS * sizeof(ge_ext)); }
        catch (const std::exception &) {
            (void)hipGetLastError();
            table_bytes_add(shared->device, -(int64_t)bytes); shared->refused[key] = table_bytes_held(shared->device); return nullptr;
        }
        try {
            BPG_LAUNCH((*this), k_tt_bases8, dim3(cdiv(2 * M0, 64)), dim3(256), gens, gens + gens_cap, bases8.as<ge_ext>(), M0);
            BPG_LAUNCH((*this), k_tt_multiples8, dim3(cdiv((uint64_t)2 * M0 * TT8_WINDOWS, 256)), dim3(256), bases8.as<ge_ext>(), table.as<ge_pniels>(), 2 * M0 * TT8_WINDOWS);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        } catch (...) {   // a table that was not built is not published: its share of the budget goes back here, its memory as the exception leaves (as in odd_ensure)
            (void)hipStreamSynchronize(st); table_bytes_add(shared->device, -(int64_t)bytes);
            throw;
        }
        return (shared->wide[M0] = std::move(table)).as<ge_pniels>();           // (its bytes were reserved above)
    }
    PinBuf h_naf, h_qsteps;
    // odd multiples (2m+1) * 2^(j*L) * P of the original generators for the width-w NAF fold of the first group (k_fold_points_wnaf, scalars
    // cut into `fold_parts` pieces of L bits); built on first use for the device's generator tables and shared with them
    const ge_niels *gens_odd = nullptr;      // shared->odd[eff_wnaf | eff_parts << 8]: a view (nullptr: no table)
    uint32_t fold_wnaf = 5;          // width of the NAF the first fold recodes its scalars in (BPG_FOLD_WNAF; one-shot profile 5, serving 8; 0 = register kernels)
    uint32_t fold_parts = 2;         // the scalars of the first fold are cut into this many parts on tables of 2^(j*L) * P (BPG_FOLD_PARTS: 1, 2, 4 or 8; one-shot 2, serving 4)
    uint64_t fold_table_budget = 64ull << 30;       // per-kind cap of the fold tables (BPG_FOLD_TABLE_GB); the cumulative bound is table_budget
    uint32_t eff_wnaf = 0, eff_parts = 0;            // what odd_ensure settled on for the current capacity
    uint32_t fold_part_bits() const { return (254 + eff_parts - 1) / eff_parts; }
    // false: no table of any width fits the budget (or the device): the caller folds with the register kernels
    bool odd_ensure() {
        eff_wnaf = fold_wnaf; eff_parts = fold_parts;
        auto table_bytes = [&](uint32_t w, uint32_t parts) { return ((uint64_t)parts * (1u << (w - 2)) - 1) * 2 * gens_cap * sizeof(ge_niels); };
        auto smaller = [&]() { if (eff_parts > 1) { eff_parts /= 2; return true; } if (eff_wnaf > 3) { eff_wnaf--; return true; } return false; };
        std::lock_guard<std::mutex> lk(shared->m);
        DevBuf odd;
        for (;;) {   // the widest profile that is already built, or fits the budgets and the device (other tenants): the next smaller one otherwise
            const uint32_t key = eff_wnaf | (eff_parts << 8);
            auto it = shared->odd.find(key);
            if (it != shared->odd.end()) { gens_odd = it->second.as<ge_niels>(); return true; }
            const uint64_t bytes = table_bytes(eff_wnaf, eff_parts);
            if (bytes <= fold_table_budget && table_reserve(key, bytes)) {
                try { odd.ensure(bytes); break; }
                catch (const std::exception &) { (void)hipGetLastError(); table_bytes_add(shared->device, -(int64_t)bytes); shared->refused[key] = table_bytes_held(shared->device); }
            }
            if (!smaller()) { gens_odd = nullptr; return false; }
        }
        const uint32_t key_built = eff_wnaf | (eff_parts << 8);
        const uint32_t NM = 1u << (eff_wnaf - 2), cnt = (uint32_t)(2 * gens_cap), L = fold_part_bits();
        DevBuf dbl, base;
        try {
        scratch_ext.ensure((size_t)cnt * sizeof(ge_ext));
        dbl.ensure((size_t)cnt * sizeof(ge_ext));
        if (eff_parts > 1) base.ensure((size_t)cnt * sizeof(ge_ext));
        const dim3 grid(cdiv(cnt, 256)), ngrid(cdiv(cdiv(cnt, NORM_K), 256));
        for (uint32_t part = 0; part < eff_parts; part++) {
            ge_niels *tab0 = odd.as<ge_niels>() + ((ptrdiff_t)part * NM - 1) * (ptrdiff_t)cnt;          // table (part, m) = tab0 + m * cnt; (0, 0) is the generator table
            if (part == 0) BPG_LAUNCH((*this), k_odd_start, grid, dim3(256), gens, scratch_ext.as<ge_ext>(), dbl.as<ge_ext>(), cnt);
            else {
                BPG_LAUNCH((*this), k_dbl_times, grid, dim3(256), gens, base.as<ge_ext>(), cnt, L, part == 1 ? 1u : 0u);      // 2^(part*L) * P
                BPG_LAUNCH((*this), k_normalize_niels, ngrid, dim3(256), base.as<ge_ext>(), tab0, cnt);
                BPG_LAUNCH((*this), k_odd_start_ext, grid, dim3(256), base.as<ge_ext>(), scratch_ext.as<ge_ext>(), dbl.as<ge_ext>(), cnt);
            }
            for (uint32_t m = 1; m < NM; m++) {
                if (m > 1) BPG_LAUNCH((*this), k_odd_step, grid, dim3(256), scratch_ext.as<ge_ext>(), dbl.as<ge_ext>(), cnt);
                BPG_LAUNCH((*this), k_normalize_niels, ngrid, dim3(256), scratch_ext.as<ge_ext>(), tab0 + (size_t)m * cnt, cnt);
            }
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
        } catch (...) {   // a table that was not built is not published: its share of the budget goes back here, its memory as the exception leaves (after this wait)
            (void)hipStreamSynchronize(st); table_bytes_add(shared->device, -(int64_t)odd.cap);
            throw;
        }
        gens_odd = (shared->odd[key_built] = std::move(odd)).as<ge_niels>();    // (its bytes were reserved above)
        return true;
    }
    uint32_t fold_split_max = 65536; // folds with at most this many outputs use the 4-wave latency variant (BPG_FOLD_SPLIT overrides; 0 = never)
    uint32_t fold_adapt = 1;        // a proof that shares the device with others takes the register fold kernels throughout and sweeps in chunks of 64 (BPG_FOLD_ADAPT: 0 never, 1 when shared, 2 always)
    bool shared_variants() const { return fold_adapt == 2 || (fold_adapt == 1 && device_shared(shared->device)); }
    bool fold_quad = true;          // small folds: four lanes per output (BPG_FOLD_QUAD=0: the four-wave split kernel)
    bool fold_quad_w = true;        // ... with width-4 NAF against multiples the quads make themselves, in the groups after the first (BPG_FOLD_QUAD_W=0: plain NAF, addends in registers)
    bool fold_reg_w = true;         // the same steps with one lane per output where the register kernels would run (BPG_FOLD_REG_W=0: plain NAF, addends in registers)
    FoldKnobs fold_knobs() const {
        FoldKnobs k;
        k.fold_wnaf = fold_wnaf; k.fold_split_max = fold_split_max; k.fold_quad = fold_quad; k.fold_quad_w = fold_quad_w; k.fold_reg_w = fold_reg_w; k.shared = shared_now;
        return k;
    }
    bool window_quad = true;        // window sums of a proof alone: four lanes per point, several blocks per window (BPG_WINDOW_QUAD=0: k_window_sums always)
    uint32_t window_quad_blocks = 288;   // ... at most this many blocks of four waves per launch (about one wave per SIMD on 256 CUs; BPG_WINDOW_QUAD_BLOCKS)
    uint32_t fold_group = 3;        // rounds per generator fold (BPG_FOLD_GROUP overrides, 1..5)
    uint32_t tt_lg = 12;            // freeze the FOLDED generators once a round is down to 2^tt_lg per side: their window tables are built per proof (BPG_TT_LG; 0 = never)
    uint32_t tt_orig_lg = 14;       // a circuit of N <= 2^tt_orig_lg freezes the ORIGINAL generators at round 0: those tables are built once and also serve A_I, A_O, S
                                    // (BPG_TT_ORIG_LG; BPG_TT_LG sets both).  Measured at 2^20 (profiles/r03_tail_start.txt): 12 beats 14 alone and in flight
    uint32_t batch_wave_mb = 512;   // lockstep batches (prove_batch): device state of one wave at most this many MB (BPG_BATCH_WAVE_MB; 0 = one proof per wave)
    DevBuf bt_dev; PinBuf bt_pin;   // prove_batch: the wave's device buffers and its pinned upload / read-back area
    // prove_template_batch with commitments (k_bt_commit_v): commitments per wave of the kernel (1..4, a block makes four times as many).  4 measured
    // fastest at 3072 commitments (profiles/template_commit.json); BPG_COMMIT_CPW stays for that measurement only (tools/diag/template_commit.py), same bytes.
    // commit_ev: recorded behind the read-back of a wave's commitments, so that the host waits for them and not for the witness evaluation queued behind
    uint32_t commit_cpw = 4;
    Event commit_ev;
    PinBuf h_raw, h_small;
    // Speculative blinding streams (Engine::blinding_begin): the leading draws of Prover::prove's TranscriptRng, produced on the context's
    // chain worker (ONE host thread, FIFO) before the circuit is known - or, for a sequence of proofs, while the previous proof's kernels run.
    // snaps[k] = generator state before draw k * SNAP (after the three leading blinding scalars).  Up to two streams are alive per context
    // (the one being consumed and the next), each with its own pinned slab.
    using BlindStream = bpg::BlindStream;                    // host/chain.hpp: the stream, its worker loops and the publication protocol (no HIP in there)
    using ChainWorker = bpg::ChainWorker;
    std::shared_ptr<ChainWorker> chain;                     // the context's own worker, or the ChainPool it is attached to
    uint32_t pool_streams = 0;                              // attached to a pool: blinding streams this context may have alive
    uint32_t chain_workers = 1;                             // threads of the chain worker (bpg_ctx_set_chain_workers / BPG_CHAIN_WORKERS); alive streams <= workers * lanes + 1
    uint32_t chain_lanes = 1;                               // streams each thread draws in lockstep (bpg_ctx_set_chain_lanes / BPG_CHAIN_LANES, 1..8)
    std::deque<std::shared_ptr<BlindStream>> blinds;        // alive streams, oldest first
    std::vector<std::shared_ptr<BlindStream>> slab_owner;   // last stream that wrote each pinned slab (workers + 1 slabs)
    std::vector<PinBuf> h_blind;
    struct SlabDev { Stream copy_st; DevBuf d; std::vector<Event> ev; };                 // (the copy stream goes last)
    static hipEvent_t block_event(const BlindStream &bs, uint64_t k) { return (*static_cast<const std::vector<Event> *>(bs.ev))[k]; }      // BlindStream::ev is SlabDev::ev, opaque to host/chain.hpp
    std::vector<std::unique_ptr<SlabDev>> slab_dev;         // device side of each slab: the uploaded draws, the copy stream, one event per block
    int last_chain_cpu = -1;
    int test_fail_upload = 0;       // test hooks: 1 the next stream's upload reports an error, 2 its copies are silently dropped
    static void blind_stop(const std::shared_ptr<BlindStream> &b) {       // returns once the worker no longer touches b's slab
        b->stop.store(true, std::memory_order_relaxed);
    }
    void blind_retire(const std::shared_ptr<BlindStream> &b) {
        blind_stop(b);
        if (chain) {   // still queued (never started)?  take it out; else wait for the worker to leave it
            std::unique_lock<std::mutex> lk(chain->mu);
            for (auto it = chain->pending.begin(); it != chain->pending.end(); ++it) if (it->get() == b.get()) { chain->pending.erase(it); b->finished.store(true); break; }
        }
        while (!b->finished.load(std::memory_order_acquire)) std::this_thread::yield();
        const int c = b->cpu.load(std::memory_order_relaxed); if (c >= 0) last_chain_cpu = c;
    }
    // done with a stream inside prove(): its worker stops at the next snapshot, and the stream leaves the alive list
    void blind_release(const std::shared_ptr<BlindStream> &b) {
        blind_stop(b);
        for (auto it = blinds.begin(); it != blinds.end(); ++it) if (it->get() == b.get()) { blinds.erase(it); break; }
    }
    void blind_cancel() {
        while (!blinds.empty()) { blind_retire(blinds.front()); blinds.pop_front(); }
    }
    void chain_shutdown() {
        blind_cancel();
        if (!chain) return;
        if (!chain->pool) chain->stop();                    // a pool's threads go on serving the other contexts
        chain.reset(); pool_streams = 0;
    }
    uint64_t gens_cap = 0;
    // BPG_GENS_CACHE_DIR (see gens_cache_path): load = read + checksum + upload + compare 2 x 64 sampled points with points derived afresh from
    // the SHAKE256 stream (k_gens_derive on 128 generators); anything that does not agree falls back to the full derivation
    DevBuf gens_load_cached(const std::string &path, uint64_t cap);        // the table, or an empty buffer
    void adopt(const std::shared_ptr<SharedTables> &sp) { shared = sp; gens = sp->gens.as<ge_niels>(); gens_cap = sp->cap; gens_odd = nullptr; }
    void gens_store_cached(const std::string &path, uint64_t cap);

    // An MSM runs on the GPU down to its W window sums per result; those (W x 128 B) travel to a pinned slot and the serial recombination
    // sum_j 2^off(j) S_j (~254 dependent doublings of one point) and the point encoding run on the host (host/fe51.hpp).  msm() queues the
    // kernels and the copy and returns a ticket; msm_points() is called after the stream has been synchronised.
    struct MsmTicket { uint32_t slot, nmsm, W; };
    static constexpr uint32_t WS_SLOTS = 8, WS_SLOT_BYTES = (uint32_t)MSM_WS_SLOT_BYTES;
    PinBuf h_wsums; uint32_t ws_next = 0;
    MsmTicket msm(const MsmJob &J, uint32_t nmsm);
    MsmKnobs msm_knobs() const {
        MsmKnobs k;
        k.cmin = msm_cmin; k.cmax = msm_cmax; k.cmax_shared = msm_cmax_shared; k.rseg = rseg; k.lgch = lgch; k.sweep_blocks_resident = sweep_blocks_resident;
        k.window_quad = window_quad; k.window_quad_blocks = window_quad_blocks; k.shared = shared_now;
        return k;
    }
    MsmRun msm_last{};                                      // the plan of the last msm() call (host side only: read by the test hook Engine::test_msm after its stream sync, never on the proving path)
    DevBuf test_skip;                                       // skip bitmaps of Engine::test_msm
    DevBuf test_fold_tab;                                   // the folded table of Engine::test_fold (the prover's own go to ipa_tabA / ipa_tabB)
    std::vector<h51::pt> msm_points(const MsmTicket &t) const {
        std::vector<h51::pt> out(t.nmsm);
        const uint32_t *w = reinterpret_cast<const uint32_t *>(h_wsums.as<uint8_t>() + (size_t)t.slot * WS_SLOT_BYTES);
        for (uint32_t m = 0; m < t.nmsm; m++) out[m] = h51::pt_horner(w + (size_t)m * t.W * 32, t.W);
        return out;
    }
    // Host -> device copy of caller-owned pageable memory through two pinned bounce slots.  A direct hipMemcpyAsync from pageable memory
    // lets the runtime pin the caller's pages for the DMA; several contexts uploading the SAME arrays from different threads (a pool
    // proving many witnesses of one circuit) then pin and unpin the same pages concurrently, which faulted the GPU.
    PinBuf stage; Event stage_ev[2];
    void h2d(void *dst, const void *src, size_t bytes) {
        const size_t SLOT = 8u << 20;
        stage.ensure(2 * SLOT);
        for (int k = 0; k < 2; k++) if (!stage_ev[k]) stage_ev[k] = Event::untimed();
        const uint8_t *s8 = static_cast<const uint8_t *>(src); uint8_t *d8 = static_cast<uint8_t *>(dst);
        int slot = 0;
        for (size_t off = 0; off < bytes; off += SLOT, slot ^= 1) {
            const size_t len = std::min(SLOT, bytes - off);
            HIPCHK(hipEventSynchronize(stage_ev[slot]));                 // the previous copy out of this slot has finished
            std::memcpy(stage.as<uint8_t>() + (size_t)slot * SLOT, s8 + off, len);
            HIPCHK(hipMemcpyAsync(d8 + off, stage.as<uint8_t>() + (size_t)slot * SLOT, len, hipMemcpyHostToDevice, st));
            HIPCHK(hipEventRecord(stage_ev[slot], st));
        }
    }
    // base^i for i < count into out, for up to three tables in one launch
    struct PowTable { Scalar base; scm *out; uint64_t count; };
    void exp_tables(std::initializer_list<PowTable> tabs) {
        ExpTables E; std::memset(&E, 0, sizeof E);
        uint32_t k = 0, lgmax = 0;
        for (const PowTable &t : tabs) {
            const uint32_t lgT = std::min<uint32_t>(ceil_log2(t.count), 16);
            E.base[k] = to_scm(t.base); E.out[k] = t.out; E.count[k] = (uint32_t)t.count; E.lgT[k] = lgT; lgmax = std::max(lgmax, lgT); k++;
        }
        BPG_LAUNCH((*this), k_exp_table, dim3(cdiv(1u << lgmax, 256), k), dim3(256), E);
    }
    // flattened_constraints(z) of a resident circuit: z^j for j <= q into zpow, then w_L | w_R | w_O | w_V | w_c (3 n + m + 1 scalars) into w - k_flatten over the
    // variable columns, the grid-wide k_flatten_const reduction over the constant column into w[3 n + m].  beside: one more power table for the same launch
    // (the verifier's y^-i).  What verify_prep() runs, and what the test hook Engine::test_weights runs on a z of its caller's choosing.
    void flatten_weights(const DeviceCircuit *c, const Scalar &z, scm *zpow, scm *w, const PowTable *beside) {
        red_partial.ensure((size_t)4096 * sizeof(scm));                     // [0,1024): delta partials, [1024,1536): w_c partials
        if (beside) exp_tables({*beside, {z, zpow, c->q + 1}}); else exp_tables({{z, zpow, c->q + 1}});      // (y^-i,) z^j: one launch
        if (c->ncols > 1)
            BPG_LAUNCH((*this), k_flatten, dim3(cdiv(c->ncols - 1, 256)), dim3(256), c->col_ptr.as<uint64_t>(), c->ent_row.as<uint32_t>(), c->ent_coef.as<uint32_t>(),
                       c->coef.as<scm>(), zpow, w, (uint32_t)(c->ncols - 1), (uint32_t)(3 * c->n));
        // w_c: grid-wide reduction over the constant-term entries
        const uint64_t e0 = c->const_begin, e1 = c->nnz;
        const uint32_t cb = std::max<uint32_t>(1, std::min<uint32_t>(cdiv(e1 - e0, 256), 512));
        BPG_LAUNCH((*this), k_flatten_const, dim3(cb), dim3(256), c->ent_row.as<uint32_t>(), c->ent_coef.as<uint32_t>(), c->coef.as<scm>(), zpow, e0, e1,
                   red_partial.as<scm>() + 1024);
        BPG_LAUNCH((*this), k_reduce_partials, dim3(1), dim3(256), red_partial.as<scm>() + 1024, cb, 1u, w + c->ncols - 1);
    }
    struct CscWork { uint32_t *counts, *starts, *cursor, *rowconst, *rowconst_start, *bsum; };
    void transpose_csr(const uint64_t *rp, const uint32_t *tv, const uint32_t *tc, uint64_t q, uint64_t nmul, uint64_t m, const CscWork &W,
                       uint64_t *col_ptr, uint32_t *ent_row, uint32_t *ent_coef, uint32_t *totals);
    // The generator fold of one group, from the choice of the kernel to the normalised table in dst (2 * shape.Mr points: G side, then H side): what
    // inner_product() runs after the last round of a group, and what the test hook Engine::test_fold runs on scalars of its caller's choosing.
    struct FoldRun { FoldKernel kernel; int32_t top; uint32_t nsteps[2], tail[2]; };           // what was launched: top of the bitmap and width-w kernels, step counts of the step kernels
    FoldRun fold_launch(const FoldShape &shape, const FoldKernel *forced, uint64_t g_M, uint64_t n, const Scalar &u_ch, const std::vector<Scalar> &sG,
                       const std::vector<Scalar> &sH, const ge_niels *Gst, const ge_niels *Hst, ge_niels *dst);
    void inner_product(Transcript &T, std::vector<uint8_t> &proof, uint64_t n, uint64_t N, const Scalar &yinv, const Scalar &u_ch, const Scalar &w,
                       const ge_niels *Gtab, const ge_niels *Htab, const ge_niels *Bn, ProveTimings *tm, double &t0);
    // The table-driven tail of the inner-product argument (hip/k_ipa.cuh k_tt_*): what inner_product() runs from the round that freezes the generators, and what
    // the test hook Engine::test_tail runs on scalars of its caller's choosing.  tail_freeze: window tables of G[0..M0), H[0..M0), B (and the 8-bit ones of the
    // original generators where try_wide and the budget allow), the per-point factors, the first coefficient tables.  tail_round: sub-round S.j on a, b of mcur
    // values each - the previous challenge applied first (tail_advance) when j > 0 - with L and R encoded into lr.  tail_challenge: the challenge drawn from them.
    // tail_last_fold: after the last round only the scalar fold remains.
    struct TailState { uint32_t lgM0 = 0, j = 0, cur = 0; Scalar u, uinv; const ge_pniels *wide = nullptr; };
    static uint32_t tail_nblk(uint32_t M0) { return cdiv((uint64_t)M0 * 8, 256); }
    void tail_freeze(TailState &S, uint32_t M0, bool first, uint64_t n, const scm &uch_m, const Scalar &Gamma, const Scalar &Eta, const ge_niels *Gst,
                     const ge_niels *Hst, const ge_niels *Bn, bool original, bool try_wide);
    void tail_advance(TailState &S, scm *a, scm *b, uint64_t mcur);
    void tail_round(TailState &S, scm *a, scm *b, uint64_t mcur, const scm &w_m, uint32_t quad_sums, uint8_t lr[64]);
    void tail_challenge(TailState &S, const Scalar &u) { S.u = u; S.uinv = u.invert(); S.j++; }
    void tail_last_fold(const TailState &S, scm *a, scm *b, uint64_t h);
    // A_I, A_O, S of a circuit of n multipliers on the window tables of the original generators G[0..M0), H[0..M0) (tt_build(.., M0, true) went before), the three
    // blindings in extras[0..2]: k_tt_commit3 and its finish, encoded into pts.  prove() and the test hook Engine::test_commit3.
    static uint32_t commit3_nblk(uint32_t M0) { return cdiv((uint64_t)M0 * 16, 256); }
    void commit3(const scm *aL, const scm *aR, const scm *aO, const scm *sL, const scm *sR, uint64_t n, uint32_t M0, uint32_t quad_sums, uint8_t pts[96]);
};

// Environment knobs are read ONCE, here, before anything touches the device: a value that does not parse or lies outside its range is an error
// of the call that creates the context (std::invalid_argument -> BPG_ERR_INVALID_ARGUMENT), never a silent default and never a fault later on
// the hot path (round 3 read BPG_RSEG with atoi on every MSM call and divided by it).
namespace {
bool env_present(const char *name) { const char *e = std::getenv(name); return e && *e; }
long env_int_strict(const char *name, long lo, long hi) {
    const char *e = std::getenv(name);
    char *end = nullptr; errno = 0;
    const long v = std::strtol(e, &end, 10);
    if (errno || end == e || *end != '\0' || v < lo || v > hi)
        throw std::invalid_argument(std::string(name) + "=" + e + ": expected an integer in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return v;
}
double env_double_strict(const char *name, double lo, double hi) {
    const char *e = std::getenv(name);
    char *end = nullptr; errno = 0;
    const double v = std::strtod(e, &end);
    if (errno || end == e || *end != '\0' || !(v >= lo) || !(v <= hi))
        throw std::invalid_argument(std::string(name) + "=" + e + ": expected a number in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return v;
}
template <class T> void env_set(const char *name, long lo, long hi, T &out) { if (env_present(name)) out = (T)env_int_strict(name, lo, hi); }
}  // namespace

Engine::Engine(int device, const EngineConfig &cfg) : device_(device) {
    if (cfg.profile > 2) throw std::invalid_argument("bpg_config.profile: 0 (default), 1 (one-shot) or 2 (serving)");
    if (cfg.table_budget_gb < 0 || cfg.table_budget_gb > 4096) throw std::invalid_argument("bpg_config.table_budget_gb: 0 (default) .. 4096");
    if (cfg.chain_workers > 64) throw std::invalid_argument("bpg_config.chain_workers: 0 (default), 1..64");
    if (cfg.chain_lanes > 8) throw std::invalid_argument("bpg_config.chain_lanes: 0 (default), 1..8");
    if (cfg.blocking_sync < -1 || cfg.blocking_sync > 2) throw std::invalid_argument("bpg_config.blocking_sync: -1 (environment, else spin), 0 (spin), 1 (blocking)");
    // What the host chose (bpg_config): the struct first, then the environment variable, then the profile's default.  Everything is settled
    // in this local Impl before the first HIP call, so a bad knob costs nothing and leaks nothing.
    std::unique_ptr<Impl> K(new Impl());
    K->device = device;
    int blocking = cfg.blocking_sync == 2 ? 0 : cfg.blocking_sync;          // -1 unset, 0 spin, 1 blocking (2: what one header revision called spin)
    if (blocking < 0 && env_present("BPG_SYNC_BLOCKING")) blocking = env_int_strict("BPG_SYNC_BLOCKING", 0, 1) ? 1 : 0;
    uint32_t profile = cfg.profile;
    if (profile == 0) { if (const char *e = std::getenv("BPG_PROFILE")) profile = (!std::strcmp(e, "serving") || !std::strcmp(e, "2")) ? 2u : 1u; else profile = 1u; }
    // one-shot (the default of a bare bpg_ctx_create): width-5 NAF fold tables on scalars cut in two (15 tables, 3.0 GB at 2^20; round 5: the same bytes as the
    // width-6 tables of whole scalars it replaces, 127 doublings instead of 253 for 42 instead of 36 additions per scalar: the first fold 5.6 -> 5.0 ms), no 8-bit
    // tail tables, 4 GB of tables in all; serving: width-8 NAF on scalars cut in four (51.5 GB at 2^20, 0.12 s), 8-bit tail tables (17.2 GB at 2^14), 96 GB
    if (profile == 2) { K->fold_wnaf = 8; K->fold_parts = 4; K->tt_wide_budget = 24ull << 30; K->table_budget = 96ull << 30; }
    else { K->fold_wnaf = 5; K->fold_parts = 2; K->tt_wide_budget = 0; K->table_budget = 4ull << 30; }
    K->profile = profile;
    {
        double gb = cfg.table_budget_gb;
        if (!(gb > 0) && env_present("BPG_TABLE_GB")) gb = env_double_strict("BPG_TABLE_GB", 0.0, 4096.0);
        if (gb > 0) K->table_budget = (uint64_t)(gb * (double)(1ull << 30));
    }
    K->chain_workers = cfg.chain_workers ? cfg.chain_workers : 1u; if (!cfg.chain_workers) env_set("BPG_CHAIN_WORKERS", 1, 64, K->chain_workers);
    K->chain_lanes = cfg.chain_lanes ? cfg.chain_lanes : 1u; if (!cfg.chain_lanes) env_set("BPG_CHAIN_LANES", 1, 8, K->chain_lanes);
    K->gens_cache_dir = cfg.gens_cache_dir;
    if (K->gens_cache_dir.empty()) { if (const char *e = std::getenv("BPG_GENS_CACHE_DIR")) K->gens_cache_dir = e; }
    // tuning knobs (diagnostics and the schedule tests; every setting gives the same bytes)
    if (env_present("BPG_MSM_CMAX")) K->msm_cmax = K->msm_cmax_shared = (uint32_t)env_int_strict("BPG_MSM_CMAX", 4, 16);
    env_set("BPG_MSM_CMIN", 2, 16, K->msm_cmin);
    env_set("BPG_MERGE", 0, 2, K->merge_equal);
    bool resident_set = false;
    if (env_present("BPG_SWEEP_RESIDENT")) { K->sweep_blocks_resident = (uint32_t)env_int_strict("BPG_SWEEP_RESIDENT", 64, 65536); resident_set = true; }
    if (env_present("BPG_RSEG")) {
        const long v = env_int_strict("BPG_RSEG", 1, 1024);
        if (v & (v - 1)) throw std::invalid_argument("BPG_RSEG: the segment length of the bucket reduction is a power of two in [1, 1024]");
        K->rseg = (uint32_t)v;
    }
    env_set("BPG_LGCH", 2, 10, K->lgch);
    env_set("BPG_FOLD_SPLIT", 0, 1 << 24, K->fold_split_max);
    if (env_present("BPG_FOLD_QUAD")) K->fold_quad = env_int_strict("BPG_FOLD_QUAD", 0, 1) != 0;
    if (env_present("BPG_FOLD_QUAD_W")) K->fold_quad_w = env_int_strict("BPG_FOLD_QUAD_W", 0, 1) != 0;
    if (env_present("BPG_FOLD_REG_W")) K->fold_reg_w = env_int_strict("BPG_FOLD_REG_W", 0, 1) != 0;
    if (env_present("BPG_WINDOW_QUAD")) K->window_quad = env_int_strict("BPG_WINDOW_QUAD", 0, 1) != 0;
    env_set("BPG_WINDOW_QUAD_BLOCKS", 1, 65536, K->window_quad_blocks);
    env_set("BPG_FOLD_ADAPT", 0, 2, K->fold_adapt);
    env_set("BPG_FOLD_GROUP", 1, 5, K->fold_group);
    if (env_present("BPG_TT_WIDE_GB")) K->tt_wide_budget = (uint64_t)(env_double_strict("BPG_TT_WIDE_GB", 0.0, 4096.0) * (double)(1ull << 30));
    if (env_present("BPG_FOLD_TABLE_GB")) K->fold_table_budget = (uint64_t)(env_double_strict("BPG_FOLD_TABLE_GB", 0.0, 4096.0) * (double)(1ull << 30));
    if (env_present("BPG_FOLD_PARTS")) { const long v = env_int_strict("BPG_FOLD_PARTS", 1, 8); if (v & (v - 1)) throw std::invalid_argument("BPG_FOLD_PARTS: 1, 2, 4 or 8"); K->fold_parts = (uint32_t)v; }
    if (env_present("BPG_FOLD_WNAF")) { const long v = env_int_strict("BPG_FOLD_WNAF", 0, 8); if (v == 1 || v == 2) throw std::invalid_argument("BPG_FOLD_WNAF: 0 (register kernels) or 3..8"); K->fold_wnaf = (uint32_t)v; }
    if (env_present("BPG_TT_LG")) K->tt_lg = K->tt_orig_lg = (uint32_t)env_int_strict("BPG_TT_LG", 0, 20);
    env_set("BPG_TT_ORIG_LG", 0, 20, K->tt_orig_lg);
    env_set("BPG_BATCH_WAVE_MB", 0, 1 << 20, K->batch_wave_mb);
    env_set("BPG_COMMIT_CPW", 1, 4, K->commit_cpw);
    env_set("BPG_CHECK_THRESHOLD", 0, 1 << 20, K->check_threshold);
    if (env_present("BPG_GENS_SHARE")) K->gens_share = env_int_strict("BPG_GENS_SHARE", 0, 1) != 0;

    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) throw DeviceError("no HIP device available: the bpg engine has no CPU path");
    if (device < 0 || device >= count) throw DeviceError("invalid device ordinal");
    HIPCHK(hipSetDevice(device));
    if (blocking == 1) { (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync); (void)hipGetLastError(); K->blocking_waits = true; }
    {   // blocks of the sweep the device holds at once: 4 per CU of THIS device (a partitioned MI355X shows fewer CUs); blocks of k_window_sums_quad per launch: one
        // wave per SIMD and an eighth more (288 on 256 CUs)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) {
            if (!resident_set) K->sweep_blocks_resident = (uint32_t)cus * 4u;
            K->wit_waves = (uint32_t)cus * 4u;
            K->cu_count = (uint32_t)cus;
            if (!env_present("BPG_WINDOW_QUAD_BLOCKS")) K->window_quad_blocks = (uint32_t)cus + (uint32_t)cus / 8u;
        }
    }
    impl_ = K.get();
    try { init_device(); } catch (...) { impl_ = nullptr; throw; }        // K still owns the Impl: what init_device() had allocated goes with it
    K.release();
}

void Engine::init_device() {
    impl_->st = Stream::blocking();
    stream_ = (hipStream_t)impl_->st;
    // Pedersen bases: B_blinding = from_uniform(SHA3-512(compress(B)))  (PedersenGens::default, reference src/bin/prover.rs:53)
    static const uint8_t Bc[32] = {0xe2, 0xf2, 0xae, 0x0a, 0x6a, 0xbc, 0x4e, 0x71, 0xa8, 0x84, 0xa9, 0x61, 0xc5, 0x00, 0x51, 0x5f,
                                   0x58, 0xe3, 0x0b, 0x6a, 0xa5, 0x82, 0xdd, 0x8d, 0xb6, 0xa6, 0x59, 0x45, 0xe0, 0x8d, 0x2d, 0x76};
    uint8_t h[64]; sha3_512_host(h, Bc, 32);
    impl_->small_in.ensure(4096); impl_->bases.ensure(3 * sizeof(ge_niels));
    impl_->stale_flag.ensure(64); HIPCHK(hipMemsetAsync(impl_->stale_flag.p, 0, 64, impl_->st));
    HIPCHK(hipMemcpyAsync(impl_->small_in.p, h, 64, hipMemcpyHostToDevice, impl_->st));
    hipLaunchKernelGGL(k_init_bases, dim3(1), dim3(64), 0, impl_->st, impl_->small_in.as<uint32_t>(), impl_->bases.as<ge_niels>());
    HIPCHK(hipGetLastError());
    // window tables of B and B_blinding for k_pedersen (64 windows x 8 multiples each, 128 KB)
    impl_->tt_bases.ensure((size_t)3 * TT_WINDOWS * sizeof(ge_ext));
    impl_->ped_table.ensure((size_t)3 * TT_WINDOWS * TT_MULTS * sizeof(ge_pniels));
    hipLaunchKernelGGL(k_tt_bases, dim3(1), dim3(256), 0, impl_->st, impl_->bases.as<ge_niels>(), impl_->bases.as<ge_niels>() + 1, impl_->bases.as<ge_niels>(),
                       impl_->tt_bases.as<ge_ext>(), 1u);
    hipLaunchKernelGGL(k_tt_multiples, dim3(cdiv(3 * TT_WINDOWS, 256)), dim3(256), 0, impl_->st, impl_->tt_bases.as<ge_ext>(), impl_->ped_table.as<ge_pniels>(),
                       (uint32_t)(3 * TT_WINDOWS));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(impl_->st));
}

Engine::~Engine() { delete impl_; }
// order: (1) no host thread of ours issues work for this context any more (the chain threads have left its streams), (2) everything this
// context queued has finished - the engine stream AND the slabs' copy streams, whose uploads read the pinned slabs - (3) only then memory goes:
// the trees the host has not freed lose theirs here (their handles stay valid), the members free themselves in reverse order of declaration - the
// generator tables and the MiMC constants with their last context - and the engine stream, the first member, goes last
Engine::Impl::~Impl() {
    chain_shutdown();
    if (!st) return;                            // the constructor failed before init_device(): nothing of this context is on a device
    (void)hipSetDevice(device);
    (void)hipStreamSynchronize(st);
    for (auto &sd : slab_dev) if (sd->copy_st) (void)hipStreamSynchronize(sd->copy_st);
    for (DeviceMerkle *t : trees) merkle_orphan(t);
}

void live_resources(uint64_t out[6]) { for (int k = 0; k < LIVE_COUNT; k++) out[k] = g_live[k].load(std::memory_order_relaxed); }
int Engine::device_count() { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; } return n; }
void Engine::profile_set(int mode) { HIPCHK(hipSetDevice(device_)); impl_->prof_reset(); impl_->prof_mode = mode; }
std::string Engine::profile_report() {
    HIPCHK(hipSetDevice(device_));
    impl_->prof_collect();
    // the effective schedule of this context first (what the knobs, the profile and the table budget settled on): bench.py derives its term
    // counts from THIS, not from its own reading of the environment
    char sch[1024];
    std::snprintf(sch, sizeof sch, "{\"_schedule\": {\"profile\": %u, \"tt_lg\": %u, \"tt_orig_lg\": %u, \"fold_group\": %u, \"fold_wnaf\": %u, \"fold_parts\": %u, "
                  "\"eff_wnaf\": %u, \"eff_parts\": %u, \"fold_adapt\": %u, \"fold_split_max\": %u, \"fold_quad\": %u, \"msm_cmax\": %u, \"msm_cmax_shared\": %u, \"msm_cmin\": %u, "
                  "\"rseg\": %u, \"lgch\": %u, \"sweep_blocks_resident\": %u, \"shared_variants_last\": %u, \"merge_equal\": %u, \"merged_last\": %u, \"merged_skipped_last\": %u, \"merge_ms_last\": %.3f, \"table_budget\": %llu, \"table_bytes\": %llu, \"check_threshold\": %u}",
                  impl_->profile, impl_->tt_lg, impl_->tt_orig_lg, impl_->fold_group, impl_->fold_wnaf, impl_->fold_parts, impl_->eff_wnaf, impl_->eff_parts,
                  impl_->fold_adapt, impl_->fold_split_max, (unsigned)impl_->fold_quad, impl_->msm_cmax, impl_->msm_cmax_shared, impl_->msm_cmin, impl_->rseg, impl_->lgch,
                  impl_->sweep_blocks_resident, (unsigned)impl_->shared_now, (unsigned)impl_->merge_equal, impl_->merged_last, impl_->merged_skipped_last, impl_->merge_ms_last, (unsigned long long)impl_->table_budget, (unsigned long long)table_bytes_held(device_), impl_->check_threshold);
    std::string out = sch;
    if (!impl_->prof_wit_ms.empty()) {
        out += ", \"_witness_launch_ms\": [";
        for (size_t i = 0; i < impl_->prof_wit_ms.size(); i++) { char b[32]; std::snprintf(b, sizeof b, "%s%.4f", i ? "," : "", impl_->prof_wit_ms[i]); out += b; }
        out += "]";
    }
    if (!impl_->prof_merkle_ms.empty()) {
        out += ", \"_merkle_launch_ms\": [";
        for (size_t i = 0; i < impl_->prof_merkle_ms.size(); i++) {
            char b[64]; std::snprintf(b, sizeof b, "%s[\"%s\", %.4f]", i ? "," : "", kKernelNames[impl_->prof_merkle_ms[i].first], impl_->prof_merkle_ms[i].second); out += b;
        }
        out += "]";
    }
    bool first = false;
    for (int i = 0; i < KID_COUNT; i++) {
        if (!impl_->prof_count[i]) continue;
        char buf[512];
        std::snprintf(buf, sizeof buf, "%s\"%s\": {\"count\": %llu, \"total_ms\": %.6f, \"alg_bytes\": %.0f, \"device_bytes\": %.0f, \"field_mults\": %.0f}",
                      first ? "" : ", ", kKernelNames[i], (unsigned long long)impl_->prof_count[i], impl_->prof_ms[i], impl_->prof_alg_bytes[i],
                      impl_->prof_act_bytes[i], impl_->prof_fm[i]);
        out += buf; first = false;
    }
    return out + "}";
}
// throughput of dependent-free field multiplications (the binding roofline of this path): returns multiplications / second
double Engine::bench_fe_mul(uint32_t iters) {
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint32_t blocks = 256 * 16, threads = 256;
    I.small_sc.ensure((size_t)blocks * threads * sizeof(fe));
    const Event a = Event::timed(), b = Event::timed();
    hipLaunchKernelGGL(k_bench_fe_mul, dim3(blocks), dim3(threads), 0, I.st, I.small_sc.as<fe>(), 8u);     // warm-up
    HIPCHK(hipEventRecord(a, I.st));
    hipLaunchKernelGGL(k_bench_fe_mul, dim3(blocks), dim3(threads), 0, I.st, I.small_sc.as<fe>(), iters);
    HIPCHK(hipEventRecord(b, I.st));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(b));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, a, b));
    return (double)blocks * threads * iters * 4.0 / (ms * 1e-3);
}

void Engine::test_fe_ops(int op, size_t n, const uint8_t *a, const uint8_t *b, uint8_t *out) {
    if (!n) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.small_sc.ensure(2 * n * 32); I.comp.ensure(n * 32);
    HIPCHK(hipMemcpyAsync(I.small_sc.p, a, n * 32, hipMemcpyHostToDevice, I.st));
    HIPCHK(hipMemcpyAsync(I.small_sc.as<uint8_t>() + n * 32, b, n * 32, hipMemcpyHostToDevice, I.st));
    hipLaunchKernelGGL(k_test_fe, dim3(cdiv(n, 64)), dim3(64), 0, I.st, I.small_sc.as<uint32_t>(), I.small_sc.as<uint32_t>() + 8 * n, I.comp.as<uint8_t>(), (uint32_t)n, (uint32_t)op);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, I.comp.p, n * 32, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
}

// bpg_test_decompress: k_decompress as verify() launches it; the affine x, y of every entry recovered on the host from the halved Niels form
void Engine::test_decompress(size_t n, const uint8_t *in, uint32_t *ok_out, uint8_t *xy_out) {
    if (!n) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.vfy_in.ensure(n * 32); I.vfy_pts.ensure(n * sizeof(ge_niels)); I.vfy_ok.ensure(n * 4);
    HIPCHK(hipMemcpyAsync(I.vfy_in.p, in, n * 32, hipMemcpyHostToDevice, I.st));
    BPG_LAUNCH(I, k_decompress, dim3(cdiv(n, 64)), dim3(64), I.vfy_in.as<uint8_t>(), I.vfy_pts.as<ge_niels>(), I.vfy_ok.as<uint32_t>(), (uint32_t)n);
    HIPCHK(hipGetLastError());
    std::vector<ge_niels> pts(n);
    HIPCHK(hipMemcpyAsync(pts.data(), I.vfy_pts.p, n * sizeof(ge_niels), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(ok_out, I.vfy_ok.p, n * 4, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    for (size_t i = 0; i < n; i++) {
        const h51::fe51 ypx = h51::fe_from_words(pts[i].ypx.v), ymx = h51::fe_from_words(pts[i].ymx.v);
        h51::fe_tobytes(xy_out + 64 * i, h51::fe_sub(ypx, ymx));
        h51::fe_tobytes(xy_out + 64 * i + 32, h51::fe_add(ypx, ymx));
    }
}

void Engine::synchronize() { HIPCHK(hipSetDevice(device_)); HIPCHK(hipStreamSynchronize(impl_->st)); }

// ------------------------------------------------------------------------------------------------ generators
void Engine::gens_ensure(uint64_t capacity) {
    if (capacity == 0 || (capacity & (capacity - 1))) throw std::invalid_argument("generator capacity must be a power of two");
    if (capacity > (1ULL << 24)) throw std::invalid_argument("generator capacity above 2^24 is not supported");
    if (capacity <= gens_cap_) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    // GeneratorsChain: SHAKE256("GeneratorsChain" || 'G'|'H' || u32le(party = 0)), 64 bytes per generator (host squeeze,
    // a serial XOF), then 2*capacity Elligator maps + one batched normalisation on the device.
    const uint64_t cap = capacity;
    std::lock_guard<std::mutex> tables_lock(g_tables_mutex);
    const bool share = I.gens_share;
    if (share) {   // another context of this device already holds tables of this capacity: adopt them
        auto it = g_tables.find({device_, cap});
        if (it != g_tables.end()) {
            if (std::shared_ptr<SharedTables> sp = it->second.lock()) { I.adopt(sp); gens_cap_ = cap; return; }
            g_tables.erase(it);
        }
    }
    auto publish = [&](DevBuf fresh) {
        auto sp = std::make_shared<SharedTables>();
        sp->device = device_; sp->cap = cap; sp->gens = std::move(fresh);
        if (share) g_tables[{device_, cap}] = sp;
        I.adopt(sp); gens_cap_ = cap;
    };
    const std::string cache_file = gens_cache_path(I.gens_cache_dir, cap);
    const bool cache_ok = !cache_file.empty() && gens_cache_trusted(I.gens_cache_dir, cache_file);       // else: derive, never read or write the cache
    if (cache_ok) { DevBuf loaded = I.gens_load_cached(cache_file, cap); if (loaded.p) { publish(std::move(loaded)); return; } }
    I.h_raw.ensure(2 * cap * 64);
    {   // the two chains are independent XOF streams: squeeze them on two threads; the streams are prefixes of one another across
        // capacities, so a process-wide cache keeps the longest one squeezed so far (contexts of a batch share it)
        struct Chain { Shake256 sh; std::vector<uint8_t> bytes; bool started = false; };
        static Chain chains[2];
        static std::mutex chain_mutex;
        std::lock_guard<std::mutex> lock(chain_mutex);
        auto extend = [&](int which) {
            Chain &c = chains[which];
            if (!c.started) {
                const uint8_t label[5] = {(uint8_t)(which ? 'H' : 'G'), 0, 0, 0, 0};
                c.sh.absorb(reinterpret_cast<const uint8_t *>("GeneratorsChain"), 15);
                c.sh.absorb(label, 5);
                c.started = true;
            }
            const size_t have = c.bytes.size(), want = (size_t)cap * 64;
            if (want > have) { c.bytes.resize(want); c.sh.squeeze(c.bytes.data() + have, want - have); }
        };
        (void)keccak_impl();                                  // calibrate once before the threads start
        std::thread th([&] { extend(1); });
        extend(0);
        th.join();
        for (int which = 0; which < 2; which++) std::memcpy(I.h_raw.as<uint8_t>() + (size_t)which * cap * 64, chains[which].bytes.data(), (size_t)cap * 64);
    }
    I.raw_rng.ensure(2 * cap * 64);
    I.scratch_ext.ensure(2 * cap * sizeof(ge_ext));
    DevBuf fresh; fresh.ensure(2 * cap * sizeof(ge_niels));
    HIPCHK(hipMemcpyAsync(I.raw_rng.p, I.h_raw.p, 2 * cap * 64, hipMemcpyHostToDevice, I.st));
    const uint32_t cnt = (uint32_t)(2 * cap);
    BPG_LAUNCH(I, k_gens_derive, dim3(cdiv(cnt, 256)), dim3(256), I.raw_rng.as<uint32_t>(), I.scratch_ext.as<ge_ext>(), cnt);
    BPG_LAUNCH(I, k_normalize_niels, dim3(cdiv(cdiv(cnt, NORM_K), 256)), dim3(256), I.scratch_ext.as<ge_ext>(), fresh.as<ge_niels>(), cnt);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
    publish(std::move(fresh));
    I.raw_rng.release(); I.scratch_ext.release(); I.h_raw.release();      // one-off derivation buffers (0.4 GB of device memory at 2^20); the prove path sizes its own
    if (cache_ok) I.gens_store_cached(cache_file, cap);
}

DevBuf Engine::Impl::gens_load_cached(const std::string &path, uint64_t cap) {
    const int fd = ::open(path.c_str(), O_RDONLY | O_NOFOLLOW | O_CLOEXEC);
    FILE *f = fd >= 0 ? ::fdopen(fd, "rb") : nullptr;
    if (!f) { if (fd >= 0) ::close(fd); return DevBuf(); }
    const size_t bytes = (size_t)2 * cap * sizeof(ge_niels);
    GensCacheHeader hd;
    bool ok = std::fread(&hd, sizeof hd, 1, f) == 1 && std::memcmp(hd.magic, kGensMagic, 8) == 0 && hd.version == 2 && hd.capacity == cap && hd.bytes == bytes;
    PinBuf host;
    if (ok) { host.ensure(bytes); ok = std::fread(host.p, 1, bytes, f) == bytes && std::fgetc(f) == EOF; }
    std::fclose(f);
    if (ok) ok = gens_checksum(host.as<uint8_t>(), bytes) == hd.checksum;
    if (!ok) return DevBuf();
    DevBuf fresh; fresh.ensure(bytes);
    HIPCHK(hipMemcpyAsync(fresh.p, host.p, bytes, hipMemcpyHostToDevice, st));
    // sample: the first 64 generators of G and of H, derived afresh (the head of each SHAKE256 chain: 4 KB) and normalised the usual way
    const uint32_t SAMPLE = (uint32_t)std::min<uint64_t>(64, cap);
    uint8_t raw[2 * 64 * 64];
    for (int which = 0; which < 2; which++) {
        Shake256 sh; const uint8_t label[5] = {(uint8_t)(which ? 'H' : 'G'), 0, 0, 0, 0};
        sh.absorb(reinterpret_cast<const uint8_t *>("GeneratorsChain"), 15); sh.absorb(label, 5);
        sh.squeeze(raw + (size_t)which * SAMPLE * 64, (size_t)SAMPLE * 64);
    }
    small_in.ensure(sizeof raw); scratch_ext.ensure((size_t)2 * SAMPLE * sizeof(ge_ext)); comp.ensure((size_t)4 * SAMPLE * 32);
    DevBuf smp; smp.ensure((size_t)2 * SAMPLE * sizeof(ge_niels));
    HIPCHK(hipMemcpyAsync(small_in.p, raw, (size_t)2 * SAMPLE * 64, hipMemcpyHostToDevice, st));
    BPG_LAUNCH((*this), k_gens_derive, dim3(cdiv(2 * SAMPLE, 256)), dim3(256), small_in.as<uint32_t>(), scratch_ext.as<ge_ext>(), 2 * SAMPLE);
    BPG_LAUNCH((*this), k_normalize_niels, dim3(1), dim3(256), scratch_ext.as<ge_ext>(), smp.as<ge_niels>(), 2 * SAMPLE);
    // compare encodings (the affine Niels form is unique up to the representative of each coordinate; the encoding is canonical)
    BPG_LAUNCH((*this), k_compress_niels, dim3(cdiv(SAMPLE, 64)), dim3(64), smp.as<ge_niels>(), comp.as<uint8_t>(), SAMPLE);
    BPG_LAUNCH((*this), k_compress_niels, dim3(cdiv(SAMPLE, 64)), dim3(64), smp.as<ge_niels>() + SAMPLE, comp.as<uint8_t>() + 32 * SAMPLE, SAMPLE);
    BPG_LAUNCH((*this), k_compress_niels, dim3(cdiv(SAMPLE, 64)), dim3(64), fresh.as<ge_niels>(), comp.as<uint8_t>() + 64 * SAMPLE, SAMPLE);
    BPG_LAUNCH((*this), k_compress_niels, dim3(cdiv(SAMPLE, 64)), dim3(64), fresh.as<ge_niels>() + cap, comp.as<uint8_t>() + 96 * SAMPLE, SAMPLE);
    HIPCHK(hipGetLastError());
    std::vector<uint8_t> enc((size_t)4 * SAMPLE * 32);
    HIPCHK(hipMemcpyAsync(enc.data(), comp.p, enc.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (std::memcmp(enc.data(), enc.data() + (size_t)2 * SAMPLE * 32, (size_t)2 * SAMPLE * 32) != 0) return DevBuf();
    return fresh;
}
void Engine::Impl::gens_store_cached(const std::string &path, uint64_t cap) {
    const size_t bytes = (size_t)2 * cap * sizeof(ge_niels);
    std::vector<uint8_t> host(bytes);
    HIPCHK(hipMemcpyAsync(host.data(), gens, bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    GensCacheHeader hd; std::memcpy(hd.magic, kGensMagic, 8); hd.version = 2; hd.capacity = cap; hd.bytes = bytes; hd.checksum = gens_checksum(host.data(), bytes);
    std::string tmp = path + ".tmp.XXXXXX";
    const int fd = ::mkstemp(&tmp[0]);                          // O_CREAT | O_EXCL, mode 0600, never through a symbolic link
    FILE *f = fd >= 0 ? ::fdopen(fd, "wb") : nullptr;
    if (!f) { if (fd >= 0) { ::close(fd); std::remove(tmp.c_str()); } return; }      // a cache that cannot be written is not an error
    const bool ok = std::fwrite(&hd, sizeof hd, 1, f) == 1 && std::fwrite(host.data(), 1, bytes, f) == bytes;
    if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) std::remove(tmp.c_str());
}

void Engine::gens_export(uint64_t first, uint64_t count, uint8_t *G_out, uint8_t *H_out) {
    if (first + count > gens_cap_) throw std::invalid_argument("gens_export: range beyond capacity");
    if (!count) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.comp.ensure(count * 32);
    for (int which = 0; which < 2; which++) {
        const ge_niels *src = I.gens + (which ? gens_cap_ : 0) + first;
        BPG_LAUNCH(I, k_compress_niels, dim3(cdiv(count, 64)), dim3(64), src, I.comp.as<uint8_t>(), (uint32_t)count);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(which ? H_out : G_out, I.comp.p, count * 32, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipStreamSynchronize(I.st));
    }
}

void Engine::pedersen_bases(uint8_t B[32], uint8_t Bb[32]) {
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.comp.ensure(64);
    BPG_LAUNCH(I, k_compress_niels, dim3(1), dim3(64), I.bases.as<ge_niels>(), I.comp.as<uint8_t>(), 2u);
    HIPCHK(hipGetLastError());
    uint8_t out[64];
    HIPCHK(hipMemcpyAsync(out, I.comp.p, 64, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    std::memcpy(B, out, 32); std::memcpy(Bb, out + 32, 32);
}

void Engine::pedersen_commit(size_t k, const uint8_t *v, const uint8_t *blind, uint8_t *out) {
    if (!k) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    // v: keep the caller's 255-bit integer (from_bits semantics); blind: reduce on the host so that bit 255 never matters
    std::vector<uint8_t> hv(k * 32), hr(k * 32);
    for (size_t i = 0; i < k; i++) {
        Scalar a = Scalar::from_bits(v + 32 * i); a.to_bytes(&hv[32 * i]);
        Scalar b = Scalar::from_bytes_mod_order(blind + 32 * i); b.to_bytes(&hr[32 * i]);
    }
    I.small_sc.ensure(2 * k * 32); I.comp.ensure(k * 32);
    HIPCHK(hipMemcpyAsync(I.small_sc.p, hv.data(), k * 32, hipMemcpyHostToDevice, I.st));
    HIPCHK(hipMemcpyAsync(I.small_sc.as<uint8_t>() + k * 32, hr.data(), k * 32, hipMemcpyHostToDevice, I.st));
    BPG_LAUNCH(I, k_pedersen, dim3((uint32_t)k), dim3(64), I.small_sc.as<uint32_t>(), I.small_sc.as<uint32_t>() + k * 8,
                       I.ped_table.as<ge_pniels>(), I.comp.as<uint8_t>(), (uint32_t)k);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, I.comp.p, k * 32, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
}

// ------------------------------------------------------------------------------------------------ MSM pipeline
// plan (host/msm_plan.hpp: every choice and every size), size the workspace from the plan, launch from the plan, ticket
Engine::Impl::MsmTicket Engine::Impl::msm(const MsmJob &J, uint32_t nmsm) {
    const MsmSegs &S = J.S;
    const MsmRun R = plan_msm(MsmShape{S.nseg, S.len, S.msm, nmsm, J.skipped}, msm_knobs());
    const MsmPlan &P = R.P;
    const uint32_t total = R.total, W = P.W, nkeys = R.nkeys, nchunks = R.nchunks, CH = R.CH;
    msm_last = R;
    starts.ensure(R.bytes_starts);
    buckets.ensure(R.bytes_buckets);
    partial.ensure(R.bytes_partial);
    arena.ensure(R.b_front + R.b_entries);
    uint16_t *digits_p = reinterpret_cast<uint16_t *>(arena_at(0));
    uint32_t *entries1_p = reinterpret_cast<uint32_t *>(arena_at(R.b_digits)), *entries_p = reinterpret_cast<uint32_t *>(arena_at(R.b_front));
    ge_ext *slotA = reinterpret_cast<ge_ext *>(arena_at(0)), *slotB = slotA + nchunks;
    heavy.ensure(R.bytes_heavy); medium.ensure(R.bytes_medium);
    counts.ensure(R.bytes_counts); starts1.ensure(R.bytes_counts); cursor.ensure(R.bytes_counts);
    blocksum.ensure(R.bytes_blocksum);
    // (kernels.cuh, "two-level sort"): digits once, coarse partition with coalesced runs, fine counting sort inside each coarse bin
    HIPCHK(hipMemsetAsync(counts.p, 0, (size_t)R.nflat * 4, st));        // tiles an MSM does not have (tmax is the longest MSM's count)
    BPG_LAUNCH_LDS((*this), KID_k_msm_digits, k_msm_digits, dim3(R.ntiles ? R.ntiles : 1), dim3(512), R.lds_digits, S, P, total, digits_p, counts.as<uint32_t>(), heavy.as<uint32_t>(), medium.as<uint32_t>());
    BPG_LAUNCH((*this), k_scan_blocksums, dim3(R.nblk1), dim3(256), counts.as<uint32_t>(), R.nflat, blocksum.as<uint32_t>());
    BPG_LAUNCH((*this), k_scan_apply, dim3(R.nblk1), dim3(256), counts.as<uint32_t>(), R.nflat, blocksum.as<uint32_t>(), starts1.as<uint32_t>(), cursor.as<uint32_t>());
    if (R.ntiles) BPG_LAUNCH((*this), k_msm_scatter1, dim3(R.ntiles, W), dim3(256), S, P, digits_p, total, starts1.as<uint32_t>(), entries1_p);
    BPG_LAUNCH((*this), k_msm_sort2, dim3(R.K), dim3(256), P, starts1.as<uint32_t>(), R.nflat, entries1_p, starts.as<uint32_t>(), entries_p);
    open_keys.ensure(R.bytes_open_keys);
    // the true entry count is starts[nkeys] (device side); threads past it exit immediately
    BPG_LAUNCH((*this), k_bucket_chunks, dim3(cdiv(nchunks, 256)), dim3(256), S, starts.as<uint32_t>(), entries_p,
               buckets.as<ge_ext>(), slotA, slotB, open_keys.as<uint32_t>(), nkeys, CH);
    // roofline bookkeeping.  Algorithmic bytes: the information content of the MSM this launch sweeps, one scalar + one
    // point = 64 B per TERM, counted once however many windows the term is cut into.  Device bytes: every (term, window) entry is a
    // 4-byte index and a 96-byte affine Niels point.  Work: one mixed addition (7 field multiplications) per entry; Mub counts zero
    // digits too (probability 2^-c each for full-width scalars).
    prof_note(KID_k_bucket_chunks, 64.0 * (double)(total - std::min(total, J.alg_discount)), 100.0 * (double)R.Mub, 7.0 * (double)R.Mub);
    if (!R.per_bucket)
        BPG_LAUNCH((*this), k_bucket_combine, dim3(cdiv(nchunks, 256)), dim3(256), starts.as<uint32_t>(), buckets.as<ge_ext>(), slotA, slotB, open_keys.as<uint32_t>(), nkeys, CH, heavy.as<uint32_t>(), medium.as<uint32_t>());
    else
        BPG_LAUNCH_ID((*this), KID_k_bucket_combine, k_bucket_combine_per_bucket, dim3(cdiv(nkeys, 256)), dim3(256), starts.as<uint32_t>(), buckets.as<ge_ext>(), slotA, slotB, nkeys, CH, heavy.as<uint32_t>());
    BPG_LAUNCH((*this), k_bucket_combine_heavy, dim3(HEAVY_BLOCKS), dim3(256), starts.as<uint32_t>(), buckets.as<ge_ext>(), slotA, slotB, CH, heavy.as<uint32_t>(), medium.as<uint32_t>());
    BPG_LAUNCH((*this), k_bucket_reduce, dim3(cdiv(R.nred, 64)), dim3(64), buckets.as<ge_ext>(), starts.as<uint32_t>(), partial.as<ge_ext>(), P.nb, R.seg, R.nsegpw, R.nred);
    wsums.ensure(R.bytes_wsums);
    if (R.quad) {
        wq_stage.ensure(R.bytes_wq_stage);
        if (!wq_tickets.p) { wq_tickets.ensure(MSM_TICKETS * 4); HIPCHK(hipMemsetAsync(wq_tickets.p, 0, MSM_TICKETS * 4, st)); }
        BPG_LAUNCH((*this), k_window_sums_quad, dim3(R.window_blocks, nmsm * W), dim3(256), partial.as<ge_ext>(), wsums.as<ge_ext>(), wq_stage.as<ge_ext>(), wq_tickets.as<uint32_t>(), R.nsegpw, R.nred,
                   ceil_log2(R.seg), R.lgper);
    } else
        BPG_LAUNCH((*this), k_window_sums, dim3(nmsm * W), dim3(R.window_threads), partial.as<ge_ext>(), wsums.as<ge_ext>(), R.nsegpw, R.nred, ceil_log2(R.seg));
    HIPCHK(hipGetLastError());
    h_wsums.ensure((size_t)WS_SLOTS * WS_SLOT_BYTES);
    MsmTicket t{ws_next, nmsm, W};
    ws_next = (ws_next + 1) % WS_SLOTS;
    HIPCHK(hipMemcpyAsync(h_wsums.as<uint8_t>() + (size_t)t.slot * WS_SLOT_BYTES, wsums.p, R.bytes_wsums, hipMemcpyDeviceToHost, st));
    return t;
}

void Engine::msm_gens(uint64_t first, uint64_t count, const uint8_t *s, const uint8_t *t, uint8_t out[32]) {
    if (first + count > gens_cap_) throw std::invalid_argument("msm_gens: range beyond capacity");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.shared_now = I.shared_variants();
    I.small_sc.ensure(2 * count * 32 + 64); I.sLR.ensure(2 * count * sizeof(scm) + 64);
    I.msm_result.ensure(4 * sizeof(ge_ext)); I.comp.ensure(128);
    if (count) {
        HIPCHK(hipMemcpyAsync(I.small_sc.p, s, count * 32, hipMemcpyHostToDevice, I.st));
        HIPCHK(hipMemcpyAsync(I.small_sc.as<uint8_t>() + count * 32, t, count * 32, hipMemcpyHostToDevice, I.st));
        BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(2 * count, 256)), dim3(256), I.small_sc.as<uint32_t>(), I.sLR.as<scm>(), (uint32_t)(2 * count));
    }
    MsmJob J = job_new();
    seg_push(J, I.sLR.as<scm>(), I.gens + first, (uint32_t)count, 0);
    seg_push(J, I.sLR.as<scm>() + count, I.gens + gens_cap_ + first, (uint32_t)count, 0);
    const Impl::MsmTicket tk = I.msm(J, 1);
    HIPCHK(hipStreamSynchronize(I.st));
    h51::pt_compress(out, I.msm_points(tk)[0]);
}

std::string Engine::test_msm(uint32_t nmsm, uint32_t nseg, const MsmSegSpec *segs, const uint8_t *scalars, uint8_t *out) {
    // every argument is checked here, before anything is queued: no index the caller chose reaches a kernel unchecked
    if (nmsm < 1 || nmsm > 4) throw std::invalid_argument("test_msm: 1..4 results");
    if (nseg > BPG_MAX_SEGS) throw std::invalid_argument("test_msm: at most 16 segments");
    if (nseg && !segs) throw std::invalid_argument("test_msm: no segment array");
    uint64_t total = 0, skipped = 0, skip_words = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        const MsmSegSpec &g = segs[k];
        if (g.table > 1) throw std::invalid_argument("test_msm: table is 0 (G) or 1 (H)");
        if (g.result >= nmsm) throw std::invalid_argument("test_msm: result index out of range");
        if (k && g.result < segs[k - 1].result) throw std::invalid_argument("test_msm: segments must be grouped by ascending result index");
        if (g.lgblk > 31) throw std::invalid_argument("test_msm: lgblk is 0..30, or 31 (contiguous)");
        if (!g.len) continue;
        const uint64_t e = g.len - 1, lg = g.lgblk;
        const uint64_t last = lg >= 31 ? e : (((e >> lg) << (lg + 1)) | (e & ((1ull << lg) - 1)));     // msm_point_index of the last element: the highest
        if (g.first >= gens_cap_ || last >= gens_cap_ - g.first) throw std::invalid_argument("test_msm: segment reaches beyond the generator table");
        total += g.len;
        if (g.skip) {
            for (uint64_t i = 0; i < g.len; i++) skipped += (g.skip[i >> 5] >> (i & 31)) & 1u;
            skip_words += (g.len + 31) / 32;
        }
    }
    if (total >= (1ull << 31)) throw std::invalid_argument("test_msm: too many terms");
    if (total && !scalars) throw std::invalid_argument("test_msm: no scalars");
    for (uint64_t i = 0; i < total; i++) {
        Scalar s; std::memcpy(s.w, scalars + 32 * i, 32);
        if (!s.is_canonical()) throw std::invalid_argument("test_msm: scalar " + std::to_string(i) + " is not canonical");
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.shared_now = I.shared_variants();
    I.small_sc.ensure(total * 32 + 64); I.sLR.ensure(total * sizeof(scm) + 64); I.test_skip.ensure(skip_words * 4 + 4);
    if (total) {
        I.h2d(I.small_sc.p, scalars, total * 32);
        BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(total, 256)), dim3(256), I.small_sc.as<uint32_t>(), I.sLR.as<scm>(), (uint32_t)total);
    }
    MsmJob J = job_new();
    uint64_t t0 = 0, w0 = 0;
    for (uint32_t k = 0; k < nseg; k++) {
        const MsmSegSpec &g = segs[k];
        if (!g.len) continue;
        const uint32_t *skip = nullptr;
        if (g.skip) {
            const uint64_t nw = (g.len + 31) / 32;
            I.h2d(I.test_skip.as<uint32_t>() + w0, g.skip, nw * 4);
            skip = I.test_skip.as<uint32_t>() + w0; w0 += nw;
        }
        seg_push(J, I.sLR.as<scm>() + t0, I.gens + (g.table ? gens_cap_ : 0) + g.first, g.len, g.result, g.lgblk, skip);
        t0 += g.len;
    }
    J.skipped = (uint32_t)skipped;
    const Impl::MsmTicket tk = I.msm(J, nmsm);
    HIPCHK(hipStreamSynchronize(I.st));
    const std::vector<h51::pt> pts = I.msm_points(tk);
    for (uint32_t m = 0; m < nmsm; m++) h51::pt_compress(out + 32 * m, pts[m]);
    // evidence: the plan msm() took, and what its kernels left on the device
    const MsmRun &L = I.msm_last;
    std::vector<uint32_t> st(L.nkeys + 1);
    uint32_t hm[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(st.data(), I.starts.p, st.size() * 4, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(hm, I.heavy.p, 4, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(hm + 1, I.medium.p, 4, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    const MsmPlan &P = L.P;
    std::string j;
    j.reserve(512 + st.size() * 11);
    auto u = [&](const char *k, uint64_t v) { j += "\""; j += k; j += "\": "; j += std::to_string(v); j += ", "; };
    j += "{";
    u("nmsm", P.nmsm); u("W", P.W); u("nb", P.nb); u("fb", P.fb); u("CB", P.CB); u("lgTile", P.lgTile); u("tmax", P.tmax);
    u("CH", L.CH); u("nchunks", L.nchunks); u("nkeys", L.nkeys); u("live", L.live); u("skipped", skipped);
    j += "\"off\": [";
    for (uint32_t w = 0; w <= P.W; w++) { if (w) j += ", "; j += std::to_string(P.off[w]); }
    j += "], \"shared\": "; j += L.shared ? "true" : "false";
    j += ", \"combine\": \""; j += L.per_bucket ? "per_bucket" : "boundary";
    j += "\", \"window_sums\": \""; j += L.quad ? "quad" : "plain"; j += "\", ";
    u("window_blocks", L.window_blocks); u("window_threads", L.window_threads);
    u("sort2_regs", 256u * SORT2_PER); u("msm_stash", MSM_STASH); u("heavy_chunks", HEAVY_CHUNKS); u("heavy_blocks", HEAVY_BLOCKS);
    u("heavy", hm[0]); u("medium", hm[1]);
    j += "\"starts\": [";
    for (size_t i = 0; i < st.size(); i++) { if (i) j += ","; j += std::to_string(st[i]); }
    j += "]}";
    return j;
}

// The generator fold of one group on scalars the caller chose (include/bpg.h bpg_test_fold): Impl::fold_launch() as inner_product() calls it, on the context's own
// generator tables, then the 2 * Mr folded points compressed.  Returns the JSON evidence of what was launched.
std::string Engine::test_fold(int32_t kernel, uint32_t lgMr, uint32_t rounds, uint32_t first, uint64_t n, const uint8_t *sG_bytes, const uint8_t *sH_bytes,
                              const uint8_t u_ch_bytes[32], uint8_t *out) {
    // every argument is checked here, before anything is queued: no index the caller chose reaches a kernel unchecked
    if (!sG_bytes || !sH_bytes || !u_ch_bytes || !out) throw std::invalid_argument("test_fold: null pointer");
    if (rounds < 1 || rounds > 5) throw std::invalid_argument("test_fold: a group has 1..5 rounds");
    if (first > 1) throw std::invalid_argument("test_fold: first is 0 or 1");
    if (kernel < -1 || kernel > (int32_t)FoldKernel::Mem) throw std::invalid_argument("test_fold: kernel is -1 (the chooser's) or 0..6");
    if (lgMr > 31 || (1ull << (lgMr + rounds)) > gens_cap_) throw std::invalid_argument("test_fold: the group-start tables reach beyond the generator tables");
    const uint64_t g_M = 1ull << (lgMr + rounds);
    const uint32_t Mr = 1u << lgMr, nterms = (1u << rounds) - 1u;
    if (first && (n <= g_M / 2 || n > g_M)) throw std::invalid_argument("test_fold: a first group has g_M/2 < n <= g_M");
    std::vector<Scalar> sG(nterms), sH(nterms);
    Scalar u_ch; std::memcpy(u_ch.w, u_ch_bytes, 32);
    if (!u_ch.is_canonical()) throw std::invalid_argument("test_fold: u_ch is not canonical");
    for (uint32_t t = 0; t < nterms; t++) {
        std::memcpy(sG[t].w, sG_bytes + 32 * (size_t)t, 32); std::memcpy(sH[t].w, sH_bytes + 32 * (size_t)t, 32);
        if (!sG[t].is_canonical() || !sH[t].is_canonical()) throw std::invalid_argument("test_fold: scalar " + std::to_string(t) + " is not canonical");
    }
    // a forced kernel: wherever choose_fold could name it under some setting of the knobs (its structural conditions; the size thresholds are dropped)
    const FoldKernel fk = (FoldKernel)(kernel < 0 ? 0 : kernel);
    if (kernel >= 0) {
        bool fits = true;
        switch (fk) {
        case FoldKernel::QuadW: fits = !first && Mr % 64 == 0 && nterms <= 7; break;
        case FoldKernel::RegW: fits = !first && Mr % 256 == 0 && nterms <= 7; break;
        case FoldKernel::Quad: fits = nterms <= 7; break;
        case FoldKernel::Split: fits = nterms >= 3 && nterms <= 15; break;
        case FoldKernel::Reg: fits = nterms == 1 || nterms == 3 || nterms == 7 || nterms == 15; break;
        case FoldKernel::Wnaf: fits = impl_->fold_wnaf >= 3; break;
        case FoldKernel::Mem: break;
        }
        if (!fits) throw std::invalid_argument("test_fold: the chooser never names this kernel for this shape");
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.shared_now = I.shared_variants();
    if (kernel >= 0 && fk == FoldKernel::Wnaf && !I.odd_ensure()) throw std::invalid_argument("test_fold: no table of odd multiples fits this device");
    I.test_fold_tab.ensure((size_t)2 * Mr * sizeof(ge_niels)); I.comp.ensure((size_t)2 * Mr * 32);
    const FoldShape shape{Mr, nterms, first != 0, true};
    const Impl::FoldRun run = I.fold_launch(shape, kernel >= 0 ? &fk : nullptr, g_M, n, u_ch, sG, sH, I.gens, I.gens + gens_cap_, I.test_fold_tab.as<ge_niels>());
    BPG_LAUNCH(I, k_compress_niels, dim3(cdiv(2 * Mr, 64)), dim3(64), I.test_fold_tab.as<ge_niels>(), I.comp.as<uint8_t>(), 2 * Mr);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, I.comp.p, (size_t)2 * Mr * 32, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    static const char *const name_of[] = {"k_fold_points_wnaf", "k_fold_points_quadw", "k_fold_points_quad", "k_fold_points_split", "k_fold_points_regw",
                                          "k_fold_points_reg", "k_fold_points"};           // in the order of FoldKernel
    std::string j = "{\"kernel\": \""; j += name_of[(int)run.kernel]; j += "\"";
    auto u = [&](const char *k, int64_t v) { j += ", \""; j += k; j += "\": "; j += std::to_string(v); };
    u("Mr", Mr); u("nterms", nterms); u("first", first); u("n", (int64_t)n);
    if (run.kernel == FoldKernel::QuadW || run.kernel == FoldKernel::RegW) {
        j += ", \"nsteps\": [" + std::to_string(run.nsteps[0]) + ", " + std::to_string(run.nsteps[1]) + "]";
        j += ", \"tail\": [" + std::to_string(run.tail[0]) + ", " + std::to_string(run.tail[1]) + "]";
    } else u("top", run.top);
    if (run.kernel == FoldKernel::Wnaf) { u("wnaf", I.eff_wnaf); u("parts", I.eff_parts); u("part_bits", I.fold_part_bits()); }
    j += "}";
    return j;
}

// The table-driven tail on scalars the caller chose (include/bpg.h bpg_test_tail): Impl::tail_freeze() and `rounds` times Impl::tail_round() as inner_product()
// calls them, on the context's own generators G[0, M0), H[0, M0) and the Pedersen base B.  Returns the JSON evidence of what was launched.
std::string Engine::test_tail(uint32_t lgM0, uint32_t tables, uint32_t first, uint64_t n, const uint8_t *a_bytes, const uint8_t *b_bytes, const uint8_t yinv_bytes[32],
                              const uint8_t u_ch_bytes[32], const uint8_t gamma0_bytes[32], const uint8_t eta0_bytes[32], const uint8_t w_bytes[32], uint32_t rounds,
                              const uint8_t *u_bytes, uint8_t *lr_out, uint8_t *ab_out) {
    // every argument is checked here, before anything is queued: no index the caller chose reaches a kernel unchecked
    if (!a_bytes || !b_bytes || !yinv_bytes || !u_ch_bytes || !gamma0_bytes || !eta0_bytes || !w_bytes || !u_bytes || !lr_out || !ab_out)
        throw std::invalid_argument("test_tail: null pointer");
    if (lgM0 < 1 || lgM0 > 14 || (1ull << lgM0) > gens_cap_) throw std::invalid_argument("test_tail: M0 is 2 .. 2^14 and at most the capacity of the generator tables");
    if (tables > 2) throw std::invalid_argument("test_tail: tables is 0 (original generators), 1 (folded-style, in the arena) or 2 (wide, 8-bit windows)");
    if (first > 1) throw std::invalid_argument("test_tail: first is 0 or 1");
    if (rounds < 1 || rounds > lgM0) throw std::invalid_argument("test_tail: rounds is 1 .. lgM0");
    const uint32_t M0 = 1u << lgM0;
    if (first && (n <= M0 / 2 || n > M0)) throw std::invalid_argument("test_tail: a first round has M0/2 < n <= M0");
    auto scalar = [](const uint8_t *p, const char *what, bool nonzero) {
        Scalar s; std::memcpy(s.w, p, 32);
        if (!s.is_canonical()) throw std::invalid_argument(std::string("test_tail: ") + what + " is not canonical");
        if (nonzero && (s.w[0] | s.w[1] | s.w[2] | s.w[3]) == 0) throw std::invalid_argument(std::string("test_tail: ") + what + " is zero");
        return s;
    };
    const Scalar yinv = scalar(yinv_bytes, "yinv", true), u_ch = scalar(u_ch_bytes, "u_ch", false), Gamma = scalar(gamma0_bytes, "gamma0", false),
                 Eta = scalar(eta0_bytes, "eta0", false), w = scalar(w_bytes, "w", false);
    std::vector<Scalar> us(rounds);
    for (uint32_t k = 0; k < rounds; k++) us[k] = scalar(u_bytes + 32 * (size_t)k, "a challenge u", true);
    for (uint32_t i = 0; i < M0; i++) { scalar(a_bytes + 32 * (size_t)i, "a scalar of a", false); scalar(b_bytes + 32 * (size_t)i, "a scalar of b", false); }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.shared_now = I.shared_variants();
    // 8-bit tables asked for: refused where the prover would fall back to the 4-bit ones, so that no case passes on other tables than it names
    if (tables == 2 && !I.wide_ensure(M0)) throw std::invalid_argument("test_tail: no 8-bit window tables for this M0 (M0 < 64, or the table budget)");
    I.small_sc.ensure((size_t)2 * M0 * 32); I.lv.ensure((size_t)M0 * sizeof(scm)); I.rv.ensure((size_t)M0 * sizeof(scm)); I.yinvpow.ensure((size_t)M0 * sizeof(scm));
    I.msm_result.ensure(4 * sizeof(ge_ext)); I.h_small.ensure(1 << 16);
    scm *a = I.lv.as<scm>(), *b = I.rv.as<scm>();
    I.h2d(I.small_sc.p, a_bytes, (size_t)M0 * 32); I.h2d(I.small_sc.as<uint8_t>() + (size_t)M0 * 32, b_bytes, (size_t)M0 * 32);
    BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(M0, 256)), dim3(256), I.small_sc.as<uint32_t>(), a, M0);
    BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(M0, 256)), dim3(256), I.small_sc.as<uint32_t>() + (size_t)M0 * 8, b, M0);
    I.exp_tables({{yinv, I.yinvpow.as<scm>(), M0}});
    const uint32_t quad_sums = I.shared_now ? 0u : 1u;
    const ge_niels *G = I.gens, *H = I.gens + gens_cap_;
    Impl::TailState S;
    I.tail_freeze(S, M0, first != 0, n, to_scm(u_ch), Gamma, Eta, G, H, I.bases.as<ge_niels>(), tables != 1, tables == 2);
    if ((tables == 2) != (S.wide != nullptr)) throw std::logic_error("test_tail: the tail settled on other tables than asked for");
    uint64_t mcur = M0;
    for (uint32_t k = 0; k < rounds; k++) {
        I.tail_round(S, a, b, mcur, to_scm(w), quad_sums, lr_out + 64 * (size_t)k);
        I.tail_challenge(S, us[k]);
        mcur /= 2;
    }
    // the last challenge: as the next round would apply it, or as the scalar fold after the last round of a proof does
    if (rounds == lgM0) I.tail_last_fold(S, a, b, mcur); else I.tail_advance(S, a, b, mcur);
    HIPCHK(hipGetLastError());
    std::vector<scm> ab(2 * mcur);
    HIPCHK(hipMemcpyAsync(ab.data(), a, mcur * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(ab.data() + mcur, b, mcur * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    for (uint64_t i = 0; i < 2 * mcur; i++) from_scm(ab[i]).to_bytes(ab_out + 32 * i);
    std::string j = "{\"kernel\": \""; j += S.wide ? "k_tt_round8" : "k_tt_round"; j += "\"";
    auto ev = [&](const char *k, int64_t v) { j += ", \""; j += k; j += "\": "; j += std::to_string(v); };
    ev("tables", tables); ev("M0", M0); ev("nblk", Impl::tail_nblk(M0)); ev("quad", quad_sums);
    j += "}";
    return j;
}

// The verifier's flattened weights of a resident circuit at a z the caller chose (include/bpg.h bpg_test_weights): Impl::flatten_weights() as verify_prep() calls
// it, laid out in the arena as there.  out = 3 n + m + 1 canonical scalars w_L | w_R | w_O | w_V | w_c.
void Engine::test_weights(DeviceCircuit *c, const uint8_t z_bytes[32], uint8_t *out) {
    if (!c || !z_bytes || !out) throw std::invalid_argument("test_weights: null pointer");
    Scalar z;
    std::memcpy(z.w, z_bytes, 32);
    if (!z.is_canonical()) throw std::invalid_argument("test_weights: z is not canonical");
    if (c->device != device_) throw std::invalid_argument("test_weights: the circuit lives on another device");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const size_t b_w = Impl::al256(c->ncols * sizeof(scm)), b_z = Impl::al256((c->q + 2) * sizeof(scm));
    I.arena.ensure(b_w + b_z);
    scm *const w = reinterpret_cast<scm *>(I.arena_at(0)), *const zpow = reinterpret_cast<scm *>(I.arena_at(b_w));
    I.flatten_weights(c, z, zpow, w, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<scm> h(c->ncols);
    HIPCHK(hipMemcpyAsync(h.data(), w, c->ncols * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    for (uint64_t k = 0; k < c->ncols; k++) from_scm(h[k]).to_bytes(out + 32 * k);
}

// A_I, A_O, S on scalars the caller chose (include/bpg.h bpg_test_commit3): Impl::commit3() as prove() calls it, on the window tables of the context's own
// generators G[0, M0), H[0, M0).  Returns the JSON evidence of what was launched.
std::string Engine::test_commit3(uint32_t lgM0, uint64_t n, const uint8_t *aL, const uint8_t *aR, const uint8_t *aO, const uint8_t *sL, const uint8_t *sR,
                                 const uint8_t *blind, uint8_t out[96]) {
    if (!aL || !aR || !aO || !sL || !sR || !blind || !out) throw std::invalid_argument("test_commit3: null pointer");
    if (lgM0 > 14 || (1ull << lgM0) > gens_cap_) throw std::invalid_argument("test_commit3: M0 is 1 .. 2^14 and at most the capacity of the generator tables");
    const uint32_t M0 = 1u << lgM0;
    if (n < 1 || n > M0) throw std::invalid_argument("test_commit3: n is 1 .. M0");
    const uint8_t *vec[5] = {aL, aR, aO, sL, sR};
    for (int v = 0; v < 5; v++) for (uint64_t i = 0; i < n; i++) {
        Scalar s; std::memcpy(s.w, vec[v] + 32 * i, 32);
        if (!s.is_canonical()) throw std::invalid_argument("test_commit3: scalar " + std::to_string(i) + " of vector " + std::to_string(v) + " is not canonical");
    }
    for (int k = 0; k < 3; k++) {
        Scalar s; std::memcpy(s.w, blind + 32 * k, 32);
        if (!s.is_canonical()) throw std::invalid_argument("test_commit3: blinding " + std::to_string(k) + " is not canonical");
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.shared_now = I.shared_variants();
    const uint64_t total = 5 * n + 3;
    I.small_sc.ensure(total * 32); I.sLR.ensure(5 * n * sizeof(scm)); I.extras.ensure(16 * sizeof(scm));
    I.msm_result.ensure(4 * sizeof(ge_ext)); I.h_small.ensure(1 << 16);
    for (int v = 0; v < 5; v++) I.h2d(I.small_sc.as<uint8_t>() + (size_t)v * n * 32, vec[v], n * 32);
    I.h2d(I.small_sc.as<uint8_t>() + 5 * n * 32, blind, 96);
    scm *d = I.sLR.as<scm>();
    BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(5 * n, 256)), dim3(256), I.small_sc.as<uint32_t>(), d, (uint32_t)(5 * n));
    BPG_LAUNCH(I, k_sc_from_bytes, dim3(1), dim3(256), I.small_sc.as<uint32_t>() + 5 * n * 8, I.extras.as<scm>(), 3u);
    const uint32_t quad_sums = I.shared_now ? 0u : 1u;
    I.tt_build(I.gens, I.gens + gens_cap_, I.bases.as<ge_niels>(), M0, true);
    I.commit3(d, d + n, d + 2 * n, d + 3 * n, d + 4 * n, n, M0, quad_sums, out);
    std::string j = "{";
    j += "\"M0\": " + std::to_string(M0) + ", \"n\": " + std::to_string(n) + ", \"nblk\": " + std::to_string(Impl::commit3_nblk(M0)) + ", \"quad\": " + std::to_string(quad_sums);
    j += "}";
    return j;
}

// ------------------------------------------------------------------------------------------------ circuit upload
// CSR (by constraint) -> CSC (by variable) on the stream: q rows over nmul multipliers per side (columns [0, 3 nmul)) and m committed variables, the constant
// terms as the last column.  W: counts, starts, cursor, rowconst, rowconst_start and the scans' block sums, each of the size host/csc_work.hpp gives for
// (3 nmul + m, q) - the second scan uses counts as scratch for q words, so a tall matrix (q > 3 nmul + m) needs more of it than the columns do.
// totals[0] = first entry of the constant-terms column, totals[1] = entries written: the caller reads them back and checks that none was lost
void Engine::Impl::transpose_csr(const uint64_t *rp, const uint32_t *tv, const uint32_t *tc, uint64_t q, uint64_t nmul, uint64_t m, const CscWork &W,
                                 uint64_t *col_ptr, uint32_t *ent_row, uint32_t *ent_coef, uint32_t *totals) {
    const uint64_t nvar = 3 * nmul + m;
    static_assert(CSC_SCAN_CHUNK == SCAN_CHUNK, "host/csc_work.hpp sizes the block sums for the chunk of k_scan_apply");
    const uint32_t nb1 = cdiv(nvar ? nvar : 1, SCAN_CHUNK), nb2 = cdiv(q ? q : 1, SCAN_CHUNK);
    HIPCHK(hipMemsetAsync(W.counts, 0, (nvar + 1) * 4, st));
    HIPCHK(hipMemsetAsync(W.rowconst, 0, (q + 1) * 4, st));
    if (q) BPG_LAUNCH((*this), k_csc_count, dim3(cdiv(q, 256)), dim3(256), rp, tv, (uint32_t)q, (uint32_t)nmul, (uint32_t)m, W.counts, W.rowconst);
    // exclusive scans: variable columns -> starts / cursor, constant terms per row -> rowconst_start
    BPG_LAUNCH((*this), k_scan_blocksums, dim3(nb1), dim3(256), W.counts, (uint32_t)nvar, W.bsum);
    BPG_LAUNCH((*this), k_scan_apply, dim3(nb1), dim3(256), W.counts, (uint32_t)nvar, W.bsum, W.starts, W.cursor);
    BPG_LAUNCH((*this), k_scan_blocksums, dim3(nb2), dim3(256), W.rowconst, (uint32_t)q, W.bsum);
    BPG_LAUNCH((*this), k_scan_apply, dim3(nb2), dim3(256), W.rowconst, (uint32_t)q, W.bsum, W.rowconst_start, W.counts /* scratch */);
    BPG_LAUNCH((*this), k_csc_colptr, dim3(cdiv(nvar + 1, 256)), dim3(256), W.starts, W.rowconst_start, (uint32_t)nvar, (uint32_t)q, col_ptr, totals);
    if (q) BPG_LAUNCH((*this), k_csc_fill, dim3(cdiv(q, 256)), dim3(256), rp, tv, tc, (uint32_t)q, (uint32_t)nmul, (uint32_t)m, W.cursor, W.rowconst_start,
                      W.starts + nvar, ent_row, ent_coef);
}

void Engine::check_instance(const FlatView &c, uint64_t n_inputs, uint64_t n_gates) {
    const uint64_t n = c.n, m = c.m, q = c.q, nnz = c.nnz, ncoef = c.ncoef;
    const bool has_witness = !(!c.aL && !c.aR && !c.aO && n > 0);
    if (has_witness && n > 0 && (!c.aL || !c.aR || !c.aO)) throw std::invalid_argument("upload: witness vectors must hold n scalars");
    if (!c.row_ptr || c.row_ptr[0] != 0 || c.row_ptr[q] != nnz || (nnz && (!c.term_var || !c.term_coef)) || (ncoef && !c.coef)) throw std::invalid_argument("upload: malformed CSR");
    if (n >= (1u << 27)) throw std::invalid_argument("upload: too many multipliers");
    const uint64_t ncols = 3 * n + m + 1;
    if (q >= (1ull << 32) || nnz >= (1ull << 32) || ncols >= (1ull << 32)) throw std::invalid_argument("upload: circuit too large");
    for (uint64_t k = 0; k < nnz; k++) {
        const uint32_t pv = c.term_var[k], kind = pv >> 29, idx = pv & 0x1fffffffu;
        if (c.term_coef[k] >= ncoef) throw std::invalid_argument("upload: coefficient index out of range");
        if (kind <= 2) { if (idx >= n) throw std::invalid_argument("upload: multiplier index out of range"); }
        else if (kind == 3) { if (idx >= m) throw std::invalid_argument("upload: committed index out of range"); }
        else if (kind == Variable::Input && n_inputs) {
            if (idx >= n_inputs) throw std::invalid_argument("upload: term " + std::to_string(k) + " names public input " + std::to_string(idx) + " (the template takes " + std::to_string(n_inputs) + ")");
        }
        else if (kind == Variable::Gated && n_gates) {
            if (idx >= n_gates) throw std::invalid_argument("upload: term " + std::to_string(k) + " names gate " + std::to_string(idx) + " (the template has " + std::to_string(n_gates) + ")");
        }
        else if (kind != 4) throw std::invalid_argument("upload: bad variable kind (term " + std::to_string(k) + " has kind " + std::to_string(kind) +
                                                        (kind == Variable::Input ? ": a public input, which only bpg_r1cs_upload_template_inputs takes)" :
                                                         kind == Variable::Gated ? ": a gated variable, which only bpg_r1cs_upload_template_gated takes)" : ")"));
    }
    for (uint64_t r = 0; r < q; r++) if (c.row_ptr[r] > c.row_ptr[r + 1]) throw std::invalid_argument("upload: malformed CSR");
}

DeviceCircuit *Engine::upload(const FlatView &c) {
    check_instance(c);                              // every refusal before the device is touched
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint64_t n = c.n, m = c.m, q = c.q, nnz = c.nnz, ncoef = c.ncoef;
    const bool has_witness = !(!c.aL && !c.aR && !c.aO && n > 0);
    // transposition CSR (by constraint) -> CSC (by variable) on the device (transpose_csr);
    // columns: [0,n) left, [n,2n) right, [2n,3n) output, [3n,3n+m) committed, 3n+m = the constant terms (only the verifier's w_c needs them)
    const uint64_t ncols = 3 * n + m + 1, nvar = ncols - 1;
    std::unique_ptr<DeviceCircuit> d(new DeviceCircuit());       // (the device is current: a failure below frees what it holds as it leaves)
    d->device = device_;
    d->owner = this;
    d->n = n; d->m = m; d->q = q; d->ncols = ncols; d->has_witness = has_witness;
    d->aL.ensure((n ? n : 1) * sizeof(scm)); d->aR.ensure((n ? n : 1) * sizeof(scm)); d->aO.ensure((n ? n : 1) * sizeof(scm));
    d->col_ptr.ensure((ncols + 1) * 8); d->ent_row.ensure((nnz ? nnz : 1) * 4); d->ent_coef.ensure((nnz ? nnz : 1) * 4);
    d->coef.ensure((ncoef ? ncoef : 1) * sizeof(scm));
    {
        // the CSR arrays travel as they are; workspace: the MSM sort buffers (no MSM runs on this context during an upload)
        I.arena.ensure((nnz ? nnz : 1) * 8);                                // term_var | term_coef
        I.plain.ensure((q + 2) * 8 + 64);                                   // row_ptr
        const CscWorkWords ws = csc_work_words(nvar, q);                     // (host/csc_work.hpp: the one size rule, shared with the lockstep wave)
        I.counts.ensure(ws.counts * 4); I.starts.ensure(ws.starts * 4); I.cursor.ensure(ws.cursor * 4);
        I.heavy.ensure(ws.rowconst * 4); I.tile_hist.ensure(ws.rowconst_start * 4); I.blocksum.ensure(ws.bsum * 4);
        I.extras.ensure(16 * sizeof(scm));
        uint32_t *tv = I.arena.as<uint32_t>(), *tc = tv + (nnz ? nnz : 1);
        uint64_t *rp = I.plain.as<uint64_t>();
        uint32_t *totals = reinterpret_cast<uint32_t *>(I.extras.as<scm>() + 8);
        if (nnz) { I.h2d(tv, c.term_var, nnz * 4); I.h2d(tc, c.term_coef, nnz * 4); }
        I.h2d(rp, c.row_ptr, (q + 1) * 8);
        I.transpose_csr(rp, tv, tc, q, n, m, {I.counts.as<uint32_t>(), I.starts.as<uint32_t>(), I.cursor.as<uint32_t>(), I.heavy.as<uint32_t>(), I.tile_hist.as<uint32_t>(), I.blocksum.as<uint32_t>()},
                        d->col_ptr.as<uint64_t>(), d->ent_row.as<uint32_t>(), d->ent_coef.as<uint32_t>(), totals);
        HIPCHK(hipGetLastError());
        uint32_t h_tot[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(h_tot, totals, 8, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipStreamSynchronize(I.st));
        d->const_begin = h_tot[0]; d->nnz = h_tot[1];
        if (d->nnz != nnz) throw std::logic_error("upload: transposition lost entries");
    }
    const size_t maxn = std::max<uint64_t>(n, ncoef);
    I.small_sc.ensure((maxn ? maxn : 1) * 32);
    const uint8_t *src[4] = {c.aL, c.aR, c.aO, c.coef};
    scm *const dst[4] = {d->aL.as<scm>(), d->aR.as<scm>(), d->aO.as<scm>(), d->coef.as<scm>()};
    const uint64_t cnts[4] = {n, n, n, ncoef};
    for (int k = 0; k < 4; k++) {
        if (!cnts[k] || (k < 3 && !has_witness)) continue;
        I.h2d(I.small_sc.p, src[k], cnts[k] * 32);
        BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(cnts[k], 256)), dim3(256), I.small_sc.as<uint32_t>(), dst[k], (uint32_t)cnts[k]);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
    }
    return d.release();
}

void Engine::free_circuit(DeviceCircuit *c) {
    if (!c) return;
    (void)hipSetDevice(device_);
    delete c;
}

// ------------------------------------------------------------------------------------------------ circuit templates (host/template.hpp, hip/k_witness.cuh)
TemplatePlan Engine::plan_template(const FlatView &c, const WitnessProgramView &p, const uint8_t *input_values) {
    check_instance(c, p.n_inputs, p.n_gates);
    check_witness_program(c, p);
    if (p.n_inputs && !input_values && c.n && c.aL) throw std::invalid_argument("template: the instance carries a witness and no values were given for its " + std::to_string(p.n_inputs) + " public inputs");
    TemplatePlan T;
    T.schedule = build_witness_schedule(c.n, c.m, p);
    // BPG_WIT_HINT_SHARE=0 (measurement only, tools/diag/range_template.py): every bit hint reduces its source again
    const bool share = !env_present("BPG_WIT_HINT_SHARE") || env_int_strict("BPG_WIT_HINT_SHARE", 0, 1) != 0;
    T.packed = pack_witness_program(c, p, T.schedule, share);       // the classes come from the caller's table: slots are constants of rows only
    T.slotted = with_parameter_slots(c, p, &T.in_slots, input_values);
    T.n_params = p.n_params; T.param_first = c.ncoef;
    T.n_inputs = p.n_inputs; T.slot_first = c.ncoef + p.n_params; T.n_gates = p.n_gates;
    T.ck_var.assign(p.ck_var, p.ck_var + p.n_ck);
    return T;
}
namespace {
// 32-byte scalars <-> the interpreter's scalars, as the test hooks below take and return them
std::vector<scm> scalars_from_bytes(const uint8_t *b, size_t count) {
    std::vector<scm> out(count ? count : 1);
    for (size_t i = 0; i < count; i++) { uint32_t w[8]; std::memcpy(w, b + 32 * i, 32); out[i] = sc_from_words(w); }
    return out;
}
void scalars_to_bytes(const std::vector<scm> &v, uint8_t *out) {
    for (size_t i = 0; i < v.size(); i++) { uint32_t w[8]; sc_to_words(w, v[i]); std::memcpy(out + 32 * i, w, 32); }
}
}  // namespace
// TEST HOOK (bpg_test_template_eval): the interpreter of k_witness.cuh compiled for the HOST, over the same packed program in the same level order
void Engine::template_eval_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out) {
    const TemplatePlan T = plan_template(c, p);
    const PackedWitnessProgram &P = T.packed;
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, c.m);
    std::vector<scm> aL(c.n), aR(c.n), aO(c.n);
    for (const WitnessSegment &s : P.segs) witness_eval_segment(s.first, s.count, P.stream.data() + s.stream, coef.data(), vv.data(), aL.data(), aR.data(), aO.data());
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
}

// TEST HOOK (bpg_test_template_eval_checkpointed): poison, every level's segments in reverse order, then the step of k_witness_ck_verify
uint64_t Engine::template_eval_checkpointed_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *v, const uint8_t *ck_values,
                                                 uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out, const uint8_t *input_values) {
    if (p.n_inputs && !input_values) throw std::invalid_argument("template_eval: the program has public inputs and no values were given for them");
    FlatView rows = c; rows.aL = rows.aR = rows.aO = nullptr;       // (the hook evaluates: a witness in the instance is not looked at)
    const TemplatePlan T = plan_template(rows, p);
    const PackedWitnessProgram &P = T.packed;
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, c.m), ck = scalars_from_bytes(ck_values, p.n_ck);
    const std::vector<scm> in = scalars_from_bytes(input_values, p.n_inputs);
    static const uint8_t kPoison[32] = {0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a,
                                        0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x0a};
    const scm poison = scalars_from_bytes(kPoison, 1)[0];
    std::vector<scm> aL(c.n, poison), aR(c.n, poison), aO(c.n, poison);
    const std::vector<uint32_t> &lp = T.schedule.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l + 1]; s-- > lp[l];)
            witness_eval_segment(P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data(), aL.data(), aR.data(), aO.data(), ck.data(),
                                 in.data());
    uint64_t first = CHECKPOINTS_HOLD;
    for (uint64_t k = p.n_ck; k-- > 0;) if (!witness_ck_holds(p.ck_var[k], ck[k], aL.data(), aR.data(), aO.data())) first = k;
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
    return first;
}

// TEST HOOK (bpg_test_template_eval_batch): k_witness_eval_batch on the host - one pass per level, per segment every item, into the wave layout
void Engine::template_eval_batch_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out) {
    const TemplatePlan T = plan_template(c, p);
    const PackedWitnessProgram &P = T.packed;
    const uint64_t N = padded_size(c.n);
    if (count > (1ull << 26) / N) throw std::invalid_argument("template_eval_batch: too many items");
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, count * c.m);
    std::vector<scm> aL(count * N, sc_zero()), aR(count * N, sc_zero()), aO(count * N, sc_zero());
    const std::vector<uint32_t> &lp = T.schedule.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l]; s < lp[l + 1]; s++)
            for (uint64_t k = 0; k < count; k++)
                witness_eval_segment(P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data() + k * c.m,
                                     aL.data() + k * N, aR.data() + k * N, aO.data() + k * N);
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
}

// TEST HOOK (bpg_test_template_eval_batch_checkpointed): the batched interpreter with item k's checkpoint values at ck_values[k * n_ck ..), under the
// discipline of template_eval_checkpointed_host - rows [0, n) of every item poisoned, the segments of every level in reverse order (per segment every
// item, as a launch has them) - then the step of k_witness_ck_verify_batch: first_out[k] = the lowest mismatching checkpoint of item k, or CHECKPOINTS_HOLD
void Engine::template_eval_batch_checkpointed_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                   uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out, uint64_t *first_out, const uint8_t *input_values) {
    if (p.n_inputs && count && !input_values) throw std::invalid_argument("template_eval_batch: the program has public inputs and no values were given for them");
    FlatView rows = c; rows.aL = rows.aR = rows.aO = nullptr;
    const TemplatePlan T = plan_template(rows, p);
    const PackedWitnessProgram &P = T.packed;
    const uint64_t N = padded_size(c.n);
    if (count > (1ull << 26) / N) throw std::invalid_argument("template_eval_batch: too many items");
    if (p.n_ck && count && !ck_values) throw std::invalid_argument("template_eval_batch: the program has checkpoints and no values were given for them");
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, count * c.m), ck = scalars_from_bytes(ck_values, count * p.n_ck);
    const std::vector<scm> in = scalars_from_bytes(input_values, count * p.n_inputs);
    static const uint8_t kPoison[32] = {0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a,
                                        0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x0a};
    const scm poison = scalars_from_bytes(kPoison, 1)[0];
    std::vector<scm> aL(count * N, sc_zero()), aR(count * N, sc_zero()), aO(count * N, sc_zero());
    for (uint64_t k = 0; k < count; k++)
        for (uint64_t i = 0; i < c.n; i++) aL[k * N + i] = aR[k * N + i] = aO[k * N + i] = poison;
    const std::vector<uint32_t> &lp = T.schedule.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l + 1]; s-- > lp[l];)
            for (uint64_t k = 0; k < count; k++)
                witness_eval_segment(P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data() + k * c.m,
                                     aL.data() + k * N, aR.data() + k * N, aO.data() + k * N, p.n_ck ? ck.data() + k * p.n_ck : nullptr,
                                     p.n_inputs ? in.data() + k * p.n_inputs : nullptr);
    for (uint64_t k = 0; k < count; k++) {
        first_out[k] = CHECKPOINTS_HOLD;
        for (uint64_t j = p.n_ck; j-- > 0;)
            if (!witness_ck_holds(p.ck_var[j], ck[k * p.n_ck + j], aL.data() + k * N, aR.data() + k * N, aO.data() + k * N)) first_out[k] = j;
    }
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
}

DeviceCircuit *Engine::upload_template(const FlatView &c, const TemplatePlan &T) {
    const PackedWitnessProgram &P = T.packed;
    FlatView f(T.slotted); f.aL = c.aL; f.aR = c.aR; f.aO = c.aO;
    std::unique_ptr<DeviceCircuit> d(upload(f));
    Impl &I = *impl_;
    d->is_template = true; d->n_params = T.n_params; d->param_first = T.param_first;
    d->wit_level_ptr = T.schedule.level_ptr;
    if (ceil_log2(c.n) <= TEMPLATE_HOST_COPY_LG) { d->host = T.slotted; d->host_view = FlatView(d->host); d->has_host = true; }
    d->wit_stream.ensure(P.stream.size() * 4); d->wit_segs.ensure(P.segs.size() * sizeof(WitnessSegment)); d->wit_v.ensure((c.m ? c.m : 1) * sizeof(scm));
    I.h2d(d->wit_stream.p, P.stream.data(), P.stream.size() * 4);
    I.h2d(d->wit_segs.p, P.segs.data(), P.segs.size() * sizeof(WitnessSegment));
    d->n_ck = T.ck_var.size();
    if (d->n_ck) {
        d->wit_ck_var.ensure(d->n_ck * 4); d->wit_ck.ensure(d->n_ck * sizeof(scm));
        I.h2d(d->wit_ck_var.p, T.ck_var.data(), d->n_ck * 4);
    }
    d->n_in = T.n_inputs; d->slot_first = T.slot_first; d->n_slots = T.in_slots.size(); d->n_gates = T.n_gates;
    if (d->n_in) {
        d->wit_in.ensure(d->n_in * sizeof(scm)); d->in_slots.ensure((d->n_slots ? d->n_slots : 1) * sizeof(InputSlot));
        if (d->n_slots) I.h2d(d->in_slots.p, T.in_slots.data(), d->n_slots * sizeof(InputSlot));
    }
    HIPCHK(hipStreamSynchronize(I.st));
    return d.release();
}

// TEST HOOK (bpg_test_template_inputs_instance): the rows with their slots, the parameter slots as an assign of param_values leaves them and the derived slots as
// k_input_slots leaves them - its product on the scalars of the device code, compiled for the host
FlatCircuit Engine::template_inputs_instance_host(const FlatView &c, const WitnessProgramView &p, const uint8_t *param_values, const uint8_t *input_values) {
    if (p.n_inputs && !input_values) throw std::invalid_argument("template_inputs_instance: the program has public inputs and no values were given for them");
    if (p.n_params && !param_values) throw std::invalid_argument("template_inputs_instance: the program has parameter rows and no values were given for them");
    FlatView rows = c; rows.aL = rows.aR = rows.aO = nullptr;
    TemplatePlan T = plan_template(rows, p);
    FlatCircuit f = std::move(T.slotted);
    const std::vector<scm> par = scalars_from_bytes(param_values, p.n_params), in = scalars_from_bytes(input_values, p.n_inputs);
    std::vector<scm> coef = scalars_from_bytes(f.coef.data(), f.coef.size() / 32);
    for (uint64_t k = 0; k < p.n_params; k++) coef[T.param_first + k] = par[k];
    for (size_t s = 0; s < T.in_slots.size(); s++) coef[T.slot_first + s] = witness_input_slot(coef[T.in_slots[s].ci], in[T.in_slots[s].p]);
    coef.resize(f.coef.size() / 32);
    if (!coef.empty()) scalars_to_bytes(coef, f.coef.data());
    return f;
}

uint64_t Engine::checkpoints_per_item(const DeviceCircuit *d) { return d ? d->n_ck : 0; }
void Engine::assign(DeviceCircuit *d, const uint8_t *v, const uint8_t *param_values) {
    if (d && d->n_ck) throw std::invalid_argument("assign: the template was uploaded with checkpoints and needs their values (bpg_r1cs_assign_checkpointed)");
    (void)assign_checkpointed(d, v, param_values, nullptr);
}
uint64_t Engine::assign_checkpointed(DeviceCircuit *d, const uint8_t *v, const uint8_t *param_values, const uint8_t *ck_values) {
    if (d && d->n_in) throw std::invalid_argument("assign: the template has public inputs and needs their values (bpg_r1cs_assign_inputs)");
    return assign_inputs(d, v, param_values, ck_values, nullptr);
}
uint64_t Engine::assign_inputs(DeviceCircuit *d, const uint8_t *v, const uint8_t *param_values, const uint8_t *ck_values, const uint8_t *input_values) {
    if (!d || !d->is_template) throw std::invalid_argument("assign: the circuit is not a template (bpg_r1cs_upload_template)");
    const uint64_t items = d->rep_count ? d->rep_count : 1, total_ck = d->n_ck * items;
    if (total_ck && !ck_values) throw std::invalid_argument("assign: the template has checkpoints and no values were given for them");
    if (d->n_in && !input_values) throw std::invalid_argument("assign: the template has public inputs and no values were given for them");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    // the previous witness is gone from here on: a failure below must not leave its caches behind either
    drop_witness(d);                                // (the equal-scalar sets belong to the witness they were built from)
    const uint64_t cnt[4] = {d->m, d->n_params, total_ck, d->n_in};
    const uint8_t *src[4] = {v, param_values, ck_values, input_values};
    scm *dst[4] = {d->wit_v.as<scm>(), d->coef.as<scm>() + d->param_first, d->wit_ck.as<scm>(), d->wit_in.as<scm>()};       // checkpoint values and inputs go up and into Montgomery form as v does
    I.small_sc.ensure((std::max(std::max(cnt[0], cnt[1]), std::max(cnt[2], cnt[3])) + 1) * 32);
    for (int k = 0; k < 4; k++) {
        if (!cnt[k]) continue;
        I.h2d(I.small_sc.p, src[k], cnt[k] * 32);
        BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(cnt[k], 256)), dim3(256), I.small_sc.as<uint32_t>(), dst[k], (uint32_t)cnt[k]);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));                                     // small_sc is staged again below
    }
    const scm *ck = total_ck ? d->wit_ck.as<scm>() : nullptr;
    const scm *in = d->n_in ? d->wit_in.as<scm>() : nullptr;
    // the derived slots of the rows, before anything reads a constant term: coef[ci] * x_p, a lane per slot
    I.fill_input_slots(d);
    // a join: ONE launch per level for all its parts (levels 0 .. the most any part has), that level's rows of the block table
    for (size_t l = 0; l + 1 < d->join_level_ptr.size(); l++) {
        const uint32_t b0 = d->join_level_ptr[l], nb = d->join_level_ptr[l + 1] - b0;
        BPG_LAUNCH(I, k_witness_eval_join, dim3(nb), dim3(64), d->join_blocks.as<uint4>() + b0, d->join_desc.as<JoinPart>(), d->wit_segs.as<uint4>(),
                   d->wit_stream.as<uint32_t>(), d->coef.as<scm>(), d->wit_v.as<scm>(), ck, in, d->aL.as<scm>(), d->aR.as<scm>(), d->aO.as<scm>());
    }
    // a level's lanes are few (a 512-leaf tree: at most 256): spread them over waves until every SIMD of the device has one
    for (size_t l = 0; l + 1 < d->wit_level_ptr.size(); l++) {
        const uint32_t s0 = d->wit_level_ptr[l], ns = d->wit_level_ptr[l + 1] - s0;
        if (d->rep_count) {         // a repeat: the source's level, a lane per (segment, item), consecutive lanes = consecutive items of one segment
            const uint32_t K = (uint32_t)d->rep_count;
            const uint32_t bps = cdiv(K, 64);                                       // 64 consecutive items of a segment per block, as k_witness_eval_batch has them
            BPG_LAUNCH(I, k_witness_eval_repeat, dim3(ns * bps), dim3(64), d->wit_segs.as<uint4>() + s0, ns, bps, d->wit_stream.as<uint32_t>(), d->coef.as<scm>(),
                       d->wit_v.as<scm>(), ck, (uint32_t)d->n_ck, in, (uint32_t)d->rep_in, (uint32_t)d->rep_n, (uint32_t)d->rep_m, K, d->aL.as<scm>(), d->aR.as<scm>(),
                       d->aO.as<scm>());
            continue;
        }
        const uint32_t lanes = std::min(64u, std::max(1u, cdiv(ns, I.wit_waves)));
        BPG_LAUNCH(I, k_witness_eval, dim3(cdiv(ns, lanes)), dim3(lanes), d->wit_segs.as<uint4>() + s0, ns, d->wit_stream.as<uint32_t>(), d->coef.as<scm>(),
                   d->wit_v.as<scm>(), ck, in, d->aL.as<scm>(), d->aR.as<scm>(), d->aO.as<scm>());
    }
    uint64_t first = CHECKPOINTS_HOLD;
    if (total_ck) {                                 // were the caller's values the circuit's own?  one launch, one 8-byte read-back
        I.ck_first.ensure(8);
        static const uint64_t kHold = CHECKPOINTS_HOLD;
        HIPCHK(hipMemcpyAsync(I.ck_first.p, &kHold, 8, hipMemcpyHostToDevice, I.st));
        if (!d->join_parts.empty())
            BPG_LAUNCH(I, k_witness_ck_verify_join, dim3(cdiv(total_ck, 256)), dim3(256), d->wit_ck_var.as<uint32_t>(), d->join_desc.as<JoinPart>(),
                       (uint32_t)d->join_parts.size(), total_ck, ck, d->aL.as<scm>(), d->aR.as<scm>(), d->aO.as<scm>(), I.ck_first.as<unsigned long long>());
        else
            BPG_LAUNCH(I, k_witness_ck_verify, dim3(cdiv(total_ck, 256)), dim3(256), d->wit_ck_var.as<uint32_t>(), (uint32_t)d->n_ck, total_ck,
                       (uint32_t)(d->rep_count ? d->rep_n : d->n), ck, d->aL.as<scm>(), d->aR.as<scm>(), d->aO.as<scm>(), I.ck_first.as<unsigned long long>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&first, I.ck_first.p, 8, hipMemcpyDeviceToHost, I.st));
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
    if (first != CHECKPOINTS_HOLD) return first;    // an inconsistent witness is never provable: the circuit stays without one (drop_witness above)
    d->has_witness = true; d->wit_v_set = true;
    return first;
}
// the derived slots from the inputs in wit_in, queued on the stream: one launch, whichever kind of template (a single one: k_input_slots; a repeat or join:
// k_input_slots_join over its descriptors)
void Engine::Impl::fill_input_slots(DeviceCircuit *d) {
    if (!d->n_slots) return;
    if (d->slot_parts)
        BPG_LAUNCH((*this), k_input_slots_join, dim3(cdiv(d->n_slots, 256)), dim3(256), d->join_desc.as<JoinPart>(), d->slot_parts, (uint64_t)d->n_slots,
                   d->in_slots.as<uint32_t>(), d->wit_in.as<scm>(), d->coef.as<scm>());
    else
        BPG_LAUNCH((*this), k_input_slots, dim3(cdiv(d->n_slots, 256)), dim3(256), d->in_slots.as<uint2>(), (uint32_t)d->n_slots, (uint32_t)d->slot_first, 0u,
                   (uint32_t)d->n_in, (uint64_t)d->n_slots, d->wit_in.as<scm>(), d->coef.as<scm>());
}
// The verifier's half of assign_inputs (include/bpg.h bpg_r1cs_set_inputs): the inputs go up and into Montgomery form, the derived slots are filled, nothing else
// happens.  The circuit is left WITHOUT a witness: whatever a_L, a_R, a_O hold was computed under other inputs.
void Engine::set_inputs(DeviceCircuit *d, const uint8_t *input_values) {
    if (!d || !d->is_template || !d->n_in) throw std::invalid_argument("set_inputs: the circuit is not a template with public inputs (bpg_r1cs_upload_template_inputs)");
    if (!input_values) throw std::invalid_argument("set_inputs: the template has public inputs and no values were given for them");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    drop_witness(d);
    I.small_sc.ensure((d->n_in + 1) * 32);
    I.h2d(I.small_sc.p, input_values, d->n_in * 32);
    BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(d->n_in, 256)), dim3(256), I.small_sc.as<uint32_t>(), d->wit_in.as<scm>(), (uint32_t)d->n_in);
    I.fill_input_slots(d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
}
// ------------------------------------------------------------------------------------------------ R1CS check on the device (hip/k_check.cuh, host/check.hpp)
// The row-major view of a resident matrix, from its column-major form: entries per row, an exclusive scan, (column, coefficient slot) pairs per row, and the
// list of rows that are too long for one lane.  Workspace: the scan buffers of the MSM (no MSM runs on this context during a check).  Queued, not waited for.
void Engine::Impl::rowview_build(DeviceCircuit *c) {
    const uint64_t q = c->q, nnz = c->nnz;
    c->rv_ptr.ensure((q + 1) * 4); c->rv_ent.ensure((nnz ? nnz : 1) * 8); c->rv_long.ensure((q + 1) * 4);
    counts.ensure((q + 2) * 4); cursor.ensure((q + 2) * 4); blocksum.ensure((size_t)(cdiv(q, SCAN_CHUNK) + 2) * 4);
    HIPCHK(hipMemsetAsync(counts.p, 0, (q + 1) * 4, st));
    HIPCHK(hipMemsetAsync(c->rv_long.p, 0, 4, st));
    if (nnz) BPG_LAUNCH((*this), k_rowview_count, dim3(cdiv(nnz, 256)), dim3(256), c->ent_row.as<uint32_t>(), c->const_begin, nnz, counts.as<uint32_t>());
    const uint32_t nb = cdiv(q, SCAN_CHUNK);
    BPG_LAUNCH((*this), k_scan_blocksums, dim3(nb), dim3(256), counts.as<uint32_t>(), (uint32_t)q, blocksum.as<uint32_t>());
    BPG_LAUNCH((*this), k_scan_apply, dim3(nb), dim3(256), counts.as<uint32_t>(), (uint32_t)q, blocksum.as<uint32_t>(), c->rv_ptr.as<uint32_t>(), cursor.as<uint32_t>());
    if (nnz) BPG_LAUNCH((*this), k_rowview_fill, dim3(cdiv(nnz, 256)), dim3(256), c->col_ptr.as<uint64_t>(), c->ent_row.as<uint32_t>(), c->ent_coef.as<uint32_t>(),
                        (uint32_t)c->ncols, c->const_begin, nnz, cursor.as<uint32_t>(), c->rv_ent.as<uint2>());
    BPG_LAUNCH((*this), k_rowview_long, dim3(cdiv(q, 256)), dim3(256), c->rv_ptr.as<uint32_t>(), (uint32_t)q, check_threshold, c->rv_long.as<uint32_t>());
    HIPCHK(hipGetLastError());
    c->rv_threshold = check_threshold; c->rv_built = true;
}

CheckReport Engine::check(DeviceCircuit *c, const uint8_t *v, uint64_t cap, uint64_t *rows_out, uint64_t *n_rows_out) {
    // every refusal first: nothing below this block runs for a refused call
    if (!c) throw std::invalid_argument("check: no circuit");
    if (!c->has_witness) throw R1CSException(R1CSError::MissingAssignment, "check: the circuit holds no witness (a verifier-side upload, or a template before assign / after a template batch)");
    if (!v && c->m && !c->is_template) throw std::invalid_argument("check: a plain upload does not keep its committed values: pass v");
    if (!v && c->m && !c->wit_v_set) throw std::invalid_argument("check: the template was uploaded with its witness and has had no assign: pass v");
    if (cap && !rows_out) throw std::invalid_argument("check: rows_out is null with cap > 0");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint64_t n = c->n, m = c->m, q = c->q;
    const scm *vals = c->wit_v.as<scm>();
    if (v && m) {                                   // the caller's values, reduced mod l as assign() reduces them; the circuit's own (wit_v) stay as they are
        I.small_sc.ensure(m * 32); I.chk_v.ensure(m * sizeof(scm));
        I.h2d(I.small_sc.p, v, m * 32);
        BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(m, 256)), dim3(256), I.small_sc.as<uint32_t>(), I.chk_v.as<scm>(), (uint32_t)m);
        vals = I.chk_v.as<scm>();
    }
    static const uint64_t kFresh[4] = {0, CHECK_NONE, 0, CHECK_NONE};
    I.chk_report.ensure(32);
    HIPCHK(hipMemcpyAsync(I.chk_report.p, kFresh, 32, hipMemcpyHostToDevice, I.st));
    unsigned long long *rep = I.chk_report.as<unsigned long long>();
    if (n) BPG_LAUNCH(I, k_check_mul, dim3(cdiv(n, 256)), dim3(256), c->aL.as<scm>(), c->aR.as<scm>(), c->aO.as<scm>(), (uint32_t)n, rep);
    const uint64_t nwords = check_bitmap_words(q);
    if (q) {
        if (!c->rv_built) I.rowview_build(c);
        I.chk_bitmap.ensure(nwords * 8);
        const CheckOperands P{c->aL.as<scm>(), c->aR.as<scm>(), c->aO.as<scm>(), vals, (uint32_t)n, (uint32_t)m};
        unsigned long long *bitmap = I.chk_bitmap.as<unsigned long long>();
        BPG_LAUNCH(I, k_check_rows, dim3(cdiv(q, 256)), dim3(256), c->rv_ptr.as<uint32_t>(), c->rv_ent.as<uint2>(), c->coef.as<scm>(), P, (uint32_t)q, c->rv_threshold, bitmap);
        // a wave per long row, one wave per SIMD of the device at most: how many rows are long stays on the device (rv_long[0])
        BPG_LAUNCH(I, k_check_rows_long, dim3(std::min<uint32_t>(cdiv(q, 4), std::max(1u, I.wit_waves / 4))), dim3(256), c->rv_ptr.as<uint32_t>(), c->rv_ent.as<uint2>(),
                   c->coef.as<scm>(), P, c->rv_long.as<uint32_t>(), bitmap);
        BPG_LAUNCH(I, k_check_count, dim3(cdiv(nwords, 256)), dim3(256), bitmap, (uint32_t)nwords, rep);
    }
    HIPCHK(hipGetLastError());
    uint64_t h[4];
    HIPCHK(hipMemcpyAsync(h, rep, 32, hipMemcpyDeviceToHost, I.st));        // the one read-back of a satisfied witness
    HIPCHK(hipStreamSynchronize(I.st));
    CheckReport R;
    R.bad_multipliers = h[0]; R.first_bad_multiplier = h[1]; R.bad_rows = h[2]; R.first_bad_row = h[3];
    uint64_t have = 0;
    if (R.bad_rows && cap) {                        // the bitmap, from the word of the first bad row on, a piece at a time until the list is full
        const uint64_t want = std::min(cap, R.bad_rows), PIECE = 1u << 17;
        std::vector<uint64_t> words;
        for (uint64_t w0 = check_word_of(R.first_bad_row); w0 < nwords && have < want; w0 += PIECE) {
            const uint64_t cnt = std::min(PIECE, nwords - w0);
            words.resize(cnt);
            HIPCHK(hipMemcpyAsync(words.data(), I.chk_bitmap.as<uint64_t>() + w0, cnt * 8, hipMemcpyDeviceToHost, I.st));
            HIPCHK(hipStreamSynchronize(I.st));
            have = check_bitmap_rows(words.data(), cnt, w0, q, want, rows_out, have);
        }
        if (have != want) throw std::logic_error("check: the violation bitmap and its count disagree");
    }
    if (n_rows_out) *n_rows_out = have;
    return R;
}
// ------------------------------------------------------------------------------------------------ a template repeated on the device (hip/k_repeat.cuh)
namespace {
// what the instance format and the device layout hold (check_instance, the 29-bit variable index, 32-bit entry and row indices, the packer's slot index)
void check_repeat_sizes(uint64_t count, uint64_t n, uint64_t m, uint64_t q, uint64_t nnz, uint64_t shared_coef, uint64_t n_params, uint64_t n_slots = 0, uint64_t n_in = 0) {
    if (count == 0) throw std::invalid_argument("template_repeat: count must be at least 1");
    auto over = [&](uint64_t a, uint64_t limit) { return a && count > (limit - 1) / a; };       // count * a >= limit
    if (over(n, 1ull << 27)) throw std::invalid_argument("template_repeat: count x n multipliers are too many (below 2^27)");
    if (over(m, 1ull << 29)) throw std::invalid_argument("template_repeat: count x m committed values exceed the 29-bit variable index");
    if (over(q, 1ull << 32)) throw std::invalid_argument("template_repeat: count x q constraints are too many (below 2^32)");
    if (over(nnz, 1ull << 32)) throw std::invalid_argument("template_repeat: count x nnz terms are too many (below 2^32)");
    if (over(3 * n + m, (1ull << 32) - 1)) throw std::invalid_argument("template_repeat: the repeated circuit has too many columns");
    if (over(n_params, (uint64_t)WIT_COEF_INDEX_MASK + 1 - std::min<uint64_t>(shared_coef, WIT_COEF_INDEX_MASK)))
        throw std::invalid_argument("template_repeat: count x n_params coefficient slots are too many");
    // a source with public inputs: shared + count (n_params + n_slots) coefficient indices below 2^30, count n_inputs below the 29-bit variable index
    if (n_slots && over(n_params + n_slots, (uint64_t)WIT_COEF_INDEX_MASK + 1 - std::min<uint64_t>(shared_coef, WIT_COEF_INDEX_MASK)))
        throw std::invalid_argument("template_repeat: count x (n_params + n_slots) coefficient slots are too many (shared + count x (" + std::to_string(n_params) + " + " +
                                    std::to_string(n_slots) + ") must stay below 2^30)");
    if (over(n_in, 1ull << 29)) throw std::invalid_argument("template_repeat: count x n_inputs public inputs exceed the 29-bit variable index");
}
}  // namespace

DeviceCircuit *Engine::repeat_template(DeviceCircuit *src, uint64_t count, bool with_inputs) {
    // every refusal first: nothing below this block runs for a refused call
    if (!src) throw std::invalid_argument("template_repeat: no circuit");
    if (!src->is_template) throw std::invalid_argument("template_repeat: the circuit is not a template (bpg_r1cs_upload_template)");
    if (src->rep_count) throw std::invalid_argument("template_repeat: the circuit is itself a repeat (repeat the template it was made from)");
    if (src->n_gates) throw std::invalid_argument("template_repeat: the template has gated variables (a repeat carries none yet: prove its items in a batch, bpg_r1cs_prove_template_batch_inputs)");
    if (src->n_in && !with_inputs) throw std::invalid_argument("template_repeat: the template has public inputs (a repeat carries none: prove its items in a batch, bpg_r1cs_prove_template_batch_inputs)");
    check_repeat_sizes(count, src->n, src->m, src->q, src->nnz, src->param_first, src->n_params, src->n_slots, src->n_in);
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint64_t K = count, n = K * src->n, m = K * src->m, q = K * src->q, nnz = K * src->nnz, ncols = 3 * n + m + 1;
    const uint64_t ncoef = src->param_first + K * (src->n_params + src->n_slots);
    const RepeatDims D{(uint32_t)src->n, (uint32_t)src->m, (uint32_t)src->q, (uint32_t)src->param_first, (uint32_t)src->n_params, (uint32_t)src->n_slots, (uint32_t)K};
    std::unique_ptr<DeviceCircuit> d(new DeviceCircuit());
    d->n = n; d->m = m; d->q = q; d->ncols = ncols; d->nnz = nnz; d->const_begin = K * src->const_begin; d->has_witness = false;
    d->owner = this;
    d->is_template = true; d->n_params = K * src->n_params; d->param_first = src->param_first; d->wit_level_ptr = src->wit_level_ptr;
    d->rep_count = K; d->rep_n = src->n; d->rep_m = src->m; d->n_ck = src->n_ck;
    d->aL.ensure(n * sizeof(scm)); d->aR.ensure(n * sizeof(scm)); d->aO.ensure(n * sizeof(scm));
    d->col_ptr.ensure((ncols + 1) * 8); d->ent_row.ensure((nnz ? nnz : 1) * 4); d->ent_coef.ensure((nnz ? nnz : 1) * 4);
    d->coef.ensure((ncoef ? ncoef : 1) * sizeof(scm));
    d->wit_stream.ensure(src->wit_stream.cap); d->wit_segs.ensure(src->wit_segs.cap); d->wit_v.ensure((m ? m : 1) * sizeof(scm));
    HIPCHK(hipMemcpyAsync(d->wit_stream.p, src->wit_stream.p, src->wit_stream.cap, hipMemcpyDeviceToDevice, I.st));
    HIPCHK(hipMemcpyAsync(d->wit_segs.p, src->wit_segs.p, src->wit_segs.cap, hipMemcpyDeviceToDevice, I.st));
    if (d->n_ck) {                                  // the source's checkpoints, per item: K n_ck values, item-major
        d->wit_ck_var.ensure(d->n_ck * 4); d->wit_ck.ensure(K * d->n_ck * sizeof(scm));
        HIPCHK(hipMemcpyAsync(d->wit_ck_var.p, src->wit_ck_var.p, d->n_ck * 4, hipMemcpyDeviceToDevice, I.st));
    }
    if (src->n_in) {                                // the source's inputs, per item: K n_in values and K n_slots derived slots, item-major, behind all parameter slots
        d->rep_in = src->n_in; d->n_in = K * src->n_in; d->n_slots = K * src->n_slots; d->slot_first = src->param_first + K * src->n_params;
        d->wit_in.ensure(d->n_in * sizeof(scm)); d->in_slots.ensure((src->n_slots ? src->n_slots : 1) * sizeof(InputSlot));
        if (src->n_slots) {                         // its own copy of the (input, coefficient index) pairs, and the one descriptor k_input_slots_join walks
            HIPCHK(hipMemcpyAsync(d->in_slots.p, src->in_slots.p, src->n_slots * sizeof(InputSlot), hipMemcpyDeviceToDevice, I.st));
            JoinPart P;
            std::memset(&P, 0, sizeof P);
            P.count = (uint32_t)K; P.n_in = (uint32_t)src->n_in; P.n_slots = (uint32_t)src->n_slots; P.base_dslot = (uint32_t)d->slot_first;
            d->join_desc.ensure(sizeof P);
            I.h2d(d->join_desc.p, &P, sizeof P);
            d->slot_parts = 1;
        }
    }
    const uint32_t gy = (uint32_t)std::min<uint64_t>(K, 1024);           // copies beyond the grid's y extent are a loop in the kernels
    BPG_LAUNCH(I, k_repeat_colptr, dim3(cdiv(3 * src->n + src->m + 1, 256), gy), dim3(256), src->col_ptr.as<uint64_t>(), D, (uint32_t)K, d->col_ptr.as<uint64_t>());
    if (src->nnz) BPG_LAUNCH(I, k_repeat_entries, dim3(cdiv(src->nnz, 256), gy), dim3(256), src->col_ptr.as<uint64_t>(), src->ent_row.as<uint32_t>(),
                             src->ent_coef.as<uint32_t>(), D, (uint32_t)K, src->nnz, d->ent_row.as<uint32_t>(), d->ent_coef.as<uint32_t>());
    if (ncoef) BPG_LAUNCH(I, k_repeat_coef, dim3(cdiv(ncoef, 256)), dim3(256), src->coef.as<scm>(), D, (uint32_t)K, d->coef.as<scm>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
    return d.release();
}

namespace {
// the rows of the repeat from the template's rows with their parameter slots: what k_repeat_* leave in HBM, row-major
FlatCircuit repeat_rows(const TemplatePlan &T, uint64_t count, const uint64_t *caps = nullptr) {
    const FlatCircuit &s = T.slotted;
    const uint64_t q = s.row_ptr.size() - 1, nnz = s.term_var.size();
    const uint64_t n_slots = T.in_slots.size();
    check_repeat_sizes(count, s.n, s.m, q, nnz, T.param_first, T.n_params, n_slots, T.n_inputs);
    if (caps) {                                     // the caller's buffers against the size formulas, before a row is made
        if (caps[0] < count * q + 1) throw std::invalid_argument("template_repeat_instance: row_ptr too short (" + std::to_string(count * q + 1) + " entries needed)");
        if (caps[1] < count * nnz) throw std::invalid_argument("template_repeat_instance: term_var / term_coef too short (" + std::to_string(count * nnz) + " entries needed)");
        if (caps[2] < T.param_first + count * (T.n_params + n_slots))
            throw std::invalid_argument("template_repeat_instance: coef too short (" + std::to_string(T.param_first + count * (T.n_params + n_slots)) + " scalars needed)");
    }
    const RepeatDims D{(uint32_t)s.n, (uint32_t)s.m, (uint32_t)q, (uint32_t)T.param_first, (uint32_t)T.n_params, (uint32_t)n_slots, (uint32_t)count};
    FlatCircuit f; f.n = count * s.n; f.m = count * s.m;
    f.row_ptr.reserve(count * q + 1); f.term_var.reserve(count * nnz); f.term_coef.reserve(count * nnz);
    for (uint64_t k = 0; k < count; k++)
        for (uint64_t r = 0; r < q; r++) {
            for (uint64_t t = s.row_ptr[r]; t < s.row_ptr[r + 1]; t++) {
                uint32_t var, coef, row;
                repeat_map(D, (uint32_t)k, s.term_var[t], s.term_coef[t], (uint32_t)r, var, coef, row);
                if (row + 1 != f.row_ptr.size()) throw std::logic_error("template_repeat: row map out of step");
                f.term_var.push_back(var); f.term_coef.push_back(coef);
            }
            f.row_ptr.push_back(f.term_var.size());
        }
    f.coef.assign(s.coef.begin(), s.coef.begin() + 32 * T.param_first);
    const auto par_end = s.coef.begin() + 32 * (T.param_first + T.n_params);
    for (uint64_t k = 0; k < count; k++) f.coef.insert(f.coef.end(), s.coef.begin() + 32 * T.param_first, par_end);
    for (uint64_t k = 0; k < count; k++) f.coef.insert(f.coef.end(), par_end, s.coef.end());       // the derived slots of a source with inputs, as they stand
    return f;
}
// what the eval hooks fill a_L, a_R, a_O with before a level runs
const uint8_t kEvalPoison[32] = {0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a,
                                 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x0a};
}  // namespace
// TEST HOOK (bpg_test_template_repeat_inputs_instance): template_repeat_instance_host for a program with public inputs - the rows as k_repeat_* leave them, the
// parameter slots as an assign of param_values leaves them (null: as the template's rows carry them) and item k's derived slots as k_input_slots_join fills them
// from input_values (count x n_inputs x 32, item-major): the same lane function, compiled for the host, over the same one-part descriptor.  caps: the caller's
// row_ptr / term / coef capacities, checked against the size formulas before anything is built.
FlatCircuit Engine::template_repeat_inputs_instance_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *param_values, const uint8_t *input_values,
                                                         const uint64_t caps[3]) {
    if (p.n_inputs && !input_values) throw std::invalid_argument("template_repeat_inputs_instance: the program has public inputs and no values were given for them");
    FlatView rows = c; rows.aL = rows.aR = rows.aO = nullptr;
    const TemplatePlan T = plan_template(rows, p);
    FlatCircuit f = repeat_rows(T, count, caps);
    if (param_values)
        for (uint64_t i = 0; i < count * T.n_params; i++) Scalar::from_bytes_mod_order(param_values + 32 * i).to_bytes(&f.coef[32 * (T.param_first + i)]);
    const uint64_t n_slots = T.in_slots.size();
    if (n_slots) {
        JoinPart P;
        std::memset(&P, 0, sizeof P);
        P.count = (uint32_t)count; P.n_in = (uint32_t)T.n_inputs; P.n_slots = (uint32_t)n_slots; P.base_dslot = (uint32_t)(T.param_first + count * T.n_params);
        std::vector<scm> coef = scalars_from_bytes(f.coef.data(), f.coef.size() / 32);
        const std::vector<scm> in = scalars_from_bytes(input_values, count * T.n_inputs);
        for (uint64_t t = count * n_slots; t-- > 0;) join_input_slot_lane(&P, 1, t, reinterpret_cast<const uint32_t *>(T.in_slots.data()), in.data(), coef.data());
        coef.resize(f.coef.size() / 32);
        scalars_to_bytes(coef, f.coef.data());
    }
    return f;
}
// TEST HOOK (bpg_test_template_eval_repeat_inputs): k_witness_eval_repeat on the host for a source with inputs and / or checkpoints, under the discipline of
// template_eval_checkpointed_host - poisoned vectors, the segments of every level and the items of every segment in REVERSE order, then the step of
// k_witness_ck_verify; returns the first mismatching flat checkpoint index (item-major) or CHECKPOINTS_HOLD
uint64_t Engine::template_eval_repeat_inputs_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, const uint8_t *ck_values,
                                                  const uint8_t *input_values, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out) {
    if (p.n_inputs && !input_values) throw std::invalid_argument("template_eval_repeat_inputs: the program has public inputs and no values were given for them");
    if (p.n_ck && !ck_values) throw std::invalid_argument("template_eval_repeat_inputs: the program has checkpoints and no values were given for them");
    FlatView rows = c; rows.aL = rows.aR = rows.aO = nullptr;
    const TemplatePlan T = plan_template(rows, p);
    const PackedWitnessProgram &P = T.packed;
    check_repeat_sizes(count, c.n, c.m, c.q, T.slotted.term_var.size(), T.param_first, T.n_params, T.in_slots.size(), T.n_inputs);
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, count * c.m), ck = scalars_from_bytes(ck_values, count * p.n_ck);
    const std::vector<scm> in = scalars_from_bytes(input_values, count * p.n_inputs);
    const scm poison = scalars_from_bytes(kEvalPoison, 1)[0];
    std::vector<scm> aL(count * c.n, poison), aR(count * c.n, poison), aO(count * c.n, poison);
    const std::vector<uint32_t> &lp = T.schedule.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l + 1]; s-- > lp[l];)
            for (uint64_t k = count; k-- > 0;)
                witness_eval_repeat_lane(P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data(), (uint32_t)c.n, (uint32_t)c.m, k,
                                         aL.data(), aR.data(), aO.data(), p.n_ck ? ck.data() : nullptr, (uint32_t)p.n_ck, p.n_inputs ? in.data() : nullptr, (uint32_t)p.n_inputs);
    uint64_t first = CHECKPOINTS_HOLD;
    for (uint64_t t = count * p.n_ck; t-- > 0;) {
        const size_t b = (size_t)(t / p.n_ck) * c.n;
        if (!witness_ck_holds(p.ck_var[t % p.n_ck], ck[t], aL.data() + b, aR.data() + b, aO.data() + b)) first = t;
    }
    aL.resize(count * c.n); aR.resize(count * c.n); aO.resize(count * c.n);
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
    return first;
}
// TEST HOOK (bpg_test_template_repeat_instance): the repeated instance, row-major, as it stands after an assign of param_values (count x n_params x 32,
// item-major, reduced as assign() reduces them; null: the slots keep the constants the template's rows carried)
FlatCircuit Engine::template_repeat_instance_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *param_values) {
    const TemplatePlan T = plan_template(c, p);
    FlatCircuit f = repeat_rows(T, count);
    if (param_values)
        for (uint64_t i = 0; i < count * T.n_params; i++) Scalar::from_bytes_mod_order(param_values + 32 * i).to_bytes(&f.coef[32 * (T.param_first + i)]);
    return f;
}
// TEST HOOK (bpg_test_template_eval_repeat): k_witness_eval_repeat on the host - one pass per level of the SOURCE, per segment every item, into the repeat's
// layout (count x n scalars per vector, no padding rows); v: count x m x 32
void Engine::template_eval_repeat_host(const FlatView &c, const WitnessProgramView &p, uint64_t count, const uint8_t *v, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out) {
    const TemplatePlan T = plan_template(c, p);
    const PackedWitnessProgram &P = T.packed;
    check_repeat_sizes(count, c.n, c.m, c.q, T.slotted.term_var.size(), T.param_first, T.n_params);
    const std::vector<scm> coef = scalars_from_bytes(c.coef, c.ncoef), vv = scalars_from_bytes(v, count * c.m);
    std::vector<scm> aL(count * c.n), aR(count * c.n), aO(count * c.n);
    const std::vector<uint32_t> &lp = T.schedule.level_ptr;
    for (size_t l = 0; l + 1 < lp.size(); l++)
        for (uint32_t s = lp[l]; s < lp[l + 1]; s++)
            for (uint64_t k = 0; k < count; k++)
                witness_eval_repeat_lane(P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data(), (uint32_t)c.n, (uint32_t)c.m, k,
                                         aL.data(), aR.data(), aO.data());
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
}

// ------------------------------------------------------------------------------------------------ templates joined on the device (hip/k_join.cuh)
namespace {
// The refusals every road to a join shares: parts holds (n, m, q, shared, n_params, n_ck, count) and sec[5] = the terms of each part's template.  The totals
// stay inside what the instance format and the device layout hold (check_repeat_sizes, summed over the parts).
void check_join_sizes(const std::vector<JoinPart> &parts) {
    if (parts.empty()) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
    if (parts.size() > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(parts.size()) + "; at most 256)");
    uint64_t n = 0, m = 0, q = 0, nnz = 0, cols = 0, coefs = 0, ck = 0, ins = 0;
    // total + count * a stays below limit
    auto add = [](uint64_t &total, uint64_t a, uint64_t count, uint64_t limit) { if (a && count > (limit - 1 - total) / a) return false; total += count * a; return true; };
    for (size_t p = 0; p < parts.size(); p++) {
        const JoinPart &P = parts[p];
        const std::string at = "template_join: part " + std::to_string(p) + ": ";
        if (P.count == 0) throw std::invalid_argument(at + "count must be at least 1");
        if (!add(n, P.n, P.count, 1ull << 27)) throw std::invalid_argument(at + "the joined multipliers are too many (below 2^27)");
        if (!add(m, P.m, P.count, 1ull << 29)) throw std::invalid_argument(at + "the joined committed values exceed the 29-bit variable index");
        if (!add(q, P.q, P.count, 1ull << 32)) throw std::invalid_argument(at + "the joined constraints are too many (below 2^32)");
        if (!add(nnz, P.sec[5], P.count, 1ull << 32)) throw std::invalid_argument(at + "the joined terms are too many (below 2^32)");
        if (!add(cols, 3 * (uint64_t)P.n + P.m, P.count, (1ull << 32) - 1)) throw std::invalid_argument(at + "the joined circuit has too many columns");
        if (!add(coefs, P.shared, 1, (uint64_t)WIT_COEF_INDEX_MASK + 1) || !add(coefs, P.n_params, P.count, (uint64_t)WIT_COEF_INDEX_MASK + 1))
            throw std::invalid_argument(at + "the joined coefficient slots are too many");
        if (!add(ck, P.n_ck, P.count, 1ull << 32)) throw std::invalid_argument(at + "the joined checkpoints are too many (below 2^32)");
        if (!add(coefs, P.n_slots, P.count, (uint64_t)WIT_COEF_INDEX_MASK + 1)) throw std::invalid_argument(at + "the joined coefficient slots are too many (derived slots of the public inputs included)");
        if (!add(ins, P.n_in, P.count, 1ull << 29)) throw std::invalid_argument(at + "the joined public inputs exceed the 29-bit variable index");
    }
}
// the block table of a join's assign(): per level, per part that has the level, per segment of it, a block for every 64 items - (part, segment in the joined
// list, first item, -).  levels[p]: the part's wit_level_ptr.
void join_block_table(const std::vector<JoinPart> &parts, const std::vector<const std::vector<uint32_t> *> &levels, std::vector<uint32_t> &table, std::vector<uint32_t> &level_ptr) {
    size_t nlev = 0;
    for (const auto *lp : levels) nlev = std::max(nlev, lp->empty() ? (size_t)0 : lp->size() - 1);
    table.clear(); level_ptr.assign(1, 0);
    for (size_t l = 0; l < nlev; l++) {
        for (size_t p = 0; p < parts.size(); p++) {
            const std::vector<uint32_t> &lp = *levels[p];
            if (l + 1 >= lp.size()) continue;
            for (uint32_t s = lp[l]; s < lp[l + 1]; s++)
                for (uint64_t first = 0; first < parts[p].count; first += 64) { table.push_back((uint32_t)p); table.push_back(parts[p].seg_first + s); table.push_back((uint32_t)first); table.push_back(0); }
        }
        if (table.size() / 4 >= (1ull << 31)) throw std::invalid_argument("template_join: too many (segment, 64 items) blocks in one assign");
        level_ptr.push_back((uint32_t)(table.size() / 4));
    }
}
}  // namespace

DeviceCircuit *Engine::join_templates(const std::vector<std::pair<DeviceCircuit *, uint64_t>> &src, bool with_inputs) {
    // every refusal first: nothing below this block runs for a refused call
    if (src.empty()) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
    if (src.size() > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(src.size()) + "; at most 256)");
    std::vector<JoinPart> parts(src.size());
    for (size_t p = 0; p < src.size(); p++) {
        const DeviceCircuit *s = src[p].first;
        const std::string at = "template_join: part " + std::to_string(p) + ": ";
        if (!s) throw std::invalid_argument(at + "no circuit");
        if (src[p].second == 0) throw std::invalid_argument(at + "count must be at least 1");
        if (!s->is_template) throw std::invalid_argument(at + "the circuit is not a template (bpg_r1cs_upload_template)");
        if (s->rep_count) throw std::invalid_argument(at + "the circuit is itself a repeat (name the template it was made from and a count)");
        if (!s->join_parts.empty()) throw std::invalid_argument(at + "the circuit is itself a join (name its parts instead)");
        if (s->n_gates) throw std::invalid_argument(at + "the template has gated variables (a join carries none yet)");
        if (s->n_in && !with_inputs) throw std::invalid_argument(at + "the template has public inputs (a join carries none)");
        if (s->device != device_) throw std::invalid_argument(at + "the circuit lives on the device of another context");
        if (src[p].second >= (1ull << 32)) throw std::invalid_argument(at + "the joined multipliers are too many (below 2^27)");
        JoinPart &P = parts[p];
        std::memset(&P, 0, sizeof P);
        P.n = (uint32_t)s->n; P.m = (uint32_t)s->m; P.q = (uint32_t)s->q; P.shared = (uint32_t)s->param_first; P.n_params = (uint32_t)s->n_params;
        P.n_ck = (uint32_t)s->n_ck; P.count = (uint32_t)src[p].second;
        P.n_in = (uint32_t)s->n_in; P.n_slots = (uint32_t)s->n_slots;
        P.sec[4] = s->const_begin; P.sec[5] = s->nnz;
    }
    check_join_sizes(parts);
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    // the sections of every part's entry list: three column pointers each (the constants column's start and the total are known here)
    for (size_t p = 0; p < parts.size(); p++)
        for (uint32_t k = 1; k <= 3; k++)
            HIPCHK(hipMemcpyAsync(&parts[p].sec[k], src[p].first->col_ptr.as<uint64_t>() + (size_t)k * parts[p].n, 8, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    const JoinTotals T = join_fill_bases(parts.data(), parts.size());
    uint64_t nsegs = 0, nwords = 0, nckv = 0;
    std::vector<const std::vector<uint32_t> *> levels;
    for (size_t p = 0; p < parts.size(); p++) {
        parts[p].seg_first = (uint32_t)nsegs; parts[p].stream_first = (uint32_t)nwords; parts[p].ck_var_first = (uint32_t)nckv;
        nsegs += src[p].first->wit_segs.cap / sizeof(WitnessSegment); nwords += src[p].first->wit_stream.cap / 4; nckv += parts[p].n_ck;
        levels.push_back(&src[p].first->wit_level_ptr);
    }
    if (nsegs >= (1ull << 32) || nwords >= (1ull << 32)) throw std::invalid_argument("template_join: the parts' witness programs are too long together");
    std::unique_ptr<DeviceCircuit> d(new DeviceCircuit());
    std::vector<uint32_t> table;
    join_block_table(parts, levels, table, d->join_level_ptr);
    const uint64_t n = T.n, m = T.m, nnz = T.nnz, ncols = 3 * n + m + 1, ncoef = T.shared + T.n_params + T.n_slots;
    d->device = device_; d->owner = this;
    d->n = n; d->m = m; d->q = T.q; d->ncols = ncols; d->nnz = nnz; d->const_begin = parts[0].sec_base[4]; d->has_witness = false;
    d->is_template = true; d->n_params = T.n_params; d->param_first = T.shared; d->n_ck = T.n_ck;
    d->aL.ensure((n ? n : 1) * sizeof(scm)); d->aR.ensure((n ? n : 1) * sizeof(scm)); d->aO.ensure((n ? n : 1) * sizeof(scm));
    d->col_ptr.ensure((ncols + 1) * 8); d->ent_row.ensure((nnz ? nnz : 1) * 4); d->ent_coef.ensure((nnz ? nnz : 1) * 4);
    d->coef.ensure((ncoef ? ncoef : 1) * sizeof(scm));
    d->wit_stream.ensure((nwords ? nwords : 1) * 4); d->wit_segs.ensure((nsegs ? nsegs : 1) * sizeof(WitnessSegment)); d->wit_v.ensure((m ? m : 1) * sizeof(scm));
    if (T.n_ck) { d->wit_ck_var.ensure(nckv * 4); d->wit_ck.ensure(T.n_ck * sizeof(scm)); }
    if (T.n_in) {                                   // the joined inputs, the derived slots behind all parameter slots, and the parts' (input, coefficient index) pairs
        uint64_t pairs = 0;
        for (const JoinPart &P : parts) pairs += P.n_slots;
        d->n_in = T.n_in; d->n_slots = T.n_slots; d->slot_first = T.shared + T.n_params; d->slot_parts = T.n_slots ? (uint32_t)parts.size() : 0;
        d->wit_in.ensure(T.n_in * sizeof(scm)); d->in_slots.ensure((pairs ? pairs : 1) * sizeof(InputSlot));
    }
    d->join_desc.ensure(parts.size() * sizeof(JoinPart)); d->join_blocks.ensure((table.empty() ? 4 : table.size()) * 4);
    I.h2d(d->join_desc.p, parts.data(), parts.size() * sizeof(JoinPart));
    if (!table.empty()) I.h2d(d->join_blocks.p, table.data(), table.size() * 4);
    const JoinPart *desc = d->join_desc.as<JoinPart>();
    for (size_t p = 0; p < parts.size(); p++) {
        const DeviceCircuit *s = src[p].first;
        const JoinPart &P = parts[p];
        if (s->wit_stream.cap) HIPCHK(hipMemcpyAsync(d->wit_stream.as<uint32_t>() + P.stream_first, s->wit_stream.p, s->wit_stream.cap, hipMemcpyDeviceToDevice, I.st));
        if (s->wit_segs.cap) HIPCHK(hipMemcpyAsync(d->wit_segs.as<WitnessSegment>() + P.seg_first, s->wit_segs.p, s->wit_segs.cap, hipMemcpyDeviceToDevice, I.st));
        if (P.n_ck) HIPCHK(hipMemcpyAsync(d->wit_ck_var.as<uint32_t>() + P.ck_var_first, s->wit_ck_var.p, (size_t)P.n_ck * 4, hipMemcpyDeviceToDevice, I.st));
        if (P.n_slots) HIPCHK(hipMemcpyAsync(d->in_slots.as<InputSlot>() + P.slot_list_first, s->in_slots.p, (size_t)P.n_slots * sizeof(InputSlot), hipMemcpyDeviceToDevice, I.st));
        const uint32_t gy = std::min<uint32_t>(P.count, 1024);              // copies beyond the grid's y extent are a loop in the kernels
        BPG_LAUNCH(I, k_join_colptr, dim3(cdiv(3 * s->n + s->m + 1, 256), gy), dim3(256), s->col_ptr.as<uint64_t>(), desc, (uint32_t)p, (uint32_t)n, (uint32_t)m, nnz,
                   d->col_ptr.as<uint64_t>());
        if (s->nnz) BPG_LAUNCH(I, k_join_entries, dim3(cdiv(s->nnz, 256), gy), dim3(256), s->ent_row.as<uint32_t>(), s->ent_coef.as<uint32_t>(), desc, (uint32_t)p,
                               d->ent_row.as<uint32_t>(), d->ent_coef.as<uint32_t>());
        const uint64_t pc = (uint64_t)P.shared + (uint64_t)P.count * ((uint64_t)P.n_params + P.n_slots);
        if (pc) BPG_LAUNCH(I, k_join_coef, dim3(cdiv(pc, 256)), dim3(256), s->coef.as<scm>(), desc, (uint32_t)p, d->coef.as<scm>());
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
    d->join_parts = std::move(parts);
    return d.release();
}
bool Engine::is_join(const DeviceCircuit *d) { return d && !d->join_parts.empty(); }
bool Engine::join_checkpoint_place(const DeviceCircuit *d, uint64_t flat, uint64_t *part, uint64_t *item, uint64_t *ck) {
    if (!is_join(d) || flat >= d->n_ck) return false;
    uint32_t p, i, c;
    join_ck_place(d->join_parts.data(), (uint32_t)d->join_parts.size(), flat, p, i, c);
    *part = p; *item = i; *ck = c;
    return true;
}

namespace {
// the parts of a join as the host hooks get them: every part's plan, and the descriptors with their bases (no sections: the hooks work on rows)
struct HostJoin { std::vector<TemplatePlan> plans; std::vector<JoinPart> parts; JoinTotals T; };
HostJoin plan_join(const std::vector<Engine::JoinSource> &src) {
    HostJoin J;
    if (src.empty()) throw std::invalid_argument("template_join: no parts (n_parts must be at least 1)");
    if (src.size() > 256) throw std::invalid_argument("template_join: too many parts (" + std::to_string(src.size()) + "; at most 256)");
    J.parts.resize(src.size());
    for (size_t p = 0; p < src.size(); p++) {
        if (src[p].count == 0 || src[p].count >= (1ull << 32))
            throw std::invalid_argument("template_join: part " + std::to_string(p) + (src[p].count ? ": the joined multipliers are too many (below 2^27)" : ": count must be at least 1"));
        FlatView rows = src[p].c;
        if (src[p].p.n_inputs) rows.aL = rows.aR = rows.aO = nullptr;       // (a part with inputs: the hooks evaluate, a witness in the instance is not looked at)
        J.plans.push_back(Engine::plan_template(rows, src[p].p));
        const TemplatePlan &T = J.plans.back();
        JoinPart &P = J.parts[p];
        std::memset(&P, 0, sizeof P);
        P.n = (uint32_t)T.slotted.n; P.m = (uint32_t)T.slotted.m; P.q = (uint32_t)(T.slotted.row_ptr.size() - 1); P.shared = (uint32_t)T.param_first;
        P.n_params = (uint32_t)T.n_params; P.n_ck = (uint32_t)T.ck_var.size(); P.count = (uint32_t)src[p].count;
        P.n_in = (uint32_t)T.n_inputs; P.n_slots = (uint32_t)T.in_slots.size();
        P.sec[5] = T.slotted.term_var.size();
    }
    check_join_sizes(J.parts);
    J.T = join_fill_bases(J.parts.data(), J.parts.size());
    return J;
}
}  // namespace
// TEST HOOK (bpg_test_template_join_instance): the joined instance, row-major - what k_join_* leave in HBM - as it stands after an assign of param_values (the
// joined slots' values in order; null: every slot keeps the constant its part's rows carried)
FlatCircuit Engine::template_join_instance_host(const std::vector<JoinSource> &src, const uint8_t *param_values, const uint8_t *input_values, const uint64_t *caps) {
    const HostJoin J = plan_join(src);
    if (J.T.n_in && !input_values) throw std::invalid_argument("template_join_inputs_instance: a part has public inputs and no values were given for them");
    if (caps) {                                     // the caller's buffers against the size formulas, before a row is made
        if (caps[0] < J.T.q + 1) throw std::invalid_argument("template_join_instance: row_ptr too short (" + std::to_string(J.T.q + 1) + " entries needed)");
        if (caps[1] < J.T.nnz) throw std::invalid_argument("template_join_instance: term_var / term_coef too short (" + std::to_string(J.T.nnz) + " entries needed)");
        if (caps[2] < J.T.shared + J.T.n_params + J.T.n_slots)
            throw std::invalid_argument("template_join_instance: coef too short (" + std::to_string(J.T.shared + J.T.n_params + J.T.n_slots) + " scalars needed)");
    }
    FlatCircuit f; f.n = J.T.n; f.m = J.T.m;
    f.row_ptr.reserve(J.T.q + 1); f.term_var.reserve(J.T.nnz); f.term_coef.reserve(J.T.nnz);
    f.coef.assign(32 * (J.T.shared + J.T.n_params + J.T.n_slots), 0);
    for (size_t p = 0; p < J.parts.size(); p++) {
        const FlatCircuit &s = J.plans[p].slotted;
        const JoinPart &P = J.parts[p];
        for (uint64_t k = 0; k < P.count; k++)
            for (uint64_t r = 0; r < P.q; r++) {
                for (uint64_t t = s.row_ptr[r]; t < s.row_ptr[r + 1]; t++) {
                    uint32_t var, coef, row;
                    join_map(J.parts.data(), (uint32_t)p, (uint32_t)k, s.term_var[t], s.term_coef[t], (uint32_t)r, var, coef, row);
                    if (row + 1 != f.row_ptr.size()) throw std::logic_error("template_join: row map out of step");
                    f.term_var.push_back(var); f.term_coef.push_back(coef);
                }
                f.row_ptr.push_back(f.term_var.size());
            }
        std::memcpy(&f.coef[32 * (size_t)P.base_shared], s.coef.data(), 32 * (size_t)P.shared);
        for (uint64_t k = 0; k < P.count; k++)
            if (P.n_params) std::memcpy(&f.coef[32 * ((size_t)P.base_slot + k * P.n_params)], s.coef.data() + 32 * (size_t)P.shared, 32 * (size_t)P.n_params);
    }
    if (param_values)
        for (uint64_t i = 0; i < J.T.n_params; i++) Scalar::from_bytes_mod_order(param_values + 32 * i).to_bytes(&f.coef[32 * (J.T.shared + i)]);
    if (J.T.n_slots) {                              // the derived slots as k_input_slots_join fills them: the same lane function over the same descriptors
        std::vector<uint32_t> pairs;
        for (const TemplatePlan &T : J.plans) for (const InputSlot &sl : T.in_slots) { pairs.push_back(sl.p); pairs.push_back(sl.ci); }
        std::vector<scm> coef = scalars_from_bytes(f.coef.data(), f.coef.size() / 32);
        const std::vector<scm> in = scalars_from_bytes(input_values, J.T.n_in);
        for (uint64_t t = J.T.n_slots; t-- > 0;) join_input_slot_lane(J.parts.data(), (uint32_t)J.parts.size(), t, pairs.data(), in.data(), coef.data());
        scalars_to_bytes(coef, f.coef.data());
    }
    return f;
}
// TEST HOOK (bpg_test_template_eval_join): k_witness_eval_join and k_witness_ck_verify_join on the host, in the order that shows what in-order execution
// hides - poisoned vectors, the levels in order and within a level the parts and their segments in REVERSE order, then the verify step; returns the first
// mismatch.  v: the joined committed values; ck_values: the joined checkpoint values (null when no part has any)
uint64_t Engine::template_eval_join_host(const std::vector<JoinSource> &src, const uint8_t *v, const uint8_t *ck_values, uint8_t *aL_out, uint8_t *aR_out, uint8_t *aO_out,
                                         const uint8_t *input_values) {
    const HostJoin J = plan_join(src);
    if (J.T.n_in && !input_values) throw std::invalid_argument("template_eval_join_inputs: a part has public inputs and no values were given for them");
    const std::vector<scm> in = scalars_from_bytes(input_values, J.T.n_in);
    if (J.T.n_ck && !ck_values) throw std::invalid_argument("template_eval_join: a part has checkpoints and no values were given for them");
    std::vector<scm> coef(J.T.shared ? J.T.shared : 1);
    size_t nlev = 0;
    for (size_t p = 0; p < J.parts.size(); p++) {
        const std::vector<scm> c = scalars_from_bytes(src[p].c.coef, J.parts[p].shared);
        std::copy(c.begin(), c.begin() + J.parts[p].shared, coef.begin() + J.parts[p].base_shared);
        nlev = std::max(nlev, J.plans[p].schedule.level_ptr.size() - 1);
    }
    const std::vector<scm> vv = scalars_from_bytes(v, J.T.m), ck = scalars_from_bytes(ck_values, J.T.n_ck);
    static const uint8_t kPoison[32] = {0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a,
                                        0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x5a, 0xa5, 0x0a};
    const scm poison = scalars_from_bytes(kPoison, 1)[0];
    std::vector<scm> aL(J.T.n, poison), aR(J.T.n, poison), aO(J.T.n, poison);
    for (size_t l = 0; l < nlev; l++)
        for (size_t p = J.parts.size(); p-- > 0;) {
            const std::vector<uint32_t> &lp = J.plans[p].schedule.level_ptr;
            const PackedWitnessProgram &P = J.plans[p].packed;
            if (l + 1 >= lp.size()) continue;
            for (uint32_t s = lp[l + 1]; s-- > lp[l];)
                for (uint64_t k = J.parts[p].count; k-- > 0;)
                    witness_eval_join_lane(J.parts[p], P.segs[s].first, P.segs[s].count, P.stream.data() + P.segs[s].stream, coef.data(), vv.data(), k,
                                           aL.data(), aR.data(), aO.data(), J.T.n_ck ? ck.data() : nullptr, J.T.n_in ? in.data() : nullptr);
        }
    uint64_t first = CHECKPOINTS_HOLD;
    for (uint64_t t = J.T.n_ck; t-- > 0;) {
        uint32_t p, item, c;
        join_ck_place(J.parts.data(), (uint32_t)J.parts.size(), t, p, item, c);
        const size_t b = (size_t)J.parts[p].base_n + (size_t)item * J.parts[p].n;
        if (!witness_ck_holds(J.plans[p].ck_var[c], ck[t], aL.data() + b, aR.data() + b, aO.data() + b)) first = t;
    }
    scalars_to_bytes(aL, aL_out); scalars_to_bytes(aR, aR_out); scalars_to_bytes(aO, aO_out);
    return first;
}

// ------------------------------------------------------------------------------------------------ equal-scalar merging of A_I, A_O (hip/k_merge.cuh)
// Built once per uploaded witness, at its first prove() on the bucket-method path (the generator tables must exist; upload() may precede them).  Cost at
// n = 993,384: a hash-table pass over the scalars, two scans over the table, one point addition per merged-away term and a batched normalisation.
void Engine::Impl::merge_build(DeviceCircuit::MergeSet &M, const scm *A, const ge_niels *PA, uint32_t nA, const scm *B, const ge_niels *PB, uint32_t nB) {
    const uint32_t nterms = nA + nB;
    M.groups = 0; M.skipped = 0;
    if (nterms < 2) return;
    MergeTerms T; T.A = A; T.B = B; T.PA = PA; T.PB = PB; T.nA = nA; T.nterms = nterms;
    const uint32_t lgslots = ceil_log2((uint64_t)2 * nterms), slots = 1u << lgslots;        // load <= 1/2
    const uint32_t nblk = cdiv(slots, SCAN_CHUNK);
    // workspace out of the arena (no MSM of this context is in flight: prove() calls this before its first launch)
    const size_t words = (size_t)7 * slots + 2 * (size_t)nterms + (size_t)nterms / 2 + 8;
    arena.ensure(words * 4); blocksum.ensure((size_t)(nblk + 1) * 4);
    uint32_t *rep = arena.as<uint32_t>(), *count = rep + slots, *msize = count + slots, *gcount = msize + slots, *moff = gcount + slots, *goff = moff + slots + 1,
             *fill = goff + slots + 1, *slot_of = fill + slots, *members = slot_of + nterms, *gslot = members + nterms;
    const uint32_t wA = (nA + 31) / 32, wB = (nB + 31) / 32;
    M.skipA.ensure((size_t)std::max(wA, 1u) * 4); M.skipB.ensure((size_t)std::max(wB, 1u) * 4);
    HIPCHK(hipMemsetAsync(rep, 0xff, (size_t)slots * 4, st));
    HIPCHK(hipMemsetAsync(count, 0, (size_t)slots * 4, st));
    HIPCHK(hipMemsetAsync(M.skipA.p, 0, (size_t)std::max(wA, 1u) * 4, st)); HIPCHK(hipMemsetAsync(M.skipB.p, 0, (size_t)std::max(wB, 1u) * 4, st));
    BPG_LAUNCH((*this), k_merge_insert, dim3(cdiv(nterms, 256)), dim3(256), T, rep, count, slot_of, lgslots);
    BPG_LAUNCH((*this), k_merge_plan, dim3(cdiv(slots, 256)), dim3(256), count, msize, gcount, slots);
    auto scan = [&](uint32_t *in, uint32_t *out) {        // exclusive scan of in[0..slots) -> out[0..slots], out[slots] = total; `fill` is the scan's scratch cursor
        BPG_LAUNCH((*this), k_scan_blocksums, dim3(nblk), dim3(256), in, slots, blocksum.as<uint32_t>());
        BPG_LAUNCH((*this), k_scan_apply, dim3(nblk), dim3(256), in, slots, blocksum.as<uint32_t>(), out, fill);
    };
    scan(msize, moff); scan(gcount, goff);
    HIPCHK(hipGetLastError());
    uint32_t tot[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&tot[0], moff + slots, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot[1], goff + slots, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint32_t skipped = tot[0], groups = tot[1];
    if (groups == 0 || skipped > nterms || groups > nterms / 2) return;        // (a group has at least two of the terms)
    HIPCHK(hipMemsetAsync(fill, 0, (size_t)slots * 4, st));
    M.sc.ensure((size_t)groups * sizeof(scm)); M.pts.ensure((size_t)groups * sizeof(ge_niels));
    scratch_ext.ensure((size_t)groups * sizeof(ge_ext));
    BPG_LAUNCH((*this), k_merge_groups, dim3(cdiv(slots, 256)), dim3(256), count, goff, gslot, slots);
    BPG_LAUNCH((*this), k_merge_members, dim3(cdiv(nterms, 256)), dim3(256), T, slot_of, count, moff, fill, members, M.skipA.as<uint32_t>(), M.skipB.as<uint32_t>());
    BPG_LAUNCH((*this), k_merge_sum, dim3(cdiv(groups, 64)), dim3(64), T, count, moff, goff, gslot, members, groups, scratch_ext.as<ge_ext>(), M.sc.as<scm>());
    BPG_LAUNCH((*this), k_normalize_niels, dim3(cdiv(cdiv(groups, NORM_K), 256)), dim3(256), scratch_ext.as<ge_ext>(), M.pts.as<ge_niels>(), groups);
    HIPCHK(hipGetLastError());
    if (merge_equal != 2) HIPCHK(hipStreamSynchronize(st));                // (redone in every proof: the sums that follow are queued on the same stream, no wait)
    M.groups = groups; M.skipped = skipped;
}
void Engine::Impl::merge_witness(DeviceCircuit *c, const ge_niels *Gtab, const ge_niels *Htab) {
    if (c->merge_tried) return;
    c->merge_tried = true;
    const uint32_t n = (uint32_t)c->n;
    if (!merge_equal || n < 2) return;
    const double t0 = now_ms();
    merge_build(c->mI, c->aL.as<scm>(), Gtab, n, c->aR.as<scm>(), Htab, n);
    merge_build(c->mO, c->aO.as<scm>(), Gtab, n, nullptr, nullptr, 0);
    merge_ms_last = now_ms() - t0;
}

// ------------------------------------------------------------------------------------------------ generator fold of one group
// dst[i] = Gst[i] + sum_t sG_t Gst[i + t*Mr], dst[Mr + i] the same on Hst with sH (host/fold_plan.hpp): which kernel folds (forced: the test hook names
// one), the scalars recoded for that kernel and uploaded, one launch, the roofline bookkeeping, the normalisation.  The caller waits for the stream.
Engine::Impl::FoldRun Engine::Impl::fold_launch(const FoldShape &shape, const FoldKernel *forced, uint64_t g_M, uint64_t n, const Scalar &u_ch,
                                               const std::vector<Scalar> &sG, const std::vector<Scalar> &sH, const ge_niels *Gst, const ge_niels *Hst, ge_niels *dst) {
    Impl &I = *this;
    const uint32_t Mr = shape.Mr, nterms = shape.nterms;
    const bool g_first = shape.first;
    I.scratch_ext.ensure((size_t)2 * Mr * sizeof(ge_ext));         // the folded points before their normalisation (2^18 of them after the first group of three rounds at 2^20)
    // the group-start tables are the original generators: width-w NAF against their precomputed odd multiples (k_fold_points_wnaf) -
    // unless no table fits the budget of this device, in which case the other kernels fold them
    const FoldKnobs knobs = I.fold_knobs();
    const FoldKernel kernel = forced ? *forced : choose_fold(shape, knobs, fold_wants_tables(shape, knobs) && I.odd_ensure());
    static const int kid_of[] = {KID_k_fold_points_wnaf, KID_k_fold_points_quadw, KID_k_fold_points_quad, KID_k_fold_points_split, KID_k_fold_points_regw,
                                 KID_k_fold_points_reg, KID_k_fold_points};          // in the order of FoldKernel
    const int fold_kid = kid_of[(int)kernel];
    const dim3 grid(cdiv(2 * Mr, 256)), grid64(cdiv(2 * Mr, 64)), block(256);     // one lane per output; four lanes per output (and the split kernel)
    ge_ext *fo = I.scratch_ext.as<ge_ext>();
    // the scalars in the format the kernel reads, written to pinned memory and uploaded
    FoldRecode rc; FoldWnaf fw; FoldQuadW fq; FoldGroup fg;
    const bool wnaf = kernel == FoldKernel::Wnaf, steps = kernel == FoldKernel::QuadW || kernel == FoldKernel::RegW;
    PinBuf &hbuf = steps ? I.h_qsteps : I.h_naf;
    DevBuf &dbuf = steps ? I.qsteps : I.naf;
    const size_t bytes = wnaf ? fold_wnaf_bytes(nterms, I.eff_parts) : steps ? (size_t)2 * QW_MAXSTEPS * 4 : fold_naf_words(nterms) * 4;
    hbuf.ensure(bytes); dbuf.ensure(bytes);
    FoldRun run{kernel, -1, {0, 0}, {0, 0}};
    if (wnaf) {                                         // width-w NAF digits per part, against the odd multiples odd_ensure() settled on
        rc = fold_recode_wnaf(sG, sH, u_ch, Mr, n, g_first, I.eff_wnaf, I.eff_parts, I.fold_part_bits(), hbuf.as<int8_t>());
        fw.Mr = Mr; fw.nterms = nterms; fw.first_group = g_first; fw.n = (uint32_t)n; fw.cap = (uint32_t)gens_cap; fw.top = rc.top;
        fw.parts = I.eff_parts; fw.NM = 1u << (I.eff_wnaf - 2);
        run.top = fw.top;
    } else if (steps) {                                 // width-4 NAF steps; the multiples the kernel makes live in the arena - no multiscalar sum of this context is in flight during a fold
        rc = fold_recode_steps(sG, sH, Mr, hbuf.as<uint32_t>(), fq);
        I.arena.ensure((size_t)3 * nterms * 2 * Mr * sizeof(ge_pniels));
        for (int c = 0; c < 2; c++) { run.nsteps[c] = fq.nsteps[c]; run.tail[c] = fq.tail[c]; }
    } else {                                            // plain NAF bitmaps
        rc = fold_recode_naf(sG, sH, u_ch, Mr, n, g_first, hbuf.as<uint32_t>());
        fg.Mr = Mr; fg.nterms = nterms; fg.first_group = g_first; fg.n = (uint32_t)n; fg.top = rc.top;
        run.top = fg.top;
    }
    HIPCHK(hipMemcpyAsync(dbuf.p, hbuf.p, bytes, hipMemcpyHostToDevice, st));
    const uint32_t *nf = dbuf.as<uint32_t>();
    double device_bytes = 96.0 * 2 * g_M + 128.0 * 2 * Mr;          // 2*g_M points read at 96 B, 2*Mr written at 128 B
    switch (kernel) {
    case FoldKernel::Wnaf:
        BPG_LAUNCH(I, k_fold_points_wnaf, grid, block, I.gens, I.gens_odd, fo, nf, fw);
        device_bytes = 96.0 * (2.0 * Mr + rc.adds_fm / 7.0) + 128.0 * 2 * Mr;       // one point read per output and per addition
        break;
    case FoldKernel::QuadW: BPG_LAUNCH(I, k_fold_points_quadw, grid64, block, Gst, Hst, fo, nf, reinterpret_cast<fe *>(I.arena_at(0)), fq); break;
    case FoldKernel::Quad: BPG_LAUNCH(I, k_fold_points_quad, grid64, block, Gst, Hst, fo, nf, fg); break;
    case FoldKernel::Split: BPG_LAUNCH(I, k_fold_points_split, grid64, block, Gst, Hst, fo, nf, fg); break;
    case FoldKernel::RegW: BPG_LAUNCH(I, k_fold_points_regw, grid, block, Gst, Hst, fo, nf, reinterpret_cast<ge_pniels *>(I.arena_at(0)), fq); break;
    case FoldKernel::Reg:       // addends in registers: one instantiation per group size (r = 1..4)
        if (nterms == 1) BPG_LAUNCH_ID(I, fold_kid, k_fold_points_reg<1>, grid, block, Gst, Hst, fo, nf, fg);
        else if (nterms == 3) BPG_LAUNCH_ID(I, fold_kid, k_fold_points_reg<3>, grid, block, Gst, Hst, fo, nf, fg);
        else if (nterms == 7) BPG_LAUNCH_ID(I, fold_kid, k_fold_points_reg<7>, grid, block, Gst, Hst, fo, nf, fg);
        else BPG_LAUNCH_ID(I, fold_kid, k_fold_points_reg<15>, grid, block, Gst, Hst, fo, nf, fg);
        break;
    case FoldKernel::Mem: BPG_LAUNCH(I, k_fold_points, grid, block, Gst, Hst, fo, nf, fg); break;
    }
    // bookkeeping for the roofline: 2*g_M points read + 2*Mr written at 32 B (information content) resp. in the device formats; field
    // multiplications: 8 per doubling, 7 per mixed addition (the split variant runs the doublings once per wave of a block)
    I.prof_note(fold_kid, 32.0 * (2.0 * g_M + 2.0 * Mr), device_bytes,
                2.0 * Mr * (8.0 * (rc.top + 1) * (kernel == FoldKernel::Split ? (nterms < 4 ? nterms : 4) : 1) + 7.0) + rc.adds_fm);
    BPG_LAUNCH(I, k_normalize_niels, dim3(cdiv(cdiv(2 * Mr, NORM_K), 256)), dim3(256), I.scratch_ext.as<ge_ext>(), dst, 2 * Mr);
    return run;
}

// ------------------------------------------------------------------------------------------------ table-driven tail and commitments
void Engine::Impl::tail_freeze(TailState &S, uint32_t M0, bool first, uint64_t n, const scm &uch_m, const Scalar &Gamma, const Scalar &Eta, const ge_niels *Gst,
                               const ge_niels *Hst, const ge_niels *Bn, bool original, bool try_wide) {
    S.lgM0 = ceil_log2(M0); S.j = 0; S.cur = 0;
    tt_f.ensure((size_t)2 * M0 * sizeof(scm)); tt_c.ensure((size_t)4 * M0 * sizeof(scm));
    tt_build(Gst, Hst, Bn, M0, original);
    S.wide = try_wide ? wide_ensure(M0) : nullptr;                             // original generators: 8-bit windows, built once per device
    BPG_LAUNCH((*this), k_tt_factors, dim3(cdiv(M0, 256)), dim3(256), yinvpow.as<scm>(), uch_m, (uint32_t)first, (uint32_t)n, M0, to_scm(Gamma), to_scm(Eta),
               tt_f.as<scm>(), tt_f.as<scm>() + M0, tt_c.as<scm>());
}
// apply the previous round's challenge: fold a, b (2*mcur -> mcur) and double the coefficient tables
void Engine::Impl::tail_advance(TailState &S, scm *a, scm *b, uint64_t mcur) {
    const uint32_t M0 = 1u << S.lgM0;
    scm *c0 = tt_c.as<scm>() + (size_t)S.cur * 2 * M0, *c1 = tt_c.as<scm>() + (size_t)(S.cur ^ 1u) * 2 * M0;
    BPG_LAUNCH((*this), k_tt_advance, dim3(cdiv(std::max<uint64_t>(mcur, 1ull << (S.j - 1)), 256)), dim3(256), a, b, to_scm(S.u), to_scm(S.uinv), (uint32_t)mcur,
               c0, c1, 1u << (S.j - 1), M0);
    S.cur ^= 1u;
}
void Engine::Impl::tail_round(TailState &S, scm *a, scm *b, uint64_t mcur, const scm &w_m, uint32_t quad_sums, uint8_t lr[64]) {
    const uint32_t M0 = 1u << S.lgM0;
    const uint64_t h = mcur / 2;
    if (S.j > 0) tail_advance(S, a, b, mcur);
    const scm *c0 = tt_c.as<scm>() + (size_t)S.cur * 2 * M0;
    const uint32_t nblk = tail_nblk(M0);
    if (S.wide) BPG_LAUNCH((*this), k_tt_round8, dim3(nblk, 2), dim3(256), S.wide, a, b, tt_f.as<scm>(), tt_f.as<scm>() + M0, c0, S.lgM0, S.j, tt_partial.as<ge_ext>(), quad_sums);
    else BPG_LAUNCH((*this), k_tt_round, dim3(nblk, 2), dim3(256), tt_table_p, a, b, tt_f.as<scm>(), tt_f.as<scm>() + M0, c0, S.lgM0, S.j,
               tt_partial.as<ge_ext>(), quad_sums);
    BPG_LAUNCH((*this), k_tt_finish, dim3(2), dim3(256), tt_partial.as<ge_ext>(), nblk, a, b, (uint32_t)h, w_m,
               tt_table_p + (size_t)2 * M0 * TT_WINDOWS * TT_MULTS, msm_result.as<ge_ext>(), quad_sums);
    HIPCHK(hipGetLastError());
    uint32_t *hp = reinterpret_cast<uint32_t *>(h_small.as<uint8_t>() + 16384);       // L, R as extended points; encoded on the host
    HIPCHK(hipMemcpyAsync(hp, msm_result.p, 2 * sizeof(ge_ext), hipMemcpyDeviceToHost, st));
    wait_stream();
    h51::pt_compress(lr, h51::pt_from_device(hp)); h51::pt_compress(lr + 32, h51::pt_from_device(hp + 32));
}
void Engine::Impl::tail_last_fold(const TailState &S, scm *a, scm *b, uint64_t h) {
    BPG_LAUNCH((*this), k_ipa_fold_scalars, dim3(cdiv(h, 256)), dim3(256), a, b, to_scm(S.u), to_scm(S.uinv), (uint32_t)h);
    HIPCHK(hipGetLastError());
}
void Engine::Impl::commit3(const scm *aL, const scm *aR, const scm *aO, const scm *sL, const scm *sR, uint64_t n, uint32_t M0, uint32_t quad_sums, uint8_t pts[96]) {
    const uint32_t nblk = commit3_nblk(M0);
    BPG_LAUNCH((*this), k_tt_commit3, dim3(nblk, 3), dim3(256), tt_table_p, aL, aR, aO, sL, sR, (uint32_t)n, M0, tt_partial.as<ge_ext>(), quad_sums);
    BPG_LAUNCH((*this), k_tt_commit3_finish, dim3(3), dim3(256), tt_partial.as<ge_ext>(), nblk, extras.as<scm>(),
               ped_table.as<ge_pniels>() + (size_t)TT_WINDOWS * TT_MULTS, msm_result.as<ge_ext>(), quad_sums);
    HIPCHK(hipGetLastError());
    uint32_t *hp = reinterpret_cast<uint32_t *>(h_small.as<uint8_t>() + 16384);           // three extended points; encoded on the host
    HIPCHK(hipMemcpyAsync(hp, msm_result.p, 3 * sizeof(ge_ext), hipMemcpyDeviceToHost, st));
    wait_stream();
    for (int k = 0; k < 3; k++) h51::pt_compress(pts + 32 * k, h51::pt_from_device(hp + 32 * k));
}

// ------------------------------------------------------------------------------------------------ inner-product argument
// InnerProductProof::create (dalek inner_product_proof.rs) on l(x) = lv, r(x) = rv with G_factors = (1.., u..), H_factors = y^-i * G_factors
// and Q = w * B: appends L_k, R_k (lg N pairs) and the final a, b to `proof`.  Rounds above 2^tt_lg generators: grouped folds with
// bucket-method MSMs; from there on: frozen generators and window tables (kernels.cuh).
void Engine::Impl::inner_product(Transcript &T, std::vector<uint8_t> &proof, uint64_t n, uint64_t N, const Scalar &yinv, const Scalar &u_ch,
                                 const Scalar &w, const ge_niels *Gtab, const ge_niels *Htab, const ge_niels *Bn, ProveTimings *tm, double &t0) {
    Impl &I = *this;
    const uint32_t lgN = ceil_log2(N);
    auto lap = [&](double *slot) { if (tm) { I.wait_stream(); double t1 = now_ms(); *slot += t1 - t0; t0 = t1; } };
    T.innerproduct_domain_sep(N);
    std::vector<Scalar> yinv_pow2(lgN + 1);
    yinv_pow2[0] = yinv; for (uint32_t k = 1; k <= lgN; k++) yinv_pow2[k] = yinv_pow2[k - 1] * yinv_pow2[k - 1];
    scm *a = I.lv.as<scm>(), *b = I.rv.as<scm>();
    if (lgN) {
        const uint64_t half = N / 2;
        I.ipa_s.ensure(4 * half * sizeof(scm));
        I.ipa_tabA.ensure(2 * half * sizeof(ge_niels)); I.ipa_tabB.ensure((half > 1 ? half : 2) * sizeof(ge_niels));
        I.naf.ensure(4096);
    }
    Scalar Gamma = Scalar::one(), Eta = Scalar::one();
    const ge_niels *Gst = Gtab, *Hst = Htab;
    const scm w_m = to_scm(w), uch_m = to_scm(u_ch);
    uint64_t mcur = N;
    // table-driven tail state (kernels.cuh "table-driven IPA tail")
    const uint32_t quad_sums = I.shared_now ? 0u : 1u;                 // the block sums of the tail kernels: quad layout for a proof alone (k_points.cuh ge_block_sum_store)
    bool tt_on = false; Impl::TailState tt;
    // grouped-fold state
    const uint32_t GRP_STRIDE = 64;
    uint32_t g_j = 0, g_r = 1, g_cur = 0, g_index = 0; uint64_t g_M = N; bool g_first = true; std::vector<Scalar> g_us;
    for (uint32_t round = 0; round < lgN; round++) {
        const uint64_t h = mcur / 2;
        const bool first = round == 0;
        if (!tt_on && ((I.tt_lg > 0 && mcur <= (1ull << I.tt_lg)) || (first && I.tt_orig_lg > 0 && mcur <= (1ull << I.tt_orig_lg)))) {
            // freeze the generators at this level: window tables for G[0..M0), H[0..M0) and B
            tt_on = true;
            const bool original = Gst == Gtab && Hst == Htab;                  // their tables: a no-op when this context already holds them (N <= 2^tt_orig_lg)
            I.tail_freeze(tt, (uint32_t)mcur, first, n, uch_m, Gamma, Eta, Gst, Hst, Bn, original, original && Gtab == I.gens);
        }
        if (tt_on) {
            uint8_t lr[64];
            I.tail_round(tt, a, b, mcur, w_m, quad_sums, lr);
            lap(tm ? &tm->ipa_msm : nullptr);
            proof.insert(proof.end(), lr, lr + 64);
            I.tail_challenge(tt, fs_ipa_round(T, lr, lr + 32));
            mcur = h;
            if (round + 1 == lgN) I.tail_last_fold(tt, a, b, h);   // last round: only the scalar fold remains
            continue;
        }
        // ---- grouped fold rounds (kernels.cuh k_ipa_prep / k_fold_points): sub-round g_j of a group of g_r rounds on tables of size g_M
        if (g_j == 0) {
            g_M = mcur; g_first = first;
            uint32_t left = ceil_log2(mcur);                               // rounds until the tables would be a single point
            if (I.tt_lg > 0 && left > I.tt_lg) left -= I.tt_lg;            // ... or until the tail freezes them
            g_r = std::min<uint32_t>(I.fold_group, left);
            g_us.clear();
            I.grp_c.ensure(4 * GRP_STRIDE * sizeof(scm));
            g_cur = 0;
            hipLaunchKernelGGL(k_set2, dim3(1), dim3(64), 0, st, I.grp_c.as<scm>(), (uint32_t)GRP_STRIDE, to_scm(Gamma), to_scm(Eta));
        }
        scm *c0 = I.grp_c.as<scm>() + (size_t)g_cur * 2 * GRP_STRIDE;
        const uint64_t cnt = g_M / 2;                                       // expanded scalars per side: h * 2^g_j
        scm *sLG = I.ipa_s.as<scm>(), *sLH = sLG + cnt, *sRG = sLH + cnt, *sRH = sRG + cnt;
        const uint32_t blocks = std::min<uint32_t>(cdiv(cnt, 256), 1024);
        const uint32_t lgh = ceil_log2(h);
        I.red_partial.ensure((size_t)blocks * 2 * sizeof(scm) + 4096);
        BPG_LAUNCH(I, k_ipa_prep, dim3(blocks), dim3(256), a, b, I.yinvpow.as<scm>(), c0, c0 + GRP_STRIDE, uch_m,
                           (uint32_t)g_first, (uint32_t)n, lgh, g_j, sLG, sLH, sRG, sRH, I.red_partial.as<scm>());
        BPG_LAUNCH_ID(I, KID_k_reduce_partials, k_reduce_partials_scaled, dim3(2), dim3(256), I.red_partial.as<scm>(), blocks, 2u, I.extras.as<scm>() + 3, w_m);
        Impl::MsmTicket tk;
        {
            MsmJob J = job_new();
            const uint32_t lgblk = g_j ? lgh : 31u;                         // every other block of h points of the group-start tables
            seg_push(J, sLG, Gst + h, (uint32_t)cnt, 0, lgblk);
            seg_push(J, sLH, Hst, (uint32_t)cnt, 0, lgblk);
            seg_push(J, I.extras.as<scm>() + 3, Bn, 1, 0);
            seg_push(J, sRG, Gst, (uint32_t)cnt, 1, lgblk);
            seg_push(J, sRH, Hst + h, (uint32_t)cnt, 1, lgblk);
            seg_push(J, I.extras.as<scm>() + 4, Bn, 1, 1);
            tk = I.msm(J, 2);
        }
        uint8_t lr[64];
        I.wait_stream();
        { const std::vector<h51::pt> LR = I.msm_points(tk); h51::pt_compress(lr, LR[0]); h51::pt_compress(lr + 32, LR[1]); }
        lap(tm ? &tm->ipa_msm : nullptr);
        proof.insert(proof.end(), lr, lr + 64);
        const Scalar u = fs_ipa_round(T, lr, lr + 32), uinv = u.invert();
        g_us.push_back(u);
        {   // fold a, b and extend the coefficient tables cG, cH (2^g_j -> 2^(g_j+1) entries)
            scm *c1 = I.grp_c.as<scm>() + (size_t)(g_cur ^ 1u) * 2 * GRP_STRIDE;
            BPG_LAUNCH(I, k_tt_advance, dim3(cdiv(std::max<uint64_t>(h, 1ull << g_j), 256)), dim3(256), a, b, to_scm(u), to_scm(uinv), (uint32_t)h,
                       c0, c1, 1u << g_j, (uint32_t)GRP_STRIDE);
            g_cur ^= 1u;
        }
        g_j++;
        if (g_j == g_r) {
            // generator fold of the whole group (host/fold_plan.hpp): the group scalars, which kernel folds, the scalars recoded for that kernel, one launch
            const uint32_t Mr = (uint32_t)(g_M >> g_r), nterms = (1u << g_r) - 1u;
            std::vector<Scalar> sG, sH;
            fold_group_scalars(g_us, yinv_pow2, g_M, g_r, sG, sH);
            ge_niels *dst = (g_index & 1) ? I.ipa_tabB.as<ge_niels>() : I.ipa_tabA.as<ge_niels>();
            I.fold_launch(FoldShape{Mr, nterms, g_first, Gst == Gtab && Hst == Htab && Gtab == I.gens}, nullptr, g_M, n, u_ch, sG, sH, Gst, Hst, dst);
            HIPCHK(hipGetLastError());
            I.wait_stream();                               // h_naf is reused by the next group
            Gst = dst; Hst = dst + Mr;
            for (const Scalar &uk : g_us) { Gamma = uk.invert() * Gamma; Eta = uk * Eta; }
            g_j = 0; g_index++;
        }
        mcur = h;
        lap(tm ? &tm->ipa_fold : nullptr);
    }
    scm ab[2];
    HIPCHK(hipMemcpyAsync(&ab[0], a, sizeof(scm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&ab[1], b, sizeof(scm), hipMemcpyDeviceToHost, st));
    I.wait_stream();
    { uint8_t o[64]; from_scm(ab[0]).to_bytes(o); from_scm(ab[1]).to_bytes(o + 32); proof.insert(proof.end(), o, o + 64); }
}

// ------------------------------------------------------------------------------------------------ prove
// Speculative start of Prover::prove's TranscriptRng (include/bpg.h: bpg_blinding_begin).  The 2n + 3 leading draws depend on the transcript
// after the last commitment (+ the "m" suffix), the commitment blindings and the external seed - not on the constraints or on n - so a
// host thread can draw them while the caller still assembles the circuit.  prove() takes the stream over only when all three match.
void Engine::blinding_begin(const Transcript &after_commitments, const std::vector<Scalar> &v_blinding, const uint8_t seed[32], uint64_t max_multipliers) {
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    if (max_multipliers == 0) { I.blind_cancel(); return; }
    if (I.chain && I.chain->pool) {     // a pool that was destroyed under this context (its threads are gone): fall back to the context's own worker
        bool gone; { std::lock_guard<std::mutex> lk(I.chain->mu); gone = I.chain->quit; }
        if (gone) { I.blind_cancel(); I.chain.reset(); I.pool_streams = 0; }
    }
    using BS = Impl::BlindStream;
    const size_t max_alive = I.pool_streams ? I.pool_streams : (size_t)I.chain_workers * I.chain_lanes + 1;
    while (I.blinds.size() >= max_alive) { I.blind_retire(I.blinds.front()); I.blinds.pop_front(); }     // the oldest gives way
    auto b = std::make_shared<BS>();
    Transcript T = after_commitments;
    T.append_u64("m", v_blinding.size());
    T.export_state(b->state);
    std::memcpy(b->seed, seed, 32); b->vb = v_blinding;
    TranscriptRng rng = T.build_rng(v_blinding, seed);
    for (int k = 0; k < 3; k++) b->first[k] = rng.random_scalar();
    b->max_draws = ((2 * max_multipliers + BS::SNAP - 1) / BS::SNAP) * BS::SNAP;
    b->inject_fail = I.test_fail_upload; I.test_fail_upload = 0;
    // pinned slab: one that no alive stream owns; its previous owner must have left it (its uploads were synchronised by the prove() that used it)
    if (I.h_blind.size() < max_alive) { I.h_blind.resize(max_alive); I.slab_owner.resize(max_alive); while (I.slab_dev.size() < max_alive) I.slab_dev.emplace_back(std::make_unique<Impl::SlabDev>()); }
    int slot = -1;
    for (size_t k = 0; k < max_alive && slot < 0; k++) {
        bool used = false;
        for (const std::shared_ptr<BS> &x : I.blinds) used |= x->slot == (int)k;
        if (!used) slot = (int)k;
    }
    if (slot < 0) throw std::logic_error("blinding_begin: no free slab");
    b->slot = slot;
    if (I.slab_owner[slot]) { I.blind_retire(I.slab_owner[slot]); I.slab_owner[slot].reset(); }
    Impl::SlabDev &sd = *I.slab_dev[slot];
    if (!sd.copy_st) sd.copy_st = Stream::non_blocking();
    HIPCHK(hipStreamSynchronize(sd.copy_st));                  // no copy of the previous owner still reads the slab
    I.h_blind[slot].ensure(b->max_draws * 64);
    sd.d.ensure(b->max_draws * 64);
    while (sd.ev.size() < b->max_draws / BS::UP + 1) sd.ev.push_back(Event::untimed());
    // The device slab changes owner here.  Two things keep this proof from reading the previous owner's draws: BlindStream::err - an upload that
    // fails is recorded BEFORE its block is published and prove() refuses the stream - and a canary against a copy that is dropped WITHOUT an error:
    // the first draw of every block is overwritten with a pattern here (1 KB of stores for a 2^20 proof, on the copy stream, ahead of the uploads),
    // k_sc_from_wide raises stale_flag on a draw that still reads as the pattern, and prove() checks the flag before the proof leaves it.  (Round 3
    // overwrote the whole slab - a 128 MB memset per 2^20 proof - with a constant nothing ever checked for.)
    {
        const uint32_t nblk = (uint32_t)((b->max_draws + BS::UP - 1) / BS::UP);        // the last block may be a partial one
        if (nblk) hipLaunchKernelGGL(k_blind_poison, dim3(cdiv((uint64_t)nblk * 16, 256)), dim3(256), 0, sd.copy_st, sd.d.as<uint32_t>(), nblk, (uint32_t)BS::UP);
        HIPCHK(hipGetLastError());
    }
    b->raw = I.h_blind[slot].as<uint8_t>();
    b->device = device_; b->copy_st = (hipStream_t)sd.copy_st; b->d_raw = sd.d.as<uint8_t>(); b->ev = &sd.ev;
    // how a drawn block reaches the device (called on the chain thread; host/chain.hpp publishes the block afterwards): an asynchronous copy on the
    // slab's own copy stream, then the block's event; the threads of a pool serve contexts of different devices, hence the hipSetDevice
    b->upload = [](BlindStream &bs, uint64_t from, uint64_t to, uint64_t k) -> int {
        hipError_t e = hipSetDevice(bs.device);
        if (e == hipSuccess && bs.inject_fail != 2) e = hipMemcpyAsync(bs.d_raw + 64 * from, bs.raw + 64 * from, (to - from) * 64, hipMemcpyHostToDevice, static_cast<hipStream_t>(bs.copy_st));
        if (e == hipSuccess) e = hipEventRecord(Impl::block_event(bs, k), static_cast<hipStream_t>(bs.copy_st));
        return (int)e;
    };
    b->snaps.assign(b->max_draws / BS::SNAP + 1, rng);
    I.slab_owner[slot] = b;
    I.blinds.push_back(b);
    if (!I.chain) { I.chain = std::make_shared<Impl::ChainWorker>(); I.chain->lanes = I.chain_lanes; (void)keccak_impl(); }
    if (!I.chain->pool) while (I.chain->th.size() < I.chain_workers) I.chain->th.emplace_back(Impl::ChainWorker::run, I.chain.get(), I.chain->lanes);
    I.chain->push(b);
}
// ChainPool: chain threads shared by the contexts attached to it (engine.hpp)
struct ChainPool::Impl { std::shared_ptr<Engine::Impl::ChainWorker> w; };
ChainPool::ChainPool(const std::vector<uint32_t> &lanes_per_thread) : impl_(new Impl()) {
    if (lanes_per_thread.empty() || lanes_per_thread.size() > 256) { delete impl_; throw std::invalid_argument("chain pool: 1..256 threads"); }
    for (uint32_t l : lanes_per_thread) if (l < 1 || l > 8) { delete impl_; throw std::invalid_argument("chain pool: 1..8 lanes per thread"); }
    impl_->w = std::make_shared<Engine::Impl::ChainWorker>();
    impl_->w->pool = true;
    (void)keccak_impl();
    for (uint32_t l : lanes_per_thread) { impl_->w->th.emplace_back(Engine::Impl::ChainWorker::run, impl_->w.get(), l); capacity_ += l; }
}
ChainPool::~ChainPool() { impl_->w->stop(); delete impl_; }
void Engine::attach_chain_pool(ChainPool *pool, uint32_t max_streams) {
    impl_->chain_shutdown();                                  // streams in flight are dropped
    if (!pool) return;
    if (max_streams < 1 || max_streams > 64) throw std::invalid_argument("chain pool: 1..64 streams per context");
    impl_->chain = pool->impl_->w; impl_->pool_streams = max_streams;
}
void Engine::set_chain_workers(uint32_t n) {
    if (n < 1 || n > 64) throw std::invalid_argument("chain workers: 1..64");
    impl_->chain_shutdown();                                  // streams in flight are dropped; threads restart with the next begin
    impl_->chain_workers = n;
}
void Engine::set_chain_lanes(uint32_t n) {
    if (n < 1 || n > 8) throw std::invalid_argument("chain lanes: 1..8");
    impl_->chain_shutdown();
    impl_->chain_lanes = n;
}
void Engine::blinding_cancel() { impl_->blind_cancel(); }
void Engine::test_fail_next_upload() { impl_->test_fail_upload = 1; }
void Engine::test_drop_next_upload() { impl_->test_fail_upload = 2; }
uint64_t Engine::table_bytes() const { return table_bytes_held(device_); }

int Engine::chain_cpu() const { return impl_->last_chain_cpu; }
bool Engine::last_shared_variants() const { return impl_->shared_now; }

std::vector<uint8_t> Engine::prove(DeviceCircuit *c, Transcript &T, const std::vector<Scalar> &v_blinding,
                                   const uint8_t rng_seed[32], uint32_t flags, ProveTimings *tm) {
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    hipStream_t st = I.st;
    ProvingGuard in_flight(device_);
    // the kernel variants of this proof are chosen HERE, once: a proof that enters or leaves prove() on another thread must not flip the
    // schedule half-way through (ProveTimings::shared_variants reports the choice, so a failing proof can be replayed with BPG_FOLD_ADAPT=0 or 2)
    I.shared_now = I.shared_variants();
    if (tm) tm->shared_variants = I.shared_now ? 1u : 0u;
    const uint64_t n = c->n, m = c->m, q = c->q;
    if (v_blinding.size() != m) throw std::invalid_argument("prove: need one blinding factor per committed variable");
    if (!c->has_witness) throw R1CSException(R1CSError::MissingAssignment, "prove: the uploaded circuit carries no assignments (verifier-side instance)");
    const uint64_t N = padded_size(n);
    const uint32_t lgN = ceil_log2(N);
    require_gens_capacity(gens_cap_, n);
    const double t_begin = now_ms();
    double t0 = t_begin;
    auto lap = [&](double *slot) { if (tm) { I.wait_stream(); double t1 = now_ms(); *slot += t1 - t0; t0 = t1; } };

    const ge_niels *Gtab = I.gens, *Htab = I.gens + gens_cap_;
    const ge_niels *Bn = I.bases.as<ge_niels>(), *Bbn = Bn + 1;

    // ---- transcript, RNG, first blindings
    T.append_u64("m", m);
    const bool expanded = (flags & 4u) != 0;          // BPG_FLAG_EXPANDED_BLINDING: no host chain to hide behind
    // a speculative blinding stream is used only when it was drawn from exactly this transcript state, these blindings and this seed
    std::shared_ptr<Impl::BlindStream> bs;
    if (!I.blinds.empty()) {
        uint8_t now[203]; T.export_state(now);
        for (const std::shared_ptr<Impl::BlindStream> &cand : I.blinds) {
            const Impl::BlindStream &b = *cand;
            bool ok = !expanded && 2 * n <= b.max_draws && std::memcmp(now, b.state, 203) == 0 && std::memcmp(rng_seed, b.seed, 32) == 0 && b.vb.size() == v_blinding.size();
            for (size_t i = 0; ok && i < b.vb.size(); i++) ok = std::memcmp(b.vb[i].as_bytes(), v_blinding[i].as_bytes(), 32) == 0;
            if (ok) { bs = cand; break; }
        }
        // no match: the alive streams may belong to later proofs of a sequence; they are bounded (two) and replaced by the next begin
    }
    // (first[] and snaps[0] were written by blinding_begin on this thread, before the worker saw the stream)
    TranscriptRng rng = T.build_rng(v_blinding, rng_seed);     // with a stream: replaced by the stream's generator once the 2n draws are in
    Scalar ib, ob, sb;
    if (bs) { ib = bs->first[0]; ob = bs->first[1]; sb = bs->first[2]; }
    else { ib = rng.random_scalar(); ob = rng.random_scalar(); sb = rng.random_scalar(); }

    // small device scalars: extras[0..2] = ib, ob, sb ; [3..4] = cL*w, cR*w (per round)
    I.extras.ensure(16 * sizeof(scm));
    I.h_small.ensure(1 << 16);
    {
        scm *hs = I.h_small.as<scm>();
        hs[0] = to_scm(ib); hs[1] = to_scm(ob); hs[2] = to_scm(sb);
        HIPCHK(hipMemcpyAsync(I.extras.p, hs, 3 * sizeof(scm), hipMemcpyHostToDevice, st));
    }
    I.msm_result.ensure(4 * sizeof(ge_ext)); I.comp.ensure(256);

    // ---- A_I, A_O (do not depend on s_L, s_R): launch, then draw the 2n RNG scalars on the host while they run
    const bool tabled = I.tt_orig_lg > 0 && N <= (1ull << I.tt_orig_lg) && n > 0;   // the generators have (or get) window tables: A_I, A_O, S are table sums
    if (tabled) I.tt_build(Gtab, Htab, Bn, (uint32_t)N, true);
    // the stream of this proof was drawn ahead (a sequence of proofs: its chain ran under the previous proof's kernels) and is complete
    const bool chain_ready = bs && bs->produced.load(std::memory_order_acquire) >= 2 * n;
    const bool merged = expanded || tabled || n < 4096 || chain_ready;   // nothing to hide behind: A_I, A_O, S in one pass after the draws (one serial tail, not four)
    Impl::MsmTicket tk_aiao{0, 0, 0}, tk_s[3]; uint32_t nparts = 0;
    // A_I's terms with equal scalars share their bucket entries (hip/k_merge.cuh): grouped once per uploaded witness, here at its first proof
    if (!tabled) { if (I.merge_equal == 2) c->merge_tried = false; I.merge_witness(c, Gtab, Htab); }
    I.merged_last = tabled ? 0u : c->mI.groups + c->mO.groups; I.merged_skipped_last = tabled ? 0u : c->mI.skipped + c->mO.skipped;
    auto push_AI = [&](MsmJob &J) {        // <a_L, G> + <a_R, H> + i_blinding * B_blinding as result 0
        const bool mg = c->mI.groups != 0;
        seg_push(J, c->aL.as<scm>(), Gtab, (uint32_t)n, 0, 31, mg ? c->mI.skipA.as<uint32_t>() : nullptr);
        seg_push(J, c->aR.as<scm>(), Htab, (uint32_t)n, 0, 31, mg ? c->mI.skipB.as<uint32_t>() : nullptr);
        if (mg) seg_push_merged(J, c->mI.sc.as<scm>(), c->mI.pts.as<ge_niels>(), c->mI.groups, 0, c->mI.skipped);
        seg_push(J, I.extras.as<scm>() + 0, Bbn, 1, 0);
    };
    auto push_AO = [&](MsmJob &J) {        // <a_O, G> + o_blinding * B_blinding as result 1
        const bool mg = c->mO.groups != 0;
        seg_push(J, c->aO.as<scm>(), Gtab, (uint32_t)n, 1, 31, mg ? c->mO.skipA.as<uint32_t>() : nullptr);
        if (mg) seg_push_merged(J, c->mO.sc.as<scm>(), c->mO.pts.as<ge_niels>(), c->mO.groups, 1, c->mO.skipped);
        seg_push(J, I.extras.as<scm>() + 1, Bbn, 1, 1);
    };
    if (!merged) {
        MsmJob J = job_new();
        push_AI(J); push_AO(J);
        tk_aiao = I.msm(J, 2);
    }
    const double t_rng0 = now_ms();
    if (!bs && !expanded) { I.h_raw.ensure((2 * n ? 2 * n : 1) * 64); I.raw_rng.ensure((2 * n ? 2 * n : 1) * 64); }      // the draws of a chain made inside this call; a blinding stream brings its own slabs
    I.sLR.ensure((2 * n ? 2 * n : 1) * sizeof(scm));
    scm *sL = I.sLR.as<scm>(), *sR = sL + n;
    // S = <s_L, G> + <s_R, H> + sb * B_blinding is accumulated in pieces as the draws arrive: <s_L, G> once s_L is complete,
    // the first 7/8 of <s_R, H> next, and only the last eighth (+ the blinding term) after the chain has ended.  (A last piece of 1/32 takes 0.05 ms off a lone
    // proof and nothing off a burst: thirteen chains end together, and their second pieces - a million terms each - then start 5 ms before the end instead of 19.)
    struct Piece { uint64_t a, b; } pieces[3] = {{0, n}, {n, n + (n - n / 8)}, {n + (n - n / 8), 2 * n}};
    if (n < (1u << 17)) { pieces[0] = {0, 0}; pieces[1] = {0, 0}; pieces[2] = {0, 2 * n}; }      // short chain: one MSM after it (each call has a ~1 ms serial tail)
    uint32_t next_piece = 0;
    auto launch_pieces = [&](uint64_t drawn) {
        while (next_piece < 3 && pieces[next_piece].b <= drawn) {
            const Piece pc = pieces[next_piece];
            const bool last = next_piece == 2;
            next_piece++;
            if (pc.b == pc.a && !last) continue;
            MsmJob J = job_new();
            if (pc.a < n) seg_push(J, sL + pc.a, Gtab + pc.a, (uint32_t)(std::min<uint64_t>(pc.b, n) - pc.a), 0);
            if (pc.b > n) { const uint64_t a2 = std::max<uint64_t>(pc.a, n) - n; seg_push(J, sR + a2, Htab + a2, (uint32_t)(pc.b - n - a2), 0); }
            if (last) seg_push(J, I.extras.as<scm>() + 2, Bbn, 1, 0);
            tk_s[nparts++] = I.msm(J, 1);
        }
    };
    // the slab on the device may still hold an earlier proof's draws: s_L, s_R must never be built from a stream whose upload failed
    auto upload_failed = [&] {
        const int uerr = bs->err.load(std::memory_order_acquire);
        if (uerr) { I.blind_release(bs); throw DeviceError(std::string("upload of the blinding draws failed: ") + hipGetErrorString((hipError_t)uerr)); }
    };
    if (expanded) {     // (include/bpg.h): one draw K, the 2n scalars are expanded from it on the device
        uint8_t msg[80]; std::memset(msg, 0, sizeof msg);
        std::memcpy(msg, "bpg blinding v1", 15);
        rng.fill_bytes(msg + 15, 64);
        BlindHead head; std::memcpy(head.lane, msg, 80); head.lane[9] &= 0x00ffffffffffffffULL;      // byte 79 belongs to the index
        if (n) BPG_LAUNCH(I, k_blind_expand, dim3(cdiv(2 * n, 256)), dim3(256), head, sL, (uint32_t)(2 * n));
    } else
    {   // s_L[0..n) then s_R[0..n): 64 uniform bytes each, drawn in slabs; each slab is uploaded and reduced mod l while the
        // host draws the next one (the copies queue behind the A_I/A_O kernels on the stream and overlap the serial chain)
        uint8_t *raw = bs ? bs->raw : I.h_raw.as<uint8_t>();
        const uint64_t slab = 1u << 16;
        if (bs && chain_ready && 2 * n > 0) {
            // the whole chain was drawn (and handed to the copy stream) before this proof started - a sequence of proofs with its chains drawn
            // ahead: wait for every block's event, then ONE conversion launch instead of one per 4 MB block (31 at 2^20)
            const uint64_t nblk = (2 * n + Impl::BlindStream::UP - 1) / Impl::BlindStream::UP;
            while (bs->uploaded_blocks.load(std::memory_order_acquire) < nblk) {
                if (bs->finished.load(std::memory_order_acquire) && bs->uploaded_blocks.load(std::memory_order_acquire) < nblk) break;     // stopped short: handled below
                std::this_thread::sleep_for(std::chrono::microseconds(40));
            }
            upload_failed();
            if (bs->uploaded_blocks.load(std::memory_order_acquire) < nblk) throw DeviceError("the blinding stream ended before its draws were uploaded");
            for (uint64_t k = 0; k < nblk; k++) HIPCHK(hipStreamWaitEvent(st, Impl::block_event(*bs, k), 0));
            BPG_LAUNCH(I, k_sc_from_wide, dim3(cdiv(2 * n, 256)), dim3(256), reinterpret_cast<const uint32_t *>(bs->d_raw), sL, (uint32_t)(2 * n), I.stale_flag.as<uint32_t>());
        } else
        {
        // the draws are converted (64 uniform bytes -> a scalar mod l) when somebody needs them: before each piece of S and after the last draw - three launches
        // for a 2^20-gate proof where rounds 1-4 made one per slab (31), every one of them behind the chain and none of them needed so early
        uint64_t conv_from = 0;
        auto convert_to = [&](uint64_t hi) {
            if (hi <= conv_from) return;
            const uint32_t *src = bs ? reinterpret_cast<const uint32_t *>(bs->d_raw) : I.raw_rng.as<uint32_t>();
            BPG_LAUNCH(I, k_sc_from_wide, dim3(cdiv(hi - conv_from, 256)), dim3(256), src + 16 * conv_from, sL + conv_from, (uint32_t)(hi - conv_from), I.stale_flag.as<uint32_t>());
            conv_from = hi;
        };
        for (uint64_t i = 0; i < 2 * n; i += slab) {
            const uint64_t cnt = std::min<uint64_t>(slab, 2 * n - i);
            if (bs) {
                // drawn (or being drawn) and uploaded block by block by the chain worker: wait until block i / UP has been handed to the copy
                // stream, then make this stream wait for its event - no host copy, no copy on this stream
                const uint64_t k = i / Impl::BlindStream::UP;
                while (bs->uploaded_blocks.load(std::memory_order_acquire) <= k) std::this_thread::sleep_for(std::chrono::microseconds(40));
                upload_failed();
                HIPCHK(hipStreamWaitEvent(st, Impl::block_event(*bs, k), 0));
            } else {
                rng.fill_draws64(raw + 64 * i, cnt);
                HIPCHK(hipMemcpyAsync(I.raw_rng.as<uint8_t>() + 64 * i, raw + 64 * i, cnt * 64, hipMemcpyHostToDevice, st));
            }
            if (!merged && i + cnt < 2 * n && next_piece < 3 && pieces[next_piece].b <= i + cnt) { convert_to(i + cnt); launch_pieces(i + cnt); }
        }
        convert_to(2 * n);
        }
    }
    if (bs) {   // take the generator back: the state before draw 2n is the last snapshot at or below it, advanced by the remainder
        const uint64_t K = (2 * n) / Impl::BlindStream::SNAP, rem = 2 * n - K * Impl::BlindStream::SNAP;
        while (bs->produced.load(std::memory_order_acquire) < K * Impl::BlindStream::SNAP) std::this_thread::sleep_for(std::chrono::microseconds(20));
        rng = bs->snaps[K];
        if (rem) { std::vector<uint8_t> skip(rem * 64); rng.fill_draws64(skip.data(), rem); }
        // done with the stream: the worker stops at its next snapshot and moves on to the next queued one; the pinned slab stays allocated
        // (the queued uploads still read it) and is not handed out again before this prove() has synchronised the stream
        I.blind_release(bs);
        { const int c = bs->cpu.load(std::memory_order_relaxed); if (c >= 0) I.last_chain_cpu = c; }
        bs.reset();
    }
    if (tm) tm->rng_host += now_ms() - t_rng0;
    lap(tm ? &tm->msm_aiao : nullptr);
    uint8_t pts[96];
    if (tabled) {
        I.commit3(c->aL.as<scm>(), c->aR.as<scm>(), c->aO.as<scm>(), sL, sR, n, (uint32_t)N, I.shared_now ? 0u : 1u, pts);
    } else if (merged) {
        MsmJob J = job_new();
        push_AI(J); push_AO(J);
        seg_push(J, sL, Gtab, (uint32_t)n, 2);
        seg_push(J, sR, Htab, (uint32_t)n, 2);
        seg_push(J, I.extras.as<scm>() + 2, Bbn, 1, 2);
        const Impl::MsmTicket tk = I.msm(J, 3);
        I.wait_stream();
        const std::vector<h51::pt> P3 = I.msm_points(tk);
        for (int k = 0; k < 3; k++) h51::pt_compress(pts + 32 * k, P3[k]);
    } else {
        launch_pieces(2 * n);
        I.wait_stream();
        const std::vector<h51::pt> AB = I.msm_points(tk_aiao);
        h51::pt Sp = I.msm_points(tk_s[0])[0];
        for (uint32_t k = 1; k < nparts; k++) Sp = h51::pt_add(Sp, I.msm_points(tk_s[k])[0]);
        h51::pt_compress(pts, AB[0]); h51::pt_compress(pts + 32, AB[1]); h51::pt_compress(pts + 64, Sp);
    }
    lap(tm ? &tm->msm_s : nullptr);

    std::vector<uint8_t> proof;
    proof_open(proof, lgN, flags, pts);
    Scalar y, z;
    fs_commitments(T, pts, nullptr, flags, y, z);
    const Scalar yinv = y.invert();

    // ---- powers, flattened weights, t-polynomial
    // y^-i stays for the inner-product argument; y^i, z^j and the flattened weights are needed until k_poly_eval only: they take the arena between the
    // S sums (synchronised above) and the first multiscalar sum of the inner-product argument
    I.yinvpow.ensure(N * sizeof(scm));
    const size_t b_w = Impl::al256((c->ncols ? c->ncols : 1) * sizeof(scm)), b_z = Impl::al256((q + 2) * sizeof(scm)), b_y = Impl::al256(N * sizeof(scm));
    I.arena.ensure(b_w + b_z + b_y);
    scm *const wAll_p = reinterpret_cast<scm *>(I.arena_at(0)), *const zpow_p = reinterpret_cast<scm *>(I.arena_at(b_w)), *const ypow_p = reinterpret_cast<scm *>(I.arena_at(b_w + b_z));
    I.exp_tables({{y, ypow_p, N}, {yinv, I.yinvpow.as<scm>(), N}, {z, zpow_p, q + 1}});      // y^i, y^-i, z^j: one launch
    if (c->ncols > 1)      // every column but the last (constant terms: verifier only)
        BPG_LAUNCH(I, k_flatten, dim3(cdiv(c->ncols - 1, 256)), dim3(256), c->col_ptr.as<uint64_t>(), c->ent_row.as<uint32_t>(),
                           c->ent_coef.as<uint32_t>(), c->coef.as<scm>(), zpow_p, wAll_p, (uint32_t)(c->ncols - 1), (uint32_t)(3 * n));
    scm *wL = wAll_p, *wR = wL + n, *wO = wR + n, *wV = wO + n;
    const uint32_t pblocks = n ? std::min<uint32_t>(cdiv(n, 256), 1024) : 1;
    I.red_partial.ensure((size_t)pblocks * 6 * sizeof(scm) + 4096); I.red_out.ensure(16 * sizeof(scm));
    BPG_LAUNCH(I, k_poly_t, dim3(pblocks), dim3(256), c->aL.as<scm>(), c->aR.as<scm>(), c->aO.as<scm>(), sL, sR, wL, wR, wO,
                       ypow_p, I.yinvpow.as<scm>(), I.red_partial.as<scm>(), (uint32_t)n);
    BPG_LAUNCH(I, k_reduce_partials, dim3(6), dim3(256), I.red_partial.as<scm>(), pblocks, 6u, I.red_out.as<scm>());
    HIPCHK(hipGetLastError());
    scm h_t[6]; std::vector<scm> h_wV(m ? m : 1);
    HIPCHK(hipMemcpyAsync(h_t, I.red_out.p, 6 * sizeof(scm), hipMemcpyDeviceToHost, st));
    if (m) HIPCHK(hipMemcpyAsync(h_wV.data(), wV, m * sizeof(scm), hipMemcpyDeviceToHost, st));
    uint32_t *h_stale = reinterpret_cast<uint32_t *>(I.h_small.as<uint8_t>() + 32768);
    HIPCHK(hipMemcpyAsync(h_stale, I.stale_flag.p, 4, hipMemcpyDeviceToHost, st));
    I.wait_stream();
    if (*h_stale) {   // a blinding draw was read from a slab position no upload of this proof wrote (k_sc_from_wide): nothing of this proof may leave
        HIPCHK(hipMemsetAsync(I.stale_flag.p, 0, 4, st));
        throw DeviceError("a blinding draw was read before it was uploaded (stale device slab): proof withheld");
    }
    Scalar t[7], tb[7];
    for (int k = 0; k < 6; k++) t[k + 1] = from_scm(h_t[k]);
    Scalar u_ch, x;
    uint8_t vv[5 * 32], rr[5 * 32], tcom[5 * 32];       // T_1, T_3, T_4, T_5, T_6 = t_k * B + tau_k * B_blinding
    poly_commit_inputs(rng, t, tb, vv, rr);
    pedersen_commit(5, vv, rr, tcom);
    fs_poly_commitments(T, tcom, u_ch, x);
    proof.insert(proof.end(), tcom, tcom + 160);
    const PolyAtX px = poly_at_x(t, tb, [&](uint64_t j) { return from_scm(h_wV[j]); }, v_blinding, ib, ob, sb, x);
    const Scalar w = fs_poly_scalars(T, px.tx, px.txb, px.eb);
    proof_poly_scalars(proof, px);

    I.lv.ensure(N * sizeof(scm)); I.rv.ensure(N * sizeof(scm));
    BPG_LAUNCH(I, k_poly_eval, dim3(cdiv(N, 256)), dim3(256), c->aL.as<scm>(), c->aR.as<scm>(), c->aO.as<scm>(), sL, sR, wL, wR, wO,
                       ypow_p, I.yinvpow.as<scm>(), to_scm(x), I.lv.as<scm>(), I.rv.as<scm>(), (uint32_t)n, (uint32_t)N);
    HIPCHK(hipGetLastError());
    lap(tm ? &tm->poly : nullptr);

    // ---- inner-product argument
    I.inner_product(T, proof, n, N, yinv, u_ch, w, Gtab, Htab, Bn, tm, t0);
    if (tm) { tm->ipa = tm->ipa_msm + tm->ipa_fold; tm->total += now_ms() - t_begin; }
    return proof;
}

// ------------------------------------------------------------------------------------------------ lockstep batch proving (include/bpg.h bpg_r1cs_prove_batch)
// K proofs of circuits with N <= 2^tt_orig_lg run prove()'s table-driven path together: every device stage is one launch for all items of a wave
// (hip/k_batch.cuh), and the Fiat-Shamir work of the items between two stages runs on a few host threads.  The draws and the transcript operations of
// each item happen in exactly prove()'s order, and every point and scalar is computed by the same arithmetic, so each proof is byte-identical.
namespace {
// host threads of a batch: the cores this process may run on (its affinity mask: what bench.py's rank placement sets), capped by the cgroup CPU quota,
// and never more than 16
uint32_t batch_host_threads() {
    cpu_set_t set; CPU_ZERO(&set);
    long n = sched_getaffinity(0, sizeof set, &set) == 0 ? CPU_COUNT(&set) : 1;
    if (FILE *f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char quota[32] = {0}; long period = 0;
        if (std::fscanf(f, "%31s %ld", quota, &period) == 2 && std::strcmp(quota, "max") != 0 && period > 0) n = std::min(n, std::max(1L, (std::atol(quota) + period - 1) / period));
        std::fclose(f);
    }
    return (uint32_t)std::max(1L, std::min(n, 16L));
}
// fn(lo, hi) over chunks of [0, count) on the caller and nthreads - 1 helpers that live for the whole call
class StageThreads {
public:
    explicit StageThreads(uint32_t n) { for (uint32_t t = 1; t < n; t++) th_.emplace_back([this] { loop(); }); }
    ~StageThreads() { { std::lock_guard<std::mutex> lk(mu_); quit_ = true; } cv_.notify_all(); for (std::thread &t : th_) t.join(); }
    void run(size_t count, const std::function<void(size_t, size_t)> &fn) {
        const size_t parts = std::min<size_t>(count, 4 * (th_.size() + 1));
        if (parts <= 1 || th_.empty()) { if (count) fn(0, count); return; }
        { std::lock_guard<std::mutex> lk(mu_); fn_ = &fn; count_ = count; parts_ = parts; next_.store(0); busy_.store((int)th_.size()); gen_++; }
        cv_.notify_all();
        work();
        while (busy_.load(std::memory_order_acquire) != 0) std::this_thread::yield();
        fn_ = nullptr;
        if (err_) { std::exception_ptr e = err_; err_ = nullptr; std::rethrow_exception(e); }
    }
private:
    void work() {
        try {
            for (size_t p; (p = next_.fetch_add(1)) < parts_;) (*fn_)(count_ * p / parts_, count_ * (p + 1) / parts_);
        } catch (...) { std::lock_guard<std::mutex> lk(err_mu_); if (!err_) err_ = std::current_exception(); next_.store(parts_); }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            { std::unique_lock<std::mutex> lk(mu_); cv_.wait(lk, [&] { return quit_ || gen_ != seen; }); if (quit_) return; seen = gen_; }
            work();
            busy_.fetch_sub(1, std::memory_order_release);
        }
    }
    std::vector<std::thread> th_;
    std::mutex mu_, err_mu_; std::condition_variable cv_;
    bool quit_ = false; uint64_t gen_ = 0;
    const std::function<void(size_t, size_t)> *fn_ = nullptr;
    size_t count_ = 0, parts_ = 0;
    std::atomic<size_t> next_{0}; std::atomic<int> busy_{0};
    std::exception_ptr err_;
};
// x[i] -> x[i]^-1 for i in [lo, hi) with one inversion (Montgomery's trick); a zero stays zero, as Scalar::invert leaves it
void batch_invert(Scalar *x, Scalar *out, size_t lo, size_t hi) {
    std::vector<Scalar> pre(hi - lo);
    Scalar acc = Scalar::one();
    for (size_t i = lo; i < hi; i++) { pre[i - lo] = acc; if (!x[i].is_zero_mod_l()) acc = acc * x[i]; }
    Scalar inv = acc.invert();
    for (size_t i = hi; i-- > lo;) {
        if (x[i].is_zero_mod_l()) { out[i] = Scalar::zero(); continue; }
        out[i] = inv * pre[i - lo]; inv = inv * x[i];
    }
}
}  // namespace

bool Engine::lockstep_eligible(uint64_t n, uint32_t flags) const {
    const uint32_t lg = impl_->tt_orig_lg;
    return n > 0 && !(flags & 4u) && lg > 0 && ceil_log2(n) <= lg;
}

bool Engine::template_lockstep(const DeviceCircuit *d) { return d && d->is_template && d->has_host; }
bool Engine::is_repeat(const DeviceCircuit *d) { return d && d->rep_count != 0; }
void Engine::drop_witness(DeviceCircuit *d) {
    d->has_witness = false;
    d->merge_tried = false; d->mI.groups = d->mI.skipped = 0; d->mO.groups = d->mO.skipped = 0;
}
void Engine::prove_template_batch(DeviceCircuit *d, size_t count, ProveItem *items, bool commit, bool checkpointed) {
    if (!template_lockstep(d)) throw std::logic_error("prove_template_batch: the circuit is not a template with a host copy of its rows");
    if (d->n_ck && !checkpointed) throw std::invalid_argument("prove_template_batch: the template has checkpoints, and a batch item carries no values for them");
    for (size_t k = 0; k < count && d->n_in; k++)
        if (!items[k].inputs) throw std::invalid_argument("prove_template_batch: the template has public inputs, and an item carries no values for them");
    drop_witness(d);
    for (size_t k = 0; k < count; k++) {
        if (!items[k].values && d->m) throw std::invalid_argument("prove_template_batch: an item without committed values");
        if (!items[k].params && d->n_params) throw std::invalid_argument("prove_template_batch: an item without parameter values");
        if (!items[k].ck && d->n_ck) throw std::invalid_argument("prove_template_batch: an item without checkpoint values");
        items[k].flat = &d->host_view; items[k].ck_first = CHECKPOINTS_HOLD;
    }
    prove_batch(count, items, d, commit && d->m);       // (a template with n_ck > 0 gets this far only when the items carry the values: the waves read d->n_ck)
    // an item whose checkpoint values were not the circuit's own rode its wave to the end: nothing it made leaves this call
    for (size_t k = 0; k < count; k++) if (items[k].ck_first != CHECKPOINTS_HOLD) { items[k].proof.clear(); items[k].commitments.clear(); }
}

namespace {
using ProveItem = Engine::ProveItem;
// ---- wave planning: groups of equal lg N, waves of at most `cap` bytes of device state (and index ranges the 29-bit variable field of the upload holds)
// n_ck: the checkpoint values every item of a checkpointed template wave brings (raw in the pinned area and its mirror, reduced behind them, 4 bytes of result);
// n_in: the public inputs every item of a wave of a template with inputs brings (raw, mirrored and reduced likewise; their derived slots are coefficients of f)
std::vector<std::vector<ProveItem *>> plan_waves(size_t count, ProveItem *items, uint64_t cap, uint64_t n_ck, uint64_t n_in) {
    std::vector<size_t> order(count);
    for (size_t k = 0; k < count; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return ceil_log2(items[a].flat->n) < ceil_log2(items[b].flat->n); });
    auto item_bytes = [&](const FlatView &f, uint64_t N) { return 28 * N * 32 + f.q * 48 + f.nnz * 24 + f.ncoef * 64 + f.m * 32 + n_ck * 64 + (n_ck ? 4 : 0) + n_in * 64 + 1024; };
    std::vector<std::vector<ProveItem *>> waves;
    for (size_t g0 = 0; g0 < count;) {
        const uint32_t lgN = ceil_log2(items[order[g0]].flat->n);
        const uint64_t N = 1ull << lgN;
        size_t g1 = g0; uint64_t bytes = 0;
        while (g1 < count && ceil_log2(items[order[g1]].flat->n) == lgN) {
            const uint64_t b = item_bytes(*items[order[g1]].flat, N);
            if (g1 > g0 && (bytes + b > cap || (g1 - g0 + 1) * N > (1ull << 26) || g1 - g0 >= 16384)) break;
            bytes += b; g1++;
        }
        waves.emplace_back();
        for (; g0 < g1; g0++) waves.back().push_back(&items[order[g0]]);
    }
    return waves;
}

// ---- where everything of one wave lives: the items' offsets in the packed (block-diagonal) instance, the pinned area and the device area.
// from_values: the witness area holds the items' committed values (a template wave) where a host-assembled wave uploads 3 K N witness scalars;
// commit: the reduced blindings of the commitments lie right behind them, and the two go up ahead of the rest (up_begin).  n_ck > 0 (a checkpointed
// template wave): K n_ck checkpoint values, item-major, behind those and ahead of the coefficients - inside the range a committing wave sends ahead, because
// it queues the witness evaluation before upload().  n_in > 0 (a template with public inputs): K n_in input values, item-major, right behind them
struct WaveLayout {
    size_t K; uint32_t lgN; uint64_t N, KN, qT, nnzT, ncoefT, mT, ckT, inT, ncols, nvar, qmax = 0;
    std::vector<uint64_t> rbase, ebase, cbase, vbase;
    uint32_t nblkC, nblkR, pblocks;
    // pinned upload area [0, up_bytes), mirrored 1:1 on the device, then the read-back area
    size_t o_wit, o_vbl, o_ck, o_in, o_coef, o_raw, o_rp, o_tv, o_tc, o_nk, o_qk, o_rb, o_bsc, o_bases, up_begin, up_bytes, o_back, pin_bytes;
    // device, behind the mirror: the scalar vectors, the transposed matrix and the workspace
    size_t d_abc, d_coef, d_sLR, d_ypow, d_yinv, d_z, d_w, d_lv, d_rv, d_fG, d_fH, d_c, d_tpart, d_t, d_ab, d_colptr, d_erow, d_ecoef, d_counts, d_starts, d_cursor,
           d_rowc, d_rowcs, d_bsum, d_part, d_pts, d_comp, d_misc, d_v, d_vcom, d_ck, d_ckfirst, d_in, dev_bytes;
    WaveLayout(const std::vector<ProveItem *> &W, bool from_values, bool commit, uint64_t n_ck, uint64_t n_in)
        : K(W.size()), lgN(ceil_log2(W[0]->flat->n)), N(1ull << lgN), KN(K * N), ckT(from_values ? K * n_ck : 0), inT(from_values ? K * n_in : 0), rbase(K + 1), ebase(K + 1), cbase(K + 1), vbase(K + 1) {
        for (size_t k = 0; k < K; k++) {
            const FlatView &f = *W[k]->flat;
            rbase[k + 1] = rbase[k] + f.q; ebase[k + 1] = ebase[k] + f.nnz; cbase[k + 1] = cbase[k] + f.ncoef; vbase[k + 1] = vbase[k] + f.m;
            qmax = std::max<uint64_t>(qmax, f.q);
        }
        qT = rbase[K]; nnzT = ebase[K]; ncoefT = cbase[K]; mT = vbase[K];
        ncols = 3 * KN + mT + 1; nvar = ncols - 1;
        if (qT >= (1ull << 32) || nnzT >= (1ull << 32) || ncols >= (1ull << 29)) throw std::invalid_argument("prove_batch: wave too large");
        nblkC = cdiv(16 * N, 256); nblkR = cdiv(8 * N, 256); pblocks = std::min<uint32_t>(cdiv(N, 256), 1024);
        size_t off = 0;
        auto take = [&](size_t b) { const size_t o = off; off += Engine::Impl::al256(b ? b : 1); return o; };
        o_wit = take(from_values ? mT * 32 : 3 * KN * 32); o_vbl = take(commit ? mT * 32 : 0); o_ck = take(ckT * 32); o_in = inT ? take(inT * 32) : off; o_coef = take(ncoefT * 32); o_raw = take(2 * KN * 64);
        o_rp = take((qT + 1) * 8); o_tv = take(nnzT * 4); o_tc = take(nnzT * 4); o_nk = take(K * 4); o_qk = take(K * 4); o_rb = take(K * 4);
        o_bsc = take(K * BSC * 32); o_bases = take(K * 3 * 32);
        up_begin = commit ? o_coef : 0; up_bytes = off;
        o_back = take(std::max<size_t>(K * 3 * 32 + 64 + K * 4, (6 * K + mT + 1) * 32 + 64));        // (commit3: A_I, A_O, S, the totals, the checkpoint results)
        pin_bytes = off;
        d_abc = take(3 * KN * 32); d_coef = take(ncoefT * 32); d_sLR = take(2 * KN * 32); d_ypow = take(KN * 32); d_yinv = take(KN * 32);
        d_z = take((qT + 1) * 32); d_w = take(ncols * 32); d_lv = take(KN * 32); d_rv = take(KN * 32); d_fG = take(KN * 32); d_fH = take(KN * 32);
        d_c = take(4 * KN * 32); d_tpart = take((size_t)pblocks * 6 * K * 32); d_t = take(6 * K * 32); d_ab = take(2 * K * 32);
        // the transposition workspace by the one size rule (host/csc_work.hpp): counts is the second scan's scratch too, qT words of it.  (It was nvar + 2
        // words here: a wave of tall items - more rows than 3 K N + mT - had that scan write on into starts and cursor, which k_csc_colptr and k_csc_fill read)
        const CscWorkWords ws = csc_work_words(nvar, qT);
        d_colptr = take((ncols + 1) * 8); d_erow = take(nnzT * 4); d_ecoef = take(nnzT * 4); d_counts = take(ws.counts * 4);
        d_starts = take(ws.starts * 4); d_cursor = take(ws.cursor * 4); d_rowc = take(ws.rowconst * 4); d_rowcs = take(ws.rowconst_start * 4);
        d_bsum = take(ws.bsum * 4); d_part = take((size_t)K * std::max(3 * nblkC, 2 * nblkR) * sizeof(ge_ext));
        d_pts = take(K * 3 * sizeof(ge_ext)); d_comp = take(K * 3 * 32); d_misc = take(64); d_v = take(from_values ? mT * 32 : 0);
        d_vcom = take(commit ? mT * 32 : 0); d_ck = take(ckT * 32); d_ckfirst = take(ckT ? K * 4 : 0);
        d_in = inT ? take(inT * 32) : off;
        dev_bytes = off;
    }
};

// ONE set of window tables of the original generators for every wave of a batch, and the kernel variant the batch took
struct BatchTables { const ge_pniels *table, *tabB, *tabBb; uint32_t M0T, quad; };

// ---- one wave: its buffers, the host state of its items between two stages, and the stages in the order prove_batch() calls them.  Where a_L, a_R, a_O
// come from (tmpl, commit) is read by make_commitments(), by witness_and_scalars() and by its host half pack_witness() only; every other stage works on the
// wave's a_L, a_R, a_O and on what WaveLayout laid out, and must stay that way
struct Wave {
    Engine &E; Engine::Impl &I; StageThreads &pool; const BatchTables &B;
    const std::vector<ProveItem *> &W; const DeviceCircuit *tmpl; const bool commit;
    const WaveLayout L;
    const size_t K; const uint64_t N, KN; const uint32_t lgN;
    uint8_t *pin, *dev, *back, *comp;
    template <class T> T *D(size_t o) const { return reinterpret_cast<T *>(dev + o); }
    scm *aL, *aR, *aO, *sL, *sR, *ypow, *yinvpow, *wL, *wR, *wO, *wV, *lv, *rv, *bsc, *h_bsc, *fG, *fH, *cc;
    uint32_t *stale, *totals; const uint32_t *nk;
    ge_ext *part, *pts;
    std::vector<TranscriptRng> rng;
    std::vector<Scalar> ib, ob, sb, y, yinv, z, u, uinv;
    std::vector<std::array<Scalar, 7>> tk, tbk;

    Wave(Engine &E_, Engine::Impl &I_, StageThreads &pool_, const BatchTables &B_, const std::vector<ProveItem *> &W_, const DeviceCircuit *tmpl_, bool commit_)
        : E(E_), I(I_), pool(pool_), B(B_), W(W_), tmpl(tmpl_), commit(commit_), L(W, tmpl_ != nullptr, commit_, tmpl_ ? tmpl_->n_ck : 0, tmpl_ ? tmpl_->n_in : 0), K(L.K), N(L.N), KN(L.KN), lgN(L.lgN),
          ib(K), ob(K), sb(K), y(K), yinv(K), z(K), u(K), uinv(K), tk(K), tbk(K) {
        I.bt_pin.ensure(L.pin_bytes); I.bt_dev.ensure(L.dev_bytes);
        pin = I.bt_pin.as<uint8_t>(); dev = I.bt_dev.as<uint8_t>(); back = pin + L.o_back; comp = dev + L.d_comp;
        aL = D<scm>(L.d_abc); aR = aL + KN; aO = aR + KN; sL = D<scm>(L.d_sLR); sR = sL + KN;
        ypow = D<scm>(L.d_ypow); yinvpow = D<scm>(L.d_yinv); wL = D<scm>(L.d_w); wR = wL + KN; wO = wR + KN; wV = wO + KN;
        lv = D<scm>(L.d_lv); rv = D<scm>(L.d_rv); bsc = D<scm>(L.o_bsc); h_bsc = reinterpret_cast<scm *>(pin + L.o_bsc);
        fG = D<scm>(L.d_fG); fH = D<scm>(L.d_fH); cc = D<scm>(L.d_c);
        stale = D<uint32_t>(L.d_misc); totals = stale + 4; nk = D<uint32_t>(L.o_nk);
        part = D<ge_ext>(L.d_part); pts = D<ge_ext>(L.d_pts);
    }

    // the wave's witnesses: committed values reduced once for the whole wave, padding rows [n, N) of the 3 K vectors zeroed (one strided fill), then one
    // launch per level with a lane per (segment, item).  A checkpointed template: the items' checkpoint values are reduced as the committed values are, the
    // levels are those of the checkpointed schedule, and one more launch leaves every item's lowest mismatch (all ones: none) where commit3() copies it back
    void reduce_values() {
        if (L.mT) BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(L.mT, 256)), dim3(256), D<const uint32_t>(L.o_wit), D<scm>(L.d_v), (uint32_t)L.mT);
        if (L.ckT) BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(L.ckT, 256)), dim3(256), D<const uint32_t>(L.o_ck), D<scm>(L.d_ck), (uint32_t)L.ckT);
        if (L.inT) BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(L.inT, 256)), dim3(256), D<const uint32_t>(L.o_in), D<scm>(L.d_in), (uint32_t)L.inT);
    }
    void eval_witnesses() {
        const uint64_t n = tmpl->n;
        const uint32_t n_ck = L.ckT ? (uint32_t)tmpl->n_ck : 0;
        if (N > n) HIPCHK(hipMemset2DAsync(aL + n, N * sizeof(scm), 0, (N - n) * sizeof(scm), 3 * K, I.st));
        for (size_t l = 0; l + 1 < tmpl->wit_level_ptr.size(); l++) {
            const uint32_t s0 = tmpl->wit_level_ptr[l], ns = tmpl->wit_level_ptr[l + 1] - s0;
            BPG_LAUNCH(I, k_witness_eval_batch, dim3(cdiv(K, 64), ns), dim3(64), tmpl->wit_segs.as<uint4>() + s0, tmpl->wit_stream.as<uint32_t>(),
                       tmpl->coef.as<scm>(), D<const scm>(L.d_v), D<const scm>(L.d_ck), n_ck, D<const scm>(L.d_in), L.inT ? (uint32_t)tmpl->n_in : 0u, (uint32_t)tmpl->m, lgN,
                       (uint32_t)K, aL, aR, aO);
        }
        if (!n_ck) return;
        HIPCHK(hipMemsetAsync(dev + L.d_ckfirst, 0xff, K * 4, I.st));
        BPG_LAUNCH(I, k_witness_ck_verify_batch, dim3(cdiv(L.ckT, 256)), dim3(256), tmpl->wit_ck_var.as<uint32_t>(), n_ck, (uint64_t)L.ckT, lgN, D<const scm>(L.d_ck),
                   aL, aR, aO, D<uint32_t>(L.d_ckfirst));
    }
    // ---- stage 1, a committing wave only: values and reduced blindings go up first, ONE launch makes the K m encodings from the reduced values the witness
    // evaluation reads, one copy brings them back; the witness evaluation is queued behind and runs while the host threads append the encodings as "V" -
    // the transcripts are needed next, by the stage that draws the blindings of A_I
    void make_commitments() {
        if (!commit) return;
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const uint64_t m = W[k]->flat->m;
                std::memcpy(pin + L.o_wit + 32 * L.vbase[k], W[k]->values, 32 * m);
                for (uint64_t j = 0; j < m; j++) (*W[k]->vb)[j].to_bytes(pin + L.o_vbl + 32 * (L.vbase[k] + j));     // reduced, as pedersen_commit uploads them
                pack_checkpoints(k);
            }
        });
        if (!I.commit_ev) I.commit_ev = Event::untimed();
        HIPCHK(hipMemcpyAsync(dev + L.o_wit, pin + L.o_wit, L.o_coef - L.o_wit, hipMemcpyHostToDevice, I.st));
        reduce_values();
        BPG_LAUNCH(I, k_bt_commit_v, dim3(cdiv(L.mT, 4 * I.commit_cpw)), dim3(256), D<const scm>(L.d_v), D<const uint32_t>(L.o_vbl),
                   I.ped_table.as<ge_pniels>(), dev + L.d_vcom, (uint32_t)L.mT, I.commit_cpw);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(back, dev + L.d_vcom, L.mT * 32, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipEventRecord(I.commit_ev, I.st));
        eval_witnesses();
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventSynchronize(I.commit_ev));
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const uint64_t m = W[k]->flat->m;
                const uint8_t *com = back + 32 * L.vbase[k];
                W[k]->commitments.assign(com, com + 32 * m);
                for (uint64_t j = 0; j < m; j++) W[k]->T->append_point("V", com + 32 * j);
            }
        });
    }
    // item k's checkpoint values, raw, at its place in the wave's list (a committing wave: before the range goes up ahead of the rest)
    void pack_checkpoints(size_t k) {
        if (L.ckT) std::memcpy(pin + L.o_ck + 32 * k * tmpl->n_ck, W[k]->ck, 32 * tmpl->n_ck);
        if (L.inT) std::memcpy(pin + L.o_in + 32 * k * tmpl->n_in, W[k]->inputs, 32 * tmpl->n_in);       // the item's public inputs travel beside them
    }
    // what item k uploads for its witness: the three vectors padded to N, or (a template) its committed values and its constant terms in the parameter
    // slots of ITS range of the wave's coefficient table
    void pack_witness(size_t k) {
        const FlatView &f = *W[k]->flat;
        const uint8_t *src[3] = {f.aL, f.aR, f.aO};
        for (int v = 0; v < 3 && !tmpl; v++) {
            uint8_t *dst = pin + L.o_wit + 32 * (v * KN + k * N);
            std::memcpy(dst, src[v], 32 * f.n); std::memset(dst + 32 * f.n, 0, 32 * (N - f.n));
        }
        if (f.ncoef) std::memcpy(pin + L.o_coef + 32 * L.cbase[k], f.coef, 32 * f.ncoef);
        if (tmpl) {
            if (f.m) std::memcpy(pin + L.o_wit + 32 * L.vbase[k], W[k]->values, 32 * f.m);
            if (!commit) pack_checkpoints(k);
            if (tmpl->n_params) std::memcpy(pin + L.o_coef + 32 * (L.cbase[k] + tmpl->param_first), W[k]->params, 32 * tmpl->n_params);
        }
    }
    // ---- stage 2, host, per item: transcript, RNG, the first three blindings and the 2n draws, packed with the instance
    void pack_and_draw() {
        rng.reserve(K);
        for (size_t k = 0; k < K; k++) { W[k]->T->append_u64("m", W[k]->flat->m); rng.push_back(W[k]->T->build_rng(*W[k]->vb, W[k]->seed)); }
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const FlatView &f = *W[k]->flat;
                const uint64_t n = f.n, b = k * N;
                ib[k] = rng[k].random_scalar(); ob[k] = rng[k].random_scalar(); sb[k] = rng[k].random_scalar();
                h_bsc[k * BSC + 0] = to_scm(ib[k]); h_bsc[k * BSC + 1] = to_scm(ob[k]); h_bsc[k * BSC + 2] = to_scm(sb[k]);
                // s_L then s_R: 64 uniform bytes each, in prove()'s order; the padding draws are zero
                uint8_t *raw = pin + L.o_raw;
                rng[k].fill_draws64(raw + 64 * b, n); std::memset(raw + 64 * (b + n), 0, 64 * (N - n));
                rng[k].fill_draws64(raw + 64 * (KN + b), n); std::memset(raw + 64 * (KN + b + n), 0, 64 * (N - n));
                pack_witness(k);
                // the block-diagonal matrix: rows after the earlier items' rows, multiplier i of item k -> column k*N + i of its block (L, R, O),
                // committed j -> 3KN + vbase + j; coefficient indices after the earlier items' coefficients
                uint64_t *rp = reinterpret_cast<uint64_t *>(pin + L.o_rp) + L.rbase[k];
                for (uint64_t r = 0; r < f.q; r++) rp[r] = L.ebase[k] + f.row_ptr[r];
                uint32_t *tv = reinterpret_cast<uint32_t *>(pin + L.o_tv) + L.ebase[k], *tc = reinterpret_cast<uint32_t *>(pin + L.o_tc) + L.ebase[k];
                for (uint64_t e = 0; e < f.nnz; e++) {
                    const uint32_t pv = f.term_var[e], kind = pv >> 29, idx = pv & 0x1fffffffu;
                    tv[e] = kind <= 2 ? (kind << 29) | (uint32_t)(b + idx) : (kind == 3 ? (3u << 29) | (uint32_t)(L.vbase[k] + idx) : pv);
                    tc[e] = (uint32_t)L.cbase[k] + f.term_coef[e];
                }
                reinterpret_cast<uint32_t *>(pin + L.o_nk)[k] = (uint32_t)n;
                reinterpret_cast<uint32_t *>(pin + L.o_qk)[k] = (uint32_t)f.q;
                reinterpret_cast<uint32_t *>(pin + L.o_rb)[k] = (uint32_t)L.rbase[k];
            }
        });
        reinterpret_cast<uint64_t *>(pin + L.o_rp)[L.qT] = L.nnzT;
    }
    // ---- stage 3: one upload (what a committing wave sent ahead is up already)
    void upload() {
        HIPCHK(hipMemcpyAsync(dev + L.up_begin, pin + L.up_begin, L.up_bytes - L.up_begin, hipMemcpyHostToDevice, I.st));
        HIPCHK(hipMemsetAsync(stale, 0, 64, I.st));
    }
    // ---- stage 4, the witness source: a_L, a_R, a_O from wherever this wave has them; then coefficients and draws to scalars
    void witness_and_scalars() {
        if (!tmpl) BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(3 * KN, 256)), dim3(256), D<const uint32_t>(L.o_wit), aL, (uint32_t)(3 * KN));
        else if (!commit) { reduce_values(); eval_witnesses(); }       // (a committing wave queued them behind its commitments)
        if (L.ncoefT) BPG_LAUNCH(I, k_sc_from_bytes, dim3(cdiv(L.ncoefT, 256)), dim3(256), D<const uint32_t>(L.o_coef), D<scm>(L.d_coef), (uint32_t)L.ncoefT);
        // a template with public inputs: every item's derived slots in ITS range of the table (all items share the template's rows: one stride), where the
        // parameter slots were patched on the host - before the flattening reads a constant term
        if (L.inT && tmpl->n_slots) BPG_LAUNCH(I, k_input_slots, dim3(cdiv(K * tmpl->n_slots, 256)), dim3(256), tmpl->in_slots.as<uint2>(), (uint32_t)tmpl->n_slots,
                                               (uint32_t)tmpl->slot_first, (uint32_t)W[0]->flat->ncoef, (uint32_t)tmpl->n_in, (uint64_t)(K * tmpl->n_slots),
                                               D<const scm>(L.d_in), D<scm>(L.d_coef));
        BPG_LAUNCH(I, k_sc_from_wide, dim3(cdiv(2 * KN, 256)), dim3(256), D<const uint32_t>(L.o_raw), sL, (uint32_t)(2 * KN), stale);
    }
    // ---- stage 5: the block-diagonal CSR -> CSC in one pass, as upload() transposes a single instance
    void transpose() {
        I.transpose_csr(D<const uint64_t>(L.o_rp), D<const uint32_t>(L.o_tv), D<const uint32_t>(L.o_tc), L.qT, KN, L.mT,
                        {D<uint32_t>(L.d_counts), D<uint32_t>(L.d_starts), D<uint32_t>(L.d_cursor), D<uint32_t>(L.d_rowc), D<uint32_t>(L.d_rowcs), D<uint32_t>(L.d_bsum)},
                        D<uint64_t>(L.d_colptr), D<uint32_t>(L.d_erow), D<uint32_t>(L.d_ecoef), totals);
    }
    // ---- stage 6: A_I, A_O, S of every item on the window tables, encoded on the device
    void commit3() {
        BPG_LAUNCH(I, k_bt_commit3, dim3(L.nblkC, 3, (uint32_t)K), dim3(256), B.table, B.M0T, aL, aR, aO, sL, sR, nk, lgN, part, B.quad);
        BPG_LAUNCH(I, k_bt_commit3_finish, dim3(3, (uint32_t)K), dim3(256), part, L.nblkC, bsc, B.tabBb, pts, B.quad);
        BPG_LAUNCH(I, k_bt_compress, dim3(cdiv(3 * K, 64)), dim3(64), pts, comp, (uint32_t)(3 * K));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(back, comp, 3 * K * 32, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipMemcpyAsync(back + 3 * K * 32, totals, 8, hipMemcpyDeviceToHost, I.st));
        if (L.ckT) HIPCHK(hipMemcpyAsync(back + 3 * K * 32 + 64, dev + L.d_ckfirst, K * 4, hipMemcpyDeviceToHost, I.st));
        I.wait_stream();
        if (reinterpret_cast<const uint32_t *>(back + 3 * K * 32)[1] != L.nnzT) throw std::logic_error("prove_batch: transposition lost entries");
        // a checkpointed wave: which items were handed values that are not the circuit's own.  Such an item stays in the wave - nothing of the plan changes -
        // and prove_template_batch() throws away what it made
        for (size_t k = 0; k < K && L.ckT; k++) {
            const uint32_t first = reinterpret_cast<const uint32_t *>(back + 3 * K * 32 + 64)[k];
            if (first != 0xffffffffu) W[k]->ck_first = first;
        }
    }
    // ---- stage 7: host: A_I1, A_O1, S1 -> y, z of every item; device: powers, flattened weights (block-diagonal CSC, z indexed by global row), t-polynomial
    void poly_t() {
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                proof_open(W[k]->proof, lgN, W[k]->flags, back + 96 * k);
                fs_commitments(*W[k]->T, back + 96 * k, nullptr, W[k]->flags, y[k], z[k]);
            }
            batch_invert(y.data(), yinv.data(), lo, hi);
            scm *hb = reinterpret_cast<scm *>(pin + L.o_bases);
            for (size_t k = lo; k < hi; k++) { hb[3 * k] = to_scm(y[k]); hb[3 * k + 1] = to_scm(yinv[k]); hb[3 * k + 2] = to_scm(z[k]); }
        });
        HIPCHK(hipMemcpyAsync(dev + L.o_bases, pin + L.o_bases, K * 3 * 32, hipMemcpyHostToDevice, I.st));
        const uint32_t lgT = std::min<uint32_t>(ceil_log2(std::max<uint64_t>(N, L.qmax)), 10);
        BPG_LAUNCH(I, k_bt_exp, dim3(cdiv(1u << lgT, 256), 3, (uint32_t)K), dim3(256), D<const scm>(L.o_bases), D<const uint32_t>(L.o_qk), D<const uint32_t>(L.o_rb),
                   lgN, lgT, ypow, yinvpow, D<scm>(L.d_z));
        BPG_LAUNCH(I, k_flatten, dim3(cdiv(L.nvar, 256)), dim3(256), D<const uint64_t>(L.d_colptr), D<const uint32_t>(L.d_erow), D<const uint32_t>(L.d_ecoef),
                   D<const scm>(L.d_coef), D<const scm>(L.d_z), wL, (uint32_t)L.nvar, (uint32_t)(3 * KN));
        BPG_LAUNCH(I, k_bt_poly_t, dim3(L.pblocks, (uint32_t)K), dim3(256), aL, aR, aO, sL, sR, wL, wR, wO, ypow, yinvpow, nk, lgN, D<scm>(L.d_tpart));
        BPG_LAUNCH(I, k_reduce_partials, dim3((uint32_t)(6 * K)), dim3(256), D<const scm>(L.d_tpart), L.pblocks, (uint32_t)(6 * K), D<scm>(L.d_t));
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(back, dev + L.d_t, 6 * K * 32, hipMemcpyDeviceToHost, I.st));
        if (L.mT) HIPCHK(hipMemcpyAsync(back + 6 * K * 32, wV, L.mT * 32, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipMemcpyAsync(back + (6 * K + L.mT) * 32, stale, 4, hipMemcpyDeviceToHost, I.st));
        I.wait_stream();
        if (*reinterpret_cast<const uint32_t *>(back + (6 * K + L.mT) * 32)) throw DeviceError("a blinding draw of the batch did not reach the device: proofs withheld");
    }
    // ---- stage 8, host: t_k, tau_k -> T_1, T_3..T_6 of every item in ONE Pedersen launch; then u, x, t_x, its blinding, e_blinding, w
    void t_commitments() {
        const scm *h_t = reinterpret_cast<const scm *>(back), *h_wV = h_t + 6 * K;
        std::vector<uint8_t> vv(5 * K * 32), rr(5 * K * 32), tcom(5 * K * 32);
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                for (int j = 0; j < 6; j++) tk[k][j + 1] = from_scm(h_t[6 * k + j]);
                poly_commit_inputs(rng[k], tk[k].data(), tbk[k].data(), &vv[160 * k], &rr[160 * k]);
            }
        });
        E.pedersen_commit(5 * K, vv.data(), rr.data(), tcom.data());
        pool.run(K, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                ProveItem &it = *W[k];
                Scalar u_ch, x;
                fs_poly_commitments(*it.T, &tcom[160 * k], u_ch, x);
                it.proof.insert(it.proof.end(), &tcom[160 * k], &tcom[160 * k] + 160);
                const PolyAtX px = poly_at_x(tk[k].data(), tbk[k].data(), [&](uint64_t j) { return from_scm(h_wV[L.vbase[k] + j]); }, *it.vb, ib[k], ob[k], sb[k], x);
                const Scalar w = fs_poly_scalars(*it.T, px.tx, px.txb, px.eb);
                proof_poly_scalars(it.proof, px);
                it.T->innerproduct_domain_sep(N);
                h_bsc[k * BSC + BSC_X] = to_scm(x); h_bsc[k * BSC + BSC_UCH] = to_scm(u_ch); h_bsc[k * BSC + BSC_W] = to_scm(w);
            }
        });
        HIPCHK(hipMemcpyAsync(bsc, h_bsc, K * BSC * 32, hipMemcpyHostToDevice, I.st));
    }
    // ---- stage 9, device: l(x), r(x) and the factors of the frozen original generators
    void poly_eval() {
        BPG_LAUNCH(I, k_bt_poly_eval, dim3(cdiv(N, 256), (uint32_t)K), dim3(256), aL, aR, aO, sL, sR, wL, wR, wO, ypow, yinvpow, bsc, nk, lgN, lv, rv);
        if (lgN) BPG_LAUNCH(I, k_bt_factors, dim3(cdiv(N, 256), (uint32_t)K), dim3(256), yinvpow, bsc, nk, lgN, fG, fH, cc);
    }
    // ---- stage 10: the inner-product argument of every item: lg N table-driven rounds
    void ipa_rounds() {
        uint32_t cur = 0;
        for (uint32_t j = 0; j < lgN; j++) {
            const uint32_t h = (uint32_t)(N >> (j + 1));
            if (j > 0) {
                const uint32_t hadv = (uint32_t)(N >> j), cnt = 1u << (j - 1);
                BPG_LAUNCH(I, k_bt_advance, dim3(cdiv(std::max(hadv, cnt), 256), (uint32_t)K), dim3(256), lv, rv, bsc, hadv, cc, cur, cnt, lgN);
                cur ^= 1u;
            }
            BPG_LAUNCH(I, k_bt_round, dim3(L.nblkR, 2, (uint32_t)K), dim3(256), B.table, B.M0T, lv, rv, fG, fH, cc, cur, lgN, j, part, B.quad);
            BPG_LAUNCH(I, k_bt_finish, dim3(2, (uint32_t)K), dim3(256), part, L.nblkR, lv, rv, h, lgN, bsc, B.tabB, pts, B.quad);
            BPG_LAUNCH(I, k_bt_compress, dim3(cdiv(2 * K, 64)), dim3(64), pts, comp, (uint32_t)(2 * K));
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(back, comp, 2 * K * 32, hipMemcpyDeviceToHost, I.st));
            I.wait_stream();
            pool.run(K, [&](size_t lo, size_t hi) {
                for (size_t k = lo; k < hi; k++) {
                    const uint8_t *lr = back + 64 * k;
                    W[k]->proof.insert(W[k]->proof.end(), lr, lr + 64);
                    u[k] = fs_ipa_round(*W[k]->T, lr, lr + 32);
                }
                batch_invert(u.data(), uinv.data(), lo, hi);
                for (size_t k = lo; k < hi; k++) { h_bsc[k * BSC + BSC_U] = to_scm(u[k]); h_bsc[k * BSC + BSC_UINV] = to_scm(uinv[k]); }
            });
            HIPCHK(hipMemcpyAsync(bsc, h_bsc, K * BSC * 32, hipMemcpyHostToDevice, I.st));
        }
    }
    // ---- stage 11: the last round's scalar fold, then the final a, b of every item
    void final_ab() {
        BPG_LAUNCH(I, k_bt_fold_scalars, dim3(cdiv(K, 256)), dim3(256), lv, rv, bsc, lgN, D<scm>(L.d_ab), (uint32_t)K);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(back, dev + L.d_ab, 2 * K * 32, hipMemcpyDeviceToHost, I.st));
        I.wait_stream();
        const scm *h_ab = reinterpret_cast<const scm *>(back);
        for (size_t k = 0; k < K; k++) {
            uint8_t o[64]; from_scm(h_ab[2 * k]).to_bytes(o); from_scm(h_ab[2 * k + 1]).to_bytes(o + 32);
            W[k]->proof.insert(W[k]->proof.end(), o, o + 64);
        }
    }
};
}  // namespace

// tmpl != nullptr: every item is a fresh witness of that template (flat = its host copy; values, params per item).  commit (a template with m > 0): the
// transcripts come in as they are BEFORE the commitments; every wave makes its own (k_bt_commit_v) and appends them before anything is drawn
void Engine::prove_batch(size_t count, ProveItem *items, DeviceCircuit *tmpl, bool commit) {
    if (!count) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    ProvingGuard in_flight(device_);                // the whole batch is one proof in flight: its kernel variants are chosen once
    I.shared_now = I.shared_variants();
    uint32_t lgmax = 0;
    for (size_t k = 0; k < count; k++) {
        if (!lockstep_eligible(items[k].flat->n, items[k].flags)) throw std::logic_error("prove_batch: an item that is not lockstep-eligible");
        lgmax = std::max(lgmax, ceil_log2(items[k].flat->n));
    }
    require_gens_capacity(gens_cap_, 1ull << lgmax);
    // ONE set of window tables of the original generators, for the largest N of the batch (an item of smaller N reads the first N rows of each half)
    const uint32_t M0T = 1u << lgmax;
    I.tt_build(I.gens, I.gens + gens_cap_, I.bases.as<ge_niels>(), M0T, true);
    const BatchTables B{I.tt_table_p, I.ped_table.as<ge_pniels>(), I.ped_table.as<ge_pniels>() + (size_t)TT_WINDOWS * TT_MULTS, M0T, I.shared_now ? 0u : 1u};
    StageThreads pool(std::min<uint32_t>(batch_host_threads(), (uint32_t)std::max<size_t>(1, count / 8)));
    for (const std::vector<ProveItem *> &W : plan_waves(count, items, (uint64_t)I.batch_wave_mb << 20, tmpl ? tmpl->n_ck : 0, tmpl ? tmpl->n_in : 0)) {
        Wave w(*this, I, pool, B, W, tmpl, commit);
        w.make_commitments();
        w.pack_and_draw();
        w.upload();
        w.witness_and_scalars();
        w.transpose();
        w.commit3();
        w.poly_t();
        w.t_commitments();
        w.poly_eval();
        w.ipa_rounds();
        w.final_ab();
    }
}

// ------------------------------------------------------------------------------------------------ verify
// Verifier::verify (dalek r1cs/verifier.rs; reference call site src/bin/verifier.rs:89-90): Fiat-Shamir replay on the host,
// then ONE multiscalar multiplication of 2N + m + 2 lgN + 13 terms through the same bucket-method kernels; accept iff it is the identity.
namespace {
// (VerifyReplay and verify_replay: host/fiat_shamir.hpp)
// the compressed points of one replayed proof in the order of its MSM terms: A_I1, A_O1, S1, A_I2, A_O2, S2, V, T_1, T_3..T_6, L_k, R_k
void verify_points(const VerifyReplay &R, const uint8_t *V, uint8_t *out) {
    size_t o = 0;
    for (int k = 0; k < 6; k++) { std::memcpy(out + o, R.pA[k], 32); o += 32; }
    if (R.m) { std::memcpy(out + o, V, R.m * 32); o += R.m * 32; }
    for (int k = 0; k < 5; k++) { std::memcpy(out + o, R.pT[k], 32); o += 32; }
    for (uint32_t k = 0; k < R.lgN; k++) { std::memcpy(out + o, R.pLR + 64 * k, 32); o += 32; }
    for (uint32_t k = 0; k < R.lgN; k++) { std::memcpy(out + o, R.pLR + 64 * k + 32, 32); o += 32; }
}
// the scalars of those points, then of B and B_blinding (npts + 2 of them); wV: the m weights of V, then w_c.  rho: the proof's weight in a batch (nullptr: none)
void verify_small_scalars(const VerifyReplay &R, const scm *wV, const Scalar &delta, const Scalar *rho, std::vector<Scalar> &hs) {
    const Scalar &x = R.x, &r = R.r, &u_ch = R.u_ch;
    const Scalar wc = from_scm(wV[R.m]);
    const Scalar xx = x * x, rxx = r * xx, xxx = x * xx;
    hs.assign(R.npts() + 2, Scalar());
    size_t o = 0;
    hs[o++] = x; hs[o++] = xx; hs[o++] = xxx;
    hs[o++] = u_ch * x; hs[o++] = u_ch * xx; hs[o++] = u_ch * xxx;
    for (uint64_t j = 0; j < R.m; j++) hs[o++] = from_scm(wV[j]) * rxx;
    hs[o++] = r * x; hs[o++] = rxx * x; hs[o++] = rxx * xx; hs[o++] = rxx * xxx; hs[o++] = rxx * xx * xx;
    for (uint32_t k = 0; k < R.lgN; k++) hs[o++] = R.uk[k] * R.uk[k];
    for (uint32_t k = 0; k < R.lgN; k++) hs[o++] = R.ukinv[k] * R.ukinv[k];
    hs[o++] = R.w * (R.tx - R.ipa * R.ipb) + r * (xx * (wc + delta) - R.tx);      // B
    hs[o++] = -R.eb - r * R.txb;                                                  // B_blinding
    if (rho) for (Scalar &s : hs) s = s * *rho;
}
// y^-i (yinvpow), z^j, the flattened weights (w_c into wV[m]) and the s vector of one replayed proof, queued on the engine stream; all but y^-i in the
// arena, read by k_verify_scalars(_acc) and nothing later.  ch: the proof's challenges on the device
struct VerifyVecs { scm *wL, *wR, *wO, *wV, *svec; };
VerifyVecs verify_prep(Engine::Impl &I, const DeviceCircuit *c, const VerifyReplay &R, const IpaChallenges *ch) {
    const uint64_t n = c->n, q = c->q, N = R.N;
    I.red_partial.ensure((size_t)4096 * sizeof(scm)); I.red_out.ensure(16 * sizeof(scm));      // [0,1024): delta partials, [1024,1536): w_c partials
    I.yinvpow.ensure(N * sizeof(scm));
    // powers of z, the flattened weights and the s vector are read by k_verify_scalars and earlier kernels only: in the arena, ahead of the one MSM
    const size_t b_w = Engine::Impl::al256(c->ncols * sizeof(scm)), b_z = Engine::Impl::al256((q + 2) * sizeof(scm)), b_y = Engine::Impl::al256(N * sizeof(scm));
    I.arena.ensure(b_w + b_z + b_y);
    scm *const wAll_p = reinterpret_cast<scm *>(I.arena_at(0)), *const zpow_p = reinterpret_cast<scm *>(I.arena_at(b_w)), *const ypow_p = reinterpret_cast<scm *>(I.arena_at(b_w + b_z));
    const Engine::Impl::PowTable yinv_table{R.yinv, I.yinvpow.as<scm>(), N};
    I.flatten_weights(c, R.z, zpow_p, wAll_p, &yinv_table);          // y^-i and z^j in one launch, then the weights
    scm *wL = wAll_p, *wR = wL + n, *wO = wR + n, *wV = wO + n;      // wV[m] = w_c
    BPG_LAUNCH(I, k_ipa_s, dim3(cdiv(N, 256)), dim3(256), ch, ypow_p, R.lgN, (uint32_t)N);
    return VerifyVecs{wL, wR, wO, wV, ypow_p};
}
// the ONE multiscalar multiplication of a verification: lv, rv on the first N generators of each half, vfy_sc on the proofs' own points and on B, B_blinding
// behind them; true iff the sum is the identity.  Synchronises the stream
bool verify_msm(Engine::Impl &I, uint64_t N, uint32_t npts) {
    MsmJob J = job_new();
    seg_push(J, I.lv.as<scm>(), I.gens, (uint32_t)N, 0);
    seg_push(J, I.rv.as<scm>(), I.gens + I.gens_cap, (uint32_t)N, 0);
    seg_push(J, I.vfy_sc.as<scm>(), I.vfy_pts.as<ge_niels>(), npts, 0);
    seg_push(J, I.vfy_sc.as<scm>() + npts, I.bases.as<ge_niels>(), 2, 0);
    const Engine::Impl::MsmTicket tk = I.msm(J, 1);
    HIPCHK(hipStreamSynchronize(I.st));
    uint8_t out[32];
    h51::pt_compress(out, I.msm_points(tk)[0]);
    return std::memcmp(out, kIdentity, 32) == 0;
}
}  // namespace

// bpg_test_verify_replay: what verify() and verify_batch() decide on the host, without a device
R1CSError Engine::test_verify_replay(uint64_t n, uint64_t m, uint64_t gens_cap, Transcript &T, const uint8_t *proof, size_t proof_len, const uint8_t seed[32],
                                     uint32_t flags) {
    VerifyReplay R;
    return verify_replay(n, m, gens_cap, T, proof, proof_len, seed, flags, R);
}

// The scripted transcript of the bpg_test_*_scripted hooks: y, z, u, x, w, u_1 .. u_lgN for a circuit of n multipliers, checked before anything is launched
void Engine::script_transcript(Transcript &T, uint64_t n, const uint8_t *script, uint64_t script_len) {
    const uint32_t lgN = ceil_log2(padded_size(n));
    if (!script) throw std::invalid_argument("scripted: null script");
    if (script_len != 5 + (uint64_t)lgN) throw std::invalid_argument("scripted: a script for lg N = " + std::to_string(lgN) + " has " + std::to_string(5 + lgN) + " entries (y, z, u, x, w, u_1 .. u_lgN), not " + std::to_string(script_len));
    std::vector<Scalar> s(script_len);
    for (uint64_t k = 0; k < script_len; k++) {
        std::memcpy(s[k].w, script + 32 * k, 32);
        if (!s[k].is_canonical()) throw std::invalid_argument("scripted: entry " + std::to_string(k) + " is not canonical");
        if ((k == 0 || k >= 5) && (s[k].w[0] | s[k].w[1] | s[k].w[2] | s[k].w[3]) == 0) throw std::invalid_argument("scripted: entry " + std::to_string(k) + " is zero (y and every u_k are inverted)");
    }
    T.attach_script(std::move(s));
}

// bpg_test_verify_replay_scripted: the same replay, with the challenges it drew (y, z, u, x, w, u_1 .. u_lgN as far as it got) and how many script entries it took
R1CSError Engine::test_verify_replay_scripted(uint64_t n, uint64_t m, uint64_t gens_cap, Transcript &T, const uint8_t *proof, size_t proof_len, const uint8_t seed[32],
                                              uint32_t flags, uint8_t *challenges_out, uint64_t *consumed_out) {
    VerifyReplay R;
    const R1CSError e = verify_replay(n, m, gens_cap, T, proof, proof_len, seed, flags, R);
    const Scalar *five[5] = {&R.y, &R.z, &R.u_ch, &R.x, &R.w};
    for (int k = 0; k < 5; k++) five[k]->to_bytes(challenges_out + 32 * k);
    for (size_t k = 0; k < R.uk.size(); k++) R.uk[k].to_bytes(challenges_out + 32 * (5 + k));
    *consumed_out = T.script_cursor();
    return e;
}

R1CSError Engine::verify(DeviceCircuit *c, Transcript &T, const uint8_t *V, const uint8_t *proof, size_t proof_len, const uint8_t seed[32], uint32_t flags) {
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    hipStream_t st = I.st;
    I.shared_now = I.shared_variants();
    VerifyReplay R;
    const R1CSError e = verify_replay(c->n, c->m, gens_cap_, T, proof, proof_len, seed, flags, R);
    if (e != R1CSError::None) return e;
    const uint64_t n = c->n, m = c->m, N = R.N;
    const uint32_t lgN = R.lgN;

    // ---- device side
    const uint32_t npts = R.npts();
    std::vector<uint8_t> hpts((size_t)npts * 32);
    verify_points(R, V, hpts.data());
    I.red_partial.ensure((size_t)4096 * sizeof(scm)); I.red_out.ensure(16 * sizeof(scm));      // [0,1024): delta partials, [1024,1536): w_c partials
    I.vfy_in.ensure((size_t)npts * 32); I.vfy_pts.ensure((size_t)npts * sizeof(ge_niels)); I.vfy_ok.ensure((size_t)npts * 4);
    I.vfy_sc.ensure((size_t)(npts + 2) * sizeof(scm)); I.vfy_ch.ensure(sizeof(IpaChallenges));
    HIPCHK(hipMemcpyAsync(I.vfy_in.p, hpts.data(), hpts.size(), hipMemcpyHostToDevice, st));
    BPG_LAUNCH(I, k_decompress, dim3(cdiv(npts, 64)), dim3(64), I.vfy_in.as<uint8_t>(), I.vfy_pts.as<ge_niels>(), I.vfy_ok.as<uint32_t>(), npts);
    {
        I.h_small.ensure(1 << 16);
        IpaChallenges *hc = reinterpret_cast<IpaChallenges *>(I.h_small.as<uint8_t>() + 8192);
        for (uint32_t k = 0; k < lgN; k++) { hc->u[k] = to_scm(R.uk[k]); hc->uinv[k] = to_scm(R.ukinv[k]); }
        HIPCHK(hipMemcpyAsync(I.vfy_ch.p, hc, sizeof(IpaChallenges), hipMemcpyHostToDevice, st));
    }
    const VerifyVecs W = verify_prep(I, c, R, I.vfy_ch.as<IpaChallenges>());
    scm *const wV = W.wV;
    I.lv.ensure(N * sizeof(scm)); I.rv.ensure(N * sizeof(scm));
    const uint32_t blocks = std::min<uint32_t>(cdiv(N, 256), 1024);
    BPG_LAUNCH(I, k_verify_scalars, dim3(blocks), dim3(256), W.wL, W.wR, W.wO, I.yinvpow.as<scm>(), W.svec, to_scm(R.x), to_scm(R.ipa), to_scm(R.ipb), to_scm(R.u_ch),
               I.lv.as<scm>(), I.rv.as<scm>(), I.red_partial.as<scm>(), (uint32_t)n, (uint32_t)N);
    BPG_LAUNCH(I, k_reduce_partials, dim3(1), dim3(256), I.red_partial.as<scm>(), blocks, 1u, I.red_out.as<scm>());
    HIPCHK(hipGetLastError());
    scm h_delta; std::vector<scm> h_wV(m + 1); std::vector<uint32_t> h_ok(npts);
    HIPCHK(hipMemcpyAsync(&h_delta, I.red_out.p, sizeof(scm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_wV.data(), wV, (m + 1) * sizeof(scm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_ok.data(), I.vfy_ok.p, npts * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t k = 0; k < npts; k++) if (!h_ok[k]) return R1CSError::VerificationError;      // optional_multiscalar_mul: a point failed to decompress
    std::vector<Scalar> hsv;
    verify_small_scalars(R, h_wV.data(), from_scm(h_delta), nullptr, hsv);
    std::vector<scm> hs(npts + 2);
    for (size_t k = 0; k < hs.size(); k++) hs[k] = to_scm(hsv[k]);
    HIPCHK(hipMemcpyAsync(I.vfy_sc.p, hs.data(), hs.size() * sizeof(scm), hipMemcpyHostToDevice, st));
    return verify_msm(I, N, npts) ? R1CSError::None : R1CSError::VerificationError;
}

// ------------------------------------------------------------------------------------------------ batch verification
// K proofs, each equation weighted by a random rho_k, summed into ONE multiscalar multiplication of 2 N_max + sum_k (npts_k) + 2 terms: the G / H scalars
// of all proofs go into two accumulators of N_max (k_verify_scalars_acc), every proof's own points keep their terms.  The sum is the identity for
// valid proofs; for an invalid one it is not, except with probability ~1/l over rho.  Host synchronisations on the accept path:
// one after the decompression, one before the small terms, one after the MSM - plus one per FLAT item, whose circuit is uploaded, used and freed.
void Engine::verify_batch(size_t count, const VerifyItem *items, const uint8_t batch_seed[32], R1CSError *status_out) {
    if (!count) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    hipStream_t st = I.st;
    I.shared_now = I.shared_variants();
    // ---- host phase: format checks and Fiat-Shamir replay of every item (the states before, for the item-by-item pass of a rejected batch)
    std::vector<VerifyReplay> R(count);
    std::vector<Transcript> before(count);                      // (copies, not exported states: a scripted transcript of the test hooks keeps its script)
    std::vector<uint8_t> live(count, 0);
    for (size_t k = 0; k < count; k++) {
        const VerifyItem &it = items[k];
        const uint64_t n = it.dc ? it.dc->n : it.flat->n, m = it.dc ? it.dc->m : it.flat->m;
        before[k] = *it.T;
        status_out[k] = verify_replay(n, m, gens_cap_, *it.T, it.proof, it.proof_len, it.seed, it.flags, R[k]);
        live[k] = status_out[k] == R1CSError::None;
    }
    // ---- the weights: a transcript of the whole batch (every proof and its replayed transcript), keyed with the caller's fresh randomness
    std::vector<Scalar> rho(count);
    {
        static const char label[] = "bpg-verify-batch-v1";
        Transcript B(reinterpret_cast<const uint8_t *>(label), sizeof label - 1);
        B.append_u64("count", count);
        for (size_t k = 0; k < count; k++) {
            uint8_t s[203]; items[k].T->export_state(s);
            B.append_message("proof", items[k].proof, items[k].proof_len);
            B.append_message("state", s, 203);
        }
        TranscriptRng rng = B.build_rng({}, batch_seed);
        for (size_t k = 0; k < count; k++) rho[k] = rng.random_scalar();
    }
    // ---- every live item's points in one decompression
    std::vector<uint32_t> pt_off(count + 1, 0);
    for (size_t k = 0; k < count; k++) pt_off[k + 1] = pt_off[k] + (live[k] ? R[k].npts() : 0);
    const uint32_t npts = pt_off[count];
    if (!npts) return;
    {
        std::vector<uint8_t> hpts((size_t)npts * 32);
        std::vector<IpaChallenges> hch(count);
        std::memset(hch.data(), 0, count * sizeof(IpaChallenges));
        for (size_t k = 0; k < count; k++) {
            if (!live[k]) continue;
            verify_points(R[k], items[k].V, &hpts[(size_t)pt_off[k] * 32]);
            for (uint32_t j = 0; j < R[k].lgN; j++) { hch[k].u[j] = to_scm(R[k].uk[j]); hch[k].uinv[j] = to_scm(R[k].ukinv[j]); }
        }
        I.vfy_in.ensure((size_t)npts * 32); I.vfy_pts.ensure((size_t)npts * sizeof(ge_niels)); I.vfy_ok.ensure((size_t)npts * 4);
        I.vfy_ch.ensure(count * sizeof(IpaChallenges));
        I.h2d(I.vfy_in.p, hpts.data(), hpts.size());
        I.h2d(I.vfy_ch.p, hch.data(), count * sizeof(IpaChallenges));
        BPG_LAUNCH(I, k_decompress, dim3(cdiv(npts, 64)), dim3(64), I.vfy_in.as<uint8_t>(), I.vfy_pts.as<ge_niels>(), I.vfy_ok.as<uint32_t>(), npts);
        HIPCHK(hipGetLastError());
        std::vector<uint32_t> h_ok(npts);
        HIPCHK(hipMemcpyAsync(h_ok.data(), I.vfy_ok.p, (size_t)npts * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = 0; k < count; k++) {
            if (!live[k]) continue;
            for (uint32_t j = pt_off[k]; j < pt_off[k + 1]; j++)
                if (!h_ok[j]) { status_out[k] = R1CSError::VerificationError; live[k] = 0; break; }     // optional_multiscalar_mul: a point failed to decompress
        }
    }
    // ---- device phase: per item the weighted G / H scalars into the accumulators, its w_V, w_c and delta into its slot [w_V.. | w_c | delta]
    uint64_t Nmax = 0; size_t nsmall = 0;
    std::vector<size_t> slot(count, 0);
    size_t b_arena = 0;
    for (size_t k = 0; k < count; k++) {
        if (!live[k]) continue;
        Nmax = std::max<uint64_t>(Nmax, R[k].N); slot[k] = nsmall; nsmall += R[k].m + 2;
        const uint64_t ncols = 3 * R[k].n + R[k].m + 1, q = items[k].dc ? items[k].dc->q : items[k].flat->q;
        b_arena = std::max(b_arena, Impl::al256(ncols * sizeof(scm)) + Impl::al256((q + 2) * sizeof(scm)) + Impl::al256(R[k].N * sizeof(scm)));
    }
    if (!Nmax) return;
    I.lv.ensure(Nmax * sizeof(scm)); I.rv.ensure(Nmax * sizeof(scm)); I.yinvpow.ensure(Nmax * sizeof(scm)); I.arena.ensure(b_arena);
    I.vfy_small.ensure(nsmall * sizeof(scm));
    HIPCHK(hipMemsetAsync(I.lv.p, 0, Nmax * sizeof(scm), st));
    HIPCHK(hipMemsetAsync(I.rv.p, 0, Nmax * sizeof(scm), st));
    for (size_t k = 0; k < count; k++) {
        if (!live[k]) continue;
        DeviceCircuit *c = items[k].dc;
        const bool own = c == nullptr;
        if (own) c = upload(*items[k].flat);                    // (synchronises the stream itself)
        try {
            const VerifyReplay &Rk = R[k];
            const VerifyVecs W = verify_prep(I, c, Rk, I.vfy_ch.as<IpaChallenges>() + k);
            const uint32_t blocks = std::min<uint32_t>(cdiv(Rk.N, 256), 1024);
            BPG_LAUNCH(I, k_verify_scalars_acc, dim3(blocks), dim3(256), W.wL, W.wR, W.wO, I.yinvpow.as<scm>(), W.svec, to_scm(Rk.x), to_scm(Rk.ipa), to_scm(Rk.ipb),
                       to_scm(Rk.u_ch), to_scm(rho[k]), I.lv.as<scm>(), I.rv.as<scm>(), I.red_partial.as<scm>(), (uint32_t)Rk.n, (uint32_t)Rk.N);
            scm *sl = I.vfy_small.as<scm>() + slot[k];
            BPG_LAUNCH(I, k_reduce_partials, dim3(1), dim3(256), I.red_partial.as<scm>(), blocks, 1u, sl + Rk.m + 1);
            HIPCHK(hipMemcpyAsync(sl, W.wV, (Rk.m + 1) * sizeof(scm), hipMemcpyDeviceToDevice, st));
            HIPCHK(hipGetLastError());
            // a flat circuit is freed only once the kernels that read it have run: one synchronisation per flat item
            if (own) { HIPCHK(hipStreamSynchronize(st)); free_circuit(c); }
        } catch (...) { if (own) { (void)hipStreamSynchronize(st); free_circuit(c); } throw; }
    }
    // ---- small terms: every live item's point scalars times rho_k; the B, B_blinding scalars summed over the items
    std::vector<scm> h_slots(nsmall);
    HIPCHK(hipMemcpyAsync(h_slots.data(), I.vfy_small.p, nsmall * sizeof(scm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<scm> hs(npts + 2);
    std::memset(hs.data(), 0, hs.size() * sizeof(scm));                // points of items that left at the decompression: scalar 0, no bucket entries
    Scalar sB, sBb;
    std::vector<Scalar> hsv;
    for (size_t k = 0; k < count; k++) {
        if (!live[k]) continue;
        const scm *sl = &h_slots[slot[k]];
        verify_small_scalars(R[k], sl, from_scm(sl[R[k].m + 1]), &rho[k], hsv);
        const uint32_t np = R[k].npts();
        for (uint32_t j = 0; j < np; j++) hs[pt_off[k] + j] = to_scm(hsv[j]);
        sB = sB + hsv[np]; sBb = sBb + hsv[np + 1];
    }
    hs[npts] = to_scm(sB); hs[npts + 1] = to_scm(sBb);
    I.vfy_sc.ensure((size_t)(npts + 2) * sizeof(scm));
    I.h2d(I.vfy_sc.p, hs.data(), hs.size() * sizeof(scm));
    if (verify_msm(I, Nmax, npts)) return;                             // one MSM for the whole batch: every live item is accepted
    // ---- a rejected batch: each live item alone, from its state before, for its exact status (costs only when the batch holds a bad proof)
    for (size_t k = 0; k < count; k++) {
        if (!live[k]) continue;
        const VerifyItem &it = items[k];
        *it.T = before[k];
        DeviceCircuit *c = it.dc;
        const bool own = c == nullptr;
        if (own) c = upload(*it.flat);
        try { status_out[k] = verify(c, *it.T, it.V, it.proof, it.proof_len, it.seed, it.flags); } catch (...) { if (own) free_circuit(c); throw; }
        if (own) free_circuit(c);
    }
}

// ------------------------------------------------------------------------------------------------ lockstep verification (hip/k_vwave.cuh, host/verify_wave_plan.hpp)
// K proofs of ONE resident circuit (include/bpg.h bpg_r1cs_verify_resident_batch): the verification equations weighted and summed into one MSM as in
// verify_batch, but every device stage is one launch per WAVE of items instead of seven stream operations per item, and the replays run on the host
// threads the proving waves use.  Per call: the replays, one k_decompress, the upload of one challenge record per item, the read-back of the K small
// slots, the small scalars on the host, one MSM.  Per wave: k_vw_exp, (k_vw_tails,) k_vw_flatten, k_vw_small, k_vw_scalars, k_vw_reduce - six launches at
// most, whatever K and N.  Three host synchronisations: after the decompression, before the small terms, after the MSM.
namespace {
struct VwCall { VerifyWavePlan P; uint64_t launches[6] = {0, 0, 0, 0, 0, 0}; };       // k_vw_exp, _tails, _flatten, _small, _scalars, _reduce
constexpr const char *kVwNames[6] = {"k_vw_exp", "k_vw_tails", "k_vw_flatten", "k_vw_small", "k_vw_scalars", "k_vw_reduce"};
uint64_t vw_tail_len(const DeviceCircuit *c) { return c->n_params + c->n_slots; }
// The device side of the call from the challenge records to the accumulators, queued on the stream and not waited for: lv, rv (N scalars each, zeroed here)
// and vfy_small (K slots [w_V | w_c | delta]).  h_ch: K records of P.ch_len scalars (hip/k_vwave.cuh).  raw / flags: K x (n_params + n_in) x 32 bytes and K
// words when some item brings constants of its own, else null.  The wave's regions live in the arena and are read by nothing after k_vw_reduce.
VwCall verify_wave_launch(Engine::Impl &I, const DeviceCircuit *c, uint64_t K, const std::vector<scm> &h_ch, const std::vector<uint8_t> *raw, const std::vector<uint32_t> *flags) {
    hipStream_t st = I.st;
    const uint64_t n = c->n, m = c->m, N = padded_size(n), n_tail = raw ? vw_tail_len(c) : 0, n_raw = c->n_params + c->n_in;
    VwCall R;
    R.P = plan_verify_wave(n, m, c->q, N, n_tail, K, I.batch_wave_mb, I.cu_count);
    const VerifyWavePlan &P = R.P;
    if (h_ch.size() != K * P.ch_len) throw std::logic_error("verify wave: challenge records do not match the plan");
    I.vfy_ch.ensure(P.bytes_ch); I.vfy_small.ensure(P.bytes_small); I.lv.ensure(N * sizeof(scm)); I.rv.ensure(N * sizeof(scm)); I.arena.ensure(P.total);
    I.h2d(I.vfy_ch.p, h_ch.data(), P.bytes_ch);
    if (n_tail) {
        I.vw_raw.ensure(std::max<size_t>(raw->size(), 32)); I.vw_flags.ensure(K * 4); I.vw_standing.ensure(n_tail * sizeof(scm));
        if (!raw->empty()) I.h2d(I.vw_raw.p, raw->data(), raw->size());
        I.h2d(I.vw_flags.p, flags->data(), K * 4);
        HIPCHK(hipMemcpyAsync(I.vw_standing.p, c->coef.as<scm>() + c->param_first, n_tail * sizeof(scm), hipMemcpyDeviceToDevice, st));
    }
    HIPCHK(hipMemsetAsync(I.lv.p, 0, N * sizeof(scm), st));
    HIPCHK(hipMemsetAsync(I.rv.p, 0, N * sizeof(scm), st));
    scm *const w = reinterpret_cast<scm *>(I.arena_at(P.off_w)), *const ypow = reinterpret_cast<scm *>(I.arena_at(P.off_y)), *const zpow = reinterpret_cast<scm *>(I.arena_at(P.off_z)),
        *const tails = n_tail ? reinterpret_cast<scm *>(I.arena_at(P.off_tail)) : nullptr, *const part = reinterpret_cast<scm *>(I.arena_at(P.off_part));
    const uint32_t nz = (uint32_t)P.z_len, lgTy = std::min<uint32_t>(ceil_log2(N), 16), lgTz = std::min<uint32_t>(ceil_log2(nz), 16), ncols = (uint32_t)P.w_len;
    const uint32_t bxN = cdiv(N, 256);
    for (uint64_t wv = 0; wv < P.waves; wv++) {
        const uint64_t k0 = wv * P.per_wave, items = P.wave_items(wv);
        const VerifyWaveChunks &C = P.wave_chunks(wv);
        const scm *ch = I.vfy_ch.as<scm>() + k0 * P.ch_len;
        BPG_LAUNCH(I, k_vw_exp, dim3(cdiv(1u << std::max(lgTy, lgTz), 256), 2, (uint32_t)items), dim3(256), ch, (uint32_t)P.ch_len, ypow, (uint32_t)N, lgTy, zpow, nz, lgTz);
        R.launches[0]++;
        if (n_tail) {
            BPG_LAUNCH(I, k_vw_tails, dim3(cdiv(items * n_tail, 256)), dim3(256), I.vw_flags.as<uint32_t>() + k0, I.vw_raw.as<uint32_t>() + 8 * k0 * n_raw, (uint32_t)n_raw,
                       c->in_slots.as<uint32_t>(), c->coef.as<scm>(), I.vw_standing.as<scm>(), (uint32_t)c->n_params, (uint32_t)n_tail, items * n_tail, tails);
            R.launches[1]++;
        }
        BPG_LAUNCH(I, k_vw_flatten, dim3(cdiv(items * ncols, 256)), dim3(256), c->col_ptr.as<uint64_t>(), c->ent_row.as<uint32_t>(), c->ent_coef.as<uint32_t>(), c->coef.as<scm>(),
                   c->n_gates ? tails : nullptr, (uint32_t)c->param_first, (uint32_t)n_tail, zpow, nz, w, ncols, (uint32_t)(3 * n), items * ncols);
        R.launches[2]++;
        BPG_LAUNCH(I, k_vw_small, dim3((uint32_t)items), dim3(256), c->ent_row.as<uint32_t>(), c->ent_coef.as<uint32_t>(), c->coef.as<scm>(), tails, (uint32_t)c->param_first,
                   (uint32_t)n_tail, c->const_begin, c->nnz, zpow, nz, ypow, w, (uint32_t)n, (uint32_t)m, (uint32_t)N, I.vfy_small.as<scm>() + k0 * P.small_len);
        R.launches[3]++;
        BPG_LAUNCH(I, k_vw_scalars, dim3(bxN, C.chunks), dim3(256), ch, (uint32_t)P.ch_len, w, ypow, (uint32_t)n, (uint32_t)m, (uint32_t)N, P.lgN, items, C.per_chunk, part);
        R.launches[4]++;
        BPG_LAUNCH(I, k_vw_reduce, dim3(bxN), dim3(256), part, C.chunks, (uint32_t)N, I.lv.as<scm>(), I.rv.as<scm>());
        R.launches[5]++;
        HIPCHK(hipGetLastError());
        {   // the profile's bookkeeping: bytes a kernel must move (scalars of 32 bytes, matrix entries of 8 + the coefficient and the power they name) and its
            // Montgomery products, per wave
            const double it = (double)items, var_ent = (double)c->const_begin, const_ent = (double)(c->nnz - c->const_begin), dN = (double)N, dn = (double)n;
            const double b_exp = 32.0 * it * (dN + nz), b_fl = it * (72.0 * var_ent + 32.0 * ncols), b_sm = it * (72.0 * const_ent + 96.0 * dn + 32.0 * (m + 2.0));
            const double b_part = 64.0 * C.chunks * dN, b_sc = it * 32.0 * (dN + 3.0 * dn + (double)P.ch_len) + b_part;
            I.prof_note(KID_k_vw_exp, b_exp, b_exp, it * (dN + nz + 2.0 * (lgTy + lgTz)));
            if (n_tail) I.prof_note(KID_k_vw_tails, 64.0 * it * n_tail, 64.0 * it * n_tail, 2.0 * it * n_tail);
            I.prof_note(KID_k_vw_flatten, b_fl, b_fl, it * var_ent);
            I.prof_note(KID_k_vw_small, b_sm, b_sm, it * (const_ent + 2.0 * dn));
            I.prof_note(KID_k_vw_scalars, b_sc, b_sc, it * dN * (2.0 * P.lgN + 8.0));
            I.prof_note(KID_k_vw_reduce, b_part + 128.0 * dN, b_part + 128.0 * dN, 0.0);
        }
    }
    return R;
}
std::string vw_evidence(const VwCall &R) {
    const VerifyWavePlan &P = R.P;
    std::string j = "{";
    auto ev = [&](const char *k, uint64_t v) { if (j.size() > 1) j += ", "; j += "\""; j += k; j += "\": "; j += std::to_string(v); };
    ev("n", P.n); ev("N", P.N); ev("count", P.count); ev("n_tail", P.n_tail); ev("item_bytes", P.item_bytes); ev("waves", P.waves); ev("items_per_wave", P.per_wave);
    ev("chunks", P.full.chunks); ev("items_per_chunk", P.full.per_chunk); ev("last_wave_items", P.wave_items(P.waves - 1)); ev("last_chunks", P.last.chunks);
    ev("last_items_per_chunk", P.last.per_chunk); ev("target_blocks", P.target_blocks); ev("wave_bytes", P.total);
    j += ", \"launches\": {";
    for (int k = 0; k < 6; k++) { if (k) j += ", "; j += "\""; j += kVwNames[k]; j += "\": "; j += std::to_string(R.launches[k]); }
    j += "}}";
    return j;
}
// who may bring what (include/bpg.h): per-item constants on a SINGLE template only, parameter values where there are parameter rows, inputs where there are inputs
void vw_check_constants(const DeviceCircuit *c, bool params, bool inputs, const std::string &who) {
    if (!params && !inputs) return;
    if (!c->is_template || c->rep_count || !c->join_parts.empty())
        throw std::invalid_argument(who + ": per-item constants are served on a single template only (a repeat or a join is verified on its standing constants)");
    if (params && !c->n_params) throw std::invalid_argument(who + ": param_values on a circuit without parameter rows");
    if (inputs && !c->n_in) throw std::invalid_argument(who + ": input_values on a circuit without public inputs");
}
}  // namespace

void Engine::check_resident_batch(const DeviceCircuit *c, size_t count, const ResidentVerifyItem *items) const {
    if (!c) throw std::invalid_argument("verify_resident_batch: null circuit");
    if (c->device != device_ || (c->owner && c->owner != this)) throw std::invalid_argument("verify_resident_batch: the circuit was uploaded on another context");
    for (size_t k = 0; k < count; k++) {
        vw_check_constants(c, items[k].params != nullptr, items[k].inputs != nullptr, "verify_resident_batch: item " + std::to_string(k));
        if (!c->n && (items[k].params || items[k].inputs)) throw std::invalid_argument("verify_resident_batch: item " + std::to_string(k) + ": constants on a circuit without multipliers");
    }
}

void Engine::verify_resident_batch(DeviceCircuit *c, size_t count, const ResidentVerifyItem *items, const uint8_t batch_seed[32], R1CSError *status_out) {
    check_resident_batch(c, count, items);
    if (!count) return;
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    hipStream_t st = I.st;
    I.shared_now = I.shared_variants();
    const uint64_t n = c->n, m = c->m, n_par = c->n_params, n_in = c->n_in, n_raw = n_par + n_in;
    bool constants = false;
    for (size_t k = 0; k < count; k++) constants |= items[k].params || items[k].inputs;
    const uint64_t n_tail = constants ? vw_tail_len(c) : 0;
    // the item-by-item pass: a circuit without multipliers as a whole, and the live items of a rejected sum.  An item's own constants are written into the table
    // for its verification; the standing tail (vw_standing, copied before the first wave) is back in place before the next item without constants and at the end
    bool dirty = false;
    auto restore = [&] { if (dirty) { HIPCHK(hipMemcpyAsync(c->coef.as<scm>() + c->param_first, I.vw_standing.p, n_tail * sizeof(scm), hipMemcpyDeviceToDevice, st)); HIPCHK(hipStreamSynchronize(st)); dirty = false; } };
    auto alone = [&](size_t k, uint64_t j) {         // j: the item's place among the records of the waves
        const ResidentVerifyItem &it = items[k];
        if (it.params || it.inputs) {
            I.vw_tail1.ensure(n_tail * sizeof(scm));
            BPG_LAUNCH(I, k_vw_tails, dim3(cdiv(n_tail, 256)), dim3(256), I.vw_flags.as<uint32_t>() + j, I.vw_raw.as<uint32_t>() + 8 * j * n_raw, (uint32_t)n_raw,
                       c->in_slots.as<uint32_t>(), c->coef.as<scm>(), I.vw_standing.as<scm>(), (uint32_t)n_par, (uint32_t)n_tail, n_tail, I.vw_tail1.as<scm>());
            HIPCHK(hipGetLastError());
            dirty = true;
            HIPCHK(hipMemcpyAsync(c->coef.as<scm>() + c->param_first, I.vw_tail1.p, n_tail * sizeof(scm), hipMemcpyDeviceToDevice, st));
        } else restore();
        status_out[k] = verify(c, *it.T, it.V, it.proof, it.proof_len, it.seed, it.flags);
    };
    if (n == 0) {       // no generator lanes to share: the existing path, item by item (no template has n = 0, so no item brings constants)
        for (size_t k = 0; k < count; k++) alone(k, 0);
        return;
    }
    // ---- host phase: format checks and Fiat-Shamir replay of every item on the host threads of the proving waves
    std::vector<VerifyReplay> R(count);
    std::vector<Transcript> before(count);
    std::vector<uint8_t> live(count, 0);
    StageThreads pool(std::min<uint32_t>(batch_host_threads(), (uint32_t)std::max<size_t>(1, count / 8)));
    pool.run(count, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++) {
            const ResidentVerifyItem &it = items[k];
            before[k] = *it.T;
            status_out[k] = verify_replay(n, m, gens_cap_, *it.T, it.proof, it.proof_len, it.seed, it.flags, R[k]);
            live[k] = status_out[k] == R1CSError::None;
        }
    });
    // ---- the weights: verify_batch's transcript (count, every proof and its replayed state, finalised with batch_seed); an item's own constants go in behind its
    // state, so a call without any draws verify_batch's weights
    std::vector<Scalar> rho(count);
    {
        static const char label[] = "bpg-verify-batch-v1";
        Transcript B(reinterpret_cast<const uint8_t *>(label), sizeof label - 1);
        B.append_u64("count", count);
        for (size_t k = 0; k < count; k++) {
            uint8_t s[203]; items[k].T->export_state(s);
            B.append_message("proof", items[k].proof, items[k].proof_len);
            B.append_message("state", s, 203);
            if (items[k].params) B.append_message("params", items[k].params, n_par * 32);
            if (items[k].inputs) B.append_message("inputs", items[k].inputs, n_in * 32);
        }
        TranscriptRng rng = B.build_rng({}, batch_seed);
        for (size_t k = 0; k < count; k++) rho[k] = rng.random_scalar();
    }
    // ---- every live item's points in one decompression (the first synchronisation): items with a bad point leave here
    const uint32_t np1 = (uint32_t)(6 + m + 5 + 2 * ceil_log2(padded_size(n)));
    std::vector<uint32_t> pt_off(count + 1, 0);
    for (size_t k = 0; k < count; k++) pt_off[k + 1] = pt_off[k] + (live[k] ? np1 : 0);
    const uint32_t npts = pt_off[count];
    if (!npts) return;
    {
        std::vector<uint8_t> hpts((size_t)npts * 32);
        pool.run(count, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; k++) if (live[k]) verify_points(R[k], items[k].V, &hpts[(size_t)pt_off[k] * 32]); });
        I.vfy_in.ensure((size_t)npts * 32); I.vfy_pts.ensure((size_t)npts * sizeof(ge_niels)); I.vfy_ok.ensure((size_t)npts * 4);
        I.h2d(I.vfy_in.p, hpts.data(), hpts.size());
        BPG_LAUNCH(I, k_decompress, dim3(cdiv(npts, 64)), dim3(64), I.vfy_in.as<uint8_t>(), I.vfy_pts.as<ge_niels>(), I.vfy_ok.as<uint32_t>(), npts);
        HIPCHK(hipGetLastError());
        std::vector<uint32_t> h_ok(npts);
        HIPCHK(hipMemcpyAsync(h_ok.data(), I.vfy_ok.p, (size_t)npts * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t k = 0; k < count; k++) {
            if (!live[k]) continue;
            for (uint32_t j = pt_off[k]; j < pt_off[k + 1]; j++)
                if (!h_ok[j]) { status_out[k] = R1CSError::VerificationError; live[k] = 0; break; }     // optional_multiscalar_mul: a point failed to decompress
        }
    }
    // ---- the waves: one challenge record per live item, in item order
    std::vector<size_t> lk;                                     // live items
    for (size_t k = 0; k < count; k++) if (live[k]) lk.push_back(k);
    const uint64_t K = lk.size();
    if (!K) return;
    const uint32_t lgN = R[lk[0]].lgN;
    const uint64_t ch_len = VW_CH_FIXED + 2 * (uint64_t)lgN;
    std::vector<scm> h_ch(K * ch_len);
    std::vector<uint8_t> raw; std::vector<uint32_t> flags;
    if (constants) { raw.assign(K * n_raw * 32, 0); flags.assign(K, 0); }
    pool.run(K, [&](size_t lo, size_t hi) {
        for (size_t j = lo; j < hi; j++) {
            const VerifyReplay &r = R[lk[j]];
            scm *h = &h_ch[j * ch_len];
            h[VW_YINV] = to_scm(r.yinv); h[VW_Z] = to_scm(r.z); h[VW_X] = to_scm(r.x); h[VW_UCH] = to_scm(r.u_ch); h[VW_A] = to_scm(r.ipa); h[VW_B] = to_scm(r.ipb);
            h[VW_RHO] = to_scm(rho[lk[j]]);
            for (uint32_t t = 0; t < lgN; t++) { h[VW_CH_FIXED + t] = to_scm(r.uk[t]); h[VW_CH_FIXED + lgN + t] = to_scm(r.ukinv[t]); }
            if (!constants) continue;
            const ResidentVerifyItem &it = items[lk[j]];
            if (it.params) { std::memcpy(&raw[j * n_raw * 32], it.params, n_par * 32); flags[j] |= VW_HAS_PARAMS; }
            if (it.inputs) { std::memcpy(&raw[(j * n_raw + n_par) * 32], it.inputs, n_in * 32); flags[j] |= VW_HAS_INPUTS; }
        }
    });
    const VwCall run = verify_wave_launch(I, c, K, h_ch, constants ? &raw : nullptr, constants ? &flags : nullptr);
    const uint64_t N = run.P.N;
    // ---- small terms (the second synchronisation): every live item's point scalars times rho_k; the B, B_blinding scalars summed over the items
    const size_t slot_len = (size_t)m + 2;
    std::vector<scm> h_slots(K * slot_len);
    HIPCHK(hipMemcpyAsync(h_slots.data(), I.vfy_small.p, h_slots.size() * sizeof(scm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<scm> hs(npts + 2);
    std::memset(hs.data(), 0, hs.size() * sizeof(scm));                // points of items that left at the decompression: scalar 0, no bucket entries
    std::vector<Scalar> sB(K), sBb(K);
    pool.run(K, [&](size_t lo, size_t hi) {
        std::vector<Scalar> hsv;
        for (size_t j = lo; j < hi; j++) {
            const size_t k = lk[j];
            const scm *sl = &h_slots[j * slot_len];
            verify_small_scalars(R[k], sl, from_scm(sl[m + 1]), &rho[k], hsv);
            for (uint32_t t = 0; t < np1; t++) hs[pt_off[k] + t] = to_scm(hsv[t]);
            sB[j] = hsv[np1]; sBb[j] = hsv[np1 + 1];
        }
    });
    Scalar tB, tBb;
    for (size_t j = 0; j < K; j++) { tB = tB + sB[j]; tBb = tBb + sBb[j]; }
    hs[npts] = to_scm(tB); hs[npts + 1] = to_scm(tBb);
    I.vfy_sc.ensure((size_t)(npts + 2) * sizeof(scm));
    I.h2d(I.vfy_sc.p, hs.data(), hs.size() * sizeof(scm));
    if (verify_msm(I, N, npts)) return;                                // one MSM for the whole call (the third synchronisation): every live item is accepted
    // ---- a rejected sum: each live item alone, from its state before, for its exact status
    try {
        for (size_t j = 0; j < K; j++) { *items[lk[j]].T = before[lk[j]]; alone(lk[j], j); }
    } catch (...) { try { restore(); } catch (...) {} throw; }
    restore();
}

// bpg_test_verify_wave_scalars: verify_wave_launch on challenge records the caller chose
std::string Engine::test_verify_wave_scalars(DeviceCircuit *c, uint64_t count, const uint8_t *challenges, const uint8_t *param_values, const uint8_t *input_values,
                                             uint8_t *g_out, uint8_t *h_out, uint8_t *small_out) {
    if (!c || !challenges || !g_out || !h_out || !small_out) throw std::invalid_argument("test_verify_wave_scalars: null pointer");
    if (c->device != device_ || (c->owner && c->owner != this)) throw std::invalid_argument("test_verify_wave_scalars: the circuit was uploaded on another context");
    if (!count || count > (1u << 20)) throw std::invalid_argument("test_verify_wave_scalars: 1 .. 2^20 items");
    if (!c->n) throw std::invalid_argument("test_verify_wave_scalars: a circuit without multipliers has no wave (it is verified item by item)");
    vw_check_constants(c, param_values != nullptr, input_values != nullptr, "test_verify_wave_scalars");
    const uint64_t N = padded_size(c->n), n_par = c->n_params, n_in = c->n_in, n_raw = n_par + n_in;
    const uint32_t lgN = ceil_log2(N);
    const uint64_t ch_len = VW_CH_FIXED + 2 * (uint64_t)lgN;
    std::vector<scm> h_ch(count * ch_len);
    for (uint64_t k = 0; k < count; k++) for (uint64_t t = 0; t < ch_len; t++) {
        Scalar s; std::memcpy(s.w, challenges + 32 * (k * ch_len + t), 32);
        const std::string at = "test_verify_wave_scalars: item " + std::to_string(k) + ", entry " + std::to_string(t);
        if (!s.is_canonical()) throw std::invalid_argument(at + " is not canonical");
        if ((t == VW_YINV || t >= VW_CH_FIXED) && s.is_zero_mod_l()) throw std::invalid_argument(at + " is zero (y^-1 and every u_k have inverses)");
        h_ch[k * ch_len + t] = to_scm(s);
    }
    for (uint64_t k = 0; k < count; k++) for (uint32_t t = 0; t < lgN; t++) {
        const Scalar one = from_scm(h_ch[k * ch_len + VW_CH_FIXED + t]) * from_scm(h_ch[k * ch_len + VW_CH_FIXED + lgN + t]);
        if (!(one == Scalar::one())) throw std::invalid_argument("test_verify_wave_scalars: item " + std::to_string(k) + ": entry u^-1_" + std::to_string(t) + " is not the inverse of u_" + std::to_string(t));
    }
    const bool constants = param_values || input_values;
    std::vector<uint8_t> raw; std::vector<uint32_t> flags;
    if (constants) {
        raw.assign(count * n_raw * 32, 0); flags.assign(count, (param_values ? VW_HAS_PARAMS : 0u) | (input_values ? VW_HAS_INPUTS : 0u));
        for (uint64_t k = 0; k < count; k++) {
            if (param_values) std::memcpy(&raw[k * n_raw * 32], param_values + k * n_par * 32, n_par * 32);
            if (input_values) std::memcpy(&raw[(k * n_raw + n_par) * 32], input_values + k * n_in * 32, n_in * 32);
        }
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const VwCall run = verify_wave_launch(I, c, count, h_ch, constants ? &raw : nullptr, constants ? &flags : nullptr);
    const size_t slot_len = (size_t)c->m + 2;
    std::vector<scm> g(N), h(N), sl(count * slot_len);
    HIPCHK(hipMemcpyAsync(g.data(), I.lv.p, N * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(h.data(), I.rv.p, N * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipMemcpyAsync(sl.data(), I.vfy_small.p, sl.size() * sizeof(scm), hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
    for (uint64_t i = 0; i < N; i++) { from_scm(g[i]).to_bytes(g_out + 32 * i); from_scm(h[i]).to_bytes(h_out + 32 * i); }
    for (size_t i = 0; i < sl.size(); i++) from_scm(sl[i]).to_bytes(small_out + 32 * i);
    return vw_evidence(run);
}

// ------------------------------------------------------------------------------------------------ MiMC sponges and Merkle trees (hip/k_mimc.cuh)
const std::vector<Scalar> &mimc_round_constants();      // host/gadgets.hpp (defined in capi.hip)

struct DeviceMerkle {
    Engine *owner = nullptr; uint32_t depth = 0;
    DevBuf tree;            // 2^(depth+1) scm in heap order, Montgomery form; entry 0 is unused
    // leaves [0, size) are the caller's, leaves [size, 2^depth) hold `empty` (bpg_merkle_build: size = 2^depth, empty = 0)
    uint64_t size = 0;
    scm empty = sc_zero();
    std::vector<scm> empty_nodes;       // E_0 .. E_depth, host copy; a tree of bpg_merkle_build computes it when bpg_merkle_empty_nodes first asks
    // the prefix layout (bpg_merkle_build_prefix; host/merkle_prefix_plan.hpp): `tree` holds merkle_prefix_slots(dims) scm, height 0 (the leaves) first, and
    // `etab` E_0 .. E_depth on the device, what a node that is not stored reads as.  Both go with the tree, on merkle_orphan too.
    bool prefix = false;
    MerklePrefixDims dims{};
    DevBuf etab;
    // the keyed layout (bpg_merkle_build_keyed; host/merkle_keyed_plan.hpp): height s (0 = the leaves) holds kcnt[s] sorted positions in kpos[s] beside their
    // values in kval[s], with room for kcap[s]; `etab` as above; `size` = kcnt[0], the keys held.  `tree` is not used.
    bool keyed = false;
    DevBuf kpos[MERKLE_KEYED_MAX_DEPTH + 1], kval[MERKLE_KEYED_MAX_DEPTH + 1];
    uint32_t kcnt[MERKLE_KEYED_MAX_DEPTH + 1] = {0}, kcap[MERKLE_KEYED_MAX_DEPTH + 1] = {0};
    void release() { tree.release(); etab.release(); for (DevBuf &b : kpos) b.release(); for (DevBuf &b : kval) b.release(); }
};

namespace {
void merkle_orphan(DeviceMerkle *t) { t->release(); t->owner = nullptr; }
// a keyed tree as its kernels take it, and the device bytes it holds: 36 bytes per entry of room at every height, and the table of constants
MkxView mkx_view(const DeviceMerkle *t) {
    MkxView V{};
    V.depth = t->depth;
    for (uint32_t s = 0; s <= t->depth; s++) { V.pos[s] = t->kpos[s].as<uint32_t>(); V.val[s] = t->kval[s].as<scm>(); V.cnt[s] = t->kcnt[s]; }
    return V;
}
uint64_t mkx_bytes(const DeviceMerkle *t) {
    uint64_t b = 32ull * (t->depth + 1);
    for (uint32_t s = 0; s <= t->depth; s++) b += (uint64_t)t->kcap[s] * (sizeof(uint32_t) + sizeof(scm));
    return b;
}
constexpr uint32_t kMerkleMaxDepth = 24;
static_assert(MERKLE_MAX_DEPTH == kMerkleMaxDepth && MERKLE_CLIMB_PARENTS == BPG_MERKLE_TOP_PARENTS, "host/merkle_plan.hpp plans for the kernels of hip/k_mimc.cuh");
// E_0 = empty, E_{k+1} = node(E_k, E_k) with the BPG_HD arithmetic of hip/k_mimc.cuh on the host: ~53 us a node, where the device pays a latency floor each
std::vector<scm> merkle_empty_chain(uint32_t depth, const scm &empty) {
    static const std::vector<scm> rc = [] {
        const std::vector<Scalar> &plain = mimc_round_constants();
        std::vector<scm> h(plain.size());
        for (size_t i = 0; i < plain.size(); i++) h[i] = to_scm(plain[i]);
        return h;
    }();
    std::vector<scm> E(depth + 1);
    E[0] = empty;
    for (uint32_t k = 0; k < depth; k++) E[k + 1] = mimc_node(E[k], E[k], rc.data());
    return E;
}
constexpr uint64_t kSpongeMaxBlocks = 1ull << 22;                  // blocks of one item: 128 MB of input, what one piece of a call stages
constexpr double kNodeProducts = 4.0 * BPG_MIMC_ROUNDS;             // Montgomery products of one two-block node
// the round constants of the context's device, converted and uploaded by the first context that asks
const scm *mimc_rc(Engine::Impl &I, int device) {
    if (I.mimc) return I.mimc->rc.as<scm>();
    std::lock_guard<std::mutex> lk(g_mimc_mutex);
    std::shared_ptr<MimcConstants> sp = g_mimc[device].lock();
    if (!sp) {
        const std::vector<Scalar> &rc = mimc_round_constants();
        std::vector<scm> h(rc.size());
        for (size_t i = 0; i < rc.size(); i++) h[i] = to_scm(rc[i]);
        sp = std::make_shared<MimcConstants>();
        sp->device = device; sp->rc.ensure(h.size() * sizeof(scm));
        HIPCHK(hipMemcpyAsync(sp->rc.p, h.data(), h.size() * sizeof(scm), hipMemcpyHostToDevice, I.st));
        HIPCHK(hipStreamSynchronize(I.st));
        g_mimc[device] = sp;
    }
    I.mimc = sp;
    return sp->rc.as<scm>();
}
// `nodes` evaluations of the node function: 64 bytes read and 32 written each, 1,944 products (what the launch log of an update is checked against)
void note_nodes(Engine::Impl &I, int id, uint64_t nodes) { I.prof_note(id, 96.0 * (double)nodes, 96.0 * (double)nodes, kNodeProducts * (double)nodes); }
}  // namespace

void Engine::mimc_sponge_many(uint64_t count, uint64_t blocks, const uint8_t *in, uint8_t *out) {
    if (!in || !out || count == 0 || blocks == 0) throw std::invalid_argument("mimc_sponge_many: a null pointer, or no items, or no blocks per item");
    if (blocks > kSpongeMaxBlocks || count > (1ull << 40)) throw std::invalid_argument("mimc_sponge_many: more than 2^22 blocks per item, or more than 2^40 items");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *rc = mimc_rc(I, device_);
    // pieces of at most 2^22 input scalars (128 MB); an item has at most that many blocks, so a piece holds at least one
    const uint64_t per = kSpongeMaxBlocks / blocks;
    for (uint64_t first = 0; first < count; first += per) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(per, count - first);
        const size_t in_bytes = (size_t)n * blocks * 32;
        I.mk_in.ensure(in_bytes); I.mk_out.ensure((size_t)n * 32);
        HIPCHK(hipMemcpyAsync(I.mk_in.p, in + (size_t)first * blocks * 32, in_bytes, hipMemcpyHostToDevice, I.st));
        BPG_LAUNCH(I, k_mimc_sponge, dim3(cdiv(n, 256)), dim3(256), I.mk_in.as<uint32_t>(), I.mk_out.as<uint32_t>(), n, (uint32_t)blocks, rc);
        HIPCHK(hipGetLastError());
        I.prof_note(KID_k_mimc_sponge, (double)in_bytes + 32.0 * n, (double)in_bytes + 32.0 * n, 2.0 * BPG_MIMC_ROUNDS * (double)n * (double)blocks);
        HIPCHK(hipMemcpyAsync(out + (size_t)first * 32, I.mk_out.p, (size_t)n * 32, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipStreamSynchronize(I.st));         // the staging buffers may grow (and move) for the next piece
    }
}

DeviceMerkle *Engine::merkle_build(uint32_t depth, const uint8_t *leaves) {
    if (depth < 1 || depth > kMerkleMaxDepth) throw std::invalid_argument("merkle_build: depth must be 1..24");
    if (!leaves) throw std::invalid_argument("merkle_build: null leaves");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *rc = mimc_rc(I, device_);
    const uint32_t nleaves = 1u << depth;
    const size_t bytes = (size_t)2 * nleaves * sizeof(scm);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + (64u << 20) > free_b)             // the tree and some room to work in: a failed 1 GB hipMalloc is a worse way to find out
        throw DeviceError("merkle_build: a tree of depth " + std::to_string(depth) + " takes " + std::to_string(bytes >> 20) + " MB and the device has " + std::to_string(free_b >> 20) + " MB free");
    std::unique_ptr<DeviceMerkle> t(new DeviceMerkle());
    t->owner = this; t->depth = depth; t->size = nleaves;
    try {
        t->tree.ensure(bytes);
        scm *tree = t->tree.as<scm>();
        HIPCHK(hipMemsetAsync(tree, 0, 2 * sizeof(scm), I.st));         // entry 0 is no node; the root is written last
        HIPCHK(hipMemcpyAsync(tree + nleaves, leaves, (size_t)nleaves * 32, hipMemcpyHostToDevice, I.st));
        BPG_LAUNCH(I, k_merkle_leaves, dim3(cdiv(nleaves, 256)), dim3(256), tree + nleaves, nleaves);
        // one launch per level while a level has more parents than one block holds, then the rest of the way to the root in one launch
        int level = (int)depth - 1;
        for (; (1u << level) > BPG_MERKLE_TOP_PARENTS; level--) {
            BPG_LAUNCH(I, k_merkle_level, dim3(cdiv(1u << level, 256)), dim3(256), tree, (uint32_t)level, rc);
            note_nodes(I, KID_k_merkle_level, 1ull << level);
        }
        BPG_LAUNCH(I, k_merkle_top, dim3(1), dim3(256), tree, (uint32_t)level, rc);
        note_nodes(I, KID_k_merkle_top, (2ull << level) - 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
    } catch (...) { (void)hipStreamSynchronize(I.st); throw; }         // (the tree goes with `t`, after this wait)
    I.trees.push_back(t.get());
    return t.release();
}

namespace {
// New leaves into place as merkle_build puts them there (a copy, then k_merkle_leaves on that interval), then the launches of the plan: the wide steps
// bottom-up and the climb.  Nothing else hashes a growing tree.
void merkle_grow(Engine::Impl &I, scm *tree, const MerkleGrowPlan &P, const uint8_t *leaves, const scm *rc) {
    const uint64_t count = P.new_size - P.old_size;
    if (!count) return;
    scm *at = tree + (1ull << P.depth) + P.old_size;
    HIPCHK(hipMemcpyAsync(at, leaves, (size_t)count * 32, hipMemcpyHostToDevice, I.st));
    BPG_LAUNCH(I, k_merkle_leaves, dim3(cdiv(count, 256)), dim3(256), at, (uint32_t)count);
    for (uint32_t k = 0; k < P.n_wide; k++) {
        const MerkleWideStep &w = P.wide[k];
        BPG_LAUNCH(I, k_merkle_level_range, dim3(cdiv(w.count, 256)), dim3(256), tree, w.first, w.count, rc);
        note_nodes(I, KID_k_merkle_level_range, w.count);
    }
    if (!P.climb || P.climb_lo < 2 || P.climb_hi < P.climb_lo || (P.climb_hi >> 1) - (P.climb_lo >> 1) >= BPG_MERKLE_TOP_PARENTS)
        throw std::logic_error("merkle plan: new leaves without a climb that fits one block");
    BPG_LAUNCH(I, k_merkle_climb, dim3(1), dim3(256), tree, P.climb_lo, P.climb_hi, rc);
    note_nodes(I, KID_k_merkle_climb, P.climb_evals);
    HIPCHK(hipGetLastError());
}
}  // namespace

DeviceMerkle *Engine::merkle_build_partial(uint32_t depth, uint64_t size, const uint8_t *leaves, const uint8_t *empty) {
    if (depth < 1 || depth > kMerkleMaxDepth) throw std::invalid_argument("merkle_build_partial: depth must be 1..24");
    if (size > (1ull << depth)) throw std::invalid_argument("merkle_build_partial: more leaves than 2^depth");
    if (size && !leaves) throw std::invalid_argument("merkle_build_partial: null leaves");
    const MerkleGrowPlan P = plan_merkle_grow(depth, 0, size);
    std::unique_ptr<DeviceMerkle> t(new DeviceMerkle());
    t->owner = this; t->depth = depth; t->size = size;
    if (empty) { uint32_t w[8]; std::memcpy(w, empty, 32); t->empty = sc_from_words(w); }
    t->empty_nodes = merkle_empty_chain(depth, t->empty);
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *rc = mimc_rc(I, device_);
    const size_t bytes = ((size_t)2 << depth) * sizeof(scm);
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + (64u << 20) > free_b)
        throw DeviceError("merkle_build_partial: a tree of depth " + std::to_string(depth) + " takes " + std::to_string(bytes >> 20) + " MB and the device has " + std::to_string(free_b >> 20) + " MB free");
    try {
        t->tree.ensure(bytes);
        scm *tree = t->tree.as<scm>();
        I.mk_in.ensure(t->empty_nodes.size() * sizeof(scm));
        HIPCHK(hipMemsetAsync(tree, 0, sizeof(scm), I.st));             // entry 0 is no node
        HIPCHK(hipMemcpyAsync(I.mk_in.p, t->empty_nodes.data(), t->empty_nodes.size() * sizeof(scm), hipMemcpyHostToDevice, I.st));
        // every empty subtree first, the root included when there is no leaf: the rightmost occupied node of a level may read an empty right child
        BPG_LAUNCH(I, k_merkle_fill_empty, dim3(cdiv(2ull << depth, 256)), dim3(256), tree, depth, (uint32_t)size, I.mk_in.as<scm>());
        I.prof_note(KID_k_merkle_fill_empty, (double)bytes, (double)bytes, 0.0);
        merkle_grow(I, tree, P, leaves, rc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
    } catch (...) { (void)hipStreamSynchronize(I.st); throw; }
    I.trees.push_back(t.get());
    return t.release();
}

void Engine::merkle_append(DeviceMerkle *t, uint64_t count, const uint8_t *leaves, uint64_t *first_index_out, uint8_t *root_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_append: not a tree of this context");
    if (t->keyed) throw std::invalid_argument("merkle_append: a keyed tree has no last leaf to append behind (bpg_merkle_put inserts keys)");
    if (t->prefix) return merkle_append_prefix(t, count, leaves, first_index_out, root_out);
    if (count > (1ull << t->depth) - t->size) throw std::invalid_argument("merkle_append: the tree holds " + std::to_string(t->size) + " of 2^" + std::to_string(t->depth) + " leaves: no room for " + std::to_string(count) + " more");
    if (count && !leaves) throw std::invalid_argument("merkle_append: null leaves");
    const uint64_t first = t->size;
    if (count) {
        const MerkleGrowPlan P = plan_merkle_grow(t->depth, first, first + count);
        HIPCHK(hipSetDevice(device_));
        Impl &I = *impl_;
        const scm *rc = mimc_rc(I, device_);
        try {
            merkle_grow(I, t->tree.as<scm>(), P, leaves, rc);
            HIPCHK(hipStreamSynchronize(I.st));
        } catch (...) { (void)hipStreamSynchronize(I.st); throw; }
        t->size = first + count;
    }
    if (first_index_out) *first_index_out = first;          // before the read-back: should that fail on the device, the leaves are in and the caller knows where
    if (root_out) merkle_nodes(t, 0, 0, 1, root_out);
}

void Engine::merkle_size(DeviceMerkle *t, uint64_t *size_out, uint32_t *depth_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_size: not a tree of this context");
    if (size_out) *size_out = t->size;
    if (depth_out) *depth_out = t->depth;
}

void Engine::merkle_empty_nodes(DeviceMerkle *t, uint8_t *out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_empty_nodes: not a tree of this context");
    if (!out) throw std::invalid_argument("merkle_empty_nodes: null output");
    if (t->empty_nodes.empty()) t->empty_nodes = merkle_empty_chain(t->depth, t->empty);
    for (size_t k = 0; k < t->empty_nodes.size(); k++) { uint32_t w[8]; sc_to_words(w, t->empty_nodes[k]); std::memcpy(out + 32 * k, w, 32); }
}

// The tree's memory is released on the context that built it, whichever caller frees it; a tree whose context is gone already (the destructor released its
// memory and cleared `owner`) is only deleted.
void Engine::merkle_free(DeviceMerkle *t) {
    if (!t) return;
    if (Engine *e = t->owner) {
        (void)hipSetDevice(e->device_);
        (void)hipStreamSynchronize(e->impl_->st);
        t->release();
        std::vector<DeviceMerkle *> &live = e->impl_->trees;
        live.erase(std::remove(live.begin(), live.end(), t), live.end());
    }
    delete t;
}

void Engine::merkle_nodes(DeviceMerkle *t, uint32_t level, uint64_t first, uint64_t count, uint8_t *out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_nodes: not a tree of this context");
    if (level > t->depth || first > (1ull << level) || count > (1ull << level) - first) throw std::invalid_argument("merkle_nodes: level above the depth, or nodes beyond the level");
    if (!count) return;
    if (!out) throw std::invalid_argument("merkle_nodes: null output");
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *src = (t->prefix || t->keyed) ? nullptr : t->tree.as<scm>() + (1ull << level) + first;
    const uint64_t per = 1ull << 20;
    I.mk_out.ensure((size_t)std::min(count, per) * 32);
    for (uint64_t at = 0; at < count; at += per) {          // stream order keeps a piece's kernel behind the copy of the piece before
        const uint32_t n = (uint32_t)std::min(per, count - at);
        if (t->keyed) {                                     // every node by lookup among the stored positions of height depth - level
            const uint32_t s = t->depth - level;
            BPG_LAUNCH(I, k_mkx_export, dim3(cdiv(n, 256)), dim3(256), t->kpos[s].as<uint32_t>(), t->kval[s].as<scm>(), t->kcnt[s], t->etab.as<scm>() + s, first + at, n, I.mk_out.as<uint32_t>());
        } else if (t->prefix)                                   // level 0 is the root: height depth - level; positions beyond the stored width read the table
            BPG_LAUNCH(I, k_mpx_export, dim3(cdiv(n, 256)), dim3(256), t->tree.as<scm>(), t->dims, t->etab.as<scm>(), t->depth - level, first + at, n, I.mk_out.as<uint32_t>());
        else
            BPG_LAUNCH(I, k_merkle_export, dim3(cdiv(n, 256)), dim3(256), src + at, n, I.mk_out.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + (size_t)at * 32, I.mk_out.p, (size_t)n * 32, hipMemcpyDeviceToHost, I.st));
    }
    HIPCHK(hipStreamSynchronize(I.st));
}

void Engine::merkle_paths(DeviceMerkle *t, uint64_t count, const uint64_t *indices, uint8_t *out, bool ancestors) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_paths: not a tree of this context");
    if (!count) return;
    if (!indices || !out) throw std::invalid_argument("merkle_paths: null pointer");
    const uint32_t d = t->depth;
    std::vector<uint32_t> idx(count);
    for (uint64_t i = 0; i < count; i++) {
        if (indices[i] >> d) throw std::invalid_argument("merkle_paths: leaf index " + std::to_string(indices[i]) + " is beyond 2^depth");
        idx[i] = (uint32_t)indices[i];
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint64_t per = 1ull << 16;                        // items per launch: at most 2^16 * 24 threads and 50 MB of siblings
    const size_t row = (size_t)d * 32;
    I.mk_in.ensure((size_t)std::min(count, per) * 4); I.mk_out.ensure((size_t)std::min(count, per) * row);
    for (uint64_t at = 0; at < count; at += per) {
        const uint32_t n = (uint32_t)std::min(per, count - at);
        HIPCHK(hipMemcpyAsync(I.mk_in.p, idx.data() + at, (size_t)n * 4, hipMemcpyHostToDevice, I.st));
        if (t->keyed)
            BPG_LAUNCH(I, k_mkx_paths, dim3(cdiv((uint64_t)n * d, 256)), dim3(256), mkx_view(t), t->etab.as<scm>(), I.mk_in.as<uint32_t>(), n, ancestors ? 1u : 0u, I.mk_out.as<uint32_t>());
        else if (t->prefix)
            BPG_LAUNCH(I, k_mpx_paths,dim3(cdiv((uint64_t)n * d, 256)), dim3(256), t->tree.as<scm>(), t->dims, t->etab.as<scm>(), I.mk_in.as<uint32_t>(), n, ancestors ? 1u : 0u, I.mk_out.as<uint32_t>());
        else
            BPG_LAUNCH(I, k_merkle_paths, dim3(cdiv((uint64_t)n * d, 256)), dim3(256), t->tree.as<scm>(), d, I.mk_in.as<uint32_t>(), n, ancestors ? 1u : 0u, I.mk_out.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + (size_t)at * row, I.mk_out.p, (size_t)n * row, hipMemcpyDeviceToHost, I.st));
    }
    HIPCHK(hipStreamSynchronize(I.st));                     // (idx outlives every copy that reads it)
}

void Engine::merkle_update(DeviceMerkle *t, uint64_t count, const uint64_t *indices, const uint8_t *leaves) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_update: not a tree of this context");
    if (!count) return;
    if (!indices || !leaves) throw std::invalid_argument("merkle_update: null pointer");
    if (t->keyed) return merkle_put(t, count, indices, leaves, nullptr, nullptr, true);       // a put restricted to held keys
    const uint32_t d = t->depth;
    if (count > (1ull << d)) throw std::invalid_argument("merkle_update: more leaves than the tree has (an index is given twice)");
    // every check first: a refused call leaves the tree as it was
    std::vector<uint32_t> cur(count);
    for (uint64_t i = 0; i < count; i++) {
        if (indices[i] >= t->size) throw std::invalid_argument("merkle_update: leaf index " + std::to_string(indices[i]) + " is beyond the " + std::to_string(t->size) + " leaves the tree holds");     // (a full tree: 2^depth)
        cur[i] = (uint32_t)indices[i];
    }
    // one staging buffer: [new leaves, 32 bytes each | their indices | the parents to recompute, level d-1 first: heap indices, sorted, each once]
    const size_t idx_off = (size_t)count * 32, lists_off = idx_off + (size_t)count * 4;
    std::vector<uint8_t> stage(lists_off);
    std::memcpy(stage.data(), leaves, idx_off);
    std::memcpy(stage.data() + idx_off, cur.data(), (size_t)count * 4);
    std::sort(cur.begin(), cur.end());
    if (std::adjacent_find(cur.begin(), cur.end()) != cur.end()) throw std::invalid_argument("merkle_update: a leaf index is given twice");
    if (!t->prefix) for (uint32_t &h : cur) h += 1u << d;    // (the prefix layout keeps positions: halving a leaf's index lv + 1 times is its ancestor of height lv + 1)
    std::vector<uint32_t> level_count(d);
    for (uint32_t lv = 0; lv < d; lv++) {                   // lv levels above the leaves' parents
        for (uint32_t &h : cur) h >>= 1;
        cur.erase(std::unique(cur.begin(), cur.end()), cur.end());      // two children of one parent recompute it once (halving keeps the order)
        level_count[lv] = (uint32_t)cur.size();
        const size_t at = stage.size();
        stage.resize(at + cur.size() * 4);
        std::memcpy(stage.data() + at, cur.data(), cur.size() * 4);
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *rc = mimc_rc(I, device_);
    I.mk_in.ensure(stage.size());
    scm *tree = t->tree.as<scm>();
    HIPCHK(hipMemcpyAsync(I.mk_in.p, stage.data(), stage.size(), hipMemcpyHostToDevice, I.st));
    const uint32_t *list = reinterpret_cast<const uint32_t *>(I.mk_in.as<uint8_t>() + lists_off);
    if (t->prefix) {                                        // the same lists as positions: list lv holds the parents of height lv + 1, all occupied, so stored
        const scm *E = t->etab.as<scm>();
        BPG_LAUNCH(I, k_mpx_set_leaves, dim3(cdiv(count, 256)), dim3(256), tree, t->dims, reinterpret_cast<const uint32_t *>(I.mk_in.as<uint8_t>() + idx_off),
                   I.mk_in.as<uint32_t>(), (uint32_t)count);
        for (uint32_t lv = 0; lv < d; lv++) {
            BPG_LAUNCH(I, k_mpx_list, dim3(cdiv(level_count[lv], 256)), dim3(256), tree, t->dims, lv, list, level_count[lv], rc, E);
            note_nodes(I, KID_k_mpx_list, level_count[lv]);
            list += level_count[lv];
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
        return;
    }
    BPG_LAUNCH(I, k_merkle_set_leaves, dim3(cdiv(count, 256)), dim3(256), tree, d, reinterpret_cast<const uint32_t *>(I.mk_in.as<uint8_t>() + idx_off),
               I.mk_in.as<uint32_t>(), (uint32_t)count);
    for (uint32_t lv = 0; lv < d; lv++) {
        BPG_LAUNCH(I, k_merkle_level_list, dim3(cdiv(level_count[lv], 256)), dim3(256), tree, list, level_count[lv], rc);
        note_nodes(I, KID_k_merkle_level_list, level_count[lv]);
        list += level_count[lv];
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(I.st));
}

// ------------------------------------------------------------------------------------------------ Merkle trees in the prefix layout (hip/k_merkle_prefix.cuh)
namespace {
static_assert(MERKLE_PREFIX_CLIMB_PARENTS == BPG_MERKLE_TOP_PARENTS, "host/merkle_prefix_plan.hpp plans for the one block of k_mpx_climb");
// the memory check of the other builders, on the bytes that are about to be allocated
void mpx_memory_check(const char *what, uint32_t depth, uint64_t reserve, uint64_t bytes) {
    size_t free_b = 0, total_b = 0;
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
    if (bytes + (64u << 20) > free_b)
        throw DeviceError(std::string(what) + ": a tree of depth " + std::to_string(depth) + " with room for " + std::to_string(reserve) + " leaves takes " + std::to_string(bytes >> 20) +
                          " MB and the device has " + std::to_string(free_b >> 20) + " MB free");
}
// New leaves into place (a copy, then k_merkle_leaves on that interval of height 0), then the launches of the plan: the wide steps bottom-up and the climb.
// Nothing else hashes a growing prefix tree.  What a launch would touch is checked against the dimensions first.
void mpx_grow(Engine::Impl &I, DeviceMerkle *t, const MerklePrefixGrowPlan &P, const uint8_t *leaves, const scm *rc) {
    const uint64_t count = P.new_size - P.old_size;
    if (!count) return;
    const MerklePrefixDims &d = t->dims;
    if (P.depth != d.depth || P.reserve != d.reserve || P.new_size > d.reserve) throw std::logic_error("merkle prefix plan: not a plan for this tree");
    scm *buf = t->tree.as<scm>();
    const scm *E = t->etab.as<scm>();
    scm *at = buf + d.off[0] + P.old_size;
    HIPCHK(hipMemcpyAsync(at, leaves, (size_t)count * 32, hipMemcpyHostToDevice, I.st));
    BPG_LAUNCH(I, k_merkle_leaves, dim3(cdiv(count, 256)), dim3(256), at, (uint32_t)count);
    for (uint32_t k = 0; k < P.n_wide; k++) {
        const MerklePrefixWideStep &w = P.wide[k];
        if (w.height >= d.depth || !w.count || (uint64_t)w.first + w.count > d.width[w.height + 1]) throw std::logic_error("merkle prefix plan: a wide step beyond the stored width");
        BPG_LAUNCH(I, k_mpx_range, dim3(cdiv(w.count, 256)), dim3(256), buf, d, w.height, w.first, w.count, rc, E);
        note_nodes(I, KID_k_mpx_range, w.count);
    }
    if (!P.climb || P.climb_height >= d.depth || P.climb_hi < P.climb_lo || P.climb_hi >= d.width[P.climb_height] || (P.climb_hi >> 1) - (P.climb_lo >> 1) >= BPG_MERKLE_TOP_PARENTS)
        throw std::logic_error("merkle prefix plan: new leaves without a climb that fits one block");
    BPG_LAUNCH(I, k_mpx_climb, dim3(1), dim3(256), buf, d, P.climb_height, P.climb_lo, P.climb_hi, rc, E);
    note_nodes(I, KID_k_mpx_climb, P.climb_evals);
    HIPCHK(hipGetLastError());
}
// The tree into a buffer with room for `reserve` > the present reserve leaves: the new buffer first, one launch of k_mpx_relayout, then the old buffer goes.
// Should anything fail the tree keeps its buffer and its reserve.
void mpx_relayout(Engine::Impl &I, DeviceMerkle *t, uint64_t reserve) {
    const MerklePrefixDims to = merkle_prefix_dims(t->depth, reserve);
    const uint32_t slots = merkle_prefix_slots(to);
    mpx_memory_check("merkle_reserve", t->depth, reserve, 32ull * slots);
    DevBuf grown;
    try {
        grown.ensure((size_t)slots * sizeof(scm));
        BPG_LAUNCH(I, k_mpx_relayout, dim3(cdiv(slots, 256)), dim3(256), grown.as<scm>(), to, t->tree.as<scm>(), t->dims, t->etab.as<scm>());
        I.prof_note(KID_k_mpx_relayout, 64.0 * slots, 64.0 * slots, 0.0);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
    } catch (...) { (void)hipStreamSynchronize(I.st); throw; }         // (`grown` goes after this wait)
    t->tree = std::move(grown);                                         // releases the old buffer
    t->dims = to;
}
}  // namespace

DeviceMerkle *Engine::merkle_build_prefix(uint32_t depth, uint64_t reserve, uint64_t size, const uint8_t *leaves, const uint8_t *empty) {
    if (depth < 1 || depth > MERKLE_PREFIX_MAX_DEPTH) throw std::invalid_argument("merkle_build_prefix: depth must be 1..32");
    if (reserve < 1 || reserve > merkle_prefix_limit(depth)) throw std::invalid_argument("merkle_build_prefix: reserve must be 1..min(2^depth, 2^24)");
    if (size > reserve) throw std::invalid_argument("merkle_build_prefix: more leaves than the reserve");
    if (size && !leaves) throw std::invalid_argument("merkle_build_prefix: null leaves");
    const MerklePrefixGrowPlan P = plan_merkle_prefix_grow(depth, reserve, 0, size);
    std::unique_ptr<DeviceMerkle> t(new DeviceMerkle());
    t->owner = this; t->depth = depth; t->size = size; t->prefix = true;
    t->dims = merkle_prefix_dims(depth, reserve);
    if (empty) { uint32_t w[8]; std::memcpy(w, empty, 32); t->empty = sc_from_words(w); }
    t->empty_nodes = merkle_empty_chain(depth, t->empty);
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const scm *rc = mimc_rc(I, device_);
    mpx_memory_check("merkle_build_prefix", depth, reserve, merkle_prefix_bytes(t->dims));
    try {
        const uint32_t slots = merkle_prefix_slots(t->dims);
        t->tree.ensure((size_t)slots * sizeof(scm));
        t->etab.ensure(t->empty_nodes.size() * sizeof(scm));
        HIPCHK(hipMemcpyAsync(t->etab.p, t->empty_nodes.data(), t->empty_nodes.size() * sizeof(scm), hipMemcpyHostToDevice, I.st));
        // every stored slot without a leaf below it first, the root included when there is no leaf: the invariant of the layout
        BPG_LAUNCH(I, k_mpx_fill, dim3(cdiv(slots, 256)), dim3(256), t->tree.as<scm>(), t->dims, (uint32_t)size, t->etab.as<scm>());
        I.prof_note(KID_k_mpx_fill, 32.0 * slots, 32.0 * slots, 0.0);
        mpx_grow(I, t.get(), P, leaves, rc);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(I.st));
    } catch (...) { (void)hipStreamSynchronize(I.st); throw; }         // (the buffers go with `t`, after this wait)
    I.trees.push_back(t.get());
    return t.release();
}

// bpg_merkle_append on a prefix tree: a tree that outgrows its reserve takes min(limit, max(2 reserve, size + count)) first, then grows from the plan
void Engine::merkle_append_prefix(DeviceMerkle *t, uint64_t count, const uint8_t *leaves, uint64_t *first_index_out, uint8_t *root_out) {
    const uint64_t limit = merkle_prefix_limit(t->depth);
    if (count > limit - t->size) throw std::invalid_argument("merkle_append: the tree holds " + std::to_string(t->size) + " of at most min(2^" + std::to_string(t->depth) + ", 2^24) leaves: no room for " + std::to_string(count) + " more");
    if (count && !leaves) throw std::invalid_argument("merkle_append: null leaves");
    const uint64_t first = t->size;
    if (count) {
        HIPCHK(hipSetDevice(device_));
        Impl &I = *impl_;
        const scm *rc = mimc_rc(I, device_);
        if (first + count > t->dims.reserve) mpx_relayout(I, t, std::min<uint64_t>(limit, std::max<uint64_t>(2ull * t->dims.reserve, first + count)));
        const MerklePrefixGrowPlan P = plan_merkle_prefix_grow(t->depth, t->dims.reserve, first, first + count);
        try {
            mpx_grow(I, t, P, leaves, rc);
            HIPCHK(hipStreamSynchronize(I.st));
        } catch (...) { (void)hipStreamSynchronize(I.st); throw; }
        t->size = first + count;
    }
    if (first_index_out) *first_index_out = first;
    if (root_out) merkle_nodes(t, 0, 0, 1, root_out);
}

void Engine::merkle_reserve(DeviceMerkle *t, uint64_t leaves) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_reserve: not a tree of this context");
    if (t->keyed) throw std::invalid_argument("merkle_reserve: a keyed tree grows its arrays height by height as keys are put");
    if (!t->prefix) throw std::invalid_argument("merkle_reserve: a tree in the dense layout holds all of its 2^depth leaves already");
    if (leaves > merkle_prefix_limit(t->depth)) throw std::invalid_argument("merkle_reserve: beyond min(2^depth, 2^24) leaves");
    if (leaves <= t->dims.reserve) return;
    HIPCHK(hipSetDevice(device_));
    mpx_relayout(*impl_, t, leaves);
}

void Engine::merkle_reserved(DeviceMerkle *t, uint64_t *reserve_out, uint64_t *bytes_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_reserved: not a tree of this context");
    if (t->keyed) {                                         // (held keys, bytes held)
        if (reserve_out) *reserve_out = t->size;
        if (bytes_out) *bytes_out = mkx_bytes(t);
        return;
    }
    if (reserve_out) *reserve_out = t->prefix ? t->dims.reserve : (1ull << t->depth);
    if (bytes_out) *bytes_out = t->prefix ? merkle_prefix_bytes(t->dims) : (2ull << t->depth) * sizeof(scm);
}

// ------------------------------------------------------------------------------------------------ Merkle trees in the keyed layout (hip/k_merkle_keyed.cuh)
static_assert(MERKLE_KEYED_CLIMB_PARENTS == BPG_MERKLE_TOP_PARENTS, "host/merkle_keyed_plan.hpp plans for the one block of k_mkx_climb");

// The host's whole share of a put: the permutation that sorts the keys.  Refused: a key at or beyond 2^depth, a key given twice.  No device, no tree.
std::vector<uint32_t> Engine::merkle_key_order(uint32_t depth, uint64_t count, const uint64_t *keys) {
    if (depth < 1 || depth > MERKLE_KEYED_MAX_DEPTH || count > MERKLE_KEYED_MAX_KEYS || (count && !keys)) throw std::invalid_argument("merkle keys: depth must be 1..32, at most 2^24 keys");
    std::vector<uint32_t> order((size_t)count);
    for (uint32_t i = 0; i < count; i++) {
        if (keys[i] >> depth) throw std::invalid_argument("merkle keys: key " + std::to_string(keys[i]) + " is beyond 2^depth");
        order[i] = i;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    for (uint32_t i = 1; i < count; i++)
        if (keys[order[i]] == keys[order[i - 1]]) throw std::invalid_argument("merkle keys: key " + std::to_string(keys[order[i]]) + " is given twice");
    return order;
}

DeviceMerkle *Engine::merkle_build_keyed(uint32_t depth, uint64_t count, const uint64_t *keys, const uint8_t *leaves, const uint8_t *empty, const std::vector<uint32_t> *sorted_order) {
    if (depth < 1 || depth > MERKLE_KEYED_MAX_DEPTH) throw std::invalid_argument("merkle_build_keyed: depth must be 1..32");
    if (count > MERKLE_KEYED_MAX_KEYS) throw std::invalid_argument("merkle_build_keyed: more than 2^24 keys");
    if (count && (!keys || !leaves)) throw std::invalid_argument("merkle_build_keyed: null keys or leaves");
    std::unique_ptr<DeviceMerkle> t(new DeviceMerkle());
    t->owner = this; t->depth = depth; t->keyed = true;
    if (empty) { uint32_t w[8]; std::memcpy(w, empty, 32); t->empty = sc_from_words(w); }
    t->empty_nodes = merkle_empty_chain(depth, t->empty);
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    try {
        // the empty tree: the table of constants and no stored node; then the one mechanism
        t->etab.ensure(t->empty_nodes.size() * sizeof(scm));
        HIPCHK(hipMemcpyAsync(t->etab.p, t->empty_nodes.data(), t->empty_nodes.size() * sizeof(scm), hipMemcpyHostToDevice, I.st));
        HIPCHK(hipStreamSynchronize(I.st));
        merkle_put(t.get(), count, keys, leaves, nullptr, nullptr, false, sorted_order);
    } catch (...) { (void)hipStreamSynchronize(I.st); throw; }         // (the buffers go with `t`, after this wait)
    I.trees.push_back(t.get());
    return t.release();
}

// The one mechanism of a keyed tree.  Host: sort the keys (the leaves follow), refuse duplicates and keys beyond 2^depth.  Device: the structure bottom-up
// (classify, scan, scatter per height; one read-back of two counts per height, at most `depth` of them), then every allocation, then the merges, then the
// hashing from plan_merkle_keyed_hash.  Nothing is stored into the tree before the last check and the last allocation.
void Engine::merkle_put(DeviceMerkle *t, uint64_t count, const uint64_t *keys, const uint8_t *leaves, uint64_t *inserted_out, uint8_t *root_out, bool held_only,
                        const std::vector<uint32_t> *sorted_order) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_put: not a tree of this context");
    if (!t->keyed) throw std::invalid_argument("merkle_put: not a keyed tree (bpg_merkle_append and bpg_merkle_update serve the dense and the prefix layout)");
    if (count > MERKLE_KEYED_MAX_KEYS) throw std::invalid_argument("merkle_put: more than 2^24 keys");
    if (count && (!keys || !leaves)) throw std::invalid_argument("merkle_put: null pointer");
    const uint32_t D = t->depth;
    uint64_t inserted = 0;
    if (count) {
        const uint32_t m0 = (uint32_t)count;
        for (uint32_t i = 0; i < m0; i++)
            if (keys[i] >> D) throw std::invalid_argument("merkle_put: key " + std::to_string(keys[i]) + " is beyond 2^depth");
        const std::vector<uint32_t> own = (sorted_order && sorted_order->size() == m0) ? std::vector<uint32_t>() : merkle_key_order(D, count, keys);
        const std::vector<uint32_t> &order = own.empty() ? *sorted_order : own;
        std::vector<uint32_t> sorted(m0);
        for (uint32_t i = 0; i < m0; i++) sorted[i] = (uint32_t)keys[order[i]];
        std::vector<uint8_t> stage((size_t)m0 * 32);
        for (uint32_t i = 0; i < m0; i++) std::memcpy(stage.data() + 32 * (size_t)i, leaves + 32 * (size_t)order[i], 32);

        HIPCHK(hipSetDevice(device_));
        Impl &I = *impl_;
        const scm *rc = mimc_rc(I, device_);
        const scm *E = t->etab.as<scm>();
        // where the dirty list and the brand-new positions of height s go: at most min(count, what the height can hold) entries each
        uint64_t off[MERKLE_KEYED_MAX_DEPTH + 2] = {0};
        for (uint32_t s = 0; s <= D; s++) off[s + 1] = off[s] + std::min<uint64_t>(m0, merkle_keyed_limit(D, s));
        const uint32_t tiles0 = (uint32_t)cdiv(m0, MERKLE_KEYED_SCAN_TILE);
        uint32_t dirty[MERKLE_KEYED_MAX_DEPTH + 1] = {0}, fresh[MERKLE_KEYED_MAX_DEPTH + 1] = {0};
        std::vector<DevBuf> npos(D + 1), nval(D + 1), retired;
        try {
            I.mkx_dirty.ensure(off[D + 1] * 4); I.mkx_fresh.ensure(off[D + 1] * 4);
            I.mkx_flags.ensure((size_t)m0 * sizeof(uint2)); I.mkx_sums.ensure((size_t)tiles0 * sizeof(uint2)); I.mkx_totals.ensure((D + 1) * sizeof(uint2));
            I.mk_in.ensure(stage.size());
            uint32_t *dl = I.mkx_dirty.as<uint32_t>(), *fl = I.mkx_fresh.as<uint32_t>();
            uint2 *flags = I.mkx_flags.as<uint2>(), *sums = I.mkx_sums.as<uint2>(), *totals = I.mkx_totals.as<uint2>();
            HIPCHK(hipMemcpyAsync(dl, sorted.data(), (size_t)m0 * 4, hipMemcpyHostToDevice, I.st));
            HIPCHK(hipMemcpyAsync(I.mk_in.p, stage.data(), stage.size(), hipMemcpyHostToDevice, I.st));
            // ---- the structure, read-only on the tree: per height held or brand-new, the brand-new positions, the dirty list of the height above
            dirty[0] = m0;
            bool classify = true;
            for (uint32_t s = 0; s < D; s++) {
                const uint32_t m = dirty[s], tiles = (uint32_t)cdiv(m, MERKLE_KEYED_SCAN_TILE);
                BPG_LAUNCH(I, k_mkx_classify, dim3(cdiv(m, 256)), dim3(256), t->kpos[s].as<uint32_t>(), t->kcnt[s], dl + off[s], m, classify ? 1u : 0u, 1u, flags);
                BPG_LAUNCH(I, k_mkx_scan_sums, dim3(tiles), dim3(256), flags, m, sums);
                BPG_LAUNCH(I, k_mkx_scan_top, dim3(1), dim3(256), sums, tiles, totals + s);
                BPG_LAUNCH(I, k_mkx_scatter, dim3(tiles), dim3(256), dl + off[s], flags, m, sums, fl + off[s], dl + off[s + 1]);
                HIPCHK(hipGetLastError());
                uint2 tot;
                HIPCHK(hipMemcpyAsync(&tot, totals + s, sizeof tot, hipMemcpyDeviceToHost, I.st));
                HIPCHK(hipStreamSynchronize(I.st));
                fresh[s] = tot.x; dirty[s + 1] = tot.y;
                if (fresh[s] > m || !tot.y || tot.y > m || (uint64_t)tot.y > merkle_keyed_limit(D, s + 1)) throw std::logic_error("merkle_put: a scan total beyond its list");
                if (s == 0) {
                    if (held_only && fresh[0]) throw std::invalid_argument("merkle_update: a key that the tree does not hold (bpg_merkle_put inserts keys)");
                    if ((uint64_t)t->kcnt[0] + fresh[0] > MERKLE_KEYED_MAX_KEYS) throw std::invalid_argument("merkle_put: the tree would hold more than 2^24 keys");
                }
                if (!fresh[s]) classify = false;            // a brand-new parent has only brand-new dirty children: nothing above is brand-new
            }
            fresh[D] = (classify && !t->kcnt[D]) ? 1u : 0u;  // the root is brand-new exactly when the tree held no key
            const MerkleKeyedHashPlan P = plan_merkle_keyed_hash(D, dirty);
            // ---- every allocation before the first store: new arrays for the heights that outgrow theirs, the scratch of a merge that stays in place
            uint64_t grow_bytes = 0, scratch = 0;
            uint32_t cap[MERKLE_KEYED_MAX_DEPTH + 1];
            for (uint32_t s = 0; s <= D; s++) {
                cap[s] = t->kcap[s];
                if (!fresh[s]) continue;
                const uint64_t need = (uint64_t)t->kcnt[s] + fresh[s];
                if (need > merkle_keyed_limit(D, s)) throw std::logic_error("merkle_put: more positions than a height has");
                cap[s] = merkle_keyed_capacity(t->kcap[s], need, merkle_keyed_limit(D, s));
                if (cap[s] != t->kcap[s]) grow_bytes += (uint64_t)cap[s] * (sizeof(uint32_t) + sizeof(scm)); else scratch = std::max<uint64_t>(scratch, need);
            }
            if (grow_bytes) {
                size_t free_b = 0, total_b = 0;
                HIPCHK(hipMemGetInfo(&free_b, &total_b));
                if (grow_bytes + (64u << 20) > free_b)
                    throw DeviceError("merkle_put: the tree needs " + std::to_string(grow_bytes >> 20) + " MB more and the device has " + std::to_string(free_b >> 20) + " MB free");
            }
            for (uint32_t s = 0; s <= D; s++)
                if (cap[s] != t->kcap[s]) { npos[s].ensure((size_t)cap[s] * sizeof(uint32_t)); nval[s].ensure((size_t)cap[s] * sizeof(scm)); }
            I.mkx_merge.ensure(scratch * (sizeof(uint32_t) + sizeof(scm)));
            // ---- the merges, bottom-up; a height that keeps its arrays merges into the scratch and is copied back in stream order
            for (uint32_t s = 0; s <= D; s++) {
                if (!fresh[s]) continue;
                const uint32_t cnt = t->kcnt[s], total = cnt + fresh[s];
                const uint32_t *fresh_s = fl + off[s];
                if (s == D) HIPCHK(hipMemsetAsync(fl + off[D], 0, 4, I.st));       // the root's one position, 0, was never scattered (no launch at height D)
                const bool grown = cap[s] != t->kcap[s];
                uint32_t *dpos = grown ? npos[s].as<uint32_t>() : I.mkx_merge.as<uint32_t>() + 8 * (size_t)total;
                scm *dval = grown ? nval[s].as<scm>() : I.mkx_merge.as<scm>();
                BPG_LAUNCH(I, k_mkx_merge, dim3(cdiv(total, 256)), dim3(256), t->kpos[s].as<uint32_t>(), t->kval[s].as<scm>(), cnt, fresh_s, fresh[s], dpos, dval, E + s);
                I.prof_note(KID_k_mkx_merge, 72.0 * total, 72.0 * total, 0.0);
                HIPCHK(hipGetLastError());
                if (grown) {
                    retired.push_back(std::move(t->kpos[s])); retired.push_back(std::move(t->kval[s]));     // released after the wait below: the merge reads them
                    t->kpos[s] = std::move(npos[s]); t->kval[s] = std::move(nval[s]);
                    t->kcap[s] = cap[s];
                } else {
                    HIPCHK(hipMemcpyAsync(t->kpos[s].p, dpos, (size_t)total * sizeof(uint32_t), hipMemcpyDeviceToDevice, I.st));
                    HIPCHK(hipMemcpyAsync(t->kval[s].p, dval, (size_t)total * sizeof(scm), hipMemcpyDeviceToDevice, I.st));
                }
                t->kcnt[s] = total;
            }
            inserted = fresh[0];
            t->size = t->kcnt[0];
            // ---- the hashing: the leaves, the wide heights bottom-up, the climb
            BPG_LAUNCH(I, k_mkx_set_leaves, dim3(cdiv(m0, 256)), dim3(256), t->kpos[0].as<uint32_t>(), t->kval[0].as<scm>(), t->kcnt[0], dl, I.mk_in.as<uint32_t>(), m0);
            for (uint32_t k = 0; k < P.n_wide; k++) {
                const uint32_t s = P.wide[k].height;
                if (s >= D || P.wide[k].count != dirty[s + 1]) throw std::logic_error("merkle keyed plan: a wide step that is not a dirty list");
                BPG_LAUNCH(I, k_mkx_level, dim3(cdiv(dirty[s + 1], 256)), dim3(256), t->kpos[s].as<uint32_t>(), t->kval[s].as<scm>(), t->kcnt[s], t->kpos[s + 1].as<uint32_t>(),
                           t->kval[s + 1].as<scm>(), t->kcnt[s + 1], dl + off[s + 1], dirty[s + 1], E + s, rc);
                note_nodes(I, KID_k_mkx_level, dirty[s + 1]);
            }
            if (!P.climb || P.climb_height >= D) throw std::logic_error("merkle keyed plan: keys without a climb");
            MkxDirty L{};
            for (uint32_t s = P.climb_height + 1; s <= D; s++) {
                if (dirty[s] > BPG_MERKLE_TOP_PARENTS) throw std::logic_error("merkle keyed plan: a climb height that does not fit one block");
                L.list[s] = dl + off[s]; L.m[s] = dirty[s];
            }
            BPG_LAUNCH(I, k_mkx_climb, dim3(1), dim3(256), mkx_view(t), L, P.climb_height, E, rc);
            note_nodes(I, KID_k_mkx_climb, P.climb_evals);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(I.st));
        } catch (...) { (void)hipStreamSynchronize(I.st); throw; }         // (`npos`, `nval` and `retired` go after this wait)
    }
    if (inserted_out) *inserted_out = inserted;
    if (root_out) merkle_nodes(t, 0, 0, 1, root_out);
}

void Engine::merkle_get(DeviceMerkle *t, uint64_t count, const uint64_t *keys, uint8_t *leaves_out, uint8_t *held_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_get: not a tree of this context");
    if (!count) return;
    if (!keys || !leaves_out) throw std::invalid_argument("merkle_get: null pointer");
    std::vector<uint32_t> idx(count);
    for (uint64_t i = 0; i < count; i++) {
        if (keys[i] >> t->depth) throw std::invalid_argument("merkle_get: key " + std::to_string(keys[i]) + " is beyond 2^depth");
        idx[i] = (uint32_t)keys[i];
    }
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    const uint64_t per = 1ull << 20;
    const size_t n_max = (size_t)std::min(count, per);
    I.mk_in.ensure(n_max * 4); I.mk_out.ensure(n_max * 33);           // [leaves | held bytes]
    for (uint64_t at = 0; at < count; at += per) {
        const uint32_t n = (uint32_t)std::min(per, count - at);
        HIPCHK(hipMemcpyAsync(I.mk_in.p, idx.data() + at, (size_t)n * 4, hipMemcpyHostToDevice, I.st));
        uint8_t *held_dev = I.mk_out.as<uint8_t>() + n_max * 32;
        if (t->keyed)
            BPG_LAUNCH(I, k_mkx_get, dim3(cdiv(n, 256)), dim3(256), t->kpos[0].as<uint32_t>(), t->kval[0].as<scm>(), t->kcnt[0], t->etab.as<scm>(), I.mk_in.as<uint32_t>(), n, I.mk_out.as<uint32_t>(), held_dev);
        else if (t->prefix)                                 // a leaf right of the reserve is not stored: E_0
            BPG_LAUNCH(I, k_mkx_gather, dim3(cdiv(n, 256)), dim3(256), t->tree.as<scm>() + t->dims.off[0], (uint64_t)t->dims.width[0], t->etab.as<scm>(), I.mk_in.as<uint32_t>(), n, I.mk_out.as<uint32_t>());
        else
            BPG_LAUNCH(I, k_mkx_gather, dim3(cdiv(n, 256)), dim3(256), t->tree.as<scm>() + (1ull << t->depth), 1ull << t->depth, (const scm *)nullptr, I.mk_in.as<uint32_t>(), n, I.mk_out.as<uint32_t>());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(leaves_out + (size_t)at * 32, I.mk_out.p, (size_t)n * 32, hipMemcpyDeviceToHost, I.st));
        if (t->keyed && held_out) HIPCHK(hipMemcpyAsync(held_out + at, held_dev, n, hipMemcpyDeviceToHost, I.st));
        HIPCHK(hipStreamSynchronize(I.st));
    }
    if (!t->keyed && held_out) for (uint64_t i = 0; i < count; i++) held_out[i] = keys[i] < t->size ? 1 : 0;         // held = index < size
}

void Engine::merkle_keys(DeviceMerkle *t, uint64_t first, uint64_t count, uint64_t *keys_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_keys: not a tree of this context");
    if (first > t->size || count > t->size - first) throw std::invalid_argument("merkle_keys: a run beyond the " + std::to_string(t->size) + " keys the tree holds");
    if (!count) return;
    if (!keys_out) throw std::invalid_argument("merkle_keys: null output");
    if (!t->keyed) { for (uint64_t i = 0; i < count; i++) keys_out[i] = first + i; return; }       // key i = i
    HIPCHK(hipSetDevice(device_));
    Impl &I = *impl_;
    I.mk_out.ensure((size_t)count * 8);
    BPG_LAUNCH(I, k_mkx_keys, dim3(cdiv(count, 256)), dim3(256), t->kpos[0].as<uint32_t>(), (uint32_t)first, (uint32_t)count, I.mk_out.as<uint64_t>());
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(keys_out, I.mk_out.p, (size_t)count * 8, hipMemcpyDeviceToHost, I.st));
    HIPCHK(hipStreamSynchronize(I.st));
}

void Engine::merkle_node_counts(DeviceMerkle *t, uint64_t *counts_out, uint64_t *bytes_out) {
    if (!t || t->owner != this) throw std::invalid_argument("merkle_node_counts: not a tree of this context");
    if (!t->keyed) throw std::invalid_argument("merkle_node_counts: not a keyed tree (bpg_merkle_reserved tells what the other layouts hold)");
    if (counts_out) for (uint32_t s = 0; s <= t->depth; s++) counts_out[s] = t->kcnt[s];
    if (bytes_out) *bytes_out = mkx_bytes(t);
}

}  // namespace bpg
