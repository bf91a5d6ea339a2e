// HIP kernels of the Bulletproofs R1CS prove path for gfx950 (MI355X).  Integer VALU work (v_mad_u64_u32 chains);
// no MFMA - this is 255-bit modular arithmetic, not a dense contraction.  Hot-path rows of SURVEY.md section 8(a):
//   a7  BulletproofGens::new            k_gens_derive + k_normalize_niels
//   a1-a3,a6  Pedersen commits          k_pedersen (window tables of B and B_blinding: k_tt_bases, k_tt_multiples)
//   a9  A_I, A_O, S multiscalar muls    k_msm_digits (digits + coarse counts), k_scan_blocksums / _apply, k_msm_scatter1, k_msm_sort2 (two-level sort), k_bucket_chunks,
//                                       k_bucket_combine(_per_bucket, _heavy), k_bucket_reduce, k_window_sums (a shared device) / k_window_sums_quad (a proof alone)
//                                       (bucket method: digits -> coarse partition in LDS -> fine counting sort -> balanced bucket sweep -> reductions;
//                                       the 17 window sums are recombined and encoded on the host, host/fe51.hpp)
//       equal scalars of a_L, a_R        k_merge_insert, k_merge_plan, k_merge_groups, k_merge_members, k_merge_sum (k_merge.cuh): terms of A_I that carry the same value share one
//                                       bucket entry per window on the sum of their generators; once per uploaded witness
//   a10 vector-polynomial phase         k_exp_table, k_flatten, k_poly_t, k_poly_eval, k_reduce_partials
//   a11 inner-product argument          above 2^12 generators (a circuit of N <= 2^14: none): k_ipa_prep, the MSM kernels, k_tt_advance, one generator fold per group of rounds -
//                                       k_fold_points_wnaf on the original generators (tables of (2m+1) * 2^(64j) * P: k_odd_start(_ext), k_odd_step,
//                                       k_dbl_times); on folded ones k_fold_points_quadw (a proof alone) / k_fold_points_regw (a shared device): width-4 NAF
//                                       steps against multiples the kernel makes itself - and k_fold_points_quad / _split / _reg<NT> / k_fold_points for the
//                                       shapes those two do not take (first groups, outputs that do not fill whole blocks); below: k_tt_bases,
//                                       k_tt_multiples, k_tt_factors, then k_tt_advance, k_tt_round, k_tt_finish per round
//   f1  Verifier::verify                k_decompress, k_flatten_const, k_ipa_s, k_verify_scalars + one MSM
//       batch verification              the same per proof with k_verify_scalars_acc (weighted g_i, h_i added into two shared accumulators) + one MSM per batch
//       lockstep verification           (k_vwave.cuh; K proofs of ONE resident circuit) per wave, whatever K and N: k_vw_exp (y^-i, z^j of every item), k_vw_tails (per-item
//                                       parameter and derived coefficient slots, only when an item brings constants), k_vw_flatten (a lane per (item, column)),
//                                       k_vw_small (a block per item: w_V, w_c, delta), k_vw_scalars (a lane per generator index, the wave's items in chunks,
//                                       s_i formed in registers), k_vw_reduce (chunk sums into the call's accumulators) + one MSM per call
//       lockstep batch proving          (N <= 2^tt_orig_lg, k_batch.cuh) one launch per stage for every proof of a wave: the upload kernels on one block-diagonal
//                                       matrix, k_bt_commit3(_finish), k_bt_compress, k_bt_exp, k_flatten, k_bt_poly_t, k_pedersen, k_bt_poly_eval, k_bt_factors,
//                                       then k_bt_advance, k_bt_round, k_bt_finish, k_bt_compress per round and k_bt_fold_scalars
//                                       k_bt_commit_v: the Pedersen commitments of a template wave's committed values, from the values the wave uploaded for its
//                                       witness evaluation - one launch per wave (bpg_r1cs_prove_template_batch_commit)
//       circuit templates               k_witness_eval (k_witness.cuh): a_L, a_R, a_O of a resident circuit from the committed values of a fresh witness, by interpreting the
//                                       recorded witness program - one launch per level of its schedule, one lane per segment (replaces the host's assembly + upload);
//                                       k_witness_ck_verify: after a checkpointed assign, the caller's intermediate values against the computed ones, a lane per checkpoint
//       a template repeated K times      (k_repeat.cuh) k_repeat_colptr, k_repeat_entries, k_repeat_coef: the K-fold circuit's column-major matrix from the template's
//                                       resident one; k_witness_eval_repeat: its witness by the template's program, a lane per (segment, item) (one proof for K witnesses)
//       templates joined                 (k_join.cuh) k_join_colptr, k_join_entries, k_join_coef: the matrix of count_0 copies of part 0, then count_1 of part 1, ... from the
//                                       parts' resident ones; k_witness_eval_join: one launch per level for ALL parts, a block = 64 items of one segment of one part;
//                                       k_witness_ck_verify_join: the checkpoints of all parts in one launch (one proof for a mixed statement)
//       MiMC sponges, Merkle trees       (k_mimc.cuh; no row of the survey: the native hash in front of Prover::commit) k_mimc_sponge: one lane per item; a tree of 2^d leaves in
//                                       one heap-ordered array: k_merkle_leaves, k_merkle_level (one launch per level, one lane per parent), k_merkle_top (the levels of at
//                                       most 256 parents in one launch), k_merkle_level_list + k_merkle_set_leaves (leaf updates: the ancestors only), k_merkle_paths
//                                       (sibling lists, or the nodes on the paths), k_merkle_export (nodes as bytes); trees that grow (capacity 2^d, n leaves):
//                                       k_merkle_fill_empty (the empty-subtree constants, once per build), k_merkle_level_range (an interval of one level),
//                                       k_merkle_climb (from at most 256 dirty parents to the root in one launch) - launched from host/merkle_plan.hpp
//       Merkle trees, prefix layout      (k_merkle_prefix.cuh; depth up to 32, only the occupied prefix of every level stored, host/merkle_prefix_plan.hpp) k_mpx_fill (the
//                                       empty-subtree constants into stored, unoccupied slots), k_mpx_range (an interval of one height), k_mpx_climb (from at most 256
//                                       dirty parents through up to 32 heights to the root in one launch), k_mpx_list + k_mpx_set_leaves (leaf updates), k_mpx_paths,
//                                       k_mpx_export (both fall back to the tree's table of constants for a node that is not stored), k_mpx_relayout (a larger reserve)
//       Merkle trees, keyed layout       (k_merkle_keyed.cuh; leaves at any 32-bit key, per height the sorted positions that have a held key below them beside their values,
//                                       host/merkle_keyed_plan.hpp) the structure of a put: k_mkx_classify (held or brand-new, head flags), k_mkx_scan_sums / k_mkx_scan_top /
//                                       k_mkx_scatter (the scan in three launches: brand-new positions and the next height's dirty list), k_mkx_merge (old and brand-new
//                                       entries into a height's new arrays); its hashing: k_mkx_set_leaves, k_mkx_level (a height of more than 256 dirty parents),
//                                       k_mkx_climb (from at most 256 dirty parents to the root in one launch); reads by lookup: k_mkx_paths, k_mkx_export, k_mkx_get,
//                                       k_mkx_keys, and k_mkx_gather (bpg_merkle_get on the other two layouts)
//       R1CS check                       (k_check.cuh; bpg_r1cs_check: which multiplier, which constraint does the resident witness break) the row-major view of the resident
//                                       matrix, once per circuit: k_rowview_count, k_scan_blocksums / _apply, k_rowview_fill, k_rowview_long; per check: k_check_mul (a lane
//                                       per multiplier), k_check_rows (a lane per short row, the wave's ballot = one word of the violation bitmap), k_check_rows_long (a
//                                       wave per long row), k_check_count (bad rows and the first of them)
// The kernels live in k_points.cuh, k_scalars.cuh, k_ipa.cuh, k_verify.cuh, k_msm.cuh, k_merge.cuh, k_batch.cuh, k_witness.cuh, k_repeat.cuh, k_join.cuh, k_mimc.cuh, k_merkle_prefix.cuh, k_merkle_keyed.cuh, k_check.cuh and k_vwave.cuh, included at the end of
// this file in that order.
// Data layout in HBM: scalars = 8 x u32 Montgomery form, 32 B each, AoS (lane i <-> element i: 2 x 16 B coalesced
// loads); generator tables = affine Niels (y+x, y-x, 2dxy), 96 B per point, G at [0,N) and H at [N,2N); window tables =
// projective Niels (y+x, y-x, z, 2dt), 128 B per entry.
#pragma once
#include <hip/hip_runtime.h>
#include "ge.cuh"
#include "sc.cuh"
#include "../host/msm_plan.hpp"    // MsmPlan (argument of the MSM kernels) and the planner that fills it
#include "../host/fold_plan.hpp"   // FoldGroup, FoldWnaf, FoldQuadW (arguments of the fold kernels) and the recoders that fill them

namespace bpg {

#define BPG_MAX_SEGS 16                 // 4 segment bits in a sorted entry (sign | segment | 27 index bits)
struct MsmSegs {
    const scm *sc[BPG_MAX_SEGS];
    const ge_niels *pts[BPG_MAX_SEGS];
    const uint32_t *skip[BPG_MAX_SEGS]; // optional bit per term: 1 = the term takes no part (its scalar was merged into another segment's term, k_merge_*); nullptr = none
    uint32_t len[BPG_MAX_SEGS];
    uint32_t start[BPG_MAX_SEGS + 1];   // prefix of len
    uint32_t msm[BPG_MAX_SEGS];
    uint32_t lgblk[BPG_MAX_SEGS];       // element e of the segment is point ((e >> lgblk) << (lgblk+1)) | (e & (2^lgblk - 1)): every
    uint32_t nseg;                      // other block of 2^lgblk points (grouped IPA rounds); 31 = contiguous
};
__device__ __forceinline__ uint32_t msm_point_index(const MsmSegs &S, uint32_t seg, uint32_t e) {
    const uint32_t lg = S.lgblk[seg];
#ifdef BPG_DIAG_INDEX_MASK
    // DIAGNOSTIC BUILD ONLY (tools/diag/mask_build.sh; never defined for the product): every gathered point index is masked, so the sweep does the
    // same arithmetic on a table that fits a cache level - wrong sums, same instruction stream - to tell exposed memory time from issue time
    return (((e >> lg) << (lg + 1)) | (e & ((1u << lg) - 1u))) & (BPG_DIAG_INDEX_MASK);
#else
    return ((e >> lg) << (lg + 1)) | (e & ((1u << lg) - 1u));
#endif
}

}  // namespace bpg

#include "k_points.cuh"
#include "k_scalars.cuh"
#include "k_ipa.cuh"
#include "k_verify.cuh"
#include "k_msm.cuh"
#include "k_merge.cuh"
#include "k_batch.cuh"
#include "k_witness.cuh"
#include "k_repeat.cuh"
#include "k_join.cuh"
#include "k_mimc.cuh"
#include "k_merkle_prefix.cuh"
#include "k_merkle_keyed.cuh"
#include "k_check.cuh"
#include "k_vwave.cuh"
