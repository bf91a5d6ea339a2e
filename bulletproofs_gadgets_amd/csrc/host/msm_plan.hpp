// What one bucket-method MSM runs, decided before anything is sized or launched: window width, two-level-sort split, tiling, chunk length of the
// sweep, arena layout, workspace sizes, how the boundary pieces are combined and how the window sums are taken.  plan_msm() is a pure function of
// the call's shape and the context's knobs - no HIP, no allocation - so tests/hostcheck/plans.cpp checks it on the CPU; Engine::Impl::msm() sizes its
// buffers and launches hip/k_msm.cuh from the value it returns, and Engine::test_msm prints that same value as its evidence.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include "r1cs_error.hpp"

namespace bpg {

// Kernel argument of hip/k_msm.cuh (passed by value): the windows, the two-level sort's split and the tiling of one call.
struct MsmPlan {
    uint32_t nmsm, W, nb, lgTile, tmax;
    uint8_t off[132];            // off[j] = j * 254 / W, the first bit of window j, j <= W (the host fills it: the kernel divided by W twice per digit)
    uint32_t fb, CB;             // two-level sort: a bucket index splits into CB coarse bins x 2^fb fine slots (nb = CB << fb)
    uint32_t term_start[5];      // first global term of MSM m (term_start[nmsm] = total)
    uint32_t tile_start[5];      // first tile of MSM m
    uint32_t bias[8];
};

#define SCAN_CHUNK 2048                 // counts per block of k_scan_blocksums / k_scan_apply
#define HEAVY_CHUNKS 32                 // a bucket spread over more chunks than this goes on the heavy list (k_bucket_combine*)
constexpr size_t MSM_POINT_BYTES = 128;                      // sizeof(ge_ext): an extended point in HBM
constexpr size_t MSM_LDS_BYTES = 64 * 1024;                  // LDS of a block: the coarse histograms of k_msm_digits
constexpr uint32_t MSM_TICKETS = 1024;                       // words of the ticket array of k_window_sums_quad: one per window
constexpr size_t MSM_WS_SLOT_BYTES = 4 * 128 * 128;          // pinned host slot of the window sums: nmsm <= 4, W <= 127 (c >= 2), 128 B per point

// The shape of one call: its segments in order (MsmSegs::len, MsmSegs::msm), the number of results, and how many terms carry a skip bit.
struct MsmShape {
    uint32_t nseg;
    const uint32_t *len, *msm;
    uint32_t nmsm;
    uint32_t skipped;            // terms whose skip bit is set (they make no entries): the window width and the entry lists are sized for the rest
};
// What the context settled on (Engine::Impl; BPG_MSM_CMIN, BPG_MSM_CMAX, BPG_RSEG, BPG_LGCH, BPG_SWEEP_RESIDENT, BPG_WINDOW_QUAD, BPG_WINDOW_QUAD_BLOCKS)
// and whether this call takes the shared-device variants.
struct MsmKnobs {
    uint32_t cmin = 2, cmax = 15, cmax_shared = 16, rseg = 8, lgch = 0, sweep_blocks_resident = 1024;
    bool window_quad = true;
    uint32_t window_quad_blocks = 288;
    bool shared = false;
};

struct MsmRun {
    MsmPlan P;
    uint32_t total, live;        // terms of the call, and those that can make entries (the others were merged away: MsmSegs::skip)
    uint32_t nkeys;              // buckets of the call: nmsm * W * nb
    uint32_t seg, nsegpw, nred;  // k_bucket_reduce: buckets per thread, segments per window, threads
    uint32_t ntiles, nflat, nblk1, K;   // two-level sort: tiles, (bin, tile) counters, scan blocks, coarse bins
    uint64_t Mub;                // upper bound of the entry count (zero digits are skipped)
    uint32_t CH, nchunks;        // balanced sweep: sorted entries per thread, threads
    // arena layout: [digits | entries1] overlaid by the sweep's partial sums (slots), then entries at b_front
    size_t b_digits, b_e1, b_entries, b_slots, b_front;
    // bytes of every workspace buffer (counts, starts1 and cursor share bytes_counts), and the dynamic LDS of k_msm_digits
    size_t bytes_starts, bytes_buckets, bytes_partial, bytes_heavy, bytes_medium, bytes_counts, bytes_blocksum, bytes_open_keys, bytes_wsums, bytes_wq_stage, lds_digits;
    bool shared;                 // planned for a device shared with other proofs
    bool per_bucket;             // boundary pieces joined by one thread per bucket (k_bucket_combine_per_bucket) instead of one per chunk boundary
    bool quad;                   // window sums by k_window_sums_quad (lgper, window_blocks) instead of k_window_sums (window_threads)
    uint32_t lgper, window_blocks, window_threads;
};

inline MsmRun plan_msm(const MsmShape &S, const MsmKnobs &knobs) {
    auto al256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    auto cdiv = [](uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); };
    MsmRun R; std::memset(&R, 0, sizeof R);
    const uint32_t nmsm = S.nmsm;
    if (nmsm < 1 || nmsm > 4) throw std::logic_error("msm: 1..4 results per call");
    uint32_t total = 0, maxseg = 1;
    for (uint32_t k = 0; k < S.nseg; k++) { total += S.len[k]; maxseg = std::max(maxseg, S.len[k]); }
    const uint32_t live = total - std::min(total, S.skipped);
    uint32_t per = live / nmsm; if (per < 1) per = 1;
    const int cap = (int)(knobs.shared ? knobs.cmax_shared : knobs.cmax);
    int cc = (int)ceil_log2(per) - 4; if (cc < (int)knobs.cmin) cc = (int)knobs.cmin; if (cc > cap) cc = cap;
    // two-level sort: entry = sign | fb fine bits | 4 segment bits | index in segment -> 27 - fb index bits; at most 512 coarse bins
    uint32_t fb = 0;
    {
        const uint32_t lgseg = ceil_log2(maxseg);
        if (lgseg > 27) throw std::invalid_argument("msm: segment too long");
        const uint32_t fbmax = std::min<uint32_t>(7, 27 - lgseg);
        if (cc - 1 > (int)fbmax + 9) cc = (int)fbmax + 10;
        fb = std::min<uint32_t>(fbmax, (uint32_t)cc - 1);
    }
    // W near-equal windows over 254 bits (window j starts at bit j * 254 / W: MsmPlan::off); the widest has cmax bits -> 2^(cmax-1) buckets per window
    const uint32_t W = (254 + (uint32_t)cc - 1) / (uint32_t)cc, cmax = (254 + W - 1) / W, nb = 1u << (cmax - 1);
    if (fb > cmax - 1) fb = cmax - 1;
    R.total = total; R.live = live; R.shared = knobs.shared;
    R.nkeys = nmsm * W * nb;
    R.seg = std::min(knobs.rseg, nb); R.nsegpw = nb / R.seg;           // both powers of two (rseg is validated at context creation)
    R.nred = nmsm * W * R.nsegpw;
    // tiling plan: the segments of one MSM are contiguous; tiles never span two MSMs
    MsmPlan &P = R.P;
    P.nmsm = nmsm; P.W = W; P.nb = nb; P.fb = fb; P.CB = nb >> fb;
    {
        const uint32_t lg = 12;                                 // k_msm_scatter1 stages one tile of entries in LDS (MSM_TILE1_MAX)
        P.lgTile = lg;
        uint32_t k = 0, start = 0;                              // start = first term of segment k
        for (uint32_t m = 0; m < nmsm; m++) {
            P.term_start[m] = k < S.nseg ? start : total;
            while (k < S.nseg && S.msm[k] == m) start += S.len[k++];
        }
        if (k != S.nseg) throw std::logic_error("msm: segments must be grouped by result in ascending order");
        P.term_start[nmsm] = total;
        for (uint32_t m = 0; m < nmsm; m++) {
            const uint32_t nt = cdiv(P.term_start[m + 1] - P.term_start[m], 1u << lg);
            P.tile_start[m + 1] = P.tile_start[m] + nt; if (nt > P.tmax) P.tmax = nt;
        }
        if (P.tmax == 0) P.tmax = 1;
        for (uint32_t j = 0; j < W; j++) { const uint32_t bit = ((j + 1) * 254u) / W - 1; P.bias[bit >> 5] |= 1u << (bit & 31); }
        for (uint32_t j = 0; j <= W; j++) P.off[j] = (uint8_t)((j * 254u) / W);
    }
    R.ntiles = P.tile_start[nmsm];
    R.bytes_starts = (size_t)(R.nkeys + 1) * 4;
    R.bytes_buckets = (size_t)R.nkeys * MSM_POINT_BYTES;
    R.bytes_partial = (size_t)2 * R.nred * MSM_POINT_BYTES;             // acc and run of every segment
    // balanced sweep: CH sorted entries per thread.  About 32, adjusted so that the launch's blocks fill the device a whole number of times: the
    // sweep keeps sweep_blocks_resident blocks of 256 threads on the CUs at once (4 waves per SIMD at its register count), and 4.25 rounds of
    // blocks cost what 5 do.  BPG_LGCH pins a power of two instead (diagnostics).
    const uint64_t Mub = (uint64_t)live * W;
    uint32_t CH = 32;
    if (knobs.lgch) CH = 1u << knobs.lgch;
    else if (knobs.shared && Mub >= (uint64_t)knobs.sweep_blocks_resident * 256 * 64) CH = 64;      // other proofs fill the device and this sweep is long: longer chunks, half the boundary pieces to combine (18.7 against 19.2 ms per proof sustained)
    else {
        const uint64_t slots = (uint64_t)knobs.sweep_blocks_resident * 256;
        uint64_t rounds = (Mub + slots * 16) / (slots * 32);    // nearest whole number of rounds at 32 entries per thread
        if (rounds < 1) rounds = 1;
        CH = (uint32_t)std::max<uint64_t>(4, (Mub + slots * rounds - 1) / (slots * rounds));
    }
    R.Mub = Mub; R.CH = CH;
    R.nchunks = cdiv(Mub ? Mub : 1, CH);
    R.b_digits = al256((size_t)(total ? total : 1) * W * 2); R.b_e1 = al256((size_t)(live ? live : 1) * W * 4); R.b_entries = R.b_e1;
    R.b_slots = al256((size_t)R.nchunks * 2 * MSM_POINT_BYTES);
    R.b_front = std::max(R.b_digits + R.b_e1, R.b_slots);
    R.bytes_heavy = ((size_t)R.nchunks / HEAVY_CHUNKS + 2) * 4; R.bytes_medium = ((size_t)R.nchunks / 2 + 2) * 4;      // a bucket on the medium list crosses at least two boundaries
    // (kernels.cuh, "two-level sort"): digits once, coarse partition with coalesced runs, fine counting sort inside each coarse bin
    const uint64_t nflat64 = (uint64_t)nmsm * W * P.CB * P.tmax;
    if (nflat64 >= (1ull << 31)) throw std::invalid_argument("msm: too many tiles");
    R.nflat = (uint32_t)nflat64; R.nblk1 = cdiv(R.nflat, SCAN_CHUNK); R.K = nmsm * W * P.CB;
    R.bytes_counts = (size_t)(R.nflat + 1) * 4; R.bytes_blocksum = (size_t)(R.nblk1 + 1) * 4;
    R.lds_digits = (size_t)W * P.CB * 4;
    if (R.lds_digits > MSM_LDS_BYTES) throw std::logic_error("msm: coarse histograms exceed the LDS of a block");
    R.bytes_open_keys = (size_t)R.nchunks * 4;
    // joining the pieces of buckets that cross chunk boundaries: one thread per boundary where chunks are at least as long as the average bucket
    // (the shared-device shape: 64-entry chunks, ~32 entries per bucket), one thread per bucket where buckets are longer (a proof alone)
    R.per_bucket = (uint64_t)CH * R.nkeys < Mub;
    R.bytes_wsums = (size_t)nmsm * W * MSM_POINT_BYTES;
    // a window's block: as many threads as it has segments, at most 512 for a proof alone (shortest chain) and 256 while the device is shared (fewest additions)
    if (!knobs.shared && knobs.window_quad) {
        // a proof alone: four lanes per point, a window spread over nblk blocks of 64 slots so that the launch is about one wave per SIMD (k_msm.cuh k_window_sums_quad);
        // per = segments per slot, nblk = blocks per window (at most 64: one slot each in the last block's second stage)
        const uint32_t nwin = nmsm * W, nsegpw = R.nsegpw;
        uint32_t lgper = 0;
        auto nblk_of = [&](uint32_t lp) { return std::max<uint32_t>(1u, nsegpw >> (6 + lp)); };
        while (nblk_of(lgper) > 1 && ((uint64_t)nwin * nblk_of(lgper) > knobs.window_quad_blocks || nblk_of(lgper) > 64)) lgper++;
        R.quad = true; R.lgper = lgper; R.window_blocks = nblk_of(lgper);
        R.bytes_wq_stage = (size_t)nwin * R.window_blocks * 2 * MSM_POINT_BYTES;
        if (nwin > MSM_TICKETS) throw std::logic_error("msm: too many windows for the ticket array");
    } else {
        R.window_threads = std::max<uint32_t>(64, std::min<uint32_t>(R.nsegpw, knobs.shared ? 256u : 512u));
    }
    if (R.bytes_wsums > MSM_WS_SLOT_BYTES) throw std::logic_error("msm: window sums exceed the host slot");
    return R;
}

}  // namespace bpg
