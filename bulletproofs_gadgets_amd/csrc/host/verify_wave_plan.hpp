// What one lockstep verification of K proofs of ONE resident circuit lays out and launches (Engine::verify_resident_batch, hip/k_vwave.cuh), decided
// before anything is sized or launched: bytes per item, items per wave, waves, the chunks of the accumulation kernel and the regions of a wave.
// plan_verify_wave() is a pure function of the circuit's sizes, the item count and two knobs - no HIP, no allocation - so
// tests/hostcheck/verify_wave_plan.cpp checks it on the CPU; the engine sizes its buffers and launches from the value it returns, and the test hook
// Engine::test_verify_wave_scalars prints that same value as its evidence.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <stdexcept>

namespace bpg {

constexpr uint64_t VW_SCALAR_BYTES = 32;            // sizeof(scm)
constexpr uint32_t VW_LANES = 256;                  // lanes of a block of every k_vw_* kernel
// Blocks of k_vw_scalars the plan aims at per compute unit.  NOBODY HAS MEASURED THIS: 4 is where the bucket sweep keeps its resident blocks
// (Engine::Impl::sweep_blocks_resident), taken over as a starting point.  tools/diag/verify_wave.py records what it gives beside every figure.
constexpr uint32_t VW_BLOCKS_PER_CU = 4;
constexpr uint64_t VW_MAX_WAVE_ITEMS = 65535;       // the item is blockIdx.z of k_vw_exp: a grid's z extent

// The chunks of one wave: k_vw_scalars runs a lane per generator index i, grid (cdiv(N, 256), chunks); the lanes of chunk c walk items
// [c * per_chunk, min(items, (c + 1) * per_chunk)) of the wave and write ONE partial sum per i.  At N = 8 .. 1024 a launch of one lane per i is
// one to four blocks, each walking every item of the wave serially, so the items are split until cdiv(N, 256) * chunks reaches `target_blocks`
// (or every item has a chunk of its own).  No chunk is empty: chunks = cdiv(items, per_chunk).
struct VerifyWaveChunks { uint32_t chunks; uint64_t per_chunk; };
inline VerifyWaveChunks plan_verify_wave_chunks(uint64_t N, uint64_t items, uint32_t target_blocks) {
    if (!N || !items || !target_blocks) throw std::logic_error("verify wave: a wave has items, lanes and a block target");
    const uint64_t bx = (N + VW_LANES - 1) / VW_LANES;
    const uint64_t want = std::max<uint64_t>(1, std::min<uint64_t>(items, (target_blocks + bx - 1) / bx));
    VerifyWaveChunks C;
    C.per_chunk = (items + want - 1) / want;
    C.chunks = (uint32_t)((items + C.per_chunk - 1) / C.per_chunk);
    return C;
}

struct VerifyWavePlan {
    uint64_t n, m, q, N, n_tail, count;
    uint32_t lgN, target_blocks;
    // scalars of one item in each region of a wave, and the bytes of all of them plus its small slot (what the wave size is cut by)
    uint64_t w_len, y_len, z_len, tail_len, small_len, item_bytes;
    uint64_t per_wave, waves;                   // items of a full wave (the last one holds count - (waves - 1) * per_wave), number of waves
    VerifyWaveChunks full, last;                // chunks of a full wave and of the last one
    // regions of a wave, item-major (vec[k * len + i]); part = [chunk][g | h][N] partial sums of k_vw_scalars.  Offsets are multiples of 256
    size_t off_w, off_y, off_z, off_tail, off_part, total;
    // per call, not per wave: challenge records ((7 + 2 lg N) scalars per item), small slots ([w_V (m) | w_c | delta] per item)
    uint64_t ch_len, bytes_ch, bytes_small;
    uint64_t wave_items(uint64_t w) const { return w + 1 < waves ? per_wave : count - (waves - 1) * per_wave; }
    const VerifyWaveChunks &wave_chunks(uint64_t w) const { return w + 1 < waves ? full : last; }
};

// n, m, q: the circuit's; N = n padded to a power of two (n > 0); n_tail = n_params + n_slots when an item brings constants of its own, else 0;
// wave_mb: BPG_BATCH_WAVE_MB as the proving waves read it (0: one item per wave); cu_count: compute units of the device.
// Refused: count above 2^32 (std::invalid_argument: the caller's), a size that does not fit 64 bits (std::length_error), a shape no circuit has
// (std::logic_error) - before anything is allocated.
inline VerifyWavePlan plan_verify_wave(uint64_t n, uint64_t m, uint64_t q, uint64_t N, uint64_t n_tail, uint64_t count, uint64_t wave_mb, uint32_t cu_count) {
    auto al256 = [](uint64_t x) { return (x + 255) & ~(uint64_t)255; };
    auto add = [](uint64_t a, uint64_t b) { if (a > ~(uint64_t)0 - b) throw std::length_error("verify wave: a size does not fit 64 bits"); return a + b; };
    auto mul = [](uint64_t a, uint64_t b) { if (a && b > ~(uint64_t)0 / a) throw std::length_error("verify wave: a size does not fit 64 bits"); return a * b; };
    if (count > (1ull << 32)) throw std::invalid_argument("verify wave: more than 2^32 items in one call");
    if (!count) throw std::logic_error("verify wave: no item");
    if (!n || N < n || (N & (N - 1)) || N > (1ull << 32)) throw std::logic_error("verify wave: N is n > 0 padded to a power of two, at most 2^32");
    if (!cu_count) throw std::logic_error("verify wave: a device has compute units");
    VerifyWavePlan P{};
    P.n = n; P.m = m; P.q = q; P.N = N; P.n_tail = n_tail; P.count = count;
    while ((1ull << P.lgN) < N) P.lgN++;
    P.target_blocks = (uint32_t)std::min<uint64_t>(mul(cu_count, VW_BLOCKS_PER_CU), 1u << 30);
    P.w_len = add(mul(3, n), m); P.y_len = N; P.z_len = add(q, 2); P.tail_len = n_tail; P.small_len = add(m, 2);
    const uint64_t scalars = add(add(add(P.w_len, P.y_len), add(P.z_len, P.tail_len)), P.small_len);
    P.item_bytes = mul(scalars, VW_SCALAR_BYTES);
    const uint64_t budget = mul(wave_mb, 1ull << 20);
    P.per_wave = std::min<uint64_t>(std::min<uint64_t>(count, VW_MAX_WAVE_ITEMS), std::max<uint64_t>(1, budget / P.item_bytes));
    P.waves = (count + P.per_wave - 1) / P.per_wave;
    P.full = plan_verify_wave_chunks(N, P.per_wave, P.target_blocks);
    P.last = plan_verify_wave_chunks(N, P.wave_items(P.waves - 1), P.target_blocks);
    const uint64_t K = P.per_wave;
    uint64_t off = 0;
    auto region = [&](uint64_t len) { const uint64_t at = off; off = add(off, al256(mul(mul(K, len), VW_SCALAR_BYTES))); return at; };
    P.off_w = (size_t)region(P.w_len); P.off_y = (size_t)region(P.y_len); P.off_z = (size_t)region(P.z_len); P.off_tail = (size_t)region(P.tail_len);
    // (the last wave can take MORE chunks than a full one: 10 items at 6 wanted are 5 chunks of 2, 6 items are 6 chunks of 1)
    P.off_part = (size_t)off; off = add(off, al256(mul(mul(mul(std::max(P.full.chunks, P.last.chunks), 2), N), VW_SCALAR_BYTES)));
    P.total = (size_t)off;
    if ((uint64_t)P.total != off) throw std::length_error("verify wave: a size does not fit the address space");
    P.ch_len = 7 + 2 * (uint64_t)P.lgN;
    P.bytes_ch = mul(mul(count, P.ch_len), VW_SCALAR_BYTES);
    P.bytes_small = mul(mul(count, P.small_len), VW_SCALAR_BYTES);
    return P;
}

}  // namespace bpg
