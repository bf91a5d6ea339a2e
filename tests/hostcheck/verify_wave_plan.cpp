// Stand-alone check of csrc/host/verify_wave_plan.hpp (built with -fsanitize=address,undefined by tests/test_verify_wave_host.py; no device, no preload):
// plan_verify_wave over N = 1, 8, 1024, 2^14; K = 1, 2, items-per-wave - 1 / exact / + 1, 1024; wave_mb = 0, 1, 512; 1 and 256 compute units; tails 0 and > 0.
//   - the regions of a wave are disjoint, 256-aligned, large enough for a full wave and sum to the total;
//   - waves x items-per-wave >= K, every wave holds at least one item, and the waves' items sum to K;
//   - chunks x items-per-chunk >= the wave's items, no chunk is empty, and the partial-sum region holds the chunks of EVERY wave;
//   - the bytes per item are the five vectors the issue names;
//   - the refusals, each with its exception type.
// Prints one line per wave_mb with the figures of the 1024-item plans, then "ok".
#include <cstdio>
#include <vector>
#include "../../bulletproofs_gadgets_amd/csrc/host/verify_wave_plan.hpp"

using namespace bpg;

static int fail(const char *what, uint64_t a = 0, uint64_t b = 0, uint64_t c = 0) { std::printf("FAIL %s (%llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b, (unsigned long long)c); return 1; }

static int check(uint64_t n, uint64_t m, uint64_t q, uint64_t N, uint64_t n_tail, uint64_t K, uint64_t wave_mb, uint32_t cus, uint64_t *plans) {
    const VerifyWavePlan P = plan_verify_wave(n, m, q, N, n_tail, K, wave_mb, cus);
    (*plans)++;
    if (P.item_bytes != 32 * ((3 * n + m) + N + (q + 2) + n_tail + (m + 2))) return fail("bytes per item", N, K);
    if (P.per_wave < 1 || P.per_wave > K) return fail("a wave holds 1 .. K items", N, K, P.per_wave);
    if (wave_mb == 0 && P.per_wave != 1) return fail("wave_mb = 0 is one item per wave", N, K, P.per_wave);
    if (wave_mb && P.per_wave > 1 && P.per_wave * P.item_bytes > (wave_mb << 20)) return fail("a wave of several items exceeds the budget", N, K, P.per_wave);
    if (wave_mb && P.per_wave < K && P.per_wave < VW_MAX_WAVE_ITEMS && (P.per_wave + 1) * P.item_bytes <= (wave_mb << 20)) return fail("a wave could hold one more item", N, K, P.per_wave);
    if (P.waves * P.per_wave < K || (P.waves - 1) * P.per_wave >= K) return fail("waves x items-per-wave covers K with no empty wave", N, K, P.waves);
    uint64_t sum = 0;
    for (uint64_t w = 0; w < P.waves; w++) {
        const uint64_t items = P.wave_items(w);
        const VerifyWaveChunks &C = P.wave_chunks(w);
        if (!items || items > P.per_wave) return fail("items of a wave", N, K, w);
        if (!C.chunks || !C.per_chunk || C.chunks * C.per_chunk < items) return fail("chunks x items-per-chunk covers the wave", N, K, w);
        if ((C.chunks - 1) * C.per_chunk >= items) return fail("an empty chunk", N, K, w);
        if (C.chunks > items) return fail("more chunks than items", N, K, w);
        const uint64_t bx = (N + 255) / 256;
        if (C.chunks > 1 && (uint64_t)(C.chunks - 1) * bx >= P.target_blocks + bx) return fail("more blocks than the target asks for", N, K, w);
        if (C.chunks < items && (uint64_t)C.chunks * bx * 2 < P.target_blocks) return fail("far fewer blocks than the target although items are left to split", N, K, w);
        if ((uint64_t)C.chunks * 2 * N * 32 > P.total - P.off_part) return fail("the partial sums of a wave do not fit their region", N, K, w);
        sum += items;
        if (w > 1 && w + 1 < P.waves) w = P.waves - 2;          // (the waves between the second and the last are the same as the first)
    }
    if (P.waves <= 3 && sum != K) return fail("the waves' items sum to K", N, K, sum);
    if (P.target_blocks != 4 * cus) return fail("block target", cus, P.target_blocks);
    // regions: [w | y | z | tail | part], each 256-aligned, in order, each as long as a full wave needs, nothing behind the last
    const size_t off[6] = {P.off_w, P.off_y, P.off_z, P.off_tail, P.off_part, P.total};
    const uint64_t need[5] = {P.per_wave * P.w_len * 32, P.per_wave * N * 32, P.per_wave * (q + 2) * 32, P.per_wave * n_tail * 32,
                              (uint64_t)(P.full.chunks > P.last.chunks ? P.full.chunks : P.last.chunks) * 2 * N * 32};
    if (off[0] != 0) return fail("the first region starts at 0");
    for (int r = 0; r < 5; r++) {
        if (off[r] % 256 || off[r + 1] % 256) return fail("region alignment", r, off[r]);
        if (off[r + 1] < off[r] || off[r + 1] - off[r] < need[r]) return fail("region too short or overlapping", r, off[r + 1] - off[r], need[r]);
        if (off[r + 1] - off[r] >= need[r] + 256) return fail("region longer than its rounding", r, off[r + 1] - off[r], need[r]);
    }
    if (P.ch_len != 7 + 2 * (uint64_t)P.lgN || (1ull << P.lgN) != N) return fail("challenge record", N, P.ch_len);
    if (P.bytes_ch != K * P.ch_len * 32 || P.bytes_small != K * (m + 2) * 32) return fail("per-call buffers", N, K);
    return 0;
}

template <class E, class F> static bool throws(F &&f) { try { f(); } catch (const E &) { return true; } catch (...) { return false; } return false; }

int main() {
    uint64_t plans = 0;
    struct Shape { uint64_t n, m, q, N; };
    const Shape shapes[] = {{1, 1, 2, 1}, {5, 2, 5, 8}, {8, 0, 0, 8}, {700, 3, 700, 1024}, {1024, 0, 2100, 1024}, {9000, 4, 20000, 1ull << 14}, {1ull << 14, 0, 1, 1ull << 14}};
    const uint64_t mbs[] = {0, 1, 512};
    const uint32_t cus[] = {1, 256};
    for (const Shape &s : shapes) for (uint64_t mb : mbs) for (uint32_t cu : cus) for (uint64_t tail : {(uint64_t)0, (uint64_t)1, (uint64_t)37}) {
        const uint64_t per = plan_verify_wave(s.n, s.m, s.q, s.N, tail, 1ull << 32, mb, cu).per_wave;       // what a wave holds when K does not bound it
        std::vector<uint64_t> Ks = {1, 2, 1024, per, per + 1};
        if (per > 1) Ks.push_back(per - 1);
        if (per > 2) { Ks.push_back(2 * per); Ks.push_back(2 * per + 1); }
        for (uint64_t K : Ks) if (check(s.n, s.m, s.q, s.N, tail, K, mb, cu, &plans)) return 1;
    }
    // the chunk rule alone, every item count around the targets
    for (uint64_t N : {(uint64_t)1, (uint64_t)8, (uint64_t)256, (uint64_t)257, (uint64_t)1024, (uint64_t)1 << 14}) for (uint32_t target : {1u, 4u, 7u, 1024u}) for (uint64_t items = 1; items <= 2100; items++) {
        const VerifyWaveChunks C = plan_verify_wave_chunks(N, items, target);
        if (!C.chunks || C.chunks * C.per_chunk < items || (C.chunks - 1) * C.per_chunk >= items) return fail("chunk rule", N, target, items);
    }
    // the figures the engine runs with on a 256-CU device
    for (uint64_t mb : mbs) {
        const VerifyWavePlan a = plan_verify_wave(56, 0, 113, 64, 0, 1024, mb, 256), b = plan_verify_wave(700, 3, 700, 1024, 0, 1024, mb, 256);
        std::printf("wave_mb %llu: N 64 K 1024: %llu waves of %llu, %u chunks of %llu | N 1024: %llu waves of %llu, %u chunks of %llu\n", (unsigned long long)mb,
                    (unsigned long long)a.waves, (unsigned long long)a.per_wave, a.full.chunks, (unsigned long long)a.full.per_chunk, (unsigned long long)b.waves,
                    (unsigned long long)b.per_wave, b.full.chunks, (unsigned long long)b.full.per_chunk);
    }
    // the refusals, each with its type: the caller's count (invalid_argument), sizes beyond 64 bits (length_error), shapes no circuit has (logic_error, not one of the others)
    auto plain_logic = [](auto &&f) { try { f(); } catch (const std::invalid_argument &) { return false; } catch (const std::length_error &) { return false; } catch (const std::logic_error &) { return true; } catch (...) {} return false; };
    if (!throws<std::invalid_argument>([] { plan_verify_wave(8, 0, 0, 8, 0, (1ull << 32) + 1, 512, 256); })) return fail("count above 2^32 is an invalid_argument");
    if (throws<std::invalid_argument>([] { plan_verify_wave(8, 0, 0, 8, 0, 1ull << 32, 512, 256); })) return fail("count 2^32 is served");
    if (!throws<std::length_error>([] { plan_verify_wave(8, ~0ull - 8, 0, 8, 0, 1, 512, 256); })) return fail("3 n + m beyond 64 bits is a length_error");
    if (!throws<std::length_error>([] { plan_verify_wave(8, 0, ~0ull - 1, 8, 0, 1, 512, 256); })) return fail("q + 2 beyond 64 bits is a length_error");
    if (!throws<std::length_error>([] { plan_verify_wave(8, 0, 1ull << 60, 8, 0, 1, 512, 256); })) return fail("bytes per item beyond 64 bits is a length_error");
    if (!throws<std::length_error>([] { plan_verify_wave(8, 0, 0, 8, 1ull << 60, 2, 512, 256); })) return fail("tail bytes beyond 64 bits is a length_error");
    if (!throws<std::length_error>([] { plan_verify_wave(8, 0, 1ull << 50, 8, 0, 1ull << 32, 1ull << 44, 256); })) return fail("wave budget beyond 64 bits is a length_error");
    if (!plain_logic([] { plan_verify_wave(8, 0, 0, 8, 0, 0, 512, 256); })) return fail("no item is a logic_error");
    if (!plain_logic([] { plan_verify_wave(0, 2, 2, 1, 0, 1, 512, 256); })) return fail("n = 0 is a logic_error");
    if (!plain_logic([] { plan_verify_wave(5, 0, 0, 6, 0, 1, 512, 256); })) return fail("N not a power of two is a logic_error");
    if (!plain_logic([] { plan_verify_wave(9, 0, 0, 8, 0, 1, 512, 256); })) return fail("N below n is a logic_error");
    if (!plain_logic([] { plan_verify_wave(8, 0, 0, 8, 0, 1, 512, 0); })) return fail("no compute unit is a logic_error");
    std::printf("plans %llu\nok\n", (unsigned long long)plans);
    return 0;
}
