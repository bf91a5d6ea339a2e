// TEST HARNESS, stand-alone: the per-lane arithmetic of lockstep verification (csrc/hip/k_vwave.cuh, the BPG_HD half) compiled for the host.
// tests/test_verify_wave_host.py builds it with -fsanitize=address,undefined, hands it one item as hex scalars and compares what it prints with the integer
// model of tests/verify_wave_cases.py.
//   argv: lgN n, then the challenge record (7 + 2 lgN scalars: y^-1, z, x, u, a, b, rho, u_k, u_k^-1), then w_L, w_R, w_O (n each), then for the tail:
//         one standing scalar, one parameter value, one coefficient and one input value (the last three any 256-bit value)
//   out:  "y i hex" for the powers of y^-1 as the threads of k_vw_exp walk them (T = 4), "g i hex" and "h i hex" for the rho-weighted lane results,
//         "s i hex" for s_i, "tail j hex" for the four cases of a tail entry, then "ok"
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_vwave.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace bpg;

static void words_of(const char *hex, uint32_t w[8]) {         // 64 hex digits, little-endian bytes
    if (std::strlen(hex) != 64) { std::printf("FAILED: a scalar is 64 hex digits\n"); std::exit(1); }
    uint8_t b[32];
    for (int i = 0; i < 32; i++) { unsigned v; std::sscanf(hex + 2 * i, "%2x", &v); b[i] = (uint8_t)v; }
    std::memcpy(w, b, 32);
}
static scm mont(const char *hex) { uint32_t w[8]; words_of(hex, w); return sc_from_words(w); }
static void print(const char *what, unsigned i, const scm &x) {
    uint32_t w[8]; sc_to_words(w, x);
    uint8_t b[32]; std::memcpy(b, w, 32);
    std::printf("%s %u ", what, i);
    for (int k = 0; k < 32; k++) std::printf("%02x", b[k]);
    std::printf("\n");
}

int main(int argc, char **argv) {
    if (argc < 3) return 1;
    const uint32_t lgN = (uint32_t)std::atoi(argv[1]), n = (uint32_t)std::atoi(argv[2]), N = 1u << lgN, ch_len = VW_CH_FIXED + 2 * lgN;
    if ((uint32_t)argc != 3 + ch_len + 3 * n + 4 || n > N || n == 0) { std::printf("FAILED: argument count\n"); return 1; }
    std::vector<scm> ch(ch_len), w(3 * n);
    for (uint32_t k = 0; k < ch_len; k++) ch[k] = mont(argv[3 + k]);
    for (uint32_t k = 0; k < 3 * n; k++) w[k] = mont(argv[3 + ch_len + k]);
    // the power table as the threads of k_vw_exp fill it: thread t walks t, t + T, ..
    std::vector<scm> ypow(N);
    const uint32_t lgT = lgN < 2 ? lgN : 2, T = 1u << lgT;
    for (uint32_t t = 0; t < T; t++) {
        scm cur, step;
        vw_pow_start(ch[VW_YINV], t, lgT, cur, step);
        for (uint32_t i = t; i < N; i += T) { ypow[i] = cur; cur = sc_mont_mul(cur, step); }
    }
    for (uint32_t i = 0; i < N; i++) print("y", i, ypow[i]);
    for (uint32_t i = 0; i < N; i++) {
        scm s_i, s_rev, g, h;
        vw_s_pair(ch.data() + VW_CH_FIXED, ch.data() + VW_CH_FIXED + lgN, lgN, i, s_i, s_rev);
        const bool real = i < n;
        const scm zero = sc_zero();
        vw_weighted_gh(ch.data(), real, ypow[i], real ? w[i] : zero, real ? w[n + i] : zero, real ? w[2 * n + i] : zero, s_i, s_rev, g, h);
        print("s", i, s_i); print("g", i, g); print("h", i, h);
    }
    // a tail of one parameter slot and one derived slot (input 0 times coefficient 0 of the shared table)
    const char *const *t4 = argv + 3 + ch_len + 3 * n;
    const scm standing[2] = {mont(t4[0]), mont(t4[0])}, coef[1] = {mont(t4[2])};
    uint32_t raw[16]; words_of(t4[1], raw); words_of(t4[3], raw + 8);
    const uint32_t slots[2] = {0, 0};
    print("tail", 0, vw_tail_entry(0, VW_HAS_PARAMS | VW_HAS_INPUTS, 1, raw, slots, coef, standing));
    print("tail", 1, vw_tail_entry(1, VW_HAS_PARAMS | VW_HAS_INPUTS, 1, raw, slots, coef, standing));
    print("tail", 2, vw_tail_entry(0, VW_HAS_INPUTS, 1, raw, slots, coef, standing));
    print("tail", 3, vw_tail_entry(1, VW_HAS_PARAMS, 1, raw, slots, coef, standing));
    std::printf("ok\n");
    return 0;
}
