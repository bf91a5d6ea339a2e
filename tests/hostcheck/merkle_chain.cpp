// TEST HARNESS, stand-alone: compiles the device's MiMC permutation and Merkle node function (csrc/hip/k_mimc.cuh, the BPG_HD half) for the host and prints
// the chain of `levels` nodes above a leaf, each node over two copies of the one before - the tree of equal leaves of reference
// src/merkle_tree/merkle_tree_gadget.rs:476-503.  tests/test_merkle_host.py builds it with -fsanitize=address,undefined and compares the lines with the
// golden levels512_be.  Usage: merkle_chain <leaf, 64 hex digits big-endian> <levels>; one big-endian hex line per level.
#include "../../bulletproofs_gadgets_amd/csrc/hip/k_mimc.cuh"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
using namespace bpg;

static const uint64_t RC[BPG_MIMC_ROUNDS][4] = {
#include "../../bulletproofs_gadgets_amd/csrc/host/mimc_rc769.inc"
};

static int hexval(char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main(int argc, char **argv) {
    if (argc != 3 || std::strlen(argv[1]) != 64) { std::fprintf(stderr, "usage: merkle_chain <64 hex digits, big-endian> <levels>\n"); return 2; }
    uint8_t le[32];
    for (int i = 0; i < 32; i++) {
        const int hi = hexval(argv[1][2 * i]), lo = hexval(argv[1][2 * i + 1]);
        if (hi < 0 || lo < 0) { std::fprintf(stderr, "not a hex digit\n"); return 2; }
        le[31 - i] = (uint8_t)(hi * 16 + lo);
    }
    const int levels = std::atoi(argv[2]);
    std::vector<scm> rc(BPG_MIMC_ROUNDS);               // on the heap: a read past the table is the sanitizer's to see
    for (int i = 0; i < BPG_MIMC_ROUNDS; i++) { uint32_t w[8]; std::memcpy(w, RC[i], 32); rc[i] = sc_from_words(w); }
    uint32_t w[8]; std::memcpy(w, le, 32);
    scm h = sc_from_words(w);
    for (int l = 0; l < levels; l++) {
        h = mimc_node(h, h, rc.data());
        sc_to_words(w, h);
        uint8_t out[32]; std::memcpy(out, w, 32);
        for (int i = 31; i >= 0; i--) std::printf("%02x", out[i]);
        std::printf("\n");
    }
    return 0;
}
