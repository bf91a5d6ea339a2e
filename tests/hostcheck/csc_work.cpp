// TEST HARNESS, stand-alone: the size rule of the transposition workspace (csrc/host/csc_work.hpp) through the host compiler.  tests/test_shape_cases_host.py
// builds it with -fsanitize=address,undefined and runs it on the (nvar, q) pairs of tests/shape_cases.py:
//     csc_work RULE nvar:q [nvar:q ...]
// For every pair the launches of Impl::transpose_csr are replayed in order - the memsets, k_csc_count, both scans (k_scan_blocksums and k_scan_apply by their
// own index arithmetic: blocks of SCAN_CHUNK keys, eight keys a thread, the total behind the last key), k_csc_colptr's and k_csc_fill's reads - and every word
// they touch is recorded against the buffer the launch was handed.  RULE says how the six buffers were laid out:
//     rule       csc_work_words(nvar, q) words each, every buffer a heap block of EXACTLY that size (the replay really writes: ASan is the second judge)
//     old-wave   what the lockstep wave laid out before the rule existed: counts, starts, cursor of nvar + 2 words, rowconst, rowconst_start of q + 2, each
//                rounded up to 256 bytes, back to back in one slab.  Nothing is written here; the replay only compares extents
// Per pair one line "nvar q ok" or "nvar q OVERRUN buffer words>capacity"; the exit status is the number of pairs that overran.  The last line is "ok" when
// none did.  Under `rule` the highest word written is also compared with csc_work_written(), so the comment in the header cannot drift from the replay.
#include "../../bulletproofs_gadgets_amd/csrc/host/csc_work.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
using namespace bpg;

enum Buf { COUNTS, STARTS, CURSOR, ROWCONST, ROWCONST_START, BSUM, NBUF };
static const char *const kName[NBUF] = {"counts", "starts", "cursor", "rowconst", "rowconst_start", "bsum"};

struct Work {
    uint64_t cap[NBUF];                                   // words the layout gives each buffer
    std::unique_ptr<uint32_t[]> mem[NBUF];                // rule: the buffers themselves
    uint64_t high[NBUF] = {0, 0, 0, 0, 0, 0};             // highest word touched, plus one
    void touch(Buf b, uint64_t first, uint64_t count, bool write) {
        if (!count) return;
        if (first + count > high[b]) high[b] = first + count;
        if (mem[b] && first + count <= cap[b] && write) for (uint64_t k = first; k < first + count; k++) mem[b][k] = (uint32_t)k;
        if (mem[b] && first + count <= cap[b] && !write) { volatile uint32_t sink = 0; for (uint64_t k = first; k < first + count; k++) sink = sink + mem[b][k]; }
    }
};

// k_scan_blocksums + k_scan_apply over nkeys keys: counts in, starts and cursor out
static void scan(Work &W, Buf counts, uint64_t nkeys, Buf starts, Buf cursor) {
    const uint64_t nb = ((nkeys ? nkeys : 1) + CSC_SCAN_CHUNK - 1) / CSC_SCAN_CHUNK;
    for (uint64_t b = 0; b < nb; b++) {
        for (uint64_t k = 0; k < CSC_SCAN_CHUNK; k++) if (b * CSC_SCAN_CHUNK + k < nkeys) W.touch(counts, b * CSC_SCAN_CHUNK + k, 1, false);
        W.touch(BSUM, b, 1, true);
    }
    for (uint64_t b = 0; b < nb; b++) {
        for (uint64_t p = 0; p < b; p++) W.touch(BSUM, p, 1, false);
        for (uint64_t t = 0; t < 256; t++)
            for (uint64_t k = 0; k < 8; k++) {
                const uint64_t idx = b * CSC_SCAN_CHUNK + t * 8 + k;
                if (idx < nkeys) { W.touch(counts, idx, 1, false); W.touch(starts, idx, 1, true); W.touch(cursor, idx, 1, true); }
            }
        if (b == nb - 1) W.touch(starts, nkeys, 1, true);
    }
}

static void transpose(Work &W, uint64_t nvar, uint64_t q) {
    W.touch(COUNTS, 0, nvar + 1, true); W.touch(ROWCONST, 0, q + 1, true);            // the memsets
    W.touch(COUNTS, 0, nvar, true); W.touch(ROWCONST, 0, q, true);                    // k_csc_count
    scan(W, COUNTS, nvar, STARTS, CURSOR);
    scan(W, ROWCONST, q, ROWCONST_START, COUNTS /* scratch */);
    W.touch(STARTS, 0, nvar + 1, false); W.touch(ROWCONST_START, q, 1, false);        // k_csc_colptr
    W.touch(CURSOR, 0, nvar, true); W.touch(ROWCONST_START, 0, q, false); W.touch(STARTS, nvar, 1, false);      // k_csc_fill
}

static uint64_t al256_words(uint64_t words) { return ((words * 4 + 255) & ~(uint64_t)255) / 4; }

int main(int argc, char **argv) {
    if (argc < 3) { std::printf("usage: csc_work rule|old-wave nvar:q ...\n"); return 255; }
    const bool rule = !std::strcmp(argv[1], "rule");
    if (!rule && std::strcmp(argv[1], "old-wave")) { std::printf("unknown rule %s\n", argv[1]); return 255; }
    int bad = 0;
    for (int a = 2; a < argc; a++) {
        char *end = nullptr;
        const uint64_t nvar = std::strtoull(argv[a], &end, 10);
        if (!end || *end != ':') { std::printf("bad pair %s\n", argv[a]); return 255; }
        const uint64_t q = std::strtoull(end + 1, &end, 10);
        if (*end) { std::printf("bad pair %s\n", argv[a]); return 255; }
        Work W;
        if (rule) {
            const CscWorkWords w = csc_work_words(nvar, q);
            const uint64_t caps[NBUF] = {w.counts, w.starts, w.cursor, w.rowconst, w.rowconst_start, w.bsum};
            for (int b = 0; b < NBUF; b++) { W.cap[b] = caps[b]; W.mem[b].reset(new uint32_t[caps[b]]); std::memset(W.mem[b].get(), 0, caps[b] * 4); }
        } else {
            const uint64_t nb = std::max((nvar + CSC_SCAN_CHUNK - 1) / CSC_SCAN_CHUNK, ((q ? q : 1) + CSC_SCAN_CHUNK - 1) / CSC_SCAN_CHUNK);
            const uint64_t caps[NBUF] = {al256_words(nvar + 2), al256_words(nvar + 2), al256_words(nvar + 2), al256_words(q + 2), al256_words(q + 2), al256_words(nb + 2)};
            for (int b = 0; b < NBUF; b++) W.cap[b] = caps[b];
        }
        transpose(W, nvar, q);
        std::string over;
        for (int b = 0; b < NBUF; b++) if (W.high[b] > W.cap[b]) over += std::string(" ") + kName[b] + " " + std::to_string(W.high[b]) + ">" + std::to_string(W.cap[b]);
        if (rule) {
            const CscWorkWords w = csc_work_written(nvar, q);
            const uint64_t said[NBUF] = {w.counts, w.starts, w.cursor, w.rowconst, w.rowconst_start, w.bsum};
            for (int b = 0; b < NBUF; b++) if (W.high[b] != said[b]) over += std::string(" ") + kName[b] + " written " + std::to_string(W.high[b]) + " not " + std::to_string(said[b]);
        }
        std::printf("%llu %llu %s%s\n", (unsigned long long)nvar, (unsigned long long)q, over.empty() ? "ok" : "OVERRUN", over.c_str());
        bad += !over.empty();
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad > 250 ? 250 : bad;
}
