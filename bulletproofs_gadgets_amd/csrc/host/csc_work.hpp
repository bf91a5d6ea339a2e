// The workspace of the CSR -> CSC transposition (engine.hip Impl::transpose_csr; hip/k_scalars.cuh k_csc_*), sized in ONE place: Engine::upload (one
// instance) and WaveLayout (the block-diagonal instance of a lockstep wave) both ask here.  Pure host code: tests/hostcheck compiles it.
//
// nvar = 3 * multipliers + committed values (the variable columns; the constant terms are column nvar), q = rows.  What writes where, in launch order:
//   memset            counts[0, nvar], rowconst[0, q]
//   k_csc_count       counts[0, nvar) (atomics), rowconst[0, q)
//   scan 1, nvar keys k_scan_blocksums: bsum[0, ceil(nvar / SCAN_CHUNK)); k_scan_apply: starts[0, nvar] (the total at nvar), cursor[0, nvar)
//   scan 2, q keys    k_scan_blocksums: bsum[0, ceil(q / SCAN_CHUNK)); k_scan_apply: rowconst_start[0, q] (the total at q) and, as the running positions it
//                     has no use for, q words of SCRATCH - for which transpose_csr hands it `counts`, dead by then: counts[0, q)
//   k_csc_colptr      reads starts[0, nvar], rowconst_start[q]
//   k_csc_fill        cursor[0, nvar) (atomics); reads rowconst_start[0, q), starts[nvar]
// So `counts` holds max(nvar + 1, q) words: the SECOND scan decides when the matrix is tall (q > nvar + 1).  A `counts` of nvar + 2 words lets that scan
// run on into whatever lies behind it - in a wave's slab `starts` and then `cursor`, which hold the first scan's results and are read next.
// A k_scan_apply block reads its whole chunk before it writes (a barrier lies between), so scan 2 may not use rowconst itself as scratch when q takes more
// than one block: a later block could read what an earlier one wrote.  `counts` is the only buffer that is dead and not being read.
#pragma once
#include <algorithm>
#include <cstdint>

namespace bpg {

constexpr uint64_t CSC_SCAN_CHUNK = 2048;        // keys per block of k_scan_blocksums / k_scan_apply (host/msm_plan.hpp SCAN_CHUNK: engine.hip asserts they agree)

struct CscWorkWords { uint64_t counts, starts, cursor, rowconst, rowconst_start, bsum; };      // 32-bit words each

// the highest word each buffer sees written (or zeroed), plus one: the rule above, term by term
constexpr CscWorkWords csc_work_written(uint64_t nvar, uint64_t q) {
    const uint64_t nb1 = ((nvar ? nvar : 1) + CSC_SCAN_CHUNK - 1) / CSC_SCAN_CHUNK, nb2 = ((q ? q : 1) + CSC_SCAN_CHUNK - 1) / CSC_SCAN_CHUNK;
    return CscWorkWords{std::max(nvar + 1, q), nvar + 1, nvar, q + 1, q + 1, std::max(nb1, nb2)};
}
// what upload() and WaveLayout allocate: one spare word each, as the buffers always had
constexpr CscWorkWords csc_work_words(uint64_t nvar, uint64_t q) {
    const CscWorkWords w = csc_work_written(nvar, q);
    return CscWorkWords{w.counts + 1, w.starts + 1, w.cursor + 2, w.rowconst + 1, w.rowconst_start + 1, w.bsum + 2};
}

}  // namespace bpg
