// The error codes of the R1CS proof system (dalek R1CSError) and the padded circuit size they speak of: what the constraint-system builder (r1cs.hpp),
// the transcript script (fiat_shamir.hpp) and the engine share, without one pulling in the other.
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

namespace bpg {

enum class R1CSError { None = 0, InvalidGeneratorsLength = 1, FormatError = 2, VerificationError = 3, MissingAssignment = 5, GadgetError = 6 };
struct R1CSException : std::runtime_error {
    R1CSError code;
    R1CSException(R1CSError c, const std::string &m) : std::runtime_error(m), code(c) {}
};
// n multipliers padded to the power of two the generators and the inner-product argument work on (1 for n = 0), and its logarithm
inline uint32_t ceil_log2(uint64_t x) { uint32_t l = 0; while ((1ULL << l) < x) l++; return l; }
inline uint64_t padded_size(uint64_t n) { return 1ULL << ceil_log2(n); }
// hint: what an entry point adds to the message for its caller
inline void require_gens_capacity(uint64_t capacity, uint64_t n, const char *hint = "") {
    if (capacity < padded_size(n)) throw R1CSException(R1CSError::InvalidGeneratorsLength, std::string("generator capacity below padded circuit size") + hint);
}

}  // namespace bpg
