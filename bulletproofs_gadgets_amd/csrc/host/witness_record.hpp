// The packed witness program of a circuit template: what host/template.hpp (pack_witness_program) writes and hip/k_witness.cuh (witness_eval_segment)
// reads.  One record per multiplier, in multiplier order:
//   word 0: number of left terms; word 1: number of right terms, or WIT_SAME_AS_LEFT alone when the right list IS the left list (no right terms follow);
//   then two words per term: the packed variable (kind << 29 | index) and coefficient class << WIT_CLASS_SHIFT | index into the coefficient table.
// Classes: +1 and -1 need no product (as in Prover::eval); a zero coefficient adds nothing and its term is dropped by the packer.
#pragma once
#include <cstdint>

namespace bpg {

constexpr uint32_t WIT_SAME_AS_LEFT = 1u << 31;
constexpr uint32_t WIT_CLASS_SHIFT = 30, WIT_COEF_INDEX_MASK = (1u << WIT_CLASS_SHIFT) - 1u;
constexpr uint32_t WIT_COEF_GENERAL = 0, WIT_COEF_PLUS_ONE = 1, WIT_COEF_MINUS_ONE = 2;

}  // namespace bpg
