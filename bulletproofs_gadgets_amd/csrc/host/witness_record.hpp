// The packed witness program of a circuit template: what host/template.hpp (pack_witness_program) writes and hip/k_witness.cuh (witness_eval_segment)
// reads.  One record per multiplier, in multiplier order:
//   word 0: number of left terms; word 1: number of right terms, or WIT_SAME_AS_LEFT alone when the right list IS the left list (no right terms follow);
//   then two words per term: the packed variable (kind << 29 | index) and coefficient class << WIT_CLASS_SHIFT | index into the coefficient table.
// Classes: +1 and -1 need no product (as in Prover::eval); a zero coefficient adds nothing and its term is dropped by the packer.
// A HINTED multiplier (bpg_witness_hints, kind BIT_PAIR) is no product: word 1 = WIT_HINT_BIT_PAIR | bit index (low 8 bits), word 0 = number of terms of the
// SOURCE, which follow; a_L = 1 - b, a_R = b, a_O = 0 with b that bit of the canonical value (mod l) of the source.  WIT_HINT_SAME_SOURCE beside it: the
// source is the previous record's (a hinted record of the same segment) - word 0 is 0, no terms follow, and the reader still holds the reduced value.
// The flags leave 29 bits for a right-term count.
// A term that names a CHECKPOINTED variable (bpg_witness_checkpoints) carries the kind WIT_KIND_CHECKPOINT and, as its index, the position in the checkpoint
// list: the reader takes the value the caller handed to assign.  The kind exists in this stream only; the variable kinds of include/bpg.h stay 0..4.
// A term that names a PUBLIC INPUT of the proof (Variable::Input, bpg_r1cs_upload_template_inputs) carries the kind WIT_KIND_INPUT and the input's index: the
// reader takes the value the caller handed to assign, as it does for a checkpoint.  This kind too exists in this stream only (the instance says 5, BPG_VAR_INPUT).
// A GATED term (Variable::Gated, bpg_r1cs_upload_template_gated: coefficient * input p * variable) takes TWO term slots, and both count in word 0 / word 1 of
// its record: the first holds the packed variable (checkpoint kind included) and WIT_COEF_GATED << WIT_CLASS_SHIFT | p - a class no plain term carries, since the
// packer drops zero coefficients - the second an unused word and the term's own class << WIT_CLASS_SHIFT | coefficient index.  A gated term whose coefficient
// is zero is dropped like any other; one whose INPUT happens to be zero is a term.  A stream without gated terms is bit for bit what it was.
#pragma once
#include <cstdint>

namespace bpg {

constexpr uint32_t WIT_SAME_AS_LEFT = 1u << 31, WIT_HINT_BIT_PAIR = 1u << 30, WIT_HINT_SAME_SOURCE = 1u << 29;
constexpr uint32_t WIT_RIGHT_COUNT_MASK = WIT_HINT_SAME_SOURCE - 1u, WIT_HINT_ARG_MASK = 0xffu;
constexpr uint32_t WIT_CLASS_SHIFT = 30, WIT_COEF_INDEX_MASK = (1u << WIT_CLASS_SHIFT) - 1u;
constexpr uint32_t WIT_COEF_GENERAL = 0, WIT_COEF_PLUS_ONE = 1, WIT_COEF_MINUS_ONE = 2, WIT_COEF_GATED = 3;
constexpr uint32_t WIT_KIND_CHECKPOINT = 5, WIT_KIND_INPUT = 6;

}  // namespace bpg
