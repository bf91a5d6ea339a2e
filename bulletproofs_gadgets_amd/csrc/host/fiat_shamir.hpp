// The Fiat-Shamir script of an R1CS proof (dalek r1cs/prover.rs, r1cs/verifier.rs, inner_product_proof.rs), written down ONCE.  Prover and verifier
// call the same steps in the same order, so a label or an ordering cannot differ between the role that makes a proof and the role that checks it:
//     "m" | fs_commitments -> y, z | fs_poly_commitments -> u, x | fs_poly_scalars -> w | innerproduct_domain_sep | fs_ipa_round -> u_k, lg N times
// Beside them: the byte layout of a proof as every proving path writes it (proof_*, poly_*), and verify_replay, which reads it back.  No device here.
#pragma once
#include <cstring>
#include <vector>
#include "merlin.hpp"
#include "scalar.hpp"
#include "r1cs_error.hpp"      // R1CSError, padded_size

namespace bpg {

static const uint8_t kIdentity[32] = {0};      // compressed identity

// ---- the transcript steps (flags: 1 = compact one-phase proof, 2 = no one-phase domain separator)
// phase1: A_I1, A_O1, S1 side by side; phase2: A_I2, A_O2, S2 as the proof holds them (the verifier of a two-phase dialect), or nullptr for an empty
// second phase: three identities (the prover, and the verifier of a compact proof)
inline void fs_commitments(Transcript &T, const uint8_t phase1[96], const uint8_t *phase2, uint32_t flags, Scalar &y, Scalar &z) {
    T.append_point("A_I1", phase1); T.append_point("A_O1", phase1 + 32); T.append_point("S1", phase1 + 64);
    if (!(flags & 2u)) T.r1cs_1phase_domain_sep();
    T.append_point("A_I2", phase2 ? phase2 : kIdentity); T.append_point("A_O2", phase2 ? phase2 + 32 : kIdentity); T.append_point("S2", phase2 ? phase2 + 64 : kIdentity);
    y = T.challenge_scalar("y"); z = T.challenge_scalar("z");
}
// pT: the encodings of T_1, T_3, T_4, T_5, T_6, side by side.  ok(point): the verifier's validate_and_append_point - a point it refuses ends the step
// BEFORE that point is appended, the earlier ones are in the transcript (false); the prover refuses nothing
template <class Ok = bool (*)(const uint8_t *)>
inline bool fs_poly_commitments(Transcript &T, const uint8_t pT[160], Scalar &u, Scalar &x, Ok ok = [](const uint8_t *) { return true; }) {
    static const char *const labels[5] = {"T_1", "T_3", "T_4", "T_5", "T_6"};
    for (int k = 0; k < 5; k++) { if (!ok(pT + 32 * k)) return false; T.append_point(labels[k], pT + 32 * k); }
    u = T.challenge_scalar("u"); x = T.challenge_scalar("x");
    return true;
}
inline Scalar fs_poly_scalars(Transcript &T, const Scalar &tx, const Scalar &txb, const Scalar &eb) {
    T.append_scalar("t_x", tx); T.append_scalar("t_x_blinding", txb); T.append_scalar("e_blinding", eb);
    return T.challenge_scalar("w");
}
inline Scalar fs_ipa_round(Transcript &T, const uint8_t L[32], const uint8_t R[32]) {
    T.append_point("L", L); T.append_point("R", R);
    return T.challenge_scalar("u");
}

// ---- the prover's side of the proof bytes: [0 if compact] A_I1 A_O1 S1 [96 zero bytes unless compact] T_1 T_3..T_6 t_x t_x_blinding e_blinding (L_k R_k)* a b
inline void proof_open(std::vector<uint8_t> &proof, uint32_t lgN, uint32_t flags, const uint8_t pts[96]) {
    proof.clear(); proof.reserve(14 * 32 + (2 * lgN + 2) * 32 + 1);
    if (flags & 1u) proof.push_back(0);
    proof.insert(proof.end(), pts, pts + 96);
    if (!(flags & 1u)) proof.insert(proof.end(), 96, 0);
}
// tau_1, tau_3..tau_6 drawn into tb[] in that order, then the five (value, blinding) pairs of T_1, T_3..T_6 as Pedersen inputs (vv, rr: 160 bytes each)
inline void poly_commit_inputs(TranscriptRng &rng, const Scalar t[7], Scalar tb[7], uint8_t *vv, uint8_t *rr) {
    static const int idx[5] = {1, 3, 4, 5, 6};
    for (int k = 0; k < 5; k++) tb[idx[k]] = rng.random_scalar();
    for (int k = 0; k < 5; k++) { t[idx[k]].to_bytes(vv + 32 * k); tb[idx[k]].to_bytes(rr + 32 * k); }
}
// t(x), its blinding (tb[2] = <w_V, v_blinding> is filled in here; wV(j): the flattened weight of committed variable j) and e_blinding
struct PolyAtX { Scalar tx, txb, eb; };
template <class WV> inline PolyAtX poly_at_x(const Scalar t[7], Scalar tb[7], WV wV, const std::vector<Scalar> &v_blinding, const Scalar &ib, const Scalar &ob, const Scalar &sb, const Scalar &x) {
    for (uint64_t j = 0; j < v_blinding.size(); j++) tb[2] += wV(j) * v_blinding[j];
    PolyAtX p;
    for (int k = 6; k >= 1; k--) { p.tx = (p.tx + t[k]) * x; p.txb = (p.txb + tb[k]) * x; }
    p.eb = x * (ib + x * (ob + x * sb));
    return p;
}
inline void proof_poly_scalars(std::vector<uint8_t> &proof, const PolyAtX &p) {
    uint8_t b[96]; p.tx.to_bytes(b); p.txb.to_bytes(b + 32); p.eb.to_bytes(b + 64);
    proof.insert(proof.end(), b, b + 96);
}

// ---- the verifier's side
// R1CSProof::from_bytes and the Fiat-Shamir replay of Verifier::verify on the host: everything verify() and verify_batch() decide before device work
struct VerifyReplay {
    uint64_t n = 0, m = 0, N = 1;
    uint32_t lgN = 0;
    const uint8_t *pA[6] = {}, *pT[5] = {}, *pLR = nullptr;
    Scalar tx, txb, eb, ipa, ipb, y, z, u_ch, x, w, r, yinv;
    std::vector<Scalar> uk, ukinv;
    uint32_t npts() const { return (uint32_t)(6 + m + 5 + 2 * lgN); }
};
inline R1CSError verify_replay(uint64_t n, uint64_t m, uint64_t gens_cap, Transcript &T, const uint8_t *proof, size_t proof_len, const uint8_t seed[32],
                               uint32_t flags, VerifyReplay &R) {
    const uint64_t N = padded_size(n);
    const uint32_t lgN = ceil_log2(N);
    R.n = n; R.m = m; R.N = N; R.lgN = lgN;
    const bool compact = flags & 1u;
    const size_t need = (compact ? 1 + 11 * 32 : 14 * 32) + (2 * (size_t)lgN + 2) * 32;
    if (proof_len != need) return R1CSError::FormatError;
    if (gens_cap < N) return R1CSError::InvalidGeneratorsLength;
    if (lgN > 32) return R1CSError::FormatError;
    const uint8_t *in = proof;
    if (compact) { if (*in++ != 0) return R1CSError::FormatError; }
    const uint8_t **pA = R.pA, **pT = R.pT;
    pA[0] = in; pA[1] = in + 32; pA[2] = in + 64; pA[3] = pA[4] = pA[5] = kIdentity; in += 96;
    if (!compact) { pA[3] = in; pA[4] = in + 32; pA[5] = in + 64; in += 96; }
    for (int k = 0; k < 5; k++) { pT[k] = in; in += 32; }
    Scalar sc5[5];                                   // t_x, t_x_blinding, e_blinding, a, b : must be canonical (R1CSProof::from_bytes)
    const uint8_t *ps[5] = {in, in + 32, in + 64, proof + proof_len - 64, proof + proof_len - 32};
    for (int k = 0; k < 5; k++) { std::memcpy(sc5[k].w, ps[k], 32); if (!sc5[k].is_canonical()) return R1CSError::FormatError; }
    in += 96;
    R.pLR = in;
    R.tx = sc5[0]; R.txb = sc5[1]; R.eb = sc5[2]; R.ipa = sc5[3]; R.ipb = sc5[4];
    auto is_ident = [](const uint8_t *p) { return std::memcmp(p, kIdentity, 32) == 0; };

    T.append_u64("m", m);
    if (is_ident(pA[0]) || is_ident(pA[1]) || is_ident(pA[2])) return R1CSError::VerificationError;      // validate_and_append_point
    fs_commitments(T, pA[0], compact ? nullptr : pA[3], flags, R.y, R.z);
    if (!fs_poly_commitments(T, pT[0], R.u_ch, R.x, [&](const uint8_t *p) { return !is_ident(p); })) return R1CSError::VerificationError;
    R.w = fs_poly_scalars(T, R.tx, R.txb, R.eb);
    T.innerproduct_domain_sep(N);
    R.uk.assign(lgN, Scalar()); R.ukinv.assign(lgN, Scalar());
    bool lr_ident = false;
    for (uint32_t k = 0; k < lgN; k++) {
        const uint8_t *Lp = R.pLR + 64 * k, *Rp = Lp + 32;
        lr_ident |= is_ident(Lp) || is_ident(Rp);
        R.uk[k] = fs_ipa_round(T, Lp, Rp); R.ukinv[k] = R.uk[k];
    }
    if (lr_ident) return R1CSError::VerificationError;
    if (lgN) Scalar::batch_invert(R.ukinv);
    TranscriptRng rng = T.build_rng({}, seed);
    R.r = rng.random_scalar();
    R.yinv = R.y.invert();
    return R1CSError::None;
}

}  // namespace bpg
