// pairing.hpp — G2 on the sextic twist and the optimal ate pairing of BN254 and BLS12-381, host code (included by plonk_api.hip).
//
// What it is for: the last step of a KZG / PLONK verification, e(A, [tau]_2) * e(-B, [1]_2) == 1 (jf-plonk's verifier), once per batch of
// proofs.  Everything per proof runs on the device (verify_kernels.hpp); this file runs a handful of pairings per batch, so it states the
// arithmetic plainly, correctness first:
//   * towers  Fq2 = Fq[u]/(u^2 + 1),  Fq6 = Fq2[v]/(v^3 - xi),  Fq12 = Fq6[w]/(w^2 - v)   (w^6 = xi), schoolbook products;
//   * G2 in affine coordinates on the twist (one Fq2 inversion per group operation);
//   * the Miller loop runs on the UNTWISTED point psi(Q) in E(Fq12): D-type (BN254, b' = b/xi) psi(x, y) = (x w^2, y w^3), M-type
//     (BLS12-381, b' = b xi) psi(x, y) = (x w^-2, y w^-3).  Lines are the affine tangents / chords evaluated at P, so no twist-specific
//     sparse multiplication exists to get wrong; the Frobenius of BN254's two extra lines is the p-th power of psi(Q)'s coordinates;
//   * final exponentiation: the easy part f^(p^6 - 1) = conj(f) / f, then a square-and-multiply by (p^6 + 1) / r (constants.h).
// Vertical lines are left out: their values lie in a proper subfield and vanish under the final exponentiation.
// Values: Montgomery residues of the library's Fq (R = 2^(32 N)), as every point of the C ABI.
#pragma once
#include <string.h>

#include "constants.h"

namespace pairing {

template <int N> struct Fq2 { Fp<N> c0, c1; };
template <int N> struct Fq6 { Fq2<N> c0, c1, c2; };
template <int N> struct Fq12 { Fq6<N> c0, c1; };

template <int N> struct Curve {
    const FpParams<N>* P;
    Fq2<N> xi, b2;             // the non-residue of the tower and the twist's b
    Fq2<N> gx, gy;             // arkworks' G2 generator
    bool m_type;
    uint64_t loop[2];          // |m| of the Miller loop, low word first
    bool loop_neg;
    const uint32_t* hard_exp;  // (p^6 + 1) / r
    int hard_words;
    const FpParams<8>* R;      // the scalar field (its modulus is the group order r)
};

template <int N> inline Fq2<N> load2(const uint32_t (*a)[N]) {
    Fq2<N> r;
    r.c0 = fp_from_limbs<N>(a[0]);
    r.c1 = fp_from_limbs<N>(a[1]);
    return r;
}

template <int N> const Curve<N>& curve();
template <> inline const Curve<8>& curve<8>() {
    static const Curve<8> c = {&BN254_FQ_PARAMS, load2<8>(BN254_XI_MONT), load2<8>(BN254_G2_B_MONT), load2<8>(BN254_G2_GEN_MONT), load2<8>(BN254_G2_GEN_MONT + 2),
                               BN254_TWIST_M != 0, {BN254_ATE_LOOP[0], BN254_ATE_LOOP[1]}, BN254_ATE_LOOP_NEG != 0, BN254_FINAL_EXP, BN254_FINAL_EXP_WORDS,
                               &BN254_FR_PARAMS};
    return c;
}
template <> inline const Curve<12>& curve<12>() {
    static const Curve<12> c = {&BLS12_381_FQ_PARAMS, load2<12>(BLS12_381_XI_MONT), load2<12>(BLS12_381_G2_B_MONT), load2<12>(BLS12_381_G2_GEN_MONT),
                                load2<12>(BLS12_381_G2_GEN_MONT + 2), BLS12_381_TWIST_M != 0, {BLS12_381_ATE_LOOP[0], BLS12_381_ATE_LOOP[1]},
                                BLS12_381_ATE_LOOP_NEG != 0, BLS12_381_FINAL_EXP, BLS12_381_FINAL_EXP_WORDS, &BLS12_381_FR_PARAMS};
    return c;
}

// ------------------------------------------------------------------------------------------------ Fq2
template <int N> inline Fq2<N> f2_zero() { return {fp_zero<N>(), fp_zero<N>()}; }
template <int N> inline Fq2<N> f2_one(const FpParams<N>& P) { return {fp_one(P), fp_zero<N>()}; }
template <int N> inline bool f2_is_zero(const Fq2<N>& a) { return fp_is_zero(a.c0) && fp_is_zero(a.c1); }
template <int N> inline bool f2_eq(const Fq2<N>& a, const Fq2<N>& b) { return fp_eq(a.c0, b.c0) && fp_eq(a.c1, b.c1); }
template <int N> inline Fq2<N> f2_add(const Fq2<N>& a, const Fq2<N>& b, const FpParams<N>& P) { return {fp_add(a.c0, b.c0, P), fp_add(a.c1, b.c1, P)}; }
template <int N> inline Fq2<N> f2_sub(const Fq2<N>& a, const Fq2<N>& b, const FpParams<N>& P) { return {fp_sub(a.c0, b.c0, P), fp_sub(a.c1, b.c1, P)}; }
template <int N> inline Fq2<N> f2_neg(const Fq2<N>& a, const FpParams<N>& P) { return {fp_neg(a.c0, P), fp_neg(a.c1, P)}; }
template <int N> inline Fq2<N> f2_mul(const Fq2<N>& a, const Fq2<N>& b, const FpParams<N>& P) {
    const Fp<N> t0 = fp_mul(a.c0, b.c0, P), t1 = fp_mul(a.c1, b.c1, P);
    const Fp<N> t2 = fp_mul(fp_add(a.c0, a.c1, P), fp_add(b.c0, b.c1, P), P);
    return {fp_sub(t0, t1, P), fp_sub(fp_sub(t2, t0, P), t1, P)};
}
template <int N> inline Fq2<N> f2_inv(const Fq2<N>& a, const FpParams<N>& P) {
    const Fp<N> t = fp_inv(fp_add(fp_sqr(a.c0, P), fp_sqr(a.c1, P), P), P);
    return {fp_mul(a.c0, t, P), fp_neg(fp_mul(a.c1, t, P), P)};
}

// ------------------------------------------------------------------------------------------------ Fq6 (v^3 = xi)
template <int N> inline Fq6<N> f6_zero() { return {f2_zero<N>(), f2_zero<N>(), f2_zero<N>()}; }
template <int N> inline Fq6<N> f6_add(const Fq6<N>& a, const Fq6<N>& b, const FpParams<N>& P) {
    return {f2_add(a.c0, b.c0, P), f2_add(a.c1, b.c1, P), f2_add(a.c2, b.c2, P)};
}
template <int N> inline Fq6<N> f6_sub(const Fq6<N>& a, const Fq6<N>& b, const FpParams<N>& P) {
    return {f2_sub(a.c0, b.c0, P), f2_sub(a.c1, b.c1, P), f2_sub(a.c2, b.c2, P)};
}
template <int N> inline Fq6<N> f6_neg(const Fq6<N>& a, const FpParams<N>& P) { return {f2_neg(a.c0, P), f2_neg(a.c1, P), f2_neg(a.c2, P)}; }
template <int N> inline Fq6<N> f6_mul(const Fq6<N>& a, const Fq6<N>& b, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    const Fq2<N> a0b0 = f2_mul(a.c0, b.c0, P), a1b1 = f2_mul(a.c1, b.c1, P), a2b2 = f2_mul(a.c2, b.c2, P);
    const Fq2<N> x12 = f2_add(f2_mul(a.c1, b.c2, P), f2_mul(a.c2, b.c1, P), P);
    const Fq2<N> x01 = f2_add(f2_mul(a.c0, b.c1, P), f2_mul(a.c1, b.c0, P), P);
    const Fq2<N> x02 = f2_add(f2_mul(a.c0, b.c2, P), f2_mul(a.c2, b.c0, P), P);
    return {f2_add(a0b0, f2_mul(C.xi, x12, P), P), f2_add(x01, f2_mul(C.xi, a2b2, P), P), f2_add(x02, a1b1, P)};
}
template <int N> inline Fq6<N> f6_mul_by_v(const Fq6<N>& a, const Curve<N>& C) { return {f2_mul(C.xi, a.c2, *C.P), a.c0, a.c1}; }
template <int N> inline Fq6<N> f6_inv(const Fq6<N>& a, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    const Fq2<N> t0 = f2_sub(f2_mul(a.c0, a.c0, P), f2_mul(C.xi, f2_mul(a.c1, a.c2, P), P), P);
    const Fq2<N> t1 = f2_sub(f2_mul(C.xi, f2_mul(a.c2, a.c2, P), P), f2_mul(a.c0, a.c1, P), P);
    const Fq2<N> t2 = f2_sub(f2_mul(a.c1, a.c1, P), f2_mul(a.c0, a.c2, P), P);
    const Fq2<N> d = f2_add(f2_mul(a.c0, t0, P), f2_mul(C.xi, f2_add(f2_mul(a.c2, t1, P), f2_mul(a.c1, t2, P), P), P), P);
    const Fq2<N> di = f2_inv(d, P);
    return {f2_mul(t0, di, P), f2_mul(t1, di, P), f2_mul(t2, di, P)};
}

// ------------------------------------------------------------------------------------------------ Fq12 (w^2 = v)
template <int N> inline Fq12<N> f12_zero() { return {f6_zero<N>(), f6_zero<N>()}; }
template <int N> inline Fq12<N> f12_one(const FpParams<N>& P) {
    Fq12<N> r = f12_zero<N>();
    r.c0.c0.c0 = fp_one(P);
    return r;
}
template <int N> inline bool f12_eq(const Fq12<N>& a, const Fq12<N>& b) { return memcmp(&a, &b, sizeof a) == 0; }   // residues are fully reduced
template <int N> inline Fq12<N> f12_add(const Fq12<N>& a, const Fq12<N>& b, const FpParams<N>& P) { return {f6_add(a.c0, b.c0, P), f6_add(a.c1, b.c1, P)}; }
template <int N> inline Fq12<N> f12_sub(const Fq12<N>& a, const Fq12<N>& b, const FpParams<N>& P) { return {f6_sub(a.c0, b.c0, P), f6_sub(a.c1, b.c1, P)}; }
template <int N> inline Fq12<N> f12_neg(const Fq12<N>& a, const FpParams<N>& P) { return {f6_neg(a.c0, P), f6_neg(a.c1, P)}; }
template <int N> inline Fq12<N> f12_conj(const Fq12<N>& a, const FpParams<N>& P) { return {a.c0, f6_neg(a.c1, P)}; }    // a^(p^6)
template <int N> inline Fq12<N> f12_mul(const Fq12<N>& a, const Fq12<N>& b, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    return {f6_add(f6_mul(a.c0, b.c0, C), f6_mul_by_v(f6_mul(a.c1, b.c1, C), C), P), f6_add(f6_mul(a.c0, b.c1, C), f6_mul(a.c1, b.c0, C), P)};
}
template <int N> inline Fq12<N> f12_inv(const Fq12<N>& a, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    const Fq6<N> d = f6_inv(f6_sub(f6_mul(a.c0, a.c0, C), f6_mul_by_v(f6_mul(a.c1, a.c1, C), C), P), C);
    return {f6_mul(a.c0, d, C), f6_neg(f6_mul(a.c1, d, C), P)};
}
// a^e for e given as 32-bit words, least significant first
template <int N> inline Fq12<N> f12_pow(const Fq12<N>& a, const uint32_t* e, int words, const Curve<N>& C) {
    Fq12<N> acc = f12_one(*C.P);
    for (int i = 32 * words - 1; i >= 0; i--) {
        acc = f12_mul(acc, acc, C);
        if ((e[i >> 5] >> (i & 31)) & 1) acc = f12_mul(acc, a, C);
    }
    return acc;
}

// ------------------------------------------------------------------------------------------------ G2 (affine, on the twist)
template <int N> struct G2 { Fq2<N> x, y; bool inf; };

template <int N> inline bool g2_on_curve(const G2<N>& q, const Curve<N>& C) {
    if (q.inf) return true;
    const FpParams<N>& P = *C.P;
    const Fq2<N> rhs = f2_add(f2_mul(f2_mul(q.x, q.x, P), q.x, P), C.b2, P);
    return f2_eq(f2_mul(q.y, q.y, P), rhs);
}
template <int N> inline G2<N> g2_neg(const G2<N>& q, const Curve<N>& C) { return {q.x, f2_neg(q.y, *C.P), q.inf}; }
// complete affine addition (P + P, P + (-P), infinity)
template <int N> inline G2<N> g2_add(const G2<N>& a, const G2<N>& b, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    if (a.inf) return b;
    if (b.inf) return a;
    Fq2<N> lam;
    if (f2_eq(a.x, b.x)) {
        if (!f2_eq(a.y, b.y) || f2_is_zero(a.y)) return {f2_zero<N>(), f2_zero<N>(), true};
        const Fq2<N> xx = f2_mul(a.x, a.x, P);
        lam = f2_mul(f2_add(f2_add(xx, xx, P), xx, P), f2_inv(f2_add(a.y, a.y, P), P), P);
    } else {
        lam = f2_mul(f2_sub(b.y, a.y, P), f2_inv(f2_sub(b.x, a.x, P), P), P);
    }
    G2<N> r;
    r.x = f2_sub(f2_sub(f2_mul(lam, lam, P), a.x, P), b.x, P);
    r.y = f2_sub(f2_mul(lam, f2_sub(a.x, r.x, P), P), a.y, P);
    r.inf = false;
    return r;
}
// k * q, k given as 32-bit words (canonical, least significant first)
template <int N> inline G2<N> g2_mul(const G2<N>& q, const uint32_t* k, int words, const Curve<N>& C) {
    G2<N> acc = {f2_zero<N>(), f2_zero<N>(), true};
    for (int i = 32 * words - 1; i >= 0; i--) {
        acc = g2_add(acc, acc, C);
        if ((k[i >> 5] >> (i & 31)) & 1) acc = g2_add(acc, q, C);
    }
    return acc;
}
// on the twist and of order r
template <int N> inline bool g2_check(const G2<N>& q, const Curve<N>& C) {
    return g2_on_curve(q, C) && g2_mul(q, C.R->p, 8, C).inf;
}

// ------------------------------------------------------------------------------------------------ Miller loop on psi(Q) in E(Fq12)
template <int N> struct P12 { Fq12<N> x, y; };

template <int N> inline P12<N> untwist(const G2<N>& q, const Curve<N>& C) {
    P12<N> r;
    r.x = f12_zero<N>();
    r.y = f12_zero<N>();
    if (!C.m_type) {                       // (x w^2, y w^3): w^2 = v, w^3 = v w
        r.x.c0.c1 = q.x;
        r.y.c1.c1 = q.y;
    } else {                               // (x w^-2, y w^-3) = (x/xi w^4, y/xi w^3): w^4 = v^2
        const Fq2<N> xi_inv = f2_inv(C.xi, *C.P);
        r.x.c0.c2 = f2_mul(q.x, xi_inv, *C.P);
        r.y.c1.c1 = f2_mul(q.y, xi_inv, *C.P);
    }
    return r;
}
// f <- f * l(P), T <- T + S (S == T: the tangent), l the line through T and S; P = (px, py) embedded in Fq12
template <int N> inline void line_step(Fq12<N>& f, P12<N>& T, const P12<N>& S, bool dbl, const Fp<N>& px, const Fp<N>& py, const Curve<N>& C) {
    const FpParams<N>& P = *C.P;
    Fq12<N> lam;
    if (dbl) {
        const Fq12<N> xx = f12_mul(T.x, T.x, C);
        lam = f12_mul(f12_add(f12_add(xx, xx, P), xx, P), f12_inv(f12_add(T.y, T.y, P), C), C);
    } else {
        lam = f12_mul(f12_sub(S.y, T.y, P), f12_inv(f12_sub(S.x, T.x, P), C), C);
    }
    Fq12<N> ep_x = f12_zero<N>(), ep_y = f12_zero<N>();
    ep_x.c0.c0.c0 = px;
    ep_y.c0.c0.c0 = py;
    const Fq12<N> l = f12_sub(f12_sub(ep_y, T.y, P), f12_mul(lam, f12_sub(ep_x, T.x, P), C), P);
    f = f12_mul(f, l, C);
    P12<N> r;
    r.x = f12_sub(f12_sub(f12_mul(lam, lam, C), T.x, P), S.x, P);
    r.y = f12_sub(f12_mul(lam, f12_sub(T.x, r.x, P), C), T.y, P);
    T = r;
}
template <int N> inline P12<N> frobenius(const P12<N>& q, const Curve<N>& C) {
    return {f12_pow(q.x, C.P->p, N, C), f12_pow(q.y, C.P->p, N, C)};
}

// f_{m,Q}(P) of the optimal ate pairing (before the final exponentiation); P affine over Fq, neither point infinity
template <int N> inline Fq12<N> miller_loop(const Fp<N>& px, const Fp<N>& py, const G2<N>& q, const Curve<N>& C) {
    const P12<N> Q = untwist(q, C);
    Fq12<N> f = f12_one(*C.P);
    P12<N> T = Q;
    const int top = C.loop[1] ? 127 - __builtin_clzll(C.loop[1]) : 63 - __builtin_clzll(C.loop[0]);
    for (int i = top - 1; i >= 0; i--) {
        f = f12_mul(f, f, C);
        line_step(f, T, T, true, px, py, C);
        if ((C.loop[i >> 6] >> (i & 63)) & 1) line_step(f, T, Q, false, px, py, C);
    }
    if (C.loop_neg) f = f12_conj(f, *C.P);            // f_{-m} = 1 / f_m up to a vertical line; conj = inverse after the final exponentiation
    if (!C.m_type) {                                  // BN: the two Frobenius lines, l_{T, pi(Q)} and l_{T + pi(Q), -pi^2(Q)}
        const P12<N> Q1 = frobenius(Q, C);
        P12<N> Q2 = frobenius(Q1, C);
        Q2.y = f12_neg(Q2.y, *C.P);
        line_step(f, T, Q1, false, px, py, C);
        line_step(f, T, Q2, false, px, py, C);
    }
    return f;
}

template <int N> inline Fq12<N> final_exponentiation(const Fq12<N>& f, const Curve<N>& C) {
    const Fq12<N> g = f12_mul(f12_conj(f, *C.P), f12_inv(f, C), C);       // f^(p^6 - 1)
    return f12_pow(g, C.hard_exp, C.hard_words, C);
}

}  // namespace pairing
