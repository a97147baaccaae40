// verify_kernels.hpp — the per-proof work of batched PLONK verification (jf-plonk's verify / batch_verify up to the pairing), included by
// synth.hip.  K proofs against one verifying key, one lane per proof, no dependence between proofs:
//   verify_scalars_kernel   input checks, the Fiat-Shamir replay (merlin / STROBE-128 over Keccak-f[1600], byte state in LDS), Z_H(zeta),
//                           L1(zeta), PI(zeta) (one inversion for all of them), r(zeta), E and the 34 coefficients of the folded check
//   verify_subgroup_kernel  BLS12-381 only: [r] P == O for each of a proof's 13 points, one lane per point
//   verify_points_kernel    rho * A and rho * B as two multi-scalar sums over the 32 + 2 points (Straus: one doubling chain per sum)
// with, as in oracle-free form of verifier_ref.verify,
//   A = W_z + u W_zw,   B = zeta W_z + u zeta w W_zw + F + u [z] - (E + u z_w) G,
//   F = [r] + sum_{i<5} v^(1+i) [w_i] + sum_{i<4} v^(6+i) [sigma_i],   [r] the linearisation over the 13 selectors, [z], [sigma_4], [t_i].
// A proof whose status word is not 0 gets A = B = O.  The pairing of the sums runs on the host (pairing.hpp).
// verify_scalars_multi_kernel / verify_points_multi_kernel do the same with a key PER PROOF (jf-plonk's batch_verify): the keys' Params and
// commitment pointers sit in one device table, lane j works under row vk_index[j] on its span of a ragged public-input list.  They share
// the lane bodies (vfy::scalars_lane, vfy::points_lane) with the one-key kernels, which stay what they were.
// g1_tree_leaves_kernel / g1_tree_level_kernel fold the K output pairs into a heap-ordered sum tree, so that the host pairs the root and,
// when that fails, bisects over nodes it reads back instead of re-adding points.
#pragma once
#include <cstring>
#include "constants.h"
#include "ec.hpp"

namespace vfy {

constexpr int NPTS = 13;                 // proof points: wires[5], z, quotient[5], W_zeta, W_zeta_omega
constexpr int NEVALS = 10;               // wires_evals[5], wire_sigma_evals[4], perm_next_eval
constexpr int NCOEF = 34;                // B over 32 points (13 selectors, 5 sigmas, G, 5 wires, z, 5 quotient chunks, W_z, W_zw), A over 2
constexpr int NDEBUG = 9;                // beta, gamma, alpha, zeta, v, u, PI(zeta), r(zeta), E
constexpr int STROBE_R = 166;
constexpr int LANES = 64;                // lanes per workgroup of the transcript kernel: 64 x 200 B of LDS

enum : uint32_t { ST_OFF_CURVE = 1, ST_SUBGROUP = 2, ST_ZETA_DOMAIN = 4, ST_NONCANONICAL = 8,
                  ST_BAD_KEY = 32, ST_BAD_SPAN = 64 };     // the multi-key kernels only (16 is the codec's)

struct Params {
    uint8_t strobe[200];                 // the transcript after the verifying-key messages
    uint32_t pos, pos_begin, cur_flags;
    uint32_t log_n, num_inputs;
    Fr k[5], omega, n_fr;                // Montgomery
};
struct KeyEntry {                        // one row of the key table of the multi-key kernels
    Params prm;
    const uint32_t* comms;               // device: 13 selector then 5 sigma commitments
};

template <int N> __device__ __forceinline__ bool lt_mod(const uint32_t* a, const uint32_t* p) {     // a < p as integers
    bool lt = false, eq = true;
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        lt = lt || (eq && a[i] < p[i]);
        eq = eq && a[i] == p[i];
    }
    return lt;
}

// ------------------------------------------------------------------------------------------------ Keccak-f[1600] / STROBE-128 / merlin
__device__ __forceinline__ uint64_t rol64(uint64_t v, int r) { return r ? (v << r) | (v >> (64 - r)) : v; }

__device__ __attribute__((noinline)) void keccak_f1600(uint8_t* st) {
    const uint64_t RC[24] = {0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull,
                             0x0000000080000001ull, 0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull,
                             0x0000000080008009ull, 0x000000008000000Aull, 0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull,
                             0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull, 0x000000000000800Aull, 0x800000008000000Aull,
                             0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    const int ROT[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};   // [x + 5 y]
    uint64_t a[25];
    uint64_t* s = reinterpret_cast<uint64_t*>(st);
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = s[i];
#pragma unroll                           // fully: RC[rnd] then needs no runtime-indexed array (which would live in scratch)
    for (int rnd = 0; rnd < 24; rnd++) {
        uint64_t c[5], b[25];
#pragma unroll
        for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
        for (int x = 0; x < 5; x++) {
            const uint64_t d = c[(x + 4) % 5] ^ rol64(c[(x + 1) % 5], 1);
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] ^= d;
        }
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) b[y + 5 * ((2 * x + 3 * y) % 5)] = rol64(a[x + 5 * y], ROT[x + 5 * y]);
#pragma unroll
        for (int x = 0; x < 5; x++)
#pragma unroll
            for (int y = 0; y < 5; y++) a[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
        a[0] ^= RC[rnd];
    }
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = a[i];
}

struct Strobe {
    uint8_t* st;                         // this lane's 200 bytes of LDS
    int pos, pos_begin, cur_flags;

    __device__ void run_f() {
        st[pos] ^= (uint8_t)pos_begin;
        st[pos + 1] ^= 0x04;
        st[STROBE_R + 1] ^= 0x80;
        keccak_f1600(st);
        pos = pos_begin = 0;
    }
    __device__ void absorb(uint8_t b) {
        st[pos] ^= b;
        if (++pos == STROBE_R) run_f();
    }
    __device__ uint8_t squeeze() {
        const uint8_t b = st[pos];
        st[pos] = 0;
        if (++pos == STROBE_R) run_f();
        return b;
    }
    __device__ void begin_op(int flags) {            // "more" is never set by the ops below except for the length prefix
        const int old_begin = pos_begin;
        pos_begin = pos + 1;
        cur_flags = flags;
        absorb((uint8_t)old_begin);
        absorb((uint8_t)flags);
        if ((flags & (4 | 32)) && pos != 0) run_f();
    }
    __device__ void label(const char* s, uint32_t len) {     // meta_ad(label) + meta_ad(le32(len), more)
        begin_op(16 | 2);
        for (; *s; s++) absorb((uint8_t)*s);
#pragma unroll
        for (int i = 0; i < 4; i++) absorb((uint8_t)(len >> (8 * i)));
    }
};

// append_message(label, canonical Fr): 32 bytes little-endian
__device__ void append_fr(Strobe& t, const char* lab, const Fr& canon) {
    t.label(lab, 32);
    t.begin_op(2);
#pragma unroll
    for (int i = 0; i < 32; i++) t.absorb((uint8_t)(canon.l[i >> 2] >> (8 * (i & 3))));
}
// append_message(label, compressed G1): x little-endian, bit 7 of the last byte = y > -y, bit 6 = infinity
template <int NQ> __device__ void append_g1(Strobe& t, const char* lab, const AffPt<NQ>& pt, const FpParams<NQ>& Q) {
    t.label(lab, 4 * NQ);
    t.begin_op(2);
    const bool inf = aff_is_inf(pt);
    const Fp<NQ> x = fp_from_mont(pt.x, Q), y = fp_from_mont(pt.y, Q);
    const Fp<NQ> ny = fp_neg(y, Q);
    const bool big = !inf && lt_mod<NQ>(ny.l, y.l);
    const uint8_t flag = inf ? 0x40 : (big ? 0x80 : 0);
#pragma unroll
    for (int i = 0; i < 4 * NQ; i++) {
        uint8_t b = inf ? 0 : (uint8_t)(x.l[i >> 2] >> (8 * (i & 3)));
        if (i == 4 * NQ - 1) b |= flag;
        t.absorb(b);
    }
}
// get_and_append_challenge: 64 bytes reduced mod r (from_le_bytes_mod_order), then absorbed as canonical Fr; returns Montgomery
__device__ Fr challenge(Strobe& t, const char* lab, const FpParams<8>& R) {
    t.label(lab, 64);
    t.begin_op(1 | 2 | 4);
    uint32_t w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) v |= (uint32_t)t.squeeze() << (8 * b);
        w[i] = v;
    }
    Fr two32 = fp_zero<8>();
    two32.l[1] = 1;
    two32 = fp_to_mont(two32, R);
    Fr acc = fp_zero<8>();
#pragma unroll
    for (int i = 15; i >= 0; i--) {
        Fr li = fp_zero<8>();
        li.l[0] = w[i];
        acc = fp_add(fp_mul(acc, two32, R), fp_to_mont(li, R), R);
    }
    append_fr(t, lab, fp_from_mont(acc, R));
    return acc;
}

template <int NQ> __device__ __forceinline__ AffPt<NQ> load_pt(const uint32_t* rec, int i) {
    AffPt<NQ> p;
    p.x = fp_from_limbs<NQ>(rec + 2 * NQ * i);
    p.y = fp_from_limbs<NQ>(rec + 2 * NQ * i + NQ);
    return p;
}

}  // namespace vfy

// ------------------------------------------------------------------------------------------------ kernel 1: checks, transcript, scalars
namespace vfy {
// One proof under one key: prm is that key's entry (a kernel argument of verify_scalars_kernel, a row of the key table of
// verify_scalars_multi_kernel), st the lane's 200 bytes of LDS already holding prm.strobe, rec the proof's record, pub ITS public inputs
// (prm.num_inputs of them).  No barrier: a lane that returns early leaves its neighbours alone.
template <int NQ>
__device__ __forceinline__ void scalars_lane(const Params& prm, uint8_t* st, const uint32_t* rec, const Fr* pub, const Fr* __restrict__ rho, uint32_t pid,
                                             Fr* __restrict__ coef, uint32_t* __restrict__ status, Fr* __restrict__ debug, const FpParams<8>& R,
                                             const FpParams<NQ>& Q, const Fp<NQ>& b) {
    const Fr* ev = reinterpret_cast<const Fr*>(rec + 2 * NQ * NPTS);
    uint32_t stw = 0;
    // input checks: coordinates and evaluations canonical, points on the curve (or (0, 0) = infinity)
    for (int i = 0; i < NPTS; i++) {
        const AffPt<NQ> p = load_pt<NQ>(rec, i);
        if (!lt_mod<NQ>(p.x.l, Q.p) || !lt_mod<NQ>(p.y.l, Q.p)) { stw |= ST_NONCANONICAL; continue; }
        if (aff_is_inf(p)) continue;
        const Fp<NQ> rhs = fp_add(fp_mul(fp_sqr(p.x, Q), p.x, Q), b, Q);
        if (!fp_eq(fp_sqr(p.y, Q), rhs)) stw |= ST_OFF_CURVE;
    }
    for (int i = 0; i < NEVALS; i++)
        if (!lt_mod<8>(ev[i].l, R.p)) stw |= ST_NONCANONICAL;
    for (uint32_t i = 0; i < prm.num_inputs; i++)
        if (!lt_mod<8>(pub[i].l, R.p)) stw |= ST_NONCANONICAL;
    if (!lt_mod<8>(rho[pid].l, R.p)) stw |= ST_NONCANONICAL;
    Fr* cf = coef + (size_t)pid * NCOEF;
    if (stw) {
        status[pid] = stw;
        return;
    }

    // Fiat-Shamir (verifier_ref.derive_challenges), continuing from the verifying-key state
    Strobe t{st, (int)prm.pos, (int)prm.pos_begin, (int)prm.cur_flags};
    for (uint32_t i = 0; i < prm.num_inputs; i++) append_fr(t, "public input", fp_from_mont(pub[i], R));
    for (int i = 0; i < 5; i++) append_g1<NQ>(t, "witness_poly_comms", load_pt<NQ>(rec, i), Q);
    const Fr beta = challenge(t, "beta", R);
    const Fr gamma = challenge(t, "gamma", R);
    append_g1<NQ>(t, "perm_poly_comms", load_pt<NQ>(rec, 5), Q);
    const Fr alpha = challenge(t, "alpha", R);
    for (int i = 6; i < 11; i++) append_g1<NQ>(t, "quot_poly_comms", load_pt<NQ>(rec, i), Q);
    const Fr zeta = challenge(t, "zeta", R);
    for (int i = 0; i < 5; i++) append_fr(t, "wire_evals", fp_from_mont(ev[i], R));
    for (int i = 5; i < 9; i++) append_fr(t, "wire_sigma_evals", fp_from_mont(ev[i], R));
    append_fr(t, "perm_next_eval", fp_from_mont(ev[9], R));
    const Fr v = challenge(t, "v", R);
    append_g1<NQ>(t, "open_proof", load_pt<NQ>(rec, 11), Q);
    append_g1<NQ>(t, "shifted_open_proof", load_pt<NQ>(rec, 12), Q);
    const Fr u = challenge(t, "u", R);

    // Z_H(zeta), L1(zeta), PI(zeta): S = sum_i pi_i w^i / (zeta - w^i) as one fraction num / den, then ONE inversion of n * den * (zeta - 1)
    const Fr one = fp_one(R);
    Fr zn = zeta;
    for (uint32_t i = 0; i < prm.log_n; i++) zn = fp_sqr(zn, R);
    const Fr zh = fp_sub(zn, one, R);
    if (fp_is_zero(zh)) {
        status[pid] = ST_ZETA_DOMAIN;
        return;
    }
    Fr num = fp_zero<8>(), den = one, wi = one;
    for (uint32_t i = 0; i < prm.num_inputs; i++) {
        const Fr d = fp_sub(zeta, wi, R);
        num = fp_add(fp_mul(num, d, R), fp_mul(fp_mul(pub[i], wi, R), den, R), R);
        den = fp_mul(den, d, R);
        wi = fp_mul(wi, prm.omega, R);
    }
    const Fr zm1 = fp_sub(zeta, one, R);
    const Fr inv = fp_inv(fp_mul(fp_mul(den, zm1, R), prm.n_fr, R), R);
    const Fr l1 = fp_mul(fp_mul(zh, den, R), inv, R);
    const Fr pi = fp_mul(fp_mul(fp_mul(zh, num, R), zm1, R), inv, R);

    // the linearisation (verifier_ref.verify)
    const Fr a = ev[0], bb = ev[1], c = ev[2], d = ev[3], e = ev[4], zw = ev[9];
    const Fr ab = fp_mul(a, bb, R), cd = fp_mul(c, d, R);
    auto pow5 = [&](const Fr& x) { const Fr x2 = fp_sqr(x, R); return fp_mul(fp_sqr(x2, R), x, R); };
    const Fr rh = rho[pid];
    auto put = [&](int j, const Fr& x) { cf[j] = fp_from_mont(fp_mul(x, rh, R), R); };
    put(0, a); put(1, bb); put(2, c); put(3, d);
    put(4, ab); put(5, cd);
    put(6, pow5(a)); put(7, pow5(bb)); put(8, pow5(c)); put(9, pow5(d));
    put(10, fp_neg(e, R)); put(11, one); put(12, fp_mul(fp_mul(ab, cd, R), e, R));
    const Fr bz = fp_mul(beta, zeta, R);
    Fr pz = alpha;
    for (int i = 0; i < 5; i++) pz = fp_mul(pz, fp_add(fp_add(ev[i], fp_mul(bz, prm.k[i], R), R), gamma, R), R);
    Fr ps = fp_mul(alpha, zw, R);
    for (int i = 0; i < 4; i++) ps = fp_mul(ps, fp_add(fp_add(ev[i], fp_mul(beta, ev[5 + i], R), R), gamma, R), R);
    const Fr a2l1 = fp_mul(fp_sqr(alpha, R), l1, R);
    const Fr r_zeta = fp_add(fp_sub(fp_mul(ps, fp_add(e, gamma, R), R), pi, R), a2l1, R);
    // E = r(zeta) + sum_{j=1..9} v^j evals ; the v powers also weigh [w_i] (v^(1+i)) and [sigma_i] (v^(6+i))
    Fr vj = one, E = r_zeta;
    for (int j = 1; j <= 9; j++) {
        vj = fp_mul(vj, v, R);
        E = fp_add(E, fp_mul(vj, ev[j - 1], R), R);
        if (j <= 5) put(18 + j, vj);             // wires: slots 19..23
        else put(13 + j - 6, vj);                // sigma_0..3: slots 13..16
    }
    put(17, fp_neg(fp_mul(ps, beta, R), R));     // sigma_4
    const Fr zeta_w = fp_mul(zeta, prm.omega, R);
    put(18, fp_neg(fp_add(E, fp_mul(u, zw, R), R), R));      // G
    put(24, fp_add(fp_add(pz, a2l1, R), u, R));              // [z]
    const Fr zn2 = fp_mul(zn, fp_sqr(zeta, R), R);
    Fr cq = fp_neg(zh, R);
    for (int i = 0; i < 5; i++) {                             // -Z_H(zeta) zeta^(i(n+2)) [t_i]
        put(25 + i, cq);
        cq = fp_mul(cq, zn2, R);
    }
    put(30, zeta);                                            // W_zeta in B
    put(31, fp_mul(u, zeta_w, R));                            // W_zeta_omega in B
    put(32, one);                                             // W_zeta in A
    put(33, u);                                               // W_zeta_omega in A
    status[pid] = 0;
    if (debug) {
        Fr* dbg = debug + (size_t)pid * NDEBUG;
        dbg[0] = beta; dbg[1] = gamma; dbg[2] = alpha; dbg[3] = zeta; dbg[4] = v; dbg[5] = u;
        dbg[6] = pi; dbg[7] = r_zeta; dbg[8] = E;
    }
}
}  // namespace vfy

// (kernels at global scope, like every other kernel of the library: codehash.py keys the machine code by kernel name)
template <int NQ>
__global__ void __launch_bounds__(vfy::LANES) verify_scalars_kernel(const vfy::Params prm, const uint32_t* __restrict__ proofs, const Fr* __restrict__ pub,
                                                               const Fr* __restrict__ rho, uint32_t k, Fr* __restrict__ coef, uint32_t* __restrict__ status,
                                                               Fr* __restrict__ debug, const FpParams<8> R, const FpParams<NQ> Q, const Fp<NQ> b) {
    using namespace vfy;
    __shared__ __attribute__((aligned(8))) uint8_t lds[LANES * 200];
    const uint32_t pid = blockIdx.x * LANES + threadIdx.x;
    uint8_t* st = lds + threadIdx.x * 200;
    for (int i = 0; i < 200; i++) st[i] = prm.strobe[i];
    if (pid >= k) return;
    scalars_lane<NQ>(prm, st, proofs + (size_t)pid * (2 * NQ * NPTS + 8 * NEVALS), pub + (size_t)pid * prm.num_inputs, rho, pid, coef, status, debug, R, Q, b);
}

// The same with a key per proof: lane j works under keys[vk_index[j]] on the public inputs [pub_off[j], pub_off[j + 1]) of a ragged list.
// Lanes of one wave may carry different log_n and num_inputs: their loops diverge, nothing else.  A lane whose index or span is bad
// reads nothing through either — not the key table, not pub — and writes only its status word (verify_points_multi_kernel gives it (O, O)):
//   ST_BAD_KEY   vk_index[j] >= n_vks
//   ST_BAD_SPAN  pub_off[j] > pub_off[j + 1], pub_off[j + 1] > pub_total, or (under a good index) a length other than the key's num_inputs
template <int NQ>
__global__ void __launch_bounds__(vfy::LANES) verify_scalars_multi_kernel(const vfy::KeyEntry* __restrict__ keys, uint32_t n_vks,
                                                                     const uint32_t* __restrict__ vk_index, const uint32_t* __restrict__ proofs,
                                                                     const Fr* __restrict__ pub, const uint64_t* __restrict__ pub_off, uint64_t pub_total,
                                                                     const Fr* __restrict__ rho, uint32_t k, Fr* __restrict__ coef,
                                                                     uint32_t* __restrict__ status, Fr* __restrict__ debug, const FpParams<8> R,
                                                                     const FpParams<NQ> Q, const Fp<NQ> b) {
    using namespace vfy;
    __shared__ __attribute__((aligned(8))) uint8_t lds[LANES * 200];
    const uint32_t pid = blockIdx.x * LANES + threadIdx.x;
    if (pid >= k) return;
    const uint32_t idx = vk_index[pid];
    const uint64_t lo = pub_off[pid], hi = pub_off[pid + 1];
    uint32_t stw = 0;
    if (idx >= n_vks) stw |= ST_BAD_KEY;
    if (lo > hi || hi > pub_total) stw |= ST_BAD_SPAN;
    else if (!stw && hi - lo != (uint64_t)keys[idx].prm.num_inputs) stw |= ST_BAD_SPAN;
    if (stw) {
        status[pid] = stw;
        return;
    }
    const Params& prm = keys[idx].prm;
    uint8_t* st = lds + threadIdx.x * 200;
    for (int i = 0; i < 200; i++) st[i] = prm.strobe[i];
    scalars_lane<NQ>(prm, st, proofs + (size_t)pid * (2 * NQ * NPTS + 8 * NEVALS), pub + lo, rho, pid, coef, status, debug, R, Q, b);
}

// ------------------------------------------------------------------------------------------------ kernel 2: r-subgroup of G1 (BLS12-381)
// (the loop below has a copy, codec::g1_times_r_is_inf in codec_kernels.hpp, kept apart so that this kernel's machine code stays what the
// counters of profiles/ were collected from: a change to the one belongs in the other too)
template <int NQ>
__global__ void __launch_bounds__(128) verify_subgroup_kernel(const uint32_t* __restrict__ proofs, uint32_t k, uint32_t* __restrict__ status,
                                                               const FpParams<8> R, const FpParams<NQ> Q) {
    using namespace vfy;
    const uint32_t gid = blockIdx.x * 128 + threadIdx.x;
    if (gid >= k * NPTS) return;
    const uint32_t pid = gid / NPTS, i = gid % NPTS;
    if (status[pid]) return;                                  // unchecked coordinates: nothing to multiply
    const AffPt<NQ> p = load_pt<NQ>(proofs + (size_t)pid * (2 * NQ * NPTS + 8 * NEVALS), i);
    if (aff_is_inf(p)) return;
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int bit = 255; bit >= 0; bit--) {
        acc = xyzz_dbl_cold(acc, Q);
        if ((R.p[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd_cold(acc, p, Q);
    }
    if (!xyzz_is_inf(acc)) atomicOr(&status[pid], (uint32_t)ST_SUBGROUP);
}

// ------------------------------------------------------------------------------------------------ kernel 3: rho A and rho B
namespace vfy {
template <int NQ> __device__ __forceinline__ AffPt<NQ> term_point(int j, const uint32_t* rec, const uint32_t* vk, const AffPt<NQ>& g) {
    if (j < 18) return load_pt<NQ>(vk, j);                    // 13 selectors, 5 sigmas
    if (j == 18) return g;
    if (j < 30) return load_pt<NQ>(rec, j - 19);              // wires, z, quotient chunks
    return load_pt<NQ>(rec, j >= 32 ? j - 21 : j - 19);       // W_z, W_zw (B: 30, 31; A: 32, 33)
}
// one output point: which = 0 rho B over the 32 points of slots 0..31, which = 1 rho A over slots 32, 33; (0, 0) for a proof that is not ok
template <int NQ>
__device__ __forceinline__ void points_lane(uint32_t pid, uint32_t which, bool ok, const uint32_t* __restrict__ proofs, const uint32_t* vk,
                                            const Fr* __restrict__ coef, uint32_t* o, const FpParams<NQ>& Q, const AffPt<NQ>& g) {
    AffPt<NQ> res;
    res.x = fp_zero<NQ>();
    res.y = fp_zero<NQ>();
    if (ok) {
        const uint32_t* rec = proofs + (size_t)pid * (2 * NQ * NPTS + 8 * NEVALS);
        const Fr* cf = coef + (size_t)pid * NCOEF;
        const int j0 = which ? 32 : 0, j1 = which ? 34 : 32;
        XyzzPt<NQ> acc = xyzz_inf<NQ>();
        for (int bit = 255; bit >= 0; bit--) {
            acc = xyzz_dbl_cold(acc, Q);
            for (int j = j0; j < j1; j++)
                if ((cf[j].l[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd_cold(acc, term_point<NQ>(j, rec, vk, g), Q);
        }
        res = xyzz_to_affine(acc, Q);
    }
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        o[i] = res.x.l[i];
        o[NQ + i] = res.y.l[i];
    }
}
}  // namespace vfy

template <int NQ>
__global__ void __launch_bounds__(64) verify_points_kernel(const uint32_t* __restrict__ proofs, const uint32_t* __restrict__ vk, uint32_t k,
                                                            const Fr* __restrict__ coef, const uint32_t* __restrict__ status, uint32_t* __restrict__ out,
                                                            const FpParams<NQ> Q, const AffPt<NQ> g) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= 2 * k) return;
    const uint32_t pid = gid >> 1;                             // gid & 1: 0 rho B, 1 rho A
    vfy::points_lane<NQ>(pid, gid & 1, status[pid] == 0, proofs, vk, coef, out + (size_t)gid * 2 * NQ, Q, g);
}

// the key points through the proof's table row; a status of 0 says that verify_scalars_multi_kernel found vk_index[pid] < n_vks
template <int NQ>
__global__ void __launch_bounds__(64) verify_points_multi_kernel(const uint32_t* __restrict__ proofs, const vfy::KeyEntry* __restrict__ keys,
                                                                  const uint32_t* __restrict__ vk_index, uint32_t k, const Fr* __restrict__ coef,
                                                                  const uint32_t* __restrict__ status, uint32_t* __restrict__ out, const FpParams<NQ> Q,
                                                                  const AffPt<NQ> g) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= 2 * k) return;
    const uint32_t pid = gid >> 1;
    const bool ok = status[pid] == 0;
    vfy::points_lane<NQ>(pid, gid & 1, ok, proofs, ok ? keys[vk_index[pid]].comms : nullptr, coef, out + (size_t)gid * 2 * NQ, Q, g);
}

// ------------------------------------------------------------------------------------------------ the fold: a sum tree over the K pairs
// d_tree: 2P - 1 pairs in heap order (P the next power of two >= k; root 0, children of i at 2i + 1 and 2i + 2, leaf j at P - 1 + j), every
// point affine with (0, 0) = infinity.  One lane per POINT (two per pair), one launch per level.  The addition is complete: xyzz_madd
// (ec.hpp) returns the other operand for an infinity on either side, doubles when x and y agree and gives infinity when only x does; a
// doubling of a point with y = 0 has ZZ = 0, which xyzz_to_affine writes as (0, 0).  One inversion per node point.
template <int NQ>
__global__ void __launch_bounds__(64) g1_tree_leaves_kernel(const uint32_t* __restrict__ points, const uint32_t* __restrict__ mask, uint32_t k, uint32_t P,
                                                             uint32_t* __restrict__ tree) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;        // point gid & 1 of leaf gid >> 1
    if (gid >= 2 * P) return;
    const uint32_t j = gid >> 1;
    const bool live = j < k && !(mask && mask[j]);
    const uint32_t* src = points + (size_t)gid * 2 * NQ;
    uint32_t* dst = tree + ((size_t)(P - 1) * 2 + gid) * 2 * NQ;
#pragma unroll
    for (int i = 0; i < 2 * NQ; i++) dst[i] = live ? src[i] : 0u;
}
template <int NQ>
__global__ void __launch_bounds__(64) g1_tree_level_kernel(uint32_t* __restrict__ tree, uint32_t m, const FpParams<NQ> Q) {
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;        // point gid & 1 of node m - 1 + (gid >> 1), the level of m nodes
    if (gid >= 2 * m) return;
    const size_t node = (size_t)(m - 1) + (gid >> 1), which = gid & 1;
    const AffPt<NQ> a = vfy::load_pt<NQ>(tree + ((2 * node + 1) * 2 + which) * 2 * NQ, 0);
    const AffPt<NQ> b = vfy::load_pt<NQ>(tree + ((2 * node + 2) * 2 + which) * 2 * NQ, 0);
    const AffPt<NQ> r = xyzz_to_affine(xyzz_madd_cold(xyzz_from_affine(a, Q), b, Q), Q);
    uint32_t* o = tree + (node * 2 + which) * 2 * NQ;
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        o[i] = r.x.l[i];
        o[NQ + i] = r.y.l[i];
    }
}

namespace vfy {

template <int NQ>
int run(const Params& prm, const void* proofs, const void* vk_pts, const void* pub, const void* rho, uint32_t k, void* out, uint32_t* status, void* debug,
        void* scratch, const FpParams<8>& R, const FpParams<NQ>& Q, const uint32_t* b, const uint32_t* gx, const uint32_t* gy, hipStream_t stream) {
    Fr* coef = (Fr*)scratch;
    const Fp<NQ> bq = fp_from_limbs<NQ>(b);
    AffPt<NQ> g;
    g.x = fp_from_limbs<NQ>(gx);
    g.y = fp_from_limbs<NQ>(gy);
    hipLaunchKernelGGL(verify_scalars_kernel<NQ>, dim3((k + LANES - 1) / LANES), dim3(LANES), 0, stream, prm, (const uint32_t*)proofs, (const Fr*)pub,
                       (const Fr*)rho, k, coef, status, (Fr*)debug, R, Q, bq);
    if (NQ == 12)
        hipLaunchKernelGGL(verify_subgroup_kernel<NQ>, dim3((k * NPTS + 127) / 128), dim3(128), 0, stream, (const uint32_t*)proofs, k, status, R, Q);
    hipLaunchKernelGGL(verify_points_kernel<NQ>, dim3((2 * k + 63) / 64), dim3(64), 0, stream, (const uint32_t*)proofs, (const uint32_t*)vk_pts, k,
                       (const Fr*)coef, (const uint32_t*)status, (uint32_t*)out, Q, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "verify_batch launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

template <int NQ>
int run_multi(const KeyEntry* keys, uint32_t n_vks, const void* proofs, const void* vk_index, const void* pub, const void* pub_off, uint64_t pub_total,
              const void* rho, uint32_t k, void* out, uint32_t* status, void* debug, void* scratch, const FpParams<8>& R, const FpParams<NQ>& Q,
              const uint32_t* b, const uint32_t* gx, const uint32_t* gy, hipStream_t stream) {
    Fr* coef = (Fr*)scratch;
    const Fp<NQ> bq = fp_from_limbs<NQ>(b);
    AffPt<NQ> g;
    g.x = fp_from_limbs<NQ>(gx);
    g.y = fp_from_limbs<NQ>(gy);
    hipLaunchKernelGGL(verify_scalars_multi_kernel<NQ>, dim3((k + LANES - 1) / LANES), dim3(LANES), 0, stream, keys, n_vks, (const uint32_t*)vk_index,
                       (const uint32_t*)proofs, (const Fr*)pub, (const uint64_t*)pub_off, pub_total, (const Fr*)rho, k, coef, status, (Fr*)debug, R, Q, bq);
    if (NQ == 12)                                             // skips every proof whose status is already set: nothing is read for a bad index
        hipLaunchKernelGGL(verify_subgroup_kernel<NQ>, dim3((k * NPTS + 127) / 128), dim3(128), 0, stream, (const uint32_t*)proofs, k, status, R, Q);
    hipLaunchKernelGGL(verify_points_multi_kernel<NQ>, dim3((2 * k + 63) / 64), dim3(64), 0, stream, (const uint32_t*)proofs, keys,
                       (const uint32_t*)vk_index, k, (const Fr*)coef, (const uint32_t*)status, (uint32_t*)out, Q, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "verify_batch_multi launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

template <int NQ> int sum_tree(const void* points, uint32_t k, const void* mask, void* tree, const FpParams<NQ>& Q, hipStream_t stream) {
    uint32_t P = 1;
    while (P < k) P <<= 1;
    hipLaunchKernelGGL(g1_tree_leaves_kernel<NQ>, dim3((2 * P + 63) / 64), dim3(64), 0, stream, (const uint32_t*)points, (const uint32_t*)mask, k, P,
                       (uint32_t*)tree);
    for (uint32_t m = P >> 1; m >= 1; m >>= 1)
        hipLaunchKernelGGL(g1_tree_level_kernel<NQ>, dim3((2 * m + 63) / 64), dim3(64), 0, stream, (uint32_t*)tree, m, Q);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "g1_sum_tree launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

static void fill_params(Params& prm, const uint8_t* strobe, const uint32_t* strobe_pos3, size_t log_n, size_t num_inputs, const uint64_t* k_mont,
                        const Fr& omega, const Fr& n_fr) {
    for (int i = 0; i < 200; i++) prm.strobe[i] = strobe[i];
    prm.pos = strobe_pos3[0];
    prm.pos_begin = strobe_pos3[1];
    prm.cur_flags = strobe_pos3[2];
    prm.log_n = (uint32_t)log_n;
    prm.num_inputs = (uint32_t)num_inputs;
    for (int i = 0; i < 5; i++) prm.k[i] = fp_from_limbs<8>((const uint32_t*)(k_mont + 4 * i));
    prm.omega = omega;
    prm.n_fr = n_fr;
}

}  // namespace vfy

size_t verify_batch_scratch_bytes(size_t k) { return k * vfy::NCOEF * sizeof(Fr); }

int verify_batch_run(int curve, const uint8_t* strobe, const uint32_t* strobe_pos3, size_t log_n, size_t num_inputs, const uint64_t* k_mont,
                     const Fr& omega, const Fr& n_fr, const void* d_proofs, const void* d_vk_pts, const void* d_pub, const void* d_rho, size_t k,
                     void* d_out, void* d_status, void* d_debug, void* scratch, hipStream_t stream) {
    vfy::Params prm;
    vfy::fill_params(prm, strobe, strobe_pos3, log_n, num_inputs, k_mont, omega, n_fr);
    if (curve == PLONK_BN254)
        return vfy::run<8>(prm, d_proofs, d_vk_pts, d_pub, d_rho, (uint32_t)k, d_out, (uint32_t*)d_status, d_debug, scratch, BN254_FR_PARAMS, BN254_FQ_PARAMS,
                           BN254_G1_B_MONT, BN254_G1_GX_MONT, BN254_G1_GY_MONT, stream);
    return vfy::run<12>(prm, d_proofs, d_vk_pts, d_pub, d_rho, (uint32_t)k, d_out, (uint32_t*)d_status, d_debug, scratch, BLS12_381_FR_PARAMS,
                        BLS12_381_FQ_PARAMS, BLS12_381_G1_B_MONT, BLS12_381_G1_GX_MONT, BLS12_381_G1_GY_MONT, stream);
}

size_t verify_key_entry_bytes() { return sizeof(vfy::KeyEntry); }

void verify_key_entry_fill(void* entry, const uint8_t* strobe, const uint32_t* strobe_pos3, size_t log_n, size_t num_inputs, const uint64_t* k_mont,
                           const Fr& omega, const Fr& n_fr, const void* d_comms) {
    vfy::KeyEntry* e = (vfy::KeyEntry*)entry;
    memset(e, 0, sizeof *e);                                  // padding too: the context compares tables as bytes
    vfy::fill_params(e->prm, strobe, strobe_pos3, log_n, num_inputs, k_mont, omega, n_fr);
    e->comms = (const uint32_t*)d_comms;
}

int verify_batch_multi_run(int curve, const void* d_key_table, size_t n_vks, const void* d_proofs, const void* d_vk_index, const void* d_pub,
                           const void* d_pub_off, size_t pub_total, const void* d_rho, size_t k, void* d_out, void* d_status, void* d_debug, void* scratch,
                           hipStream_t stream) {
    const vfy::KeyEntry* keys = (const vfy::KeyEntry*)d_key_table;
    if (curve == PLONK_BN254)
        return vfy::run_multi<8>(keys, (uint32_t)n_vks, d_proofs, d_vk_index, d_pub, d_pub_off, pub_total, d_rho, (uint32_t)k, d_out, (uint32_t*)d_status, d_debug,
                                 scratch, BN254_FR_PARAMS, BN254_FQ_PARAMS, BN254_G1_B_MONT, BN254_G1_GX_MONT, BN254_G1_GY_MONT, stream);
    return vfy::run_multi<12>(keys, (uint32_t)n_vks, d_proofs, d_vk_index, d_pub, d_pub_off, pub_total, d_rho, (uint32_t)k, d_out, (uint32_t*)d_status, d_debug,
                              scratch, BLS12_381_FR_PARAMS, BLS12_381_FQ_PARAMS, BLS12_381_G1_B_MONT, BLS12_381_G1_GX_MONT, BLS12_381_G1_GY_MONT, stream);
}

int g1_sum_tree_run(int curve, const void* d_points, size_t k, const void* d_mask, void* d_tree, hipStream_t stream) {
    if (curve == PLONK_BN254) return vfy::sum_tree<8>(d_points, (uint32_t)k, d_mask, d_tree, BN254_FQ_PARAMS, stream);
    return vfy::sum_tree<12>(d_points, (uint32_t)k, d_mask, d_tree, BLS12_381_FQ_PARAMS, stream);
}
