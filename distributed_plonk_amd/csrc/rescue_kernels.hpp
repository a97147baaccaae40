// rescue_kernels.hpp — the Rescue permutation and Merkle trees over it on the device (included by synth.hip after solve_kernels.hpp, whose
// solve_pow_fixed and ROOT5 exponent these kernels share: the hash a circuit proves with builder.rescue_permutation is the one computed here).
//
// State s in Fr^4, MDS matrix M (4 x 4), round keys K[0 .. 24] (4 elements each), alpha = 5 — jellyfish's structure (width 4, 12 rounds):
//     permute(s):  s <- s + K[0]
//                  for i in 0 .. 11:   s <- M (s_j^(1/5))_j + K[2i+1]          x^(1/5) = x^d, d = 5^-1 mod (r - 1); 0 -> 0
//                                      s <- M (s_j^5)_j     + K[2i+2]
//     hash2(l, r) = permute((l, r, 0, 0))[0]
// A Merkle tree over L = 2^k leaves is one buffer of 2L - 1 Fr in heap order: node 0 the root, the children of node m at 2m + 1 (left) and
// 2m + 2 (right), leaf i at node L - 1 + i, node[m] = hash2(node[2m+1], node[2m+2]).
//
// params: 116 Fr, Montgomery, in a device buffer: M row-major (16), then K[t][i] at 16 + 4t + i.  Every index into it is uniform over the
// grid, so its reads are scalar loads.
//
// One lane per state, the state in registers.  A round is 4 x ~335 products for the inverse S-boxes (solve_hints.hpp's count per power),
// 4 x 3 for x^5 and 2 x 16 for the two matrix products: 12 x (1340 + 12 + 32) ~ 16.6 k products per permutation.  The four inverse S-boxes
// run one after another through solve_pow_fixed — its window table is 56 VGPRs, four of them would not fit the register file — as FOUR TURNS
// OF ONE LOOP over a state that rotates by one element per turn: every register index stays a constant (an index s[j] with j a loop counter
// would send the state to scratch memory, and so does a conditional between two Fr lvalues: solve_pow_kernel), and the power's code exists
// once per kernel instead of four times.
#pragma once

constexpr int RESCUE_ROUNDS = 12;
constexpr int RESCUE_KEYS = 2 * RESCUE_ROUNDS + 1;
constexpr int RESCUE_PARAM_FR = 16 + 4 * RESCUE_KEYS;          // 116

// s <- M t + K[key]
__device__ __forceinline__ void rescue_affine(const Fr& t0, const Fr& t1, const Fr& t2, const Fr& t3, const Fr* __restrict__ prm, int key, Fr& s0, Fr& s1,
                                              Fr& s2, Fr& s3, const FrParams& P) {
    const Fr* k = prm + 16 + 4 * key;
#define RESCUE_ROW(i) \
    fp_add(fp_add(fp_add(fp_mul(prm[4 * (i)], t0, P), fp_mul(prm[4 * (i) + 1], t1, P), P), fp_add(fp_mul(prm[4 * (i) + 2], t2, P), fp_mul(prm[4 * (i) + 3], t3, P), P), P), k[i], P)
    const Fr r0 = RESCUE_ROW(0), r1 = RESCUE_ROW(1), r2 = RESCUE_ROW(2), r3 = RESCUE_ROW(3);
#undef RESCUE_ROW
    s0 = r0; s1 = r1; s2 = r2; s3 = r3;
}

__device__ __forceinline__ Fr rescue_pow5(const Fr& x, const FrParams& P) {
    const Fr x2 = fp_sqr(x, P);
    return fp_mul(fp_sqr(x2, P), x, P);
}

__device__ __forceinline__ void rescue_permute_body(Fr& s0, Fr& s1, Fr& s2, Fr& s3, const Fr* __restrict__ prm, const SolveExponent& e, const FrParams& P) {
    s0 = fp_add(s0, prm[16], P);
    s1 = fp_add(s1, prm[17], P);
    s2 = fp_add(s2, prm[18], P);
    s3 = fp_add(s3, prm[19], P);
#pragma unroll 1
    for (int i = 0; i < RESCUE_ROUNDS; i++) {
#pragma unroll 1
        for (int j = 0; j < 4; j++) {                              // after four turns the state is back in order
            const Fr y = solve_pow_fixed(s0, e, P);
            s0 = s1; s1 = s2; s2 = s3; s3 = y;
        }
        rescue_affine(s0, s1, s2, s3, prm, 2 * i + 1, s0, s1, s2, s3, P);
        const Fr p0 = rescue_pow5(s0, P), p1 = rescue_pow5(s1, P), p2 = rescue_pow5(s2, P), p3 = rescue_pow5(s3, P);
        rescue_affine(p0, p1, p2, p3, prm, 2 * i + 2, s0, s1, s2, s3, P);
    }
}

// states: [count][4] Fr, permuted in place
__global__ void __launch_bounds__(CIRC_THREADS) rescue_permute_kernel(Fr* __restrict__ states, uint64_t count, const Fr* __restrict__ prm, const SolveExponent e,
                                                                      const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    Fr* s = states + 4 * t;
    Fr s0 = s[0], s1 = s[1], s2 = s[2], s3 = s[3];
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    s[0] = s0; s[1] = s1; s[2] = s2; s[3] = s3;
}

// One level of a tree in heap order: the `parents` nodes from `first` on, each from its two children (which lie beyond the level: no lane
// reads what another writes).
__global__ void __launch_bounds__(CIRC_THREADS) rescue_merkle_level_kernel(Fr* __restrict__ nodes, uint64_t first, uint64_t parents, const Fr* __restrict__ prm,
                                                                           const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= parents) return;
    const uint64_t m = first + t;
    Fr s0 = nodes[2 * m + 1], s1 = nodes[2 * m + 2], s2 = fp_zero<8>(), s3 = fp_zero<8>();
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    nodes[m] = s0;
}

static inline int rescue_exponent(int curve, SolveExponent* e_root5, const char* who) {
    SolveExponent e_inv;
    if (!solve_exponents(fr_params(curve), &e_inv, e_root5)) return plonk_fail(PLONK_ERR_ARG, "%s: 5 divides r - 1, ROOT5 is not defined on this field", who);
    return PLONK_OK;
}

// count > 0 states; enqueued on `stream`, not synchronised
int rescue_permute_run(int curve, const Fr* d_params, Fr* d_states, size_t count, hipStream_t stream, const char* who) {
    SolveExponent e;
    int rc = rescue_exponent(curve, &e, who);
    if (rc) return rc;
    const uint64_t blocks = ((uint64_t)count + CIRC_THREADS - 1) / CIRC_THREADS;
    if (blocks > 0x7FFFFFFFull) return plonk_fail(PLONK_ERR_ARG, "%s: count = %zu exceeds one launch (2^31 - 1 workgroups of %u states)", who, count, CIRC_THREADS);
    ProfScope ps("rescue_permute", stream);
    hipLaunchKernelGGL(rescue_permute_kernel, dim3((uint32_t)blocks), dim3(CIRC_THREADS), 0, stream, d_states, (uint64_t)count, d_params, e, fr_params(curve));
    return circ_launch_status("rescue_permute");
}

// 1 <= log_leaves <= 31: one launch per level, bottom-up (level l holds the 2^l nodes from 2^l - 1 on); enqueued, not synchronised
int rescue_merkle_run(int curve, const Fr* d_params, Fr* d_nodes, unsigned log_leaves, hipStream_t stream, const char* who) {
    SolveExponent e;
    int rc = rescue_exponent(curve, &e, who);
    if (rc) return rc;
    ProfScope ps("rescue_merkle", stream);
    for (int l = (int)log_leaves - 1; l >= 0; l--) {
        const uint64_t parents = (uint64_t)1 << l;
        hipLaunchKernelGGL(rescue_merkle_level_kernel, dim3(circ_grid_of(parents, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, d_nodes, parents - 1, parents, d_params,
                           e, fr_params(curve));
        if ((rc = circ_launch_status("rescue_merkle_level"))) return rc;
    }
    return PLONK_OK;
}
