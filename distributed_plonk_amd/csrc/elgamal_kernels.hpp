// elgamal_kernels.hpp — the Rescue sponge, the Rescue counter-mode stream and the ElGamal shared key on the device (included by synth.hip after
// edwards_kernels.hpp: rescue_permute_body, rescue_acc_node_or_zero, ed_mul_body and solve_pow_fixed are shared, nothing of them is changed).
// The functions builder.py's rescue_sponge, rescue_stream and elgamal_encrypt prove, computed in bulk.
//
// permute is rescue_kernels.hpp's width-4 permutation.  The fourth state element is the capacity and carries the domain: hash2 / hash3 use 0,
// the sponge starts at L, the stream uses -1.
//     sponge(x_0 .. x_{L-1}; n_out)   s = (0, 0, 0, L);  for b = 0 .. ceil(L / 3) - 1:  s[j] += x[3b + j] (j < 3, 3b + j < L),  s = permute(s);
//                                     the result is s[0 : n_out], n_out in 1 .. 3.   sponge((a, b, c); 1) = permute((a, b, c, 3))[0] != hash3(a, b, c)
//     stream                          ks_j = permute((k, j, 0, -1))[0 : 3] for block j >= 0 under key k; element i of a text of L elements uses
//                                     ks_{i div 3}[i mod 3]: encryption adds it, decryption subtracts it
//     dh_key(scalar, point)           S = [scalar] point (the residue of the scalar in [0, r), as in edwards_kernels.hpp),  k = hash3(S.x, S.y, 0)
//                                     ElGamal: E = [r] G, S = [r] ek = [dk] E, ct_i = m_i + ks_{i div 3}[i mod 3]
//
// One lane per message (sponge: the blocks are a chain), per (text, block) (stream: counter mode has no chain, and a Rescue launch wants
// width) and per pair (dh_key), the state in registers.  What rescue_kernels.hpp says about scratch memory holds: the absorbed elements of a
// partial last block are read at a clamped index and ANDed with a zero mask (rescue_acc_node_or_zero), the sign of the stream and the
// replacement of a point off the curve are selects per limb (ed_pick), and no conditional stands between two Fr lvalues.
//
// dh_key is TWO launches through a buffer of count points: the multiplication with its inversion (the mul kernel's body behind the curve
// check), then the permutation.  One kernel doing both in a lane was built first and measured (profiles/elgamal.txt): 205 VGPRs, no scratch,
// 263.6 ms for 2^20 keys on BN254 where the two kernels take 241.3 ms together.  A kernel has ONE register allocation: fused, the permutation
// (three quarters of the products) ran under the multiplication loop's 2 waves per SIMD instead of its own 3, and its single chain of
// dependent products per S-box has less to overlap than the point formulas.  The buffer costs 128 bytes of traffic per key against 21.8 k
// products.
#pragma once

static_assert(ELGAMAL_LANES_PER_GROUP == CIRC_THREADS, "plonk_internal.hpp's launch limit");

// out[t][0 : n_out] = sponge(in[t][0 : L]; n_out)
__global__ void __launch_bounds__(CIRC_THREADS) rescue_sponge_kernel(const Fr* __restrict__ in, uint64_t L, uint64_t count, uint32_t n_out, Fr* __restrict__ out,
                                                                     const Fr* __restrict__ prm, const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    const Fr* x = in + t * L;
    Fr s0 = fp_zero<8>(), s1 = fp_zero<8>(), s2 = fp_zero<8>(), s3 = rescue_acc_fr_of_u64(L, P);
#pragma unroll 1
    for (uint64_t i = 0; i < L; i += 3) {
        s0 = fp_add(s0, x[i], P);
        s1 = fp_add(s1, rescue_acc_node_or_zero(x, i + 1, L), P);
        s2 = fp_add(s2, rescue_acc_node_or_zero(x, i + 2, L), P);
        rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    }
    Fr* o = out + t * n_out;
    o[0] = s0;
    if (n_out > 1) o[1] = s1;
    if (n_out > 2) o[2] = s2;
}

// lane (i, j), j < nblocks = ceil(L / 3):  out[i][3j + k] = in[i][3j + k] +- permute((keys[i], j, 0, -1))[k] for k < 3 and 3j + k < L; out may be in
__global__ void __launch_bounds__(CIRC_THREADS) rescue_stream_kernel(const Fr* __restrict__ keys, const Fr* in, uint64_t L, uint64_t nblocks, uint64_t lanes,
                                                                     uint32_t decrypt, Fr* out, const Fr* __restrict__ prm, const SolveExponent e, const FrParams P) {
    const uint64_t lane = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (lane >= lanes) return;
    const uint64_t i = lane / nblocks, j = lane % nblocks;
    Fr s0 = keys[i], s1 = rescue_acc_fr_of_u64(j, P), s2 = fp_zero<8>(), s3 = fp_neg(fp_one(P), P);
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    const bool sub = decrypt != 0;
    const uint64_t at = i * L + 3 * j, left = L - 3 * j;                 // left >= 1: j < nblocks
    const Fr v0 = in[at];
    out[at] = ed_pick(sub, fp_sub(v0, s0, P), fp_add(v0, s0, P));
    if (left > 1) {
        const Fr v1 = in[at + 1];
        out[at + 1] = ed_pick(sub, fp_sub(v1, s1, P), fp_add(v1, s1, P));
    }
    if (left > 2) {
        const Fr v2 = in[at + 2];
        out[at + 2] = ed_pick(sub, fp_sub(v2, s2, P), fp_add(v2, s2, P));
    }
}

// shared[t] = [scalars[t]] points[t], affine; a point off the curve is taken for the identity (0, 1)
__global__ void __launch_bounds__(CIRC_THREADS) edwards_dh_point_kernel(const Fr* __restrict__ scalars, const Fr* __restrict__ points, uint64_t count,
                                                                        Fr* __restrict__ shared, const EdCurve c, const SolveExponent e_inv, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    Fr x = points[2 * t], y = points[2 * t + 1];
    {
        const Fr xx = fp_sqr(x, P), yy = fp_sqr(y, P);
        const bool on = fp_eq(fp_add(fp_mul(c.a, xx, P), yy, P), fp_add(fp_one(P), fp_mul(c.d, fp_mul(xx, yy, P), P), P));
        x = ed_pick(on, x, fp_zero<8>());
        y = ed_pick(on, y, fp_one(P));
    }
    const EdPoint r = ed_mul_body(ed_scalar_of(scalars[t], P), P.bits, x, y, c, P);
    ed_store_affine(r, shared + 2 * t, e_inv, P);
}

// keys[t] = hash3(shared[t].x, shared[t].y, 0)
__global__ void __launch_bounds__(CIRC_THREADS) edwards_dh_hash_kernel(const Fr* __restrict__ shared, uint64_t count, Fr* __restrict__ keys, const Fr* __restrict__ prm,
                                                                       const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    Fr s0 = shared[2 * t], s1 = shared[2 * t + 1], s2 = fp_zero<8>(), s3 = fp_zero<8>();
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    keys[t] = s0;
}

// ---------------------------------------------------------------------------------------------- launchers (enqueued on `stream`, not synchronised)
// L >= 1, 1 <= n_out <= 3, count >= 1; in: [count][L] Fr, out: [count][n_out] Fr
int rescue_sponge_run(int curve, const Fr* d_params, const Fr* d_in, uint64_t L, uint64_t count, unsigned n_out, Fr* d_out, hipStream_t stream, const char* who) {
    SolveExponent e;
    int rc = rescue_exponent(curve, &e, who);
    if (rc) return rc;
    uint32_t grid;
    if ((rc = rescue_acc_grid(count, who, &grid))) return rc;
    ProfScope ps("rescue_sponge", stream);
    hipLaunchKernelGGL(rescue_sponge_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_in, L, count, (uint32_t)n_out, d_out, d_params, e, fr_params(curve));
    return circ_launch_status("rescue_sponge");
}

// L >= 1, count >= 1; keys: [count] Fr; in, out: [count][L] Fr, out may be in
int rescue_stream_run(int curve, const Fr* d_params, const Fr* d_keys, const Fr* d_in, uint64_t L, uint64_t count, int decrypt, Fr* d_out, hipStream_t stream,
                      const char* who) {
    SolveExponent e;
    int rc = rescue_exponent(curve, &e, who);
    if (rc) return rc;
    const uint64_t nblocks = (L + 2) / 3;
    if (count > 0xFFFFFFFFFFFFFFFFull / nblocks)
        return plonk_fail(PLONK_ERR_ARG, "%s: count = %llu texts of L = %llu elements exceed one launch", who, (unsigned long long)count, (unsigned long long)L);
    uint32_t grid;
    if ((rc = rescue_acc_grid(count * nblocks, who, &grid))) return rc;
    ProfScope ps("rescue_stream", stream);
    hipLaunchKernelGGL(rescue_stream_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_keys, d_in, L, nblocks, count * nblocks, decrypt ? 1u : 0u, d_out, d_params, e,
                       fr_params(curve));
    return circ_launch_status("rescue_stream");
}

// count >= 1; params: HOST, the Edwards words; d_rescue: the Rescue tables on the device; d_shared: count points of working space
int edwards_dh_key_run(int curve, const uint64_t* params, const Fr* d_rescue, const Fr* d_scalars, const Fr* d_points, size_t count, Fr* d_keys, Fr* d_shared,
                       hipStream_t stream, const char* who) {
    SolveExponent e_root5;
    int rc = rescue_exponent(curve, &e_root5, who);
    if (rc) return rc;
    uint32_t grid;
    if ((rc = edwards_grid(count, who, &grid))) return rc;
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_dh_key", stream);
    hipLaunchKernelGGL(edwards_dh_point_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_scalars, d_points, (uint64_t)count, d_shared, h.c, h.e_inv, fr_params(curve));
    if ((rc = circ_launch_status("edwards_dh_point"))) return rc;
    hipLaunchKernelGGL(edwards_dh_hash_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, (const Fr*)d_shared, (uint64_t)count, d_keys, d_rescue, e_root5, fr_params(curve));
    return circ_launch_status("edwards_dh_hash");
}
