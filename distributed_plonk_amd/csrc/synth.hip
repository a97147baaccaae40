// synth.hip — small element-wise device kernels around the hot path:
//   * into_repr over a coefficient vector (commit_polynomial, worker.rs:118)
//   * element-wise field ops for pinning the arithmetic layer against the oracle
//   * seeded synthetic inputs (the reference draws from thread_rng: dispatcher.rs:187-200):
//     uniform Fr, and SRS-like G1 bases (k_j*G tiled, or pairwise-distinct sums A_i + B_j)
#include "constants.h"
#include "ec.hpp"
#include "plonk_internal.hpp"

template <int N> static const FpParams<N>& field_params(int curve, int field);
template <> const FpParams<8>& field_params<8>(int curve, int field) {
    if (field == 0) return curve == PLONK_BN254 ? BN254_FR_PARAMS : BLS12_381_FR_PARAMS;
    return BN254_FQ_PARAMS;
}
template <> const FpParams<12>& field_params<12>(int, int) { return BLS12_381_FQ_PARAMS; }

template <typename T> __device__ __forceinline__ T ld16(const T* p) {
    T r;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
    return r;
}
template <typename T> __device__ __forceinline__ void st16(T* p, const T& v) {
    uint4* d = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

// ---------------------------------------------------------------------------------------------- field ops
template <int N>
__global__ void __launch_bounds__(256) field_op_kernel(int op, const Fp<N>* __restrict__ a, const Fp<N>* __restrict__ b, Fp<N>* __restrict__ out,
                                                       uint64_t n, const FpParams<N> P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Fp<N> x = ld16(a + i), y = b ? ld16(b + i) : x, r;
    switch (op) {
        case 0: r = fp_mul(x, y, P); break;
        case 1: r = fp_add(x, y, P); break;
        case 2: r = fp_sub(x, y, P); break;
        case 3: r = fp_to_mont(x, P); break;
        case 4: r = fp_from_mont(x, P); break;
        case 5: r = fp_inv(x, P); break;
        default: r = fp_sqr(x, P); break;
    }
    st16(out + i, r);
}

int field_op_dev(int curve, int field, int op, const void* a, const void* b, void* out, size_t n, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    if (op < 0 || op > 6) return plonk_fail(PLONK_ERR_ARG, "field op %d", op);
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (field == 1 && curve == PLONK_BLS12_381)
        hipLaunchKernelGGL(field_op_kernel<12>, dim3(grid), dim3(256), 0, stream, op, (const Fp<12>*)a, (const Fp<12>*)b, (Fp<12>*)out, (uint64_t)n,
                           field_params<12>(curve, field));
    else
        hipLaunchKernelGGL(field_op_kernel<8>, dim3(grid), dim3(256), 0, stream, op, (const Fp<8>*)a, (const Fp<8>*)b, (Fp<8>*)out, (uint64_t)n,
                           field_params<8>(curve, field));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "field_op launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

int fr_from_mont_dev(int curve, const Fr* in, Fr* out, size_t n, hipStream_t stream) {
    return field_op_dev(curve, 0, 4, in, nullptr, out, n, stream);
}

// ---------------------------------------------------------------------------------------------- synthetic Fr
__device__ __forceinline__ uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// Fp::rand of ark-ff 0.3.0: draw limbs, mask the top REPR_SHAVE_BITS, accept if < p; the accepted
// raw limbs are the Montgomery representation.  Element i has its own stream (seed, i).
__device__ __forceinline__ Fr rand_fr_elem(uint64_t seed, uint64_t i, const FrParams& P) {
    uint64_t s = seed ^ (0xD1B54A32D192ED03ull * (i + 1));
    const int shave = 256 - P.bits;
    Fr r;
    for (;;) {
        uint64_t l[4];
        for (int k = 0; k < 4; k++) l[k] = splitmix64(s);
        l[3] &= (~0ull) >> shave;
#pragma unroll
        for (int k = 0; k < 4; k++) { r.l[2 * k] = (uint32_t)l[k]; r.l[2 * k + 1] = (uint32_t)(l[k] >> 32); }
        // accept if r < p
        uint64_t br = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) { uint64_t t = (uint64_t)r.l[k] - P.p[k] - br; br = (t >> 32) & 1; }
        if (br) break;
    }
    return r;
}

__global__ void __launch_bounds__(256) synth_fr_kernel(uint64_t seed, Fr* __restrict__ out, uint64_t n, const FrParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st16(out + i, rand_fr_elem(seed, i, P));
}

int synth_fr_dev(int curve, uint64_t seed, Fr* out, size_t n, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    hipLaunchKernelGGL(synth_fr_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, seed, out, (uint64_t)n, fr_params(curve));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "synth_fr launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

// ---------------------------------------------------------------------------------------------- synthetic bases
// P_j = k_j * G with k_j = the raw limbs of rand_fr(seed)[j] (same rule as oracle orc_gen_bases)
template <int NQ>
__global__ void __launch_bounds__(64) synth_points_kernel(uint64_t seed, uint64_t count, AffPt<NQ>* __restrict__ out, const AffPt<NQ> G,
                                                          const FrParams FR, const FpParams<NQ> P) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    const Fr k = rand_fr_elem(seed, j, FR);
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int i = 255; i >= 0; i--) {
        acc = xyzz_dbl_cold(acc, P);
        if ((k.l[i >> 5] >> (i & 31)) & 1) acc = xyzz_madd_cold(acc, G, P);
    }
    st16(out + j, xyzz_to_affine(acc, P));
}

template <int NQ>
__global__ void __launch_bounds__(256) synth_tile_kernel(AffPt<NQ>* __restrict__ pts, uint64_t unique, uint64_t n) {
    const uint64_t i = unique + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    st16(pts + i, ld16(pts + (i % unique)));
}

// P_i = A[i % na] + B[i / na]
template <int NQ>
__global__ void __launch_bounds__(128) synth_sum_kernel(const AffPt<NQ>* __restrict__ A, uint64_t na, const AffPt<NQ>* __restrict__ B,
                                                        AffPt<NQ>* __restrict__ out, uint64_t n, const FpParams<NQ> P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    XyzzPt<NQ> a = xyzz_from_affine(ld16(A + (i % na)), P);
    a = xyzz_madd_cold(a, ld16(B + (i / na)), P);
    st16(out + i, xyzz_to_affine(a, P));
}

template <int NQ> static AffPt<NQ> generator_affine(int curve);
template <> AffPt<8> generator_affine<8>(int) {
    AffPt<8> g;
    g.x = fp_from_limbs<8>(BN254_G1_GX_MONT); g.y = fp_from_limbs<8>(BN254_G1_GY_MONT);
    return g;
}
template <> AffPt<12> generator_affine<12>(int) {
    AffPt<12> g;
    g.x = fp_from_limbs<12>(BLS12_381_G1_GX_MONT); g.y = fp_from_limbs<12>(BLS12_381_G1_GY_MONT);
    return g;
}

template <int NQ>
static int synth_bases_t(int curve, uint64_t seed, size_t unique, size_t n, void* d_out, hipStream_t stream) {
    const FpParams<NQ>& P = field_params<NQ>(curve, 1);
    AffPt<NQ>* out = (AffPt<NQ>*)d_out;
    if (unique > n) unique = n;
    hipLaunchKernelGGL(synth_points_kernel<NQ>, dim3((uint32_t)((unique + 63) / 64)), dim3(64), 0, stream, seed, (uint64_t)unique, out,
                       generator_affine<NQ>(curve), fr_params(curve), P);
    if (n > unique)
        hipLaunchKernelGGL(synth_tile_kernel<NQ>, dim3((uint32_t)((n - unique + 255) / 256)), dim3(256), 0, stream, out, (uint64_t)unique, (uint64_t)n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "synth_bases launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

int synth_bases_dev(int curve, uint64_t seed, size_t unique, size_t n, void* d_out, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    if (curve == PLONK_BN254) return synth_bases_t<8>(curve, seed, unique, n, d_out, stream);
    return synth_bases_t<12>(curve, seed, unique, n, d_out, stream);
}

template <int NQ>
static int synth_distinct_t(int curve, uint64_t seed, size_t n, void* d_out, hipStream_t stream) {
    const FpParams<NQ>& P = field_params<NQ>(curve, 1);
    const size_t na = 4096, nbb = (n + na - 1) / na;
    AffPt<NQ>* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&tmp, (na + nbb) * sizeof(AffPt<NQ>)));
    int rc = synth_bases_t<NQ>(curve, seed, na, na, tmp, stream);
    if (!rc) rc = synth_bases_t<NQ>(curve, seed + 1, nbb, nbb, tmp + na, stream);
    if (!rc) {
        hipLaunchKernelGGL(synth_sum_kernel<NQ>, dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, stream, tmp, (uint64_t)na, tmp + na,
                           (AffPt<NQ>*)d_out, (uint64_t)n, P);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = plonk_fail(PLONK_ERR_HIP, "synth_sum launch: %s", hipGetErrorString(e));
    }
    (void)hipStreamSynchronize(stream);
    (void)hipFree(tmp);
    return rc;
}

int synth_bases_distinct_dev(int curve, uint64_t seed, size_t n, void* d_out, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    if (curve == PLONK_BN254) return synth_distinct_t<8>(curve, seed, n, d_out, stream);
    return synth_distinct_t<12>(curve, seed, n, d_out, stream);
}

// ---------------------------------------------------------------------------------------------- trapdoor SRS
// P_i = tau^i * G, i < n: a KZG commit key whose trapdoor the test knows (the reference's universal_setup draws tau from rng and
// forgets it, dispatcher2.rs:1278).  With it commit(f) = f(tau) * G, and the verifier's pairing check becomes an equation in G1
// (oracle/verifier_ref.py) — which is what lets bench.py verify a whole 2^24-gate proof.  Fixed-base, 8-bit windows: a table
// T[w][b] = b * 2^(8w) * G (32 x 256 affine points) and at most 32 mixed additions + one inversion per point.
template <int NQ>
__global__ void __launch_bounds__(64) srs_table_kernel(AffPt<NQ>* __restrict__ table, const AffPt<NQ> G, const FpParams<NQ> P) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;      // e = w * 256 + b
    if (e >= 32 * 256) return;
    const uint32_t w = e >> 8, b = e & 255;
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int i = 7; i >= 0; i--) {
        acc = xyzz_dbl_cold(acc, P);
        if ((b >> i) & 1) acc = xyzz_madd_cold(acc, G, P);
    }
    for (uint32_t i = 0; i < 8 * w; i++) acc = xyzz_dbl_cold(acc, P);
    st16(table + e, xyzz_to_affine(acc, P));
}

template <int NQ>
__global__ void __launch_bounds__(128) srs_points_kernel(const AffPt<NQ>* __restrict__ table, const Fr tau, uint64_t n, AffPt<NQ>* __restrict__ out,
                                                         const FrParams FR, const FpParams<NQ> P) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Fr s = fp_from_mont(fp_pow_u64(tau, i, FR), FR);          // tau^i, canonical
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int w = 0; w < 32; w++) {
        const uint32_t b = (s.l[w >> 2] >> ((w & 3) * 8)) & 255;
        if (b) acc = xyzz_madd_cold(acc, ld16(table + w * 256 + b), P);
    }
    st16(out + i, xyzz_to_affine(acc, P));
}

template <int NQ>
static int synth_srs_t(int curve, const Fr& tau, size_t n, void* d_out, hipStream_t stream) {
    const FpParams<NQ>& P = field_params<NQ>(curve, 1);
    AffPt<NQ>* table = nullptr;
    HIP_TRY(hipMalloc((void**)&table, 32 * 256 * sizeof(AffPt<NQ>)));
    hipLaunchKernelGGL(srs_table_kernel<NQ>, dim3(32 * 256 / 64), dim3(64), 0, stream, table, generator_affine<NQ>(curve), P);
    hipLaunchKernelGGL(srs_points_kernel<NQ>, dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, stream, table, tau, (uint64_t)n, (AffPt<NQ>*)d_out,
                       fr_params(curve), P);
    hipError_t e = hipGetLastError();
    const hipError_t es = hipStreamSynchronize(stream);       // the table must outlive both kernels; a fault inside them surfaces here
    (void)hipFree(table);
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "synth_srs launch: %s", hipGetErrorString(e));
    if (es != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "synth_srs: %s", hipGetErrorString(es));
    return PLONK_OK;
}

int synth_srs_dev(int curve, const uint64_t* tau_mont, size_t n, void* d_out, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    const Fr tau = fp_from_limbs<8>((const uint32_t*)tau_mont);
    if (curve == PLONK_BN254) return synth_srs_t<8>(curve, tau, n, d_out, stream);
    return synth_srs_t<12>(curve, tau, n, d_out, stream);
}

// ---------------------------------------------------------------------------------------------- a random SATISFIED circuit
// The reference's generate_circuit (dispatcher2.rs:1214-1270) builds a Merkle-membership circuit with jellyfish, which is not
// available here; north_star asks for synthetic random circuits.  One lane per gate j:
//   * wiring: column i of gate j reads variable P_i(j), P_i a seeded bijection of [0, n) (xor-shift, odd multiplier, offset), so
//     every variable occurs once per column and the copy constraints are n cycles of length 5 that hop between pseudo-random
//     gates: (i, j) -> (i+1, P_{i+1}^-1(P_i(j)));
//   * witness: value(v) = rand_fr(seed, v); wires[i][j] = value(P_i(j)) — equal along every cycle by construction;
//   * selectors: 12 of the 13 are uniform random, q_c is solved so the gate equation of dispatcher2.rs:465-477 holds;
//   * public input: uniform on the first num_inputs gates, zero elsewhere (part of the solved equation);
//   * id_perm[i*n + j] = k_i * w^j (extended_id_permutation), sigma evaluations = id_perm[perm_idx] written directly.
struct CircuitSynthParams {
    uint64_t seed, n, num_inputs;
    uint32_t log_n, shift;
    uint64_t mul[5], mul_inv[5], off[5];
    Fr k[5];
    Fr omega;
};
__device__ __forceinline__ uint64_t cs_fwd(const CircuitSynthParams& c, int i, uint64_t j) {
    const uint64_t mask = c.n - 1;
    j ^= j >> c.shift;
    return (j * c.mul[i] + c.off[i]) & mask;
}
__device__ __forceinline__ uint64_t cs_inv(const CircuitSynthParams& c, int i, uint64_t v) {
    const uint64_t mask = c.n - 1;
    uint64_t j = ((v - c.off[i]) * c.mul_inv[i]) & mask;
    return j ^ (j >> c.shift);                  // 2 * shift >= log n: the xor-shift is an involution
}

__global__ void __launch_bounds__(128) synth_circuit_kernel(const CircuitSynthParams c, Fr* __restrict__ wires, Fr* __restrict__ sel, Fr* __restrict__ sigma,
                                                            Fr* __restrict__ id_perm, uint64_t* __restrict__ perm_idx, Fr* __restrict__ pub,
                                                            const FrParams P) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= c.n) return;
    Fr w[5];
    const Fr wj = fp_pow_u64(c.omega, j, P);
    for (int i = 0; i < 5; i++) {
        const uint64_t v = cs_fwd(c, i, j);
        w[i] = rand_fr_elem(c.seed, v, P);
        st16(wires + i * c.n + j, w[i]);
        const int i2 = i == 4 ? 0 : i + 1;
        const uint64_t j2 = cs_inv(c, i2, v);
        perm_idx[i * c.n + j] = (uint64_t)i2 * c.n + j2;
        st16(id_perm + i * c.n + j, fp_mul(c.k[i], wj, P));
        st16(sigma + i * c.n + j, fp_mul(c.k[i2], fp_pow_u64(c.omega, j2, P), P));
    }
    Fr q[13];
    for (int t = 0; t < 13; t++) q[t] = rand_fr_elem(c.seed + 0x1000 + t, j, P);
    const Fr pi = j < c.num_inputs ? rand_fr_elem(c.seed + 0x2000, j, P) : fp_zero<8>();
    const Fr ab = fp_mul(w[0], w[1], P), cd = fp_mul(w[2], w[3], P);
    Fr acc = pi;
    for (int t = 0; t < 4; t++) {
        acc = fp_add(acc, fp_mul(q[t], w[t], P), P);                                  // q_lc
        const Fr w2 = fp_sqr(w[t], P);
        acc = fp_add(acc, fp_mul(q[6 + t], fp_mul(fp_sqr(w2, P), w[t], P), P), P);    // q_hash * w^5
    }
    acc = fp_add(acc, fp_mul(q[4], ab, P), P);                                        // q_mul
    acc = fp_add(acc, fp_mul(q[5], cd, P), P);
    acc = fp_add(acc, fp_mul(q[12], fp_mul(fp_mul(ab, cd, P), w[4], P), P), P);       // q_ecc * abcde
    acc = fp_sub(acc, fp_mul(q[10], w[4], P), P);                                     // - q_o * e
    q[11] = fp_neg(acc, P);                                                           // q_c
    for (int t = 0; t < 13; t++) st16(sel + t * c.n + j, q[t]);
    st16(pub + j, pi);
}

static uint64_t inv_odd_u64(uint64_t a) {        // a^-1 mod 2^64 by Newton iteration
    uint64_t x = a;
    for (int i = 0; i < 6; i++) x *= 2 - a * x;
    return x;
}
static uint64_t host_splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int synth_circuit_dev(int curve, uint64_t seed, size_t n, size_t num_inputs, const uint64_t* k_mont, const Fr& omega_n, void* d_wires, void* d_sel,
                      void* d_sigma, void* d_id_perm, void* d_perm_idx, void* d_pub, hipStream_t stream) {
    CircuitSynthParams c;
    c.seed = seed; c.n = n; c.num_inputs = num_inputs;
    c.log_n = 0;
    while (((size_t)1 << c.log_n) < n) c.log_n++;
    c.shift = c.log_n ? (c.log_n + 1) / 2 : 1;
    uint64_t s = seed ^ 0xC1C5EEDull;
    for (int i = 0; i < 5; i++) {
        c.mul[i] = host_splitmix(s) | 1;
        c.mul_inv[i] = inv_odd_u64(c.mul[i]);
        c.off[i] = host_splitmix(s);
        c.k[i] = fp_from_limbs<8>((const uint32_t*)(k_mont + 4 * i));
    }
    c.omega = omega_n;
    hipLaunchKernelGGL(synth_circuit_kernel, dim3((uint32_t)((n + 127) / 128)), dim3(128), 0, stream, c, (Fr*)d_wires, (Fr*)d_sel, (Fr*)d_sigma,
                       (Fr*)d_id_perm, (uint64_t*)d_perm_idx, (Fr*)d_pub, fr_params(curve));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "synth_circuit launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

// ---------------------------------------------------------------------------------------------- user circuits
// preprocessing of circuits given as gate wiring (jellyfish's arithmetised form): kernels and launchers live in their own header
#include "circuit_kernels.hpp"
// the witness of such a circuit solved level by level from the gates that define its variables
#include "solve_kernels.hpp"
// the Rescue permutation and Merkle trees over it, on the solver's fixed-exponent power
#include "rescue_kernels.hpp"
// the ternary accumulator over it, its membership paths, and the scatter that starts a solve from inputs on the device
#include "rescue_acc_kernels.hpp"
// the embedded twisted Edwards curve over Fr: scalar multiplication, addition and the curve / subgroup check, on the same power for the inversion
#include "edwards_kernels.hpp"
// the Rescue sponge and counter-mode stream, and the ElGamal shared key [scalar] point -> hash3: the two bodies above in one lane
#include "elgamal_kernels.hpp"

// ---------------------------------------------------------------------------------------------- batched proof verification
// the per-proof work of jf-plonk's verify / batch_verify up to the pairing: kernels and launcher in their own header
#include "verify_kernels.hpp"
// what a prover, a ceremony and a key file hand over is bytes: ark-serialize's G1 and Fr encodings read and written on the device
#include "codec_kernels.hpp"
// a KZG opening outside a proof -> its pair of the folded pairing check (plonk_kzg_pairs_dev), on vfy's point loads and status bits
#define KZG_KERNELS_POINTS
#include "kzg_kernels.hpp"
#undef KZG_KERNELS_POINTS
