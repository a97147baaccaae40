// codec_kernels.hpp — ark-serialize 0.3 bytes <-> the library's Montgomery limbs on the device, included by synth.hip.  What `to_bytes!` writes
// for a G1Affine (compressed: x little-endian with two flag bits in the last byte; uncompressed: x then y) and for an Fr (32 bytes
// little-endian, canonical) is read and written here, one lane per element, no dependence between elements:
//   g1_decode_kernel     bytes -> x || y Montgomery (2Q u64, (0, 0) = infinity).  Compressed: y = (x^3 + b)^((q+1)/4) (both base fields have
//                        q = 3 mod 4; fp_sqrt_3mod4 of fp.hpp, ~1.4 products per bit), one squaring to test it, the sign from the flag.
//   g1_subgroup_kernel   BLS12-381, on request, after the decode: [r] P == O, the loop of verify_subgroup_kernel as a __device__ body
//   g1_encode_kernel     the inverse: vfy::append_g1 writing to memory instead of a transcript
//   fr_decode_kernel / fr_encode_kernel
//   proof_layout_kernel  the four Vec length prefixes of a serialized Proof (5, 5, 5, 4)
//   codec_first_bad_kernel   the lowest index with a non-zero status word
// Every element is addressed as  base + o * stride + j * inner_stride  with i = o * inner + j (CodecShape): a plain strided array has
// inner = 1; the 13 points and 10 scalars of a proof record are four launches with inner = 6, 7, 5, 5.  Bytes are loaded and stored one at
// a time: a stride need not be a multiple of 4.  A bad element is a bit OR-ed into its status word (atomicOr: the elements of one record may
// share a word) and (0, 0) — or 0 — in the output, never an error.
#pragma once
#include "constants.h"
#include "ec.hpp"
#include "verify_kernels.hpp"

namespace codec {

enum : uint32_t { ST_NO_POINT = 1, ST_SUBGROUP = 2, ST_NONCANONICAL = 8, ST_LAYOUT = 16 };      // 1, 2, 8: the meanings of vfy::ST_*
constexpr uint8_t FLAG_SIGN = 0x80, FLAG_INF = 0x40;

template <int N> __device__ __forceinline__ Fp<N> load_le(const uint8_t* s) {
    Fp<N> r;
#pragma unroll
    for (int i = 0; i < N; i++)
        r.l[i] = (uint32_t)s[4 * i] | ((uint32_t)s[4 * i + 1] << 8) | ((uint32_t)s[4 * i + 2] << 16) | ((uint32_t)s[4 * i + 3] << 24);
    return r;
}
template <int N> __device__ __forceinline__ void store_le(uint8_t* d, const Fp<N>& v, uint8_t flags) {
#pragma unroll
    for (int i = 0; i < 4 * N; i++) {
        uint8_t b = (uint8_t)(v.l[i >> 2] >> (8 * (i & 3)));
        if (i == 4 * N - 1) b |= flags;
        d[i] = b;
    }
}
template <int N> __device__ __forceinline__ void store_limbs(uint64_t* d, const Fp<N>& v) {
#pragma unroll
    for (int i = 0; i < N / 2; i++) d[i] = (uint64_t)v.l[2 * i] | ((uint64_t)v.l[2 * i + 1] << 32);
}
template <int N> __device__ __forceinline__ Fp<N> load_limbs(const uint64_t* s) {
    Fp<N> r;
#pragma unroll
    for (int i = 0; i < N / 2; i++) {
        const uint64_t w = s[i];
        r.l[2 * i] = (uint32_t)w;
        r.l[2 * i + 1] = (uint32_t)(w >> 32);
    }
    return r;
}

// [r] P == O (P affine, not infinity): the loop of verify_subgroup_kernel
template <int NQ> __device__ bool g1_times_r_is_inf(const AffPt<NQ>& p, const FpParams<8>& R, const FpParams<NQ>& Q) {
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int bit = 255; bit >= 0; bit--) {
        acc = xyzz_dbl_cold(acc, Q);
        if ((R.p[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd_cold(acc, p, Q);
    }
    return xyzz_is_inf(acc);
}

// y as ark-ff orders it: is the canonical integer of y (Montgomery in) the larger of {y, q - y}
template <int N> __device__ __forceinline__ bool y_is_larger(const Fp<N>& y_mont, const FpParams<N>& Q) {
    const Fp<N> y = fp_from_mont(y_mont, Q);
    const Fp<N> ny = fp_neg(y, Q);
    return vfy::lt_mod<N>(ny.l, y.l);
}

}  // namespace codec

// ------------------------------------------------------------------------------------------------ G1
// (kernels at global scope, like every other kernel of the library: codehash.py keys the machine code by kernel name)
template <int NQ>
__global__ void __launch_bounds__(128) g1_decode_kernel(const uint8_t* __restrict__ bytes, uint64_t* __restrict__ out, uint32_t* __restrict__ status,
                                                        const CodecShape s, int uncompressed, const FpParams<NQ> Q, const Fp<NQ> b) {
    using namespace codec;
    const uint64_t i = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= s.count) return;
    const uint64_t o = i / s.inner, j = i % s.inner;
    const uint8_t* src = bytes + o * s.in_stride + j * s.in_inner;
    uint64_t* dst = out + o * s.out_stride + j * s.out_inner;
    Fp<NQ> x = load_le<NQ>(src), y = fp_zero<NQ>();
    if (uncompressed) y = load_le<NQ>(src + 4 * NQ);
    const uint32_t flags = (uncompressed ? y.l[NQ - 1] : x.l[NQ - 1]) >> 30;      // of the last byte; bit 1: sign, bit 0: infinity
    if (uncompressed) y.l[NQ - 1] &= 0x3FFFFFFFu;
    else x.l[NQ - 1] &= 0x3FFFFFFFu;
    const bool sign = flags & 2, inf = flags & 1;
    uint32_t st = 0;
    AffPt<NQ> p;
    p.x = fp_zero<NQ>();
    p.y = fp_zero<NQ>();
    if ((sign && inf) || (sign && uncompressed)) st = ST_NONCANONICAL;
    else if (inf) {
        if (!fp_is_zero(x) || !fp_is_zero(y)) st = ST_NONCANONICAL;
    } else if (!vfy::lt_mod<NQ>(x.l, Q.p) || !vfy::lt_mod<NQ>(y.l, Q.p)) st = ST_NONCANONICAL;
    else {
        const Fp<NQ> xm = fp_to_mont(x, Q);
        const Fp<NQ> rhs = fp_add(fp_mul(fp_sqr(xm, Q), xm, Q), b, Q);
        Fp<NQ> ym = uncompressed ? fp_to_mont(y, Q) : fp_sqrt_3mod4(rhs, Q);
        if (!fp_eq(fp_sqr(ym, Q), rhs)) st = ST_NO_POINT;
        else {
            if (!uncompressed && y_is_larger(ym, Q) != sign) ym = fp_neg(ym, Q);
            p.x = xm;
            p.y = ym;
        }
    }
    store_limbs<NQ>(dst, p.x);
    store_limbs<NQ>(dst + NQ / 2, p.y);
    if (st) atomicOr(status + o * s.status_stride, st);
}

// BLS12-381, on request: the decoded points once more, one lane per point; a point outside the r-subgroup becomes (0, 0) and status 2.  Its
// own launch: the out-of-line point operations cost the caller 248 VGPRs and a stack frame (as in verify_subgroup_kernel), which the power
// above — 100 / 150 VGPRs, no scratch — should not pay for when the check is not asked for, or on BN254.
template <int NQ>
__global__ void __launch_bounds__(128) g1_subgroup_kernel(uint64_t* __restrict__ out, uint32_t* __restrict__ status, const CodecShape s, const FpParams<8> R,
                                                          const FpParams<NQ> Q) {
    using namespace codec;
    const uint64_t i = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    if (i >= s.count) return;
    const uint64_t o = i / s.inner, j = i % s.inner;
    uint64_t* dst = out + o * s.out_stride + j * s.out_inner;
    AffPt<NQ> p;
    p.x = load_limbs<NQ>(dst);
    p.y = load_limbs<NQ>(dst + NQ / 2);
    if (aff_is_inf(p) || g1_times_r_is_inf(p, R, Q)) return;
    store_limbs<NQ>(dst, fp_zero<NQ>());
    store_limbs<NQ>(dst + NQ / 2, fp_zero<NQ>());
    atomicOr(status + o * s.status_stride, (uint32_t)ST_SUBGROUP);
}

template <int NQ>
__global__ void __launch_bounds__(256) g1_encode_kernel(const uint64_t* __restrict__ in, uint8_t* __restrict__ bytes, const CodecShape s, int uncompressed,
                                                        const FpParams<NQ> Q) {
    using namespace codec;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.count) return;
    const uint64_t o = i / s.inner, j = i % s.inner;
    const uint64_t* src = in + o * s.in_stride + j * s.in_inner;
    uint8_t* dst = bytes + o * s.out_stride + j * s.out_inner;
    AffPt<NQ> p;
    p.x = load_limbs<NQ>(src);
    p.y = load_limbs<NQ>(src + NQ / 2);
    const bool inf = aff_is_inf(p);
    const Fp<NQ> x = fp_from_mont(p.x, Q);                      // (0, 0) stays (0, 0)
    if (uncompressed) {
        store_le<NQ>(dst, x, 0);
        store_le<NQ>(dst + 4 * NQ, fp_from_mont(p.y, Q), inf ? FLAG_INF : 0);
    } else {
        store_le<NQ>(dst, x, inf ? FLAG_INF : (y_is_larger(p.y, Q) ? FLAG_SIGN : 0));
    }
}

// ------------------------------------------------------------------------------------------------ Fr
__global__ void __launch_bounds__(256) fr_decode_kernel(const uint8_t* __restrict__ bytes, uint64_t* __restrict__ out, uint32_t* __restrict__ status,
                                                        const CodecShape s, const FpParams<8> R) {
    using namespace codec;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.count) return;
    const uint64_t o = i / s.inner, j = i % s.inner;
    const Fr v = load_le<8>(bytes + o * s.in_stride + j * s.in_inner);
    const bool ok = vfy::lt_mod<8>(v.l, R.p);
    store_limbs<8>(out + o * s.out_stride + j * s.out_inner, ok ? fp_to_mont(v, R) : fp_zero<8>());
    if (!ok) atomicOr(status + o * s.status_stride, (uint32_t)ST_NONCANONICAL);
}

__global__ void __launch_bounds__(256) fr_encode_kernel(const uint64_t* __restrict__ in, uint8_t* __restrict__ bytes, const CodecShape s, const FpParams<8> R) {
    using namespace codec;
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= s.count) return;
    const uint64_t o = i / s.inner, j = i % s.inner;
    store_le<8>(bytes + o * s.out_stride + j * s.out_inner, fp_from_mont(load_limbs<8>(in + o * s.in_stride + j * s.in_inner), R), 0);
}

// ------------------------------------------------------------------------------------------------ Proof layout, first bad index
// the u64 little-endian lengths of wires_poly_comms, split_quot_poly_comms, wires_evals and wire_sigma_evals (transcript.serialize_proof)
__global__ void __launch_bounds__(256) proof_layout_kernel(const uint8_t* __restrict__ bytes, uint64_t rec_bytes, uint32_t point_bytes, uint64_t k,
                                                           uint32_t* __restrict__ status) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const uint8_t* rec = bytes + i * rec_bytes;
    const uint32_t off[4] = {0, 8 + 6 * point_bytes, 16 + 13 * point_bytes, 16 + 13 * point_bytes + 8 + 5 * 32};
    const uint32_t want[4] = {5, 5, 5, 4};
    bool ok = true;
#pragma unroll
    for (int f = 0; f < 4; f++) {
        uint64_t v = 0;
#pragma unroll
        for (int t = 0; t < 8; t++) v |= (uint64_t)rec[off[f] + t] << (8 * t);
        ok = ok && v == want[f];
    }
    if (!ok) atomicOr(status + i, (uint32_t)codec::ST_LAYOUT);
}

__global__ void __launch_bounds__(256) codec_first_bad_kernel(const uint32_t* __restrict__ status, uint64_t count, uint64_t status_stride,
                                                              unsigned long long* __restrict__ first) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    if (status[i * status_stride]) atomicMin(first, (unsigned long long)i);
}

// ------------------------------------------------------------------------------------------------ launchers (plonk_internal.hpp)
namespace codec {
inline int launched(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return PLONK_OK;
}
inline uint32_t grid_of(uint64_t count, uint32_t lanes) { return (uint32_t)((count + lanes - 1) / lanes); }
}  // namespace codec

int codec_g1_decode_run(int curve, const void* d_bytes, void* d_out, void* d_status, const CodecShape& s, int uncompressed, int check_subgroup,
                        hipStream_t stream, const char* who) {
    if (curve == PLONK_BN254) {                   // cofactor 1: on the curve is in the group
        hipLaunchKernelGGL(g1_decode_kernel<8>, dim3(codec::grid_of(s.count, 128)), dim3(128), 0, stream, (const uint8_t*)d_bytes, (uint64_t*)d_out,
                           (uint32_t*)d_status, s, uncompressed, BN254_FQ_PARAMS, fp_from_limbs<8>(BN254_G1_B_MONT));
    } else {
        hipLaunchKernelGGL(g1_decode_kernel<12>, dim3(codec::grid_of(s.count, 128)), dim3(128), 0, stream, (const uint8_t*)d_bytes, (uint64_t*)d_out,
                           (uint32_t*)d_status, s, uncompressed, BLS12_381_FQ_PARAMS, fp_from_limbs<12>(BLS12_381_G1_B_MONT));
        if (check_subgroup)
            hipLaunchKernelGGL(g1_subgroup_kernel<12>, dim3(codec::grid_of(s.count, 128)), dim3(128), 0, stream, (uint64_t*)d_out, (uint32_t*)d_status, s,
                               BLS12_381_FR_PARAMS, BLS12_381_FQ_PARAMS);
    }
    return codec::launched(who);
}

int codec_g1_encode_run(int curve, const void* d_xy, void* d_bytes, const CodecShape& s, int uncompressed, hipStream_t stream, const char* who) {
    if (curve == PLONK_BN254)
        hipLaunchKernelGGL(g1_encode_kernel<8>, dim3(codec::grid_of(s.count, 256)), dim3(256), 0, stream, (const uint64_t*)d_xy, (uint8_t*)d_bytes, s,
                           uncompressed, BN254_FQ_PARAMS);
    else
        hipLaunchKernelGGL(g1_encode_kernel<12>, dim3(codec::grid_of(s.count, 256)), dim3(256), 0, stream, (const uint64_t*)d_xy, (uint8_t*)d_bytes, s,
                           uncompressed, BLS12_381_FQ_PARAMS);
    return codec::launched(who);
}

int codec_fr_decode_run(int curve, const void* d_bytes, void* d_out, void* d_status, const CodecShape& s, hipStream_t stream, const char* who) {
    hipLaunchKernelGGL(fr_decode_kernel, dim3(codec::grid_of(s.count, 256)), dim3(256), 0, stream, (const uint8_t*)d_bytes, (uint64_t*)d_out,
                       (uint32_t*)d_status, s, fr_params(curve));
    return codec::launched(who);
}

int codec_fr_encode_run(int curve, const void* d_fr, void* d_bytes, const CodecShape& s, hipStream_t stream, const char* who) {
    hipLaunchKernelGGL(fr_encode_kernel, dim3(codec::grid_of(s.count, 256)), dim3(256), 0, stream, (const uint64_t*)d_fr, (uint8_t*)d_bytes, s,
                       fr_params(curve));
    return codec::launched(who);
}

size_t codec_proof_bytes(int curve) { return 13 * (curve == PLONK_BN254 ? 32 : 48) + 352; }

// k serialized proofs -> k records of plonk_verify_batch_dev and one status word each: two point launches (the points before and after the
// second Vec prefix), two scalar launches, the layout check
int codec_proofs_run(int curve, const void* d_bytes, size_t k, void* d_proofs, void* d_status, hipStream_t stream, const char* who) {
    const uint64_t nb = curve == PLONK_BN254 ? 32 : 48, q2 = nb / 4, rec_in = codec_proof_bytes(curve), rec_out = 13 * q2 + 40;
    const uint8_t* in = (const uint8_t*)d_bytes;
    uint64_t* out = (uint64_t*)d_proofs;
    HIP_TRY(hipMemsetAsync(d_status, 0, k * sizeof(uint32_t), stream));
    const uint64_t evals = 16 + 13 * nb;
    int rc = codec_g1_decode_run(curve, in + 8, out, d_status, CodecShape{k * 6, 6, rec_in, nb, rec_out, q2, 1}, 0, 1, stream, who);
    if (!rc) rc = codec_g1_decode_run(curve, in + 16 + 6 * nb, out + 6 * q2, d_status, CodecShape{k * 7, 7, rec_in, nb, rec_out, q2, 1}, 0, 1, stream, who);
    if (!rc) rc = codec_fr_decode_run(curve, in + evals + 8, out + 13 * q2, d_status, CodecShape{k * 5, 5, rec_in, 32, rec_out, 4, 1}, stream, who);
    if (!rc) rc = codec_fr_decode_run(curve, in + evals + 16 + 5 * 32, out + 13 * q2 + 20, d_status, CodecShape{k * 5, 5, rec_in, 32, rec_out, 4, 1}, stream, who);
    if (rc) return rc;
    hipLaunchKernelGGL(proof_layout_kernel, dim3(codec::grid_of(k, 256)), dim3(256), 0, stream, in, rec_in, (uint32_t)nb, (uint64_t)k, (uint32_t*)d_status);
    return codec::launched(who);
}

int codec_first_bad_run(const void* d_status, size_t count, size_t status_stride, unsigned long long* d_first, hipStream_t stream, const char* who) {
    hipLaunchKernelGGL(codec_first_bad_kernel, dim3(codec::grid_of(count, 256)), dim3(256), 0, stream, (const uint32_t*)d_status, (uint64_t)count,
                       (uint64_t)status_stride, d_first);
    return codec::launched(who);
}
