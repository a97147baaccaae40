// edwards_kernels.hpp — the embedded twisted Edwards curve over Fr on the device (included by synth.hip after rescue_kernels.hpp; shares
// solve_pow_fixed and the inverse exponent r - 2 of solve_hints.hpp for the one inversion per result): the group that builder.py's point
// gadgets prove, computed in bulk.
//
//     E:  a x^2 + y^2 = 1 + d x^2 y^2   over Fr,   a a square, d a non-square (edwards.py refuses other parameters)
// so the addition law has no exceptional case on E: every denominator below is non-zero for curve points, doubling, inverses, the identity
// (0, 1) and the points of small order included.  Points cross the ABI affine, (x, y) = 2 Fr Montgomery; inside a kernel a point is extended,
// (X : Y : Z : T) with x = X / Z, y = Y / Z, T = X Y / Z:
//     add   (Hisil-Wong-Carter-Dawson 2008, unified, the second point affine: Z2 = 1, T2 = x2 y2)
//           A = X1 x2, B = Y1 y2, C = d T1 T2, E = (X1 + Y1)(x2 + y2) - A - B, F = Z1 - C, G = Z1 + C, H = B - a A
//           X3 = E F, Y3 = G H, T3 = E H, Z3 = F G                                   10 products (two of them by the constants a and d)
//     dbl   A = X1^2, B = Y1^2, C = 2 Z1^2, D = a A, E = (X1 + Y1)^2 - A - B, G = D + B, F = G - C, H = D - B
//           X3 = E F, Y3 = G H, T3 = E H, Z3 = F G                                    9 products
//     affine  zi = Z^(r - 2) (~335 products), x = X zi, y = Y zi
// A scalar is an Fr element and stands for its canonical residue k in [0, r): [k] P walks the bits of k from bit `nbits` - 1 down, doubling
// and then ALWAYS adding P, and keeps the sum where the bit is set — a select per limb, so the lanes of a wave never diverge and the trip
// count is the same for all of them: nbits (9 + 10) + 1 + 335 + 2 ~ 5.2 k products per [k] P at nbits = bit_length(r).  The bits come out of
// a shift register of 8 words, every index a constant: a word indexed by the loop counter would send the scalar to scratch memory, and a
// per-lane window table indexed by a per-lane digit would do the same to the table (rescue_kernels.hpp on both), so there is no window here.
//
// [k] G for the fixed generator reads a table in global memory instead: ED_WINDOWS = 64 windows of 4 bits, table[w][j] = [j 16^w] G affine for
// j = 0 .. 15 (j = 0 the identity: the addition is complete, so a zero digit needs no branch) — 64 x 16 x 64 B = 64 KB, built by
// edwards_table_kernel once per parameter set.  One lane gathers 64 entries and adds them: 64 x 11 + 335 + 2 ~ 1.0 k products.
#pragma once

constexpr int ED_WINDOW_BITS = 4;
constexpr int ED_WINDOWS = 64;                                       // 4 x 64 = 256 >= bit_length(r) on both fields
constexpr int ED_TABLE_POINTS = ED_WINDOWS << ED_WINDOW_BITS;        // 1024 affine points, 64 KB
constexpr int ED_PARAM_WORDS = 4 * 4 + 4;                            // a, d, G.x, G.y (Montgomery), then l as 4 plain u64

static_assert((size_t)ED_PARAM_WORDS == EDWARDS_PARAM_WORDS && (size_t)ED_TABLE_POINTS * 2 * sizeof(Fr) == EDWARDS_TABLE_BYTES, "plonk_internal.hpp's sizes");
static_assert(ED_TABLE_POINTS % CIRC_THREADS == 0, "the table kernel's grid");

struct EdCurve {
    Fr a, d;
};
struct EdScalar {
    uint32_t w[8];                                                   // a plain integer, little-endian
};
struct EdPoint {
    Fr X, Y, Z, T;
};

__device__ __forceinline__ Fr ed_pick(bool take, const Fr& yes, const Fr& no) {
    Fr r;
    const uint32_t m = take ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = (yes.l[i] & m) | (no.l[i] & ~m);
    return r;
}

__device__ __forceinline__ EdPoint ed_identity(const FrParams& P) {
    EdPoint r;
    r.X = fp_zero<8>(); r.Y = fp_one(P); r.Z = r.Y; r.T = r.X;
    return r;
}

// p + (x2, y2), t2 = x2 y2
__device__ __forceinline__ EdPoint ed_add_affine(const EdPoint& p, const Fr& x2, const Fr& y2, const Fr& t2, const EdCurve& c, const FrParams& P) {
    const Fr A = fp_mul(p.X, x2, P), B = fp_mul(p.Y, y2, P);
    const Fr C = fp_mul(c.d, fp_mul(p.T, t2, P), P);
    const Fr E = fp_sub(fp_sub(fp_mul(fp_add(p.X, p.Y, P), fp_add(x2, y2, P), P), A, P), B, P);
    const Fr F = fp_sub(p.Z, C, P), G = fp_add(p.Z, C, P), H = fp_sub(B, fp_mul(c.a, A, P), P);
    EdPoint r;
    r.X = fp_mul(E, F, P); r.Y = fp_mul(G, H, P); r.T = fp_mul(E, H, P); r.Z = fp_mul(F, G, P);
    return r;
}

__device__ __forceinline__ EdPoint ed_double(const EdPoint& p, const EdCurve& c, const FrParams& P) {
    const Fr A = fp_sqr(p.X, P), B = fp_sqr(p.Y, P), C = fp_dbl(fp_sqr(p.Z, P), P), D = fp_mul(c.a, A, P);
    const Fr E = fp_sub(fp_sub(fp_sqr(fp_add(p.X, p.Y, P), P), A, P), B, P);
    const Fr G = fp_add(D, B, P), F = fp_sub(G, C, P), H = fp_sub(D, B, P);
    EdPoint r;
    r.X = fp_mul(E, F, P); r.Y = fp_mul(G, H, P); r.T = fp_mul(E, H, P); r.Z = fp_mul(F, G, P);
    return r;
}

// [k] (x, y) for the low `nbits` bits of k, 1 <= nbits <= 256 and uniform over the grid
__device__ __forceinline__ EdPoint ed_mul_body(const EdScalar& k, int nbits, const Fr& x, const Fr& y, const EdCurve& c, const FrParams& P) {
    const Fr t = fp_mul(x, y, P);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = k.w[j];
#pragma unroll 1
    for (int s = 256 - nbits; s > 0; s--) {                          // bit nbits - 1 to the top of w[7]
#pragma unroll
        for (int j = 7; j > 0; j--) w[j] = (w[j] << 1) | (w[j - 1] >> 31);
        w[0] <<= 1;
    }
    EdPoint acc = ed_identity(P);
#pragma unroll 1
    for (int i = 0; i < nbits; i++) {
        const bool bit = (w[7] >> 31) != 0;
#pragma unroll
        for (int j = 7; j > 0; j--) w[j] = (w[j] << 1) | (w[j - 1] >> 31);
        w[0] <<= 1;
        acc = ed_double(acc, c, P);
        const EdPoint sum = ed_add_affine(acc, x, y, t, c, P);
        acc.X = ed_pick(bit, sum.X, acc.X);
        acc.Y = ed_pick(bit, sum.Y, acc.Y);
        acc.Z = ed_pick(bit, sum.Z, acc.Z);
        acc.T = ed_pick(bit, sum.T, acc.T);
    }
    return acc;
}

__device__ __forceinline__ EdScalar ed_scalar_of(const Fr& s, const FrParams& P) {
    const Fr plain = fp_from_mont(s, P);
    EdScalar k;
#pragma unroll
    for (int j = 0; j < 8; j++) k.w[j] = plain.l[j];
    return k;
}

__device__ __forceinline__ void ed_store_affine(const EdPoint& p, Fr* out, const SolveExponent& e_inv, const FrParams& P) {
    const Fr zi = solve_pow_fixed(p.Z, e_inv, P);
    out[0] = fp_mul(p.X, zi, P);
    out[1] = fp_mul(p.Y, zi, P);
}

// out[t] = [scalars[t]] points[t]; out may be points
__global__ void __launch_bounds__(CIRC_THREADS) edwards_mul_kernel(const Fr* __restrict__ scalars, const Fr* points, uint64_t count, Fr* out, const EdCurve c,
                                                                   const SolveExponent e_inv, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    const Fr x = points[2 * t], y = points[2 * t + 1];
    const EdPoint r = ed_mul_body(ed_scalar_of(scalars[t], P), P.bits, x, y, c, P);
    ed_store_affine(r, out + 2 * t, e_inv, P);
}

// table[w][j] = [j 16^w] (gx, gy), one lane per entry
__global__ void __launch_bounds__(CIRC_THREADS) edwards_table_kernel(Fr* __restrict__ table, const Fr gx, const Fr gy, const EdCurve c, const SolveExponent e_inv,
                                                                     const FrParams P) {
    const uint32_t t = blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= (uint32_t)ED_TABLE_POINTS) return;
    const uint32_t win = t >> ED_WINDOW_BITS, digit = t & ((1u << ED_WINDOW_BITS) - 1);
    EdScalar k;
#pragma unroll
    for (uint32_t j = 0; j < 8; j++) k.w[j] = (win >> 3) == j ? digit << (ED_WINDOW_BITS * (win & 7)) : 0u;      // a window never straddles a word
    const EdPoint r = ed_mul_body(k, 256, gx, gy, c, P);
    ed_store_affine(r, table + 2 * t, e_inv, P);
}

// out[t] = [scalars[t]] G from the table of G
__global__ void __launch_bounds__(CIRC_THREADS) edwards_fixed_mul_kernel(const Fr* __restrict__ scalars, uint64_t count, const Fr* __restrict__ table, Fr* __restrict__ out,
                                                                         const EdCurve c, const SolveExponent e_inv, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    const EdScalar k = ed_scalar_of(scalars[t], P);
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = k.w[j];
    EdPoint acc = ed_identity(P);
#pragma unroll 1
    for (uint32_t win = 0; win < (uint32_t)ED_WINDOWS; win++) {
        const uint32_t digit = w[0] & ((1u << ED_WINDOW_BITS) - 1);          // < 16: the entry lies inside the table whatever the scalar
#pragma unroll
        for (int j = 0; j < 7; j++) w[j] = (w[j] >> ED_WINDOW_BITS) | (w[j + 1] << (32 - ED_WINDOW_BITS));
        w[7] >>= ED_WINDOW_BITS;
        const Fr* e = table + 2 * ((win << ED_WINDOW_BITS) + digit);
        const Fr x = e[0], y = e[1];
        acc = ed_add_affine(acc, x, y, fp_mul(x, y, P), c, P);
    }
    ed_store_affine(acc, out + 2 * t, e_inv, P);
}

// out[t] = p[t] + q[t]; out may be p or q
__global__ void __launch_bounds__(CIRC_THREADS) edwards_add_kernel(const Fr* p, const Fr* q, uint64_t count, Fr* out, const EdCurve c, const SolveExponent e_inv,
                                                                   const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    EdPoint a;
    a.X = p[2 * t]; a.Y = p[2 * t + 1]; a.Z = fp_one(P); a.T = fp_mul(a.X, a.Y, P);
    const Fr x = q[2 * t], y = q[2 * t + 1];
    const EdPoint r = ed_add_affine(a, x, y, fp_mul(x, y, P), c, P);
    ed_store_affine(r, out + 2 * t, e_inv, P);
}

// flags[t]: bit 0 the point satisfies the curve equation; bit 1 it does and [l] point is the identity (X = 0 and Y = Z)
__global__ void __launch_bounds__(CIRC_THREADS) edwards_check_kernel(const Fr* __restrict__ points, uint64_t count, uint32_t* __restrict__ flags, const EdCurve c,
                                                                     const EdScalar order, int order_bits, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= count) return;
    const Fr x = points[2 * t], y = points[2 * t + 1];
    const Fr xx = fp_sqr(x, P), yy = fp_sqr(y, P);
    const bool on = fp_eq(fp_add(fp_mul(c.a, xx, P), yy, P), fp_add(fp_one(P), fp_mul(c.d, fp_mul(xx, yy, P), P), P));
    const EdPoint r = ed_mul_body(order, order_bits, x, y, c, P);
    const bool sub = on && fp_is_zero(r.X) && fp_eq(r.Y, r.Z);
    flags[t] = (on ? 1u : 0u) | (sub ? 2u : 0u);
}

// ---------------------------------------------------------------------------------------------- launchers (enqueued on `stream`, not synchronised)
struct EdHostParams {
    EdCurve c;
    Fr gx, gy;
    EdScalar order;
    int order_bits;
    SolveExponent e_inv;
};

// params: ED_PARAM_WORDS u64 on the host
static inline EdHostParams edwards_host_params(int curve, const uint64_t* params) {
    EdHostParams h;
    const uint32_t* w = (const uint32_t*)params;
    h.c.a = fp_from_limbs<8>(w);
    h.c.d = fp_from_limbs<8>(w + 8);
    h.gx = fp_from_limbs<8>(w + 16);
    h.gy = fp_from_limbs<8>(w + 24);
    h.order_bits = 1;
    for (int j = 0; j < 8; j++) {
        h.order.w[j] = w[32 + j];
        for (int b = 0; b < 32; b++)
            if ((h.order.w[j] >> b) & 1u) h.order_bits = 32 * j + b + 1;
    }
    SolveExponent root5;
    (void)solve_exponents(fr_params(curve), &h.e_inv, &root5);       // r - 2 is written whether or not the fifth root exists
    return h;
}

static inline int edwards_grid(size_t count, const char* who, uint32_t* grid) {
    const uint64_t blocks = ((uint64_t)count + CIRC_THREADS - 1) / CIRC_THREADS;
    if (blocks > 0x7FFFFFFFull) return plonk_fail(PLONK_ERR_ARG, "%s: count = %zu exceeds one launch (2^31 - 1 workgroups of %u points)", who, count, CIRC_THREADS);
    *grid = (uint32_t)blocks;
    return PLONK_OK;
}

int edwards_table_run(int curve, const uint64_t* params, Fr* d_table, hipStream_t stream) {
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_table", stream);
    hipLaunchKernelGGL(edwards_table_kernel, dim3(ED_TABLE_POINTS / CIRC_THREADS), dim3(CIRC_THREADS), 0, stream, d_table, h.gx, h.gy, h.c, h.e_inv, fr_params(curve));
    return circ_launch_status("edwards_table");
}

int edwards_mul_run(int curve, const uint64_t* params, const Fr* d_scalars, const Fr* d_points, size_t count, Fr* d_out, hipStream_t stream, const char* who) {
    uint32_t grid;
    int rc = edwards_grid(count, who, &grid);
    if (rc) return rc;
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_mul", stream);
    hipLaunchKernelGGL(edwards_mul_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_scalars, d_points, (uint64_t)count, d_out, h.c, h.e_inv, fr_params(curve));
    return circ_launch_status("edwards_mul");
}

int edwards_fixed_mul_run(int curve, const uint64_t* params, const Fr* d_scalars, size_t count, const Fr* d_table, Fr* d_out, hipStream_t stream, const char* who) {
    uint32_t grid;
    int rc = edwards_grid(count, who, &grid);
    if (rc) return rc;
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_fixed_mul", stream);
    hipLaunchKernelGGL(edwards_fixed_mul_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_scalars, (uint64_t)count, d_table, d_out, h.c, h.e_inv, fr_params(curve));
    return circ_launch_status("edwards_fixed_mul");
}

int edwards_add_run(int curve, const uint64_t* params, const Fr* d_p, const Fr* d_q, size_t count, Fr* d_out, hipStream_t stream, const char* who) {
    uint32_t grid;
    int rc = edwards_grid(count, who, &grid);
    if (rc) return rc;
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_add", stream);
    hipLaunchKernelGGL(edwards_add_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_p, d_q, (uint64_t)count, d_out, h.c, h.e_inv, fr_params(curve));
    return circ_launch_status("edwards_add");
}

int edwards_check_run(int curve, const uint64_t* params, const Fr* d_points, size_t count, uint32_t* d_flags, hipStream_t stream, const char* who) {
    uint32_t grid;
    int rc = edwards_grid(count, who, &grid);
    if (rc) return rc;
    const EdHostParams h = edwards_host_params(curve, params);
    ProfScope ps("edwards_check", stream);
    hipLaunchKernelGGL(edwards_check_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_points, (uint64_t)count, d_flags, h.c, h.order, h.order_bits, fr_params(curve));
    return circ_launch_status("edwards_check");
}
