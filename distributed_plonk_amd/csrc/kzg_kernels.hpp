// kzg_kernels.hpp — KZG openings outside a PLONK proof: one polynomial opened at many device-resident points, and the per-opening pair of the
// folded pairing check.  One header, two halves, each built in the translation unit that already holds what it needs:
//   KZG_KERNELS_POLY    (poly_ops.hip: PoCtx, the F29 helpers, block_total)      plonk_poly_open_many_dev
//   KZG_KERNELS_POINTS  (synth.hip, after verify_kernels.hpp: vfy::load_pt, ST_*) plonk_kzg_pairs_dev
//
// ---- many-point evaluation and synthetic division
// For f of `len` coefficients and M points z_j:  q_(len-2) = f_(len-1), q_(i-1) = f_i + z q_i, y = f_0 + z q_0 — the value is the remainder of
// the pass that makes the quotient.  Four launches whatever M is, over a grid of points x coefficient tiles (KZ_TILE = KZ_LANES lanes x KZ_CH
// consecutive coefficients); the points run along grid.x, so the workgroups in flight together read the SAME coefficient tile:
//   K0  kzg_point_table_kernel  one lane per point: the status word (z < p), rep(z^(2^s)) for s <= log2 KZ_TILE — z, the lane powers' factors,
//                               z^KZ_CH ... z^(KZ_CH * KZ_LANES / 2), z^KZ_LANES, W = z^KZ_TILE — and W^(per * 2^s), the top scan's multipliers
//   K1  kzg_agg_kernel          tile t of point j:  A_t = sum_e f[1 + t KZ_TILE + e] z^e — the lane-strided coalesced Horner of poly_div_agg_kernel,
//                               z^L built in the lane from the table's squarings (log2 KZ_LANES products at most)
//   K2  kzg_top_kernel          one workgroup per point:  X_t = sum_(u > t) A_u W^(u-t-1) (q at the first index above tile t), as
//                               poly_div_top_kernel; one step further is q_0, and y = f_0 + z q_0 is stored from here (so values need no K3)
//   K3  kzg_apply_kernel        tile t of point j: coefficients through LDS so that lane L owns KZ_CH consecutive ones; lane aggregate, then a
//                               lane-level suffix scan V_L += z^(KZ_CH d) V_(L+d), then the recurrence down the lane's chunk
// THE CHOICE FOR z = 0: the lane-level scan multiplies by z^(KZ_CH d) and nothing is ever divided by a power of z — there is no inverse, no
// scale / unscale and no branch on the point.  z = 0 is the point whose powers are all 0 (and z^0 = 1, which the lane power starts from): the
// scan then adds nothing and q_(i-1) = f_i falls out.  Cost: log2 KZ_LANES products per lane in the scan instead of the two of scale / unscale.
// A point z >= p gets status ST_NONCANONICAL, the value 0 and a row of zeros; its table row is never read.
//
// Arithmetic as in poly_ops.hip: HBM holds R = 2^256 Montgomery residues, canonical; constants (every power of z) are rep(c) = c 2^261,
// canonical, so f29_mul(data, rep(c)) = data * c in R form.  rep(z) = f29_mul(z_R, rep(2^5)), rep(2^5) a per-curve constant from the host.
//
// ---- the per-opening pair
// An opening (C, pi, z, y) holds iff e(pi, [tau]_2) = e(C - y G + z pi, [1]_2).  With rho per opening the pair of _bisect_on_device_tree
// (e(A, beta_h) e(-B, h) == 1) is  A = rho pi,  B = rho C + (rho z) pi - (rho y) G.
//   kzg_check_kernel     one lane per opening: coordinates, z, y, rho canonical; C and pi on the curve or (0, 0); the three scalars
//   kzg_subgroup_kernel  BLS12-381: [r] P == O for C and pi, one lane per point (the loop of verify_subgroup_kernel)
//   kzg_points_kernel    two lanes per opening as verify_points_kernel: lane 0 rho B (three terms, one doubling chain), lane 1 rho A
#pragma once

#ifdef KZG_KERNELS_POLY
#define KZ_LANES 128
#define KZ_CH 8
#define KZ_TILE (KZ_LANES * KZ_CH)
#define KZ_LOG_CH 3
#define KZ_LOG_LANES 7
#define KZ_LOG_TILE (KZ_LOG_CH + KZ_LOG_LANES)
#define KZ_TOP 256                       // lanes of the one-workgroup-per-point top kernel
#define KZ_LOG_TOP 8
#define KZ_TAB_LANES 64                  // points per workgroup of the table kernel
// a point's table row: [0, KZ_LOG_TILE] rep(z^(2^s)); then KZ_LOG_TOP entries rep(W^(per 2^s))
#define KZT_POW 0
#define KZT_WSTEP (KZ_LOG_TILE + 1)
#define KZT_N (KZT_WSTEP + KZ_LOG_TOP)
#define KZ_MAX_GRID_Y 65535u
static_assert((1 << KZ_LOG_CH) == KZ_CH && (1 << KZ_LOG_LANES) == KZ_LANES && (1 << KZ_LOG_TOP) == KZ_TOP,
              "kzg: z^KZ_CH, z^KZ_LANES, z^KZ_TILE and the scan steps are entries of the table of squarings");
static_assert(KZ_TILE == KZ_LANES * KZ_CH && KZ_LOG_TILE == KZ_LOG_CH + KZ_LOG_LANES, "kzg: a tile is KZ_LANES lanes x KZ_CH consecutive coefficients");
static_assert(KZ_CH == 8, "kzg_word pads one LDS word per 8 elements, and a lane's chunk is one such group");
static_assert(KZ_TOP >= 2 && KZ_LANES >= 2, "kzg: the scans need two lanes");
// the lazy sums below stay under 16 p (f29_mul takes < 2^261 with limbs < 2^31; 16 p < 2^259): a lane aggregate (< 2.4 p), the carry term
// (< 1.36 p) and one product (< 1.36 p) per scan step
static_assert(24 + 14 + 14 * KZ_LOG_LANES <= 160 && 24 + 14 * KZ_LOG_TOP <= 160, "kzg: a scan's lazy sum exceeds 16 p");

__device__ __forceinline__ F29 kz_zero() {
    F29 r;
#pragma unroll
    for (int l = 0; l < 9; l++) r.l[l] = 0;
    return r;
}
__device__ __forceinline__ bool kz_canonical(const Fr& v, const FrParams& P) {        // v < p as integers
    bool lt = false, eq = true;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        lt = lt || (eq && v.l[i] < P.p[i]);
        eq = eq && v.l[i] == P.p[i];
    }
    return lt;
}

// K0: one lane per point.  `per` = tiles per lane of the top kernel (a property of the call, not of the point)
__global__ void __launch_bounds__(KZ_TAB_LANES) kzg_point_table_kernel(const Fr* __restrict__ points, uint32_t m, uint64_t per, const F29 rep32,
                                                                       F29* __restrict__ table, uint32_t* __restrict__ status, const PoCtx c) {
    const uint32_t j = blockIdx.x * KZ_TAB_LANES + threadIdx.x;
    if (j >= m) return;
    const F29Params& fp = c.f29;
    const Fr z = load_fr(points + j);
    if (!kz_canonical(z, c.fp)) {
        status[j] = 8u;                                  // vfy::ST_NONCANONICAL; the row stays unwritten and unread
        return;
    }
    status[j] = 0;
    F29* row = table + (size_t)j * KZT_N;
    F29 pw = f29_canon(f29_mul(f29_from_sat(z), rep32, fp), fp);          // z 2^256 * 2^266 / 2^261 = rep(z)
    for (int s = 0; s <= KZ_LOG_TILE; s++) {
        row[KZT_POW + s] = pw;
        pw = f29_canon(f29_sqr(pw, fp), fp);
    }
    // W^per by square and multiply, then its squarings
    F29 b = row[KZT_POW + KZ_LOG_TILE], ws = params_one(fp);
    for (uint64_t e = per; e; e >>= 1) {
        if (e & 1) ws = f29_mul(ws, b, fp);
        b = f29_canon(f29_sqr(b, fp), fp);
    }
    ws = f29_canon(ws, fp);
    for (int s = 0; s < KZ_LOG_TOP; s++) {
        row[KZT_WSTEP + s] = ws;
        ws = f29_canon(f29_sqr(ws, fp), fp);
    }
}

// K1: agg[j * nt + t] = A_t of point j (canonical Fr, R form).  grid (m, min(nt, 65535)): tiles beyond the grid's height by stride
__global__ void __launch_bounds__(KZ_LANES) kzg_agg_kernel(const Fr* __restrict__ poly, uint64_t len, uint64_t nt, const F29* __restrict__ table,
                                                           const uint32_t* __restrict__ status, Fr* __restrict__ agg, const PoCtx c) {
    __shared__ uint32_t sh[KZ_LANES][9];
    const F29Params& fp = c.f29;
    const uint32_t j = blockIdx.x, L = threadIdx.x;
    if (status[j]) return;                               // the whole workgroup: j is the block's
    const F29* row = table + (size_t)j * KZT_N;
    const F29 zl = load_f29(row + KZT_POW + KZ_LOG_LANES);
    F29 zL = params_one(fp);                             // rep(z^L) from the squarings: z^0 = 1 for every z, 0 included
    for (int s = 0; s < KZ_LOG_LANES; s++)
        if ((L >> s) & 1) zL = f29_mul(zL, load_f29(row + KZT_POW + s), fp);          // normalised, < 1.36 p
    for (uint64_t t = blockIdx.y; t < nt; t += gridDim.y) {
        const uint64_t base = 1 + t * KZ_TILE + L;
        F29 acc = kz_zero();
        bool any = false;
#pragma unroll
        for (int k = KZ_CH - 1; k >= 0; k--) {
            const uint64_t i = base + (uint64_t)k * KZ_LANES;
            if (i < len) {
                const F29 ci = f29_from_sat(load_fr(poly + i));
                acc = any ? f29_add(f29_mul(acc, zl, fp), ci) : ci;       // < 1.36 p + p, limbs < 2^30: inside f29_mul's operand range
                any = true;
            }
        }
        Fr mine = fp_zero<8>();
        if (any) mine = f29_to_sat(f29_canon(f29_mul(acc, zL, fp), fp));  // * z^L, canonical
        const Fr tot = block_total<OpAdd, KZ_LANES>(mine, sh, c);
        if (L == 0) store_fr(agg + (size_t)j * nt + t, tot);
    }
}

// K2: one workgroup per point.  X_t = A_(t+1) + W X_(t+1), X_(nt-1) = 0; lane l owns the tiles [l per, (l+1) per).  One step below tile 0
// is q_0, and the value y = f_0 + z q_0 (f_0 alone for len == 1, 0 for len == 0).  carry may be NULL (values only).
__global__ void __launch_bounds__(KZ_TOP) kzg_top_kernel(const Fr* __restrict__ poly, uint64_t len, const Fr* __restrict__ agg_all, Fr* __restrict__ carry_all,
                                                         uint64_t nt, uint64_t per, const F29* __restrict__ table, const uint32_t* __restrict__ status,
                                                         Fr* __restrict__ values, const PoCtx c) {
    __shared__ uint32_t sh[KZ_TOP][9];
    const F29Params& fp = c.f29;
    const uint32_t j = blockIdx.x;
    const int t = threadIdx.x;
    if (status[j]) {
        if (t == 0) store_fr(values + j, fp_zero<8>());
        return;
    }
    const F29* row = table + (size_t)j * KZT_N;
    const Fr* agg = agg_all + (size_t)j * nt;
    Fr* carry = carry_all ? carry_all + (size_t)j * nt : nullptr;
    const F29 w = load_f29(row + KZT_POW + KZ_LOG_TILE);
    const uint64_t lo = (uint64_t)t * per < nt ? (uint64_t)t * per : nt, hi = lo + per < nt ? lo + per : nt;
    // G_l = sum_{u in run} A_u W^(u - lo)
    F29 g = kz_zero();
    for (uint64_t u = hi; u > lo; u--) {
        const F29 a = f29_from_sat(load_fr(agg + u - 1));
        g = (u == hi) ? a : f29_add(f29_mul(g, w, fp), a);
    }
    f29_norm(g);                                                              // < 2.4 p
    // inclusive suffix windows: V_l <- V_l + W^(per d) V_(l+d)
    OpMul::to_words(sh[t], g);
    __syncthreads();
    int s = 0;
    for (int d = 1; d < KZ_TOP; d <<= 1, s++) {
        F29 o;
        const bool on = t + d < KZ_TOP;
        if (on) o = OpMul::from_words(sh[t + d]);
        __syncthreads();
        if (on) {
            g = f29_add(g, f29_mul(o, load_f29(row + KZT_WSTEP + s), fp));    // + < 1.36 p per step: < 16 p after KZ_LOG_TOP steps (static_assert above)
            f29_norm(g);
            OpMul::to_words(sh[t], g);
        }
        __syncthreads();
    }
    // q just above this lane's run is V_(l+1); then down the run.  Lane 0 ends on X_(-1) = q_0.
    F29 x = kz_zero();
    if (t + 1 < KZ_TOP) x = OpMul::from_words(sh[t + 1]);
    for (uint64_t u = hi; u > lo; u--) {
        if (carry) store_fr(carry + u - 1, f29_to_sat(f29_canon_lazy(x, fp)));   // x normalised, < 16 p
        x = f29_add(f29_mul(x, w, fp), f29_from_sat(load_fr(agg + u - 1)));      // < 2.4 p, limbs < 2^30
        f29_norm(x);
    }
    if (t == 0) {
        // x = q_0 (V_1 itself when lane 0 has no tile: then nt == 0 and it is 0), normalised, < 16 p
        Fr y = fp_zero<8>();
        if (len) {
            F29 v = f29_add(f29_mul(x, load_f29(row + KZT_POW), fp), f29_from_sat(load_fr(poly)));    // z q_0 + f_0 < 2.4 p
            f29_norm(v);
            y = f29_to_sat(f29_canon_lazy(v, fp));
        }
        store_fr(values + j, y);
    }
}

// LDS layout of a tile: element e at word e*8 + (e >> 3) — one pad word per 8 elements makes both the coalesced (lane = e mod KZ_LANES) and the
// chunked (lane = e / KZ_CH) accesses 2 lanes per bank (poly_div_apply_kernel's layout)
__device__ __forceinline__ uint32_t kz_word(uint32_t e) { return e * 8 + (e >> 3); }
#define KZ_LDS_WORDS (KZ_TILE * 8 + KZ_TILE / 8)
// K3: row j of the quotients, outputs t KZ_TILE + e from the coefficients 1 + t KZ_TILE + e.  grid as K1.
__global__ void __launch_bounds__(KZ_LANES) kzg_apply_kernel(const Fr* __restrict__ poly, uint64_t len, uint64_t nt, const F29* __restrict__ table,
                                                             const uint32_t* __restrict__ status, const Fr* __restrict__ carry_all,
                                                             Fr* __restrict__ quot, uint64_t q_stride, const PoCtx c) {
    __shared__ uint32_t tile[KZ_LDS_WORDS];
    __shared__ uint32_t sh[KZ_LANES][9];
    const F29Params& fp = c.f29;
    const uint32_t j = blockIdx.x, L = threadIdx.x;
    Fr* out = quot + (size_t)j * q_stride;
    if (status[j]) {                                     // a point that is no residue: a row of zeros (the padding beyond len - 1 is not touched)
        for (uint64_t t = blockIdx.y; t < nt; t += gridDim.y)
            for (uint32_t e = L; e < KZ_TILE; e += KZ_LANES)
                if (t * KZ_TILE + e + 1 < len) store_fr(out + t * KZ_TILE + e, fp_zero<8>());
        return;
    }
    const F29* row = table + (size_t)j * KZT_N;
    const F29 z = load_f29(row + KZT_POW);
    for (uint64_t t = blockIdx.y; t < nt; t += gridDim.y) {
        const uint64_t j0 = t * KZ_TILE;
        // coalesced loads -> LDS
#pragma unroll
        for (int m = 0; m < KZ_CH; m++) {
            const uint32_t e = m * KZ_LANES + L;
            const uint64_t k = j0 + 1 + e;
            Fr v = fp_zero<8>();
            if (k < len) v = load_fr(poly + k);
            uint32_t* w = tile + kz_word(e);
#pragma unroll
            for (int i = 0; i < 8; i++) w[i] = v.l[i];
        }
        __syncthreads();
        // the lane's KZ_CH consecutive coefficients are read from LDS where they are used, never held in an indexed array (scratch memory)
        auto coeff = [&](int i) {
            const uint32_t* w = tile + kz_word(L * KZ_CH + i);
            Fr v;
#pragma unroll
            for (int k = 0; k < 8; k++) v.l[k] = w[k];
            return f29_from_sat(v);
        };
        // lane aggregate a_L = sum_i x[i] z^i; the tile's carry enters as the term above the last lane: a_(KZ_LANES-1) += z^KZ_CH X_t
        F29 a = coeff(KZ_CH - 1);
        for (int i = KZ_CH - 2; i >= 0; i--) a = f29_add(f29_mul(a, z, fp), coeff(i));        // < 2.4 p, limbs < 2^30
        const F29 xt = f29_from_sat(load_fr(carry_all + (size_t)j * nt + t));
        if (L == KZ_LANES - 1) a = f29_add(a, f29_mul(xt, load_f29(row + KZT_POW + KZ_LOG_CH), fp));    // < 3.8 p, limbs < 2^31
        f29_norm(a);
        // inclusive suffix scan over the lanes: V_L <- V_L + z^(KZ_CH d) V_(L+d); V_L = q at the lane's first index
        OpMul::to_words(sh[L], a);
        __syncthreads();
        int s = KZ_LOG_CH;
        for (uint32_t d = 1; d < KZ_LANES; d <<= 1, s++) {
            F29 o;
            const bool on = L + d < KZ_LANES;
            if (on) o = OpMul::from_words(sh[L + d]);
            __syncthreads();
            if (on) {
                a = f29_add(a, f29_mul(o, load_f29(row + KZT_POW + s), fp));     // + < 1.36 p per step: < 16 p after KZ_LOG_LANES steps (static_assert above)
                f29_norm(a);
                OpMul::to_words(sh[L], a);
            }
            __syncthreads();
        }
        // q at the first index above this lane's chunk: the next lane's V, the tile's carry for the last lane
        F29 q = L + 1 < KZ_LANES ? OpMul::from_words(sh[L + 1]) : xt;
        // the recurrence down the chunk; slot (L, i) of the tile is read, then overwritten, by this lane only
        for (int i = KZ_CH - 1; i >= 0; i--) {
            q = f29_add(f29_mul(q, z, fp), coeff(i));                            // < 2.4 p, limbs < 2^30
            F29 qn = q;
            f29_norm(qn);
            const Fr v = f29_to_sat(f29_canon_lazy(qn, fp));                     // canonical without a product
            uint32_t* w = tile + kz_word(L * KZ_CH + i);
#pragma unroll
            for (int k = 0; k < 8; k++) w[k] = v.l[k];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < KZ_CH; m++) {
            const uint32_t e = m * KZ_LANES + L;
            const uint64_t o = j0 + e;
            if (o + 1 < len) {
                const uint32_t* w = tile + kz_word(e);
                Fr v;
#pragma unroll
                for (int k = 0; k < 8; k++) v.l[k] = w[k];
                store_fr(out + o, v);
            }
        }
        __syncthreads();                                 // the next tile of this workgroup reuses both LDS arrays
    }
}

static uint64_t kz_tiles(uint64_t len) { return len < 2 ? 0 : (len - 1 + KZ_TILE - 1) / KZ_TILE; }     // tiles of the len - 1 quotient coefficients
size_t poly_open_many_tile() { return KZ_TILE; }
size_t poly_open_many_top_lanes() { return KZ_TOP; }
// the point tables, the tile aggregates and the carries
size_t poly_open_many_scratch_bytes(size_t len, size_t m) {
    return align256(m * KZT_N * sizeof(F29)) + 2 * align256(m * (kz_tiles(len) + 1) * 32) + 256;
}

int poly_open_many_run(NttTables& T, const void* d_poly, size_t len, const void* d_points, size_t m, void* d_values, void* d_quot, size_t q_stride,
                       void* d_status, void* scratch, hipStream_t stream) {
    if (m == 0) return PLONK_OK;
    const uint64_t nt = kz_tiles(len);
    const uint64_t per = (nt + KZ_TOP - 1) / KZ_TOP;
    char* s = (char*)scratch;
    F29* table = (F29*)s; s += align256(m * KZT_N * sizeof(F29));
    Fr* agg = (Fr*)s; s += align256(m * (nt + 1) * 32);
    Fr* carry = (Fr*)s;
    const PoCtx c = make_ctx(T);
    Fr h32 = fp_zero<8>();
    h32.l[0] = 32;
    const F29 rep32 = host_rep(fp_to_mont(h32, T.fp), T.fp);                   // rep(2^5): per curve, not per point
    const bool quot = d_quot && nt;
    const dim3 grid((uint32_t)m, (uint32_t)(nt < KZ_MAX_GRID_Y ? nt : KZ_MAX_GRID_Y));
    {
        ProfScope ps("poly_open_many_kernels", stream);
        hipLaunchKernelGGL(kzg_point_table_kernel, dim3((uint32_t)((m + KZ_TAB_LANES - 1) / KZ_TAB_LANES)), dim3(KZ_TAB_LANES), 0, stream, (const Fr*)d_points,
                           (uint32_t)m, per, rep32, table, (uint32_t*)d_status, c);
        if (nt)
            hipLaunchKernelGGL(kzg_agg_kernel, grid, dim3(KZ_LANES), 0, stream, (const Fr*)d_poly, (uint64_t)len, nt, (const F29*)table,
                               (const uint32_t*)d_status, agg, c);
        hipLaunchKernelGGL(kzg_top_kernel, dim3((uint32_t)m), dim3(KZ_TOP), 0, stream, (const Fr*)d_poly, (uint64_t)len, (const Fr*)agg, quot ? carry : (Fr*)nullptr,
                           nt, per, (const F29*)table, (const uint32_t*)d_status, (Fr*)d_values, c);
        if (quot)
            hipLaunchKernelGGL(kzg_apply_kernel, grid, dim3(KZ_LANES), 0, stream, (const Fr*)d_poly, (uint64_t)len, nt, (const F29*)table,
                               (const uint32_t*)d_status, (const Fr*)carry, (Fr*)d_quot, (uint64_t)q_stride, c);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "poly_open_many launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}
#endif  // KZG_KERNELS_POLY

#ifdef KZG_KERNELS_POINTS
namespace kzg {
// an opening record in u32 words: C (2 NQ), pi (2 NQ), z (8), y (8)
template <int NQ> constexpr int rec_words() { return 4 * NQ + 16; }
constexpr int NSCAL = 3;                 // per opening: rho, rho z, -(rho y), canonical integers
}  // namespace kzg

template <int NQ>
__global__ void __launch_bounds__(64) kzg_check_kernel(const uint32_t* __restrict__ recs, const Fr* __restrict__ rho, uint32_t k, Fr* __restrict__ scal,
                                                       uint32_t* __restrict__ status, const FpParams<8> R, const FpParams<NQ> Q, const Fp<NQ> b) {
    using namespace vfy;
    const uint32_t pid = blockIdx.x * 64 + threadIdx.x;
    if (pid >= k) return;
    const uint32_t* rec = recs + (size_t)pid * kzg::rec_words<NQ>();
    uint32_t stw = 0;
    for (int i = 0; i < 2; i++) {
        const AffPt<NQ> p = load_pt<NQ>(rec, i);
        if (!lt_mod<NQ>(p.x.l, Q.p) || !lt_mod<NQ>(p.y.l, Q.p)) { stw |= ST_NONCANONICAL; continue; }
        if (aff_is_inf(p)) continue;
        const Fp<NQ> rhs = fp_add(fp_mul(fp_sqr(p.x, Q), p.x, Q), b, Q);
        if (!fp_eq(fp_sqr(p.y, Q), rhs)) stw |= ST_OFF_CURVE;
    }
    const Fr z = fp_from_limbs<8>(rec + 4 * NQ), y = fp_from_limbs<8>(rec + 4 * NQ + 8), rh = rho[pid];
    if (!lt_mod<8>(z.l, R.p) || !lt_mod<8>(y.l, R.p) || !lt_mod<8>(rh.l, R.p)) stw |= ST_NONCANONICAL;
    status[pid] = stw;
    if (stw) return;
    Fr* sc = scal + (size_t)pid * kzg::NSCAL;
    sc[0] = fp_from_mont(rh, R);
    sc[1] = fp_from_mont(fp_mul(rh, z, R), R);
    sc[2] = fp_from_mont(fp_neg(fp_mul(rh, y, R), R), R);
}

// BLS12-381: [r] P == O for C and pi (the loop of verify_subgroup_kernel, which stays as it is)
template <int NQ>
__global__ void __launch_bounds__(128) kzg_subgroup_kernel(const uint32_t* __restrict__ recs, uint32_t k, uint32_t* __restrict__ status, const FpParams<8> R,
                                                           const FpParams<NQ> Q) {
    using namespace vfy;
    const uint32_t gid = blockIdx.x * 128 + threadIdx.x;
    if (gid >= 2 * k) return;
    const uint32_t pid = gid >> 1;
    if (status[pid] & (ST_OFF_CURVE | ST_NONCANONICAL)) return;              // unchecked coordinates: nothing to multiply
    const AffPt<NQ> p = load_pt<NQ>(recs + (size_t)pid * kzg::rec_words<NQ>(), gid & 1);
    if (aff_is_inf(p)) return;
    XyzzPt<NQ> acc = xyzz_inf<NQ>();
    for (int bit = 255; bit >= 0; bit--) {
        acc = xyzz_dbl_cold(acc, Q);
        if ((R.p[bit >> 5] >> (bit & 31)) & 1) acc = xyzz_madd_cold(acc, p, Q);
    }
    if (!xyzz_is_inf(acc)) atomicOr(&status[pid], (uint32_t)ST_SUBGROUP);
}

// two lanes per opening: gid & 1 = 0 rho B = rho C + (rho z) pi - (rho y) G, 1 rho A = rho pi; (0, 0) for an opening with a status
template <int NQ>
__global__ void __launch_bounds__(64) kzg_points_kernel(const uint32_t* __restrict__ recs, uint32_t k, const Fr* __restrict__ scal,
                                                        const uint32_t* __restrict__ status, uint32_t* __restrict__ out, const FpParams<NQ> Q,
                                                        const AffPt<NQ> g) {
    using namespace vfy;
    const uint32_t gid = blockIdx.x * 64 + threadIdx.x;
    if (gid >= 2 * k) return;
    const uint32_t pid = gid >> 1, which = gid & 1;
    AffPt<NQ> res;
    res.x = fp_zero<NQ>();
    res.y = fp_zero<NQ>();
    if (status[pid] == 0) {
        const uint32_t* rec = recs + (size_t)pid * kzg::rec_words<NQ>();
        const Fr* sc = scal + (size_t)pid * kzg::NSCAL;
        const AffPt<NQ> cm = load_pt<NQ>(rec, 0), pi = load_pt<NQ>(rec, 1);
        const Fr s0 = sc[0], s1 = sc[1], s2 = sc[2];
        XyzzPt<NQ> acc = xyzz_inf<NQ>();
        for (int bit = 255; bit >= 0; bit--) {
            acc = xyzz_dbl_cold(acc, Q);
            const int w = bit >> 5, sh = bit & 31;
            if (which) {
                if ((s0.l[w] >> sh) & 1) acc = xyzz_madd_cold(acc, pi, Q);
            } else {
                if ((s0.l[w] >> sh) & 1) acc = xyzz_madd_cold(acc, cm, Q);
                if ((s1.l[w] >> sh) & 1) acc = xyzz_madd_cold(acc, pi, Q);
                if ((s2.l[w] >> sh) & 1) acc = xyzz_madd_cold(acc, g, Q);
            }
        }
        res = xyzz_to_affine(acc, Q);
    }
    uint32_t* o = out + (size_t)gid * 2 * NQ;
#pragma unroll
    for (int i = 0; i < NQ; i++) {
        o[i] = res.x.l[i];
        o[NQ + i] = res.y.l[i];
    }
}

namespace kzg {
template <int NQ>
int run(const void* recs, const void* rho, uint32_t k, const uint32_t* g_xy, void* out, uint32_t* status, void* scratch, const FpParams<8>& R,
        const FpParams<NQ>& Q, const uint32_t* b, hipStream_t stream) {
    Fr* scal = (Fr*)scratch;
    const Fp<NQ> bq = fp_from_limbs<NQ>(b);
    AffPt<NQ> g;
    g.x = fp_from_limbs<NQ>(g_xy);
    g.y = fp_from_limbs<NQ>(g_xy + NQ);
    hipLaunchKernelGGL(kzg_check_kernel<NQ>, dim3((k + 63) / 64), dim3(64), 0, stream, (const uint32_t*)recs, (const Fr*)rho, k, scal, status, R, Q, bq);
    if (NQ == 12)
        hipLaunchKernelGGL(kzg_subgroup_kernel<NQ>, dim3((2 * k + 127) / 128), dim3(128), 0, stream, (const uint32_t*)recs, k, status, R, Q);
    hipLaunchKernelGGL(kzg_points_kernel<NQ>, dim3((2 * k + 63) / 64), dim3(64), 0, stream, (const uint32_t*)recs, k, (const Fr*)scal,
                       (const uint32_t*)status, (uint32_t*)out, Q, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "kzg_pairs launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}
}  // namespace kzg

size_t kzg_pairs_scratch_bytes(size_t k) { return k * kzg::NSCAL * sizeof(Fr); }

int kzg_pairs_run(int curve, const void* d_openings, const void* d_rho, size_t k, const uint64_t* g_xy, void* d_out, void* d_status, void* scratch,
                  hipStream_t stream) {
    if (curve == PLONK_BN254)
        return kzg::run<8>(d_openings, d_rho, (uint32_t)k, (const uint32_t*)g_xy, d_out, (uint32_t*)d_status, scratch, BN254_FR_PARAMS, BN254_FQ_PARAMS,
                           BN254_G1_B_MONT, stream);
    return kzg::run<12>(d_openings, d_rho, (uint32_t)k, (const uint32_t*)g_xy, d_out, (uint32_t*)d_status, scratch, BLS12_381_FR_PARAMS, BLS12_381_FQ_PARAMS,
                        BLS12_381_G1_B_MONT, stream);
}
#endif  // KZG_KERNELS_POINTS
