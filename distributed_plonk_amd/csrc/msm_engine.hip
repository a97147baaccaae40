// msm_engine.hip — Pippenger multi-scalar multiplication sum_i s_i * P_i on gfx950.
//
// What it replaces: ark-ec 0.3.0 VariableBaseMSM::multi_scalar_mul as called by the reference at
// src/worker.rs:179-182 (varMsm), :117-123,405 (commit_polynomial / round1), src/dispatcher.rs:1052
// and src/dispatcher2.rs:835-893.  Only the group element is contractual
// (Appendix A.1), so the GPU algorithm is free to differ from the CPU one:
//
//   1/2. level 1   ONE pass over the scalars: every scalar leaves Montgomery form once and is cut into W = ceil((bits+1)/c) SIGNED c-bit
//                  digits, stored planar, and the same lanes count the per-(slice, window) partition histograms in LDS
//                                                                              (sort_digits_hist_kernel; scan_* turns counts into ranges)
//   3. sort        two-level LDS-staged counting sort of the (window, |digit|) keys: the level-1 scatter reads its slice of digits ONCE
//                  (16 per lane, kept in registers across count -> scan -> rank) and leaves coalesced runs per partition; then one workgroup
//                  per partition orders its L2-resident entries and emits the bucket offsets — the staged kernel reads a partition that is
//                  one chunk of at most 18 entries per lane ONCE as well                  (sort_scatter / sort_partition[_staged])
//                  Bytes through HBM at 2^24 points x 13 windows: 32 B per scalar (0.5 GB) + five passes of 4 B per (point, window) —
//                  dig written and read, tmp written and read, sorted written (0.87 GB each) = 4.9 GB, where the separate digits and
//                  histogram kernels moved 5.7 GB and the second sweeps of both sort levels asked the caches for 1.7 GB more
//                  (profiles/r07_msm_sort_passes.txt)
//   3b. schedule   bucket ids counting-sorted by size, so a wave's lanes own equally loaded buckets
//   4. accumulate  one lane per bucket walks its segment and adds the resident limb-form bases (negated for
//                  negative digits) into an XYZZ accumulator held in VGPRs   (msm_accumulate_kernel;
//                  same-x exceptional additions are redone by msm_accumulate_redo_kernel)
//   5. reduce      sum_d d*B_d per window as a pyramid of running-sum passes over chunks of K = 4 entries
//                  (msm_reduce_level_kernel, fast path + redo), then per-level sums (msm_points_sum_kernel)
//   6. fold        V_w = Sigma + sum_l 4^l A_l per window and the W window sums -> one point (W*c doublings), on the
//                  host; the result is returned as a normalised Jacobian triple (x, y, 1) / (1, 1, 0).
//   (opt.)         a fixed-base window table built at `init` (planes 2^(c*G*t) * P_i) lets a scalar's W windows share G bucket sets
//                  (msm_table_kernel); measured a wash on MI355X and off by default — see the comment there.
//
// Zero scalars and digit 0 never touch a bucket (the reference filters zeros too); scalar 1 needs no
// special case (digit 1 in window 0).  Infinity bases are skipped, P+P and P+(-P) are handled in
// ec_lazy.hpp (device) / ec.hpp (host fold).  No MFMA: ~10 Fq Montgomery products per (point, window) dominate everything — the
// kernel is v_mad_u64_u32 bound; algorithmic HBM bytes are n*(sizeof(affine)+32).
#include <algorithm>
#include <cstring>
#include <type_traits>

#include "constants.h"
#include "msm_kernels.hpp"
#include "plonk_internal.hpp"

template <int NQ> static const FpParams<NQ>& fq_params(int curve);
template <> const FpParams<8>& fq_params<8>(int) { return BN254_FQ_PARAMS; }
template <> const FpParams<12>& fq_params<12>(int) { return BLS12_381_FQ_PARAMS; }
template <int NQ> using LimbParams = FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>;      // the lazy limb arithmetic of the curve's base field
template <int NQ> using BucketL = XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>;            // a bucket, and every partial sum of the reduction
template <int NQ> static const LimbParams<NQ>& fl_params(int curve) {
    static const LimbParams<NQ> P = fl_make_params<LimbGeom<NQ>::NL, LimbGeom<NQ>::B, NQ>(fq_params<NQ>(curve));
    return P;
}

size_t msm_limb_base_bytes(int curve) { return curve == PLONK_BN254 ? sizeof(BaseRec<8>) : sizeof(BaseRec<12>); }

// ---------------------------------------------------------------------------------------------- the SRS: conversion, check, resident form, table
int bases_convert_ark(int curve, const void* d_raw, size_t n, void* d_compact, unsigned long long* d_bad, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (curve == PLONK_BN254)
        hipLaunchKernelGGL(bases_convert_kernel<8>, dim3(grid), dim3(256), 0, stream, (const uint32_t*)d_raw, (uint64_t)n, (AffPt<8>*)d_compact, d_bad);
    else
        hipLaunchKernelGGL(bases_convert_kernel<12>, dim3(grid), dim3(256), 0, stream, (const uint32_t*)d_raw, (uint64_t)n, (AffPt<12>*)d_compact, d_bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "bases_convert launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

// d_bad: two device words, zeroed to {~0, 0} here unless `keep` (the ark conversion has already written its findings)
template <int NQ> static int bases_check_t(int curve, const void* d_xy, size_t n, unsigned long long* d_bad, bool keep, const char* who, hipStream_t stream) {
    const FpParams<NQ>& P = fq_params<NQ>(curve);
    if (!keep) {
        static const unsigned long long init[2] = {~0ull, 0ull};
        HIP_TRY(hipMemcpyAsync(d_bad, init, sizeof init, hipMemcpyHostToDevice, stream));
    }
    Fp<NQ> b = fp_zero<NQ>(), one;
    for (int k = 0; k < NQ; k++) one.l[k] = P.one[k];
    for (int k = 0; k < (curve == PLONK_BN254 ? 3 : 4); k++) b = fp_add(b, one, P);          // y^2 = x^3 + 3 (BN254) / + 4 (BLS12-381), Montgomery form
    if (n) hipLaunchKernelGGL(bases_check_kernel<NQ>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, (const AffPt<NQ>*)d_xy, (uint64_t)n, P, b, d_bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "bases_check launch: %s", hipGetErrorString(e));
    unsigned long long h[2] = {~0ull, 0ull};
    HIP_TRY(hipMemcpyAsync(h, d_bad, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h[1] == 0) return PLONK_OK;
    return plonk_fail(PLONK_ERR_ARG, "%s: base %llu of %zu is not a curve point (%s%s%s) — wrong layout, field order or stride?  (PLONK_BASES_XY: x||y, "
                      "PLONK_BASES_ARK: x, y, infinity byte; Montgomery limbs; plonk_set_option(\"check_bases\", 0) skips this check)", who, h[0], n,
                      (h[1] & BASES_BAD_FLAG) ? "infinity flag byte is neither 0 nor 1; " : "", (h[1] & BASES_BAD_RANGE) ? "coordinate not below the modulus; " : "",
                      (h[1] & BASES_BAD_CURVE) ? "y^2 != x^3 + b" : "");
}
int bases_check(int curve, const void* d_xy, size_t n, unsigned long long* d_bad, bool keep, const char* who, hipStream_t stream) {
    return curve == PLONK_BN254 ? bases_check_t<8>(curve, d_xy, n, d_bad, keep, who, stream) : bases_check_t<12>(curve, d_xy, n, d_bad, keep, who, stream);
}

// XY (reference layout) -> resident limb form; d_out holds n * msm_limb_base_bytes(curve) bytes
int bases_to_limbs(int curve, const void* d_xy, size_t n, void* d_out, hipStream_t stream) {
    if (n == 0) return PLONK_OK;
    const uint32_t grid = (uint32_t)((n + 255) / 256);
    if (curve == PLONK_BN254)
        hipLaunchKernelGGL(bases_to_limbs_kernel<8>, dim3(grid), dim3(256), 0, stream, (const AffPt<8>*)d_xy, (uint64_t)n, (BaseRec<8>*)d_out, fl_params<8>(curve));
    else
        hipLaunchKernelGGL(bases_to_limbs_kernel<12>, dim3(grid), dim3(256), 0, stream, (const AffPt<12>*)d_xy, (uint64_t)n, (BaseRec<12>*)d_out, fl_params<12>(curve));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "bases_to_limbs launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}

// The fixed-base window table: msm_table_kernel (msm_kernels.hpp) says what it holds and why it is off by default.
template <int NQ> static int msm_table_build_t(int curve, void* d_table, size_t n, size_t stride, int shift, int T, hipStream_t stream) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const FpParams<NQ>& P = fq_params<NQ>(curve);
    Fp<NQ> pm2;
    uint64_t br = 2;
    for (int i = 0; i < NQ; i++) { uint64_t t = (uint64_t)P.p[i] - br; pm2.l[i] = (uint32_t)t; br = (t >> 32) & 1; }
    hipLaunchKernelGGL(msm_table_kernel<NQ>, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, stream, (BaseRec<NQ>*)d_table, (uint64_t)n, (uint64_t)stride, shift, T,
                       fl_params<NQ>(curve), fl_from_sat<NL, B, NQ>(pm2));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "msm_table launch: %s", hipGetErrorString(e));
    return PLONK_OK;
}
// d_table: T planes of `stride` points, plane 0 already holds the bases (bases_to_limbs); plane t = 2^(shift * t) * plane 0, shift = c * G
int msm_table_build(int curve, void* d_table, size_t n, size_t stride, int shift, int T, hipStream_t stream) {
    if (n == 0 || T < 2) return PLONK_OK;
    if (curve == PLONK_BN254) return msm_table_build_t<8>(curve, d_table, n, stride, shift, T, stream);
    return msm_table_build_t<12>(curve, d_table, n, stride, shift, T, stream);
}

// ---------------------------------------------------------------------------------------------- cost model, window and table plans
// level-1 partition bits of the sort for 2^cb buckets per window: 2^10 partitions (16-entry runs per 16384-entry slice, two
// level-1 workgroups per CU), more only when a level-2 workgroup would otherwise own more than 2^11 buckets.
static bool sort_geometry(int cb, size_t n, int* lp_out) {
    const int lp = std::max(std::min(cb, 10), cb - 11);
    if (lp > 13 || n > ((size_t)1 << 27)) return false;        // 2^13 + 1 level-1 bins; <= 8192 slice offsets in the level-2 LDS
    *lp_out = lp;
    return true;
}

#define MSM_TABLE_MAX_C 21                           // widest window the table plan considers (the level-2 sort is staged in LDS up to 2^10 buckets per partition ...)
static constexpr double REDUCE_COST = 2.7 * 3300.0;          // VALU instructions per bucket in the reduction pyramid (round 3: the x2 for its low occupancy went
                                                      // with the split per-level sums and the LDS-staged level-2 sort: c = 20 now wins at 2^24 points)
// measured issue cost (profiles/r01_pmc_sq_2p24.json): ~2480 VALU instructions per mixed addition, ~3300 per full
// addition; the reduction pyramid does ~2.7 full additions per bucket
static bool window_usable(size_t n, int bits, int c) {
    int lp;
    if (!sort_geometry(c - 1, n, &lp)) return false;
    const int W = (bits + 1 + c - 1) / c;
    const int top_bits = bits - (W - 1) * c;                   // entropy of the last window's digit
    return !(W > 1 && top_bits < std::min(c - 3, 8));          // a near-empty top window puts every point in a few buckets
}
// G = bucket sets per scalar vector (plain: G = W)
static double window_cost(size_t n, int bits, int c, int G) {
    const int W = (bits + 1 + c - 1) / c;
    const double sets = (double)std::min(std::max(G, 1), W);
    // one lane per bucket: below 4 waves per SIMD (262144 lanes) the additions are latency-bound and the SIMDs idle in
    // proportion (measured: 2^16 points at c = 8 -> 4096 lanes, 10 ms; the same points at c = 15 -> 0.3 ms)
    const double lanes = sets * (double)((size_t)1 << (c - 1));
    const double par = std::min(1.0, lanes / 262144.0);
    return (double)W * (double)n * 2480.0 / par + sets * (double)((size_t)1 << (c - 1)) * REDUCE_COST;
}
static int choose_window(size_t n, int bits, double* cost_out = nullptr) {
    double best = 1e300;
    int bc = 4;
    for (int c = 4; c <= 20; c++) {
        if (!window_usable(n, bits, c)) continue;
        const double cost = window_cost(n, bits, c, (bits + 1 + c - 1) / c);
        if (cost < best) { best = cost; bc = c; }
    }
    if (cost_out) *cost_out = best;
    return bc;
}

// Plan of the fixed-base table for an SRS of n points: window width c (0 = no table: too small to pay off, or over budget), W windows per scalar,
// G bucket sets per scalar, T = ceil(W / G) planes.  mode 1: only when the cost model sees a gain; mode 2: always (tests).  The widest table the
// budget allows wins ties; force_c / force_sets (options "msm_table_c" / "msm_table_sets") pin a shape (tests, experiments).
int msm_table_plan(int curve, size_t n, int mode, size_t budget_bytes, int force_c, int force_sets, int* W_out, int* G_out, int* T_out) {
    *W_out = 1; *G_out = 1; *T_out = 1;
    if (mode == 0 || n == 0) return 0;
    const int bits = fr_params(curve).bits;
    const double pb = (double)msm_limb_base_bytes(curve);
    double plain = 0;
    choose_window(n, bits, &plain);
    const int fc = force_c > 0 ? force_c : (getenv("PLONK_MSM_TAB_C") ? atoi(getenv("PLONK_MSM_TAB_C")) : 0);       // "msm_table_c" / "msm_table_sets" options;
    const int fg = force_sets > 0 ? force_sets : (getenv("PLONK_MSM_TAB_G") ? atoi(getenv("PLONK_MSM_TAB_G")) : 0);   // the variables serve tools that cannot reach the context
    double best = 1e300;
    int bc = 0, bG = 1;
    for (int c = 4; c <= MSM_TABLE_MAX_C; c++) {
        if (fc > 0 && c != fc) continue;
        if (!window_usable(n, bits, c)) continue;
        const int W = (bits + 1 + c - 1) / c;
        if (W < 2) continue;
        for (int G = 1; G < W; G++) {                            // G = W would be the plain plan
            if (fg > 0 && G != fg) continue;
            const int T = (W + G - 1) / G;
            if (fg <= 0 && G != (W + T - 1) / T) continue;       // skip shapes that a table of the same size serves with fewer sets
            if ((double)T * (double)n * pb > (double)budget_bytes) continue;
            const double cost = window_cost(n, bits, c, G) * (1.0 + 1e-4 * T);      // ties: the smaller table
            if (cost < best) { best = cost; bc = c; bG = G; }
        }
    }
    if (!bc) return 0;
    if (mode == 1 && (n < ((size_t)1 << 16) || best > 0.97 * plain)) return 0;
    const int W = (bits + 1 + bc - 1) / bc;
    *W_out = W; *G_out = bG; *T_out = (W + bG - 1) / bG;
    return bc;
}

// Window width and bucket sets per scalar vector for an MSM over n points: the table's shape when one is resident and beats the best plain plan
// for THIS n (small sub-ranges and forced windows do not use it), else the plain plan (G = W1).
static int plan_window(size_t n, int bits, int window_bits, const MsmTable& tab, int* G_out) {
    if (window_bits <= 0 && tab.c > 0 && window_usable(n, bits, tab.c)) {
        double plain = 0;
        choose_window(n, bits, &plain);
        if (tab.force || window_cost(n, bits, tab.c, tab.G) < plain) { *G_out = tab.G; return tab.c; }
    }
    const int c = window_bits > 0 ? std::min(std::max(window_bits, 2), 20) : choose_window(n, bits);
    *G_out = (bits + 1 + c - 1) / c;
    return c;
}

// The plan of one launch set of msm_slice — n points, K scalar vectors against the same bases — as plain host arithmetic: no launch, no device
// access (n_cu, the CU count of the device, is handed in; only `persistent` depends on it).  msm_slice consumes exactly this and plonk_msm_plan
// reports it, so a test asserts the branch it means to run from what the engine decided (tests/msm_plans.py restates it in Python).
struct MsmPlan {
    int c, G, W1, W, cb, Wr;         // window bits, bucket sets and windows per vector, windows of the batch, log2 buckets per window, bucket sets
    uint64_t nsub, nbuckets, max_heavy;
    uint32_t heavy_thresh;
    SetGeom sg;
    SortGeom g;                      // stage_cap included
    bool packed;                     // the level-1 scatter carries the partition in the entry's top bits (sort_scatter_kernel: ebits + lp <= 32)
    uint64_t nhist, nscan_blocks;
    int nlev;                        // reduction pyramid
    uint64_t lev_n[16], lev_k[16], lev_nch[16], pyr;
    uint32_t gsplit;                 // workgroups per (level, window) sum
    bool grid_mode;
    uint32_t g_logL, g_logH, g_nbits;
    bool fused_order;                // effective: the bucket-size histogram rides in the level-2 sort
    size_t lds_staged;
    bool staged;                     // sort_partition_staged_kernel (else sort_partition_kernel)
    uint32_t acc_grid;               // workgroups of the accumulation ...
    bool persistent;                 // ... as persistent waves on a work counter
    bool fused_y3;                   // "msm_fused_y3": which instantiation of the accumulate kernel
};

static int msm_plan(size_t n, int K, int bits, int window_bits, const MsmTable& tab, const MsmWorkspace& ws, int n_cu, MsmPlan& p) {
    int G = 1;
    const int c = plan_window(n, bits, window_bits, tab, &G);
    const int W1 = (bits + 1 + c - 1) / c;             // windows per scalar vector (signed digits: one spare bit for the last carry)
    const bool merged = G < W1;                        // fixed-base table in use: G bucket sets per vector, window g + t*G reads plane t
    if (merged && (W1 != tab.W || G != tab.G)) return plonk_fail(PLONK_ERR_STATE, "msm: table built for %d windows in %d sets, plan has %d in %d", tab.W, tab.G, W1, G);
    const int W = K * W1;                              // windows of the whole batch
    const int cb = c - 1;                              // 2^(c-1) buckets per window
    const uint64_t nb = (uint64_t)1 << cb;
    const int Wr = K * G;                              // bucket sets to accumulate and reduce
    p.nsub = (uint64_t)W * nb;                         // (window, bucket) segments the sort produces
    p.nbuckets = (uint64_t)Wr * nb;                    // accumulators
    if (p.nbuckets >= 0xffffffffull) return plonk_fail(PLONK_ERR_ARG, "msm: %llu buckets", (unsigned long long)p.nbuckets);
    const uint64_t avg = ((uint64_t)n * W) / p.nbuckets + 1;
    p.heavy_thresh = (uint32_t)std::max<uint64_t>(HEAVY_BUCKET, 4 * avg);
    SetGeom& sg = p.sg;
    sg.cb = (uint32_t)cb; sg.G = (uint32_t)G; sg.W1 = (uint32_t)W1; sg.tab_stride = merged ? tab.stride : 0;
    sg.bin_shift = 0;
    while ((avg >> sg.bin_shift) > 96) sg.bin_shift++;        // keep the average bucket inside the 256 size bins
    if ((uint64_t)n * W >= 0xffffffffull) return plonk_fail(PLONK_ERR_ARG, "msm slice too large");
    SortGeom& g = p.g;
    g.n = n; g.W = W; g.cb = cb; g.stage_cap = 0;
    if (!sort_geometry(cb, n, &g.lp)) return plonk_fail(PLONK_ERR_ARG, "msm: window %d too wide for %zu points", c, n);
    g.low_bits = cb - g.lp;
    g.nblk = (uint32_t)((n + SORT_SLICE - 1) / SORT_SLICE);
    g.nreal = (uint32_t)W << g.lp;
    {
        uint32_t ln = 1;
        while (((uint64_t)1 << ln) < (uint64_t)n) ln++;
        g.idx_bits = ((uint32_t)g.low_bits + 1 + ln <= 32) ? ln : 0;
        if (ws.sort_slice_index) g.idx_bits = 0;       // "msm_sort_slice_index" (tests): the form of wide windows at huge n, valid at any size
    }
    p.c = c; p.G = G; p.W1 = W1; p.W = W; p.cb = cb; p.Wr = Wr;
    p.max_heavy = ((uint64_t)n * W) / p.heavy_thresh + 1;     // a bucket is heavy only above heavy_thresh entries
    p.packed = (uint32_t)g.low_bits + SORT_SLICE_LOG + 1 + (uint32_t)g.lp <= 32;
    p.nhist = ((uint64_t)g.nreal + W) * g.nblk;
    p.nscan_blocks = (p.nhist + SCAN_CHUNK - 1) / SCAN_CHUNK;
    // reduction pyramid geometry
    p.nlev = 0;
    for (uint64_t cur = nb; cur > 1 && p.nlev < 15; p.nlev++) {
        p.lev_n[p.nlev] = cur;
        p.lev_k[p.nlev] = std::min<uint64_t>(REDUCE_K, cur);
        p.lev_nch[p.nlev] = cur / p.lev_k[p.nlev];
        cur = p.lev_nch[p.nlev];
    }
    p.pyr = 0;
    for (int l = 0; l < p.nlev; l++) p.pyr += (uint64_t)Wr * p.lev_nch[l];
    // plain mode: the per-(level, window) sums of large pyramids are split over `gsplit` workgroups and folded by a second launch
    // (one workgroup per 2048 level-0 values: at 2^13 values per window — c = 16, the 2^20-point plan — a single workgroup walked 32 points per lane
    //  before its 8-step tree, the deepest dependent chain of a small MSM's reduction)
    p.gsplit = (uint32_t)std::min<uint64_t>(32, std::max<uint64_t>(1, (p.nlev ? p.lev_nch[0] : 1) / 2048));
    // "msm_reduce_grid": buckets of a set as an H x L grid (5b); row / column sums in the limb form, then logL + 1 + logH bit sums per set
    p.grid_mode = ws.reduce_grid != 0 && cb >= 2;
    p.g_logL = (uint32_t)(cb + 1) / 2; p.g_logH = (uint32_t)cb - p.g_logL; p.g_nbits = p.g_logL + 1 + p.g_logH;
    // the bucket-size histogram rides in the level-2 sort when a bucket is one sorted segment (no fixed-base table).  "msm_fused_order": 1 (default) = for
    // launches of >= 2^23 points in total, where it takes 3 % off the commitment phase of a 2^24 step; below that the level-2 sort loses more to the
    // histogram's atomics than the two saved launches give back (+0.7 % per 2^20 step; profiles/r05_msm_fused_order.txt); 2 = always (tests); 0 = never
    p.fused_order = (ws.fused_order == 2 || (ws.fused_order == 1 && (uint64_t)n * (uint64_t)K >= ((uint64_t)1 << 23))) && sg.tab_stride == 0 && sg.G == sg.W1;
    // the staged level-2 kernel: 78 KiB of LDS per workgroup (two per CU); what the counters and the slice starts leave is the staging buffer
    const size_t lds_fixed = (((size_t)1 << g.low_bits) + (g.idx_bits ? 0 : g.nblk)) * 4;
    p.lds_staged = 78 * 1024;
    g.stage_cap = lds_fixed + 4096 * 4 <= p.lds_staged ? (uint32_t)((p.lds_staged - lds_fixed) / 4) : 0;
    if (ws.sort_stage_cap > 0 && g.stage_cap) g.stage_cap = std::min<uint32_t>(g.stage_cap, std::max<uint32_t>((uint32_t)ws.sort_stage_cap, STAGE_THREADS));   // tests: force the chunked path
    p.staged = g.low_bits >= 8 && g.stage_cap >= STAGE_THREADS && !getenv("PLONK_MSM_NO_STAGED_SORT");
    // "msm_acc_persist" (default 4): the accumulation as that many workgroups per CU of persistent waves; 0 = one lane per bucket over the whole grid
    p.acc_grid = (uint32_t)((p.nbuckets + 255) / 256);
    p.persistent = false;
    if (ws.acc_persist != 0) {
        const uint32_t pgrid = ws.acc_persist > 0 ? (uint32_t)n_cu * (uint32_t)ws.acc_persist : (uint32_t)(-ws.acc_persist);   // < 0: absolute grid (tests)
        if (pgrid < p.acc_grid) { p.persistent = true; p.acc_grid = pgrid; }      // small problems keep the plain grid
    }
    p.fused_y3 = ws.fused_y3 != 0;
    return PLONK_OK;
}

// CU count of the CURRENT device, cached per device (a process may drive several GPUs from several threads)
static int device_cu_count(int* out) {
    static int cu_of_dev[64];
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int n_cu = dev >= 0 && dev < 64 ? __atomic_load_n(&cu_of_dev[dev], __ATOMIC_ACQUIRE) : 0;
    if (!n_cu) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev));
        n_cu = std::max(prop.multiProcessorCount, 1);
        if (dev >= 0 && dev < 64) __atomic_store_n(&cu_of_dev[dev], n_cu, __ATOMIC_RELEASE);
    }
    *out = n_cu;
    return PLONK_OK;
}

// points per slice of an MSM ("msm_slice_log", default 2^26: workspace sizing) and scalar vectors per launch set for slices of m points: as far as
// the 32-bit entry indices of the sort (m * W1 * K < 2^32), grid.y of the per-window launches and "msm_batch_max" allow
static size_t msm_slice_points(const MsmWorkspace& ws) { return (size_t)1 << std::min(std::max(ws.slice_log, 8), 26); }
static int msm_group(size_t m, int K, int bits, int window_bits, const MsmTable& tab, const MsmWorkspace& ws) {
    int G_ = 1;
    const int c = plan_window(m, bits, window_bits, tab, &G_);
    const int W1 = (bits + 1 + c - 1) / c;
    const uint64_t per = (uint64_t)m * W1;
    int group = (int)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)K, (0xfffffff0ull / per)));
    if ((uint64_t)group * W1 > 65535) group = 65535 / W1;                    // grid.y of the per-window launches
    return std::min(group, std::min(std::max(ws.batch_max, 1), 64));
}
// How an MSM of K vectors over n points is cut into launch sets: the slice that starts at point s has m points, and its launch sets start at the
// vectors 0, group, 2 * group, ...  msm_run_t walks these, plonk_msm_plan reports the plan of the one at (0, 0).
struct MsmLaunchSets {
    size_t m;
    int group;
    int kn(int K, int k0) const { return std::min(group, K - k0); }      // vectors of the launch set that starts at vector k0
};
static MsmLaunchSets msm_launch_sets(size_t n, int K, size_t s, int bits, int window_bits, const MsmTable& tab, const MsmWorkspace& ws) {
    const size_t m = std::min(msm_slice_points(ws), n - s);
    return {m, msm_group(m, K, bits, window_bits, tab, ws)};
}

// plonk_msm_plan: the plan of the FIRST launch set of an MSM of K vectors over n points (later sets of a sliced or grouped MSM differ only in
// their point and vector counts), as the integers of include/plonk_hip.h (PLONK_MSM_PLAN_*).  The only device access is the CU count.
int msm_plan_query(int curve, size_t n, int K, const MsmWorkspace& ws, int window_bits, const MsmTable& tab, int32_t* out, int n_out) {
    if (n == 0 || K <= 0) return plonk_fail(PLONK_ERR_ARG, "msm plan: %zu points, %d vectors", n, K);
    if (!out || n_out < PLONK_MSM_PLAN_FIELDS) return plonk_fail(PLONK_ERR_ARG, "msm plan: room for %d of %d fields", out ? n_out : 0, PLONK_MSM_PLAN_FIELDS);
    const int bits = fr_params(curve).bits;
    const MsmLaunchSets sets = msm_launch_sets(n, K, 0, bits, window_bits, tab, ws);
    const int kn = sets.kn(K, 0);
    int n_cu = 0;
    int rc = device_cu_count(&n_cu);
    if (rc) return rc;
    MsmPlan p;
    if ((rc = msm_plan(sets.m, kn, bits, window_bits, tab, ws, n_cu, p))) return rc;
    out[PLONK_MSM_PLAN_C] = p.c; out[PLONK_MSM_PLAN_W1] = p.W1; out[PLONK_MSM_PLAN_G] = p.G; out[PLONK_MSM_PLAN_CB] = p.cb;
    out[PLONK_MSM_PLAN_LP] = p.g.lp; out[PLONK_MSM_PLAN_LOW_BITS] = p.g.low_bits; out[PLONK_MSM_PLAN_NBLK] = (int32_t)p.g.nblk;
    out[PLONK_MSM_PLAN_IDX_BITS] = (int32_t)p.g.idx_bits; out[PLONK_MSM_PLAN_PACKED] = p.packed; out[PLONK_MSM_PLAN_STAGED] = p.staged;
    out[PLONK_MSM_PLAN_STAGE_CAP] = (int32_t)p.g.stage_cap; out[PLONK_MSM_PLAN_FUSED_ORDER] = p.fused_order; out[PLONK_MSM_PLAN_NLEV] = p.nlev;
    out[PLONK_MSM_PLAN_LAST_K] = p.nlev ? (int32_t)p.lev_k[p.nlev - 1] : 0; out[PLONK_MSM_PLAN_GSPLIT] = (int32_t)p.gsplit;
    out[PLONK_MSM_PLAN_HEAVY_THRESH] = (int32_t)std::min<uint32_t>(p.heavy_thresh, 0x7fffffffu); out[PLONK_MSM_PLAN_PERSISTENT] = p.persistent;
    out[PLONK_MSM_PLAN_GRID_MODE] = p.grid_mode; out[PLONK_MSM_PLAN_STAGE_MAX_CHUNKS] = (int32_t)STAGE_MAX_CHUNKS; out[PLONK_MSM_PLAN_STAGE_THREADS] = STAGE_THREADS;
    out[PLONK_MSM_PLAN_HEAVY_BUCKET] = (int32_t)HEAVY_BUCKET; out[PLONK_MSM_PLAN_HEAVY_SEGS] = HEAVY_SEGS; out[PLONK_MSM_PLAN_SORT_SLICE_LOG] = SORT_SLICE_LOG;
    out[PLONK_MSM_PLAN_N] = (int32_t)sets.m; out[PLONK_MSM_PLAN_K] = kn; out[PLONK_MSM_PLAN_N_CU] = n_cu;
    out[PLONK_MSM_PLAN_ACC_GRID] = (int32_t)std::min<uint32_t>(p.acc_grid, 0x7fffffffu); out[PLONK_MSM_PLAN_BIN_SHIFT] = (int32_t)p.sg.bin_shift;
    return PLONK_OK;
}

// ---------------------------------------------------------------------------------------------- workspace
void msm_ws_release(MsmWorkspace& ws) {
    if (ws.d_buf) (void)hipFree(ws.d_buf);
    ws.d_buf = nullptr; ws.bytes = 0;
}

static int ensure_ws(MsmWorkspace& ws, size_t bytes) {
    if (ws.bytes >= bytes) return PLONK_OK;
    if (ws.d_buf) (void)hipFree(ws.d_buf);
    ws.d_buf = nullptr; ws.bytes = 0;
    HIP_TRY(hipMalloc(&ws.d_buf, bytes));
    ws.bytes = bytes;
    return PLONK_OK;
}

// The buffers of one launch set, carved from the workspace.  The integer ones (sort, scan, bucket order) know nothing of the curve.
struct MsmSortBuffers {
    uint32_t *dig, *tmp, *blk_hist, *blk_off, *offsets, *bsums, *sorted, *order;
    uint32_t *redo, *heavy;                  // [0] = count, [1..] = list; filled by the accumulation, zeroed by the bucket order
    uint32_t *ghist, *bin_cursor;            // SIZE_BINS words each, contiguous
};
template <int NQ> struct MsmBuffers : MsmSortBuffers {
    uint32_t* work;                          // work counter of the persistent accumulation
    BucketL<NQ> *buckets, *acc_arr, *s_arr;
    XyzzPt<NQ>* wsum;
    BucketL<NQ> *wpart, *hpart, *grid_r, *grid_c;
    XyzzPt<NQ>* gbits;
};
// Lays the buffers of plan p out from d_base, piece after piece, every one 256-byte aligned, and returns the bytes they take; with d_base = nullptr
// it only sizes, and the pointers it leaves in b mean nothing.
template <int NQ> static size_t msm_carve(const MsmPlan& p, void* d_base, MsmBuffers<NQ>& b) {
    size_t off = 0;
    auto take = [&](auto*& ptr, size_t count) {
        ptr = reinterpret_cast<std::decay_t<decltype(ptr)>>((uintptr_t)d_base + off);
        off = (off + count * sizeof(*ptr) + 255) / 256 * 256;
    };
    const size_t entries = (size_t)p.g.n * p.W, sums = (size_t)p.Wr * (p.nlev + 1);
    take(b.dig, entries);
    take(b.tmp, entries);
    take(b.blk_hist, p.nhist + 1);
    take(b.blk_off, p.nhist + 1);
    take(b.offsets, p.nsub + 1);
    take(b.bsums, p.nscan_blocks + 1);
    take(b.sorted, entries);
    take(b.order, p.nbuckets);
    take(b.redo, p.nbuckets + 1);
    static_assert(SIZE_BINS * 4 % 256 == 0, "bin_cursor follows ghist without a gap");
    take(b.ghist, SIZE_BINS);
    take(b.bin_cursor, SIZE_BINS);
    take(b.work, 1);
    take(b.heavy, p.max_heavy + 1);
    take(b.buckets, p.nbuckets);
    take(b.acc_arr, p.pyr);
    take(b.s_arr, p.pyr);
    take(b.wsum, sums);
    take(b.wpart, p.gsplit > 1 ? sums * p.gsplit : 0);
    take(b.hpart, p.max_heavy * HEAVY_SEGS);
    take(b.grid_r, p.grid_mode ? (size_t)p.Wr * (((size_t)1 << p.g_logL) + ((size_t)1 << p.g_logH)) : 0);       // column sums R_lo, then row sums C_hi
    if (d_base) b.grid_c = b.grid_r + ((size_t)p.Wr << p.g_logL);
    take(b.gbits, p.grid_mode ? (size_t)p.Wr * p.g_nbits : 0);
    return off;
}

// ---------------------------------------------------------------------------------------------- the phases: launches only, checked once by msm_slice
static int launch_sort(const MsmPlan& p, const MsmSortBuffers& b, const uint32_t* const* d_scalars, const size_t* lens, int K, bool scalars_mont,
                       const FrParams& FR, hipStream_t stream) {
    const SortGeom& g = p.g;
    const SizeHist szh{p.fused_order ? b.ghist : nullptr, p.sg.bin_shift, p.nbuckets};
    if (p.fused_order) HIP_TRY(hipMemsetAsync(b.ghist, 0, 2 * SIZE_BINS * 4, stream));
    ProfScope ps("msm_sort", stream);
    // digits + level-1 histograms, one workgroup per (slice, vector); the windows of a vector in groups of what the LDS budget holds
    ScalarVecs sv;
    for (int k = 0; k < MSM_MAX_GROUP; k++) { sv.ptr[k] = k < K ? d_scalars[k] : nullptr; sv.len[k] = k < K ? (uint64_t)lens[k] : 0; }
    const uint32_t np = (1u << g.lp) + 1;
    const int wgroup = std::min<int>(p.W1, std::max<int>(1, (int)(DIGHIST_LDS_WORDS / np)));
    static DeviceOnce attr0;
    HIP_TRY(attr0.run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_digits_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); }));
    hipLaunchKernelGGL(sort_digits_hist_kernel, dim3(g.nblk, (uint32_t)K), dim3(DIGHIST_THREADS), (size_t)wgroup * np * 4, stream, sv, g, p.c, p.W1, wgroup, b.dig,
                       b.blk_hist, scalars_mont ? 1 : 0, FR);
    hipLaunchKernelGGL(scan_block_sums_kernel, dim3((uint32_t)p.nscan_blocks), dim3(SCAN_THREADS), 0, stream, b.blk_hist, p.nhist, b.bsums);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(1024), 0, stream, b.bsums, p.nscan_blocks, b.blk_off + p.nhist);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((uint32_t)p.nscan_blocks), dim3(SCAN_THREADS), 0, stream, b.blk_hist, p.nhist, b.bsums, b.blk_off);
    static DeviceOnce attr;
    HIP_TRY(attr.run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_scatter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); }));
    hipLaunchKernelGGL(sort_scatter_kernel, dim3(g.nblk, p.W), dim3(SCATTER_THREADS), (2 * ((size_t)(1u << g.lp) + 1) + 1 + SORT_SLICE) * 4, stream, b.dig, g,
                       b.blk_off, b.tmp);
    if (p.staged) {
        static DeviceOnce attr2;
        HIP_TRY(attr2.run([] { return hipFuncSetAttribute(reinterpret_cast<const void*>(&sort_partition_staged_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024); }));
        hipLaunchKernelGGL(sort_partition_staged_kernel, dim3(g.nreal), dim3(STAGE_THREADS), p.lds_staged, stream, b.tmp, g, b.blk_off, b.sorted, b.offsets, szh);
    } else {
        hipLaunchKernelGGL(sort_partition_kernel, dim3(g.nreal), dim3(256), (((size_t)1 << g.low_bits) + g.nblk) * 4, stream, b.tmp, g, b.blk_off, b.sorted, b.offsets, szh);
    }
    return PLONK_OK;
}

static int launch_bucket_order(const MsmPlan& p, const MsmSortBuffers& b, hipStream_t stream) {
    ProfScope ps("msm_bucket_order", stream);
    HIP_TRY(hipMemsetAsync(b.redo, 0, 4, stream));
    HIP_TRY(hipMemsetAsync(b.heavy, 0, 4, stream));
    const uint32_t bgrid = (uint32_t)((p.nbuckets + 255) / 256);
    if (p.fused_order) {
        hipLaunchKernelGGL(bucket_size_place_kernel, dim3(bgrid), dim3(256), 0, stream, b.offsets, p.nbuckets, p.sg, b.bin_cursor, b.order, (const uint32_t*)b.ghist);
    } else {
        HIP_TRY(hipMemsetAsync(b.ghist, 0, 2 * SIZE_BINS * 4, stream));
        hipLaunchKernelGGL(bucket_size_hist_kernel, dim3(bgrid), dim3(256), 0, stream, b.offsets, p.nbuckets, p.sg, b.ghist);
        hipLaunchKernelGGL(bucket_size_scan_kernel, dim3(1), dim3(SIZE_BINS), 0, stream, b.ghist, b.bin_cursor);
        hipLaunchKernelGGL(bucket_size_place_kernel, dim3(bgrid), dim3(256), 0, stream, b.offsets, p.nbuckets, p.sg, b.bin_cursor, b.order, (const uint32_t*)nullptr);
    }
    return PLONK_OK;
}

template <int NQ, bool FUSED_Y3>
static void launch_accumulate_kernel(const MsmPlan& p, const MsmBuffers<NQ>& b, const BaseRec<NQ>* d_bases, const LimbParams<NQ>& FLP, hipStream_t stream) {
    hipLaunchKernelGGL((msm_accumulate_kernel<NQ, FUSED_Y3>), dim3(p.acc_grid), dim3(256), 0, stream, d_bases, b.sorted, b.offsets, b.order, p.nbuckets, p.sg,
                       p.heavy_thresh, b.buckets, b.redo, b.redo + 1, b.heavy, b.heavy + 1, p.persistent ? b.work : nullptr, FLP);
}
// accumulate, the heavy buckets over HEAVY_SEGS workgroups each, and the buckets that met an exceptional addition again
template <int NQ>
static int launch_accumulate(const MsmPlan& p, const MsmBuffers<NQ>& b, const BaseRec<NQ>* d_bases, const LimbParams<NQ>& FLP, hipStream_t stream) {
    if (p.persistent) HIP_TRY(hipMemsetAsync(b.work, 0, 4, stream));
    { ProfScope ps("msm_accumulate_kernel", stream);
    if (p.fused_y3) launch_accumulate_kernel<NQ, true>(p, b, d_bases, FLP, stream);
    else launch_accumulate_kernel<NQ, false>(p, b, d_bases, FLP, stream); }
    { ProfScope ps("msm_heavy", stream);
    hipLaunchKernelGGL(msm_heavy_kernel<NQ>, dim3(128, HEAVY_SEGS), dim3(256), 256 * sizeof(BucketL<NQ>), stream, d_bases, b.sorted, b.offsets, p.sg,
                       b.heavy, b.heavy + 1, b.hpart, FLP);
    hipLaunchKernelGGL(msm_heavy_finish_kernel<NQ>, dim3(16), dim3(64), 0, stream, b.heavy, b.heavy + 1, b.hpart, b.buckets, FLP); }
    { ProfScope ps("msm_accumulate_redo_kernel", stream);
    hipLaunchKernelGGL(msm_accumulate_redo_kernel<NQ>, dim3(256), dim3(64), 0, stream, d_bases, b.sorted, b.offsets, p.sg, b.buckets, b.redo,
                       b.redo + 1, FLP); }
    return PLONK_OK;
}

// 5: the pyramid of running-sum passes, then the per-(level, window) sums -> wsum[w][nlev + 1]
template <int NQ> static int launch_reduce_pyramid(const MsmPlan& p, const MsmBuffers<NQ>& b, const LimbParams<NQ>& FLP, hipStream_t stream) {
    const uint32_t nsums = (uint32_t)(p.nlev + 1);
    SumJobs jobs = {};
    const BucketL<NQ>* in = b.buckets;
    uint64_t at = 0;
    for (int l = 0; l < p.nlev; l++) {
        const uint64_t total_chunks = (uint64_t)p.Wr * p.lev_nch[l];
        HIP_TRY(hipMemsetAsync(b.redo, 0, 4, stream));          // the accumulate redo list is dead by now: reuse it per level
        hipLaunchKernelGGL(msm_reduce_level_kernel<NQ>, dim3((uint32_t)((total_chunks + 255) / 256)), dim3(256), 0, stream, in, p.lev_n[l],
                           (uint32_t)p.lev_k[l], p.lev_nch[l], total_chunks, b.acc_arr + at, b.s_arr + at, b.redo, b.redo + 1, FLP);
        hipLaunchKernelGGL(msm_reduce_level_redo_kernel<NQ>, dim3(64), dim3(64), 0, stream, in, p.lev_n[l], (uint32_t)p.lev_k[l], p.lev_nch[l],
                           b.acc_arr + at, b.s_arr + at, b.redo, b.redo + 1, FLP);
        jobs.src[l] = b.acc_arr + at;
        jobs.count[l] = p.lev_nch[l];
        in = b.s_arr + at;
        at += total_chunks;
    }
    jobs.src[p.nlev] = in;            // the single entry left per window: Sigma (nb == 1: the bucket itself)
    jobs.count[p.nlev] = 1;
    if (p.gsplit > 1) {
        hipLaunchKernelGGL((msm_points_sum_kernel<NQ, true>), dim3(nsums, p.Wr, p.gsplit), dim3(256), 256 * sizeof(BucketL<NQ>), stream, jobs, (XyzzPt<NQ>*)nullptr,
                           nsums, p.gsplit, FLP, b.wpart);
        jobs = {};      // second launch: fold the gsplit partials of every (level, window)
        for (uint32_t l = 0; l < nsums; l++) {
            jobs.src[l] = b.wpart + (size_t)l * p.gsplit;
            jobs.count[l] = p.gsplit;
            jobs.wstride[l] = (uint64_t)nsums * p.gsplit;
        }
    }
    hipLaunchKernelGGL((msm_points_sum_kernel<NQ, false>), dim3(nsums, p.Wr, 1), dim3(256), 256 * sizeof(BucketL<NQ>), stream, jobs, b.wsum, nsums, 1u, FLP,
                       (BucketL<NQ>*)nullptr);
    return PLONK_OK;
}
// 5b ("msm_reduce_grid"): row / column sums, then the bit sums -> gbits[w][g_nbits]
template <int NQ> static int launch_reduce_grid(const MsmPlan& p, const MsmBuffers<NQ>& b, const LimbParams<NQ>& FLP, hipStream_t stream) {
    // segments per output: 64 interleaved segments keep the serial part shortest; problems with lanes to spare trade a tree level for a longer
    // serial part (T up to 8 inputs per lane) while the launch still has >= 2^18 lanes — fewer LDS tree additions per bucket
    auto pick_seg = [&](uint32_t logY) {
        uint32_t ls = std::min<uint32_t>(logY, 6);
        while (ls > 3 && (logY - ls) < 3 && (((uint64_t)p.Wr << p.cb) >> (logY - ls + 1)) >= ((uint64_t)1 << 18)) ls--;
        return ls;
    };
    const uint32_t log_segc = pick_seg(p.g_logH), log_segr = pick_seg(p.g_logL);
    const uint32_t cwc = 256u >> log_segc, cwr = 256u >> log_segr;
    const uint32_t colblocks = (uint32_t)((((uint64_t)1 << p.g_logL) + cwc - 1) / cwc), rowblocks = (uint32_t)((((uint64_t)1 << p.g_logH) + cwr - 1) / cwr);
    hipLaunchKernelGGL(msm_grid_sums_kernel<NQ>, dim3(colblocks + rowblocks, p.Wr), dim3(256), 256 * sizeof(BucketL<NQ>), stream, b.buckets, p.g_logL, p.g_logH, log_segc,
                       log_segr, colblocks, b.grid_r, b.grid_c, FLP);
    hipLaunchKernelGGL(msm_bit_sums_kernel<NQ>, dim3(p.g_nbits, p.Wr), dim3(256), 256 * sizeof(BucketL<NQ>), stream, b.grid_r, b.grid_c, p.g_logL, p.g_logH, b.gbits, FLP);
    return PLONK_OK;
}
template <int NQ> static int launch_reduce(const MsmPlan& p, const MsmBuffers<NQ>& b, const LimbParams<NQ>& FLP, hipStream_t stream) {
    ProfScope ps("msm_reduce", stream);
    return p.grid_mode ? launch_reduce_grid<NQ>(p, b, FLP, stream) : launch_reduce_pyramid<NQ>(p, b, FLP, stream);
}

// ---------------------------------------------------------------------------------------------- 6: fold (host)
// hw: the nlev + 1 sums of one window.  V_w = Sigma + sum_l nch_l A_l,  nch_l = nch_(l+1) * K_(l+1),  nch_(nlev-1) = 1:  Horner from level 0
template <int NQ> static XyzzPt<NQ> window_value_pyramid(const MsmPlan& p, const XyzzPt<NQ>* hw, const FpParams<NQ>& P) {
    XyzzPt<NQ> v = xyzz_inf<NQ>();
    for (int l = 0; l < p.nlev; l++) {
        if (!xyzz_is_inf(v))
            for (uint64_t k = p.lev_k[l]; k > 1; k >>= 1) v = xyzz_dbl(v, P);
        v = xyzz_add(v, hw[l], P);
    }
    return xyzz_add(v, hw[p.nlev], P);
}
// tr: the g_nbits bit sums of one window.  V_w = sum_(b <= logL) 2^b TR_b + 2^logL * sum_(b < logH) 2^b TC_b: one Horner over the merged
// coefficients, from the top bit
template <int NQ> static XyzzPt<NQ> window_value_grid(const MsmPlan& p, const XyzzPt<NQ>* tr, const FpParams<NQ>& P) {
    const int logL = (int)p.g_logL, logH = (int)p.g_logH;
    XyzzPt<NQ> v = xyzz_inf<NQ>();
    for (int b = logL + (logH ? logH - 1 : 0); b >= 0; b--) {
        if (!xyzz_is_inf(v)) v = xyzz_dbl(v, P);
        if (b <= logL) v = xyzz_add(v, tr[b], P);
        if (b >= logL && b - logL < logH) v = xyzz_add(v, tr[b + 1], P);       // TC_(b - logL): the TC follow the logL + 1 TR
    }
    return v;
}
// h: the downloaded sums of the Wr = K * G bucket sets, nlev + 1 (pyramid) or g_nbits (grid) each.  Vector k: total = sum_g 2^(c*g) * V_(k*G + g), Horner from the top set
template <int NQ> static void msm_fold(const MsmPlan& p, const XyzzPt<NQ>* h, int K, const FpParams<NQ>& P, XyzzPt<NQ>* h_result) {
    for (int k = 0; k < K; k++) {
        XyzzPt<NQ> total = xyzz_inf<NQ>();
        for (int w = (k + 1) * p.G - 1; w >= k * p.G; w--) {
            if (!xyzz_is_inf(total))
                for (int i = 0; i < p.c; i++) total = xyzz_dbl(total, P);
            total = xyzz_add(total, p.grid_mode ? window_value_grid<NQ>(p, h + (size_t)w * p.g_nbits, P) : window_value_pyramid<NQ>(p, h + (size_t)w * (p.nlev + 1), P), P);
        }
        h_result[k] = total;
    }
}

// ---------------------------------------------------------------------------------------------- driver
// K >= 1 scalar vectors against the SAME bases in one set of launches (the independent commitments of a prover round): vector k
// supplies the windows k*W1 .. (k+1)*W1 - 1 of one big (window, bucket) problem, so the sort, the bucket accumulation and the
// reduction pyramid each run once over K times the work — no per-MSM launch gaps, wave tails or host round trips, which is what
// bounds small MSMs (2^20 - 2^21 points per rank / per configs[1]).  lens[k] <= n valid scalars in vector k.
template <int NQ>
static int msm_slice(int curve, const BaseRec<NQ>* d_bases, const uint32_t* const* d_scalars, const size_t* lens, int K, bool scalars_mont,
                     size_t n, XyzzPt<NQ>* h_result, MsmWorkspace& ws, int window_bits, const MsmTable& tab, hipStream_t stream) {
    if (K > MSM_MAX_GROUP) return plonk_fail(PLONK_ERR_ARG, "msm: %d vectors in one launch set", K);
    int rc, n_cu = 0;
    if (ws.acc_persist != 0 && (rc = device_cu_count(&n_cu))) return rc;
    MsmPlan p;
    if ((rc = msm_plan(n, K, fr_params(curve).bits, window_bits, tab, ws, n_cu, p))) return rc;
    MsmBuffers<NQ> b;
    if ((rc = ensure_ws(ws, msm_carve<NQ>(p, nullptr, b)))) return rc;
    msm_carve<NQ>(p, ws.d_buf, b);

    const LimbParams<NQ>& FLP = fl_params<NQ>(curve);
    if ((rc = launch_sort(p, b, d_scalars, lens, K, scalars_mont, fr_params(curve), stream))) return rc;
    if ((rc = launch_bucket_order(p, b, stream))) return rc;
    if ((rc = launch_accumulate<NQ>(p, b, d_bases, FLP, stream))) return rc;
    if ((rc = launch_reduce<NQ>(p, b, FLP, stream))) return rc;
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "msm launch: %s", hipGetErrorString(e));

    std::vector<XyzzPt<NQ>> h((size_t)p.Wr * (p.grid_mode ? p.g_nbits : (uint32_t)p.nlev + 1));
    HIP_TRY(hipMemcpyAsync(h.data(), p.grid_mode ? b.gbits : b.wsum, h.size() * sizeof(XyzzPt<NQ>), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    msm_fold<NQ>(p, h.data(), K, fq_params<NQ>(curve), h_result);
    return PLONK_OK;
}

// K scalar vectors (lens[k] valid scalars each) against bases[0 .. n): out = K Jacobian points.  One msm_slice per launch set (msm_launch_sets).
template <int NQ>
static int msm_run_t(int curve, const void* d_bases, const uint32_t* const* d_scalars, const size_t* lens, int K, bool scalars_mont, size_t n, uint32_t* h_out_jac,
                     MsmWorkspace& ws, int window_bits, const MsmTable& tab, hipStream_t stream) {
    const FpParams<NQ>& P = fq_params<NQ>(curve);
    std::vector<XyzzPt<NQ>> total((size_t)K, xyzz_inf<NQ>());
    for (size_t s = 0; s < n; s += msm_slice_points(ws)) {
        const MsmLaunchSets sets = msm_launch_sets(n, K, s, fr_params(curve).bits, window_bits, tab, ws);
        for (int k0 = 0; k0 < K; k0 += sets.group) {
            const int kn = sets.kn(K, k0);
            std::vector<const uint32_t*> ptrs(kn);
            std::vector<size_t> ln(kn);
            for (int k = 0; k < kn; k++) {
                ptrs[k] = d_scalars[k0 + k] + 8 * s;
                ln[k] = lens[k0 + k] > s ? std::min(lens[k0 + k] - s, sets.m) : 0;
            }
            std::vector<XyzzPt<NQ>> part(kn);
            int rc = msm_slice<NQ>(curve, (const BaseRec<NQ>*)d_bases + s, ptrs.data(), ln.data(), kn, scalars_mont, sets.m, part.data(), ws,
                                   window_bits, tab, stream);
            if (rc) return rc;
            for (int k = 0; k < kn; k++) total[k0 + k] = xyzz_add(total[k0 + k], part[k], P);
        }
    }
    for (int k = 0; k < K; k++) {
        JacPt<NQ> j = jac_from_xyzz_normalised(total[k], P);
        memcpy((char*)h_out_jac + (size_t)k * sizeof j, &j, sizeof j);
    }
    return PLONK_OK;
}

int msm_run_many(int curve, const void* d_bases, const uint32_t* const* d_scalars, const size_t* lens, int K, bool scalars_mont, size_t n, uint32_t* h_out_jac,
                 MsmWorkspace& ws, int window_bits, const MsmTable& tab, hipStream_t stream) {
    if (K <= 0) return PLONK_OK;
    if (curve == PLONK_BN254) return msm_run_t<8>(curve, d_bases, d_scalars, lens, K, scalars_mont, n, h_out_jac, ws, window_bits, tab, stream);
    return msm_run_t<12>(curve, d_bases, d_scalars, lens, K, scalars_mont, n, h_out_jac, ws, window_bits, tab, stream);
}

int msm_run(int curve, const void* d_bases, const uint32_t* d_scalars, bool scalars_mont, size_t n, uint32_t* h_out_jac, MsmWorkspace& ws, int window_bits,
            const MsmTable& tab, hipStream_t stream) {
    return msm_run_many(curve, d_bases, &d_scalars, &n, 1, scalars_mont, n, h_out_jac, ws, window_bits, tab, stream);
}

template <int NQ> static void jac_add_host_t(int curve, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    const FpParams<NQ>& P = fq_params<NQ>(curve);
    JacPt<NQ> ja, jb;
    memcpy(&ja, a, sizeof ja); memcpy(&jb, b, sizeof jb);
    XyzzPt<NQ> s = xyzz_add(xyzz_from_jac(ja, P), xyzz_from_jac(jb, P), P);
    JacPt<NQ> r = jac_from_xyzz_normalised(s, P);
    memcpy(out, &r, sizeof r);
}
int msm_jac_add_host(int curve, const uint32_t* a, const uint32_t* b, uint32_t* out) {
    if (curve == PLONK_BN254) jac_add_host_t<8>(curve, a, b, out); else jac_add_host_t<12>(curve, a, b, out);
    return PLONK_OK;
}
template <int NQ> static void jac_to_affine_host_t(int curve, const uint32_t* jac, uint32_t* out_xy, int* is_inf) {
    const FpParams<NQ>& P = fq_params<NQ>(curve);
    JacPt<NQ> j;
    memcpy(&j, jac, sizeof j);
    XyzzPt<NQ> x = xyzz_from_jac(j, P);
    *is_inf = xyzz_is_inf(x) ? 1 : 0;
    AffPt<NQ> a = xyzz_to_affine(x, P);
    if (*is_inf) a.y = fp_one(P);          // arkworks' affine zero is (0, 1, infinity = true)
    memcpy(out_xy, &a, sizeof a);
}
int msm_jac_to_affine_host(int curve, const uint32_t* jac, uint32_t* out_xy, int* is_inf) {
    if (curve == PLONK_BN254) jac_to_affine_host_t<8>(curve, jac, out_xy, is_inf); else jac_to_affine_host_t<12>(curve, jac, out_xy, is_inf);
    return PLONK_OK;
}
