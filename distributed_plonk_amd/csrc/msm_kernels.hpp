// msm_kernels.hpp — the device side of the Pippenger MSM (msm_engine.hip describes the algorithm and holds the planner and the launches):
// the kernels in pipeline order, the geometry and argument structs they take and the launch-shape constants the host shares with them.
#pragma once
#include "ec.hpp"
#include "ec_lazy.hpp"

#define BASES_BAD_CURVE 1u
#define BASES_BAD_RANGE 2u
#define BASES_BAD_FLAG 4u

// Wave priority of everything in an MSM that is NOT the bucket accumulation (build flag -DMSM_SIDE_PRIO=1..3; default 0 = no instruction): a SIMD's
// arbiter issues the highest-priority ready wave first and the oldest among equals, so beside another stream's accumulation (four long-lived
// VALU-bound waves per SIMD) the short memory- / latency-bound phases of the next MSM otherwise queue behind it for every instruction.
#ifndef MSM_SIDE_PRIO
#define MSM_SIDE_PRIO 0
#endif
#if MSM_SIDE_PRIO > 0
#define MSM_SIDE_PRIO_ENTER() __builtin_amdgcn_s_setprio(MSM_SIDE_PRIO)
#else
#define MSM_SIDE_PRIO_ENTER() ((void)0)
#endif

// ---------------------------------------------------------------------------------------------- helpers
template <typename T> __device__ __forceinline__ T load16(const T* p) {
    static_assert(sizeof(T) % 16 == 0, "16-byte multiple");
    T r;
    const uint4* s = reinterpret_cast<const uint4*>(p);
    uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
    return r;
}
template <typename T> __device__ __forceinline__ void store16(T* p, const T& v) {
    uint4* d = reinterpret_cast<uint4*>(p);
    const uint4* s = reinterpret_cast<const uint4*>(&v);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 16; i++) d[i] = s[i];
}

// Signed c-bit digits: d_w in [-2^(c-1), 2^(c-1)], sum_w d_w 2^(wc) = s.  Bucket index |d|-1 in [0, 2^(c-1)),
// the sign travels in bit 31 of the sorted point index (a negative digit adds -P: y -> -y).  Halves the
// bucket count (and the reduction work) of the unsigned decomposition arkworks uses; the group element
// is the same.  W*c >= bits+1 guarantees the last carry is absorbed.
__device__ __forceinline__ uint32_t scalar_raw_digit(const uint32_t* s, int bit0, int c) {
    const int limb = bit0 >> 5, off = bit0 & 31;
    if (limb >= 8) return 0;
    uint64_t v = s[limb];
    if (limb + 1 < 8) v |= (uint64_t)s[limb + 1] << 32;
    return (uint32_t)(v >> off) & ((1u << c) - 1);
}

// ---- 3: two-level LDS-staged counting sort of the (window, bucket) keys.
// Level 1 splits every window into 2^lp partitions by the top bits of the bucket index (all traffic in
// contiguous pieces, no global atomics: per-slice histograms + one exclusive scan give every (slice, partition)
// its exact range).  Level 2 sorts one partition per workgroup with LDS counters; its ~64 KiB of entries stay
// in L2.  Replaces a histogram + scatter pair that issued one HBM atomic and one 4-byte random store per
// (point, window) — 16x write amplification once n*W*4 B outgrows the 256 MiB Infinity Cache.
#define SORT_SLICE_LOG 14
#define SORT_SLICE (1 << SORT_SLICE_LOG)      // entries per level-1 workgroup
// A level-1 entry is  bucket_low << 15 | sign << 14 | (point index - slice start): the slice number is not stored, the
// level-2 workgroup recovers it from the entry's position (its partition is the concatenation of one run per slice,
// whose boundaries are the scanned histogram).  This keeps 2^10 level-1 partitions — 16-entry contiguous runs per
// (slice, partition) — for every window width; packing the full point index used to force 2^12 partitions (4-entry runs,
// sort 5.7 -> 10 ms) once c reached 20.
struct SortGeom {
    uint64_t n;
    int W, cb, lp, low_bits;
    uint32_t nblk;               // slices per window
    uint32_t nreal;              // W << lp : real partitions; the W "digit == 0" partitions follow them
    uint32_t idx_bits;           // > 0: level-1 entries carry the FULL point index in idx_bits bits (low_bits + 1 + idx_bits <= 32), so the
                                 // level-2 workgroup needs no search for the slice; 0: index within the slice only (wide windows / huge n)
    uint32_t stage_cap;          // entries the staged level-2 kernel orders in LDS at a time (what its LDS budget leaves beside the counters and slice starts)
};

// ---- 1 + level-1 histograms in ONE pass over the scalars (one workgroup per (slice, scalar vector)).
// Digits, planar: dig[w*n + i] = magnitude | sign << 31   (magnitude 0 = no contribution).
// scalars_mont != 0: the scalars are Fr in Montgomery form and `into_repr` (commit_polynomial, worker.rs:117-123) is taken here,
// on the fly, instead of in a separate pass that wrote 32 B per scalar to HBM and read them back.
// `len` <= n scalars of a vector are valid; positions len .. n-1 get zero digits (a batch of commitments pads its shorter polynomials).
// Every lane cuts its scalars into all W1 digits, writes them and counts each in the LDS histogram of its window: the digits are not
// read back for the histograms (one launch per vector and one pass over `dig` less than a digits kernel followed by a histogram kernel).
// The W1 * (2^lp + 1) counters of a vector are taken in GROUPS of `wgroup` windows where they outgrow DIGHIST_LDS_WORDS (narrow windows:
// many of them); the groups after the first read back the digits this very lane wrote.
#define MSM_MAX_GROUP 64                      // scalar vectors per launch set (msm_group)
#define DIGHIST_THREADS 1024                  // 16 scalars per lane; two workgroups = eight waves per SIMD
#define DIGHIST_LDS_WORDS (78 * 256)          // 78 KiB of counters at most: two workgroups per CU, like the level-1 scatter
struct ScalarVecs {
    const uint32_t* ptr[MSM_MAX_GROUP];
    uint64_t len[MSM_MAX_GROUP];
};
__global__ void __launch_bounds__(DIGHIST_THREADS, 8) sort_digits_hist_kernel(const ScalarVecs sv, SortGeom g, int c, int W1, int wgroup, uint32_t* dig,
                                                                           uint32_t* __restrict__ blk_hist, int scalars_mont, const FpParams<8> FR) {
    MSM_SIDE_PRIO_ENTER();
    extern __shared__ uint32_t h[];                       // [wgroup][2^lp + 1], last bin of a window: zero digits
    const uint32_t np = (1u << g.lp) + 1;
    const uint32_t kv = blockIdx.y, blk = blockIdx.x;
    const uint32_t* __restrict__ scalars = sv.ptr[kv];
    const uint64_t len = sv.len[kv];
    const uint64_t beg = (uint64_t)blk * SORT_SLICE, end = beg + SORT_SLICE < g.n ? beg + SORT_SLICE : g.n;
    uint32_t* d = dig + (uint64_t)kv * W1 * g.n;
    const uint32_t half = 1u << (c - 1);
    for (int w0 = 0; w0 < W1; w0 += wgroup) {
        const int w1 = w0 + wgroup < W1 ? w0 + wgroup : W1;
        const uint32_t nh = (uint32_t)(w1 - w0) * np;
        for (uint32_t k = threadIdx.x; k < nh; k += blockDim.x) h[k] = 0;
        __syncthreads();
        for (uint64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
            if (w0 > 0) {                                 // later group: the digits are there
                for (int w = w0; w < w1; w++) {
                    const uint32_t mag = d[(uint64_t)w * g.n + i] & 0x7fffffffu;
                    atomicAdd(&h[(uint32_t)(w - w0) * np + (mag ? ((mag - 1) >> g.low_bits) : (np - 1))], 1u);
                }
                continue;
            }
            if (i >= len) {
                for (int w = 0; w < W1; w++) {
                    d[(uint64_t)w * g.n + i] = 0;
                    if (w < w1) atomicAdd(&h[(uint32_t)w * np + (np - 1)], 1u);
                }
                continue;
            }
            uint32_t s[8];
            const uint4* sp = reinterpret_cast<const uint4*>(scalars + 8 * i);
            const uint4 lo = sp[0], hi = sp[1];
            s[0] = lo.x; s[1] = lo.y; s[2] = lo.z; s[3] = lo.w; s[4] = hi.x; s[5] = hi.y; s[6] = hi.z; s[7] = hi.w;
            if (scalars_mont) {
                Fp<8> v;
#pragma unroll
                for (int k = 0; k < 8; k++) v.l[k] = s[k];
                v = fp_from_mont(v, FR);
#pragma unroll
                for (int k = 0; k < 8; k++) s[k] = v.l[k];
            }
            uint32_t carry = 0;
            for (int w = 0; w < W1; w++) {
                // static limb selection keeps s[] in registers
                const int bit0 = w * c, limb = bit0 >> 5, off = bit0 & 31;
                uint64_t v = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    if (k == limb) v |= s[k];
                    if (k == limb + 1) v |= (uint64_t)s[k] << 32;
                }
                const uint32_t raw = ((uint32_t)(v >> off) & ((1u << c) - 1)) + carry;
                carry = raw > half;
                const uint32_t mag = carry ? (1u << c) - raw : raw;
                d[(uint64_t)w * g.n + i] = mag | (carry << 31);
                if (w < w1) atomicAdd(&h[(uint32_t)w * np + (mag ? ((mag - 1) >> g.low_bits) : (np - 1))], 1u);
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < nh; k += blockDim.x) {
            const uint32_t wl = k / np, kk = k - wl * np;
            const uint64_t w = (uint64_t)kv * W1 + w0 + wl;           // window of the whole batch
            const uint64_t pid = (kk == np - 1) ? (uint64_t)g.nreal + w : (w << g.lp) + kk;
            blk_hist[pid * g.nblk + blk] = h[k];
        }
        __syncthreads();                                  // the counters are free for the next group
    }
}

// Level-1 scatter.  A wave's 64 entries go to 64 different partitions, so storing them straight to HBM costs one
// write transaction per 4-byte entry (measured WRITE_SIZE 7x the payload).  Instead the slice is first ordered by
// partition in LDS (counts -> exclusive scan -> ranks), then copied out with consecutive lanes writing consecutive
// addresses of each partition's run.
#define SCATTER_THREADS 1024     // 16 waves on a ~74 KiB LDS footprint: two workgroups = eight waves per SIMD hide the LDS-atomic and HBM latency
#define SCATTER_PER (SORT_SLICE / SCATTER_THREADS)      // digits of the slice per lane
__global__ void __launch_bounds__(SCATTER_THREADS, 8) sort_scatter_kernel(const uint32_t* __restrict__ dig, SortGeom g, const uint32_t* __restrict__ blk_off,
                                                                       uint32_t* __restrict__ tmp) {
    MSM_SIDE_PRIO_ENTER();
    extern __shared__ uint32_t sm[];
    const uint32_t np = (1u << g.lp) + 1;                 // last bin: zero digits (dropped)
    uint32_t* cnt = sm;                                   // [np]   counts, then running cursors
    uint32_t* loc = sm + np;                              // [np+1] exclusive local offsets
    uint32_t* buf = sm + 2 * np + 1;                      // [SORT_SLICE] entries ordered by partition
    const uint32_t w = blockIdx.y, blk = blockIdx.x;
    for (uint32_t k = threadIdx.x; k < np; k += blockDim.x) cnt[k] = 0;
    __syncthreads();
    const uint64_t beg = (uint64_t)blk * SORT_SLICE, end = beg + SORT_SLICE < g.n ? beg + SORT_SLICE : g.n;
    const uint32_t* d = dig + (uint64_t)w * g.n;
    // the lane's SCATTER_PER digits are read ONCE and stay in registers for the rank sweep below; what lies beyond `end` (the last, partial
    // slice) reads as a zero digit, which neither sweep counts (the zero bin stays empty here: only the histogram kernel needs it)
    uint32_t e[SCATTER_PER];
#pragma unroll
    for (int r = 0; r < SCATTER_PER; r++) {
        const uint64_t i = beg + threadIdx.x + (uint32_t)r * SCATTER_THREADS;
        e[r] = i < end ? d[i] : 0u;
    }
#pragma unroll
    for (int r = 0; r < SCATTER_PER; r++) {
        const uint32_t mag = e[r] & 0x7fffffffu;
        if (mag) atomicAdd(&cnt[(mag - 1) >> g.low_bits], 1u);
    }
    __syncthreads();
    // exclusive scan of the np counts (np <= 8193): every lane a contiguous strip, then a strip-sum scan
    __shared__ uint32_t strip[SCATTER_THREADS];
    const uint32_t per = (np + blockDim.x - 1) / blockDim.x;
    const uint32_t s0 = threadIdx.x * per < np ? threadIdx.x * per : np, s1 = s0 + per < np ? s0 + per : np;
    uint32_t acc = 0;
    for (uint32_t k = s0; k < s1; k++) acc += cnt[k];
    strip[threadIdx.x] = acc;
    __syncthreads();
    for (int dd = 1; dd < SCATTER_THREADS; dd <<= 1) {
        const uint32_t t = (int)threadIdx.x >= dd ? strip[threadIdx.x - dd] : 0;
        __syncthreads();
        strip[threadIdx.x] += t;
        __syncthreads();
    }
    uint32_t run = strip[threadIdx.x] - acc;
    for (uint32_t k = s0; k < s1; k++) { const uint32_t v = cnt[k]; loc[k] = run; cnt[k] = run; run += v; }
    if (threadIdx.x == blockDim.x - 1) loc[np] = strip[blockDim.x - 1];
    __syncthreads();
    // rank into LDS.  While the packed entry leaves room (low_bits + 15 + lp <= 32, i.e. windows up to 18 bits) the partition
    // number rides in the entry's top bits, so the copy-out below needs no search.
    const uint32_t low_mask = (1u << g.low_bits) - 1;
    const uint32_t ebits = (uint32_t)g.low_bits + SORT_SLICE_LOG + 1;
    const bool packed = ebits + (uint32_t)g.lp <= 32;
#pragma unroll
    for (int r = 0; r < SCATTER_PER; r++) {
        const uint32_t mag = e[r] & 0x7fffffffu;
        if (!mag) continue;
        const uint32_t key = mag - 1, part = key >> g.low_bits;
        const uint32_t pos = atomicAdd(&cnt[part], 1u);
        uint32_t v = ((key & low_mask) << (SORT_SLICE_LOG + 1)) | ((e[r] >> 31) << SORT_SLICE_LOG) | (threadIdx.x + (uint32_t)r * SCATTER_THREADS);
        if (packed && g.lp) v |= part << ebits;
        buf[pos] = v;
    }
    __syncthreads();
    // copy out: position j of the ordered slice belongs to the partition whose [loc[k], loc[k+1]) contains it
    const uint32_t nreal_local = loc[np - 1];             // entries with a non-zero digit
    const uint32_t emask = ebits >= 32 ? 0xffffffffu : ((1u << ebits) - 1);
    for (uint32_t j = threadIdx.x; j < nreal_local; j += blockDim.x) {
        const uint32_t v = buf[j];
        uint32_t lo;
        if (packed) {
            lo = g.lp ? (v >> ebits) : 0;
        } else {
            lo = 0;
            uint32_t hi = np - 1;                         // largest k with loc[k] <= j
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (loc[mid] <= j) lo = mid; else hi = mid; }
        }
        const uint64_t pid = ((uint64_t)w << g.lp) + lo;
        uint32_t out = packed ? (v & emask) : v;
        if (g.idx_bits) {                                 // re-pack with the full point index: low | sign | (slice start + index in slice)
            const uint32_t in = out & (SORT_SLICE - 1), sg = (out >> SORT_SLICE_LOG) & 1u, lowb = out >> (SORT_SLICE_LOG + 1);
            out = (lowb << (g.idx_bits + 1)) | (sg << g.idx_bits) | (uint32_t)(beg + in);
        }
        tmp[blk_off[pid * g.nblk + blk] + (j - loc[lo])] = out;
    }
}

// one workgroup per real partition: final order + bucket offsets
// The bucket-size histogram of step 3b (SIZE_BINS bins, bin 0 = largest) is taken HERE when `ghist` is given (round 5: plain bucket sets, where a
// bucket is one sorted segment and its size is the count this kernel has in its hands): one launch and one pass over the offsets less per MSM.
#define SIZE_BINS 256
struct SizeHist {
    uint32_t* ghist;          // nullptr: step 3b counts the sizes itself (bucket sets merged over windows: the fixed-base table)
    uint32_t bin_shift;
    uint64_t nbuckets;
};
__device__ __forceinline__ uint32_t size_bin_of(uint32_t entries, uint32_t bin_shift) {
    const uint32_t sz = entries >> bin_shift;
    return (SIZE_BINS - 1) - (sz < SIZE_BINS - 1 ? sz : SIZE_BINS - 1);      // bin 0 = largest
}
__global__ void __launch_bounds__(256) sort_partition_kernel(const uint32_t* __restrict__ tmp, SortGeom g, const uint32_t* __restrict__ blk_off,
                                                             uint32_t* __restrict__ sorted, uint32_t* __restrict__ offsets, const SizeHist sz) {
    MSM_SIDE_PRIO_ENTER();
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t shist[SIZE_BINS];
    if (sz.ghist) shist[threadIdx.x] = 0;
    const uint32_t nlow = 1u << g.low_bits;
    uint32_t* cnt = lds;                       // [2^low_bits] counts -> cursors
    uint32_t* run0 = lds + nlow;               // [nblk] start of every slice's run inside this partition
    const uint64_t pid = blockIdx.x;
    const uint32_t* po = blk_off + pid * g.nblk;
    const uint32_t pbeg = po[0], pend = po[g.nblk];
    for (uint32_t k = threadIdx.x; k < nlow; k += blockDim.x) cnt[k] = 0;
    for (uint32_t k = threadIdx.x; k < g.nblk; k += blockDim.x) run0[k] = po[k];
    __syncthreads();
    const int sh = g.idx_bits ? (int)g.idx_bits + 1 : SORT_SLICE_LOG + 1;
    for (uint32_t j = pbeg + threadIdx.x; j < pend; j += blockDim.x) atomicAdd(&cnt[tmp[j] >> sh], 1u);
    __syncthreads();
    if (threadIdx.x == 0) {                    // nlow <= 2048: a serial exclusive scan is negligible
        uint32_t run = pbeg;
        for (uint32_t k = 0; k < nlow; k++) {
            const uint32_t v = cnt[k];
            cnt[k] = run;
            run += v;
            if (sz.ghist && (pid << g.low_bits) + k < sz.nbuckets) shist[size_bin_of(v, sz.bin_shift)]++;
        }
    }
    __syncthreads();
    if (sz.ghist && shist[threadIdx.x]) atomicAdd(&sz.ghist[threadIdx.x], shist[threadIdx.x]);
    for (uint32_t k = threadIdx.x; k < nlow; k += blockDim.x) offsets[(pid << g.low_bits) + k] = cnt[k];
    if (pid == g.nreal - 1 && threadIdx.x == 0) offsets[(uint64_t)g.nreal << g.low_bits] = pend;      // end sentinel
    __syncthreads();
    const uint32_t in_mask = SORT_SLICE - 1;
    // Final placement: direct 4-byte scatter into the partition's 2^low_bits bucket runs.  Fine while the open runs of the
    // workgroups in flight fit the write-combining reach of L1/L2 (c <= 17 at 2^24: 1.5 ms); at c = 20 (512 runs per
    // partition) it costs 6.3 ms.  Ordering the partition in LDS first was measured and rejected: 64 KiB of staging per
    // workgroup leaves one workgroup per CU (7.3 ms), and 4096-entry partitions that would stage in 16 KiB double the
    // level-1 kernels instead (profiles/r01_msm_table_experiment.txt).
    if (g.idx_bits) {                          // entries carry the full point index: no slice search
        const uint32_t imask = (1u << g.idx_bits) - 1;
        for (uint32_t j = pbeg + threadIdx.x; j < pend; j += blockDim.x) {
            const uint32_t e = tmp[j];
            const uint32_t pos = atomicAdd(&cnt[e >> sh], 1u);
            sorted[pos] = (e & imask) | (((e >> g.idx_bits) & 1u) << 31);
        }
        return;
    }
    for (uint32_t j = pbeg + threadIdx.x; j < pend; j += blockDim.x) {
        const uint32_t e = tmp[j];
        uint32_t lo = 0, hi = g.nblk;          // slice = largest b with run0[b] <= j
        while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (run0[mid] <= j) lo = mid; else hi = mid; }
        const uint32_t pos = atomicAdd(&cnt[e >> sh], 1u);
        sorted[pos] = ((lo << SORT_SLICE_LOG) + (e & in_mask)) | (((e >> SORT_SLICE_LOG) & 1u) << 31);
    }
}

// Level 2 for WIDE windows (2^low_bits >= 256 buckets per partition, i.e. c >= 19 at 2^24 points): the direct scatter above keeps
// 512 one-cache-line runs open per workgroup for the workgroup's whole life, and with ~2000 workgroups in flight those partial lines
// fall out of L2 before they are full (6.2 ms at c = 20 against 1.5 ms at c = 17 for the same bytes).  Here the partition is ordered in
// LDS and leaves in consecutive addresses: counts -> exclusive scan -> ranks into the LDS buffer -> coalesced copy-out.  1024 lanes on
// ~78 KiB of LDS: two workgroups = eight waves per SIMD, like the level-1 scatter.  A partition larger than the buffer (g.stage_cap
// entries: above 2^24 points a partition holds 2^15 and more, and skewed scalars can fill one at any size) is ordered in several CHUNKS
// of consecutive buckets: every chunk streams the partition again (its 128 - 256 KiB are L2 / Infinity-Cache resident) and stages only
// the entries of its own buckets; a single chunk that still does not fit (one huge bucket) takes the direct path.  Late round 3: before,
// such partitions — all of them at 2^25 and 2^26 points — fell back to the direct kernel: sort 17.3 / 35.6 ms beside 30.6 / 59.9 ms of accumulation.
#define STAGE_THREADS 1024
#define STAGE_MAX_CHUNKS 8u
#define STAGE_KEEP 18              // entries a lane keeps in registers between the two sweeps: 18 * 1024 = the largest buffer the 78 KiB leave at 2^24 points
__global__ void __launch_bounds__(STAGE_THREADS, 8) sort_partition_staged_kernel(const uint32_t* __restrict__ tmp, SortGeom g, const uint32_t* __restrict__ blk_off,
                                                                              uint32_t* __restrict__ sorted, uint32_t* __restrict__ offsets, const SizeHist sz) {
    MSM_SIDE_PRIO_ENTER();
    extern __shared__ uint32_t lds[];
    __shared__ uint32_t shist[SIZE_BINS];
    if (sz.ghist && threadIdx.x < SIZE_BINS) shist[threadIdx.x] = 0;
    const uint32_t nlow = 1u << g.low_bits;
    uint32_t* cnt = lds;                       // [2^low_bits] counts -> cursors (relative to the partition start)
    uint32_t* run0 = lds + nlow;               // [nblk] start of every slice's run inside this partition (idx_bits == 0 only)
    uint32_t* buf = run0 + (g.idx_bits ? 0 : g.nblk);      // [stage_cap] final entries in bucket order
    uint32_t* strip = buf;                     // [STAGE_THREADS] scratch of the scan, dead before buf is filled (stage_cap >= STAGE_THREADS)
    const uint64_t pid = blockIdx.x;
    const uint32_t* po = blk_off + pid * g.nblk;
    const uint32_t pbeg = po[0], pend = po[g.nblk], len = pend - pbeg;
    const int sh = g.idx_bits ? (int)g.idx_bits + 1 : SORT_SLICE_LOG + 1;
    for (uint32_t k = threadIdx.x; k < nlow; k += blockDim.x) cnt[k] = 0;
    if (!g.idx_bits)
        for (uint32_t k = threadIdx.x; k < g.nblk; k += blockDim.x) run0[k] = po[k];
    __syncthreads();
    // The common case — the partition fits the buffer in one chunk AND a lane's share fits STAGE_KEEP registers — reads the partition ONCE: the
    // entries of the count sweep stay in registers for the placement.  Everything else (chunks, the direct path, a partition of more than
    // STAGE_KEEP * STAGE_THREADS entries) streams it again below.
    const bool keep = len <= g.stage_cap && len <= (uint32_t)STAGE_KEEP * STAGE_THREADS;
    uint32_t ent[STAGE_KEEP];
    if (keep) {
#pragma unroll
        for (int r = 0; r < STAGE_KEEP; r++) {
            const uint32_t j = pbeg + threadIdx.x + (uint32_t)r * STAGE_THREADS;
            ent[r] = j < pend ? tmp[j] : 0u;
            if (j < pend) atomicAdd(&cnt[ent[r] >> sh], 1u);
        }
    } else {
        for (uint32_t j = pbeg + threadIdx.x; j < pend; j += blockDim.x) atomicAdd(&cnt[tmp[j] >> sh], 1u);
    }
    __syncthreads();
    // exclusive scan of the nlow (<= 2048) counts: two entries per lane at most, then a strip-sum scan
    const uint32_t per = (nlow + blockDim.x - 1) / blockDim.x;
    const uint32_t s0 = threadIdx.x * per < nlow ? threadIdx.x * per : nlow, s1 = s0 + per < nlow ? s0 + per : nlow;
    uint32_t acc = 0;
    for (uint32_t k = s0; k < s1; k++) acc += cnt[k];
    strip[threadIdx.x] = acc;
    __syncthreads();
    for (int dd = 1; dd < STAGE_THREADS; dd <<= 1) {
        const uint32_t t = (int)threadIdx.x >= dd ? strip[threadIdx.x - dd] : 0;
        __syncthreads();
        strip[threadIdx.x] += t;
        __syncthreads();
    }
    uint32_t run = strip[threadIdx.x] - acc;
    __syncthreads();                           // every lane has read its strip value: the scratch may be overwritten from here on
    for (uint32_t k = s0; k < s1; k++) {
        const uint32_t v = cnt[k];
        cnt[k] = run;
        offsets[(pid << g.low_bits) + k] = pbeg + run;
        run += v;
        if (sz.ghist && (pid << g.low_bits) + k < sz.nbuckets) atomicAdd(&shist[size_bin_of(v, sz.bin_shift)], 1u);      // (zeroed before the first barrier above)
    }
    if (pid == g.nreal - 1 && threadIdx.x == 0) offsets[(uint64_t)g.nreal << g.low_bits] = pend;      // end sentinel
    __syncthreads();
    if (sz.ghist && threadIdx.x < SIZE_BINS && shist[threadIdx.x]) atomicAdd(&sz.ghist[threadIdx.x], shist[threadIdx.x]);
    const uint32_t in_mask = SORT_SLICE - 1;
    const uint32_t imask = g.idx_bits ? (1u << g.idx_bits) - 1 : 0;
    if (keep) {                                // one chunk from the registers: the cursors start at 0 and end at len
#pragma unroll
        for (int r = 0; r < STAGE_KEEP; r++) {
            const uint32_t j = pbeg + threadIdx.x + (uint32_t)r * STAGE_THREADS;
            if (j >= pend) continue;
            const uint32_t e = ent[r];
            uint32_t val;
            if (g.idx_bits) {
                val = (e & imask) | (((e >> g.idx_bits) & 1u) << 31);
            } else {
                uint32_t lo = 0, hi = g.nblk;  // slice = largest b with run0[b] <= j
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (run0[mid] <= j) lo = mid; else hi = mid; }
                val = ((lo << SORT_SLICE_LOG) + (e & in_mask)) | (((e >> SORT_SLICE_LOG) & 1u) << 31);
            }
            buf[atomicAdd(&cnt[e >> sh], 1u)] = val;
        }
        __syncthreads();
        for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) sorted[pbeg + j] = buf[j];
        return;
    }
    // chunks of consecutive buckets: one when the partition fits the buffer, else sized for 3/4 of it (bucket sizes fluctuate)
    const uint32_t cap = g.stage_cap;
    // (a partition far beyond that — the 2^14-bucket top window of a c = 20 decomposition puts 2^19 entries in each of its partitions — would stream
    //  itself dozens of times from one workgroup: it takes the direct path in one pass, as before)
    uint32_t nch = len <= cap ? 1u : min(nlow, (len + (cap - cap / 4) - 1) / (cap - cap / 4));
    const bool direct = nch > STAGE_MAX_CHUNKS;
    if (direct) nch = 1;
    const uint32_t bper = (nlow + nch - 1) / nch;
    for (uint32_t k0 = 0; k0 < nlow; k0 += bper) {
        const uint32_t k1 = k0 + bper < nlow ? k0 + bper : nlow;
        const uint32_t base = cnt[k0], cend = k1 < nlow ? cnt[k1] : len;       // cursors of this chunk's buckets are still at their starts
        const bool staged = !direct && cend - base <= cap;
        __syncthreads();                       // all lanes hold base / cend before the cursors move
        for (uint32_t j = pbeg + threadIdx.x; j < pend; j += blockDim.x) {
            const uint32_t e = tmp[j], bk = e >> sh;
            if (bk < k0 || bk >= k1) continue;
            uint32_t val;
            if (g.idx_bits) {
                val = (e & imask) | (((e >> g.idx_bits) & 1u) << 31);
            } else {
                uint32_t lo = 0, hi = g.nblk;  // slice = largest b with run0[b] <= j
                while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (run0[mid] <= j) lo = mid; else hi = mid; }
                val = ((lo << SORT_SLICE_LOG) + (e & in_mask)) | (((e >> SORT_SLICE_LOG) & 1u) << 31);
            }
            const uint32_t pos = atomicAdd(&cnt[bk], 1u);
            if (staged) buf[pos - base] = val; else sorted[pbeg + pos] = val;
        }
        __syncthreads();
        if (staged)
            for (uint32_t j = threadIdx.x; j < cend - base; j += blockDim.x) sorted[pbeg + base + j] = buf[j];
        __syncthreads();                       // the buffer is free for the next chunk
    }
}

// ---------------------------------------------------------------------------------------------- 3b: schedule buckets by size
// One lane owns one bucket, so a wave runs as long as its fullest bucket.  A counting sort of the bucket
// ids by (clamped) size, largest first, puts equally loaded buckets in the same wave.
// Bucket sets.  Plain: one set per window.  With the fixed-base window table (msm_table_kernel): G sets per scalar vector — set s = k*G + g of
// vector k collects the windows w = g, g + G, g + 2G, ... < W1 of that vector; the entries of (window w, bucket b) are the sorted segment
// ((k*W1 + w) << cb) + b and their bases come from plane t = w / G of the table (2^(c*G*t) * P_i).  Plain mode is G = W1 (one segment, plane 0).
struct SetGeom {
    uint32_t cb;          // log2 buckets per set
    uint32_t G;           // sets per scalar vector
    uint32_t W1;          // windows per scalar vector
    uint32_t bin_shift;   // size-bin resolution (entries >> bin_shift)
    uint64_t tab_stride;  // points between the planes of the table (0: plain)
};
// first segment of set-bucket sb; the following ones are seg_step(g) apart
__device__ __forceinline__ uint64_t seg_first(const SetGeom& g, uint32_t sb, uint32_t* w0) {
    const uint32_t s = sb >> g.cb, b = sb & ((1u << g.cb) - 1u);
    const uint32_t k = s / g.G, gi = s - k * g.G;
    *w0 = gi;
    return (((uint64_t)k * g.W1 + gi) << g.cb) + b;
}
__device__ __forceinline__ uint64_t seg_step(const SetGeom& g) { return (uint64_t)g.G << g.cb; }
__device__ __forceinline__ uint32_t bucket_entries(const uint32_t* offsets, uint32_t sb, const SetGeom& g) {
    uint32_t w;
    uint64_t seg = seg_first(g, sb, &w);
    uint32_t sz = 0;
    for (; w < g.W1; w += g.G, seg += seg_step(g)) sz += offsets[seg + 1] - offsets[seg];
    return sz;
}
__device__ __forceinline__ uint32_t size_bin(const uint32_t* offsets, uint32_t sb, const SetGeom& g) {
    return size_bin_of(bucket_entries(offsets, sb, g), g.bin_shift);     // merged buckets hold more entries: the host scales them into the 256 bins
}
__global__ void __launch_bounds__(256) bucket_size_hist_kernel(const uint32_t* __restrict__ offsets, uint64_t nbuckets, SetGeom g, uint32_t* __restrict__ ghist) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t h[SIZE_BINS];
    h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b < nbuckets) atomicAdd(&h[size_bin(offsets, (uint32_t)b, g)], 1u);
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&ghist[threadIdx.x], h[threadIdx.x]);
}
__global__ void __launch_bounds__(SIZE_BINS) bucket_size_scan_kernel(const uint32_t* __restrict__ ghist, uint32_t* __restrict__ bin_cursor) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t buf[SIZE_BINS];
    const uint32_t v = ghist[threadIdx.x];
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int d = 1; d < SIZE_BINS; d <<= 1) {
        uint32_t t = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += t;
        __syncthreads();
    }
    bin_cursor[threadIdx.x] = buf[threadIdx.x] - v;
}
// ghist != nullptr (round 5): bin_cursor arrives ZEROED and every workgroup scans the finished histogram itself (256 values: eight LDS steps) — the
// one-workgroup scan launch in between is gone; ghist == nullptr: bin_cursor holds the scanned starts (bucket_size_scan_kernel).
__global__ void __launch_bounds__(256) bucket_size_place_kernel(const uint32_t* __restrict__ offsets, uint64_t nbuckets, SetGeom g,
                                                                uint32_t* __restrict__ bin_cursor, uint32_t* __restrict__ order, const uint32_t* __restrict__ ghist) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t h[SIZE_BINS];
    __shared__ uint32_t base[SIZE_BINS];
    __shared__ uint32_t pre[SIZE_BINS];
    h[threadIdx.x] = 0;
    uint32_t start = 0;
    if (ghist != nullptr) {
        const uint32_t v = ghist[threadIdx.x];
        pre[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < SIZE_BINS; d <<= 1) {
            const uint32_t t = (int)threadIdx.x >= d ? pre[threadIdx.x - d] : 0;
            __syncthreads();
            pre[threadIdx.x] += t;
            __syncthreads();
        }
        start = pre[threadIdx.x] - v;
    }
    __syncthreads();
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bin = 0, rank = 0;
    if (b < nbuckets) { bin = size_bin(offsets, (uint32_t)b, g); rank = atomicAdd(&h[bin], 1u); }
    __syncthreads();
    if (h[threadIdx.x]) base[threadIdx.x] = start + atomicAdd(&bin_cursor[threadIdx.x], h[threadIdx.x]);
    __syncthreads();
    if (b < nbuckets) order[base[bin] + rank] = (uint32_t)b;
}

// ---------------------------------------------------------------------------------------------- 2: exclusive scan (u32)
#define SCAN_ITEMS 16
#define SCAN_THREADS 256
#define SCAN_CHUNK (SCAN_ITEMS * SCAN_THREADS)

__global__ void __launch_bounds__(SCAN_THREADS) scan_block_sums_kernel(const uint32_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ block_sums) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t red[SCAN_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t s = 0;
    for (int k = 0; k < SCAN_ITEMS; k++) if (base + k < n) s += in[base + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int d = SCAN_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) red[threadIdx.x] += red[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) block_sums[blockIdx.x] = red[0];
}

__global__ void __launch_bounds__(1024) scan_top_kernel(uint32_t* __restrict__ block_sums, uint64_t nblocks, uint32_t* __restrict__ total_out) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t buf[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint64_t base = 0; base < nblocks; base += 1024) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t v = i < nblocks ? block_sums[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int d = 1; d < 1024; d <<= 1) {
            uint32_t t = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        const uint32_t incl = buf[threadIdx.x];
        if (i < nblocks) block_sums[i] = carry + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry += incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total_out = carry;
}

__global__ void __launch_bounds__(SCAN_THREADS) scan_apply_kernel(const uint32_t* __restrict__ in, uint64_t n, const uint32_t* __restrict__ block_offsets,
                                                                  uint32_t* __restrict__ out) {
    MSM_SIDE_PRIO_ENTER();
    __shared__ uint32_t buf[SCAN_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * SCAN_CHUNK + (uint64_t)threadIdx.x * SCAN_ITEMS;
    uint32_t v[SCAN_ITEMS];
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { v[k] = (base + k < n) ? in[base + k] : 0; s += v[k]; }
    buf[threadIdx.x] = s;
    __syncthreads();
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        uint32_t t = (int)threadIdx.x >= d ? buf[threadIdx.x - d] : 0;
        __syncthreads();
        buf[threadIdx.x] += t;
        __syncthreads();
    }
    uint32_t run = block_offsets[blockIdx.x] + buf[threadIdx.x] - s;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// ---------------------------------------------------------------------------------------------- 4: bucket accumulation
// Limb geometry of the lazy base-field arithmetic per curve (flimb.hpp)
template <int NQ> struct LimbGeom;
template <> struct LimbGeom<8> { static constexpr int NL = 9, B = 29; };      // BN254 Fq, R' = 2^261
template <> struct LimbGeom<12> { static constexpr int NL = 14, B = 28; };    // BLS12-381 Fq, R' = 2^392

template <typename T> __device__ __forceinline__ T load8(const T* p) {
    static_assert(sizeof(T) % 8 == 0, "8-byte multiple");
    T r;
    const uint2* s = reinterpret_cast<const uint2*>(p);
    uint2* d = reinterpret_cast<uint2*>(&r);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 8; i++) d[i] = s[i];
    return r;
}
template <typename T> __device__ __forceinline__ void store8(T* p, const T& v) {
    uint2* d = reinterpret_cast<uint2*>(p);
    const uint2* s = reinterpret_cast<const uint2*>(&v);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 8; i++) d[i] = s[i];
}

// Resident form of a base point (round 4).  Rounds 1-3 kept bases as unsaturated limbs (9 x 29 bits per coordinate: 72 B per BN254 point, 112 B on
// BLS12-381) so that a gather needed no re-limbing — but a 72-byte record straddles 64-byte sectors, and the accumulation gathers every base once
// per window: PMC showed 127 GB of fetches per batched launch for 3 GB of algorithmic bytes.  Bases now rest as the same canonical R'-Montgomery
// residues in SATURATED 32-bit words, x || y = 64 B (BN254) / 96 B (BLS12-381): a BN254 record is exactly one aligned 64-byte sector, fetched with
// four dwordx4 loads and re-limbed in registers (+30 of ~2500 VALU instructions per addition).  Infinity stays (0, 0).  Same box, alternating
// builds (profiles/r04_packed_bases_experiment.txt): accumulate 16.23 -> 15.6 ms at 2^24, commitments of the 2^24 step 275 -> 271 ms, of the 2^20
// step 23.9 -> 23.5 ms, BLS12-381 unchanged; 11 % less resident memory.
template <int NQ> using BaseRec = AffPt<NQ>;
template <int NQ> __device__ __forceinline__ AffL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> load_base(const BaseRec<NQ>* p) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const AffPt<NQ> a = load16(p);
    AffL<NL, B> r;
    r.x = fl_from_sat<NL, B, NQ>(a.x);
    r.y = fl_from_sat<NL, B, NQ>(a.y);
    return r;
}
template <int NQ> __device__ __forceinline__ void store_base(BaseRec<NQ>* p, const AffL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>& q) {   // q canonical (< p), normalised
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    AffPt<NQ> a;
    a.x = fl_to_sat<NL, B, NQ>(q.x);
    a.y = fl_to_sat<NL, B, NQ>(q.y);
    store16(p, a);
}

// SRS bases: reference layout (x||y, R = 2^(32N) Montgomery, canonical) -> resident limb form (R' Montgomery)
template <int NQ>
__global__ void __launch_bounds__(256) bases_to_limbs_kernel(const AffPt<NQ>* __restrict__ in, uint64_t n,
                                                             BaseRec<NQ>* __restrict__ out,
                                                             const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const AffPt<NQ> a = load16(in + i);
    const FL<NL, B> fix = fl_load_const<NL, B>(P.r2fix);
    AffL<NL, B> o;
    o.x = fl_canon_lt2p(fl_mul(fl_from_sat<NL, B, NQ>(a.x), fix, P), P);
    o.y = fl_canon_lt2p(fl_mul(fl_from_sat<NL, B, NQ>(a.y), fix, P), P);
    store_base<NQ>(out + i, o);
}

template <int NQ>
__device__ __forceinline__ void store_std(XyzzPt<NQ>* dst, const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>& acc,
                                          const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>& P) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    // back to the canonical R = 2^(32N) Montgomery form the rest of the pipeline (and the reference) uses
    const FL<NL, B> rs = fl_load_const<NL, B>(P.r_std);
    XyzzPt<NQ> o;
    o.x = fl_to_sat<NL, B, NQ>(fl_canon_lt2p(fl_mul(acc.x, rs, P), P));
    o.y = fl_to_sat<NL, B, NQ>(fl_canon_lt2p(fl_mul(acc.y, rs, P), P));
    o.zz = fl_to_sat<NL, B, NQ>(fl_canon_lt2p(fl_mul(acc.zz, rs, P), P));
    o.zzz = fl_to_sat<NL, B, NQ>(fl_canon_lt2p(fl_mul(acc.zzz, rs, P), P));
    store16(dst, o);
}

#define HEAVY_BUCKET 2048u      // entries above which a bucket is shared by HEAVY_SEGS workgroups
#define HEAVY_SEGS 8
// Hot kernel: lane i owns bucket order[i] (size-sorted).  Exceptional additions (same x) abort the
// bucket, which is queued for msm_accumulate_redo_kernel — keeps calls, scratch and the doubling
// formula out of this kernel.
template <int NQ, bool FUSED_Y3>
__global__ void __launch_bounds__(256) msm_accumulate_kernel(const BaseRec<NQ>* __restrict__ bases,
                                                             const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                                             const uint32_t* __restrict__ order, uint64_t nbuckets, SetGeom geom,
                                                             uint32_t heavy_thresh, XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ buckets, uint32_t* __restrict__ redo_count,
                                                             uint32_t* __restrict__ redo_list, uint32_t* __restrict__ heavy_count,
                                                             uint32_t* __restrict__ heavy_list, uint32_t* __restrict__ work,
                                                             const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    // work == nullptr: one lane per bucket, grid = nbuckets / 256.  work != nullptr: PERSISTENT waves — the grid is a fixed number of workgroups
    // (msm_acc_persist per CU, default 4 = every wave slot the registers allow) and every wave takes the next 64 buckets of the size-ordered
    // list from a global counter until the list is exhausted: no rounds of workgroups, so the 2^14 thousand-entry buckets of a c = 20 top window
    // (the launch's 13 ms critical path, started first) never hold a half-empty round open behind them, and the tail is one 64-bucket group per
    // wave: 16.6 -> 16.1 ms alone at 2^24, commitments -1.4 ... -2.4 % per step (profiles/r03_commit_overlap_experiment.txt).
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (;;) {
        if (work) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(work, 64u);
            base = (uint32_t)__shfl((int)base, 0);
            if (base >= nbuckets) break;
            i = (uint64_t)base + lane;
        }
        if (i < nbuckets) {
            const uint32_t b = order[i];
            const uint32_t total = bucket_entries(offsets, b, geom);
            if (total > heavy_thresh) {   // skewed scalars / a nearly empty top window: one lane must not walk it alone
                heavy_list[atomicAdd(heavy_count, 1u)] = b;
            } else {
                // ONE loop over the bucket's entries, across its segments (one per table plane; plain mode: a single segment).  A loop per segment
                // would run every segment as long as the wave's LONGEST one: the lanes of a wave are matched by total size, not per segment —
                // measured +38 % (2^24 points) to +80 % (2^22) on the merged accumulation, which rounds 1-2 mistook for a gather penalty.
                uint32_t w;
                uint64_t seg = seg_first(geom, b, &w);
                const uint64_t step = seg_step(geom);
                uint32_t j = offsets[seg], end = offsets[seg + 1];
                const BaseRec<NQ>* tb = bases;                               // plane t: 2^(c*G*t) * P_i
                XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
                bool ok = true;
                for (uint32_t it = 0; it < total; it++) {
                    while (j == end) { seg += step; tb += geom.tab_stride; j = offsets[seg]; end = offsets[seg + 1]; }   // `total` guarantees a next entry
                    const uint32_t e = sorted[j++];
                    AffL<NL, B> q = load_base<NQ>(tb + (e & 0x7fffffffu));
                    if (affl_is_inf(q)) continue;
                    if (e >> 31) q = affl_neg(q, P);
                    if (!xyzzl_madd_fast<NL, B, FUSED_Y3>(acc, q, P)) { ok = false; break; }
                }
                if (ok) store8(buckets + b, acc);
                else redo_list[atomicAdd(redo_count, 1u)] = b;
            }
        }
        if (!work) break;
    }
}

// Heavy buckets: HEAVY_SEGS workgroups share one bucket (strided slices), every lane accumulates a strided subset
// with the complete addition, an LDS tree folds the workgroup, msm_heavy_finish_kernel folds the segments.
template <int NQ>
__global__ void __launch_bounds__(256) msm_heavy_kernel(const BaseRec<NQ>* __restrict__ bases,
                                                        const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                                        SetGeom geom,
                                                        const uint32_t* __restrict__ heavy_count, const uint32_t* __restrict__ heavy_list,
                                                        XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ partial,
                                                        const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XyzzL<NL, B>* sh = reinterpret_cast<XyzzL<NL, B>*>(smem_raw);
    const uint32_t total = *heavy_count, seg = blockIdx.y;
    for (uint32_t h = blockIdx.x; h < total; h += gridDim.x) {
        const uint32_t b = heavy_list[h];
        XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
        uint32_t w;
        uint64_t sg = seg_first(geom, b, &w);
        const BaseRec<NQ>* tb = bases;
        for (; w < geom.W1; w += geom.G, sg += seg_step(geom), tb += geom.tab_stride) {
            const uint32_t beg = offsets[sg], end = offsets[sg + 1];
            for (uint32_t j = beg + seg * blockDim.x + threadIdx.x; j < end; j += HEAVY_SEGS * blockDim.x) {
                const uint32_t e = sorted[j];
                AffL<NL, B> q = load_base<NQ>(tb + (e & 0x7fffffffu));
                if (affl_is_inf(q)) continue;            // before negating: affl_neg would turn (0,0) into (0, 2p)
                if (e >> 31) q = affl_neg(q, P);
                acc = xyzzl_madd(acc, q, P);
            }
        }
        __syncthreads();
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int d = blockDim.x / 2; d > 0; d >>= 1) {
            if ((int)threadIdx.x < d) {
                const XyzzL<NL, B> a = sh[threadIdx.x], b2 = sh[threadIdx.x + d];
                sh[threadIdx.x] = xyzzl_add(a, b2, P);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) store8(partial + (uint64_t)h * HEAVY_SEGS + seg, sh[0]);
    }
}

template <int NQ>
__global__ void __launch_bounds__(64) msm_heavy_finish_kernel(const uint32_t* __restrict__ heavy_count, const uint32_t* __restrict__ heavy_list,
                                                              const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ partial,
                                                              XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ buckets,
                                                              const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint32_t total = *heavy_count;
    for (uint32_t h = blockIdx.x * blockDim.x + threadIdx.x; h < total; h += gridDim.x * blockDim.x) {
        XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
        for (int s = 0; s < HEAVY_SEGS; s++) acc = xyzzl_add(acc, load8(partial + (uint64_t)h * HEAVY_SEGS + s), P);
        store8(buckets + heavy_list[h], acc);
    }
}

template <int NQ>
__global__ void __launch_bounds__(64) msm_accumulate_redo_kernel(const BaseRec<NQ>* __restrict__ bases,
                                                                 const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ offsets,
                                                                 SetGeom geom,
                                                                 XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ buckets, const uint32_t* __restrict__ redo_count,
                                                                 const uint32_t* __restrict__ redo_list,
                                                                 const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint32_t total = *redo_count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t b = redo_list[i];
        XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
        uint32_t w;
        uint64_t sg = seg_first(geom, b, &w);
        const BaseRec<NQ>* tb = bases;
        for (; w < geom.W1; w += geom.G, sg += seg_step(geom), tb += geom.tab_stride) {
            const uint32_t beg = offsets[sg], end = offsets[sg + 1];
            for (uint32_t j = beg; j < end; j++) {
                const uint32_t e = sorted[j];
                AffL<NL, B> q = load_base<NQ>(tb + (e & 0x7fffffffu));
                if (affl_is_inf(q)) continue;
                if (e >> 31) q = affl_neg(q, P);
                acc = xyzzl_madd(acc, q, P);
            }
        }
        store8(buckets + b, acc);
    }
}

#ifndef REDUCE_LOGK
#define REDUCE_LOGK 2
#endif
#define REDUCE_K (1u << REDUCE_LOGK)
// ---------------------------------------------------------------------------------------------- 5: window reduction
// V_w = sum_j (j+1) * B_j over the 2^cb buckets of a window, as a short pyramid of running-sum passes:
//   level l holds n_l = 2^cb / K^l entries E_j with weights (j+1) (K = REDUCE_K = 4: the serial depth 2K*log_K(2^cb) is what
//   bounds this phase, not its work); one lane takes the STRIDED chunk {ch + t * nch_l : t < K_l} (nch_l = n_l / K_l chunks; K_l =
//   min(K, n_l)) and emits  acc = sum_t t * E_(ch + t nch)  and  S_ch = sum_t E_(ch + t nch)  (2K point additions, no scalar
//   multiplications).  Since (j+1) = (ch+1) + t * nch_l:  sum_j (j+1) E_j = sum_ch (ch+1) S_ch + nch_l * sum_ch acc_ch — the S values
//   are the next level's entries with the same kind of weights.  With A_l = sum of level l's acc values and Sigma = the single entry
//   left at the top:  V_w = Sigma + sum_l nch_l * A_l  (host: Horner, log2 K_l doublings per level).  Strided rather than contiguous
//   chunks (round 3): consecutive lanes read consecutive 144-byte entries, a wave's working set per step is 9 KiB instead of 36 KiB.
// All in lazy limb arithmetic (ec_lazy.hpp); only the W*(L+1) results are converted to the standard form.
template <int NQ>
__global__ void __launch_bounds__(256) msm_reduce_level_kernel(const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ in, uint64_t n_in,
                                                               uint32_t K, uint64_t nch, uint64_t total,
                                                               XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_acc,
                                                               XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_s,
                                                               uint32_t* __restrict__ redo_count, uint32_t* __restrict__ redo_list,
                                                               const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= total) return;
    const uint64_t w = id / nch, ch = id % nch;
    const XyzzL<NL, B>* E = in + w * n_in + ch;           // STRIDED chunk: entries ch, ch + nch, ..., ch + (K-1)*nch
    XyzzL<NL, B> running = xyzzl_inf<NL, B>(), acc = xyzzl_inf<NL, B>();
    bool ok = true;
    for (uint32_t d = K; d-- > 0;) {
        if (!xyzzl_add_fast(acc, running, P)) { ok = false; break; }
        if (!xyzzl_add_fast(running, load8(E + (uint64_t)d * nch), P)) { ok = false; break; }
    }
    if (ok) {
        store8(out_acc + id, acc);
        store8(out_s + id, running);
    } else {
        redo_list[atomicAdd(redo_count, 1u)] = (uint32_t)id;      // same-x additions: redone by the complete kernel
    }
}

template <int NQ>
__global__ void __launch_bounds__(64) msm_reduce_level_redo_kernel(const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ in, uint64_t n_in,
                                                                   uint32_t K, uint64_t nch,
                                                                   XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_acc,
                                                                   XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_s,
                                                                   const uint32_t* __restrict__ redo_count, const uint32_t* __restrict__ redo_list,
                                                                   const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint32_t total = *redo_count;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint64_t id = redo_list[i];
        const uint64_t w = id / nch, ch = id % nch;
        const XyzzL<NL, B>* E = in + w * n_in + ch;
        XyzzL<NL, B> running = xyzzl_inf<NL, B>(), acc = xyzzl_inf<NL, B>();
        for (uint32_t d = K; d-- > 0;) {
            acc = xyzzl_add(acc, running, P);
            running = xyzzl_add(running, load8(E + (uint64_t)d * nch), P);
        }
        store8(out_acc + id, acc);
        store8(out_s + id, running);
    }
}

// block (l, w): sum of `count[l]` consecutive limb-form points starting at src[l] + w*count[l]  ->  standard form
struct SumJobs {
    const void* src[16];
    uint64_t count[16];
    uint64_t wstride[16];      // points between the inputs of consecutive windows (0: = count, the dense layout of the pyramid arrays)
};
// RAW: the block's sum stays in the limb form (input of a second, combining launch) instead of being converted to the standard form.
// Workgroup z of the `nsplit` = gridDim.z that share a block's sum takes every nsplit-th stride of it and writes partial z.  The host splits the sums
// of large pyramids (c = 20: 2^17 level-0 values per window) this way, RAW, and folds the partials with a second, unsplit launch (nsplit = 1) —
// one workgroup per (level, window) used to walk 512 points per lane: 6.6 of the 9 ms a c = 20 reduction took.
template <int NQ, bool RAW = false>
__global__ void __launch_bounds__(256) msm_points_sum_kernel(SumJobs jobs, XyzzPt<NQ>* __restrict__ out, uint32_t nlevels, uint32_t nsplit,
                                                             const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P,
                                                             XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_raw = nullptr) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XyzzL<NL, B>* sh = reinterpret_cast<XyzzL<NL, B>*>(smem_raw);
    const uint32_t l = blockIdx.x, w = blockIdx.y, z = blockIdx.z;
    const uint64_t cnt = jobs.count[l];
    const XyzzL<NL, B>* src = reinterpret_cast<const XyzzL<NL, B>*>(jobs.src[l]) + (uint64_t)w * (jobs.wstride[l] ? jobs.wstride[l] : cnt);
    XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
    for (uint64_t i = (uint64_t)z * blockDim.x + threadIdx.x; i < cnt; i += (uint64_t)nsplit * blockDim.x) acc = xyzzl_add(acc, load8(src + i), P);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int d = blockDim.x / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const XyzzL<NL, B> a = sh[threadIdx.x], b2 = sh[threadIdx.x + d];
            sh[threadIdx.x] = xyzzl_add(a, b2, P);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (RAW) store8(out_raw + ((uint64_t)w * nlevels + l) * nsplit + z, sh[0]);
        else store_std<NQ>(out + ((uint64_t)w * nlevels + l) * nsplit + z, sh[0], P);
    }
}

// ---------------------------------------------------------------------------------------------- 5b: window reduction as a grid
// "msm_reduce_grid" (off by default: measured, lost to the pyramid, kept as an option — DESIGN.md §0 item 5):
// V_w = sum_j (j+1) B_j with the bucket index split as j = hi * L + lo (L = 2^ceil(cb/2) columns, H = 2^cb / L rows):
//     V_w = sum_lo (lo+1) R_lo + L * sum_hi hi * C_hi,      R_lo = sum_hi B[hi][lo] (column sums),  C_hi = sum_lo B[hi][lo] (row sums),
// and a weighted sum of <= 1024 points is taken bit by bit: sum_i k_i X_i = sum_b 2^b * (sum of the X_i whose weight k_i has bit b) — the
// host's Horner supplies the 2^b.  Same two additions per bucket as the pyramid, but every sum is a TREE: the serial depth of a window's
// reduction is T + log2(SEG) additions for the row / column sums (one launch, both kinds side by side) plus <= 2 + 8 for the bit sums,
// against 5 additions for each of the pyramid's (c-1)/2 dependent launches and a 16-deep per-level sum.  What it targets is the latency-
// bound reduction of SMALL problems (2^20 points: 8 + 2 launches, 1.7 ms beside 2.4 ms of accumulation); at 2^24 points the work is the same.
//
// One workgroup of 256 lanes = CW outputs x SEG interleaved segments; a lane adds T = Y / SEG inputs, then the SEG partial sums of an
// output meet in an LDS tree.  kind 0 (blockIdx.x < colblocks): column sums — lane (seg, cx), consecutive lanes read consecutive columns
// of one row; kind 1: row sums — lane (cx, seg), consecutive lanes read consecutive entries of one row.
template <int NQ>
__global__ void __launch_bounds__(256) msm_grid_sums_kernel(const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ in, uint32_t logL, uint32_t logH,
                                                            uint32_t log_segc, uint32_t log_segr, uint32_t colblocks,
                                                            XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_r,
                                                            XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ out_c,
                                                            const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XyzzL<NL, B>* sh = reinterpret_cast<XyzzL<NL, B>*>(smem_raw);
    const uint32_t tid = threadIdx.x, w = blockIdx.y;
    const bool col = blockIdx.x < colblocks;
    const uint32_t blk = col ? blockIdx.x : blockIdx.x - colblocks;
    const uint32_t log_seg = col ? log_segc : log_segr;
    const uint32_t SEG = 1u << log_seg, CW = 256u >> log_seg;
    const uint32_t seg = col ? tid / CW : tid & (SEG - 1);
    const uint32_t cx = col ? tid % CW : tid >> log_seg;
    const uint32_t X = 1u << (col ? logL : logH), Y = 1u << (col ? logH : logL);
    const uint32_t x = blk * CW + cx;
    const XyzzL<NL, B>* E = in + ((uint64_t)w << (logL + logH));
    XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
    if (x < X) {
        for (uint32_t y = seg; y < Y; y += SEG) {
            const uint64_t j = col ? ((uint64_t)y << logL) + x : ((uint64_t)x << logL) + y;
            acc = xyzzl_add(acc, load8(E + j), P);
        }
    }
    sh[tid] = acc;
    __syncthreads();
    const uint32_t stride = col ? CW : 1u;
    for (uint32_t d = SEG >> 1; d > 0; d >>= 1) {
        if (seg < d) {
            const XyzzL<NL, B> a = sh[tid], b2 = sh[tid + d * stride];
            sh[tid] = xyzzl_add(a, b2, P);
        }
        __syncthreads();
    }
    if (seg == 0 && x < X) store8((col ? out_r : out_c) + (uint64_t)w * X + x, sh[tid]);
}

// block (b, w): b <= logL: the column sums R_lo whose weight (lo + 1) has bit b;  b > logL: the row sums C_hi whose weight hi has bit b - logL - 1.
// The indices with the bit set are enumerated (no lane walks an entry it skips); standard-form result at out[w * nbits + b].
template <int NQ>
__global__ void __launch_bounds__(256) msm_bit_sums_kernel(const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ r_sums,
                                                           const XyzzL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B>* __restrict__ c_sums, uint32_t logL, uint32_t logH,
                                                           XyzzPt<NQ>* __restrict__ out, const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P) {
    MSM_SIDE_PRIO_ENTER();
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    XyzzL<NL, B>* sh = reinterpret_cast<XyzzL<NL, B>*>(smem_raw);
    const uint32_t b = blockIdx.x, w = blockIdx.y, nbits = logL + 1 + logH;
    const bool cols = b <= logL;
    const uint32_t bit = cols ? b : b - logL - 1;
    const uint32_t n = 1u << (cols ? logL : logH), add = cols ? 1u : 0u;
    const XyzzL<NL, B>* src = (cols ? r_sums : c_sums) + (uint64_t)w * n;
    XyzzL<NL, B> acc = xyzzl_inf<NL, B>();
    const uint32_t half = n > 1 ? n >> 1 : 1;
    for (uint32_t u = threadIdx.x; u < half; u += blockDim.x) {
        const uint32_t k = ((u >> bit) << (bit + 1)) | (1u << bit) | (u & ((1u << bit) - 1));      // u-th weight with bit `bit` set
        if (k >= add && k - add < n) acc = xyzzl_add(acc, load8(src + (k - add)), P);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int d = blockDim.x / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const XyzzL<NL, B> a = sh[threadIdx.x], b2 = sh[threadIdx.x + d];
            sh[threadIdx.x] = xyzzl_add(a, b2, P);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) store_std<NQ>(out + (uint64_t)w * nbits + b, sh[0], P);
}

// ---------------------------------------------------------------------------------------------- ark layout -> compact
// arkworks GroupAffine { x, y, infinity: bool } padded to 8 bytes: stride 16*Q64 + 8 bytes.
template <int NQ>
__global__ void __launch_bounds__(256) bases_convert_kernel(const uint32_t* __restrict__ raw, uint64_t n, AffPt<NQ>* __restrict__ out,
                                                            unsigned long long* __restrict__ bad /* [0]: first offending index, [1]: reasons */) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t* s = raw + i * (2 * NQ + 2);
    AffPt<NQ> p;
    const bool inf = (s[2 * NQ] & 0xff) != 0;
    if (bad != nullptr && (s[2 * NQ] & 0xff) > 1) {            // `infinity: bool` is 0 or 1 in Rust: anything else is not a GroupAffine at this stride
        atomicMin(bad, (unsigned long long)i);
        atomicOr(bad + 1, (unsigned long long)BASES_BAD_FLAG);
    }
#pragma unroll
    for (int k = 0; k < NQ; k++) { p.x.l[k] = inf ? 0 : s[k]; p.y.l[k] = inf ? 0 : s[NQ + k]; }
    store16(out + i, p);
}

// ---------------------------------------------------------------------------------------------- the SRS, checked at the boundary
// Every base must be a point of the curve: coordinates reduced, y^2 = x^3 + b, or the (0, 0) this library reads as infinity.  The Rust
// side hands over `[G1Affine]` by reinterpreting memory (utils.rs:27-43, worker.rs:136-141) and `GroupAffine {x, y, infinity}` has no
// guaranteed field order: swapped coordinates, a shifted stride or a different padding would otherwise give commitments that are
// garbage with PLONK_OK.  One lane per point, 3 saturated Montgomery products: ~1 ms at 2^24 points, once per init.
template <int NQ>
__global__ void __launch_bounds__(256) bases_check_kernel(const AffPt<NQ>* __restrict__ pts, uint64_t n, const FpParams<NQ> P, const Fp<NQ> b_mont,
                                                          unsigned long long* __restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const AffPt<NQ> a = load16(pts + i);
    if (aff_is_inf(a)) return;
    uint32_t why = 0;
    bool xr = false, yr = false;                               // < p ?
    for (int k = NQ - 1; k >= 0; k--) { if (a.x.l[k] != P.p[k]) { xr = a.x.l[k] < P.p[k]; break; } }
    for (int k = NQ - 1; k >= 0; k--) { if (a.y.l[k] != P.p[k]) { yr = a.y.l[k] < P.p[k]; break; } }
    if (!xr || !yr) why = BASES_BAD_RANGE;
    else if (!fp_eq(fp_sqr(a.y, P), fp_add(fp_mul(fp_sqr(a.x, P), a.x, P), b_mont, P))) why = BASES_BAD_CURVE;
    if (why) {
        atomicMin(bad, (unsigned long long)i);
        atomicOr(bad + 1, (unsigned long long)why);
    }
}

// ---------------------------------------------------------------------------------------------- fixed-base window table
// The SRS is fixed between `init` calls (worker.rs:141), so shifted copies of it can be built once and kept resident: plane t holds
// 2^(c*G*t) * P_i (T planes x 64 / 96 B per point; 288 GB of HBM make this cheap).  Window w = g + t*G of a scalar then reads its bases from
// plane t and adds into the bucket set of window g: a scalar vector needs G bucket sets instead of W — the reduction pyramid, the
// bucket ordering and the host fold shrink W/G-fold (G = 1: one set for all windows), and with fewer, fuller buckets a wider window pays.
// Lane i walks its point through the T-1 shifts: c*G doublings (lazy XYZZ), one Fermat inversion, back to the canonical affine limb form
// the accumulate kernel reads.
// HISTORY: rounds 1-2 measured the merged accumulation 34 % slower per addition (23.8 vs 17.8 ms) and blamed the gathers from a 15.7 GB
// table.  Round 3 found the cause elsewhere (profiles/r03_msm_table_experiment.txt): the kernel ran one loop PER SEGMENT, and a wave's lanes
// are matched by their buckets' TOTAL size, so every segment ran as long as the wave's longest — +80 % at 2^22 points (3.9 GB table), +38 % at 2^24.
// The accumulate kernel now runs one loop over all entries of a bucket, and bases gathered from 4.8 GB (2^26 points) cost what 1.2 GB costs.
// What is left (+8 % per addition at 4 planes, +15 % at 13: the segment boundaries inside the loop) cancels what the smaller pyramid saves: OFF by
// default (`msm_precompute` = 0), kept as an option with its tests (tests/test_gpu_msm_table.py).
template <int NQ>
__global__ void __launch_bounds__(64) msm_table_kernel(BaseRec<NQ>* __restrict__ table, uint64_t n, uint64_t stride, int shift, int T,
                                                       const FLParams<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> P,
                                                       const FL<LimbGeom<NQ>::NL, LimbGeom<NQ>::B> pm2 /* p - 2, limb form */) {
    constexpr int NL = LimbGeom<NQ>::NL, B = LimbGeom<NQ>::B;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    AffL<NL, B> q = load_base<NQ>(table + i);
    for (int w = 1; w < T; w++) {
        if (!affl_is_inf(q)) {
            XyzzL<NL, B> a = xyzzl_dbl_affine(q, P);
            for (int k = 1; k < shift; k++) a = xyzzl_dbl(a, P);
            // 1 / ZZZ by Fermat; 1/Z = ZZ / ZZZ; x = X / Z^2, y = Y / ZZZ   (an infinity gives 0 -> (0, 0) = infinity)
            FL<NL, B> inv = fl_load_const<NL, B>(P.one);
            for (int bit = NL * B - 1; bit >= 0; bit--) {
                inv = fl_sqr(inv, P);
                if ((pm2.l[bit / B] >> (bit % B)) & 1) inv = fl_mul(inv, a.zzz, P);
            }
            const FL<NL, B> u = fl_mul(a.zz, inv, P);
            q.x = fl_canon_lt2p(fl_mul(a.x, fl_sqr(u, P), P), P);
            q.y = fl_canon_lt2p(fl_mul(a.y, inv, P), P);
        }
        store_base<NQ>(table + (uint64_t)w * stride + i, q);
    }
}
