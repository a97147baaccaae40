// circuit_kernels.hpp — preprocessing of a user circuit given in jellyfish's arithmetised form (included by synth.hip):
//   * the copy-constraint permutation from the gate wiring (compute_wire_permutation): a stable LSD radix sort of the
//     (variable, position) pairs, a linking pass and the id_perm / sigma writer;
//   * witness placement wires[p] = witness[wire_vars[p]];
//   * the satisfiability check (check_circuit_satisfiability): first failing gate, first broken copy constraint.
// Every output is a pure function of the input: no scatter lets atomic arrival order decide a value (the only atomics are LDS
// histogram counts and one atomicMin per workgroup for error reports).  Device intrinsics are limited to block barriers and
// atomics so that tests/hostemu runs the same code on the CPU.
#pragma once
#include "plonk_internal.hpp"

constexpr uint32_t CIRC_THREADS = 256;
constexpr uint32_t CIRC_ITEMS = 8;                        // elements per thread of a sort tile
constexpr uint32_t CIRC_TILE = CIRC_THREADS * CIRC_ITEMS;           // 2048 elements: 11 bits of in-tile index
constexpr uint32_t CIRC_TILE_BITS = 11;
constexpr uint32_t CIRC_DIGITS = 256;                     // 8-bit radix digits
constexpr uint32_t CIRC_ID_CHUNK = 16;                    // gates per thread of the id_perm writer (one power of w, then a running product)
constexpr unsigned long long CIRC_NONE = ~0ull;

static_assert(CIRC_TILE == 1u << CIRC_TILE_BITS, "tile index bits");

// min over the workgroup (blockDim.x == CIRC_THREADS); red: CIRC_THREADS words of LDS.  Every thread gets the result.
__device__ __forceinline__ unsigned long long circ_block_min(unsigned long long v, unsigned long long* red) {
    const uint32_t t = threadIdx.x;
    red[t] = v;
    __syncthreads();
    for (uint32_t s = CIRC_THREADS / 2; s > 0; s >>= 1) {
        if (t < s && red[t + s] < red[t]) red[t] = red[t + s];
        __syncthreads();
    }
    const unsigned long long r = red[0];
    __syncthreads();
    return r;
}

// exclusive prefix sum over the workgroup (blockDim.x == CIRC_THREADS); buf: CIRC_THREADS words of LDS.  Returns this thread's prefix;
// *total receives the sum of all.
__device__ __forceinline__ uint32_t circ_block_exclusive_scan(uint32_t v, uint32_t* buf, uint32_t* total) {
    const uint32_t t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (uint32_t s = 1; s < CIRC_THREADS; s <<= 1) {
        const uint32_t add = t >= s ? buf[t - s] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const uint32_t incl = buf[t];
    *total = buf[CIRC_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// ---------------------------------------------------------------------------------------------- validation
// first_bad = min(first_bad, the smallest index p < count with ids[p] >= limit); one atomic per workgroup that found one
__global__ void __launch_bounds__(CIRC_THREADS) circuit_ids_check_kernel(const uint32_t* __restrict__ ids, uint64_t count, uint64_t limit,
                                                                    unsigned long long* __restrict__ first_bad) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad = CIRC_NONE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t p = base + k * CIRC_THREADS + threadIdx.x;
        if (p < count && ids[p] >= limit && p < bad) bad = p;
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first_bad, bad);
}

// ---------------------------------------------------------------------------------------------- stable LSD radix sort
// hist[d * tiles + tile] = how many keys of the tile have digit d (digit-major: an exclusive scan of the flat array gives every
// (digit, tile) its first output slot, tiles of one digit in order — which is what makes the scatter stable)
__global__ void __launch_bounds__(CIRC_THREADS) circuit_radix_hist_kernel(const uint32_t* __restrict__ keys, uint64_t count, uint32_t shift, uint32_t tiles,
                                                                     uint32_t* __restrict__ hist) {
    __shared__ uint32_t cnt[CIRC_DIGITS];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t p = base + k * CIRC_THREADS + threadIdx.x;
        if (p < count) atomicAdd(&cnt[(keys[p] >> shift) & (CIRC_DIGITS - 1)], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of a[0 .. len) in three launches: per-block sums, a one-workgroup scan of the sums, per-block rescan + offset
__global__ void __launch_bounds__(CIRC_THREADS) circuit_scan_reduce_kernel(const uint32_t* __restrict__ a, uint64_t len, uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE + (uint64_t)threadIdx.x * CIRC_ITEMS;
    uint32_t s = 0;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++)
        if (base + k < len) s += a[base + k];
    uint32_t total;
    (void)circ_block_exclusive_scan(s, buf, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ void __launch_bounds__(CIRC_THREADS) circuit_scan_sums_kernel(uint32_t* __restrict__ sums, uint32_t nb) {
    __shared__ uint32_t buf[CIRC_THREADS];
    const uint32_t per = (nb + CIRC_THREADS - 1) / CIRC_THREADS;
    const uint32_t lo = threadIdx.x * per;
    uint32_t s = 0;
    for (uint32_t i = lo; i < lo + per && i < nb; i++) s += sums[i];
    uint32_t total;
    uint32_t run = circ_block_exclusive_scan(s, buf, &total);
    for (uint32_t i = lo; i < lo + per && i < nb; i++) {
        const uint32_t v = sums[i];
        sums[i] = run;
        run += v;
    }
}

__global__ void __launch_bounds__(CIRC_THREADS) circuit_scan_apply_kernel(uint32_t* __restrict__ a, uint64_t len, const uint32_t* __restrict__ sums) {
    __shared__ uint32_t buf[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE + (uint64_t)threadIdx.x * CIRC_ITEMS;
    uint32_t v[CIRC_ITEMS], s = 0;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        v[k] = base + k < len ? a[base + k] : 0;
        s += v[k];
    }
    uint32_t total;
    uint32_t run = circ_block_exclusive_scan(s, buf, &total) + sums[blockIdx.x];
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        if (base + k < len) a[base + k] = run;
        run += v[k];
    }
}

// One pass: the tile's (digit << 11 | in-tile index) words are sorted in LDS (bitonic; the index makes every word distinct, so the
// order among equal digits is the input order), and element s of the sorted tile goes to offs[digit][tile] + (s - first s of its digit).
// vin == nullptr: the payload is the element's own position (first pass).
__global__ void __launch_bounds__(CIRC_THREADS) circuit_radix_scatter_kernel(const uint32_t* __restrict__ kin, const uint32_t* __restrict__ vin, uint64_t count,
                                                                        uint32_t shift, uint32_t tiles, const uint32_t* __restrict__ offs,
                                                                        uint32_t* __restrict__ kout, uint32_t* __restrict__ vout) {
    __shared__ uint32_t skey[CIRC_TILE];
    __shared__ uint32_t sval[CIRC_TILE];
    __shared__ uint32_t word[CIRC_TILE];
    __shared__ uint32_t first[CIRC_DIGITS];
    const uint32_t t = threadIdx.x;
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint32_t li = k * CIRC_THREADS + t;
        const uint64_t p = base + li;
        if (p < count) {
            const uint32_t key = kin[p];
            skey[li] = key;
            sval[li] = vin ? vin[p] : (uint32_t)p;
            word[li] = (((key >> shift) & (CIRC_DIGITS - 1)) << CIRC_TILE_BITS) | li;
        } else {
            word[li] = 0xFFFFFFFFu;                      // sorts last, never written out
        }
    }
    __syncthreads();
    for (uint32_t size = 2; size <= CIRC_TILE; size <<= 1) {
        for (uint32_t j = size >> 1; j > 0; j >>= 1) {
            for (uint32_t k = 0; k < CIRC_TILE / 2 / CIRC_THREADS; k++) {
                const uint32_t q = k * CIRC_THREADS + t;               // pair index
                const uint32_t i = 2 * q - (q & (j - 1));         // lower element of the pair
                const uint32_t a = word[i], b = word[i + j];
                const bool up = (i & size) == 0;
                if ((a > b) == up) { word[i] = b; word[i + j] = a; }
            }
            __syncthreads();
        }
    }
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint32_t s = k * CIRC_THREADS + t;
        const uint32_t w = word[s];
        if (w != 0xFFFFFFFFu && (s == 0 || (word[s - 1] >> CIRC_TILE_BITS) != (w >> CIRC_TILE_BITS))) first[w >> CIRC_TILE_BITS] = s;
    }
    __syncthreads();
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint32_t s = k * CIRC_THREADS + t;
        const uint32_t w = word[s];
        if (w == 0xFFFFFFFFu) continue;
        const uint32_t d = w >> CIRC_TILE_BITS, li = w & (CIRC_TILE - 1);
        const uint32_t dst = offs[(uint64_t)d * tiles + blockIdx.x] + (s - first[d]);
        kout[dst] = skey[li];
        vout[dst] = sval[li];
    }
}

// ---------------------------------------------------------------------------------------------- cycles
// sk / sv: the sorted variables and their positions.  A segment head records start[var]; every element links to its successor in
// sorted order, the segment's last element back to start[var].
__global__ void __launch_bounds__(CIRC_THREADS) circuit_link_heads_kernel(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint64_t count,
                                                                     uint32_t* __restrict__ start) {
    const uint64_t s = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (s >= count) return;
    const uint32_t v = sk[s];
    if (s == 0 || sk[s - 1] != v) start[v] = sv[s];
}

__global__ void __launch_bounds__(CIRC_THREADS) circuit_link_kernel(const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint64_t count,
                                                               const uint32_t* __restrict__ start, uint64_t* __restrict__ perm_idx) {
    const uint64_t s = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (s >= count) return;
    const uint32_t v = sk[s];
    const uint32_t nxt = (s + 1 < count && sk[s + 1] == v) ? sv[s + 1] : start[v];
    perm_idx[sv[s]] = nxt;
}

// id_perm[i*n + j] = k_i * w^j: thread t of block b owns gates j0 + r*CIRC_THREADS (j0 = b*CIRC_THREADS*CIRC_ID_CHUNK + t, r < CIRC_ID_CHUNK), one power
// w^j0 and a running product by w^CIRC_THREADS
struct CircIdPermParams {
    Fr k[5];
    Fr omega, omega_step;
};
__global__ void __launch_bounds__(CIRC_THREADS) circuit_id_perm_kernel(const CircIdPermParams c, uint64_t n, Fr* __restrict__ id_perm, const FrParams P) {
    uint64_t j = (uint64_t)blockIdx.x * CIRC_THREADS * CIRC_ID_CHUNK + threadIdx.x;
    if (j >= n) return;
    Fr w = fp_pow_u64(c.omega, j, P);
    for (uint32_t r = 0; r < CIRC_ID_CHUNK && j < n; r++, j += CIRC_THREADS) {
#pragma unroll
        for (int i = 0; i < 5; i++) id_perm[i * n + j] = fp_mul(c.k[i], w, P);
        w = fp_mul(w, c.omega_step, P);
    }
}

__global__ void __launch_bounds__(CIRC_THREADS) circuit_sigma_kernel(const Fr* __restrict__ id_perm, const uint64_t* __restrict__ perm_idx, uint64_t count,
                                                                Fr* __restrict__ sigma) {
    const uint64_t p = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (p >= count) return;
    sigma[p] = id_perm[perm_idx[p]];
}

// ---------------------------------------------------------------------------------------------- witness, check
__global__ void __launch_bounds__(CIRC_THREADS) circuit_witness_kernel(const uint32_t* __restrict__ ids, uint64_t count, const Fr* __restrict__ witness,
                                                                  uint64_t num_vars, Fr* __restrict__ wires, unsigned long long* __restrict__ first_bad) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad = CIRC_NONE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t p = base + k * CIRC_THREADS + threadIdx.x;
        if (p >= count) break;
        const uint32_t v = ids[p];
        if (v < num_vars) wires[p] = witness[v];
        else if (p < bad) bad = p;
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first_bad, bad);
}

// The part of gate j's equation that does not read wire 4: q_c + PI + sum q_lc*w + q_mul0*ab + q_mul1*cd + sum q_hash*w^5 of the four
// input values.  *abcd (if asked for) receives ab*cd, the factor of the q_ecc term.  The witness solver (solve_kernels.hpp) divides
// this by q_o; the check below completes it.
__device__ __forceinline__ Fr circ_gate_inputs_value(const Fr& a, const Fr& b, const Fr& c, const Fr& d, const Fr* __restrict__ sel,
                                                const Fr* __restrict__ pub, uint64_t n, uint64_t j, const FrParams& P, Fr* abcd) {
    const Fr ab = fp_mul(a, b, P), cd = fp_mul(c, d, P);
    if (abcd) *abcd = fp_mul(ab, cd, P);
    Fr acc = fp_add(sel[11 * n + j], pub[j], P);                                              // q_c + PI
    acc = fp_add(acc, fp_mul(sel[4 * n + j], ab, P), P);                                      // q_mul
    acc = fp_add(acc, fp_mul(sel[5 * n + j], cd, P), P);
    const auto lin_hash = [&](int t, const Fr& w) {                                          // q_lc * w + q_hash * w^5
        const Fr w2 = fp_sqr(w, P);
        acc = fp_add(acc, fp_mul(sel[t * n + j], w, P), P);
        acc = fp_add(acc, fp_mul(sel[(6 + t) * n + j], fp_mul(fp_sqr(w2, P), w, P), P), P);
    };
    lin_hash(0, a);                                  // written out: a loop over an array of the wires keeps that array in scratch
    lin_hash(1, b);
    lin_hash(2, c);
    lin_hash(3, d);
    return acc;
}

// q_c + PI + sum q_lc*w + q_mul0*ab + q_mul1*cd + sum q_hash*w^5 + q_ecc*abcde - q_o*e at gate j (the quotient kernel's gate term)
__device__ __forceinline__ Fr circ_gate_value(const Fr* __restrict__ wires, const Fr* __restrict__ sel, const Fr* __restrict__ pub, uint64_t n, uint64_t j,
                                         const FrParams& P) {
    const Fr a = wires[j], b = wires[n + j], c = wires[2 * n + j], d = wires[3 * n + j], e = wires[4 * n + j];
    Fr abcd;
    Fr acc = circ_gate_inputs_value(a, b, c, d, sel, pub, n, j, P, &abcd);
    acc = fp_add(acc, fp_mul(sel[12 * n + j], fp_mul(abcd, e, P), P), P);                     // q_ecc * abcde
    return fp_sub(acc, fp_mul(sel[10 * n + j], e, P), P);                                     // - q_o * e
}

// One lane per gate.  out[0]: first gate whose TurboPlonk equation fails; out[1]: first position p with wires[p] != wires[perm_idx[p]];
// out[2]: first position whose perm_idx is >= 5n (that entry is not followed).
__global__ void __launch_bounds__(CIRC_THREADS) circuit_check_kernel(const Fr* __restrict__ wires, const Fr* __restrict__ sel, const Fr* __restrict__ pub,
                                                                const uint64_t* __restrict__ perm_idx, uint64_t n, unsigned long long* __restrict__ out,
                                                                const FrParams P) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t j = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    unsigned long long bad_gate = CIRC_NONE, bad_copy = CIRC_NONE, bad_idx = CIRC_NONE;
    if (j < n) {
        if (!fp_is_zero(circ_gate_value(wires, sel, pub, n, j, P))) bad_gate = j;
        if (perm_idx) {
            for (int i = 0; i < 5; i++) {
                const uint64_t p = i * n + j, q = perm_idx[p];
                if (q >= 5 * n) { if (p < bad_idx) bad_idx = p; }
                else if (!fp_eq(wires[p], wires[q]) && p < bad_copy) bad_copy = p;
            }
        }
    }
    bad_gate = circ_block_min(bad_gate, red);
    bad_copy = circ_block_min(bad_copy, red);
    bad_idx = circ_block_min(bad_idx, red);
    if (threadIdx.x == 0) {
        if (bad_gate != CIRC_NONE) atomicMin(out, bad_gate);
        if (bad_copy != CIRC_NONE) atomicMin(out + 1, bad_copy);
        if (bad_idx != CIRC_NONE) atomicMin(out + 2, bad_idx);
    }
}

static inline uint32_t circ_grid_of(uint64_t count, uint64_t per_block) { return (uint32_t)((count + per_block - 1) / per_block); }

static inline int circ_launch_status(const char* who) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return plonk_fail(PLONK_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
    return PLONK_OK;
}

// the 8-bit passes that cover ids < num_vars (at least one)
static inline int circ_radix_passes(uint64_t num_vars) {
    int bits = 0;
    while (bits < 32 && (num_vars - 1) >> bits) bits++;
    return bits <= 8 ? 1 : (bits + 7) / 8;
}

// The stable sort of N (key, position) pairs in `passes` 8-bit passes.  *kin: the keys (not modified unless it is keys[1], which the second
// pass overwrites); *vin: their payloads, nullptr = each element's own position.  On return *kin / *vin address the sorted pairs, in
// keys[(passes - 1) & 1] / vals[(passes - 1) & 1].  hist: 256 * ceil(N / 2048) words, sums: one word per 2048 of those.
static inline int circ_radix_sort(const uint32_t** kin, const uint32_t** vin, uint64_t N, int passes, uint32_t* const keys[2], uint32_t* const vals[2],
                                  uint32_t* hist, uint32_t* sums, hipStream_t stream) {
    const uint32_t tiles = circ_grid_of(N, CIRC_TILE);
    const uint64_t hist_len = (uint64_t)CIRC_DIGITS * tiles;
    const uint32_t scan_blocks = circ_grid_of(hist_len, CIRC_TILE);
    int rc;
    for (int pass = 0; pass < passes; pass++) {
        const uint32_t shift = 8 * pass;
        uint32_t* ko = keys[pass & 1];
        uint32_t* vo = vals[pass & 1];
        hipLaunchKernelGGL(circuit_radix_hist_kernel, dim3(tiles), dim3(CIRC_THREADS), 0, stream, *kin, N, shift, tiles, hist);
        hipLaunchKernelGGL(circuit_scan_reduce_kernel, dim3(scan_blocks), dim3(CIRC_THREADS), 0, stream, (const uint32_t*)hist, hist_len, sums);
        hipLaunchKernelGGL(circuit_scan_sums_kernel, dim3(1), dim3(CIRC_THREADS), 0, stream, sums, scan_blocks);
        hipLaunchKernelGGL(circuit_scan_apply_kernel, dim3(scan_blocks), dim3(CIRC_THREADS), 0, stream, hist, hist_len, (const uint32_t*)sums);
        hipLaunchKernelGGL(circuit_radix_scatter_kernel, dim3(tiles), dim3(CIRC_THREADS), 0, stream, *kin, *vin, N, shift, tiles, (const uint32_t*)hist, ko, vo);
        if ((rc = circ_launch_status("circuit_radix_sort"))) return rc;
        *kin = ko;
        *vin = vo;
    }
    return PLONK_OK;
}

// scratch layout (bytes, each piece 256-aligned): flag | 4 sort arrays of 5n u32 | hist | block sums | start[num_vars]
struct CircPermScratch {
    size_t flag = 0, keys[2] = {0, 0}, vals[2] = {0, 0}, hist = 0, sums = 0, start = 0, total = 0;
    uint64_t count = 0, hist_len = 0;
    uint32_t tiles = 0, scan_blocks = 0;
    CircPermScratch(size_t n, size_t num_vars) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        count = 5 * (uint64_t)n;
        tiles = circ_grid_of(count, CIRC_TILE);
        hist_len = (uint64_t)CIRC_DIGITS * tiles;
        scan_blocks = circ_grid_of(hist_len, CIRC_TILE);
        size_t at = al(sizeof(unsigned long long));
        for (int b = 0; b < 2; b++) { keys[b] = at; at += al(count * 4); vals[b] = at; at += al(count * 4); }
        hist = at; at += al(hist_len * 4);
        sums = at; at += al((size_t)scan_blocks * 4);
        start = at; at += al(num_vars * 4);
        total = at;
    }
};

static inline int circ_read_flag(const unsigned long long* d_flag, unsigned long long* h, hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(h, d_flag, sizeof(*h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return PLONK_OK;
}

size_t circuit_permutation_scratch_bytes(size_t n, size_t num_vars) { return CircPermScratch(n, num_vars).total; }

int circuit_permutation_run(int curve, const uint32_t* wire_vars, size_t n, size_t num_vars, const uint64_t* k_mont, const Fr& omega_n,
                            Fr* id_perm, uint64_t* perm_idx, Fr* sigma, void* scratch, hipStream_t stream) {
    const CircPermScratch L(n, num_vars);
    char* base = (char*)scratch;
    unsigned long long* d_flag = (unsigned long long*)base;
    uint32_t* keys[2] = {(uint32_t*)(base + L.keys[0]), (uint32_t*)(base + L.keys[1])};
    uint32_t* vals[2] = {(uint32_t*)(base + L.vals[0]), (uint32_t*)(base + L.vals[1])};
    uint32_t* hist = (uint32_t*)(base + L.hist);
    uint32_t* sums = (uint32_t*)(base + L.sums);
    uint32_t* start = (uint32_t*)(base + L.start);
    const uint64_t N = L.count;
    int rc;
    {   // every id below num_vars before any id indexes anything
        HIP_TRY(hipMemsetAsync(d_flag, 0xFF, sizeof(*d_flag), stream));
        hipLaunchKernelGGL(circuit_ids_check_kernel, dim3(L.tiles), dim3(CIRC_THREADS), 0, stream, wire_vars, N, (uint64_t)num_vars, d_flag);
        if ((rc = circ_launch_status("circuit_ids_check"))) return rc;
        unsigned long long bad = CIRC_NONE;
        if ((rc = circ_read_flag(d_flag, &bad, stream))) return rc;
        if (bad != CIRC_NONE)
            return plonk_fail(PLONK_ERR_ARG, "plonk_circuit_permutation_dev: wire %llu of gate %llu reads a variable id >= num_vars = %zu",
                              bad / n, bad % n, num_vars);
    }
    {
        ProfScope ps("circuit_sort", stream);
        const uint32_t* kin = wire_vars;
        const uint32_t* vin = nullptr;
        if ((rc = circ_radix_sort(&kin, &vin, N, circ_radix_passes(num_vars), keys, vals, hist, sums, stream))) return rc;
        hipLaunchKernelGGL(circuit_link_heads_kernel, dim3(circ_grid_of(N, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, kin, vin, N, start);
        hipLaunchKernelGGL(circuit_link_kernel, dim3(circ_grid_of(N, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, kin, vin, N, (const uint32_t*)start, perm_idx);
        if ((rc = circ_launch_status("circuit_link"))) return rc;
    }
    {
        ProfScope ps("circuit_sigma", stream);
        const FrParams& P = fr_params(curve);
        CircIdPermParams c;
        for (int i = 0; i < 5; i++) c.k[i] = fp_from_limbs<8>((const uint32_t*)(k_mont + 4 * i));
        c.omega = omega_n;
        c.omega_step = fp_pow_u64(omega_n, CIRC_THREADS, P);
        hipLaunchKernelGGL(circuit_id_perm_kernel, dim3(circ_grid_of(n, (uint64_t)CIRC_THREADS * CIRC_ID_CHUNK)), dim3(CIRC_THREADS), 0, stream, c, (uint64_t)n, id_perm, P);
        hipLaunchKernelGGL(circuit_sigma_kernel, dim3(circ_grid_of(N, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, (const Fr*)id_perm, (const uint64_t*)perm_idx, N, sigma);
        if ((rc = circ_launch_status("circuit_sigma"))) return rc;
    }
    return PLONK_OK;
}

int circuit_witness_run(const uint32_t* wire_vars, size_t n, const Fr* witness, size_t num_vars, Fr* wires, void* scratch, hipStream_t stream) {
    unsigned long long* d_flag = (unsigned long long*)scratch;
    const uint64_t N = 5 * (uint64_t)n;
    int rc;
    {
        ProfScope ps("circuit_witness", stream);
        HIP_TRY(hipMemsetAsync(d_flag, 0xFF, sizeof(*d_flag), stream));
        hipLaunchKernelGGL(circuit_witness_kernel, dim3(circ_grid_of(N, CIRC_TILE)), dim3(CIRC_THREADS), 0, stream, wire_vars, N, witness, (uint64_t)num_vars, wires, d_flag);
        if ((rc = circ_launch_status("circuit_witness"))) return rc;
    }
    unsigned long long bad = CIRC_NONE;
    if ((rc = circ_read_flag(d_flag, &bad, stream))) return rc;
    if (bad != CIRC_NONE)
        return plonk_fail(PLONK_ERR_ARG, "plonk_circuit_witness_dev: wire %llu of gate %llu reads a variable id >= num_vars = %zu", bad / n, bad % n,
                          num_vars);
    return PLONK_OK;
}

int circuit_check_run(int curve, const Fr* wires, const Fr* sel, const Fr* pub, const uint64_t* perm_idx, size_t n, int64_t* first_bad_gate,
                      int64_t* first_bad_copy, void* scratch, hipStream_t stream) {
    unsigned long long* d_out = (unsigned long long*)scratch;
    unsigned long long h[3];
    int rc;
    {
        ProfScope ps("circuit_check", stream);
        HIP_TRY(hipMemsetAsync(d_out, 0xFF, sizeof(h), stream));
        hipLaunchKernelGGL(circuit_check_kernel, dim3(circ_grid_of(n, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, wires, sel, pub, perm_idx, (uint64_t)n, d_out,
                           fr_params(curve));
        if ((rc = circ_launch_status("circuit_check"))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(h, d_out, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h[2] != CIRC_NONE)
        return plonk_fail(PLONK_ERR_ARG, "plonk_circuit_check_dev: perm_idx[%llu] is >= 5n = %llu", h[2], 5ull * n);
    *first_bad_gate = h[0] == CIRC_NONE ? -1 : (int64_t)h[0];
    *first_bad_copy = h[1] == CIRC_NONE ? -1 : (int64_t)h[1];
    return PLONK_OK;
}
