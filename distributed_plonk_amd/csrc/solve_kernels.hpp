// solve_kernels.hpp — the witness of a user circuit solved on the device (included by synth.hip after circuit_kernels.hpp).  The
// counterpart of building a circuit with jellyfish's PlonkCircuit and reading its witness back (the reference's generate_circuit,
// dispatcher2.rs:1226-1271): every variable that a gate defines — def_gate[v] = g, v on wire 4 of g — is computed from the gate equation
//     witness[v] = (q_c + PI + sum q_lc*w + q_mul0*ab + q_mul1*cd + sum q_hash*w^5) / q_o        (circ_gate_inputs_value / q_o)
// level by level over the dependency graph:
//   * validation: every wire id < num_vars, and for every defined v: def_gate[v] < n, wire 4 of that gate reads v (so no two
//     variables can claim one gate), q_o != 0, q_ecc == 0 — before anything is indexed by an id;
//   * one lane per gate: which of wires 0-3 are live (q_lc, q_hash or the wire's q_mul non-zero), how many of the live ones read a
//     variable that is itself defined (the gate's pending count), and the sort keys: the variable for such a wire, a sentinel
//     (num_vars, sorts last) for every other position.  Gates with nothing pending form level 0;
//   * the stable radix sort of circuit_kernels.hpp over the 4n (key, position) pairs: the run of a variable is its consumer list;
//   * one launch per level: a lane per frontier gate evaluates and stores its variable, then walks the variable's consumers,
//     decrements their pending counts (atomicAdd of -1) and appends a gate whose count reaches zero to the next frontier.  The host
//     reads the next frontier's size between launches.  A value written in one launch is read only by later launches.
// Each defining gate is evaluated exactly once; the work is O(n) plus a launch and a 8-byte read per level.  Which lane appends first
// varies, the frontier's order with it — no output depends on that order: the witness, the number of levels and of evaluations, and
// the smallest unsolved variable (a dependency cycle; min-reduced as in the check kernel) are functions of the input alone.
//
// With a hint_op array (plonk_circuit_solve_hints_dev; solve_hints.hpp) a gate may instead define its variable by a HINT — an inverse, a
// quotient, a fifth root or a bit of the values on its wires 2 and 3, its live wires then being those sources alone — and the level loop
// runs over THREE lists per level, one per class of cost: gates and BIT hints, INV / DIV hints (x^(r-2)), ROOT5 hints (x^d), each class
// with a launch of its own, all three releasing consumers into the three lists of the next level by the gate's class (kept in its state
// word), whose sizes the host reads in one 24-byte copy.  The determinism argument holds for the three-list loop as it does for one list:
// a gate enters the list of its own class exactly once, in the level after the last of its sources was written, whichever lane
// decrements last; its value depends on source VALUES only, and those were written by earlier levels (the launches of one level write
// distinct variables and read none of them); levels counts iterations of the loop — dependency levels, not launches — and evaluations
// the list entries.  So order within a list, and which of a level's launches runs first, reach no output.  Without hint_op (NULL, and
// plonk_circuit_solve_dev) the kernels, launches and reads are the ones described above, untouched.
#pragma once
#include "circuit_kernels.hpp"

constexpr uint32_t SOLVE_NONE = 0xFFFFFFFFu;       // def_gate: "given"; start: "no consumers"
constexpr uint32_t SOLVE_PENDING = 7u;             // state bits 0-2: live inputs not written yet (0 .. 4)
constexpr uint32_t SOLVE_LIVE_SHIFT = 4;           // state bits 4-7: wire i < 4 is live
constexpr uint32_t SOLVE_DEF = 1u << 8;            // state bit 8: the gate defines the variable on its wire 4

// words of the flag area
enum { SOLVE_F_BAD_ID = 0, SOLVE_F_BAD_GATE, SOLVE_F_BAD_WIRE4, SOLVE_F_BAD_QO, SOLVE_F_BAD_QECC, SOLVE_F_DEFINED, SOLVE_F_UNSOLVED, SOLVE_F_COUNT0,
       SOLVE_F_COUNT1, SOLVE_F_WORDS,
       // with hints (solve_hints.hpp): three more minima, then the frontier sizes as 2 x 3 words (parity, class) instead of COUNT0 / COUNT1
       SOLVE_F_BAD_OP = SOLVE_F_WORDS, SOLVE_F_BAD_ARG, SOLVE_F_STRAY, SOLVE_F_HCOUNT, SOLVE_F_HINT_WORDS = SOLVE_F_HCOUNT + 6 };

// One lane per variable (a tile of 2048 per workgroup).  A valid definition marks its gate; flags: the smallest offending variable per
// kind of failure, and the number of valid definitions.
__global__ void __launch_bounds__(CIRC_THREADS) solve_validate_kernel(const uint32_t* __restrict__ def_gate, uint64_t num_vars, const uint32_t* __restrict__ wire_vars,
                                                                 const Fr* __restrict__ sel, uint64_t n, uint32_t* __restrict__ state,
                                                                 unsigned long long* __restrict__ flags) {
    __shared__ unsigned long long red[CIRC_THREADS];
    __shared__ uint32_t sbuf[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad_gate = CIRC_NONE, bad_w4 = CIRC_NONE, bad_qo = CIRC_NONE, bad_ecc = CIRC_NONE;
    uint32_t defined = 0;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t v = base + k * CIRC_THREADS + threadIdx.x;
        if (v >= num_vars) break;
        const uint32_t g = def_gate[v];
        if (g == SOLVE_NONE) continue;
        if (g >= n) { if (v < bad_gate) bad_gate = v; }
        else if (wire_vars[4 * n + g] != v) { if (v < bad_w4) bad_w4 = v; }
        else if (fp_is_zero(sel[10 * n + g])) { if (v < bad_qo) bad_qo = v; }
        else if (!fp_is_zero(sel[12 * n + g])) { if (v < bad_ecc) bad_ecc = v; }
        else { state[g] = SOLVE_DEF; defined++; }          // one writer: wire 4 of g names a single variable
    }
    bad_gate = circ_block_min(bad_gate, red);
    bad_w4 = circ_block_min(bad_w4, red);
    bad_qo = circ_block_min(bad_qo, red);
    bad_ecc = circ_block_min(bad_ecc, red);
    uint32_t total;
    (void)circ_block_exclusive_scan(defined, sbuf, &total);
    if (threadIdx.x == 0) {
        if (bad_gate != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_GATE, bad_gate);
        if (bad_w4 != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_WIRE4, bad_w4);
        if (bad_qo != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_QO, bad_qo);
        if (bad_ecc != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_QECC, bad_ecc);
        if (total) atomicAdd(flags + SOLVE_F_DEFINED, (unsigned long long)total);
    }
}

// One lane per gate: liveness, pending count and the four sort keys; gates with nothing pending are appended to the first frontier
// (one atomic per workgroup).  Runs after validation: every id indexes def_gate in bounds.
__global__ void __launch_bounds__(CIRC_THREADS) solve_keys_kernel(const uint32_t* __restrict__ wire_vars, const uint32_t* __restrict__ def_gate,
                                                             const Fr* __restrict__ sel, uint64_t n, uint32_t sentinel, uint32_t* __restrict__ state,
                                                             uint32_t* __restrict__ keys, uint32_t* __restrict__ frontier,
                                                             unsigned long long* __restrict__ frontier_count) {
    __shared__ uint32_t sbuf[CIRC_THREADS];
    __shared__ unsigned long long slot;
    const uint64_t j = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    uint32_t ready = 0;
    if (j < n) {
        uint32_t key[4] = {sentinel, sentinel, sentinel, sentinel};
        if (state[j] & SOLVE_DEF) {
            uint32_t mask = 0, pending = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const bool live = !fp_is_zero(sel[i * n + j]) || !fp_is_zero(sel[(6 + i) * n + j]) || !fp_is_zero(sel[(4 + i / 2) * n + j]);
                if (!live) continue;
                mask |= 1u << i;
                const uint32_t v = wire_vars[i * n + j];
                if (def_gate[v] != SOLVE_NONE) { key[i] = v; pending++; }
            }
            state[j] = SOLVE_DEF | (mask << SOLVE_LIVE_SHIFT) | pending;
            ready = pending == 0;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) keys[i * n + j] = key[i];
    }
    uint32_t total;
    const uint32_t at = circ_block_exclusive_scan(ready, sbuf, &total);
    if (threadIdx.x == 0 && total) slot = atomicAdd(frontier_count, (unsigned long long)total);
    __syncthreads();
    if (ready) frontier[slot + at] = (uint32_t)j;
}

// start[v] = the first sorted slot of variable v's consumers (start is preset to SOLVE_NONE)
__global__ void __launch_bounds__(CIRC_THREADS) solve_heads_kernel(const uint32_t* __restrict__ sk, uint64_t count, uint32_t sentinel, uint32_t* __restrict__ start) {
    const uint64_t s = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (s >= count) return;
    const uint32_t v = sk[s];
    if (v != sentinel && (s == 0 || sk[s - 1] != v)) start[v] = (uint32_t)s;
}

// One level: a lane per frontier gate.  The gathers of the live input values are the memory cost; a dead wire is not read.
__global__ void __launch_bounds__(CIRC_THREADS) solve_level_kernel(const uint32_t* __restrict__ frontier, uint64_t frontier_len, const uint32_t* __restrict__ wire_vars,
                                                              const Fr* __restrict__ sel, const Fr* __restrict__ pub, uint64_t n, Fr* __restrict__ witness,
                                                              const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint64_t count,
                                                              const uint32_t* __restrict__ start, uint32_t* __restrict__ state, uint32_t* __restrict__ next,
                                                              unsigned long long* __restrict__ next_count, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= frontier_len) return;
    const uint64_t g = frontier[t];
    const uint32_t live = state[g] >> SOLVE_LIVE_SHIFT;
    const Fr zero = fp_zero<8>();
    const Fr a = (live & 1) ? witness[wire_vars[g]] : zero;
    const Fr b = (live & 2) ? witness[wire_vars[n + g]] : zero;
    const Fr c = (live & 4) ? witness[wire_vars[2 * n + g]] : zero;
    const Fr d = (live & 8) ? witness[wire_vars[3 * n + g]] : zero;
    Fr val = circ_gate_inputs_value(a, b, c, d, sel, pub, n, g, P, nullptr);
    const Fr q_o = sel[10 * n + g], one = fp_one(P);
    if (!fp_eq(q_o, one)) val = fp_eq(q_o, fp_neg(one, P)) ? fp_neg(val, P) : fp_mul(val, fp_inv(q_o, P), P);
    const uint32_t v = wire_vars[4 * n + g];
    witness[v] = val;
    for (uint64_t s = start[v]; s < count && sk[s] == v; s++) {          // SOLVE_NONE >= count: no consumers
        const uint32_t cg = sv[s] & (uint32_t)(n - 1);                    // position i*n + gate, n a power of two
        const uint32_t old = atomicAdd(&state[cg], 0xFFFFFFFFu);
        if ((old & SOLVE_PENDING) == 1) next[atomicAdd(next_count, 1ull)] = cg;
    }
}

// the smallest defined variable whose gate still waits for an input: a dependency cycle (or something downstream of one)
__global__ void __launch_bounds__(CIRC_THREADS) solve_unsolved_kernel(const uint32_t* __restrict__ def_gate, uint64_t num_vars, const uint32_t* __restrict__ state,
                                                                 unsigned long long* __restrict__ first) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad = CIRC_NONE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t v = base + k * CIRC_THREADS + threadIdx.x;
        if (v >= num_vars) break;
        const uint32_t g = def_gate[v];
        if (g != SOLVE_NONE && (state[g] & SOLVE_PENDING) && v < bad) bad = v;
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first, bad);
}

#include "solve_hints.hpp"

// scratch layout (bytes, each piece 256-aligned): flags | 4 sort arrays of 4n u32 | hist | block sums | start[num_vars] | state[n] | 2 frontiers of n u32
// (with hints: 2 frontiers of 3 lists of n u32, one list per class)
struct SolveScratch {
    size_t keys[2] = {0, 0}, vals[2] = {0, 0}, hist = 0, sums = 0, start = 0, state = 0, frontier[2] = {0, 0}, total = 0;
    uint64_t count = 0;
    SolveScratch(size_t n, size_t num_vars, bool hints) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        count = 4 * (uint64_t)n;
        const uint64_t hist_len = (uint64_t)CIRC_DIGITS * circ_grid_of(count, CIRC_TILE);
        size_t at = al(SOLVE_F_HINT_WORDS * sizeof(unsigned long long));
        for (int b = 0; b < 2; b++) { keys[b] = at; at += al(count * 4); vals[b] = at; at += al(count * 4); }
        hist = at; at += al(hist_len * 4);
        sums = at; at += al((size_t)circ_grid_of(hist_len, CIRC_TILE) * 4);
        start = at; at += al(num_vars * 4);
        state = at; at += al(n * 4);
        for (int b = 0; b < 2; b++) { frontier[b] = at; at += al((hints ? SOLVE_CLASSES : 1) * n * 4); }
        total = at;
    }
};

size_t circuit_solve_scratch_bytes(size_t n, size_t num_vars, bool hints) { return SolveScratch(n, num_vars, hints).total; }

// The solver's device pointers into its scratch area.
struct SolveBuffers {
    unsigned long long* flags;
    uint32_t *keys[2], *vals[2], *hist, *sums, *start, *state, *frontier[2];
    SolveBuffers(const SolveScratch& L, void* scratch) {
        char* base = (char*)scratch;
        flags = (unsigned long long*)base;
        for (int b = 0; b < 2; b++) {
            keys[b] = (uint32_t*)(base + L.keys[b]);
            vals[b] = (uint32_t*)(base + L.vals[b]);
            frontier[b] = (uint32_t*)(base + L.frontier[b]);
        }
        hist = (uint32_t*)(base + L.hist);
        sums = (uint32_t*)(base + L.sums);
        start = (uint32_t*)(base + L.start);
        state = (uint32_t*)(base + L.state);
    }
};

// Everything before the level loop, shared by the solver and by the schedule recorder (solve_replay.hpp): validation with its error texts,
// the state words and sort keys, the first frontier (in B.frontier[0], its size in the flag area) and the consumer lists *sk / *sv with their
// heads in B.start.  *defined: the number of defining gates; 0 = nothing was sorted and there is nothing to solve.
static int solve_prepare(const uint32_t* wire_vars, size_t n, size_t num_vars, const Fr* sel, const uint32_t* def_gate, const uint32_t* hint_op,
                         const SolveScratch& L, const SolveBuffers& B, hipStream_t stream, const char* who, uint64_t* defined, const uint32_t** sk,
                         const uint32_t** sv) {
    const bool hints = hint_op != nullptr;
    unsigned long long* d_flags = B.flags;
    uint32_t* state = B.state;
    const uint64_t N = L.count;
    const uint32_t sentinel = (uint32_t)num_vars;        // num_vars <= 2^32 - 2: larger than every id, and not SOLVE_NONE
    const uint32_t var_tiles = circ_grid_of(num_vars, CIRC_TILE);
    unsigned long long h[SOLVE_F_HINT_WORDS];
    const size_t flag_words = hints ? SOLVE_F_HINT_WORDS : SOLVE_F_WORDS;
    int rc;
    *defined = 0;
    {
        ProfScope ps("solve_setup", stream);
        // flags: the minima start at all-ones, the three counters at zero
        HIP_TRY(hipMemsetAsync(d_flags, 0xFF, flag_words * sizeof(*d_flags), stream));
        HIP_TRY(hipMemsetAsync(d_flags + SOLVE_F_DEFINED, 0, sizeof(*d_flags), stream));
        if (hints) HIP_TRY(hipMemsetAsync(d_flags + SOLVE_F_HCOUNT, 0, 6 * sizeof(*d_flags), stream));
        else HIP_TRY(hipMemsetAsync(d_flags + SOLVE_F_COUNT0, 0, 2 * sizeof(*d_flags), stream));
        HIP_TRY(hipMemsetAsync(state, 0, n * 4, stream));
        hipLaunchKernelGGL(circuit_ids_check_kernel, dim3(circ_grid_of(5 * (uint64_t)n, CIRC_TILE)), dim3(CIRC_THREADS), 0, stream, wire_vars, 5 * (uint64_t)n,
                           (uint64_t)num_vars, d_flags + SOLVE_F_BAD_ID);
        if (hints) {
            hipLaunchKernelGGL(solve_hint_validate_kernel, dim3(var_tiles), dim3(CIRC_THREADS), 0, stream, def_gate, (uint64_t)num_vars, wire_vars, sel, hint_op,
                               (uint64_t)n, state, d_flags);
            hipLaunchKernelGGL(solve_hint_stray_kernel, dim3(circ_grid_of(n, CIRC_TILE)), dim3(CIRC_THREADS), 0, stream, hint_op, (uint64_t)n, (const uint32_t*)state,
                               d_flags + SOLVE_F_STRAY);
        } else {
            hipLaunchKernelGGL(solve_validate_kernel, dim3(var_tiles), dim3(CIRC_THREADS), 0, stream, def_gate, (uint64_t)num_vars, wire_vars, sel, (uint64_t)n, state,
                               d_flags);
        }
        if ((rc = circ_launch_status("solve_validate"))) return rc;
        HIP_TRY(hipMemcpyAsync(h, d_flags, flag_words * sizeof(*h), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h[SOLVE_F_BAD_ID] != CIRC_NONE)
            return plonk_fail(PLONK_ERR_ARG, "%s: wire %llu of gate %llu reads a variable id >= num_vars = %zu", who, h[SOLVE_F_BAD_ID] / n,
                              h[SOLVE_F_BAD_ID] % n, num_vars);
        unsigned long long bad = CIRC_NONE;
        int why = 0;
        for (int f = SOLVE_F_BAD_GATE; f <= SOLVE_F_BAD_QECC; f++)
            if (h[f] < bad) { bad = h[f]; why = f; }
        if (hints)
            for (int f = SOLVE_F_BAD_OP; f <= SOLVE_F_BAD_ARG; f++)
                if (h[f] < bad) { bad = h[f]; why = f; }
        if (why) {
            uint32_t g = 0;
            HIP_TRY(hipMemcpyAsync(&g, def_gate + bad, sizeof(g), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            const char* what = why == SOLVE_F_BAD_GATE    ? "that gate is >= n"
                               : why == SOLVE_F_BAD_WIRE4 ? "wire 4 of that gate reads another variable"
                               : why == SOLVE_F_BAD_QO    ? "q_o is zero at that gate"
                               : why == SOLVE_F_BAD_QECC  ? "q_ecc is not zero at that gate"
                               : why == SOLVE_F_BAD_OP    ? "hint_op there has an unknown opcode (1 INV, 2 DIV, 3 ROOT5, 4 BIT)"
                                                          : "the BIT hint there has an argument >= 256";
            return plonk_fail(PLONK_ERR_ARG, "%s: variable %llu is defined by gate %u, but %s (n = %zu)", who, bad, g, what, n);
        }
        if (hints && h[SOLVE_F_STRAY] != CIRC_NONE)
            return plonk_fail(PLONK_ERR_ARG, "%s: hint_op is not zero at gate %llu, which defines no variable", who, h[SOLVE_F_STRAY]);
        if (h[SOLVE_F_DEFINED] == 0) return PLONK_OK;
        *defined = h[SOLVE_F_DEFINED];
        HIP_TRY(hipMemsetAsync(B.start, 0xFF, num_vars * 4, stream));
        if (hints)
            hipLaunchKernelGGL(solve_hint_keys_kernel, dim3(circ_grid_of(n, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, wire_vars, def_gate, sel, hint_op, (uint64_t)n,
                               sentinel, state, B.keys[1], B.frontier[0], d_flags + SOLVE_F_HCOUNT);
        else
            hipLaunchKernelGGL(solve_keys_kernel, dim3(circ_grid_of(n, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, wire_vars, def_gate, sel, (uint64_t)n, sentinel, state,
                               B.keys[1], B.frontier[0], d_flags + SOLVE_F_COUNT0);
        if ((rc = circ_launch_status("solve_keys"))) return rc;
    }
    *sk = B.keys[1];
    *sv = nullptr;
    {
        ProfScope ps("solve_sort", stream);
        if ((rc = circ_radix_sort(sk, sv, N, circ_radix_passes((uint64_t)num_vars + 1), B.keys, B.vals, B.hist, B.sums, stream))) return rc;
        hipLaunchKernelGGL(solve_heads_kernel, dim3(circ_grid_of(N, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, *sk, N, sentinel, B.start);
        if ((rc = circ_launch_status("solve_heads"))) return rc;
    }
    return PLONK_OK;
}

// hint_op NULL: the hint-free solver, kernel for kernel what it was before hints existed.  who: the entry point named in error texts.
int circuit_solve_run(int curve, const uint32_t* wire_vars, size_t n, size_t num_vars, const Fr* sel, const Fr* pub, const uint32_t* def_gate,
                      const uint32_t* hint_op, Fr* witness, int64_t* unsolved_var, uint64_t* levels, uint64_t* evaluations, void* scratch, hipStream_t stream,
                      const char* who) {
    const bool hints = hint_op != nullptr;
    const SolveScratch L(n, num_vars, hints);
    const SolveBuffers B(L, scratch);
    unsigned long long* d_flags = B.flags;
    uint32_t* const start = B.start;
    uint32_t* const state = B.state;
    uint32_t* const* frontier = B.frontier;
    const uint64_t N = L.count;
    const FrParams& P = fr_params(curve);
    const uint32_t var_tiles = circ_grid_of(num_vars, CIRC_TILE);
    SolveExponent e_inv, e_root5;
    if (hints && !solve_exponents(P, &e_inv, &e_root5)) return plonk_fail(PLONK_ERR_ARG, "%s: 5 divides r - 1, ROOT5 is not defined on this field", who);
    int rc;
    *unsolved_var = -1;
    *levels = 0;
    *evaluations = 0;
    uint64_t defined = 0;
    const uint32_t* sk = nullptr;
    const uint32_t* sv = nullptr;
    if ((rc = solve_prepare(wire_vars, n, num_vars, sel, def_gate, hint_op, L, B, stream, who, &defined, &sk, &sv))) return rc;
    if (!defined) return PLONK_OK;
    uint64_t done = 0, depth = 0;
    if (hints) {
        // Per level: class 0 (gates, BIT), class 1 (INV, DIV) and class 2 (ROOT5) each in a launch of its own over its own list; all three read
        // values of earlier levels only and release into the three lists of the other parity, whose sizes come back in one 24-byte read.
        ProfScope ps("solve_levels", stream);
        unsigned long long len[SOLVE_CLASSES] = {0, 0, 0};
        auto read_counts = [&](const unsigned long long* d) -> int {
            HIP_TRY(hipMemcpyAsync(len, d, sizeof(len), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            return PLONK_OK;
        };
        if ((rc = read_counts(d_flags + SOLVE_F_HCOUNT))) return rc;
        for (int cur = 0; len[0] + len[1] + len[2]; cur ^= 1) {
            const unsigned long long all = len[0] + len[1] + len[2];
            if (len[0] > n || len[1] > n || len[2] > n || all > defined - done)
                return plonk_fail(PLONK_ERR_HIP, "%s: a frontier of %llu gates with %llu left", who, all, (unsigned long long)(defined - done));
            unsigned long long* d_next = d_flags + SOLVE_F_HCOUNT + SOLVE_CLASSES * (cur ^ 1);
            HIP_TRY(hipMemsetAsync(d_next, 0, sizeof(len), stream));
            const uint32_t* fr = frontier[cur];
            if (len[0])
                hipLaunchKernelGGL(solve_hint_level_kernel, dim3(circ_grid_of(len[0], CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, fr, (uint64_t)len[0], wire_vars, sel, pub,
                                   hint_op, (uint64_t)n, witness, sk, sv, N, (const uint32_t*)start, state, frontier[cur ^ 1], d_next, P);
            if (len[1])
                hipLaunchKernelGGL(solve_pow_kernel, dim3(circ_grid_of(len[1], CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, fr + n, (uint64_t)len[1], wire_vars, hint_op,
                                   (uint64_t)n, witness, sk, sv, N, (const uint32_t*)start, state, frontier[cur ^ 1], d_next, e_inv, P);
            if (len[2])
                hipLaunchKernelGGL(solve_pow_kernel, dim3(circ_grid_of(len[2], CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, fr + 2 * n, (uint64_t)len[2], wire_vars, hint_op,
                                   (uint64_t)n, witness, sk, sv, N, (const uint32_t*)start, state, frontier[cur ^ 1], d_next, e_root5, P);
            if ((rc = circ_launch_status("solve_level"))) return rc;
            done += all;
            depth++;
            if ((rc = read_counts(d_next))) return rc;
        }
    } else {
        ProfScope ps("solve_levels", stream);
        unsigned long long len = 0;
        if ((rc = circ_read_flag(d_flags + SOLVE_F_COUNT0, &len, stream))) return rc;
        for (int cur = 0; len; cur ^= 1) {
            if (len > defined - done) return plonk_fail(PLONK_ERR_HIP, "%s: a frontier of %llu gates with %llu left", who, len, (unsigned long long)(defined - done));
            unsigned long long* d_next = d_flags + SOLVE_F_COUNT0 + (cur ^ 1);
            HIP_TRY(hipMemsetAsync(d_next, 0, sizeof(*d_next), stream));
            hipLaunchKernelGGL(solve_level_kernel, dim3(circ_grid_of(len, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, (const uint32_t*)frontier[cur], (uint64_t)len,
                               wire_vars, sel, pub, (uint64_t)n, witness, sk, sv, N, (const uint32_t*)start, state, frontier[cur ^ 1], d_next, P);
            if ((rc = circ_launch_status("solve_level"))) return rc;
            done += len;
            depth++;
            if ((rc = circ_read_flag(d_next, &len, stream))) return rc;
        }
    }
    *levels = depth;
    *evaluations = done;
    if (done != defined) {
        unsigned long long first = CIRC_NONE;
        hipLaunchKernelGGL(solve_unsolved_kernel, dim3(var_tiles), dim3(CIRC_THREADS), 0, stream, def_gate, (uint64_t)num_vars, (const uint32_t*)state,
                           d_flags + SOLVE_F_UNSOLVED);
        if ((rc = circ_launch_status("solve_unsolved"))) return rc;
        if ((rc = circ_read_flag(d_flags + SOLVE_F_UNSOLVED, &first, stream))) return rc;
        *unsolved_var = first == CIRC_NONE ? -1 : (int64_t)first;
    }
    return PLONK_OK;
}

#include "solve_replay.hpp"
