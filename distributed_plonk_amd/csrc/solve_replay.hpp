// solve_replay.hpp — the solver's schedule recorded once and replayed for batches of witnesses (included by solve_kernels.hpp after
// circuit_solve_run, whose setup — validation, state words, consumer lists — the recorder shares through solve_prepare).
//
// Which gate is evaluated in which level is a function of wire_vars, selector_evals, def_gate and hint_op alone.  The solver finds it out
// while it computes values: a launch, an atomic frontier append and a host read per level, for every witness again.
//   * circuit_schedule_run walks the same levels once, structurally: its level kernel writes no field value; it records key 3L + c for the
//     gate (level L, cost class c of solve_hints.hpp) and releases consumers as the solver does.  The frontier's order still depends on
//     which lane appends first; the recorded keys do not, and the existing stable radix sort of (key, gate) turns them into
//     order[0 .. evaluations) sorted by (L, c, gate) with the segment starts seg[3L + c] — a function of the circuit alone.
//   * circuit_replay_run evaluates K witnesses from that order with no atomics, no sort and no host read: per segment one WIDE launch of
//     seg_len x K lanes, or, for a run of consecutive narrow segments, one FUSED launch in which workgroup b walks the run for witness b
//     with a barrier between levels.  Each gate goes through the value code of the solver (circ_gate_inputs_value / q_o, the BIT select,
//     solve_pow_fixed), so a replayed witness is bit-identical to a solved one.
// Determinism of the fused form: a variable is written exactly once per witness, by the gate that defines it, in the level the schedule
// gave that gate; a gate of level L reads live wires only, and those read given variables or variables of levels < L, which the same
// workgroup wrote before a barrier it has passed (or an earlier launch wrote).  The segments of one level write distinct variables and
// read none of them, so no barrier separates them.  Witnesses never share a variable, workgroups never wait for each other.
#pragma once

constexpr uint32_t REPLAY_NONE = 0xFFFFFFFFu;      // level key of a gate that was never evaluated: sorts behind every 3L + c

__device__ const Fr replay_zero_pi = {};           // PI of a gate that carries no public input

// One level of the structural walk: a lane per frontier gate records the gate's key and releases the consumers of its variable into the
// next frontier (one list: the class travels in the state word).  level3 = 3 * level.
__global__ void __launch_bounds__(CIRC_THREADS) replay_schedule_level_kernel(const uint32_t* __restrict__ frontier, uint64_t frontier_len,
                                                                             const uint32_t* __restrict__ wire_vars, uint64_t n, const uint32_t* __restrict__ sk,
                                                                             const uint32_t* __restrict__ sv, uint64_t count, const uint32_t* __restrict__ start,
                                                                             uint32_t* __restrict__ state, uint32_t* __restrict__ next,
                                                                             unsigned long long* __restrict__ next_count, uint32_t* __restrict__ level_key,
                                                                             uint32_t level3) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= frontier_len) return;
    const uint64_t g = frontier[t];
    level_key[g] = level3 + ((state[g] >> SOLVE_CLASS_SHIFT) & 3u);       // nothing is pending at g: no lane touches its state word any more
    const uint32_t v = wire_vars[4 * n + g];
    for (uint64_t s = start[v]; s < count && sk[s] == v; s++) {           // SOLVE_NONE >= count: no consumers
        const uint32_t cg = sv[s] & (uint32_t)(n - 1);
        const uint32_t old = atomicAdd(&state[cg], 0xFFFFFFFFu);
        if ((old & SOLVE_PENDING) == 1) next[atomicAdd(next_count, 1ull)] = cg;
    }
}

// The value of gate g's variable for the witness W, stored: what solve_level_kernel / solve_hint_level_kernel (cls 0) and solve_pow_kernel
// (cls 1: e = r - 2, cls 2: e = d) compute.  Liveness is what the keys kernels derive from the selectors; a dead wire is not read.
// pub: this witness's num_inputs public inputs.  cls and e are uniform over the wave.
__device__ __forceinline__ void replay_gate(uint64_t g, uint32_t cls, const uint32_t* __restrict__ wire_vars, const Fr* __restrict__ sel,
                                            const uint32_t* __restrict__ hint_op, const Fr* __restrict__ pub, uint64_t num_inputs, uint64_t n, Fr* W,
                                            const SolveExponent& e, const FrParams& P) {
    const uint32_t h = hint_op ? hint_op[g] : 0u;
    const Fr zero = fp_zero<8>();
    Fr val;
    if (cls) {
        const bool div = (h & 0xFFu) == SOLVE_OP_DIV;
        const Fr s0 = W[wire_vars[2 * n + g]];
        Fr base = s0;
        if (div) base = W[wire_vars[3 * n + g]];
        val = solve_pow_fixed(base, e, P);
        if (div) val = fp_mul(s0, val, P);
    } else if (h) {                                                        // BIT
        const Fr x = fp_from_mont(W[wire_vars[2 * n + g]], P);
        const uint32_t k = h >> 8;
        uint32_t word = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) word = (k >> 5) == i ? x.l[i] : word;
        val = ((word >> (k & 31)) & 1u) ? fp_one(P) : zero;
    } else {
        const Fr* q = sel + g;                                             // q[t * n]: selector t of gate g
        const bool mul0 = !fp_is_zero(q[4 * n]), mul1 = !fp_is_zero(q[5 * n]);
        Fr a = zero, b = zero, c = zero, d = zero;
        if (mul0 || !fp_is_zero(q[0]) || !fp_is_zero(q[6 * n])) a = W[wire_vars[g]];
        if (mul0 || !fp_is_zero(q[n]) || !fp_is_zero(q[7 * n])) b = W[wire_vars[n + g]];
        if (mul1 || !fp_is_zero(q[2 * n]) || !fp_is_zero(q[8 * n])) c = W[wire_vars[2 * n + g]];
        if (mul1 || !fp_is_zero(q[3 * n]) || !fp_is_zero(q[9 * n])) d = W[wire_vars[3 * n + g]];
        val = circ_gate_inputs_value(a, b, c, d, q, g < num_inputs ? pub + g : &replay_zero_pi, n, 0, P, nullptr);
        const Fr q_o = q[10 * n], one = fp_one(P);
        if (!fp_eq(q_o, one)) val = fp_eq(q_o, fp_neg(one, P)) ? fp_neg(val, P) : fp_mul(val, fp_inv(q_o, P), P);
    }
    W[wire_vars[4 * n + g]] = val;
}

// WIDE: one segment order[lo .. lo + len) of class cls for all K witnesses, lane t = b * len + i.
__global__ void __launch_bounds__(CIRC_THREADS) replay_wide_kernel(const uint32_t* __restrict__ order, uint32_t lo, uint32_t len, uint64_t K, uint32_t cls,
                                                                   const uint32_t* __restrict__ wire_vars, const Fr* __restrict__ sel,
                                                                   const uint32_t* __restrict__ hint_op, const Fr* __restrict__ pub, uint64_t num_inputs, uint64_t n,
                                                                   uint64_t num_vars, Fr* witness, const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= (uint64_t)len * K) return;
    const uint64_t b = t / len;
    const uint64_t g = order[lo + (uint32_t)(t - b * len)];
    if (g >= n) return;
    replay_gate(g, cls, wire_vars, sel, hint_op, pub + b * num_inputs, num_inputs, n, witness + b * num_vars, e, P);
}

// FUSED: the segments s0 .. s1 of the schedule (segment s = 3L + c starts at seg[s]) for witness blockIdx.x, the workgroup's lanes striding
// over each segment.  A level reads what earlier levels wrote to global memory: a barrier where the level changes, none between the
// classes of one level.  Every lane of the workgroup reaches every barrier: s, s1 and seg are uniform.
__global__ void __launch_bounds__(CIRC_THREADS) replay_fused_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ seg, uint32_t s0, uint32_t s1,
                                                                    const uint32_t* __restrict__ wire_vars, const Fr* __restrict__ sel,
                                                                    const uint32_t* __restrict__ hint_op, const Fr* __restrict__ pub, uint64_t num_inputs, uint64_t n,
                                                                    uint64_t num_vars, Fr* witness, const SolveExponent e_inv, const SolveExponent e_root5,
                                                                    const FrParams P) {
    Fr* W = witness + (uint64_t)blockIdx.x * num_vars;
    const Fr* my_pub = pub + (uint64_t)blockIdx.x * num_inputs;
    for (uint32_t s = s0; s < s1; s++) {
        const uint32_t cls = s % 3u;
        if (cls == 0 && s != s0) __syncthreads();
        const uint32_t hi = seg[s + 1];
        for (uint32_t i = seg[s] + threadIdx.x; i < hi; i += CIRC_THREADS) {
            const uint64_t g = order[i];
            if (g < n) replay_gate(g, cls, wire_vars, sel, hint_op, my_pub, num_inputs, n, W, cls == 2 ? e_root5 : e_inv, P);
        }
    }
}

// scratch of the recorder: the solver's, then the level keys [n] and the segment heads [3n + 1] (a level holds at least one gate)
struct ScheduleScratch {
    SolveScratch solve;
    size_t level_key = 0, heads = 0, total = 0;
    ScheduleScratch(size_t n, size_t num_vars, bool hints) : solve(n, num_vars, hints) {
        auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
        size_t at = solve.total;
        level_key = at; at += al(n * 4);
        heads = at; at += al((3 * n + 1) * 4);
        total = at;
    }
};

size_t circuit_schedule_scratch_bytes(size_t n, size_t num_vars, bool hints) { return ScheduleScratch(n, num_vars, hints).total; }

// order: device u32 [n]; seg: HOST, 3n + 1 words of which 3 * levels + 1 are written.  Synchronises.
int circuit_schedule_run(const uint32_t* wire_vars, size_t n, size_t num_vars, const Fr* sel, const uint32_t* def_gate, const uint32_t* hint_op, uint32_t* order,
                         uint32_t* seg, int64_t* unsolved_var, uint64_t* levels, uint64_t* evaluations, void* scratch, hipStream_t stream, const char* who) {
    const bool hints = hint_op != nullptr;
    const ScheduleScratch L(n, num_vars, hints);
    const SolveBuffers B(L.solve, scratch);
    uint32_t* level_key = (uint32_t*)((char*)scratch + L.level_key);
    uint32_t* heads = (uint32_t*)((char*)scratch + L.heads);
    unsigned long long* d_flags = B.flags;
    const uint64_t N = L.solve.count;
    int rc;
    *unsolved_var = -1;
    *levels = 0;
    *evaluations = 0;
    seg[0] = 0;
    uint64_t defined = 0;
    const uint32_t* sk = nullptr;
    const uint32_t* sv = nullptr;
    if ((rc = solve_prepare(wire_vars, n, num_vars, sel, def_gate, hint_op, L.solve, B, stream, who, &defined, &sk, &sv))) return rc;
    if (!defined) return PLONK_OK;
    uint64_t done = 0, depth = 0;
    {
        // The first frontier is where the keys kernel put it: one list, or with hints one list per class.  Every later one is a single list, its
        // size in COUNT0 / COUNT1 by parity (with hints those two words are otherwise unused).
        ProfScope ps("schedule_levels", stream);
        HIP_TRY(hipMemsetAsync(level_key, 0xFF, n * 4, stream));
        unsigned long long first[SOLVE_CLASSES] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(first, d_flags + (hints ? SOLVE_F_HCOUNT : SOLVE_F_COUNT0), (hints ? SOLVE_CLASSES : 1) * sizeof(*first), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        unsigned long long len = first[0] + first[1] + first[2];
        for (int cur = 0; len; cur ^= 1) {
            if (len > defined - done) return plonk_fail(PLONK_ERR_HIP, "%s: a frontier of %llu gates with %llu left", who, len, (unsigned long long)(defined - done));
            unsigned long long* d_next = d_flags + SOLVE_F_COUNT0 + (cur ^ 1);
            HIP_TRY(hipMemsetAsync(d_next, 0, sizeof(*d_next), stream));
            for (int c = 0; c < (depth == 0 ? SOLVE_CLASSES : 1); c++) {
                const unsigned long long part = depth == 0 ? first[c] : len;
                if (!part) continue;
                hipLaunchKernelGGL(replay_schedule_level_kernel, dim3(circ_grid_of(part, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream,
                                   (const uint32_t*)B.frontier[cur] + c * n, (uint64_t)part, wire_vars, (uint64_t)n, sk, sv, N, (const uint32_t*)B.start, B.state,
                                   B.frontier[cur ^ 1], d_next, level_key, (uint32_t)(3 * depth));
            }
            if ((rc = circ_launch_status("schedule_level"))) return rc;
            done += len;
            depth++;
            if ((rc = circ_read_flag(d_next, &len, stream))) return rc;
        }
    }
    *levels = depth;
    *evaluations = done;
    if (done != defined) {
        unsigned long long first = CIRC_NONE;
        hipLaunchKernelGGL(solve_unsolved_kernel, dim3(circ_grid_of(num_vars, CIRC_TILE)), dim3(CIRC_THREADS), 0, stream, def_gate, (uint64_t)num_vars,
                           (const uint32_t*)B.state, d_flags + SOLVE_F_UNSOLVED);
        if ((rc = circ_launch_status("solve_unsolved"))) return rc;
        if ((rc = circ_read_flag(d_flags + SOLVE_F_UNSOLVED, &first, stream))) return rc;
        *unsolved_var = first == CIRC_NONE ? -1 : (int64_t)first;
    }
    {
        // (key, gate) sorted by the stable radix sort: gates of one key stay in ascending order.  The passes cover keys <= 3 * levels; the
        // low bits of REPLAY_NONE are all ones, above every recorded key, so the gates that were never evaluated sort last in those passes too.
        ProfScope ps("schedule_sort", stream);
        const uint64_t segments = 3 * depth;
        const uint32_t* kin = level_key;
        const uint32_t* vin = nullptr;
        if ((rc = circ_radix_sort(&kin, &vin, n, circ_radix_passes(segments + 1), B.keys, B.vals, B.hist, B.sums, stream))) return rc;
        HIP_TRY(hipMemsetAsync(heads, 0xFF, segments * 4, stream));
        hipLaunchKernelGGL(solve_heads_kernel, dim3(circ_grid_of(n, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, kin, (uint64_t)n, REPLAY_NONE, heads);
        if ((rc = circ_launch_status("schedule_heads"))) return rc;
        HIP_TRY(hipMemcpyAsync(order, vin, n * 4, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(seg, heads, segments * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        seg[segments] = (uint32_t)done;
        for (uint64_t s = segments; s-- > 0;)
            if (seg[s] == REPLAY_NONE) seg[s] = seg[s + 1];                // an empty segment starts where the next one does
    }
    return PLONK_OK;
}

// The launch plan is read off seg alone: a maximal run of consecutive segments of at most fuse_width gates each goes into one fused launch
// when it holds more than one non-empty segment, every other non-empty segment into a wide launch.  Enqueued only.
// d_seg: the 3 * levels + 1 words of seg on the device (read by fused launches only).
int circuit_replay_run(int curve, const uint32_t* wire_vars, size_t n, size_t num_vars, const Fr* sel, const uint32_t* hint_op, const uint32_t* order,
                       const uint32_t* seg, const uint32_t* d_seg, uint64_t levels, const Fr* pub, size_t num_inputs, Fr* witness, size_t K, unsigned fuse_width,
                       hipStream_t stream, const char* who) {
    const FrParams& P = fr_params(curve);
    SolveExponent e_inv, e_root5;
    if (!solve_exponents(P, &e_inv, &e_root5)) {
        if (hint_op) return plonk_fail(PLONK_ERR_ARG, "%s: 5 divides r - 1, ROOT5 is not defined on this field", who);
        e_root5 = e_inv;
    }
    const uint64_t segments = 3 * levels;
    ProfScope ps("replay_levels", stream);
    auto wide = [&](uint64_t s) {
        const uint32_t len = seg[s + 1] - seg[s];
        if (!len) return;
        hipLaunchKernelGGL(replay_wide_kernel, dim3(circ_grid_of((uint64_t)len * K, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, order, seg[s], len, (uint64_t)K,
                           (uint32_t)(s % 3), wire_vars, sel, hint_op, pub, (uint64_t)num_inputs, (uint64_t)n, (uint64_t)num_vars, witness,
                           s % 3 == 2 ? e_root5 : e_inv, P);
    };
    for (uint64_t s = 0; s < segments;) {
        uint64_t end = s, busy = 0;
        while (fuse_width && end < segments && seg[end + 1] - seg[end] <= fuse_width) busy += seg[end + 1] != seg[end], end++;
        if (busy > 1) {
            hipLaunchKernelGGL(replay_fused_kernel, dim3((uint32_t)K), dim3(CIRC_THREADS), 0, stream, order, d_seg, (uint32_t)s, (uint32_t)end, wire_vars, sel, hint_op,
                               pub, (uint64_t)num_inputs, (uint64_t)n, (uint64_t)num_vars, witness, e_inv, e_root5, P);
            s = end;
        } else if (end > s) {
            for (; s < end; s++) wide(s);
        } else {
            wide(s++);
        }
    }
    return circ_launch_status("replay");
}
