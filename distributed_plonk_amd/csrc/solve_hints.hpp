// solve_hints.hpp — hinted definitions of the witness solver (included by solve_kernels.hpp after its own kernels, whose state word, flag
// area and consumer lists these kernels share).  A gate g with a non-zero opcode in hint_op[g] (bits 0-7; bits 8-31 an argument) defines
// the variable on its wire 4 from the VALUES on wire 2 (s0) and wire 3 (s1) by a computation that is not a gate — the gate's selectors are
// not read here; they carry whatever constraint checks the result:
//     1 INV    s0^-1, 0 for s0 = 0            2 DIV    s0 * s1^-1, 0 for s1 = 0
//     3 ROOT5  s0^d, d = 5^-1 mod (r - 1)     4 BIT    bit `arg` of the canonical residue of s0 (0 above the field's bit length)
// Its dependencies are its source wires alone (wire 2; wire 3 for DIV): wires 0 and 1 are dead for scheduling whatever the selectors
// say, so a check such as x * y = 1 may read the gate's own output there.
//
// INV, DIV and ROOT5 are fixed-exponent powers of ~254 bits (r - 2, or d): 329 to 340 field products at the 3-bit window used here,
// depending on field and exponent (counted in profiles/circuit_hints.txt), against the ~20 of a gate evaluation.  A pow lane among gate lanes would hold its wave an order of
// magnitude longer, so frontier gates are released into one dense list per CLASS, each class with a launch of its own per level:
//     class 0  ordinary gates and BIT hints  -> solve_hint_level_kernel
//     class 1  INV and DIV, exponent r - 2   -> solve_pow_kernel
//     class 2  ROOT5, exponent d             -> solve_pow_kernel
// The exponent is a kernel argument, so every window digit is a scalar and the table lookup a uniform branch: no divergence.
#pragma once

constexpr uint32_t SOLVE_OP_INV = 1, SOLVE_OP_DIV = 2, SOLVE_OP_ROOT5 = 3, SOLVE_OP_BIT = 4, SOLVE_OP_LAST = 4;
constexpr uint32_t SOLVE_BIT_ARGS = 256;           // BIT arguments lie in [0, 256)
constexpr uint32_t SOLVE_CLASS_SHIFT = 9;          // state bits 9-10: the frontier class of the gate
constexpr int SOLVE_CLASSES = 3;
constexpr int SOLVE_POW_WINDOW = 3;                // 7 table entries of 8 words: 56 VGPRs; 4 bits would cost 120 for 4 to 12 products fewer

__device__ __forceinline__ uint32_t solve_class_of(uint32_t opcode) {
    return (opcode == SOLVE_OP_INV || opcode == SOLVE_OP_DIV) ? 1u : opcode == SOLVE_OP_ROOT5 ? 2u : 0u;
}

struct SolveExponent {
    uint32_t w[8];                                 // little-endian, < 2^255
};

// The variant of solve_validate_kernel for a circuit with hints.  At a hint gate q_o and q_ecc are free; its opcode and argument are checked.
__global__ void __launch_bounds__(CIRC_THREADS) solve_hint_validate_kernel(const uint32_t* __restrict__ def_gate, uint64_t num_vars,
                                                                           const uint32_t* __restrict__ wire_vars, const Fr* __restrict__ sel,
                                                                           const uint32_t* __restrict__ hint_op, uint64_t n, uint32_t* __restrict__ state,
                                                                           unsigned long long* __restrict__ flags) {
    __shared__ unsigned long long red[CIRC_THREADS];
    __shared__ uint32_t sbuf[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad_gate = CIRC_NONE, bad_w4 = CIRC_NONE, bad_qo = CIRC_NONE, bad_ecc = CIRC_NONE, bad_op = CIRC_NONE, bad_arg = CIRC_NONE;
    uint32_t defined = 0;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t v = base + k * CIRC_THREADS + threadIdx.x;
        if (v >= num_vars) break;
        const uint32_t g = def_gate[v];
        if (g == SOLVE_NONE) continue;
        if (g >= n) { if (v < bad_gate) bad_gate = v; continue; }
        if (wire_vars[4 * n + g] != v) { if (v < bad_w4) bad_w4 = v; continue; }
        const uint32_t h = hint_op[g], opcode = h & 0xFFu;
        if (h == 0) {
            if (fp_is_zero(sel[10 * n + g])) { if (v < bad_qo) bad_qo = v; }
            else if (!fp_is_zero(sel[12 * n + g])) { if (v < bad_ecc) bad_ecc = v; }
            else { state[g] = SOLVE_DEF; defined++; }
        } else if (opcode == 0 || opcode > SOLVE_OP_LAST) { if (v < bad_op) bad_op = v; }      // an argument without an opcode is none either
        else if (opcode == SOLVE_OP_BIT && (h >> 8) >= SOLVE_BIT_ARGS) { if (v < bad_arg) bad_arg = v; }
        else { state[g] = SOLVE_DEF; defined++; }
    }
    bad_gate = circ_block_min(bad_gate, red);
    bad_w4 = circ_block_min(bad_w4, red);
    bad_qo = circ_block_min(bad_qo, red);
    bad_ecc = circ_block_min(bad_ecc, red);
    bad_op = circ_block_min(bad_op, red);
    bad_arg = circ_block_min(bad_arg, red);
    uint32_t total;
    (void)circ_block_exclusive_scan(defined, sbuf, &total);
    if (threadIdx.x == 0) {
        if (bad_gate != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_GATE, bad_gate);
        if (bad_w4 != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_WIRE4, bad_w4);
        if (bad_qo != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_QO, bad_qo);
        if (bad_ecc != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_QECC, bad_ecc);
        if (bad_op != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_OP, bad_op);
        if (bad_arg != CIRC_NONE) atomicMin(flags + SOLVE_F_BAD_ARG, bad_arg);
        if (total) atomicAdd(flags + SOLVE_F_DEFINED, (unsigned long long)total);
    }
}

// One lane per gate, after the validation kernel on the same stream: the smallest gate with a non-zero hint_op that defines no variable.
__global__ void __launch_bounds__(CIRC_THREADS) solve_hint_stray_kernel(const uint32_t* __restrict__ hint_op, uint64_t n, const uint32_t* __restrict__ state,
                                                                        unsigned long long* __restrict__ first) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t base = (uint64_t)blockIdx.x * CIRC_TILE;
    unsigned long long bad = CIRC_NONE;
    for (uint32_t k = 0; k < CIRC_ITEMS; k++) {
        const uint64_t g = base + k * CIRC_THREADS + threadIdx.x;
        if (g < n && hint_op[g] && !(state[g] & SOLVE_DEF) && g < bad) bad = g;
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first, bad);
}

// The variant of solve_keys_kernel: a hint gate's live wires are its sources; the gate's class goes into its state word, and a gate
// with nothing pending into the first frontier of its class (one atomic per workgroup and class).
__global__ void __launch_bounds__(CIRC_THREADS) solve_hint_keys_kernel(const uint32_t* __restrict__ wire_vars, const uint32_t* __restrict__ def_gate,
                                                                       const Fr* __restrict__ sel, const uint32_t* __restrict__ hint_op, uint64_t n,
                                                                       uint32_t sentinel, uint32_t* __restrict__ state, uint32_t* __restrict__ keys,
                                                                       uint32_t* __restrict__ frontier, unsigned long long* __restrict__ frontier_count) {
    __shared__ uint32_t sbuf[CIRC_THREADS];
    __shared__ unsigned long long slot[SOLVE_CLASSES];
    const uint64_t j = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    uint32_t ready = 0, cls = 0;
    if (j < n) {
        uint32_t key[4] = {sentinel, sentinel, sentinel, sentinel};
        if (state[j] & SOLVE_DEF) {
            const uint32_t opcode = hint_op[j] & 0xFFu;
            uint32_t mask = 0, pending = 0;
            cls = solve_class_of(opcode);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                bool live;
                if (opcode) live = i == 2 || (i == 3 && opcode == SOLVE_OP_DIV);
                else live = !fp_is_zero(sel[i * n + j]) || !fp_is_zero(sel[(6 + i) * n + j]) || !fp_is_zero(sel[(4 + i / 2) * n + j]);
                if (!live) continue;
                mask |= 1u << i;
                const uint32_t v = wire_vars[i * n + j];
                if (def_gate[v] != SOLVE_NONE) { key[i] = v; pending++; }
            }
            state[j] = SOLVE_DEF | (cls << SOLVE_CLASS_SHIFT) | (mask << SOLVE_LIVE_SHIFT) | pending;
            ready = pending == 0;
        }
#pragma unroll
        for (int i = 0; i < 4; i++) keys[i * n + j] = key[i];
    }
    uint32_t at = 0;
    for (uint32_t c = 0; c < (uint32_t)SOLVE_CLASSES; c++) {
        const uint32_t mine = ready && cls == c;
        uint32_t total;
        const uint32_t a = circ_block_exclusive_scan(mine, sbuf, &total);
        if (mine) at = a;
        if (threadIdx.x == 0 && total) slot[c] = atomicAdd(frontier_count + c, (unsigned long long)total);
    }
    __syncthreads();
    if (ready) frontier[cls * n + slot[cls] + at] = (uint32_t)j;
}

// Store the value of gate g's variable and release its consumers: each into the next frontier of its own class (next: 3 lists of n).
__device__ __forceinline__ void solve_hint_release(const Fr& val, uint64_t g, const uint32_t* __restrict__ wire_vars, uint64_t n, Fr* __restrict__ witness,
                                                   const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint64_t count,
                                                   const uint32_t* __restrict__ start, uint32_t* __restrict__ state, uint32_t* __restrict__ next,
                                                   unsigned long long* __restrict__ next_count) {
    const uint32_t v = wire_vars[4 * n + g];
    witness[v] = val;
    for (uint64_t s = start[v]; s < count && sk[s] == v; s++) {
        const uint32_t cg = sv[s] & (uint32_t)(n - 1);
        const uint32_t old = atomicAdd(&state[cg], 0xFFFFFFFFu);
        if ((old & SOLVE_PENDING) == 1) {
            // one atomic per class with an address that is uniform over the wave, which the compiler folds into one atomic per wave as it does
            // in solve_level_kernel; on `next_count + c` with c per lane every lane's atomic went out alone (measured: 15 x the kernel's time)
            const uint32_t c = (old >> SOLVE_CLASS_SHIFT) & 3u;
            unsigned long long at0 = 0, at1 = 0, at2 = 0;                 // (an if / else chain is merged back into one atomic on a per-lane address)
            if (c == 0) at0 = atomicAdd(next_count, 1ull);
            if (c == 1) at1 = atomicAdd(next_count + 1, 1ull);
            if (c == 2) at2 = atomicAdd(next_count + 2, 1ull);
            next[c * n + (at0 | at1 | at2)] = cg;
        }
    }
}

// One level of class 0: solve_level_kernel's evaluation for an ordinary gate, a bit of the canonical residue for a BIT hint.
__global__ void __launch_bounds__(CIRC_THREADS) solve_hint_level_kernel(const uint32_t* __restrict__ frontier, uint64_t frontier_len,
                                                                        const uint32_t* __restrict__ wire_vars, const Fr* __restrict__ sel,
                                                                        const Fr* __restrict__ pub, const uint32_t* __restrict__ hint_op, uint64_t n,
                                                                        Fr* __restrict__ witness, const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv,
                                                                        uint64_t count, const uint32_t* __restrict__ start, uint32_t* __restrict__ state,
                                                                        uint32_t* __restrict__ next, unsigned long long* __restrict__ next_count, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= frontier_len) return;
    const uint64_t g = frontier[t];
    const uint32_t h = hint_op[g];
    const Fr zero = fp_zero<8>();
    Fr val;
    if (h) {                                                               // class 0 holds no other hint than BIT
        const Fr x = fp_from_mont(witness[wire_vars[2 * n + g]], P);
        const uint32_t k = h >> 8;                                         // < 256 (validated); the residue is < r, so bits above r's length are 0
        uint32_t word = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) word = (k >> 5) == i ? x.l[i] : word;          // a select per limb: no indexed register file access
        val = ((word >> (k & 31)) & 1u) ? fp_one(P) : zero;
    } else {
        const uint32_t live = state[g] >> SOLVE_LIVE_SHIFT;
        Fr a = zero, b = zero, c = zero, d = zero;
        if (live & 1) a = witness[wire_vars[g]];
        if (live & 2) b = witness[wire_vars[n + g]];
        if (live & 4) c = witness[wire_vars[2 * n + g]];
        if (live & 8) d = witness[wire_vars[3 * n + g]];
        val = circ_gate_inputs_value(a, b, c, d, sel, pub, n, g, P, nullptr);
        const Fr q_o = sel[10 * n + g], one = fp_one(P);
        if (!fp_eq(q_o, one)) val = fp_eq(q_o, fp_neg(one, P)) ? fp_neg(val, P) : fp_mul(val, fp_inv(q_o, P), P);
    }
    solve_hint_release(val, g, wire_vars, n, witness, sk, sv, count, start, state, next, next_count);
}

// x^e by a fixed window of SOLVE_POW_WINDOW bits, most significant digit first.  e is uniform (a kernel argument), so `digit`, `started` and the
// switch are scalar; the table stays in registers because every index into it is a constant.  0^e = 0 for e > 0.
__device__ __forceinline__ Fr solve_pow_fixed(const Fr& x, const SolveExponent& e, const FrParams& P) {
    static_assert(SOLVE_POW_WINDOW == 3, "the table and the switch below are written for 3 bits");
    const Fr x2 = fp_sqr(x, P), x3 = fp_mul(x2, x, P), x4 = fp_sqr(x2, P), x5 = fp_mul(x4, x, P), x6 = fp_sqr(x3, P), x7 = fp_mul(x6, x, P);
    Fr acc = fp_one(P);
    bool started = false;
    // the exponent as a shift register of 8 scalar words, every index a constant: bit 255 is zero and dropped, 85 digits of 3 bits follow
    uint32_t w[8];
#pragma unroll
    for (int j = 7; j > 0; j--) w[j] = (e.w[j] << 1) | (e.w[j - 1] >> 31);
    w[0] = e.w[0] << 1;
#pragma unroll 1
    for (int i = 0; i < 255 / SOLVE_POW_WINDOW; i++) {
        const uint32_t digit = w[7] >> (32 - SOLVE_POW_WINDOW);
#pragma unroll
        for (int j = 7; j > 0; j--) w[j] = (w[j] << SOLVE_POW_WINDOW) | (w[j - 1] >> (32 - SOLVE_POW_WINDOW));
        w[0] <<= SOLVE_POW_WINDOW;
        if (started) {
            acc = fp_sqr(acc, P);
            acc = fp_sqr(acc, P);
            acc = fp_sqr(acc, P);
        }
        if (!digit) continue;
        Fr m;
        switch (digit) {
            case 1: m = x; break;
            case 2: m = x2; break;
            case 3: m = x3; break;
            case 4: m = x4; break;
            case 5: m = x5; break;
            case 6: m = x6; break;
            default: m = x7; break;
        }
        acc = started ? fp_mul(acc, m, P) : m;
        started = true;
    }
    return acc;
}

// One level of class 1 (INV, DIV; e = r - 2) or class 2 (ROOT5; e = d): a lane per hint.
__global__ void __launch_bounds__(CIRC_THREADS) solve_pow_kernel(const uint32_t* __restrict__ frontier, uint64_t frontier_len, const uint32_t* __restrict__ wire_vars,
                                                                 const uint32_t* __restrict__ hint_op, uint64_t n, Fr* __restrict__ witness,
                                                                 const uint32_t* __restrict__ sk, const uint32_t* __restrict__ sv, uint64_t count,
                                                                 const uint32_t* __restrict__ start, uint32_t* __restrict__ state, uint32_t* __restrict__ next,
                                                                 unsigned long long* __restrict__ next_count, const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= frontier_len) return;
    const uint64_t g = frontier[t];
    const bool div = (hint_op[g] & 0xFFu) == SOLVE_OP_DIV;
    const Fr s0 = witness[wire_vars[2 * n + g]];
    Fr base = s0;                                                          // (a conditional of two lvalues would put s0 into scratch memory)
    if (div) base = witness[wire_vars[3 * n + g]];
    Fr val = solve_pow_fixed(base, e, P);
    if (div) val = fp_mul(s0, val, P);
    solve_hint_release(val, g, wire_vars, n, witness, sk, sv, count, start, state, next, next_count);
}

// The exponents on the host: r - 2, and d = 5^-1 mod (r - 1) = ((r - 1) k + 1) / 5 for the k in 1 .. 4 that makes the division exact.
// false: 5 divides r - 1 (neither of the two scalar fields).
static inline bool solve_exponents(const FrParams& P, SolveExponent* inv, SolveExponent* root5) {
    uint64_t br = 2;
    for (int i = 0; i < 8; i++) {
        const uint64_t t = (uint64_t)P.p[i] - br;
        inv->w[i] = (uint32_t)t;
        br = (t >> 32) & 1;
    }
    uint32_t m[8];                                                         // r - 1 (r is odd)
    for (int i = 0; i < 8; i++) m[i] = P.p[i];
    m[0] -= 1;
    for (uint32_t k = 1; k < 5; k++) {
        uint32_t num[9];
        uint64_t c = 1;
        for (int i = 0; i < 8; i++) {
            c += (uint64_t)m[i] * k;
            num[i] = (uint32_t)c;
            c >>= 32;
        }
        num[8] = (uint32_t)c;
        uint32_t q[9];
        uint64_t rem = 0;
        for (int i = 8; i >= 0; i--) {
            const uint64_t cur = (rem << 32) | num[i];
            q[i] = (uint32_t)(cur / 5);
            rem = cur % 5;
        }
        if (rem == 0 && q[8] == 0) {
            for (int i = 0; i < 8; i++) root5->w[i] = q[i];
            return true;
        }
    }
    return false;
}
