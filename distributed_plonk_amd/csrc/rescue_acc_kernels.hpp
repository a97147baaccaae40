// rescue_acc_kernels.hpp — the ternary Rescue accumulator on the device (included by synth.hip after rescue_kernels.hpp, whose
// rescue_permute_body every kernel here shares): jellyfish's sparse, append-only 3-ary Merkle tree, the structure the reference's test
// circuit proves memberships in (generate_circuit, dispatcher2.rs:1226-1271).
//
//     hash3(a, b, c) = permute((a, b, c, 0))[0]
//     level 0    c_0 = count nodes:               node_0[i]     = hash3(0, i, elems[i])               (the uid i as a field element)
//     level j+1  c_{j+1} = ceil(c_j / 3) nodes:   node_{j+1}[t] = hash3(x_0, x_1, x_2),   x_k = node_j[3t+k] if 3t+k < c_j else 0
// for j < height <= 40 (3^40 < 2^64).  An empty subtree is 0, not hash3(0, 0, 0), and no all-empty node is computed: 3t < c_j for every
// parent t.  The levels lie one after another in ONE buffer, leaves first: offset_0 = 0, offset_{j+1} = offset_j + c_j; the root is last.
//
// One lane per node, the state in registers, as in rescue_kernels.hpp, and what that header says about scratch memory holds here: a child
// beyond c_j must become zero WITHOUT a conditional between two Fr lvalues (the compiler would keep both in scratch and index them).  So
// the lane reads node_j[min(3t+k, c_j - 1)], an address that always exists, and ANDs the limbs with an all-ones or all-zero word.  The path
// kernel chooses its two siblings the same way: the choice is made between two INDICES, and one load follows.
//
// From the first level with one node the tree is a chain hash3(x, 0, 0) of up to 40 links, each needing the one before: ONE launch, one
// lane looping, instead of a launch per level.  A build is (levels with c_j > 1) + 2 launches: the leaves, the ragged levels, the chain.
#pragma once

constexpr unsigned RESCUE_ACC_MAX_HEIGHT = 40;

// the field element of an unsigned 64-bit integer, Montgomery
__device__ __forceinline__ Fr rescue_acc_fr_of_u64(uint64_t v, const FrParams& P) {
    Fr a = fp_zero<8>();
    a.l[0] = (uint32_t)v;
    a.l[1] = (uint32_t)(v >> 32);
    return fp_to_mont(a, P);
}

// level[i] for i < c, zero beyond; c >= 1
__device__ __forceinline__ Fr rescue_acc_node_or_zero(const Fr* __restrict__ level, uint64_t i, uint64_t c) {
    Fr x = level[i < c ? i : c - 1];
    const uint32_t keep = i < c ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int w = 0; w < 8; w++) x.l[w] &= keep;
    return x;
}

// node_0[i] = hash3(0, i, elems[i])
__global__ void __launch_bounds__(CIRC_THREADS) rescue_acc_leaf_kernel(const Fr* __restrict__ elems, uint64_t count, Fr* __restrict__ nodes, const Fr* __restrict__ prm,
                                                                       const SolveExponent e, const FrParams P) {
    const uint64_t i = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (i >= count) return;
    Fr s0 = fp_zero<8>(), s1 = rescue_acc_fr_of_u64(i, P), s2 = elems[i], s3 = fp_zero<8>();
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    nodes[i] = s0;
}

// One ragged level: the `parents` = ceil(c / 3) nodes of `above` from the c >= 1 nodes of `below` (two disjoint ranges of the buffer).
__global__ void __launch_bounds__(CIRC_THREADS) rescue_acc_level_kernel(const Fr* __restrict__ below, uint64_t c, Fr* __restrict__ above, uint64_t parents,
                                                                        const Fr* __restrict__ prm, const SolveExponent e, const FrParams P) {
    const uint64_t t = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= parents) return;
    Fr s0 = below[3 * t], s1 = rescue_acc_node_or_zero(below, 3 * t + 1, c), s2 = rescue_acc_node_or_zero(below, 3 * t + 2, c), s3 = fp_zero<8>();
    rescue_permute_body(s0, s1, s2, s3, prm, e, P);
    above[t] = s0;
}

// The chain above a level of one node: chain[k + 1] = hash3(chain[k], 0, 0), k < steps; chain[0] is filled.  One lane: `lanes` is 1.
// It is an ARGUMENT so that the lane index stays unknown to the compiler.  Written with a literal lane 0, every value of the kernel is
// provably uniform and the whole chain moves to the scalar unit, which has no 64-bit multiply-add: 46 k scalar instructions and 438 SGPRs
// parked in VGPR lanes, measured at 23 ms per link (profiles/rescue_probe.txt).  Indexed by t < lanes it is the vector code of the level kernel.
__global__ void __launch_bounds__(CIRC_THREADS) rescue_acc_tail_kernel(Fr* __restrict__ chain, uint32_t steps, uint32_t lanes, const Fr* __restrict__ prm,
                                                                       const SolveExponent e, const FrParams P) {
    const uint32_t t = blockIdx.x * CIRC_THREADS + threadIdx.x;
    if (t >= lanes) return;
    Fr s0 = chain[t];
#pragma unroll 1
    for (uint32_t k = 0; k < steps; k++) {
        Fr s1 = fp_zero<8>(), s2 = fp_zero<8>(), s3 = fp_zero<8>();
        rescue_permute_body(s0, s1, s2, s3, prm, e, P);
        chain[k + 1 + t] = s0;
    }
}

// The membership witnesses of m uids in the layout builder-side membership_circuit takes its inputs in: out is row-major, (2 + 4 height) rows
// of m Fr — row 0 the uids, row 1 their elems, rows 2 + 4j .. 5 + 4j the sib1, sib2, is_left, is_right of level j.  One lane per (k, j), lane
// index j * m + k.  At level j the node on the path is number q = uid / 3^j of the level, its position in its group of three q mod 3, the group
// starts at g = q - q mod 3; sib1, sib2 are the two other members in ascending position, zero beyond c_j.  A uid >= count writes nothing and
// reports the smallest such k.
__global__ void __launch_bounds__(CIRC_THREADS) rescue_acc_paths_kernel(const Fr* __restrict__ nodes, uint64_t count, uint32_t height, const Fr* __restrict__ elems,
                                                                        const uint64_t* __restrict__ uids, uint64_t m, Fr* __restrict__ out,
                                                                        unsigned long long* __restrict__ first_bad, const FrParams P) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t lane = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    unsigned long long bad = CIRC_NONE;
    if (lane < m * height) {
        const uint32_t j = (uint32_t)(lane / m);
        const uint64_t k = lane % m;
        const uint64_t uid = uids[k];
        if (uid >= count) bad = k;
        else {
            uint64_t off = 0, c = count, q = uid;             // level j: its offset, its node count, the path's node in it
            for (uint32_t l = 0; l < j; l++) { off += c; c = (c + 2) / 3; q /= 3; }
            const uint32_t pos = (uint32_t)(q % 3);
            const uint64_t g = q - pos;
            const Fr* level = nodes + off;
            Fr* row = out + (2 + 4 * (uint64_t)j) * m + k;
            row[0] = rescue_acc_node_or_zero(level, g + (pos == 0 ? 1 : 0), c);
            row[m] = rescue_acc_node_or_zero(level, g + (pos == 2 ? 1 : 2), c);
            const Fr one = fp_one(P);
            Fr is_left = one, is_right = one;
            const uint32_t left = pos == 0 ? 0xFFFFFFFFu : 0u, right = pos == 2 ? 0xFFFFFFFFu : 0u;
#pragma unroll
            for (int w = 0; w < 8; w++) { is_left.l[w] &= left; is_right.l[w] &= right; }
            row[2 * m] = is_left;
            row[3 * m] = is_right;
            if (j == 0) {
                out[k] = rescue_acc_fr_of_u64(uid, P);
                out[m + k] = elems[uid];
            }
        }
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first_bad, bad);
}

// witness[input_vars[k]] = inputs[k], k < num_inputs: the given variables of a circuit from values already on the device.  An id >= num_vars
// writes nothing and reports the smallest such k.
__global__ void __launch_bounds__(CIRC_THREADS) circuit_scatter_inputs_kernel(const uint32_t* __restrict__ input_vars, uint64_t num_inputs, const Fr* __restrict__ inputs,
                                                                              Fr* __restrict__ witness, uint64_t num_vars, unsigned long long* __restrict__ first_bad) {
    __shared__ unsigned long long red[CIRC_THREADS];
    const uint64_t k = (uint64_t)blockIdx.x * CIRC_THREADS + threadIdx.x;
    unsigned long long bad = CIRC_NONE;
    if (k < num_inputs) {
        const uint32_t v = input_vars[k];
        if (v < num_vars) witness[v] = inputs[k];
        else bad = k;
    }
    bad = circ_block_min(bad, red);
    if (threadIdx.x == 0 && bad != CIRC_NONE) atomicMin(first_bad, bad);
}

static inline int rescue_acc_grid(uint64_t lanes, const char* who, uint32_t* grid) {
    const uint64_t blocks = (lanes + CIRC_THREADS - 1) / CIRC_THREADS;
    if (blocks > 0x7FFFFFFFull) return plonk_fail(PLONK_ERR_ARG, "%s: %llu lanes exceed one launch (2^31 - 1 workgroups of %u)", who, (unsigned long long)lanes, CIRC_THREADS);
    *grid = (uint32_t)blocks;
    return PLONK_OK;
}

// 1 <= height <= 40, 1 <= count <= 3^height; nodes: sum c_j Fr, every one written.  Enqueued on `stream`, not synchronised.
int rescue_acc_build_run(int curve, const Fr* d_params, const Fr* d_elems, uint64_t count, unsigned height, Fr* d_nodes, hipStream_t stream, const char* who) {
    SolveExponent e;
    int rc = rescue_exponent(curve, &e, who);
    if (rc) return rc;
    uint32_t grid;
    if ((rc = rescue_acc_grid(count, who, &grid))) return rc;
    ProfScope ps("rescue_acc_build", stream);
    hipLaunchKernelGGL(rescue_acc_leaf_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_elems, count, d_nodes, d_params, e, fr_params(curve));
    if ((rc = circ_launch_status("rescue_acc_leaf"))) return rc;
    uint64_t off = 0, c = count;
    unsigned j = 0;
    for (; j < height && c > 1; j++) {
        const uint64_t parents = (c + 2) / 3;
        hipLaunchKernelGGL(rescue_acc_level_kernel, dim3(circ_grid_of(parents, CIRC_THREADS)), dim3(CIRC_THREADS), 0, stream, (const Fr*)(d_nodes + off), c, d_nodes + off + c,
                           parents, d_params, e, fr_params(curve));
        if ((rc = circ_launch_status("rescue_acc_level"))) return rc;
        off += c;
        c = parents;
    }
    if (j < height) {                                         // c == 1 at level j: height - j links of the chain
        hipLaunchKernelGGL(rescue_acc_tail_kernel, dim3(1), dim3(1), 0, stream, d_nodes + off, (uint32_t)(height - j), 1u, d_params, e, fr_params(curve));
        if ((rc = circ_launch_status("rescue_acc_tail"))) return rc;
    }
    return PLONK_OK;
}

// m >= 1 uids; out: (2 + 4 height) * m Fr.  scratch: 8 bytes.  Synchronises (reads the uid check's verdict).
int rescue_acc_paths_run(int curve, const Fr* d_nodes, uint64_t count, unsigned height, const Fr* d_elems, const uint64_t* d_uids, uint64_t m, Fr* d_out, void* scratch,
                         hipStream_t stream, const char* who) {
    unsigned long long* d_flag = (unsigned long long*)scratch;
    uint32_t grid;
    int rc = rescue_acc_grid(m * height, who, &grid);
    if (rc) return rc;
    {
        ProfScope ps("rescue_acc_paths", stream);
        HIP_TRY(hipMemsetAsync(d_flag, 0xFF, sizeof(*d_flag), stream));
        hipLaunchKernelGGL(rescue_acc_paths_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_nodes, count, (uint32_t)height, d_elems, d_uids, m, d_out, d_flag,
                           fr_params(curve));
        if ((rc = circ_launch_status("rescue_acc_paths"))) return rc;
    }
    unsigned long long bad = CIRC_NONE;
    if ((rc = circ_read_flag(d_flag, &bad, stream))) return rc;
    if (bad != CIRC_NONE) return plonk_fail(PLONK_ERR_ARG, "%s: d_uids[%llu] is >= count = %llu", who, bad, (unsigned long long)count);
    return PLONK_OK;
}

// num_inputs >= 1.  scratch: 8 bytes.  Synchronises (reads the id check's verdict).
int circuit_scatter_inputs_run(const uint32_t* d_input_vars, size_t num_inputs, const Fr* d_inputs, Fr* d_witness, size_t num_vars, void* scratch, hipStream_t stream,
                               const char* who) {
    unsigned long long* d_flag = (unsigned long long*)scratch;
    uint32_t grid;
    int rc = rescue_acc_grid(num_inputs, who, &grid);
    if (rc) return rc;
    {
        ProfScope ps("circuit_scatter_inputs", stream);
        HIP_TRY(hipMemsetAsync(d_flag, 0xFF, sizeof(*d_flag), stream));
        hipLaunchKernelGGL(circuit_scatter_inputs_kernel, dim3(grid), dim3(CIRC_THREADS), 0, stream, d_input_vars, (uint64_t)num_inputs, d_inputs, d_witness,
                           (uint64_t)num_vars, d_flag);
        if ((rc = circ_launch_status("circuit_scatter_inputs"))) return rc;
    }
    unsigned long long bad = CIRC_NONE;
    if ((rc = circ_read_flag(d_flag, &bad, stream))) return rc;
    if (bad != CIRC_NONE) return plonk_fail(PLONK_ERR_ARG, "%s: d_input_vars[%llu] is >= num_vars = %zu", who, bad, num_vars);
    return PLONK_OK;
}
