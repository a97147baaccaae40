/* plonk_hip.h — C ABI of the MI355X-native MSM + NTT hot path (libplonk_hip.so).
 *
 * Drop-in boundary for MengLing-L/distributed_plonk's worker: one entry point per Cap'n Proto method
 * of `interface PlonkSlave` @0..@6 and `interface PlonkPeer` @0 (reference
 * src/hello_world.capnp:16-24,49-50; server src/worker.rs:125-439; clients src/dispatcher.rs:50-175,
 * src/dispatcher2.rs:961-1086), plus the three third-party operator calls the worker makes
 * (VariableBaseMSM::multi_scalar_mul, Radix2EvaluationDomain::{fft,ifft}_in_place, Fr::pow loops), and — further down — the
 * O(n) loops the dispatcher runs itself in `Prover::prove` (src/dispatcher2.rs:329-344, 435-504, 545-688: SURVEY.md §8f) as
 * device-resident calls, with the coset-class primitives a multi-rank prover is built from.
 * Plain pointers and sizes only; the caller owns every host buffer; the library owns device memory
 * inside the context.  INTEGRATION.md shows the Rust `extern "C"` block a maintainer would add.
 *
 * Byte layouts are the reference's raw memory layouts (src/utils.rs:27-43):
 *   Fr            4 x u64 little-endian, Montgomery form (R = 2^256), fully reduced
 *   MSM scalar    4 x u64 little-endian, canonical (`into_repr()`)
 *   Fq            4 x u64 (BN254) / 6 x u64 (BLS12-381), Montgomery
 *   G1 projective X || Y || Z (Jacobian, Montgomery), infinity = Z == 0
 *   G1 affine     PLONK_BASES_XY: x || y, infinity encoded as x = y = 0 (not on either curve)
 *                 PLONK_BASES_ARK: arkworks' in-memory `GroupAffine {x, y, infinity: bool}` with the
 *                 struct padded to 8 bytes (72 B BN254 / 104 B BLS12-381) — what `init` puts on the wire
 *
 * Every function returns 0 (PLONK_OK) or a negative error code; nothing throws across the boundary.
 * The reference panics (`.unwrap()`) on malformed input (worker.rs:131,253,303); here ranges, sizes
 * and domain two-adicity are validated and reported.  A context is bound to one GPU and is not
 * thread-safe (the reference worker is a single-threaded tokio LocalSet, worker.rs:441-448); DIFFERENT contexts may be
 * driven from different host threads concurrently (two contexts on one GPU overlap independent commitments).
 */
#ifndef PLONK_HIP_H
#define PLONK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct plonk_ctx plonk_ctx;

enum { PLONK_BN254 = 0, PLONK_BLS12_381 = 1 };
enum { PLONK_BASES_XY = 0, PLONK_BASES_ARK = 1 };
enum {
    PLONK_OK = 0,
    PLONK_ERR_ARG = -1,       /* bad argument (range, size, null) */
    PLONK_ERR_DOMAIN = -2,    /* DomainCreationError: log2(size) > two-adicity, or not a power of two */
    PLONK_ERR_HIP = -3,       /* HIP runtime error (no device, out of memory, launch failure) */
    PLONK_ERR_STATE = -4,     /* call order violated (unknown task id, rows missing, ...) */
    PLONK_ERR_EXCHANGE = -5   /* the exchange callback failed */
};

/* src/utils.rs:3-8 / hello_world.capnp:8-13 */
typedef struct { uint64_t row_start, row_end, col_start, col_end; } plonk_fft_workload;
/* src/utils.rs:21-25 / hello_world.capnp:3-6 */
typedef struct { uint64_t start, end; } plonk_msm_workload;

/* Worker<->worker transport for fft2Prepare (replaces the per-exchange TCP + Cap'n Proto
 * connections of worker.rs:303-338).  Called once per fft2_prepare with device pointers:
 * `send` holds n_ranks blocks of `bytes_per_peer` bytes (block p goes to rank p), `recv` receives
 * n_ranks blocks (block p came from rank p).  `stream` is the hipStream_t the buffers are ordered on.
 * An RCCL all-to-all (ncclSend/ncclRecv group, or torch.distributed.all_to_all_single) implements it.
 * Return 0 on success. */
typedef int (*plonk_exchange_fn)(void* user, const void* send, void* recv, size_t bytes_per_peer,
                                 int n_ranks, void* stream);

/* ---- in-library transport: RCCL over xGMI (replaces the worker<->worker TCP + Cap'n Proto links of worker.rs:280-345,412-438
 * and the `result: Data` replies the dispatcher adds up, dispatcher.rs:236-238).  One process per GPU.  Rank 0 obtains an id with
 * plonk_comm_unique_id and ships its 128 bytes to the other ranks out of band (the reference's config/network.json + TCP play
 * that role); every rank then calls plonk_comm_init — a collective: it returns when all `world` ranks have joined.  With a
 * communicator attached, plonk_fft2_prepare(ctx, id, NULL, NULL) performs the all-to-all itself (grouped ncclSend/ncclRecv on the
 * context's stream); the callback form stays for tests and for hosts that bring their own transport.  Two contexts of one
 * process (two streams) need two communicators, created in the same order on every rank, and every rank must issue its
 * collectives in the same order.  The library chains every collective it issues on a GPU behind the previous one (an event wait on
 * the issuing stream), whatever communicator it belongs to: collectives of different communicators are never in flight together
 * (RCCL gives no progress guarantee for that), they still overlap the other contexts' compute. */
#define PLONK_COMM_ID_BYTES 128
int plonk_comm_unique_id(void* out_id);
int plonk_comm_init(plonk_ctx* ctx, const void* id, int rank, int world);
int plonk_comm_destroy(plonk_ctx* ctx);
/* rank / world as RCCL reports them (ncclCommUserRank / ncclCommCount), and the RCCL version code (ncclGetVersion) */
int plonk_comm_info(plonk_ctx* ctx, int* rank, int* world, int* rccl_version);
/* plonk_exchange_fn backed by the context's communicator: pass as `exchange` with user = ctx (what a NULL callback selects) */
int plonk_exchange_rccl(void* user, const void* send, void* recv, size_t bytes_per_peer, int n_ranks, void* stream);
/* diagnostic plonk_exchange_fn (bench.py --simulate-ranks: one rank's share of an n_ranks job on ONE GPU): blocks 1 .. n_ranks-1 of
 * `send` are copied to the same blocks of `recv` on `stream`, device to device — the bytes a real exchange would move, through the
 * same buffers, at HBM instead of xGMI speed.  Results are meaningless; `user` is ignored. */
int plonk_exchange_standin(void* user, const void* send, void* recv, size_t bytes_per_peer, int n_ranks, void* stream);
/* device buffers, ordered on the context's stream, not synchronised: block p of d_send -> rank p / every rank's d_send -> block
 * `rank` of everybody's d_recv.  The two data-path collectives of the coset-class prover.
 * THREAD RULE (all collectives of this library, plonk_fft2_prepare's exchange included): the collectives of one DEVICE must come from
 * ONE host thread — the first that issues one on that device owns it until the device's last communicator is destroyed; a call from
 * another thread returns PLONK_ERR_STATE instead of risking a cross-rank deadlock (two threads cannot promise the same issue order on
 * every rank).  A host whose runtime migrates one logical task between OS threads sets the environment variable
 * PLONK_COMM_ANY_THREAD=1 and serialises its collectives itself.
 * ORDER CHECK (diagnostic): with PLONK_COMM_CHECK_ORDER=1 in every rank's environment (or plonk_set_option(ctx, "comm_check_order", 1) on
 * every rank: the switch is process-wide) each collective is preceded by an all-gather of a 24-byte tag — the communicator's ordinal among
 * the device's communicators in creation order, the kind of collective, its byte count, the device's collective count — over the device's
 * FIRST communicator, and every rank returns PLONK_ERR_STATE when the tags differ: ranks that enter their collectives in different orders
 * (two tasks finished in different orders, a different kind or size on one rank) get an error naming both sides instead of a silent
 * deadlock inside RCCL.  Costs a host round trip per collective: for the first runs on a new machine, not for production. */
int plonk_comm_alltoall_dev(plonk_ctx* ctx, const void* d_send, void* d_recv, size_t bytes_per_peer);
int plonk_comm_allgather_dev(plonk_ctx* ctx, const void* d_send, void* d_recv, size_t bytes);
/* host buffers (partial commitment points, 96 / 144 B each): out receives world * bytes.  Synchronises. */
int plonk_comm_allgather_host(plonk_ctx* ctx, const void* in, size_t bytes, void* out);

/* ---- lifetime ------------------------------------------------------------------------------- */
/* State::new, worker.rs:455-472. */
int plonk_create(plonk_ctx** out, int device, int curve);
void plonk_destroy(plonk_ctx* ctx);
const char* plonk_last_error(void);
/* HIP stream all work of this context is ordered on (for callers that share device buffers). */
void* plonk_stream(plonk_ctx* ctx);
int plonk_sync(plonk_ctx* ctx);

/* ---- PlonkSlave @0 init — worker.rs:126-157, client dispatcher.rs:50-68 ----------------------
 * Stores the SRS bases on the device and fixes the two evaluation domains (n and the quotient
 * domain m); either size may be 0 (dispatcher.rs:215 passes 0,0 for the MSM test).
 * The bases are CHECKED: every one must be a point of the curve (coordinates below the modulus, y^2 = x^3 + b), the infinity this
 * layout encodes ((0, 0) in PLONK_BASES_XY; any x, y with the flag byte = 1 in PLONK_BASES_ARK), and an ark flag byte must be 0 or 1 —
 * else PLONK_ERR_ARG naming the first offending index, and the context is left WITHOUT bases.  The reference reinterprets
 * `[G1Affine]` memory (utils.rs:27-43, worker.rs:136-141) and `GroupAffine {x, y, infinity}` is a default-repr Rust struct whose field
 * order is not guaranteed: swapped coordinates, a shifted stride or different padding fail here instead of yielding commitments that are
 * garbage with PLONK_OK.  ~1 ms per 2^24 points; plonk_set_option(ctx, "check_bases", 0) skips it. */
int plonk_init(plonk_ctx* ctx, const void* bases, size_t n_bases, int base_layout,
               size_t domain_size, size_t quot_domain_size);

/* ---- PlonkSlave @1 varMsm — worker.rs:159-185, client dispatcher.rs:70-92 --------------------
 * out_jacobian = sum_i scalars[i] * bases[start + i], i < min(end - start, n_scalars). */
int plonk_var_msm(plonk_ctx* ctx, const plonk_msm_workload* workload, const uint64_t* scalars,
                  size_t n_scalars, uint64_t* out_jacobian);

/* ---- PlonkSlave @2 fftInit — worker.rs:187-233 ----------------------------------------------- */
int plonk_fft_init(plonk_ctx* ctx, uint64_t id, const plonk_fft_workload* workloads, size_t n_workloads,
                   size_t me, int is_quot, int is_inv, int is_coset);
/* ---- PlonkSlave @3 fft1 — worker.rs:235-278 (helper :66-94).  One decimated row of c elements;
 * i is the LOCAL row index (global row = i + workloads[me].row_start, worker.rs:267). */
int plonk_fft1(plonk_ctx* ctx, uint64_t id, uint64_t i, const uint64_t* v, size_t len);
/* ---- PlonkSlave @4 fft2Prepare + PlonkPeer @0 fftExchange — worker.rs:280-345, 412-438 --------
 * Row pass on every local row, then the all-to-all block transpose.  Collective: every rank calls
 * it for the same id.  Transport precedence: a non-NULL `exchange` callback; else the context's RCCL communicator (plonk_comm_init)
 * when the task has exactly as many workloads as the communicator has ranks; a single-workload task stays local (nothing to
 * exchange) whether or not the context joined a communicator; anything else is PLONK_ERR_ARG. */
int plonk_fft2_prepare(plonk_ctx* ctx, uint64_t id, plonk_exchange_fn exchange, void* user);
/* ---- PlonkSlave @5 fft2 — worker.rs:347-381 (helper :96-115).  out_cols receives num_cols
 * columns of r elements each (column-major blobs, as the reply of worker.rs:366-376); the task is
 * removed (worker.rs:378). */
int plonk_fft2(plonk_ctx* ctx, uint64_t id, uint64_t* out_cols);
/* ---- PlonkSlave @6 round1 — worker.rs:383-408.  evals: n = domain_size Fr; blinders: the two
 * coefficients (b0, b1) of the degree-1 blinding polynomial the reference draws from thread_rng
 * (worker.rs:400), supplied explicitly so results are reproducible.  The blinded polynomial
 * (n + 2 coefficients) stays resident (`state.wire`, worker.rs:58); its commitment is returned. */
int plonk_round1(plonk_ctx* ctx, const uint64_t* evals, size_t n, const uint64_t* blinders,
                 uint64_t* out_commit_jacobian);
int plonk_get_wire(plonk_ctx* ctx, uint64_t* out_coeffs, size_t n_coeffs);

/* ---- third-party operator boundary (ark-poly / ark-ec calls the worker makes) ----------------
 * Whole-vector transform, dispatcher.rs:594,632,667 / dispatcher2.rs:507: host buffer of n = 2^k
 * Fr transformed in place ({fft,ifft,coset_fft,coset_ifft}_in_place). */
int plonk_ntt(plonk_ctx* ctx, uint64_t* v, size_t n, int is_inv, int is_coset);
/* commit_polynomial, worker.rs:117-123 / dispatcher2.rs:835-893: Montgomery coefficients ->
 * into_repr -> zero-pad to the SRS -> MSM.  Host buffers. */
int plonk_commit(plonk_ctx* ctx, const uint64_t* coeffs_mont, size_t n_coeffs, uint64_t* out_jacobian);
/* G1Projective addition / normalisation used by the dispatcher's reduce (dispatcher.rs:236-238) and
 * `Commitment(commitment.into())` (dispatcher2.rs:892).  Host-side, tiny. */
int plonk_g1_add(int curve, const uint64_t* a_jac, const uint64_t* b_jac, uint64_t* out_jac);
int plonk_g1_to_affine(int curve, const uint64_t* jac, uint64_t* out_xy, int* is_infinity);
/* Keccak-f[1600] in place on a 200-byte state (lane (x, y) at byte 8 * (x + 5 y), little-endian): the permutation under merlin / STROBE-128,
 * i.e. under the reference's Fiat-Shamir transcript (dispatcher2.rs:44-154; merlin 3.0.0, Cargo.toml:40).  Host-side, tiny: a host whose language
 * has no fast Keccak (the Python mirror) runs its transcript's ~25 permutations per proof through this. */
int plonk_keccak_f1600(uint8_t* state200);
/* ip_transpose, transpose.rs:413 (rows x cols -> cols x rows of Fr), host buffer. */
int plonk_transpose(plonk_ctx* ctx, uint64_t* v, size_t rows, size_t cols);

/* ---- device-resident variants (no host staging; pointers are HBM addresses on ctx's device) ---
 * d_in is used as workspace and destroyed unless d_in == d_out (then an internal scratch is used). */
int plonk_ntt_dev(plonk_ctx* ctx, void* d_in, void* d_out, size_t n, int is_inv, int is_coset);
int plonk_msm_dev(plonk_ctx* ctx, size_t start, size_t end, const void* d_scalars, uint64_t* out_jacobian);
int plonk_commit_dev(plonk_ctx* ctx, const void* d_coeffs_mont, size_t n_coeffs, uint64_t* out_jacobian);
/* The shard [start, start + count) of commit_polynomial (dispatcher2.rs:870-890 hands each worker such a range): d_coeffs_mont points
 * at coefficient `start`; out = sum_{i < count} into_repr(coeff[start + i]) * bases[start + i].  The shards' points add up to the
 * commitment. */
int plonk_commit_range_dev(plonk_ctx* ctx, const void* d_coeffs_mont, size_t start, size_t count, uint64_t* out_jacobian);
/* k commit_polynomial calls against the same key in ONE set of kernel launches — the independent commitments of a prover round
 * (dispatcher2.rs:313-321: five wire polynomials; :519-531: five quotient parts; :690-697: two opening proofs).  Polynomial i has
 * n_coeffs[i] Montgomery coefficients at d_coeffs_mont[i] (point at coefficient `start`), paired with bases [start, start + n_coeffs[i]);
 * out_jacobians receives k Jacobian triples.  Same points as k calls of plonk_commit_range_dev(.., start, n_coeffs[i], ..): the scalar
 * vectors become extra windows of one Pippenger problem (one sort, one bucket accumulation, one reduction), which removes the
 * per-MSM launch gaps, wave tails and host round trips that bound small MSMs. */
int plonk_commit_many_dev(plonk_ctx* ctx, size_t k, const void* const* d_coeffs_mont, const size_t* n_coeffs, size_t start, uint64_t* out_jacobians);
/* All local rows at once, row-major [num_rows][c] in HBM (replaces num_rows fft1 calls).  d_rows is CONSUMED: the buffer must stay
 * alive until plonk_fft2_prepare returns, which runs the row pass with d_rows as its inter-pass workspace (c > 2^9) and leaves
 * garbage in it — like plonk_ntt_dev's d_in. */
int plonk_fft1_dev(plonk_ctx* ctx, uint64_t id, void* d_rows);
/* The same for the rows of a ZERO-PADDED vector (the reference pads n + 2 / n + 3 coefficients to the 8n-point domain before it
 * decimates, dispatcher2.rs:746, 754): d_rows is [num_rows][row_len] — the leading row_len coefficients of every decimated row, the
 * rest of each row being zero by construction and never materialised (row b of the padded 8n vector has c/8 leading entries, one
 * more for b < 3).  Forward transforms only; the row pass then runs as 2^k independent (c/2^k)-point transforms per row.  The
 * buffer is NOT modified and must stay alive until plonk_fft2_prepare returns. */
int plonk_fft1_dev_compact(plonk_ctx* ctx, uint64_t id, const void* d_rows, size_t row_len);
/* Result of fft2 left in HBM.  layout 0: [num_cols][r] (the reference's reply); layout 1:
 * [r][num_cols] (natural order restricted to this rank's columns: element (j, i) = X[(i + col_start) + j*c]). */
int plonk_fft2_dev(plonk_ctx* ctx, uint64_t id, void* d_out, int layout);
int plonk_transpose_dev(plonk_ctx* ctx, const void* d_in, void* d_out, size_t rows, size_t cols);

/* ---- next row: quotient polynomial coset evaluations — dispatcher2.rs:362-504 --------------
 * Device pointers to the m = quot_domain_size coset evaluations the prover obtained from its 25 coset-FFTs
 * (dispatcher2.rs:382-432), in the selector order of :443-456: q_lc[0..3], q_mul[0..1], q_hash[0..3], q_o, q_c, q_ecc. */
typedef struct {
    const void* selectors[13];
    const void* sigmas[5];
    const void* wires[5];
    const void* perm;        /* permutation product polynomial z */
    const void* pub_input;
} plonk_quotient_inputs;
/* d_out[i] = 1/Z_H(x_i) * (gate(x_i) + alpha * perm(x_i)) + alpha^2/n * (z(x_i) - 1)/(x_i - 1), x_i = g * w_m^i, exactly as
 * the loop at dispatcher2.rs:435-504.  alpha, beta, gamma: transcript challenges; k: vk.k[0..5] — all Fr, Montgomery,
 * host pointers.  Uses the domains fixed by plonk_init.  The quotient's coefficient form is then
 * plonk_ntt_dev(d_out, ..., m, is_inv = 1, is_coset = 1) (dispatcher2.rs:507).
 * NO ALIASING: d_out must not overlap any input vector (a lane reads `perm` at its own index and at the shifted index of z(wX), and the
 * split formulation writes d_out before it reads wires, sigmas and perm) — an overlapping call is PLONK_ERR_ARG. */
int plonk_quotient_evals_dev(plonk_ctx* ctx, const plonk_quotient_inputs* in, const uint64_t* alpha, const uint64_t* beta,
                             const uint64_t* gamma, const uint64_t* k, void* d_out);

/* The same on ONE coset class: all inputs hold the m/G evaluations at the points x_j, j = class_offset + class_stride * k
 * (plonk_coset_eval_dev with shift g * w_m^class_offset), d_out[k] is the quotient evaluation at that point.  G = class_stride
 * must be a power of two dividing m/n, so z(w x) — point j + m/n — stays inside the class: rank-local with no halo. */
int plonk_quotient_evals_class_dev(plonk_ctx* ctx, const plonk_quotient_inputs* in, const uint64_t* alpha, const uint64_t* beta,
                                   const uint64_t* gamma, const uint64_t* k, uint32_t class_stride, uint32_t class_offset, void* d_out);

/* ---- next row: permutation grand product — dispatcher2.rs:329-344 ---------------------------
 * d_out[0] = 1, d_out[j+1] = d_out[j] * prod_i (w_i[j] + gamma + beta*id[i*n+j]) / prod_i (w_i[j] + gamma + beta*id[perm[i*n+j]]),
 * j < n-1: the `product_vec` the reference builds gate by gate on the host.  d_wires[i]: n wire values
 * witness[wire_variables[i][j]] (Fr, Montgomery); d_id_perm: the 5n values of extended_id_permutation; d_perm_idx: 5n u64,
 * perm_i * n + perm_j of wire_permutation[i*n+j]; beta, gamma: host.  PLONK_ERR_ARG if an index is >= 5n or a denominator
 * is zero (the reference panics: Fp division unwraps the inverse).  Synchronises the context's stream. */
int plonk_perm_product_dev(plonk_ctx* ctx, const void* const d_wires[5], const void* d_id_perm, const void* d_perm_idx,
                           const uint64_t* beta, const uint64_t* gamma, size_t n, void* d_out);
/* A worker's slice of that vector, up to the product of the gates before it: d_out[t] = prod over gates first <= j < first + t of the
 * same ratio, t < count (first + count <= n; gate n-1 contributes 1 as in the reference's loop, which stops at n-2).  With
 * count = slice + 1 the last value is the slice's total: G workers exchange those 32-byte totals, and worker s multiplies its slice by the
 * totals of the workers before it (class_prover.py) — the reference's serial dispatcher loop distributed like its FFTs
 * (dispatcher2.rs:329-344 next to :732-787).  The pointers are to the WHOLE vectors (n / 5n entries).  Same errors; synchronises. */
int plonk_perm_product_range_dev(plonk_ctx* ctx, const void* const d_wires[5], const void* d_id_perm, const void* d_perm_idx,
                                 const uint64_t* beta, const uint64_t* gamma, size_t n, size_t first, size_t count, void* d_out);

/* ---- next row: round 4/5 polynomial operations — dispatcher2.rs:545-555,566-633,646-688 ------
 * Coefficient vectors are device pointers to Fr (Montgomery); scalars (points, coefficients, blinders) are host Fr. */
/* out = poly(point): DensePolynomial::evaluate (:545-555).  len < 2^30.  Synchronises. */
int plonk_poly_eval_dev(plonk_ctx* ctx, const void* d_poly, size_t len, const uint64_t* point, uint64_t* out);
/* d_out[i] = sum_{t<k} coeffs[t] * d_polys[t][i] over the terms with i < lens[t], i < out_len (k <= 32): the scalar*poly sums
 * that build lin_poly and batch_poly (:566-633,646-649).  d_out must not alias an input. */
int plonk_poly_lincomb_dev(plonk_ctx* ctx, size_t k, const void* const* d_polys, const size_t* lens, const uint64_t* coeffs,
                           void* d_out, size_t out_len);
/* d_out[0..len-1) = quotient of poly / (X - point), remainder dropped: the synthetic-division loops of :651-666,672-688. */
int plonk_poly_div_linear_dev(plonk_ctx* ctx, const void* d_poly, size_t len, const uint64_t* point, void* d_out);
/* y_j = f(z_j) and q_j = (f - y_j)/(X - z_j) for m device-resident points, one set of launches.
 * d_values: m Fr.  d_quotients: NULL (values only) or m rows of q_stride Fr (q_stride >= len - 1), row j = q_j.
 * d_status: m u32, 0 ok, | 8 point not canonical.  len < 2^30, m <= 2^16.  Enqueued on the context's stream, not synchronised.
 * Points, coefficients and results are Montgomery Fr.  A point >= the modulus gets the value 0 and a row of zeros; the words of a row beyond
 * len - 1 are left alone.  len == 0: every value 0; len == 1: the values f_0, nothing written to d_quotients; m == 0: no launch.  An output
 * that overlaps d_poly (or d_points) is PLONK_ERR_ARG.  No point is special: 0 is opened by the same launches as any other (csrc/kzg_kernels.hpp). */
int plonk_poly_open_many_dev(plonk_ctx* ctx, const void* d_poly, size_t len, const void* d_points, size_t m,
                             void* d_values, void* d_quotients, size_t q_stride, void* d_status);
/* The shape of plonk_poly_open_many_dev's kernels: coefficients per tile, lanes of the per-point top scan (tests follow them). */
size_t plonk_poly_open_many_tile(void);
size_t plonk_poly_open_many_top_lanes(void);
/* *degree = index of the highest non-zero coefficient, -1 for the zero polynomial: DensePolynomial::degree() after the
 * trimming of from_coefficients_vec — the WrongQuotientPolyDegree check of :511-518 without a host copy.  Synchronises. */
int plonk_poly_degree_dev(plonk_ctx* ctx, const void* d_poly, size_t len, int64_t* degree);
/* d_poly (n + k coefficients, the top k already valid, normally zero) += (sum_{i<k} blinders[i] X^i) * (X^n - 1):
 * DensePolynomial::rand(k-1).mul_by_vanishing_poly(domain) + poly (:311-312 k = 2, :347-348 k = 3).  k <= 4, any n >= 1 (a domain smaller
 * than the mask included). */
int plonk_blind_dev(plonk_ctx* ctx, void* d_poly, size_t n, const uint64_t* blinders, size_t k);

/* ---- evaluation on / interpolation from an ARBITRARY coset (building block of coset-class parallelism) ------
 * d_out[k] = poly(shift * w_size^k), k < size; size a power of two, len <= 8*size (coefficients beyond `size` fold back, since
 * X^size = shift^size on the coset).  shift = Fr::multiplicative_generator(), size = m: quot_domain.coset_fft (dispatcher2.rs:387-424)
 * of the zero-padded vector.  shift = g * w_m^s, size = m/G: the evaluations at the points of index s, s+G, s+2G, ... of that
 * same coset FFT — rank s's share of every round-3 vector with no communication.
 * Zero-padding aware: the `size - len` zero coefficients the reference appends (dispatcher2.rs:746) are never loaded, multiplied or
 * stored — with len <= size/2 the transform runs as 2^k independent (size/2^k)-point transforms of the same coefficients on the
 * sub-cosets (shift * w_size^q) * <w_(size/2^k)> whose results are interleaved into natural order by the last pass' stores.
 * d_poly is not modified; d_out must not alias it. */
int plonk_coset_eval_dev(plonk_ctx* ctx, const void* d_poly, size_t len, size_t size, const uint64_t* shift, void* d_out);
/* E = iNTT_size(d_evals) (d_evals is destroyed), d_out[t] = scale * shift^-(i0+t) * E[(i0+t) mod size], t < count.
 * shift = g, scale = 1, i0 = 0, count = size: quot_domain.coset_ifft (dispatcher2.rs:507).  With scale = 1/G and shift = g * w_m^s,
 * the sum over s < G of these vectors is coefficient i0+t of the polynomial interpolating all G cosets. */
int plonk_coset_interp_dev(plonk_ctx* ctx, void* d_evals, size_t size, const uint64_t* shift, const uint64_t* scale, size_t i0, size_t count,
                           void* d_out);

/* `classes` vectors of `size` values (d_in: class-major, class s at d_in + s * in_stride; in_stride = 0: size) -> natural order:
 * d_out[t * classes + s] = scale * d_in[s * in_stride + t'], t' = t, or (size - t) mod size with reverse != 0; scale = NULL: 1.
 * classes in {1, 2, 4, 8}; not in place.  What the dispatcher does
 * with the column replies of a distributed transform (dispatcher2.rs:776-787: concatenate + transpose), for transforms split by
 * residue class: a size-n iFFT over G workers is, on worker s, plonk_coset_eval_dev(evaluations, n, n / G, shift = w_n^-s) — the
 * evaluations read as coefficients, folded G-fold onto n / G points — then an all-gather, then this call with reverse = 1,
 * scale = 1 / n: coefficient s + G t of the interpolant is 1/n times value (n/G - t) mod n/G of class s. */
int plonk_class_interleave_dev(plonk_ctx* ctx, const void* d_in, size_t classes, size_t size, size_t in_stride, int reverse, const uint64_t* scale,
                               void* d_out);

/* ---- device memory + synthetic inputs (bench / tests; the reference uses thread_rng) ---------- */
/* Give back every cache the context can rebuild on demand (exchange buffers of finished FFT tasks, NTT factor planes and tables derived per
 * problem size, MSM workspace, scratch): a worker's State outlives a circuit (worker.rs:42-59) and would otherwise keep the last problem's
 * tens of GiB.  The SRS, the domains, open FFT tasks and the communicator stay.  Synchronises the context's stream. */
int plonk_trim(plonk_ctx* ctx);
int plonk_dev_alloc(plonk_ctx* ctx, size_t bytes, void** out);
int plonk_dev_free(plonk_ctx* ctx, void* p);
int plonk_memcpy_h2d(plonk_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int plonk_memcpy_d2h(plonk_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);
int plonk_memcpy_d2d(plonk_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);
int plonk_memcpy_d2d_async(plonk_ctx* ctx, void* d_dst, const void* d_src, size_t bytes);   /* ordered on the context's stream, not synchronised */
int plonk_memset_dev(plonk_ctx* ctx, void* d_dst, int byte, size_t bytes);
/* n uniform Fr (Montgomery limbs drawn like ark-ff's Fp::rand: mask + rejection), element i from
 * stream (seed, i). */
int plonk_synth_fr(plonk_ctx* ctx, uint64_t seed, void* d_out, size_t n);
/* SRS-like bases in PLONK_BASES_XY layout.  unique > 0: `unique` points k_j*G tiled to n (the
 * distribution of dispatcher.rs:190-196); unique == 0: n pairwise-distinct points A[i%4096] + B[i/4096]. */
int plonk_synth_bases(plonk_ctx* ctx, uint64_t seed, size_t unique, size_t n, void* d_out);
/* A KZG commit key with a KNOWN trapdoor: d_out[i] = tau^i * G, i < n (PLONK_BASES_XY).  The reference's universal_setup
 * (dispatcher2.rs:1278) draws tau and forgets it; keeping it makes commit(f) = f(tau) * G, so a proof can be verified in G1 without
 * a pairing (oracle/verifier_ref.py) — how bench.py checks a whole 2^24-gate proof.  tau: host Fr, Montgomery. */
int plonk_synth_srs(plonk_ctx* ctx, const uint64_t* tau, size_t n, void* d_out);
/* A random SATISFIED TurboPlonk instance of n = 2^k gates, generated in HBM (the reference's generate_circuit, dispatcher2.rs:1214-1270,
 * needs jellyfish's circuit builder; north_star asks for synthetic random circuits).  Column i of gate j reads variable P_i(j) for
 * seeded bijections P_i, so the copy constraints are n cycles of length 5 between pseudo-random gates; witness values are uniform
 * per variable; 12 selectors are uniform and q_c is solved so that the gate equation of dispatcher2.rs:465-477 holds; the first
 * num_inputs gates carry uniform public inputs.  Outputs (device): wires [5][n] Fr, selector EVALUATIONS [13][n] and sigma
 * EVALUATIONS [5][n] on the n-point domain (coefficient form = plonk_ntt_dev(.., is_inv = 1)), id_perm [5n] = k_i * w^j
 * (extended_id_permutation), perm_idx [5n] u64 (perm_i * n + perm_j), pub_input [n].  k: vk.k[0..5], host Fr. */
int plonk_synth_circuit(plonk_ctx* ctx, uint64_t seed, size_t n, size_t num_inputs, const uint64_t* k, void* d_wires, void* d_selector_evals,
                        void* d_sigma_evals, void* d_id_perm, void* d_perm_idx, void* d_pub_input);
/* Preprocessing of a user circuit given as jellyfish's arithmetised form (wire_variables, witness, selectors, public inputs).
 * Device pointers, host Fr in Montgomery form, ordered on the context's stream.  n: the gate count, a power of two >= 2 within the
 * field's two-adicity (PLONK_ERR_DOMAIN otherwise).  Positions are p = i*n + j (wire column i < 5, gate j < n).  Ids are checked on the
 * device before any of them is used as an index: an out-of-range id returns PLONK_ERR_ARG naming the first offending position, and
 * nothing is read or written out of bounds.
 *
 * The copy-constraint permutation (jellyfish compute_wire_permutation).  wire_vars: u32 [5][n], wire_vars[i*n + j] = the variable
 * gate j's wire i reads, each < num_vars; k: vk.k[0..5] (5 x 4 u64).  The positions of one variable, in increasing order, form a
 * cycle whose last position links back to the first (a variable read once maps its position to itself):
 *   id_perm [5n] Fr:   id_perm[i*n + j] = k_i * w^j
 *   perm_idx [5n] u64: the position after p in the cycle of p's variable
 *   sigma_evals [5n] Fr: id_perm[perm_idx[p]]  (the 5 sigma polynomials in evaluation form)
 * Bit-identical from run to run (a stable device radix sort of (variable, position), then a linking pass).  Scratch from the context
 * (2 x 2 x 5n u32 + 4 * num_vars bytes), given back by plonk_trim.  Returns once the work is enqueued. */
int plonk_circuit_permutation_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, size_t num_vars, const uint64_t* k, void* d_id_perm,
                                  void* d_perm_idx, void* d_sigma_evals);
/* Witness placement: wires[p] = witness[wire_vars[p]], p < 5n; witness: num_vars Fr.  Synchronises (reads the id check's verdict). */
int plonk_circuit_witness_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, const void* d_witness, size_t num_vars, void* d_wires);
/* Satisfiability (jellyfish check_circuit_satisfiability).  wires [5][n], selector_evals [13][n] (q_lc 0-3, q_mul 4-5, q_hash 6-9, q_o 10,
 * q_c 11, q_ecc 12), pub_input [n] evaluations.  *first_bad_gate = the smallest gate j where
 *   q_c + PI + sum q_lc*w + q_mul0*ab + q_mul1*cd + sum q_hash*w^5 + q_ecc*abcde - q_o*e != 0, or -1.
 * perm_idx [5n] u64 or NULL: *first_bad_copy = the smallest position p with wires[p] != wires[perm_idx[p]], or -1 (always -1 without
 * perm_idx); an entry >= 5n returns PLONK_ERR_ARG.  Synchronises. */
int plonk_circuit_check_dev(plonk_ctx* ctx, const void* d_wires, const void* d_selector_evals, const void* d_pub_input, const void* d_perm_idx,
                            size_t n, int64_t* first_bad_gate, int64_t* first_bad_copy);
/* The witness solved on the device: the counterpart of building a circuit with jellyfish's PlonkCircuit (create_variable, the arithmetic
 * gates) and taking its witness, as the reference's generate_circuit / check_circuit_satisfiability do at dispatcher2.rs:1226-1271.
 * def_gate: u32 [num_vars], the gate that defines the variable, or 0xFFFFFFFF = given.  witness: num_vars Fr, in/out: given variables
 * hold their values on entry, every defined variable v is written with
 *   (q_c + PI + sum q_lc*w + q_mul0*ab + q_mul1*cd + sum q_hash*w^5) / q_o   at gate def_gate[v], whose wire 4 reads v
 * (q_o = +-1 costs no inversion).  wire_vars, selector_evals, pub_input as above; num_vars <= 2^32 - 2.  Checked on the device before any id
 * is used as an index, PLONK_ERR_ARG naming the variable and gate otherwise: wire ids < num_vars; def_gate[v] < n; wire 4 of that gate
 * reads v (hence no two variables claim one gate); q_o != 0 and q_ecc == 0 there.  Wire i < 4 of a gate is a dependency only where it is
 * live (q_lc[i], q_hash[i] or q_mul[i/2] non-zero); a dead wire may read anything.  Evaluation runs level by level: level 0 is the defining
 * gates none of whose live wires reads a defined variable, a gate joins level L+1 when the last of them was written in level L.  Every
 * defining gate is evaluated once: O(n) work, a stable radix sort of the 4n (variable, consumer) pairs and one launch per level.
 *   *unsolved_var  -1, or the smallest defined variable that could not be solved (a dependency cycle); the witness is then incomplete
 *   *levels        dependency levels evaluated;   *evaluations   gate evaluations performed (= defined variables on success)
 * All outputs are functions of the input alone.  Scratch from the context (4 x 4n u32 for the sort, 3n u32, 4 * num_vars bytes), given
 * back by plonk_trim.  Synchronises. */
int plonk_circuit_solve_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, size_t num_vars, const void* d_selector_evals, const void* d_pub_input,
                            const void* d_def_gate, void* d_witness, int64_t* unsolved_var, uint64_t* levels, uint64_t* evaluations);
/* plonk_circuit_solve_dev with HINTED definitions: values that no gate equation yields (an inverse, a fifth root, a bit), which a gate then only
 * checks — division, is_zero, range checks, the inverse S-box of a Rescue round.  hint_op: u32 [n] or NULL; NULL is plonk_circuit_solve_dev
 * itself (the same kernels, outputs and error texts).  hint_op[g]: bits 0-7 an opcode, bits 8-31 an argument; 0 = an ordinary gate.  A
 * non-zero opcode makes g a hint gate: the variable on its wire 4 (def_gate[v] = g as above) is computed from the values s0 on wire 2 and s1
 * on wire 3, and no selector of g is read — the selectors carry the check (typically q_o = 0 and a product or a power on wires 0-1):
 *   1 INV    s0^-1, 0 for s0 = 0            2 DIV    s0 * s1^-1, 0 for s1 = 0
 *   3 ROOT5  s0^d, d = 5^-1 mod (r - 1)     4 BIT    bit `arg` (< 256) of the canonical residue of s0; 0 at and above the field's bit length
 * A hint gate depends on its source wires only (wire 2; wire 3 too for DIV): wires 0 and 1 are dead for scheduling whatever the selectors
 * say and may read the gate's own output.  Levels and counters as above.  Checked on the device as above, except that q_o != 0 and
 * q_ecc == 0 are not required at a hint gate; PLONK_ERR_ARG naming the variable and gate for an unknown opcode or a BIT argument >= 256, and
 * naming the gate for a non-zero hint_op at a gate that defines no variable.  Per level the ordinary gates and BIT hints, the INV / DIV hints
 * and the ROOT5 hints run as separate launches over separate lists (a power costs ~330 field products, a gate ~20).  Scratch: 4n u32 more than
 * plonk_circuit_solve_dev.  Synchronises. */
int plonk_circuit_solve_hints_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, size_t num_vars, const void* d_selector_evals,
                                  const void* d_pub_input, const void* d_def_gate, const void* d_hint_op, void* d_witness, int64_t* unsolved_var,
                                  uint64_t* levels, uint64_t* evaluations);
/* The solver's schedule, recorded once per circuit: which gate is evaluated in which level depends on wire_vars, selector_evals, def_gate and
 * hint_op alone, not on the witness.  The same validation as plonk_circuit_solve_hints_dev with the same error texts (under this entry's name);
 * hint_op NULL: no hints.  The levels are then walked structurally — no field value is read or written, no witness or public input is needed —
 * and every defining gate gets the key 3L + c: L its level, c its cost class (0 an ordinary gate or a BIT hint, 1 INV / DIV, 2 ROOT5; without
 * hints class 0 only).  The stable radix sort of (key, gate) gives
 *   d_order  u32 [n], device: d_order[0 .. *evaluations) = the evaluated gates sorted by (L, c, gate)
 *   seg      HOST, 3n + 1 words of which 3 * *levels + 1 are written: seg[3L + c] = the first slot of that segment, seg[3 * *levels] = *evaluations
 * a function of the circuit alone, whichever lane appended first during the walk.  *unsolved_var, *levels, *evaluations: what the solver
 * reports for the same circuit.  Scratch: the solver's and 4n + 1 u32.  Synchronises. */
int plonk_circuit_schedule_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, size_t num_vars, const void* d_selector_evals, const void* d_def_gate,
                               const void* d_hint_op, void* d_order, uint32_t* seg, int64_t* unsolved_var, uint64_t* levels, uint64_t* evaluations);
/* fuse_width of plonk_circuit_replay_dev unless the caller has a reason for another (profiles/solve_replay.txt) */
#define PLONK_REPLAY_FUSE_DEFAULT 256
/* K witnesses solved from a recorded schedule (d_order, seg, levels of plonk_circuit_schedule_dev for the same d_wire_vars, d_selector_evals and
 * d_hint_op).  d_witness: K x num_vars Fr, witness b at d_witness + b * num_vars * 32 — what plonk_circuit_witness_dev and
 * plonk_circuit_check_dev take — with the given variables in place and zero elsewhere; d_pub_inputs: K x num_inputs Fr (NULL iff num_inputs = 0),
 * the public input of witness b at gate g < num_inputs is pub[b][g], 0 at every other gate.  Every evaluated gate goes through the solver's own
 * value code, so witness b is bit-identical to what plonk_circuit_solve*_dev writes for the same inputs.  No atomics, no sort, no host read and
 * no synchronisation between launches; the launches are chosen from seg alone:
 *   wide    one launch per non-empty segment, seg_len x K lanes
 *   fused   one launch for a maximal run of consecutive segments of at most fuse_width gates each (when it holds more than one non-empty
 *           segment): workgroup b walks the run for witness b, its lanes striding over each segment, a barrier where the level changes
 * fuse_width = 0 never fuses.  The result does not depend on fuse_width.  PLONK_ERR_ARG naming the argument, checked on the host before the
 * context is touched: a NULL pointer, d_pub_inputs given without num_inputs or the reverse, num_inputs > n, K = 0, levels > n, seg decreasing or
 * seg[3 * levels] > n.  An entry of d_order >= n is skipped; a schedule of another circuit is not defended against.  seg is copied; returns once
 * the work is enqueued on the context's stream. */
int plonk_circuit_replay_dev(plonk_ctx* ctx, const void* d_wire_vars, size_t n, size_t num_vars, const void* d_selector_evals, const void* d_hint_op,
                             const void* d_order, const uint32_t* seg, uint64_t levels, const void* d_pub_inputs, size_t num_inputs, void* d_witness, size_t K,
                             unsigned fuse_width);
/* The Rescue permutation on the device, the one builder.py's rescue_permutation proves: state s in Fr^4, alpha = 5, 12 rounds (jellyfish's
 * structure),
 *   s <- s + K[0];   12 times:  s <- M (s_j^(1/5))_j + K[2i+1],   s <- M (s_j^5)_j + K[2i+2]        x^(1/5) = x^d, d = 5^-1 mod (r - 1); 0 -> 0
 * and hash2(l, r) = permute((l, r, 0, 0))[0].  params: HOST, 116 Fr Montgomery = M row-major (16) then K[0..24] (100; K[t][i] at 16 + 4t + i),
 * kept in a context-owned device buffer and uploaded again only when the bytes differ from the last call's (distributed_plonk_amd/rescue.py
 * derives the project's default parameters).  d_states: [count][4] Fr Montgomery, permuted in place, one lane per state (~16.6 k field products
 * each).  Ordered on the context's stream; returns once the work is enqueued (plonk_sync, or any synchronising call, waits for it).  count = 0
 * is a no-op.  PLONK_ERR_ARG for a NULL params or d_states. */
int plonk_rescue_permute_dev(plonk_ctx* ctx, const uint64_t* params, void* d_states, size_t count);
/* A Merkle tree over 2^log_leaves leaves with hash2 above, in heap order in one buffer of 2^(log_leaves+1) - 1 Fr: node 0 is the root, the
 * children of node m are 2m+1 (left) and 2m+2 (right), leaf i is node 2^log_leaves - 1 + i.  The leaves are filled on entry; every inner node
 * is written, node[m] = hash2(node[2m+1], node[2m+2]): log_leaves launches, bottom-up, on the context's stream; returns once they are
 * enqueued.  log_leaves = 0 is a no-op (the leaf is the root).  PLONK_ERR_ARG for a NULL params or d_nodes, or log_leaves > 31. */
int plonk_rescue_merkle_dev(plonk_ctx* ctx, const uint64_t* params, void* d_nodes, unsigned log_leaves);
/* The ternary Rescue accumulator: jellyfish's sparse, append-only 3-ary Merkle tree, the one the reference's test circuit proves memberships
 * in (generate_circuit, dispatcher2.rs:1226-1271: TREE_HEIGHT = 32, 50 leaves at uids 0 .. 49).  With hash3(a, b, c) = permute((a, b, c, 0))[0]:
 *   level 0    c_0 = count nodes:               node_0[i]     = hash3(0, i, elems[i])             (the uid i as a field element)
 *   level j+1  c_{j+1} = ceil(c_j / 3) nodes:   node_{j+1}[t] = hash3(x_0, x_1, x_2),  x_k = node_j[3t+k] if 3t+k < c_j, else 0
 * for j < height.  An empty subtree is 0 (not hash3(0, 0, 0)) and no all-empty node is computed.  d_nodes: sum_{j <= height} c_j Fr (at most
 * 1.5 count + height), the levels one after another from the leaves up: offset_0 = 0, offset_{j+1} = offset_j + c_j; the root is the last
 * element.  d_elems: count Fr, Montgomery; params as for plonk_rescue_permute_dev.  One launch for the leaves, one per level with more than
 * one node, and ONE for the chain hash3(x, 0, 0) above the first level of one node.  Ordered on the context's stream; returns once the work
 * is enqueued.  PLONK_ERR_ARG naming the argument for a NULL pointer, height outside 1 .. 40, count outside 1 .. 3^height. */
int plonk_rescue_acc_build_dev(plonk_ctx* ctx, const uint64_t* params, const void* d_elems, size_t count, unsigned height, void* d_nodes);
/* The membership witnesses of m uids of a built accumulator, written where a solve takes them from.  d_uids: u64 [m].  For level j < height
 * the node on the path of uid i is number q = floor(i / 3^j) of the level, pos_j = q mod 3 its position in the group of three from
 * g = 3 floor(i / 3^(j+1)) on; sib1_j, sib2_j are the two OTHER members of the group in ascending position (0 beyond c_j),
 * is_left_j = [pos_j = 0], is_right_j = [pos_j = 2] as field 0 / 1.  d_inputs_out: (2 + 4 height) rows of m Fr, row-major: the uids as field
 * elements, elems[uid], then per level sib1_j, sib2_j, is_left_j, is_right_j — the order in which distributed_plonk_amd/membership.py creates
 * the inputs of its circuit.  m = 0 is a no-op.  PLONK_ERR_ARG as above, and naming the first k with d_uids[k] >= count (checked on the device;
 * nothing is written for such a k).  Synchronises. */
int plonk_rescue_acc_paths_dev(plonk_ctx* ctx, const void* d_nodes, size_t count, unsigned height, const void* d_elems, const void* d_uids, size_t m,
                               void* d_inputs_out);
/* witness[input_vars[k]] = inputs[k], k < num_inputs: the given variables of plonk_circuit_solve_dev's witness from values already on the
 * device.  d_input_vars: u32 [num_inputs]; d_inputs: num_inputs Fr; d_witness: num_vars Fr.  num_inputs = 0 is a no-op.  PLONK_ERR_ARG for a
 * NULL pointer, num_vars outside 1 .. 2^32 - 2, and naming the first k with input_vars[k] >= num_vars (checked on the device; nothing is
 * written for such a k).  Synchronises. */
int plonk_circuit_scatter_inputs_dev(plonk_ctx* ctx, const void* d_input_vars, size_t num_inputs, const void* d_inputs, void* d_witness, size_t num_vars);
/* The embedded twisted Edwards curve E: a x^2 + y^2 = 1 + d x^2 y^2 over the context's Fr (Baby Jubjub on BN254, Jubjub on BLS12-381;
 * distributed_plonk_amd/edwards.py holds the parameters), the group builder.py's point gadgets prove.  a is a square and d a non-square, so the
 * addition law is complete: doubling, inverses, the identity (0, 1) and the points of small order need no special case.  params: HOST, 20 u64 =
 * a, d, G.x, G.y as Fr Montgomery, then the order l of G as 4 plain limbs; they travel as kernel arguments.  Points: [count][2] Fr Montgomery,
 * affine (x, y).  Scalars: [count] Fr Montgomery; a scalar stands for its canonical residue k in [0, r), so a hash output multiplies a point
 * directly.  One lane per element, extended coordinates in registers, one inversion (~335 products) per result.  All four are ordered on the
 * context's stream and return once the work is enqueued; count = 0 is a no-op; PLONK_ERR_ARG naming the argument for a NULL pointer, and for a
 * count beyond one launch.
 * mul: d_out[i] = [k_i] d_points[i], bit_length(r) doublings and as many additions, each computed and then selected (~5.2 k products, no
 * divergence).  d_out may be d_points.  The points must lie on E (plonk_edwards_check_dev); for others the result is unspecified. */
int plonk_edwards_mul_dev(plonk_ctx* ctx, const uint64_t* params, const void* d_scalars, const void* d_points, size_t count, void* d_out);
/* d_out[i] = [k_i] G from a table of [j 16^w] G, j < 16, w < 64 (64 KB, affine) in a context-owned device buffer: built on the device when the
 * 20 words of params differ from those of the last call, then 64 gathered additions per lane (~1.0 k products). */
int plonk_edwards_fixed_mul_dev(plonk_ctx* ctx, const uint64_t* params, const void* d_scalars, size_t count, void* d_out);
/* d_out[i] = d_p[i] + d_q[i] by the unified law (also the doubling: d_p = d_q), affine and exact.  d_out may be d_p or d_q. */
int plonk_edwards_add_dev(plonk_ctx* ctx, const uint64_t* params, const void* d_p, const void* d_q, size_t count, void* d_out);
/* d_flags: u32 [count].  Bit 0: the point satisfies the curve equation.  Bit 1: it does and [l] point = (0, 1), i.e. it lies in the subgroup of
 * prime order l (l < r: one run of mul's loop over bit_length(l) bits, without the inversion). */
int plonk_edwards_check_dev(plonk_ctx* ctx, const uint64_t* params, const void* d_points, size_t count, void* d_flags);
/* A variable-length hash and public-key encryption over the two families above, the functions builder.py's rescue_sponge, rescue_stream and
 * elgamal_encrypt prove.  permute is the width-4 Rescue permutation; its fourth state element is the capacity and carries the domain: hash2 and
 * hash3 use 0, the sponge starts at L, the stream uses -1.  rescue_params: HOST, 116 Fr as for plonk_rescue_permute_dev (uploaded again only when
 * the bytes differ; the copy is ordered on the stream).  The sponge and the stream are ONE launch each, the key two; all are ordered on the
 * context's stream and return once the work is enqueued; count = 0 is a no-op.  PLONK_ERR_ARG naming the entry point and the argument — for a NULL pointer, L = 0 or L >= 2^32, n_out outside
 * 1 .. 3, and a lane count beyond one launch (2^31 - 1 workgroups of 256 lanes) — before anything is uploaded or launched.
 * sponge: d_out[i][0 : n_out] = s[0 : n_out] after  s = (0, 0, 0, L);  for b < ceil(L / 3):  s[j] += x_i[3b + j] (j < 3, 3b + j < L), s = permute(s).
 * d_inputs: [count][L] Fr Montgomery, row-major; d_out: [count][n_out] Fr.  One lane per message, ceil(L / 3) permutations each.  The length in
 * the capacity separates (a) from (a, 0); sponge((a, b, c); 1) = permute((a, b, c, 3))[0] is NOT hash3(a, b, c), by design. */
int plonk_rescue_sponge_dev(plonk_ctx* ctx, const uint64_t* rescue_params, const void* d_inputs, size_t L, size_t count, unsigned n_out, void* d_out);
/* Counter mode: block j >= 0 of the keystream under key k is ks_j = permute((k, j, 0, -1))[0 : 3], and element t of a text of L elements uses
 * ks_{t div 3}[t mod 3].  d_out[i][t] = d_in[i][t] + ks (decrypt = 0) or d_in[i][t] - ks (decrypt != 0) under d_keys[i].  d_keys: [count] Fr;
 * d_in, d_out: [count][L] Fr, row-major; d_out may be d_in (and must not overlap d_keys).  One lane per (text, block): count x ceil(L / 3) lanes;
 * exactly count x L elements are written. */
int plonk_rescue_stream_dev(plonk_ctx* ctx, const uint64_t* rescue_params, const void* d_keys, const void* d_in, size_t L, size_t count, int decrypt, void* d_out);
/* The shared key of the ElGamal / Rescue hybrid: d_keys[i] = hash3(S.x, S.y, 0) for S = [k_i] d_points[i], scalars and points as for
 * plonk_edwards_mul_dev.  With ek = [dk] G, encryption under randomness r < l is E = [r] G (plonk_edwards_fixed_mul_dev), key from (r, ek), then
 * plonk_rescue_stream_dev; decryption takes the key from (dk, E).  One lane per pair, ~21.8 k products, in TWO launches: mul's loop with its one
 * inversion, then the permutation, with the shared points in a context-owned buffer of 64 count bytes between them (plonk_trim gives it back;
 * a call that needs a larger one than the last waits for the device while it is replaced).  One kernel doing both was measured 9 % slower
 * than the two: DESIGN.md §4.3.  A point that does not satisfy the curve equation is taken for the identity (0, 1) —
 * its key is hash3(0, 1, 0) —; whether a point lies in the subgroup of order l is plonk_edwards_check_dev's verdict, not an error here. */
int plonk_edwards_dh_key_dev(plonk_ctx* ctx, const uint64_t* edwards_params, const uint64_t* rescue_params, const void* d_scalars, const void* d_points, size_t count,
                             void* d_keys);
/* G2 and the pairing, host-only (no context, no GPU), for the verifier's last step e(A, [tau]_2) * e(-B, [1]_2) == 1 (jf-plonk's verify).
 * G2 points lie on the sextic twist (BN254: y^2 = x^3 + 3/(9+u), BLS12-381: y^2 = x^3 + 4(1+u); Fq2 = Fq[u]/(u^2+1)) and are encoded as
 * x.c0 || x.c1 || y.c0 || y.c1 Montgomery limbs (4Q u64), all zero = infinity; G1 points as x || y (2Q u64), (0, 0) = infinity.  Coordinates
 * must be canonical residues on the curve (PLONK_ERR_ARG otherwise).  No element of the target group crosses the ABI. */
int plonk_g2_generator(int curve, uint64_t* out);                     /* arkworks' G2 generator */
int plonk_g2_mul(int curve, const uint64_t* scalar, const uint64_t* in, uint64_t* out);     /* scalar: Fr, Montgomery */
/* *ok = 1 iff pt is a canonical point on the twist in the order-r subgroup (or infinity); a bad point is a verdict, not an error. */
int plonk_g2_check(int curve, const uint64_t* pt, int* ok);
/* *is_one = 1 iff prod_{i<k} e(P_i, Q_i) == 1 (optimal ate, one final exponentiation).  g1_xy: k G1 points, g2_xy: k G2 points; pairs
 * with an infinity are skipped.  Subgroup membership of the Q_i is the caller's (plonk_g2_check). */
int plonk_pairing_check(int curve, size_t k, const uint64_t* g1_xy, const uint64_t* g2_xy, int* is_one);

/* Batched verification, the per-proof part (jf-plonk's verify / batch_verify up to the pairing), one lane per proof.  For proof j it
 * writes rho_j*A_j and rho_j*B_j of the folded check
 *     A = W_zeta + u W_zeta_omega,   B = zeta W_zeta + u zeta w W_zeta_omega + F + u [z] - (E + u z(zeta w)) G
 * (F, E, the linearisation: DESIGN.md §9), so that e(sum rho A, [tau]_2) == e(sum rho B, [1]_2) accepts the batch.  The Fiat-Shamir
 * transcript is replayed on the device from the state after the verifying-key messages (append_vk_and_pub_input with the public-input
 * count and no inputs): its 200 bytes and pos / pos_begin / cur_flags.
 *   d_proofs     k records, each the 13 points (wires_poly_comms[5], prod_perm_poly_comm, split_quot_poly_comms[5], opening_proof,
 *                shifted_opening_proof: 2Q u64 each, (0, 0) = infinity) then the 10 Fr (wires_evals[5], wire_sigma_evals[4],
 *                perm_next_eval; 4 u64 each), Montgomery
 *   d_pub_inputs k x num_inputs Fr;  d_rho k Fr (rho = 1: the single-proof check)
 *   d_out_points k x [rho B, rho A] affine G1 (2Q u64 each), (0, 0) for a proof whose status is not 0
 *   d_status     k u32: 0 ok, | 1 a point off the curve, | 2 a point outside the r-subgroup (BLS12-381), | 4 zeta in the domain,
 *                | 8 a coordinate or scalar not canonical
 *   d_debug      NULL or k x 9 Fr: beta, gamma, alpha, zeta, v, u, PI(zeta), r(zeta), E
 * Device pointers, ordered on the context's stream; needs no SRS.  Returns once the work is enqueued. */
typedef struct plonk_verify_key {
    uint64_t domain_size;           /* n, a power of two >= 2 (PLONK_ERR_DOMAIN otherwise) */
    uint64_t num_inputs;            /* public inputs per proof, <= n */
    uint64_t k[5][4];               /* coset separators, Fr Montgomery */
    const void* d_comms;            /* device: the 13 selector then 5 sigma commitments, affine as the proof points */
    uint8_t transcript_state[200];
    uint32_t transcript_pos[3];     /* pos (< 166), pos_begin, cur_flags */
} plonk_verify_key;
int plonk_verify_batch_dev(plonk_ctx* ctx, const plonk_verify_key* vk, size_t k, const void* d_proofs, const void* d_pub_inputs, const void* d_rho,
                           void* d_out_points, void* d_status, void* d_debug);
/* The same with one verifying key PER PROOF (jf-plonk's batch_verify): a block that mixes circuits, each with its own domain size and
 * public-input count, is one call and one pairing check.
 *   vks           HOST array of n_vks keys (1 .. 4096), each with its own d_comms, each checked as plonk_verify_batch_dev checks its key; an
 *                 error names the key's index.  The library derives omega, n and log2 n per key and keeps them, the transcript states and
 *                 the commitment pointers in a device table of its own (uploaded again only when a call's keys differ from the last call's)
 *   d_proofs      k records as above: the layout does not depend on the key
 *   d_vk_index    k u32: the key of proof j
 *   d_pub_offsets k + 1 u64, in Fr elements into d_pub_inputs (pub_total elements; NULL allowed when pub_total is 0): proof j owns
 *                 [off[j], off[j+1]), possibly empty
 *   d_rho, d_out_points, d_status, d_debug as above, with two more status bits, verdicts like the others:
 *                 | 32 the key index is >= n_vks, | 64 the span is bad: off[j] > off[j+1], off[j+1] > pub_total, or (under a good index) a
 *                 length other than the key's num_inputs.  Such a proof reads nothing through its index or span and gets (0, 0) twice.
 * Lanes of one wave may run under different keys; they diverge in the loops over log2 n and the public inputs only. */
int plonk_verify_batch_multi_dev(plonk_ctx* ctx, const plonk_verify_key* vks, size_t n_vks, size_t k, const void* d_proofs, const void* d_vk_index,
                                 const void* d_pub_inputs, const void* d_pub_offsets, size_t pub_total, const void* d_rho, void* d_out_points,
                                 void* d_status, void* d_debug);
/* The fold of a batch as a sum tree on the device.  d_points: k pairs [rho B, rho A] of affine G1 points with canonical coordinates
 * (exactly d_out_points above; k <= 2^22); d_mask: NULL or k u32, a non-zero word turning its pair into two infinities (the status words).
 * d_tree receives 2P - 1 pairs in heap order, P the next power of two >= k: the root is node 0, the children of node i are 2i + 1 and
 * 2i + 2, leaf j is node P - 1 + j, leaves >= k are infinity, every inner node is the pair of sums of its children's pairs.  The addition
 * is complete (equal inputs, opposite inputs — the sum is written (0, 0) —, infinity on either side or both).  One launch for the leaves
 * and one per level, one lane per output point, one inversion per inner point; enqueued on the context's stream; k = 0 is a no-op. */
int plonk_g1_sum_tree_dev(plonk_ctx* ctx, const void* d_points, size_t k, const void* d_mask, void* d_tree);
/* k opening records [C (2Q u64), pi (2Q u64), z (4 u64), y (4 u64)] -> d_out_points k x [rho B, rho A] as plonk_verify_batch_dev writes them,
 * d_status k u32: | 1 off the curve, | 2 outside the r-subgroup (BLS12-381), | 8 coordinate or scalar not canonical; a record with a status gets
 * (0, 0) twice.  g_xy: the open key's G (HOST, 2Q u64).  Feeds plonk_g1_sum_tree_dev unchanged.  Enqueued, not synchronised; needs no SRS.
 * An opening (C, pi, z, y) of a KZG commitment holds iff e(pi, [tau]_2) = e(C - y G + z pi, [1]_2); with d_rho (k Fr) the pair is
 * A = rho pi, B = rho C + (rho z) pi - (rho y) G.  Points affine Montgomery with (0, 0) = infinity, z, y and rho Montgomery Fr; k <= 2^22. */
int plonk_kzg_pairs_dev(plonk_ctx* ctx, size_t k, const void* d_openings, const void* d_rho, const uint64_t* g_xy, void* d_out_points, void* d_status);
/* ark-serialize 0.3 bytes <-> Montgomery limbs (`to_bytes!` of the reference; csrc/codec_kernels.hpp), one lane per element.
 * A G1Affine is, compressed, its x coordinate little-endian (32 B BN254 / 48 B BLS12-381) with two flags in the top bits of the last byte:
 * 0x80 "y is the larger of {y, -y} as integers", 0x40 infinity; uncompressed, x then y (64 B / 96 B), the last byte of y carrying only 0x40.
 * An Fr is 32 bytes little-endian, canonical.  Decoding a compressed point is one Fq power, y = (x^3 + b)^((q+1)/4) (q = 3 mod 4 on both
 * curves), and one squaring to test it.  Element i is read at base + i * stride and written at base + i * stride on the other side (strides
 * in BYTES on the byte side — any value >= the element, no alignment needed — and in u64 on the limb side); what lies between elements is
 * left untouched.  Points come out as x || y (2Q u64, the PLONK_BASES_XY / proof-record form, (0, 0) = infinity).
 * A bad element is never an error code: its bits are OR-ed (atomically) into the u32 at d_status + i * status_stride (in u32; 0 lets all
 * elements share one word) and (0, 0) — for an Fr, 0 — is written.  The caller clears the status words first.
 *     1   no point has this x, or the uncompressed pair is off the curve
 *     2   outside the r-subgroup (only with check_subgroup != 0 and only on BLS12-381: [r] P != O; BN254's G1 has cofactor 1)
 *     8   non-canonical: a coordinate >= q or a scalar >= r, both flags set, the infinity flag with a non-zero coordinate (stricter than
 *         ark-serialize, which as far as the public sources show ignores those bytes: DESIGN.md §5), the sign flag in an uncompressed element
 *     16  (plonk_proofs_from_bytes_dev) a Vec length prefix of the serialized Proof differs from 5, 5, 5, 4
 * 1, 2 and 8 mean what they mean in plonk_verify_batch_dev's status.  The *_dev entry points are ordered on the context's stream and
 * return once enqueued; count = 0 is a no-op; a NULL pointer with count > 0, a stride shorter than the element, an unknown encoding and a
 * count beyond one launch are PLONK_ERR_ARG naming the entry point. */
enum { PLONK_BYTES_COMPRESSED = 0, PLONK_BYTES_UNCOMPRESSED = 1 };
int plonk_g1_from_bytes_dev(plonk_ctx* ctx, const void* d_bytes, size_t in_stride, size_t count, int encoding, int check_subgroup, void* d_out_xy,
                            size_t out_stride_u64, void* d_status, size_t status_stride);
int plonk_g1_to_bytes_dev(plonk_ctx* ctx, const void* d_xy, size_t in_stride_u64, size_t count, int encoding, void* d_bytes, size_t out_stride);
int plonk_fr_from_bytes_dev(plonk_ctx* ctx, const void* d_bytes, size_t in_stride, size_t count, void* d_out, size_t out_stride_u64, void* d_status,
                            size_t status_stride);
int plonk_fr_to_bytes_dev(plonk_ctx* ctx, const void* d_fr, size_t in_stride_u64, size_t count, void* d_bytes, size_t out_stride);
/* k serialized `Proof`s (768 B each on BN254, 976 B on BLS12-381: 13 compressed points and 10 Fr behind four u64 Vec lengths, the layout of
 * transcript.serialize_proof — not pinned by a reference-generated proof) -> k records of plonk_verify_batch_dev in d_proofs
 * and one status word per proof in d_status (cleared here).  Five launches, seven on BLS12-381: two point decodes (each followed there by
 * the r-subgroup check as a launch of its own), two scalar decodes, the length prefixes.  A proof with a non-zero status must not be handed
 * to the verifier as if it were sound: its bad elements are zeros. */
int plonk_proofs_from_bytes_dev(plonk_ctx* ctx, const void* d_bytes, size_t k, void* d_proofs, void* d_status);
/* *first = the lowest i < count with a non-zero u32 at d_status + i * status_stride, -1 when there is none.  Synchronises. */
int plonk_codec_first_bad_dev(plonk_ctx* ctx, const void* d_status, size_t count, size_t status_stride, int64_t* first);
/* plonk_init for an SRS given as bytes (HOST memory, n_bases elements back to back): upload, decode into a temporary, plonk_init_dev.  One
 * bad point makes an SRS unusable: PLONK_ERR_ARG naming the first bad index and its status, and the context is left without bases. */
int plonk_init_bytes(plonk_ctx* ctx, const void* bytes, size_t n_bases, int encoding, int check_subgroup, size_t domain_size, size_t quot_domain_size);
/* G2 points as bytes, host only (the two G2 points of a verifier's key): x.c0 || x.c1 (|| y.c0 || y.c1) little-endian, Q bytes x 8 each, the
 * flags in the last byte.  "Larger y" compares c1 first and c0 on a tie.  The root in Fq2 = Fq[u]/(u^2 + 1) is taken through the norm:
 * alpha = sqrt(c0^2 + c1^2), x0 = sqrt((c0 +- alpha) / 2), x1 = c1 / (2 x0), and checked by squaring.  *status: the bits above, 2 from
 * plonk_g2_check's test, on both curves; out: 4Q u64 as for plonk_g2_mul, zeros unless *status = 0.  plonk_g2_to_bytes wants a point
 * plonk_g2_mul would accept (PLONK_ERR_ARG otherwise). */
int plonk_g2_from_bytes(int curve, const uint8_t* in, int encoding, uint64_t* out, int* status);
int plonk_g2_to_bytes(int curve, const uint64_t* in, int encoding, uint8_t* out);
/* Use n_bases points already in HBM (PLONK_BASES_XY) as the SRS without a host round trip; they are
 * re-encoded into the library's resident form (x || y as canonical R'-Montgomery residues in 32-bit words: 64 B / 96 B per point), the caller keeps its buffer. */
int plonk_init_dev(plonk_ctx* ctx, const void* d_bases_xy, size_t n_bases, size_t domain_size,
                   size_t quot_domain_size);
/* element-wise field ops on the device, for pinning the arithmetic layer.
 * field: 0 Fr, 1 Fq.  op: 0 mul, 1 add, 2 sub, 3 to_mont, 4 from_mont, 5 inverse, 6 square.  Host buffers. */
int plonk_debug_field_op(plonk_ctx* ctx, int field, int op, const uint64_t* a, const uint64_t* b,
                         uint64_t* out, size_t n);
/* tuning knobs, each stored in the context it is set on (other contexts — also ones driven from other host threads — keep theirs):
 * key "msm_window" (bits, 0 = auto), "ntt_max_log_r" (<= 9), "msm_slice_log" (8..26: MSMs above 2^value points are
 * computed slice by slice and the partial points added; default 26, for tests of the slicing path), "msm_batch_max"
 * (scalar vectors per launch set of plonk_commit_many_dev, default 32; 1 = one MSM at a time), "msm_acc_persist" (workgroups per CU of the
 * persistent bucket accumulation, default 4; 0 = one lane per bucket over the whole grid; < 0 = an absolute grid, for tests),
 * "msm_precompute" (fixed-base window table built at the next init: 0 off = default, 1 when the cost model predicts a gain, 2 whenever a usable
 * shape exists — a pinned width that is unusable for the SRS at hand falls back to no table, never to an error),
 * "msm_table_c" (0 or 4..21) / "msm_table_sets" / "msm_table_budget_mib" (the table's window width, bucket sets per scalar and memory budget;
 * 0 = the plan's choice), "msm_sort_stage_cap" (tests: caps the LDS staging buffer of the level-2 sort), "msm_sort_slice_index" (tests, default 0:
 * 1 = the level-1 sort entries carry the index within their 2^14-point slice at any size, the form that otherwise needs wide windows above 2^22
 * points), "msm_reduce_grid" (default 0: the window
 * reduction as tree sums over the bucket grid instead of the running-sum pyramid — faster for one small MSM alone, not beside another context's
 * accumulation: profiles/r04_pin_nop_experiment.txt), "msm_fused_order" (the bucket-size histogram inside the level-2 sort: 1 = for launches of
 * >= 2^23 points (default), 2 = always, 0 = never), "msm_fused_y3", "ntt_shoup" (both curves, default 1: precomputed-quotient butterflies in
 * the NTT passes; 0 = Montgomery butterflies), "ntt_coset_twiddles" (default 1: the first pass of a coset transform — plonk_coset_eval_dev classes
 * of two or more passes, the whole-vector forward coset NTT — takes its row scale in per-class butterfly twiddles instead of a product at load,
 * where the pass has the production shape: width >= 5, "ntt_shoup" on; 0 = the row-table product; same results), "ntt_plane_budget" (tests: BYTES of NTT factor planes the context may hold, < 0 = the default of
 * 48 GiB; takes effect at the next transform, frees nothing and keeps what is cached — whole-vector and distributed transforms that get no plane
 * form their factors on the fly, plonk_coset_eval_dev / plonk_fft1_dev_compact fail with PLONK_ERR_HIP), "check_bases" (default 1: plonk_init* verifies that every base is a curve point), "quotient_fuse" (6 = default: the compact kernel; 0-5, 7: other formulations).
 * INTEGRATION.md §6 has the table. */
int plonk_set_option(plonk_ctx* ctx, const char* key, int64_t value);
/* The plan the MSM engine would run for K scalar vectors over n points under this context's options (window, table, the msm_* knobs): the host-side
 * choices of kernels and layouts, computed by the function the engine itself consumes.  Nothing is launched or allocated.  An MSM above the slice
 * size or the batching limits runs as several launch sets; the plan is that of the first (PLONK_MSM_PLAN_N points, PLONK_MSM_PLAN_K vectors).
 * out receives PLONK_MSM_PLAN_FIELDS integers (n_out >= that); PLONK_ERR_ARG where the engine would refuse the MSM. */
enum {
    PLONK_MSM_PLAN_C = 0,            /* window bits */
    PLONK_MSM_PLAN_W1,               /* windows per scalar vector */
    PLONK_MSM_PLAN_G,                /* bucket sets per scalar vector (= W1 without a fixed-base table) */
    PLONK_MSM_PLAN_CB,               /* log2 buckets per window = c - 1 */
    PLONK_MSM_PLAN_LP,               /* log2 level-1 partitions per window */
    PLONK_MSM_PLAN_LOW_BITS,         /* log2 buckets per partition = cb - lp */
    PLONK_MSM_PLAN_NBLK,             /* 2^SORT_SLICE_LOG-point slices per window */
    PLONK_MSM_PLAN_IDX_BITS,         /* bits of the point index in a level-1 entry; 0 = index within the slice, slice recovered by search */
    PLONK_MSM_PLAN_PACKED,           /* 1 = the level-1 scatter carries the partition in the entry (low_bits + SORT_SLICE_LOG + 1 + lp <= 32) */
    PLONK_MSM_PLAN_STAGED,           /* 1 = LDS-staged level-2 kernel, 0 = direct */
    PLONK_MSM_PLAN_STAGE_CAP,        /* entries of the staging buffer (also reported when the direct kernel runs) */
    PLONK_MSM_PLAN_FUSED_ORDER,      /* 1 = the bucket-size histogram is taken inside the level-2 sort (effective, not the option) */
    PLONK_MSM_PLAN_NLEV,             /* levels of the reduction pyramid */
    PLONK_MSM_PLAN_LAST_K,           /* inputs per chunk of the last level (2 for odd cb, else 4; 0 without levels) */
    PLONK_MSM_PLAN_GSPLIT,           /* workgroups per (level, window) sum; > 1 adds the fold launch */
    PLONK_MSM_PLAN_HEAVY_THRESH,     /* entries above which a bucket goes to the heavy kernel */
    PLONK_MSM_PLAN_PERSISTENT,       /* 1 = accumulation as persistent waves on a work counter (depends on the device's CU count) */
    PLONK_MSM_PLAN_GRID_MODE,        /* 1 = grid reduction instead of the pyramid */
    PLONK_MSM_PLAN_STAGE_MAX_CHUNKS, /* kernel constants the data-dependent choices rest on ... */
    PLONK_MSM_PLAN_STAGE_THREADS,
    PLONK_MSM_PLAN_HEAVY_BUCKET,
    PLONK_MSM_PLAN_HEAVY_SEGS,
    PLONK_MSM_PLAN_SORT_SLICE_LOG,
    PLONK_MSM_PLAN_N,                /* points of the (first) launch set */
    PLONK_MSM_PLAN_K,                /* scalar vectors of the (first) launch set */
    PLONK_MSM_PLAN_N_CU,             /* CUs of the current device */
    PLONK_MSM_PLAN_ACC_GRID,         /* workgroups of the accumulation */
    PLONK_MSM_PLAN_BIN_SHIFT,        /* resolution of the bucket-size bins */
    PLONK_MSM_PLAN_FIELDS
};
int plonk_msm_plan(plonk_ctx* ctx, size_t n, int K, int32_t* out, int n_out);
/* Timing of the kernels launched by the last plonk_*_dev call on this context, measured with HIP
 * events on the context's stream (milliseconds). */
int plonk_last_kernel_ms(plonk_ctx* ctx, double* out_ms);

/* Per-kernel timing with HIP events recorded on the context's stream around every kernel launch
 * (off by default).  Names: "ntt_pass_kernel", "ntt_pass_kernel<9>" (per in-LDS size), "ntt_pass_coset_tw" (the passes among them that ran
 * with coset twiddles, option "ntt_coset_twiddles"), "ntt_gen_plane", "ntt_gen_epi_plane",
 * "ntt_gen_shift_plane" (the generators of the inter-pass, output-factor and shared-input first-pass planes: one launch per plane built),
 * "msm_sort" (digits, histograms, scan, both sort levels), "msm_bucket_order", "msm_accumulate_kernel", "msm_accumulate_redo_kernel", "msm_heavy",
 * "msm_reduce", "quotient_evals_kernel", "perm_terms_kernel", "perm_scan_num", "perm_scan_den_final",
 * "poly_eval_kernel", "poly_lincomb_kernel", "poly_scale_kernel", "poly_div_scan", "rccl_alltoall", "rccl_allgather" (the collective
 * as the stream saw it, waiting for peers included).  total_ms / launches accumulate until reset. */
int plonk_profile_enable(plonk_ctx* ctx, int on);
int plonk_profile_reset(plonk_ctx* ctx);
int plonk_profile_get(plonk_ctx* ctx, const char* name, double* total_ms, uint64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* PLONK_HIP_H */
