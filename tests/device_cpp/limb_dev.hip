// Device build (hipcc, gfx950) of the hot path's limb arithmetic for tests/test_gpu_limb_arith.py — TEST INFRASTRUCTURE, no entry point of
// the C ABI.  tests/host_cpp/fp29_host.cpp and ec_lazy_host.cpp run csrc/fp29.hpp, flimb.hpp and ec_lazy.hpp as g++ compiles them; this file
// runs the same functions as gfx950 code: the accumulator pins (F29_CHAIN / FL_CHAIN) exist only there, and the column sums become chains of
// v_mad_u64_u32 only there.  Same operation set and buffer layouts as the two host files, batched: one element per lane, 256 lanes per
// workgroup, a tail guard, one kernel instantiation per operation (the compiler sees one formula per kernel, as inside the MSM kernels).
// Every entry point allocates its device buffers, copies in, launches, synchronises, copies out, frees, and returns the HIP status.
// tests/device_cpp/build.py also compiles it with g++ against tests/hostemu/hip/hip_runtime.h, which checks the harness where no GPU exists.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../distributed_plonk_amd/csrc/fp29.hpp"
#include "../../distributed_plonk_amd/csrc/ec_lazy.hpp"
#include "../../distributed_plonk_amd/csrc/constants.h"

namespace {
constexpr uint32_t LANES = 256;

// ---------------------------------------------------------------------------------------------- limb loads / stores
template <int NL, int B> FP_HD FL<NL, B> ld(const uint32_t* s) {
    FL<NL, B> r;
    for (int i = 0; i < NL; i++) r.l[i] = s[i];
    return r;
}
template <int NL, int B> FP_HD void st(uint32_t* d, const FL<NL, B>& a) {
    for (int i = 0; i < NL; i++) d[i] = a.l[i];
}
template <int NL, int B> FP_HD XyzzL<NL, B> ld4(const uint32_t* s) {
    XyzzL<NL, B> r;
    r.x = ld<NL, B>(s); r.y = ld<NL, B>(s + NL); r.zz = ld<NL, B>(s + 2 * NL); r.zzz = ld<NL, B>(s + 3 * NL);
    return r;
}
template <int NL, int B> FP_HD void st4(uint32_t* d, const XyzzL<NL, B>& a) {
    st(d, a.x); st(d + NL, a.y); st(d + 2 * NL, a.zz); st(d + 3 * NL, a.zzz);
}
template <int NL, int B> FP_HD AffL<NL, B> ld2(const uint32_t* s) {
    AffL<NL, B> r;
    r.x = ld<NL, B>(s); r.y = ld<NL, B>(s + NL);
    return r;
}
FP_HD F29 ld29(const uint32_t* s) {
    F29 r;
    for (int i = 0; i < 9; i++) r.l[i] = s[i];
    return r;
}
FP_HD void st29(uint32_t* d, const F29& a) {
    for (int i = 0; i < 9; i++) d[i] = a.l[i];
}

// ---------------------------------------------------------------------------------------------- kernels: fp29.hpp
// the parameters travel as the NTT pass kernel receives them: by value, in the kernel arguments
__global__ void __launch_bounds__(256) pbar_kernel(uint32_t* out, const F29Params P) {
    if (blockIdx.x == 0 && threadIdx.x < 9) out[threadIdx.x] = P.pbar[threadIdx.x];
}
// prepared constants as the pass kernel reads them from its table (F29S records)
__global__ void __launch_bounds__(256) shoup_const_kernel(const F29S* tab, uint32_t* c29, uint32_t* cq29, uint64_t n) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    for (int i = 0; i < 9; i++) { c29[9 * k + i] = tab[k].c[i]; cq29[9 * k + i] = tab[k].cq[i]; }
}
// OP: 0 f29_mul_shoup(x, c, cq), 1 f29_mul(x, c), 2 f29_canon_lazy(x)
template <int OP>
__global__ void __launch_bounds__(256) fr_op_kernel(const uint32_t* x, const uint32_t* c, const uint32_t* cq, uint32_t* r, uint64_t n, const F29Params P) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    const F29 a = ld29(x + 9 * k);
    F29 o;
    if constexpr (OP == 0) o = f29_mul_shoup(a, c + 9 * k, cq + 9 * k, P);
    else if constexpr (OP == 1) o = f29_mul(a, ld29(c + 9 * k), P);
    else o = f29_canon_lazy(a, P);
    st29(r + 9 * k, o);
}

// ---------------------------------------------------------------------------------------------- kernels: flimb.hpp / ec_lazy.hpp
// the parameters travel as the MSM kernels receive them: FLParams by value
template <int NL, int B> __global__ void __launch_bounds__(256) params_kernel(uint32_t* out, const FLParams<NL, B> P) {
    if (blockIdx.x != 0 || threadIdx.x >= (uint32_t)NL) return;
    const uint32_t* rows[8] = {P.p, P.p2, P.c2, P.c4, P.c8, P.one, P.r_std, P.r2fix};
    for (int r = 0; r < 8; r++) out[r * NL + threadIdx.x] = rows[r][threadIdx.x];
    if (threadIdx.x == 0) out[8 * NL] = P.inv;
}
// OP: 0 mul(a, b), 1 sqr(a), 2 dot2(a, b, c, d)
template <int NL, int B, int OP>
__global__ void __launch_bounds__(256) field_op_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r, uint64_t n,
                                                       const FLParams<NL, B> P) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    const FL<NL, B> x = ld<NL, B>(a + k * NL);
    FL<NL, B> o;
    if constexpr (OP == 0) o = fl_mul(x, ld<NL, B>(b + k * NL), P);
    else if constexpr (OP == 1) o = fl_sqr(x, P);
    else o = fl_dot2(x, ld<NL, B>(b + k * NL), ld<NL, B>(c + k * NL), ld<NL, B>(d + k * NL), P);
    st(r + k * NL, o);
}
// the second operand of add (3), add_fast (4) and dbl (5) is an accumulator of 4 NL limbs, of every other operation an affine point of 2 NL
constexpr int curve_b_limbs(int op, int NL) { return (op >= 3 && op <= 5 ? 4 : 2) * NL; }
// OP: 0 madd_fast (plain Y3), 1 madd_fast (fused Y3), 2 madd (complete), 3 add (complete), 4 add_fast, 5 dbl, 6 dbl_affine, 7 neg (affine)
// a: n accumulators (4 NL limbs each), b: n operands (curve_b_limbs), out: n x 4 NL limbs (neg writes the first 2 NL), flag: the fast paths' result
template <int NL, int B, int OP>
__global__ void __launch_bounds__(256) curve_op_kernel(const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* flag, uint64_t n, const FLParams<NL, B> P) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    XyzzL<NL, B> acc = ld4<NL, B>(a + k * 4 * NL);
    const uint32_t* bk = b + k * curve_b_limbs(OP, NL);
    uint32_t* dst = out + k * 4 * NL;
    bool ok = true;
    if constexpr (OP == 0) ok = xyzzl_madd_fast<NL, B, false>(acc, ld2<NL, B>(bk), P);
    else if constexpr (OP == 1) ok = xyzzl_madd_fast<NL, B, true>(acc, ld2<NL, B>(bk), P);
    else if constexpr (OP == 2) acc = xyzzl_madd(acc, ld2<NL, B>(bk), P);
    else if constexpr (OP == 3) acc = xyzzl_add(acc, ld4<NL, B>(bk), P);
    else if constexpr (OP == 4) ok = xyzzl_add_fast(acc, ld4<NL, B>(bk), P);
    else if constexpr (OP == 5) acc = xyzzl_dbl(acc, P);
    else if constexpr (OP == 6) acc = xyzzl_dbl_affine(ld2<NL, B>(bk), P);
    else {
        const AffL<NL, B> q = affl_neg(ld2<NL, B>(bk), P);
        st(dst, q.x); st(dst + NL, q.y);
        flag[k] = 1;
        return;
    }
    st4(dst, acc);
    flag[k] = ok ? 1 : 0;
}
// saturated Montgomery (R = 2^(32N), the reference's form) <-> limb form (R' = 2^(B NL)): what bases_to_limbs_kernel / store_std do
template <int NL, int B, int N>
__global__ void __launch_bounds__(256) from_std_kernel(const uint32_t* s, uint32_t* out, uint64_t n, const FLParams<NL, B> P) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    Fp<N> a;
    for (int i = 0; i < N; i++) a.l[i] = s[k * N + i];
    st(out + k * NL, fl_canon_lt2p(fl_mul(fl_from_sat<NL, B, N>(a), ld<NL, B>(P.r2fix), P), P));
}
template <int NL, int B, int N>
__global__ void __launch_bounds__(256) to_std_kernel(const uint32_t* s, uint32_t* out, uint64_t n, const FLParams<NL, B> P) {
    const uint64_t k = (uint64_t)blockIdx.x * LANES + threadIdx.x;
    if (k >= n) return;
    const FL<NL, B> v = fl_canon_lt2p(fl_mul(ld<NL, B>(s + k * NL), ld<NL, B>(P.r_std), P), P);
    const Fp<N> o = fl_to_sat<NL, B, N>(v);
    for (int i = 0; i < N; i++) out[k * N + i] = o.l[i];
}

// ---------------------------------------------------------------------------------------------- host side
// The device buffers of one call: inputs are copied in when they are added, outputs start as zeros and are copied back by finish(),
// which also frees everything.  The first HIP error sticks and is what the entry point returns; nothing is launched after one.
class Io {
    struct Out { void* d; void* h; size_t bytes; };
    std::vector<void*> all_;
    std::vector<Out> outs_;
    hipError_t err_;
    void note(hipError_t e) { if (err_ == hipSuccess) err_ = e; }
    void* alloc(size_t bytes) {
        void* d = nullptr;
        if (err_ != hipSuccess) return nullptr;
        note(hipMalloc(&d, bytes ? bytes : 4));
        if (d != nullptr) all_.push_back(d);
        return d;
    }
public:
    explicit Io(int dev) : err_(hipSetDevice(dev)) {}
    bool ok() const { return err_ == hipSuccess; }
    template <typename T> const T* in(const T* h, size_t count) {
        if (h == nullptr) return nullptr;
        void* d = alloc(count * sizeof(T));
        if (d != nullptr && count) note(hipMemcpy(d, h, count * sizeof(T), hipMemcpyHostToDevice));
        return (const T*)d;
    }
    template <typename T> T* out(T* h, size_t count) {
        void* d = alloc(count * sizeof(T));
        if (d != nullptr) {
            note(hipMemset(d, 0, count * sizeof(T)));
            outs_.push_back({d, h, count * sizeof(T)});
        }
        return (T*)d;
    }
    int finish() {
        note(hipGetLastError());
        note(hipDeviceSynchronize());
        for (const Out& o : outs_)
            if (err_ == hipSuccess && o.bytes) note(hipMemcpy(o.h, o.d, o.bytes, hipMemcpyDeviceToHost));
        for (void* d : all_) (void)hipFree(d);
        return (int)err_;
    }
};
dim3 grid_for(long n) { return dim3((uint32_t)(((uint64_t)n + LANES - 1) / LANES)); }

const FpParams<8>& fr_params(int curve) { return curve == 0 ? BN254_FR_PARAMS : BLS12_381_FR_PARAMS; }
// the same construction msm_engine.hip uses (fl_params<NQ>)
const FLParams<9, 29>& bn() {
    static const FLParams<9, 29> P = fl_make_params<9, 29, 8>(BN254_FQ_PARAMS);
    return P;
}
const FLParams<14, 28>& bls() {
    static const FLParams<14, 28> P = fl_make_params<14, 28, 12>(BLS12_381_FQ_PARAMS);
    return P;
}

template <int OP> int fr_op(int dev, int curve, const uint32_t* x, const uint32_t* c, const uint32_t* cq, uint32_t* r, long n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    Io io(dev);
    const uint32_t* dx = io.in(x, 9 * (size_t)n);
    const uint32_t* dc = io.in(c, 9 * (size_t)n);
    const uint32_t* dq = io.in(cq, 9 * (size_t)n);
    uint32_t* dr = io.out(r, 9 * (size_t)n);
    if (io.ok() && n > 0)
        hipLaunchKernelGGL((fr_op_kernel<OP>), grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, dx, dc, dq, dr, (uint64_t)n, f29_make_params(fr_params(curve)));
    return io.finish();
}

template <int NL, int B> int params(int dev, const FLParams<NL, B>& P, uint32_t* out) {
    Io io(dev);
    uint32_t* d = io.out(out, 8 * NL + 1);
    if (io.ok()) hipLaunchKernelGGL((params_kernel<NL, B>), dim3(1), dim3(LANES), 0, (hipStream_t) nullptr, d, P);
    return io.finish();
}

template <int NL, int B, int OP>
void launch_field(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r, long n, const FLParams<NL, B>& P) {
    hipLaunchKernelGGL((field_op_kernel<NL, B, OP>), grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, a, b, c, d, r, (uint64_t)n, P);
}
template <int NL, int B>
int field_op(int dev, const FLParams<NL, B>& P, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r, long n) {
    if (n < 0 || op < 0 || op > 2 || a == nullptr || (op != 1 && b == nullptr) || (op == 2 && (c == nullptr || d == nullptr))) return (int)hipErrorInvalidValue;
    Io io(dev);
    const size_t w = (size_t)NL * (size_t)n;
    const uint32_t* da = io.in(a, w);
    const uint32_t* db = op != 1 ? io.in(b, w) : nullptr;
    const uint32_t* dc = op == 2 ? io.in(c, w) : nullptr;
    const uint32_t* dd = op == 2 ? io.in(d, w) : nullptr;
    uint32_t* dr = io.out(r, w);
    if (io.ok() && n > 0) {
        if (op == 0) launch_field<NL, B, 0>(da, db, dc, dd, dr, n, P);
        else if (op == 1) launch_field<NL, B, 1>(da, db, dc, dd, dr, n, P);
        else launch_field<NL, B, 2>(da, db, dc, dd, dr, n, P);
    }
    return io.finish();
}

template <int NL, int B, int OP> void launch_curve(const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* flag, long n, const FLParams<NL, B>& P) {
    hipLaunchKernelGGL((curve_op_kernel<NL, B, OP>), grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, a, b, out, flag, (uint64_t)n, P);
}
template <int NL, int B> int curve_op(int dev, const FLParams<NL, B>& P, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* flag, long n) {
    if (n < 0 || op < 0 || op > 7 || a == nullptr || b == nullptr) return (int)hipErrorInvalidValue;
    Io io(dev);
    const uint32_t* da = io.in(a, 4 * (size_t)NL * (size_t)n);
    const uint32_t* db = io.in(b, (size_t)curve_b_limbs(op, NL) * (size_t)n);
    uint32_t* dout = io.out(out, 4 * (size_t)NL * (size_t)n);
    int32_t* dflag = io.out(flag, (size_t)n);
    if (io.ok() && n > 0) {
        switch (op) {
        case 0: launch_curve<NL, B, 0>(da, db, dout, dflag, n, P); break;
        case 1: launch_curve<NL, B, 1>(da, db, dout, dflag, n, P); break;
        case 2: launch_curve<NL, B, 2>(da, db, dout, dflag, n, P); break;
        case 3: launch_curve<NL, B, 3>(da, db, dout, dflag, n, P); break;
        case 4: launch_curve<NL, B, 4>(da, db, dout, dflag, n, P); break;
        case 5: launch_curve<NL, B, 5>(da, db, dout, dflag, n, P); break;
        case 6: launch_curve<NL, B, 6>(da, db, dout, dflag, n, P); break;
        default: launch_curve<NL, B, 7>(da, db, dout, dflag, n, P); break;
        }
    }
    return io.finish();
}

template <int NL, int B, int N> int std_conv(int dev, const FLParams<NL, B>& P, bool to, const uint32_t* s, uint32_t* out, long n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    Io io(dev);
    const uint32_t* ds = io.in(s, (size_t)(to ? NL : N) * (size_t)n);
    uint32_t* dout = io.out(out, (size_t)(to ? N : NL) * (size_t)n);
    if (io.ok() && n > 0) {
        if (to) hipLaunchKernelGGL((to_std_kernel<NL, B, N>), grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, ds, dout, (uint64_t)n, P);
        else hipLaunchKernelGGL((from_std_kernel<NL, B, N>), grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, ds, dout, (uint64_t)n, P);
    }
    return io.finish();
}
}  // namespace

extern "C" {
// n constants in the reference's Montgomery form (n x 8 u32) -> prepared constants c, cq (n x 9 limbs each): prepared on the host by the
// function the NTT tables are built with, uploaded as F29S records, read back through a kernel
int shoup_const(int dev, int curve, const uint32_t* c_mont, uint32_t* c29, uint32_t* cq29, long n) {
    if (n < 0) return (int)hipErrorInvalidValue;
    std::vector<F29S> tab((size_t)n);
    for (long k = 0; k < n; k++) {
        Fp<8> c;
        for (int i = 0; i < 8; i++) c.l[i] = c_mont[8 * k + i];
        tab[(size_t)k] = f29_shoup_from_mont256(c, fr_params(curve));
    }
    Io io(dev);
    const F29S* dt = io.in(tab.data(), (size_t)n);
    uint32_t* dc = io.out(c29, 9 * (size_t)n);
    uint32_t* dq = io.out(cq29, 9 * (size_t)n);
    if (io.ok() && n > 0) hipLaunchKernelGGL(shoup_const_kernel, grid_for(n), dim3(LANES), 0, (hipStream_t) nullptr, dt, dc, dq, (uint64_t)n);
    return io.finish();
}
int get_pbar(int dev, int curve, uint32_t* out) {
    Io io(dev);
    uint32_t* d = io.out(out, 9);
    if (io.ok()) hipLaunchKernelGGL(pbar_kernel, dim3(1), dim3(LANES), 0, (hipStream_t) nullptr, d, f29_make_params(fr_params(curve)));
    return io.finish();
}
// n products: x (n x 9 limbs, lazy), c / cq (n x 9) -> r (n x 9)
int shoup_mul(int dev, int curve, const uint32_t* x, const uint32_t* c, const uint32_t* cq, uint32_t* r, long n) { return fr_op<0>(dev, curve, x, c, cq, r, n); }
// the Montgomery multiplier on the same operands: x * (c * 2^261 mod p) / 2^261
int mont_mul(int dev, int curve, const uint32_t* x, const uint32_t* cm, uint32_t* r, long n) { return fr_op<1>(dev, curve, x, cm, nullptr, r, n); }
// normalised values below 48p -> canonical
int canon_lazy(int dev, int curve, const uint32_t* x, uint32_t* r, long n) { return fr_op<2>(dev, curve, x, nullptr, nullptr, r, n); }

int ecl_params(int dev, int curve, uint32_t* out) { return curve == 0 ? params(dev, bn(), out) : params(dev, bls(), out); }
int ecl_field_op(int dev, int curve, int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d, uint32_t* r, long n) {
    return curve == 0 ? field_op(dev, bn(), op, a, b, c, d, r, n) : field_op(dev, bls(), op, a, b, c, d, r, n);
}
int ecl_curve_op(int dev, int curve, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, int32_t* flag, long n) {
    return curve == 0 ? curve_op(dev, bn(), op, a, b, out, flag, n) : curve_op(dev, bls(), op, a, b, out, flag, n);
}
int ecl_from_std(int dev, int curve, const uint32_t* s, uint32_t* out, long n) {
    return curve == 0 ? std_conv<9, 29, 8>(dev, bn(), false, s, out, n) : std_conv<14, 28, 12>(dev, bls(), false, s, out, n);
}
int ecl_to_std(int dev, int curve, const uint32_t* s, uint32_t* out, long n) {
    return curve == 0 ? std_conv<9, 29, 8>(dev, bn(), true, s, out, n) : std_conv<14, 28, 12>(dev, bls(), true, s, out, n);
}
}
