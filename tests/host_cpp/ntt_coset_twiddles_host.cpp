// Host build (g++, the emulation's hip_runtime.h for the qualifiers) of the folded first pass's butterfly chain for
// tests/test_ntt_coset_twiddles_host.py: ntt_butterflies<9, K, false, true, true> of csrc/ntt_kernels.hpp driven over one 512-row column in the
// order ntt_pass_kernel<9, 4, true, true, true> runs it (radix-4 steps at stages 0, 2, 4, 6, the radix-2 remainder at stage 8), with a
// snapshot of the column after every step.
#include "../../distributed_plonk_amd/csrc/ntt_kernels.hpp"
#include "../../distributed_plonk_amd/csrc/constants.h"

static const FpParams<8>& params(int curve) { return curve == 0 ? BN254_FR_PARAMS : BLS12_381_FR_PARAMS; }

template <int K>
static void chain_step(F29* col, int s0, const F29S* tab, const F29Params& fp) {
    constexpr int R = 512, RADIX = 1 << K;
    const uint32_t h = 1u << s0;
    for (uint32_t G = 0; G < R / RADIX; G++) {
        const uint32_t lo = G & (h - 1), hi = G >> s0, a0 = (hi << (s0 + K)) | lo;
        F29 v[RADIX];
        for (int k = 0; k < RADIX; k++) v[k] = col[a0 + k * h];
        ntt_butterflies<9, K, false, true, true>(v, s0, lo, nullptr, tab, fp);
        for (int k = 0; k < RADIX; k++) col[a0 + k * h] = v[k];
    }
}

extern "C" {
void get_c4p(int curve, uint32_t* out) {
    const F29Params P = f29_make_params(params(curve));
    for (int i = 0; i < 9; i++) out[i] = P.c4p[i];
}
// x: 512 x 9 limbs in natural input order (normalised); tab: 511 x (9 + 9) limbs (c, cq), stage after stage; snaps: 5 x 512 x 9 limbs, the
// column in output-row order after the steps ending at stages 2, 4, 6, 8 and 9
void coset_chain(int curve, const uint32_t* x, const uint32_t* tab, uint32_t* snaps) {
    const F29Params P = f29_make_params(params(curve));
    static F29S t[511];
    for (int e = 0; e < 511; e++) {
        for (int i = 0; i < 9; i++) { t[e].c[i] = tab[18 * e + i]; t[e].cq[i] = tab[18 * e + 9 + i]; }
        t[e].pad[0] = t[e].pad[1] = 0;
    }
    static F29 col[512];
    for (uint32_t a = 0; a < 512; a++) {
        const uint32_t row = brev(a, 9);
        for (int i = 0; i < 9; i++) col[row].l[i] = x[9 * a + i];
    }
    int snap = 0;
    auto take = [&] {
        for (int r = 0; r < 512; r++)
            for (int i = 0; i < 9; i++) snaps[(snap * 512 + r) * 9 + i] = col[r].l[i];
        snap++;
    };
    for (int s = 0; s < 8; s += 2) { chain_step<2>(col, s, t, P); take(); }
    chain_step<1>(col, 8, t, P);
    take();
}
}
