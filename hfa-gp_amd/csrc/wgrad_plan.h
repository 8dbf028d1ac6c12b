// Host plan of the weight-gradient kernels (exact fp32 wgrad.hip, split-bf16 wgrad_bf16.hip): the tiles, which kernel runs, the
// split-K policy.  gfx950 only.
#pragma once
#include "common.h"

namespace hfagp {

constexpr int TPH = 2, TPW = 16, WT = 64;        // wgrad.hip: position tile (rows x columns), ci / co tile
constexpr int QH = 4, QW = 16, CT = 64;          // wgrad_bf16.hip: the same

// wgrad_bf16.hip: the 3x3 conv / all nine taps of the up-sampling conv in one launch; slabs [ksplit][Cout][Cin][9] in a->workspace
int launch_wgrad3x3_bf16(const HfagpWgradArgs* a, hipStream_t s);
int launch_wgrad_up_bf16(const HfagpWgradArgs* a, hipStream_t s);

// Whether the split-bf16 kernels take the call (hfagp.h, HfagpWgradArgs::precision): whole 64-channel tiles; the up-sampling
// kernel also takes the partial ci tile of the first super-resolution layer (Cin = 32).  Everything else runs in exact fp32.
static inline bool wgrad_split16(const HfagpWgradArgs* a) {
    const bool up = a->mode == HFAGP_CONVT3X3_UP2;
    return a->precision == HFAGP_PREC_BF16X3 && (a->mode == HFAGP_CONV3X3 || up) && a->Cout % CT == 0 &&
           (a->Cin % CT == 0 || (up && a->Cin == 32));
}

// row stride of dd in elements (ABI 12: 0 = Cout)
static inline int wgrad_dd_stride(const HfagpWgradArgs* a) { return a->dd_stride > 0 ? a->dd_stride : a->Cout; }

// split-K policy (ABI 11; the host used to carry a copy of it): one resident block per CU for the split-bf16 kernel (measured 5 %
// better than two rounds: half the slabs to write and reduce), two rounds for the fp32 one; never more slabs than position tiles
// of the kernel that will run
static inline int32_t wgrad_ksplit_policy(const HfagpWgradArgs* a) {
    const bool split16 = wgrad_split16(a);
    const int rows = split16 ? QH : TPH, cols = split16 ? QW : TPW;
    const long long units = (long long)a->B * ((a->H + rows - 1) / rows) * ((a->W + cols - 1) / cols);
    const long long tiles = (long long)((a->Cin + CT - 1) / CT) * ((a->Cout + CT - 1) / CT);
    const long long want = (split16 ? kNumCU : 2 * kNumCU) / (tiles > 0 ? tiles : 1);
    long long k = want < 1 ? 1 : want;
    if (k > units) k = units;
    if (k > 256) k = 256;
    return (int32_t)(k < 1 ? 1 : k);
}

}  // namespace hfagp
