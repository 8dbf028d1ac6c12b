// Weight preparation for the 16-bit matrix-pipe kernels: a conv weight [Cout][Cin][taps] becomes the split B-operand image
// [part][tap][Cin/8][Cout][8] (bf16 or fp16 parts by operand kind, split_mfma.h) that modconv_bf16.hip, upconv_fir.hip, smallconv.hip,
// torgb_skip.hip and wgrad_bf16.hip read as MFMA fragments — one weight at a time (hfagp_weight_prep_split / _prec / _scaled) or all
// the weights of a step in one launch (hfagp_weight_prep_batch).  wp_emit is the one place that writes image bits.
#include <algorithm>
#include "split_mfma.h"

namespace hfagp {

// Scaled float16 weight images (hfagp.h "Weight images"): max |w| of the tensor first — as the bit pattern of a non-negative float,
// which orders like an unsigned integer, one atomic per block into a slot cleared before — then the prep kernels store w 2^-e
// (weight_image_exp of that maximum: exact) and leave the maximum where the consumers find it.  No host synchronisation.
__device__ __forceinline__ void publish_weight_absmax(float absmax, bool nan, float* slot) {
    unsigned m = nan ? 0x7fffffffu : __builtin_bit_cast(unsigned, absmax);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o));
    __shared__ unsigned wmax[4];
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(slot), max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
}
// (a NaN weight must not vanish in fmaxf: the slot then holds a NaN pattern, above every finite one, and e is 0)
__global__ void __launch_bounds__(256) weight_absmax_kernel(const float* __restrict__ w, long long n, float* slot) {
    float m = 0.f;
    bool nan = false;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float v = w[i];
        nan |= v != v;
        m = fmaxf(m, fabsf(v));
    }
    publish_weight_absmax(m, nan, slot);
}

// the parts of 8 consecutive K values r -> dst[q n_img + idx], q = 0 .. parts - 1 (F16X2 reads the F16X3 image: two fp16 parts of the
// weights); sc = 2^-e of a scaled float16 image, 1 otherwise
__device__ __forceinline__ void wp_emit(float (&r)[8], uint4* dst, long long n_img, long long idx, int kd, float sc) {
    if (kd == 5) kd = 4;
    if (kd == 1 || kd == 4) {
        unsigned u[4];
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] *= sc;          // (2^-e of a scaled image, 1 otherwise)
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = pack_f16(r[2 * e], r[2 * e + 1]);
        dst[idx] = make_uint4(u[0], u[1], u[2], u[3]);
        if (kd == 4) {
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = pack_f16(r[2 * e] - f16_lo_back(u[e]), r[2 * e + 1] - f16_hi_back(u[e]));
            dst[n_img + idx] = make_uint4(u[0], u[1], u[2], u[3]);
        }
        return;
    }
    float t[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = r[e];
    for (int q = 0; q < kd; ++q) {
        unsigned u[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            u[e] = pack_bf16(t[2 * e], t[2 * e + 1]);
            t[2 * e] -= __builtin_bit_cast(float, u[e] << 16);
            t[2 * e + 1] -= __builtin_bit_cast(float, u[e] & 0xffff0000u);
        }
        dst[q * n_img + idx] = make_uint4(u[0], u[1], u[2], u[3]);
    }
}

// weight [Cout][Cin][taps] -> wb [parts][taps][Cin/8][Cout][8] bf16 or fp16 (operand kind kd); thread = (tap, ci group, co)
__global__ void __launch_bounds__(256) weight_prep_split_kernel(const float* __restrict__ w, uint4* __restrict__ wb,
                                                                int Cout, int Cin, int taps, int kd, const float* w_absmax) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int cq8 = Cin >> 3;
    const long long n = (long long)taps * cq8 * Cout;
    if (idx >= n) return;
    const int co = (int)(idx % Cout);
    const int g = (int)((idx / Cout) % cq8);
    const int t = (int)(idx / ((long long)Cout * cq8));
    float r[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = w[((size_t)co * Cin + 8 * g + e) * taps + t];
    wp_emit(r, wb, n, idx, kd, ldexpf(1.f, -weight_image_exp(w_absmax)));
}

// Batched weight preparation (round 5; ABI 11): while the generator is being TUNED its weights change every step, and every step
// needs, per conv layer, the forward B-operand image, the image of the Cin/Cout TRANSPOSE for the bwd-data GEMM and wsq for the
// demodulation — 47 weight_prep_split launches + 23 weight_prep launches (which also wrote an fp32 image nobody read) = 1.2 ms of a
// 15 ms step.  Here ONE launch serves all layers: a block stages a 32 (co) x 32 (ci) x taps tile of one weight in LDS with coalesced
// reads and emits the three outputs from it — the weight is read once, every output leaves in 512-byte runs.
constexpr int kWPMax = 48;
struct WPItem { const float* w; uint4* img; uint4* img_t; float* wsq; float* amax; int Cout, Cin, taps, kd, kd_t, tile0; };
struct WPBatch { WPItem it[kWPMax]; int n; };

__global__ void __launch_bounds__(64) weight_absmax_clear_kernel(const WPBatch b) {
    if ((int)threadIdx.x < b.n && b.it[threadIdx.x].amax) *b.it[threadIdx.x].amax = 0.f;
}

// (the grid of weight_prep_batch_kernel: a block takes the same 32 x 32 x taps tile)
__global__ void __launch_bounds__(256) weight_absmax_batch_kernel(const WPBatch b) {
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i + 1].tile0) ++i;
    const WPItem& a = b.it[i];
    if (!a.amax) return;
    const int tci_n = a.Cin >> 5;
    const int tl = blockIdx.x - a.tile0, co0 = (tl / tci_n) * 32, ci0 = (tl % tci_n) * 32;
    const int row = 32 * a.taps;
    float m = 0.f;
    bool nan = false;
    for (int e = threadIdx.x; e < 32 * row; e += 256) {
        const int co = e / row, r = e - co * row;
        const float v = a.w[((size_t)(co0 + co) * a.Cin + ci0) * a.taps + r];
        nan |= v != v;
        m = fmaxf(m, fabsf(v));
    }
    publish_weight_absmax(m, nan, a.amax);
}

__global__ void __launch_bounds__(256) weight_prep_batch_kernel(const WPBatch b) {
    __shared__ float tile[32][32 * 9 + 1];                     // [co][ci * taps + t]
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i + 1].tile0) ++i;
    const WPItem& a = b.it[i];
    const float sc = ldexpf(1.f, -weight_image_exp(a.amax));
    const int tci_n = a.Cin >> 5;
    const int tl = blockIdx.x - a.tile0, co0 = (tl / tci_n) * 32, ci0 = (tl % tci_n) * 32;
    const int taps = a.taps, row = 32 * taps;
    for (int e = threadIdx.x; e < 32 * row; e += 256) {
        const int co = e / row, r = e - co * row;
        tile[co][r] = a.w[((size_t)(co0 + co) * a.Cin + ci0) * taps + r];
    }
    __syncthreads();
    const long long n_f = (long long)taps * (a.Cin >> 3) * a.Cout, n_t = (long long)taps * (a.Cout >> 3) * a.Cin;
    for (int e = threadIdx.x; e < taps * 4 * 32; e += 256) {
        const int c = e & 31, g = (e >> 5) & 3, t = e >> 7;
        float r[8];
        if (a.img) {                                           // forward image: 8 consecutive ci of (tap t, co c)
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] = tile[c][(8 * g + k) * taps + t];
            wp_emit(r, a.img, n_f, ((long long)t * (a.Cin >> 3) + (ci0 >> 3) + g) * a.Cout + co0 + c, a.kd, sc);
        }
        if (a.img_t) {                                         // image of the transpose: 8 consecutive co of (tap t, ci c)
#pragma unroll
            for (int k = 0; k < 8; ++k) r[k] = tile[8 * g + k][c * taps + t];
            wp_emit(r, a.img_t, n_t, ((long long)t * (a.Cout >> 3) + (co0 >> 3) + g) * a.Cin + ci0 + c, a.kd_t, sc);
        }
    }
    if (a.wsq)
        for (int e = threadIdx.x; e < 32 * 32; e += 256) {
            const int ci = e & 31, co = e >> 5;
            float sq = 0.f;
            for (int t = 0; t < taps; ++t) { const float v = tile[co][ci * taps + t]; sq += v * v; }
            a.wsq[(size_t)(co0 + co) * a.Cin + ci0 + ci] = sq;
        }
}

}  // namespace hfagp

using namespace hfagp;

static int weight_prep_kind(const float* weight, void* wb, float* w_absmax, int32_t Cout, int32_t Cin, int32_t taps, int kd,
                            void* stream) {
    HFAGP_REQUIRE(weight && wb, HFAGP_EBADARG, "weight_prep_split: null pointer");
    HFAGP_REQUIRE(Cin % 8 == 0 && Cout > 0 && (taps == 1 || taps == 9), HFAGP_EUNSUPPORTED,
                  "weight_prep_split: Cin=%d must be a multiple of 8, taps=%d in {1,9}", Cin, taps);
    const long long n = (long long)taps * (Cin / 8) * Cout;
    if (w_absmax) {
        HFAGP_REQUIRE(kind_f16(kd), HFAGP_EBADARG, "weight_prep_scaled: only the float16 kinds have a scaled image");
        if (hipMemsetAsync(w_absmax, 0, sizeof(float), (hipStream_t)stream) != hipSuccess) return check_launch("weight_prep_scaled");
        weight_absmax_kernel<<<(unsigned)std::min<long long>((8 * n + 1023) / 1024, 1024), 256, 0, (hipStream_t)stream>>>(
            weight, 8 * n, w_absmax);
    }
    weight_prep_split_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        weight, reinterpret_cast<uint4*>(wb), Cout, Cin, taps, kd, w_absmax);
    return check_launch("weight_prep_split");
}

extern "C" int hfagp_weight_prep_split(const float* weight, void* wb, int32_t Cout, int32_t Cin, int32_t taps,
                                       int32_t nparts, void* stream) {
    HFAGP_REQUIRE(nparts >= 1 && nparts <= 3, HFAGP_EUNSUPPORTED, "weight_prep_split: nparts=%d in {1,2,3}", nparts);
    return weight_prep_kind(weight, wb, nullptr, Cout, Cin, taps, nparts, stream);
}

extern "C" int hfagp_weight_prep_prec(const float* weight, void* wb, int32_t Cout, int32_t Cin, int32_t taps,
                                      int32_t precision, void* stream) {
    const int kd = kind_of(precision);
    HFAGP_REQUIRE(kd != 0, HFAGP_EBADARG, "weight_prep_prec: precision %d has no 16-bit weight image", precision);
    return weight_prep_kind(weight, wb, nullptr, Cout, Cin, taps, kd, stream);
}

extern "C" int hfagp_weight_prep_scaled(const float* weight, void* wb, float* w_absmax, int32_t Cout, int32_t Cin, int32_t taps,
                                        int32_t precision, void* stream) {
    const int kd = kind_of(precision);
    HFAGP_REQUIRE(kd != 0 && w_absmax, HFAGP_EBADARG, "weight_prep_scaled: precision %d / null w_absmax", precision);
    return weight_prep_kind(weight, wb, w_absmax, Cout, Cin, taps, kd, stream);
}

extern "C" int hfagp_weight_prep_batch(const HfagpWeightPrepItem* items, int32_t n, void* stream) {
    HFAGP_REQUIRE(items && n >= 1 && n <= kWPMax, HFAGP_EBADARG, "weight_prep_batch: 1..%d items", kWPMax);
    WPBatch b;
    int tiles = 0;
    bool any_scaled = false;
    for (int i = 0; i < n; ++i) {
        const HfagpWeightPrepItem& a = items[i];
        HFAGP_REQUIRE(a.weight && (a.image || a.image_t || a.wsq), HFAGP_EBADARG, "weight_prep_batch: null pointer (item %d)", i);
        HFAGP_REQUIRE(a.Cout % 32 == 0 && a.Cin % 32 == 0 && (a.taps == 1 || a.taps == 9), HFAGP_EUNSUPPORTED,
                      "weight_prep_batch: item %d: Cout=%d, Cin=%d must be multiples of 32, taps=%d in {1,9}", i, a.Cout, a.Cin, a.taps);
        const int kd = a.image ? kind_of(a.precision) : 0, kd_t = a.image_t ? kind_of(a.precision_t) : 0;
        HFAGP_REQUIRE((!a.image || kd != 0) && (!a.image_t || kd_t != 0), HFAGP_EBADARG,
                      "weight_prep_batch: item %d: precision without a 16-bit weight image", i);
        // (max |w| only where a float16 image of the item will be scaled by it)
        float* amax = (kind_f16(kd) || kind_f16(kd_t)) ? a.w_absmax : nullptr;
        any_scaled |= amax != nullptr;
        b.it[i] = WPItem{a.weight, reinterpret_cast<uint4*>(a.image), reinterpret_cast<uint4*>(a.image_t), a.wsq, amax, a.Cout, a.Cin,
                         a.taps, kd, kd_t, tiles};
        tiles += (a.Cout / 32) * (a.Cin / 32);
    }
    b.n = n;
    if (any_scaled) {
        weight_absmax_clear_kernel<<<1, 64, 0, (hipStream_t)stream>>>(b);
        weight_absmax_batch_kernel<<<(unsigned)tiles, 256, 0, (hipStream_t)stream>>>(b);
    }
    weight_prep_batch_kernel<<<(unsigned)tiles, 256, 0, (hipStream_t)stream>>>(b);
    return check_launch("weight_prep_batch");
}
