// What the 16-bit matrix-pipe conv GEMMs share (modconv_bf16.hip, upconv_fir.hip; smallconv.hip and upfir_lean.hip take the
// layout constants only).  Each piece has ONE definition and is inlined into every main loop that uses it; a main loop keeps what
// is its own: the item schedule (which tap converts which patch slot, where load_a / read_a sit relative to the MFMAs), its
// registers, and whatever could not move here without changing the compiled kernel (profiles/conv16_single_source_isa.md).
//   * LDS layout of the 16-channel loops' patch image: APITCH, RowPitch, BNB;
//   * up_items: the 9 (phase, tap) items of the merged up-conv and their four LDS shift groups;
//   * a16_load / a16_store: the 16-channel loops' patch staging (fetch; style, mask, split, store of the parts).
// The part-order table of an operand kind (kind_order) and the split itself (split4) are split_mfma.h's.
#pragma once
#include "modconv_plan.h"
#include "split_mfma.h"

namespace hfagp {

constexpr int APITCH = 48;       // LDS bytes per patch position and part: 16 bf16 + 16 B pad (3 x 16-B slots, odd)
// LDS row pitch of the patch in positions.  32 (a multiple of 16) makes every 16-lane group of a ds_read_b128
// cover 16 consecutive columns -> 16 distinct 16-B slots, no bank conflicts (the groups are {0-3,12-15,20-27},...);
// the 3-part image would not fit twice per CU at that pitch and keeps the dense one (1 extra LDS cycle per group).
template <int NP> struct RowPitch { static constexpr int value = NP <= 2 ? 32 : PW + 2; };
constexpr int BNB = 128;         // output channels per block

// The 9 (phase, tap) items of a merged up-conv chunk, grouped by their LDS shift so that each shifted A fragment is read once:
//   shift ( 0, 0): phase 0 w[0], phase 1 w[1], phase 2 w[3], phase 3 w[4]
//   shift (-1, 0): phase 0 w[6], phase 1 w[7]        shift (0,-1): phase 0 w[2], phase 2 w[5]        shift (-1,-1): phase 0 w[8]
namespace up_items {
constexpr int NITEM = 9;
constexpr int I_GRP[NITEM] = {0, 0, 0, 0, 1, 1, 2, 2, 3};
constexpr int I_PHASE[NITEM] = {0, 1, 2, 3, 0, 1, 0, 2, 0};
constexpr int I_W[NITEM] = {0, 1, 3, 4, 6, 7, 2, 5, 8};
constexpr int G_FIRST[4] = {0, 4, 6, 8};               // first item of each shift group
// patch position of tile position (0, 0) under shift group g, for a patch row pitch of lp positions
constexpr int group_pos(int g, int lp) { return (g == 0 || g == 2 ? lp : 0) + (g < 2 ? 1 : 0); }
}  // namespace up_items

// ---- patch staging of the 16-channel loops (32x32x16 MFMA, [part][position][16 ch + pad] patch image)
// fetch of the N float4 patch slots of `chunk` (fp16 storage: four halves in the low two registers)
template <bool XH, int N>
__device__ __forceinline__ void a16_load(float4 (&ra)[N], const char* xb, int chunk, const unsigned (&aoff)[N]) {
    const char* xc = xb + (long long)chunk * (CKB * (XH ? 2 : 4));
#pragma unroll
    for (int k = 0; k < N; ++k) {
        if constexpr (XH) {
            const uint2 u = *reinterpret_cast<const uint2*>(xc + aoff[k]);
            ra[k].x = __builtin_bit_cast(float, u.x);
            ra[k].y = __builtin_bit_cast(float, u.y);
        } else {
            ra[k] = *reinterpret_cast<const float4*>(xc + aoff[k]);
        }
    }
}
// one fetched slot x: scale by the style sv and the mask m (zero padding and the fp16 range guard in one factor), split, write part
// q to buf + q a_part + lds_a
template <int KD, bool XH>
__device__ __forceinline__ void a16_store(char* buf, int a_part, int lds_a, float m, const float4 sv, const float4& x) {
    constexpr int NP = kind_parts_a(KD);
    uint2 parts[NP];
    if constexpr (XH) {
        // fp16 storage: the halves are the operand already; the style (|s| <= 1 after the range guard, |x| <= the
        // layer's clamp) goes on with two packed fp16 multiplies, as EG3D's fp16 blocks do
        const f32x2 s01 = {sv.x * m, sv.y * m}, s23 = {sv.z * m, sv.w * m};
        const f16x2 x01 = __builtin_bit_cast(f16x2, __builtin_bit_cast(unsigned, x.x));
        const f16x2 x23 = __builtin_bit_cast(f16x2, __builtin_bit_cast(unsigned, x.y));
        parts[0] = make_uint2(__builtin_bit_cast(unsigned, x01 * __builtin_convertvector(s01, f16x2)),
                              __builtin_bit_cast(unsigned, x23 * __builtin_convertvector(s23, f16x2)));
    } else {
        split4<KD>(make_float4(x.x * (sv.x * m), x.y * (sv.y * m), x.z * (sv.z * m), x.w * (sv.w * m)), parts);   // (F16X2: one saturating fp16 part)
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) *reinterpret_cast<uint2*>(buf + q * a_part + lds_a) = parts[q];
}

// ---- epilogue operands of the conv GEMM loops (modconv_bf16.hip).  A lane's noise, dcoef, bias and rgb_w values are fetched as ONE
// batch in front of its first store, and neither the batch nor the store nest holds a branch: an operand that is absent is read
// through a resource of zero bytes (the load returns 0 without touching memory), a load of a row or column past the image is
// clamped into it, and the store of an element outside the image gets the offset EPI_OOB, beyond any resource (dropped by the range
// check).  Loads that sit between the stores are each waited for with vmcnt(0), which on this target drains the store in front as
// well: 64 L2 round trips in series per lane in the previous form of these epilogues.
// Only the vector offset and the instruction's immediate take part in the range check, the scalar offset does not: whatever can be
// out of range goes into the vector offset.
constexpr unsigned EPI_OOB = 0x80000000u;
// resource over `bytes` bytes at p (wave-uniform arguments); none at all for p == nullptr
__device__ __forceinline__ __amdgpu_buffer_rsrc_t epi_rsrc(const void* p, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? bytes : 0u, 0x00020000);
}
__device__ __forceinline__ float epi_load(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, byte_off, 0, 0));
}
__device__ __forceinline__ void epi_store(__amdgpu_buffer_rsrc_t r, unsigned byte_off, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, byte_off, 0, 0);
}
// the loaded value x is in its register from here on: the wait for the batch stands here, in front of the stores, and not where
// the compiler sinks the first use to (behind the stores, a wait for x is a wait for them: vmcnt retires in order)
__device__ __forceinline__ void epi_landed(float& x) { asm volatile("" : "+v"(x)); }

// the streaming up-sampling layer for Cin = 32 (upfir_lean.hip), planned and launched from upconv_fir.hip's entry points
struct LeanParams {
    const float* x; const void* wt; const float* styles; const float* dcoef; const float* noise; const float* bias;
    const float* x_absmax; const float* w_absmax; float* y_absmax; float* y;
    long long x_batch_stride;
    int B, H, W, Cout;
    int nstrip, nseg, nsteps;       // column strips of 28 output columns, row segments per strip, steps (8 output rows) per column
    int act; float noise_strength, alpha, gain, clamp;
};
bool upfir_lean_plan(const HfagpModconvArgs* a, LeanParams& lp, long long min_blocks);
int launch_upfir_lean(const HfagpModconvArgs* a, LeanParams& lp, hipStream_t s);

}  // namespace hfagp
