// The adjoint of the tri-plane decoder, once: what every kernel that differentiates through gather -> decoder shares
// (raymarch_bwd.hip: tiles / cols / df; raymarch_camera.hip; planes_query_bwd.hip; raymarch_normals.hip).  Each fp32 piece sits
// next to its 16-bit sibling.  The kernels keep what is theirs: schedule, software pipeline, what they do with dL/dF.
//   decoder_images_lds      wave 0: the forward decoder image (fp32 or split fp16) into LDS
//   build_grad[16]_lds      the A operands of the two backward products into LDS
//   gather8_mfma            gather in the forward's quad layout, shuffled to the MFMA layout
//   colour_logit_grad       dL/d(colour logit) from the upstream colour gradient
//   decoder_bwd[16]_lds     dH, dF from dO, d sigma and the saved pre-activations
//   dec_grad_*              decoder-parameter gradients (PG): per-tile operand images + 64 MFMAs, one flush per wave
//   publish_df / publish_taps / scatter_tile_runs    dL/dF -> d planes by run-merged 128-byte atomics
//   gather_position_grad    positional derivative of the bilinear gather
//   gather_position_cross_grad   the same plus the mixed second derivative of the tap weights, one read of the texels;
//   decoder_dh_lds          dH alone (raymarch_normals_camera.hip)
//   publish_taps2 / scatter_tile_runs2 / w0_mul / w0t_mul / nrm_grad_*     second order (raymarch_normals_bwd.hip): the scatter
//                           with two value / weight sets, the fp32 products with W0', the weight-gradient sums
//   build_w0_lds            the fp32 A operands of W0' for w0_mul next to a 16-bit forward image (planes_query_normals_bwd.hip)
#pragma once
#include "raymarch_common.h"

namespace hfagp {

// ---------------------------------------------------------------- LDS images
template <bool DEC16>
__device__ __forceinline__ void decoder_images_lds(const HfagpRaymarchArgs& a, float* wfwd, int lane, int j, int g) {
    DecoderRegs dec;
    load_decoder(a, j, g, dec);
    if constexpr (DEC16) {
        Dec16Regs d16;
        make_dec16(dec, a.planes_absmax, lane, d16);
        store_dec16_lds(d16, wfwd, lane);
    } else {
        store_decoder_lds(dec, wfwd, lane);
    }
}

// A operands of the two fp32 backward products, lane-linear ([step][lane]: conflict-free ds_read_b32), built by all `nthreads`
// threads of the block:   w1t[mt][ot*4+r][lane] = W1[1 + 16ot + 4g + r][16mt + j] * g1     (4 * 8 * 64 floats)
//                         w0t[ft][mt*4+r][lane] = W0[16mt + 4g + r][16ft + j] * g0         (2 * 16 * 64 floats)
// COLOUR = false: w0t alone (as build_grad16_lds<false>); w1t is not touched.
template <bool COLOUR = true>
__device__ __forceinline__ void build_grad_lds(const HfagpRaymarchArgs& a, float* w1t, float* w0t, int tid, int nthreads) {
    const float g0 = a.decoder_lr_mul * 0.17677669529663687f, g1 = a.decoder_lr_mul * 0.125f;
    if constexpr (COLOUR) {
        for (int i = tid; i < 4 * 8 * 64; i += nthreads) {
            const int l = i & 63, st = (i >> 6) & 7, mt = i >> 9, jj = l & 15, gg = l >> 4;
            w1t[i] = a.dec_w1[(1 + 16 * (st >> 2) + 4 * gg + (st & 3)) * 64 + 16 * mt + jj] * g1;
        }
    }
    for (int i = tid; i < 2 * 16 * 64; i += nthreads) {
        const int l = i & 63, st = (i >> 6) & 15, ft = i >> 10, jj = l & 15, gg = l >> 4;
        w0t[i] = a.dec_w0[(16 * (st >> 2) + 4 * gg + (st & 3)) * 32 + 16 * ft + jj] * g0;
    }
}

// Gradient A operands (split bf16: a gradient needs fp32's exponent range; ~2^-16 per product is ample for a gradient):
//   g1img rows mt*4+q (hi), 16+mt*4+q (lo):        A[16mt + j][k = (g, c)] = W1[1 + 16(c>>2) + 4g + (c&3)][16mt + j] * g1
//   g0img rows (ft*2+ks)*4+q (hi), 16+... (lo):    A[16ft + j][k = (g, c)] = W0[16(2ks + (c>>2)) + 4g + (c&3)][16ft + j] * g0
// built by whichever waves the block has (`wave` of `nwaves`).  COLOUR = false: g0img alone (a caller without colour gradients:
// raymarch_normals.hip); g1img is not touched.
template <bool COLOUR = true>
__device__ __forceinline__ void build_grad16_lds(const HfagpRaymarchArgs& a, float* g1img, float* g0img, int lane, int wave,
                                                 int nwaves) {
    const int j = lane & 15, g = lane >> 4;
    const float g0 = a.decoder_lr_mul * 0.17677669529663687f, g1 = a.decoder_lr_mul * 0.125f;
    unsigned* i1 = reinterpret_cast<unsigned*>(g1img);
    unsigned* i0 = reinterpret_cast<unsigned*>(g0img);
    for (int t = (COLOUR ? 0 : 4) + wave; t < 8; t += nwaves) {
        float v[8];
        u32x4r hi, lo;
        if (t < 4) {
            const int mt = t;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = a.dec_w1[(1 + 16 * (c >> 2) + 4 * g + (c & 3)) * 64 + 16 * mt + j] * g1;
            split8_bf16(v, hi, lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) { i1[(mt * 4 + q) * 64 + lane] = hi[q]; i1[(16 + mt * 4 + q) * 64 + lane] = lo[q]; }
        } else {
            const int ft = (t - 4) >> 1, ks = (t - 4) & 1;
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = a.dec_w0[(16 * (2 * ks + (c >> 2)) + 4 * g + (c & 3)) * 32 + 16 * ft + j] * g0;
            split8_bf16(v, hi, lo);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                i0[((ft * 2 + ks) * 4 + q) * 64 + lane] = hi[q];
                i0[(16 + (ft * 2 + ks) * 4 + q) * 64 + lane] = lo[q];
            }
        }
    }
}

// ---------------------------------------------------------------- gather in the MFMA layout
// quad layout (lane 4q + r: sample q, channel group r) -> MFMA layout (lane 16g + j: sample j, channel group g)
__device__ __forceinline__ void quad_to_mfma(float f[8], int lane) {
    const int src = 4 * (lane & 15) + (lane >> 4);
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = __shfl(f[c], src);
}
// gather in the quad layout of raymarch_kernel (4 adjacent lanes per texel line; zq = the depth of sample lane >> 2), then to
// the MFMA layout
__device__ __forceinline__ void gather8_mfma(const RayParams& p, int b, const float o3[3], const float d3[3], float zq, int lane,
                                             float f[8]) {
    PlaneTaps tq[3];
    sample_taps(p, o3, d3, zq, tq);
    gather8(p.a, b, lane & 3, tq, f);
    quad_to_mfma(f, lane);
}

// ---------------------------------------------------------------- decoder adjoint
// dL/do (colour logits) in the C layout: lane (j, g), register r of tile ot -> channel 16ot + 4g + r
//   colour = sigmoid(o) * 1.002 - 0.001;  up = dL/dcolour of that register (the product below associates left to right)
__device__ __forceinline__ void colour_logit_grad(const f32x4 o[2], const float up[2][4], f32x4 dO[2]) {
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sg = sigmoid_f(o[ot][r]);
            dO[ot][r] = up[ot][r] * 1.002f * sg * (1.f - sg);
        }
}
// the ray kernels' upstream:  dL/dcolour = omega * 2 dL/dfeat  (gfeat: load_g_feat4 of channels 16ot + 4g ..)
__device__ __forceinline__ void ray_colour_logit_grad(const f32x4 o[2], float omega, const float4 gfeat[2], f32x4 dO[2]) {
    float up[2][4];
#pragma unroll
    for (int ot = 0; ot < 2; ++ot) {
        const float gv[4] = {gfeat[ot].x, gfeat[ot].y, gfeat[ot].z, gfeat[ot].w};
#pragma unroll
        for (int r = 0; r < 4; ++r) up[ot][r] = omega * 2.f * gv[r];
    }
    colour_logit_grad(o, up, dO);
}

// decoder backward on the fp32 matrix pipe (32 + 32 v_mfma_f32_16x16x4_f32), same signature as decoder_bwd16_lds below:
//   dH^T[64x16] = W1c^T . dO^T + wsig (x) dsigma, times sigmoid(Hpre)      A[i][k] = W1[1 + c(k)][16mt + i],  c(k) = 16ot + 4g + r
//   dF^T[32x16] = W0^T . dH^T                                              A[i][k] = W0[16mt + 4g + r][16ft + i]
// dimg: the DecoderRegs image (store_decoder_lds).  COLOUR = false: dO and w1t are not read.
// (the lane is added to each image's base FIRST, as decoder_fwd_lds does: base + constant is the form whose constant folds into
// the ds_read offset; with  w1t[step * 64 + lane]  raymarch_bwd_camera_kernel<96, false> needs 170 registers instead of 167 and
// loses its third wave per SIMD)
template <bool COLOUR = true>
__device__ __forceinline__ void decoder_bwd_lds(const float* dimg, const float* w1t, const float* w0t, int lane,
                                                const f32x4 dO[2], float dsig, const f32x4 hp[4], f32x4 dH[4], f32x4 dF[2]) {
    const float* W1 = w1t + lane;
    const float* W0 = w0t + lane;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float* ws_ = dimg + (kDecWsig + mt * 4) * 64 + lane;
        dH[mt] = f32x4{ws_[0] * dsig, ws_[64] * dsig, ws_[128] * dsig, ws_[192] * dsig};
        if constexpr (COLOUR) {
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float wA = W1[(mt * 8 + ot * 4 + r) * 64];
                    dH[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wA, dO[ot][r], dH[mt], 0, 0, 0);
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) dH[mt][r] *= sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
    }
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
        dF[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float wA = W0[(ft * 16 + mt * 4 + r) * 64];
                dF[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(wA, dH[mt][r], dF[ft], 0, 0, 0);
            }
    }
}

// decoder backward on the 16-bit pipe: dH (pre-activation gradient, C layout of the hidden tiles) and dF (C layout of the
// two feature tiles) from dO (colour-logit gradients), d sigma, the saved pre-activations.  COLOUR = false: dO is all zeros
// (the adjoint of sigma alone); dO and g1img are not read and the second-layer colour product is not formed.
template <bool COLOUR = true>
__device__ __forceinline__ void decoder_bwd16_lds(const float* dimg, const float* g1img, const float* g0img, int lane,
                                                  const f32x4 dO[2], float dsig, const f32x4 hp[4], f32x4 dH[4], f32x4 dF[2]) {
    u32x4r oh = {}, ol = {};
    if constexpr (COLOUR) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = dO[c >> 2][c & 3];
        split8_bf16(v, oh, ol);
    }
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float* ws_ = dimg + (kDec16Wsig + mt * 4) * 64 + lane;
        dH[mt] = f32x4{ws_[0] * dsig, ws_[64] * dsig, ws_[128] * dsig, ws_[192] * dsig};
        if constexpr (COLOUR)
            dH[mt] = mfma3_bf16(lds_row4(g1img, mt * 4, lane), lds_row4(g1img, 16 + mt * 4, lane), oh, ol, dH[mt]);
#pragma unroll
        for (int r = 0; r < 4; ++r) dH[mt][r] *= sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
    }
    u32x4r dh[2], dl[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = dH[2 * ks + (c >> 2)][c & 3];
        split8_bf16(v, dh[ks], dl[ks]);
    }
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
        dF[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            dF[ft] = mfma3_bf16(lds_row4(g0img, (ft * 2 + ks) * 4, lane), lds_row4(g0img, 16 + (ft * 2 + ks) * 4, lane),
                                dh[ks], dl[ks], dF[ft]);
    }
}

// ---------------------------------------------------------------- decoder-parameter gradients (PG)
// per-tile operand images for the sample-contracting products
//   dW1c[32x64] += dO[32x16] . SP^T[16x64]      dW0[64x32] += dHpre[64x16] . F[16x32]
struct GradLds {
    float sp[64 * 17], dp[64 * 17], dO[32 * 17], f[16 * 33];
};

struct DecGrads { float *w0, *b0, *w1, *b1; };   // [64][32], [64], [33][64], [33]; accumulated with atomics

struct DecGradAcc {                              // a wave's running sums over its tiles
    f32x4 aw1[2][4], aw0[4][2];                  // dW1c tiles [ct][kt], dW0 tiles [kt][ft]
    float s_dO[2][4], s_dp[4][4], s_sw[4][4], s_ds;      // per-lane bias / sigma-row sums
};

__device__ __forceinline__ void dec_grad_zero(DecGradAcc& acc) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            acc.aw1[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc.aw0[y][x] = f32x4{0.f, 0.f, 0.f, 0.f};
            acc.s_dO[x][y] = 0.f;
        }
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) { acc.s_dp[x][y] = 0.f; acc.s_sw[x][y] = 0.f; }
    acc.s_ds = 0.f;
}

// one 16-sample tile: operand images for the weight-gradient products + running bias / sigma-row sums, then the 64 MFMAs
// (a lane that must not contribute passes dO = dsig = 0: then dH = 0 and every product and sum it enters is 0)
__device__ __forceinline__ void dec_grad_tile(DecGradAcc& acc, GradLds& gl, int j, int g, const float f[8], const f32x4 h[4],
                                              const f32x4 dH[4], const f32x4 dO[2], float dsig) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gl.sp[(16 * mt + 4 * g + r) * 17 + j] = h[mt][r];
            gl.dp[(16 * mt + 4 * g + r) * 17 + j] = dH[mt][r];
            acc.s_dp[mt][r] += dH[mt][r];
            acc.s_sw[mt][r] += dsig * h[mt][r];
        }
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gl.dO[(16 * ot + 4 * g + r) * 17 + j] = dO[ot][r];
            acc.s_dO[ot][r] += dO[ot][r];
        }
#pragma unroll
    for (int t = 0; t < 8; ++t) gl.f[j * 33 + 8 * g + t] = f[t];
    if (g == 0) acc.s_ds += dsig;
    WAVE_SYNC();
    // MFMA operands: A[i][k] -> lane (i = j, k = g); B[k][n] -> lane (k = g, n = j); 4 samples per step
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int smp = 4 * st + g;
        float a1[2], bsp[4], a0[4], bf[2];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) a1[ct] = gl.dO[(16 * ct + j) * 17 + smp];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            bsp[kt] = gl.sp[(16 * kt + j) * 17 + smp];
            a0[kt] = gl.dp[(16 * kt + j) * 17 + smp];
        }
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) bf[ft] = gl.f[smp * 33 + 16 * ft + j];
#pragma unroll
        for (int ct = 0; ct < 2; ++ct)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
                acc.aw1[ct][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ct], bsp[kt], acc.aw1[ct][kt], 0, 0, 0);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
                acc.aw0[kt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kt], bf[ft], acc.aw0[kt][ft], 0, 0, 0);
    }
}

// end of the kernel: one set of atomics per wave.  effective weight = parameter * gain  ->  d parameter = d effective * gain
__device__ __forceinline__ void dec_grad_flush(const DecGradAcc& acc, const DecGrads& dg, float lr_mul, int lane) {
    const int j = lane & 15, g = lane >> 4;
    const float g0 = lr_mul * 0.17677669529663687f, g1 = lr_mul * 0.125f, gb = lr_mul;
    // C layout: lane (col = j, rows 4g + r)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                unsafeAtomicAdd(dg.w1 + (1 + 16 * ct + 4 * g + r) * 64 + 16 * kt + j, acc.aw1[ct][kt][r] * g1);
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                unsafeAtomicAdd(dg.w0 + (16 * kt + 4 * g + r) * 32 + 16 * ft + j, acc.aw0[kt][ft][r] * g0);
    // per-lane running sums: reduce over the 16 sample lanes (j), lane j == 0 commits
    auto red16 = [](float v) {
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
        return v;
    };
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float vb = red16(acc.s_dp[mt][r]), vw = red16(acc.s_sw[mt][r]);
            if (j == 0) {
                unsafeAtomicAdd(dg.b0 + 16 * mt + 4 * g + r, vb * gb);
                unsafeAtomicAdd(dg.w1 + 16 * mt + 4 * g + r, vw * g1);          // sigma row of W1
            }
        }
#pragma unroll
    for (int ot = 0; ot < 2; ++ot)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = red16(acc.s_dO[ot][r]);
            if (j == 0) unsafeAtomicAdd(dg.b1 + 1 + 16 * ot + 4 * g + r, v * gb);
        }
    const float vs = red16(acc.s_ds);
    if (lane == 0) unsafeAtomicAdd(dg.b1, vs * gb);
}

// ---------------------------------------------------------------- dL/dF -> d planes: run-merged atomic scatter of a tile
struct TileLds {
    float df[16 * 32];        // dL/dfeature of the 16 samples, [sample][channel]
    __attribute__((aligned(16))) int   idx[12 * 16];       // texel index of every tap, [plane*4 + tap][sample]
    __attribute__((aligned(16))) float wgt[12 * 16];       // bilinear weight / 3 (0: outside the plane, or a sample that is not there)
};

// lane (j, g), register r of tile ft -> feature channel 16ft + 4g + r of sample j  (Lds: TileLds, or the column kernel's ColTileLds)
template <class Lds>
__device__ __forceinline__ void publish_df(Lds& lds, int j, int g, int ft, f32x4 dF) {
    *reinterpret_cast<float4*>(&lds.df[j * 32 + 16 * ft + 4 * g]) = make_float4(dF[0], dF[1], dF[2], dF[3]);
}
// a lane (j, g = pl) publishes plane pl's taps of sample j, tap-major [plane*4 + tap][sample]: the scatter reads 16 samples as b128.
// One plane per call, under the caller's `if (g == pl)`: a function that takes the three planes' taps and tests g itself is
// optimised on its own into one block reading taps[g], and that dynamic index puts the caller's taps into scratch memory.
__device__ __forceinline__ void publish_taps(TileLds& lds, int pl, const PlaneTaps& t, int j, bool valid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lds.idx[(pl * 4 + k) * 16 + j] = t.idx[k];
        lds.wgt[(pl * 4 + k) * 16 + j] = valid ? t.w[k] * 0.3333333333333333f : 0.f;
    }
}
// lane = channel, half-wave hf walks tap (2kp + hf) of one plane through the 16 samples (depth-sorted along a ray) and MERGES
// RUNS: consecutive samples whose tap lands on the same texel (the plane the ray is steep to moves < 1 texel per sample; the
// importance samples cluster; sorted or repeated points) are summed in a register and leave as one 128-byte atomic: 96 -> ~67
// atomics per tile on the bench workload (plane (x,y): 3.0 taps per run, the two depth planes: 1.1).  Measured 9.3 -> 8.8 ms per
// 4 frames; without any atomics the call takes 2.7 ms, i.e. the cost follows the number of DISTINCT lines touched more than the
// number of atomic instructions.  The texel index is inside the plane by construction (plane_taps clamps it); a weight of 0
// issues nothing.  NPK: tap pairs walked = 2 per plane (4: plane 2 is left to the mirror; 6: all three planes).
// base: the frame's three planes [3][H][W][32]; plane_stride = H * W * 32.
template <int NPK>
__device__ __forceinline__ void scatter_tile_runs(const TileLds& lds, float* base, size_t plane_stride, int lane) {
    const int c = lane & 31, hf = lane >> 5;
    base += c;
    float dfc[16];                             // dL/dfeature[sample][c] of the tile: read once, used by every tap
#pragma unroll
    for (int sm = 0; sm < 16; ++sm) dfc[sm] = lds.df[sm * 32 + c];
#pragma unroll 1
    for (int pk = 0; pk < NPK; ++pk) {
        const int pl = pk >> 1, k = 2 * (pk & 1) + hf;
        float* pbase = base + (size_t)pl * plane_stride;
        float wv[16];
        int tv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {          // the 16 samples of this tap: 4 + 4 ds_read_b128 (half-wave broadcast)
            const float4 w4 = *reinterpret_cast<const float4*>(&lds.wgt[(pl * 4 + k) * 16 + 4 * q]);
            const int4 t4 = *reinterpret_cast<const int4*>(&lds.idx[(pl * 4 + k) * 16 + 4 * q]);
            wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
            tv[4 * q] = t4.x; tv[4 * q + 1] = t4.y; tv[4 * q + 2] = t4.z; tv[4 * q + 3] = t4.w;
        }
        int cur = -1;
        float run = 0.f;
#pragma unroll
        for (int sm = 0; sm < 16; ++sm) {
            const float wgt = wv[sm];
            const int t = tv[sm];
            const float v = dfc[sm] * wgt;
            if (wgt != 0.f) {
                if (t == cur) {
                    run += v;
                } else {
#ifndef HFAGP_NO_ATOMICS
                    if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
#endif
                    cur = t;
                    run = v;
                }
            }
        }
#ifndef HFAGP_NO_ATOMICS
        if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
#endif
    }
}

// ---------------------------------------------------------------- positional derivative of the gather
// Lane (j, g) holds dL/dF of channels 16 ft + 4 g + r of a sample at the normalised position q and forms its share of
// P_k = <dL/dF, texel_k> for the twelve taps (lines the gather has just pulled in), then
//   dL/dq = sum_planes (dL/dix, dL/diy) routed to the two coordinates the plane projects (plane_coords).
// sx, sy: d pixel / d grid coordinate (plane_pixel) times the mean over the planes = W / 2 / 3, H / 2 / 3.
// dq is this lane's share: the caller sums the four g lanes of the sample.
__device__ __forceinline__ void gather_position_grad(const HfagpRaymarchArgs& a, int b, int g, const float q[3], const f32x4 dF[2],
                                                     float sx, float sy, float dq[3]) {
    dq[0] = dq[1] = dq[2] = 0.f;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        float gx, gy;
        plane_coords(a, q, pl, gx, gy);
        PlaneTapsD t;
        plane_taps_d(a, gx, gy, t);
        const char* base = reinterpret_cast<const char*>(a.planes + ((size_t)(b * 3 + pl) * a.H * a.W) * 32);
        float4 v0[4], v1[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned off = ((unsigned)t.idx[k] * 32u + 4u * g) * 4u;      // < 2^32: one plane
            v0[k] = *reinterpret_cast<const float4*>(base + off);
            v1[k] = *reinterpret_cast<const float4*>(base + off + 64);
        }
        float P[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float acc = dF[0][0] * v0[k].x;
            acc = fmaf(dF[0][1], v0[k].y, acc);
            acc = fmaf(dF[0][2], v0[k].z, acc);
            acc = fmaf(dF[0][3], v0[k].w, acc);
            acc = fmaf(dF[1][0], v1[k].x, acc);
            acc = fmaf(dF[1][1], v1[k].y, acc);
            acc = fmaf(dF[1][2], v1[k].z, acc);
            acc = fmaf(dF[1][3], v1[k].w, acc);
            P[k] = t.ok[k] ? acc : 0.f;
        }
        // dL/dix = (P1 - P0)(1 - fy) + (P3 - P2) fy,  dL/diy = (P2 - P0)(1 - fx) + (P3 - P1) fx.  The FMA is written out: under
        // -ffp-contract the compiler fuses ONE of the two products of  a b + c d, and which one follows the operand order its
        // optimiser happens to leave, not the source's; it changes when code moves.  These are the two it fused (in all three
        // planes) in the camera, point-query and normals kernels these lines come from: their results keep their bits.
        const float dix = fmaf(1.f - t.fy, P[1] - P[0], t.fy * (P[3] - P[2])) * sx;
        const float diy = fmaf(t.fx, P[3] - P[1], (1.f - t.fx) * (P[2] - P[0])) * sy;
        // planes (x,y), (x,z), (z,x) [plane_axes 0] or (z,y): plane_coords
        if (pl == 0) { dq[0] += dix; dq[1] += diy; }
        else if (pl == 1) { dq[0] += dix; dq[2] += diy; }
        else {
            dq[2] += dix;
            if (a.plane_axes == 0) dq[0] += diy; else dq[1] += diy;
        }
    }
}

// gather_position_grad of dF PLUS the mixed second derivative of the bilinear weights (raymarch_normals_camera.hip), from one
// read of the twelve texel lines: the positional gradient of a loss that also reaches g = J^T a (J = dF / dq) through
// gamma_q = dL/dg.  Bilinear weights have no pure second derivative, only d2 w_k / dgx dgy = s_k (W / 2)(H / 2) with
// s = (+1, -1, -1, +1) for nw, ne, sw, se, so per plane, with (cx, cy) the components of gamma_q its two coordinates carry
// (plane_coords) and zero padding through ok_k,
//   m = (W / 2)(H / 2) sum_k s_k ok_k <texel_k, a> / 3,    dL/dgx = [gather_position_grad's] + m cy,    dL/dgy = [...] + m cx,
// routed to dq as gather_position_grad routes its terms.  Lane (j, g) holds dF and a = d sigma / dF (av) of channels
// 16 ft + 4 g + r and forms its share.  sx, sy: gather_position_grad's; sxy = (W / 2)(H / 2) / 3.
__device__ __forceinline__ void gather_position_cross_grad(const HfagpRaymarchArgs& a, int b, int g, const float q[3],
                                                           const f32x4 dF[2], const f32x4 av[2], const float gq[3], float sx,
                                                           float sy, float sxy, float dq[3]) {
    dq[0] = dq[1] = dq[2] = 0.f;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        float gx, gy;
        plane_coords(a, q, pl, gx, gy);
        PlaneTapsD t;
        plane_taps_d(a, gx, gy, t);
        const char* base = reinterpret_cast<const char*>(a.planes + ((size_t)(b * 3 + pl) * a.H * a.W) * 32);
        float P[4], A[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned off = ((unsigned)t.idx[k] * 32u + 4u * g) * 4u;      // < 2^32: one plane
            const float4 v0 = *reinterpret_cast<const float4*>(base + off);
            const float4 v1 = *reinterpret_cast<const float4*>(base + off + 64);
            float acc = dF[0][0] * v0.x, aca = av[0][0] * v0.x;
            acc = fmaf(dF[0][1], v0.y, acc); aca = fmaf(av[0][1], v0.y, aca);
            acc = fmaf(dF[0][2], v0.z, acc); aca = fmaf(av[0][2], v0.z, aca);
            acc = fmaf(dF[0][3], v0.w, acc); aca = fmaf(av[0][3], v0.w, aca);
            acc = fmaf(dF[1][0], v1.x, acc); aca = fmaf(av[1][0], v1.x, aca);
            acc = fmaf(dF[1][1], v1.y, acc); aca = fmaf(av[1][1], v1.y, aca);
            acc = fmaf(dF[1][2], v1.z, acc); aca = fmaf(av[1][2], v1.z, aca);
            acc = fmaf(dF[1][3], v1.w, acc); aca = fmaf(av[1][3], v1.w, aca);
            P[k] = t.ok[k] ? acc : 0.f;
            A[k] = t.ok[k] ? aca : 0.f;
        }
        const float m = ((A[0] - A[1]) - (A[2] - A[3])) * sxy;
        const float cx = pl == 2 ? gq[2] : gq[0];
        const float cy = pl == 0 ? gq[1] : pl == 1 ? gq[2] : (a.plane_axes == 0 ? gq[0] : gq[1]);
        const float dix = fmaf(m, cy, fmaf(1.f - t.fy, P[1] - P[0], t.fy * (P[3] - P[2])) * sx);
        const float diy = fmaf(m, cx, fmaf(t.fx, P[3] - P[1], (1.f - t.fx) * (P[2] - P[0])) * sy);
        if (pl == 0) { dq[0] += dix; dq[1] += diy; }
        else if (pl == 1) { dq[0] += dix; dq[2] += diy; }
        else {
            dq[2] += dix;
            if (a.plane_axes == 0) dq[0] += diy; else dq[1] += diy;
        }
    }
}

// dH = wsig * sigmoid(hp) alone (d sigma = 1, no colour gradient): the first half of decoder_bwd[16]_lds<false>, for a caller
// that forms a = W0'^T dH itself (w0t_mul).  dimg: the decoder image of decoder_images_lds<DEC16>.
template <bool DEC16>
__device__ __forceinline__ void decoder_dh_lds(const float* dimg, int lane, const f32x4 hp[4], f32x4 dH[4]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        const float* ws_ = dimg + ((DEC16 ? kDec16Wsig : kDecWsig) + mt * 4) * 64 + lane;
        dH[mt] = f32x4{ws_[0], ws_[64], ws_[128], ws_[192]};
#pragma unroll
        for (int r = 0; r < 4; ++r) dH[mt][r] *= sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
    }
}

// ---------------------------------------------------------------- second order: the backward of the normals
// (raymarch_normals_bwd.hip) differentiates the decoder adjoint itself.  Its pieces sit here next to their first-order
// siblings: the scatter with two value / weight sets, the two fp32 products with W0', and the weight-gradient sums.

// ---- d planes: the run-merged line scatter (scatter_tile_runs) with TWO value / weight sets per tap: the
// texel of tap k receives  dF w_k / 3 + a w'_k / 3  as ONE 128-byte atomic per run (two calls of scatter_tile_runs<6> would issue
// two: the cost of the scatter follows the atomics).  Same tables, same walk, same merging rule; a tap is skipped when both of
// its weights are 0 (outside the plane, or a sample that contributes nothing).
struct Tile2Lds {
    float df[16 * 32];                                      // dL/dF, then a = d sigma / dF, of the 16 samples, [sample][channel]
    __attribute__((aligned(16))) int   idx[12 * 16];        // texel index of every tap, [plane*4 + tap][sample]
    __attribute__((aligned(16))) float wgt[12 * 16];        // w_k / 3
    __attribute__((aligned(16))) float dwg[12 * 16];        // w'_k / 3
};
// a lane (j, g = pl) publishes plane pl's taps of sample j (one plane per call, under the caller's `if (g == pl)`: publish_taps)
__device__ __forceinline__ void publish_taps2(Tile2Lds& lds, int pl, const PlaneTaps& t, const PlaneTaps& dt, int j, bool valid) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lds.idx[(pl * 4 + k) * 16 + j] = t.idx[k];
        lds.wgt[(pl * 4 + k) * 16 + j] = valid ? t.w[k] * 0.3333333333333333f : 0.f;
        lds.dwg[(pl * 4 + k) * 16 + j] = valid ? dt.w[k] * 0.3333333333333333f : 0.f;
    }
}
// lane (j, g), register r of tile ft -> channel 16 ft + 4 g + r of sample j (publish_df); then the column of channel lane & 31
__device__ __forceinline__ void publish_df2(Tile2Lds& lds, int j, int g, const f32x4 v[2]) {
#pragma unroll
    for (int ft = 0; ft < 2; ++ft)
        *reinterpret_cast<float4*>(&lds.df[j * 32 + 16 * ft + 4 * g]) = make_float4(v[ft][0], v[ft][1], v[ft][2], v[ft][3]);
}
__device__ __forceinline__ void channel_column(const Tile2Lds& lds, int lane, float col[16]) {
#pragma unroll
    for (int sm = 0; sm < 16; ++sm) col[sm] = lds.df[sm * 32 + (lane & 31)];
}
// dfc, avc: this lane's channel of dL/dF and of a for the 16 samples (channel_column: the two pass through lds.df one after the other)
template <int NPK>
__device__ __forceinline__ void scatter_tile_runs2(const Tile2Lds& lds, const float dfc[16], const float avc[16], float* base,
                                                   size_t plane_stride, int lane) {
    const int c = lane & 31, hf = lane >> 5;
    base += c;
#pragma unroll 1
    for (int pk = 0; pk < NPK; ++pk) {
        const int pl = pk >> 1, k = 2 * (pk & 1) + hf;
        float* pbase = base + (size_t)pl * plane_stride;
        float wv[16], dv[16];
        int tv[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 w4 = *reinterpret_cast<const float4*>(&lds.wgt[(pl * 4 + k) * 16 + 4 * q]);
            const float4 d4 = *reinterpret_cast<const float4*>(&lds.dwg[(pl * 4 + k) * 16 + 4 * q]);
            const int4 t4 = *reinterpret_cast<const int4*>(&lds.idx[(pl * 4 + k) * 16 + 4 * q]);
            wv[4 * q] = w4.x; wv[4 * q + 1] = w4.y; wv[4 * q + 2] = w4.z; wv[4 * q + 3] = w4.w;
            dv[4 * q] = d4.x; dv[4 * q + 1] = d4.y; dv[4 * q + 2] = d4.z; dv[4 * q + 3] = d4.w;
            tv[4 * q] = t4.x; tv[4 * q + 1] = t4.y; tv[4 * q + 2] = t4.z; tv[4 * q + 3] = t4.w;
        }
        int cur = -1;
        float run = 0.f;
#pragma unroll
        for (int sm = 0; sm < 16; ++sm) {
            const int t = tv[sm];
            const float v = fmaf(avc[sm], dv[sm], dfc[sm] * wv[sm]);
            if (wv[sm] != 0.f || dv[sm] != 0.f) {
                if (t == cur) {
                    run += v;
                } else {
                    if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
                    cur = t;
                    run = v;
                }
            }
        }
        if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
    }
}

// out^T[32x16] = W0'^T . x^T on the fp32 matrix pipe (the second product of decoder_bwd_lds): x in the C layout of the hidden
// tiles, out in the C layout of the two feature tiles (channel 16 ft + 4 g + r)
__device__ __forceinline__ void w0t_mul(const float* w0t, int lane, const f32x4 x[4], f32x4 out[2]) {
    const float* W0 = w0t + lane;
#pragma unroll
    for (int ft = 0; ft < 2; ++ft) {
        out[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                out[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(W0[(ft * 16 + mt * 4 + r) * 64], x[mt][r], out[ft], 0, 0, 0);
    }
}
// v^T[64x16] = W0' . u^T on the fp32 matrix pipe (layer 1 of decoder_fwd_lds without its bias): w0f rows mt * 8 + t of lane
// (j, g) = W0'[16 mt + j][8 g + t]; u in the gather's layout (channels 8 g + t), v in the C layout of the hidden tiles
__device__ __forceinline__ void w0_mul(const float* w0f, int lane, const float u[8], f32x4 v[4]) {
    const float* W = w0f + lane;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        v[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 8; ++t) v[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(W[(mt * 8 + t) * 64], u[t], v[mt], 0, 0, 0);
    }
}

// the fp32 A operands of W0' for w0_mul where the forward image is the 16-bit one (rows 0-31 of the fp32 image of
// store_decoder_lds otherwise), built by all `nthreads` threads of the block: w0f[mt * 8 + t][lane] = W0[16 mt + j][8 g + t] * g0
__device__ __forceinline__ void build_w0_lds(const HfagpRaymarchArgs& a, float* w0f, int tid, int nthreads) {
    const float g0 = a.decoder_lr_mul * 0.17677669529663687f;
    for (int i = tid; i < 32 * 64; i += nthreads) {
        const int l = i & 63, row = i >> 6;              // row = mt * 8 + t
        w0f[i] = a.dec_w0[(16 * (row >> 3) + (l & 15)) * 32 + 8 * (l >> 4) + (row & 7)] * g0;
    }
}

// operand images of the sample-contracting products  dW0'[64x32] += x[64x16] . F[16x32] + dH[64x16] . u[16x32]
struct NrmGradLds {
    float x[64 * 17], dh[64 * 17], f[16 * 33], u[16 * 33];
};
struct NrmGradAcc {                              // a wave's running sums over its tiles
    f32x4 aw0[4][2];                             // dW0' tiles [kt][ft]
    float s_x[4][4], s_sw[4][4], s_ds;           // per-lane b0' / sigma-row sums, dbsig
};

// one tile of the weight-gradient products (the operand layouts of dec_grad_tile)
__device__ __forceinline__ void nrm_grad_tile(NrmGradAcc& acc, NrmGradLds& gl, int j, int g, const float f[8], const float u[8],
                                              const f32x4 x[4], const f32x4 dH[4]) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gl.x[(16 * mt + 4 * g + r) * 17 + j] = x[mt][r];
            gl.dh[(16 * mt + 4 * g + r) * 17 + j] = dH[mt][r];
        }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        gl.f[j * 33 + 8 * g + t] = f[t];
        gl.u[j * 33 + 8 * g + t] = u[t];
    }
    WAVE_SYNC();
    // MFMA operands: A[i][k] -> lane (i = j, k = g); B[k][n] -> lane (k = g, n = j); 4 samples per step
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        const int smp = 4 * st + g;
        float ax[4], ad[4], bf[2], bu[2];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            ax[kt] = gl.x[(16 * kt + j) * 17 + smp];
            ad[kt] = gl.dh[(16 * kt + j) * 17 + smp];
        }
#pragma unroll
        for (int ft = 0; ft < 2; ++ft) {
            bf[ft] = gl.f[smp * 33 + 16 * ft + j];
            bu[ft] = gl.u[smp * 33 + 16 * ft + j];
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) {
                acc.aw0[kt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(ax[kt], bf[ft], acc.aw0[kt][ft], 0, 0, 0);
                acc.aw0[kt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(ad[kt], bu[ft], acc.aw0[kt][ft], 0, 0, 0);
            }
    }
}

// end of the kernel: one set of atomics per wave, with the gains of dec_grad_flush; the colour rows of the second layer get nothing.
// SIGMA_BIAS = false: a caller without a first-order d sigma (planes_query_normals_bwd.hip) leaves d_dec_b1 alone altogether.
template <bool SIGMA_BIAS = true>
__device__ __forceinline__ void nrm_grad_flush(const NrmGradAcc& acc, const DecGrads& dg, float lr_mul, int lane) {
    const int j = lane & 15, g = lane >> 4;
    const float g0 = lr_mul * 0.17677669529663687f, g1 = lr_mul * 0.125f, gb = lr_mul;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                unsafeAtomicAdd(dg.w0 + (16 * kt + 4 * g + r) * 32 + 16 * ft + j, acc.aw0[kt][ft][r] * g0);
    auto red16 = [](float v) {
        v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
        return v;
    };
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float vb = red16(acc.s_x[mt][r]), vw = red16(acc.s_sw[mt][r]);
            if (j == 0) {
                unsafeAtomicAdd(dg.b0 + 16 * mt + 4 * g + r, vb * gb);
                unsafeAtomicAdd(dg.w1 + 16 * mt + 4 * g + r, vw * g1);          // sigma row of W1
            }
        }
    if constexpr (SIGMA_BIAS) {
        const float vs = red16(acc.s_ds);
        if (lane == 0) unsafeAtomicAdd(dg.b1, vs * gb);
    }
}

}  // namespace hfagp
