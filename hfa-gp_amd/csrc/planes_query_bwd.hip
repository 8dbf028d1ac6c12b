// Backward of the tri-plane point query (planes_query.hip) for explicit points (gfx950): from dL/dsigma and dL/drgb at the
// points to dL/dplanes, dL/dcoords and the decoder-parameter gradients.  Composed of the renderer's shared device functions:
//   per 16-point tile (a wave; lane = 16 g + j, j = point, g = channel group, as the forward):
//     plane_taps + gather8 (the forward's bits: scale_rn of planes_query_common.h) -> decoder_fwd[16]_lds<true> ->
//     dO = g_rgb * 1.002 * s (1 - s),  d sigma = g_sigma (the raw output: no softplus) -> decoder adjoint (split bf16 on the
//     16-bit pipe, or the exact fp32 MFMA loop) = dL/dF, lane (j, g) holding channels 16 ft + 4 g + r of point j;
//   d planes: dL/dF transposed through LDS so that a half-wave owns the 32 channels of ONE texel line, then run-merged fp32
//     atomics of full 128-byte lines, 12 taps per point with weight w_k / 3 (the scatter of raymarch_bwd_tiles_kernel).  EVERY
//     plane is scattered at its true texels: free points on square planes do mirror between planes 1 and 2 too, but a caller
//     adds this gradient to the ray marcher's, whose mirror_plane_kernel OVERWRITES plane 2 — so this kernel runs after it
//     and adds to all three.  Lanes past M and taps outside the plane carry weight 0 and issue nothing;
//   d coords (DCOORD): the positional derivative of the gather (raymarch_bwd_camera_kernel's arithmetic: plane_taps_d,
//     P_k = <dL/dF, texel_k>, (dix, diy) routed by plane_coords, times coord_scale), reduced over the four g lanes of a
//     point by two cross-row shuffles: one writer per point, plain stores, no atomics;
//   decoder gradients (PG): the sample-contracting MFMA products of raymarch_bwd_tiles_kernel<PG> accumulated across a wave's
//     tiles, one set of atomics per wave at the end.  That code is a COPY of the one in raymarch_bwd.hip (GradLds, the operand
//     images, the flush): lifting it into raymarch_common.h reorders that unit's device code, and its listing is pinned.
// Schedule: raymarch_common.h ray_schedule over tiles, one round of resident workgroups.
#include "raymarch_common.h"
#include "planes_query_common.h"

namespace hfagp {

constexpr int kQbWaves = 4;

struct QueryBwdParams {
    HfagpRaymarchArgs a;       // planes, decoder, B / H / W, plane_axes, decoder_lr_mul, planes_absmax (the shared helpers' view)
    const float* coords;       // [Bc][M][3]
    const float* g_sigma;      // [B][M] or NULL
    const float* g_rgb;        // [B][M][32] or NULL
    float* d_planes;           // [B][3][H][W][32] or NULL, accumulated into
    float* d_coords;           // [B][M][3] (DCOORD)
    long long M, tiles_per_b, total_tiles;
    long long coords_bstride;  // elements between identities in coords (0: broadcast)
    float coord_scale;         // fp32(2 / box_warp), as the forward
};

struct QueryDecGrads { float *w0, *b0, *w1, *b1; };   // [64][32], [64], [33][64], [33]; accumulated with atomics (PG)

struct QueryTileLds {
    float df[16 * 32];                                     // dL/dfeature of the 16 points, [point][channel]
    __attribute__((aligned(16))) int   idx[12 * 16];       // texel index of every tap, [plane*4 + tap][point]
    __attribute__((aligned(16))) float wgt[12 * 16];       // bilinear weight / 3 (0: outside the plane, or a lane past M)
};

// operand images of the decoder-weight products (as GradLds of raymarch_bwd.hip)
//   dW1c[32x64] += dO[32x16] . SP^T[16x64]      dW0[64x32] += dHpre[64x16] . F[16x32]
struct QueryGradLds {
    float sp[64 * 17], dp[64 * 17], dO[32 * 17], f[16 * 33];
};

template <bool DEC16, bool PG, bool DCOORD>
__global__ void __launch_bounds__(kQbWaves * 64, PG ? 1 : 2)
planes_query_bwd_kernel(const QueryBwdParams p, const QueryDecGrads dg) {
    __shared__ QueryTileLds lds_all[kQbWaves];
    __shared__ __attribute__((aligned(16))) float glds_raw[PG ? kQbWaves * sizeof(QueryGradLds) / sizeof(float) : 1];
    // the decoder images, as in raymarch_bwd_camera_kernel: backward A operands w1t / w0t, forward image wfwd
    __shared__ float w1t[4 * 8 * 64];
    __shared__ float w0t[2 * 16 * 64];
    __shared__ float wfwd[kDecLdsRows * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    QueryTileLds& lds = lds_all[wave];
    if (wave == 0) {
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
    if constexpr (DEC16) {
        build_grad16_lds(a, w1t, w0t, lane, wave, kQbWaves);
    } else {
        const float g0 = a.decoder_lr_mul * 0.17677669529663687f, g1 = a.decoder_lr_mul * 0.125f;
        for (int i = threadIdx.x; i < 4 * 8 * 64; i += kQbWaves * 64) {
            const int l = i & 63, st = (i >> 6) & 7, mt = i >> 9, jj = l & 15, gg = l >> 4;
            w1t[i] = a.dec_w1[(1 + 16 * (st >> 2) + 4 * gg + (st & 3)) * 64 + 16 * mt + jj] * g1;
        }
        for (int i = threadIdx.x; i < 2 * 16 * 64; i += kQbWaves * 64) {
            const int l = i & 63, st = (i >> 6) & 15, ft = i >> 10, jj = l & 15, gg = l >> 4;
            w0t[i] = a.dec_w0[(16 * (st >> 2) + 4 * gg + (st & 3)) * 32 + 16 * ft + jj] * g0;
        }
    }
    __syncthreads();

    QueryGradLds& gl = reinterpret_cast<QueryGradLds*>(glds_raw)[PG ? wave : 0];      // never dereferenced unless PG
    f32x4 aw1[2][4], aw0[4][2];                      // PG: dW1c tiles [ct][kt], dW0 tiles [kt][ft]
    float s_dO[2][4], s_dp[4][4], s_sw[4][4], s_ds = 0.f;
    if constexpr (PG) {
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) {
                aw1[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
                aw0[y][x] = f32x4{0.f, 0.f, 0.f, 0.f};
                s_dO[x][y] = 0.f;
            }
#pragma unroll
        for (int x = 0; x < 4; ++x)
#pragma unroll
            for (int y = 0; y < 4; ++y) { s_dp[x][y] = 0.f; s_sw[x][y] = 0.f; }
    }
    // d pixel / d grid coordinate (plane_pixel) times the mean over the planes
    const float sx = (float)a.W * 0.5f * 0.3333333333333333f, sy = (float)a.H * 0.5f * 0.3333333333333333f;

    const RaySchedule sch = ray_schedule(p.total_tiles, wave, kQbWaves);
#pragma unroll 1
    for (long long t = sch.begin; t < sch.end; t += sch.stride) {
        const int b = __builtin_amdgcn_readfirstlane((int)(t / p.tiles_per_b));     // wave-uniform
        const long long m0 = (t - (long long)b * p.tiles_per_b) * 16;
        const bool valid = m0 + j < p.M;
        const long long m = min(m0 + j, p.M - 1);            // a lane past M recomputes the last point and contributes nothing
        const long long pt = (long long)b * p.M + m;         // 64-bit: B * M * 32 passes 2^31
        float q[3];
        {
            const float* c = p.coords + (long long)b * p.coords_bstride + m * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = scale_rn(p.coord_scale, c[k]);
        }
        PlaneTaps taps[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            float gx, gy;
            plane_coords(a, q, pl, gx, gy);
            plane_taps(a, gx, gy, taps[pl]);
        }
        float f[8];
        gather8(a, b, g, taps, f);
        int ln = lane;
        asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
        f32x4 hp[4], h[4], o[2];
        float sigma;
        if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
        else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);

        // upstream gradients: rgb = sigmoid(o) * 1.002 - 0.001, sigma = the raw output
        const float dsig = (valid && p.g_sigma) ? p.g_sigma[pt] : 0.f;
        f32x4 dO[2];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
            float4 gf = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && p.g_rgb) gf = *reinterpret_cast<const float4*>(p.g_rgb + pt * 32 + 16 * ot + 4 * g);
            const float gv[4] = {gf.x, gf.y, gf.z, gf.w};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sg = sigmoid_f(o[ot][r]);
                dO[ot][r] = gv[r] * 1.002f * sg * (1.f - sg);
            }
        }
        f32x4 dH[4];
        f32x4 dF[2];
        if constexpr (DEC16) decoder_bwd16_lds(wfwd, w1t, w0t, ln, dO, dsig, hp, dH, dF);
#pragma unroll
        for (int mt = 0; mt < (DEC16 ? 0 : 4); ++mt) {
            const float* ws_ = wfwd + (48 + mt * 4) * 64 + ln;
            dH[mt] = f32x4{ws_[0] * dsig, ws_[64] * dsig, ws_[128] * dsig, ws_[192] * dsig};
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float wA = w1t[(mt * 8 + ot * 4 + r) * 64 + ln];
                    dH[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wA, dO[ot][r], dH[mt], 0, 0, 0);
                }
#pragma unroll
            for (int r = 0; r < 4; ++r) dH[mt][r] *= sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
        }
        if constexpr (!DEC16) {
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) {
                dF[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float wA = w0t[(ft * 16 + mt * 4 + r) * 64 + ln];
                        dF[ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(wA, dH[mt][r], dF[ft], 0, 0, 0);
                    }
            }
        }
        // lane (j, g), register r of tile ft -> feature channel 16 ft + 4 g + r of point j

        if constexpr (PG) {
            // operand images for the weight-gradient products + running bias / sigma-row sums (a lane past M: dO = dsig = 0,
            // so dH = 0 and every product and sum it enters is 0)
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gl.sp[(16 * mt + 4 * g + r) * 17 + j] = h[mt][r];
                    gl.dp[(16 * mt + 4 * g + r) * 17 + j] = dH[mt][r];
                    s_dp[mt][r] += dH[mt][r];
                    s_sw[mt][r] += dsig * h[mt][r];
                }
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    gl.dO[(16 * ot + 4 * g + r) * 17 + j] = dO[ot][r];
                    s_dO[ot][r] += dO[ot][r];
                }
#pragma unroll
            for (int tt = 0; tt < 8; ++tt) gl.f[j * 33 + 8 * g + tt] = f[tt];
            if (g == 0) s_ds += dsig;
            WAVE_SYNC();
            // MFMA operands: A[i][k] -> lane (i = j, k = g); B[k][n] -> lane (k = g, n = j); 4 points per step
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
                        aw1[ct][kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[ct], bsp[kt], aw1[ct][kt], 0, 0, 0);
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft)
                        aw0[kt][ft] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[kt], bf[ft], aw0[kt][ft], 0, 0, 0);
            }
        }

        if constexpr (DCOORD) {
            // ---- positional derivative: this lane's share (its 8 channels) of P_k = <dL/dF, texel_k> for the twelve taps
            // (lines the gather above has just pulled in)
            float dq[3] = {0.f, 0.f, 0.f};
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) {
                float gx, gy;
                plane_coords(a, q, pl, gx, gy);
                PlaneTapsD td;
                plane_taps_d(a, gx, gy, td);
                const char* base = reinterpret_cast<const char*>(a.planes + ((size_t)(b * 3 + pl) * a.H * a.W) * 32);
                float4 v0[4], v1[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned off = ((unsigned)td.idx[k] * 32u + 4u * g) * 4u;      // < 2^32: one plane
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
                    P[k] = td.ok[k] ? acc : 0.f;
                }
                const float dix = ((P[1] - P[0]) * (1.f - td.fy) + (P[3] - P[2]) * td.fy) * sx;
                const float diy = ((P[2] - P[0]) * (1.f - td.fx) + (P[3] - P[1]) * td.fx) * sy;
                // planes (x,y), (x,z), (z,x) [plane_axes 0] or (z,y): plane_coords
                if (pl == 0) { dq[0] += dix; dq[1] += diy; }
                else if (pl == 1) { dq[0] += dix; dq[2] += diy; }
                else {
                    dq[2] += dix;
                    if (a.plane_axes == 0) dq[0] += diy; else dq[1] += diy;
                }
            }
            // the four channel groups of point j sit 16 lanes apart: two cross-row shuffles; q = coord_scale * p
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = dq[k];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                dq[k] = v * p.coord_scale;
            }
            if (valid && g == 0) {
                float* dst = p.d_coords + pt * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k] = dq[k];
            }
        }

        if (p.d_planes) {                      // (uniform over the launch)
#pragma unroll
            for (int ft = 0; ft < 2; ++ft)
                *reinterpret_cast<float4*>(&lds.df[j * 32 + 16 * ft + 4 * g]) =
                    make_float4(dF[ft][0], dF[ft][1], dF[ft][2], dF[ft][3]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)                 // lane (j, g = pl) publishes plane pl's taps of point j
                if (g == pl) {                             // tap-major [plane*4 + tap][point]: the scatter reads 16 points as b128
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        lds.idx[(pl * 4 + k) * 16 + j] = taps[pl].idx[k];
                        lds.wgt[(pl * 4 + k) * 16 + j] = valid ? taps[pl].w[k] * 0.3333333333333333f : 0.f;
                    }
                }
            WAVE_SYNC();
            // ---- scatter: lane = channel, half-wave hf walks tap (2 kp + hf) of one plane through the 16 points and MERGES
            // RUNS: consecutive points whose tap lands on the same texel are summed in a register and leave as one 128-byte
            // atomic (sorted or repeated points; the texel index is inside the plane by construction: plane_taps clamps it)
            const int c = lane & 31, hf = lane >> 5;
            float* base = p.d_planes + (size_t)b * 3 * a.H * a.W * 32 + c;
            float dfc[16];                             // dL/dfeature[point][c] of the tile: read once, used by every tap
#pragma unroll
            for (int sm = 0; sm < 16; ++sm) dfc[sm] = lds.df[sm * 32 + c];
#pragma unroll 1
            for (int pk = 0; pk < 6; ++pk) {
                const int pl = pk >> 1, k = 2 * (pk & 1) + hf;
                float* pbase = base + (size_t)pl * a.H * a.W * 32;
                float wv[16];
                int tv[16];
#pragma unroll
                for (int qq = 0; qq < 4; ++qq) {       // the 16 points of this tap: 4 + 4 ds_read_b128 (half-wave broadcast)
                    const float4 w4 = *reinterpret_cast<const float4*>(&lds.wgt[(pl * 4 + k) * 16 + 4 * qq]);
                    const int4 t4 = *reinterpret_cast<const int4*>(&lds.idx[(pl * 4 + k) * 16 + 4 * qq]);
                    wv[4 * qq] = w4.x; wv[4 * qq + 1] = w4.y; wv[4 * qq + 2] = w4.z; wv[4 * qq + 3] = w4.w;
                    tv[4 * qq] = t4.x; tv[4 * qq + 1] = t4.y; tv[4 * qq + 2] = t4.z; tv[4 * qq + 3] = t4.w;
                }
                int cur = -1;
                float run = 0.f;
#pragma unroll
                for (int sm = 0; sm < 16; ++sm) {
                    const float wgt = wv[sm];
                    const int tx = tv[sm];
                    const float v = dfc[sm] * wgt;
                    if (wgt != 0.f) {
                        if (tx == cur) {
                            run += v;
                        } else {
                            if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
                            cur = tx;
                            run = v;
                        }
                    }
                }
                if (cur >= 0) unsafeAtomicAdd(pbase + (size_t)cur * 32, run);
            }
        }
        WAVE_SYNC();                            // the next tile overwrites the wave's LDS tables
    }
    if constexpr (PG) {
        // effective weight = parameter * gain  ->  d parameter = d effective * gain
        const float g0 = a.decoder_lr_mul * 0.17677669529663687f, g1 = a.decoder_lr_mul * 0.125f, gb = a.decoder_lr_mul;
        if (sch.begin < sch.end) {              // (a wave without a tile holds zeros: nothing to add)
            // C layout: lane (col = j, rows 4g + r)
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        unsafeAtomicAdd(dg.w1 + (1 + 16 * ct + 4 * g + r) * 64 + 16 * kt + j, aw1[ct][kt][r] * g1);
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        unsafeAtomicAdd(dg.w0 + (16 * kt + 4 * g + r) * 32 + 16 * ft + j, aw0[kt][ft][r] * g0);
            // per-lane running sums: reduce over the 16 point lanes (j), lane j == 0 commits
            auto red16 = [](float v) {
                v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4); v += __shfl_xor(v, 8);
                return v;
            };
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float vb = red16(s_dp[mt][r]), vw = red16(s_sw[mt][r]);
                    if (j == 0) {
                        unsafeAtomicAdd(dg.b0 + 16 * mt + 4 * g + r, vb * gb);
                        unsafeAtomicAdd(dg.w1 + 16 * mt + 4 * g + r, vw * g1);          // sigma row of W1
                    }
                }
#pragma unroll
            for (int ot = 0; ot < 2; ++ot)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = red16(s_dO[ot][r]);
                    if (j == 0) unsafeAtomicAdd(dg.b1 + 1 + 16 * ot + 4 * g + r, v * gb);
                }
            const float vs = red16(s_ds);
            if (lane == 0) unsafeAtomicAdd(dg.b1, vs * gb);
        }
    }
}

template <bool DEC16, bool PG, bool DCOORD>
static int launch(const QueryBwdParams& p, const QueryDecGrads& dg, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of tiles
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, planes_query_bwd_kernel<DEC16, PG, DCOORD>, kQbWaves * 64, 0) != hipSuccess ||
            n < 1)
            n = 1;
        resident = n;
    }
    long long blocks = (p.total_tiles + kQbWaves - 1) / kQbWaves;
    const long long cap = (long long)kNumCU * resident;
    if (blocks > cap) blocks = cap;
    planes_query_bwd_kernel<DEC16, PG, DCOORD><<<(unsigned)blocks, kQbWaves * 64, 0, s>>>(p, dg);
    return check_launch("planes_query_bwd");
}

template <bool DEC16, bool PG>
static int launch_c(const QueryBwdParams& p, const QueryDecGrads& dg, hipStream_t s) {
    return p.d_coords ? launch<DEC16, PG, true>(p, dg, s) : launch<DEC16, PG, false>(p, dg, s);
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_planes_query_bwd(const HfagpPlanesQueryBwdArgs* q, void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "planes_query_bwd: null pointer");
    HFAGP_REQUIRE(q->planes && q->dec_w0 && q->dec_b0 && q->dec_w1 && q->dec_b1, HFAGP_EBADARG, "planes_query_bwd: null pointer");
    HFAGP_REQUIRE(q->coords, HFAGP_EUNSUPPORTED, "planes_query_bwd: explicit points only (grid mode has no backward)");
    HFAGP_REQUIRE(q->g_sigma || q->g_rgb, HFAGP_EBADARG, "planes_query_bwd: null pointer (g_sigma and g_rgb: pass at least one)");
    const bool pg = q->d_dec_w0 || q->d_dec_b0 || q->d_dec_w1 || q->d_dec_b1;
    HFAGP_REQUIRE(!pg || (q->d_dec_w0 && q->d_dec_b0 && q->d_dec_w1 && q->d_dec_b1), HFAGP_EBADARG,
                  "planes_query_bwd: the four decoder gradients go together (all or none)");
    HFAGP_REQUIRE(q->d_planes || q->d_coords || pg, HFAGP_EBADARG,
                  "planes_query_bwd: null pointer (d_planes, d_coords, d_dec_*: pass at least one output)");
    HFAGP_REQUIRE(q->B > 0 && q->H > 1 && q->W > 1, HFAGP_EBADARG, "planes_query_bwd: bad dims B=%d H=%d W=%d", q->B, q->H, q->W);
    HFAGP_REQUIRE((long long)q->H * q->W <= (1ll << 25), HFAGP_EUNSUPPORTED,
                  "planes_query_bwd: planes of %d x %d texels (32-bit texel offsets need H * W <= 2^25)", q->H, q->W);
    HFAGP_REQUIRE(q->plane_axes == 0 || q->plane_axes == 1, HFAGP_EBADARG, "planes_query_bwd: plane_axes must be 0 or 1");
    HFAGP_REQUIRE(q->box_warp > 0.0, HFAGP_EBADARG, "planes_query_bwd: box_warp must be > 0");
    HFAGP_REQUIRE(q->M > 0, HFAGP_EBADARG, "planes_query_bwd: M must be > 0");
    HFAGP_REQUIRE(q->Bc == 1 || q->Bc == q->B, HFAGP_EBADARG, "planes_query_bwd: Bc=%d must be 1 or B=%d", q->Bc, q->B);
    QueryBwdParams p = {};
    p.a.planes = q->planes;
    p.a.dec_w0 = q->dec_w0; p.a.dec_b0 = q->dec_b0; p.a.dec_w1 = q->dec_w1; p.a.dec_b1 = q->dec_b1;
    p.a.B = q->B; p.a.H = q->H; p.a.W = q->W;
    p.a.plane_axes = q->plane_axes;
    p.a.box_warp = (float)q->box_warp;
    p.a.decoder_lr_mul = q->decoder_lr_mul;
    p.a.planes_absmax = q->planes_absmax;
    p.coords = q->coords;
    p.g_sigma = q->g_sigma;
    p.g_rgb = q->g_rgb;
    p.d_planes = q->d_planes;
    p.d_coords = q->d_coords;
    p.coord_scale = (float)(2.0 / q->box_warp);
    p.M = q->M;
    p.tiles_per_b = (q->M + 15) / 16;
    p.total_tiles = p.tiles_per_b * q->B;
    p.coords_bstride = q->Bc == 1 ? 0 : q->M * 3;
    const QueryDecGrads dg = {q->d_dec_w0, q->d_dec_b0, q->d_dec_w1, q->d_dec_b1};
    const bool dec16 = q->planes_absmax != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return pg ? launch_c<true, true>(p, dg, s) : launch_c<true, false>(p, dg, s);
    return pg ? launch_c<false, true>(p, dg, s) : launch_c<false, false>(p, dg, s);
}
