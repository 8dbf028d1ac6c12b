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
//     tiles, one set of atomics per wave at the end (dec_grad_* of decoder_adjoint.h, the same functions).
// Schedule: raymarch_common.h ray_schedule over tiles, one round of resident workgroups.
#include "decoder_adjoint.h"
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

template <bool DEC16, bool PG, bool DCOORD>
__global__ void __launch_bounds__(kQbWaves * 64, PG ? 1 : 2)
planes_query_bwd_kernel(const QueryBwdParams p, const DecGrads dg) {
    __shared__ TileLds lds_all[kQbWaves];
    __shared__ __attribute__((aligned(16))) float glds_raw[PG ? kQbWaves * sizeof(GradLds) / sizeof(float) : 1];
    // the decoder images, as in raymarch_bwd_camera_kernel: backward A operands w1t / w0t, forward image wfwd
    __shared__ float w1t[4 * 8 * 64];
    __shared__ float w0t[2 * 16 * 64];
    __shared__ float wfwd[kDecLdsRows * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    TileLds& lds = lds_all[wave];
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    if constexpr (DEC16) build_grad16_lds(a, w1t, w0t, lane, wave, kQbWaves);
    else build_grad_lds(a, w1t, w0t, threadIdx.x, kQbWaves * 64);
    __syncthreads();

    GradLds& gl = reinterpret_cast<GradLds*>(glds_raw)[PG ? wave : 0];      // never dereferenced unless PG
    DecGradAcc acc;                                  // PG: a wave's sums over its tiles
    if constexpr (PG) dec_grad_zero(acc);
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
        float up[2][4];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) {
            float4 gf = make_float4(0.f, 0.f, 0.f, 0.f);
            if (valid && p.g_rgb) gf = *reinterpret_cast<const float4*>(p.g_rgb + pt * 32 + 16 * ot + 4 * g);
            up[ot][0] = gf.x; up[ot][1] = gf.y; up[ot][2] = gf.z; up[ot][3] = gf.w;
        }
        f32x4 dO[2];
        colour_logit_grad(o, up, dO);
        f32x4 dH[4];
        f32x4 dF[2];
        if constexpr (DEC16) decoder_bwd16_lds(wfwd, w1t, w0t, ln, dO, dsig, hp, dH, dF);
        else decoder_bwd_lds(wfwd, w1t, w0t, ln, dO, dsig, hp, dH, dF);
        // (dF: lane (j, g), register r of tile ft -> feature channel 16 ft + 4 g + r of point j)

        // (a lane past M: dO = dsig = 0, so it adds nothing to the decoder gradients)
        if constexpr (PG) dec_grad_tile(acc, gl, j, g, f, h, dH, dO, dsig);

        if constexpr (DCOORD) {
            // ---- positional derivative of the gather: this lane's share (its 8 channels)
            float dq[3];
            gather_position_grad(a, b, g, q, dF, sx, sy, dq);
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
            // dL/dF transposed through LDS, then run-merged atomics into all three planes; a lane past M publishes weight 0
#pragma unroll
            for (int ft = 0; ft < 2; ++ft) publish_df(lds, j, g, ft, dF[ft]);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                if (g == pl) publish_taps(lds, pl, taps[pl], j, valid);
            WAVE_SYNC();
            scatter_tile_runs<6>(lds, p.d_planes + (size_t)b * 3 * a.H * a.W * 32, (size_t)a.H * a.W * 32, lane);
        }
        WAVE_SYNC();                            // the next tile overwrites the wave's LDS tables
    }
    if constexpr (PG) {
        if (sch.begin < sch.end) dec_grad_flush(acc, dg, a.decoder_lr_mul, lane);      // (a wave without a tile holds zeros)
    }
}

template <bool DEC16, bool PG, bool DCOORD>
static int launch(const QueryBwdParams& p, const DecGrads& dg, hipStream_t s) {
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
static int launch_c(const QueryBwdParams& p, const DecGrads& dg, hipStream_t s) {
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
    const DecGrads dg = {q->d_dec_w0, q->d_dec_b0, q->d_dec_w1, q->d_dec_b1};
    const bool dec16 = q->planes_absmax != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return pg ? launch_c<true, true>(p, dg, s) : launch_c<true, false>(p, dg, s);
    return pg ? launch_c<false, true>(p, dg, s) : launch_c<false, false>(p, dg, s);
}
