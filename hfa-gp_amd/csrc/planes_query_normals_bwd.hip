// Backward of the point normals (planes_query_normals.hip) for explicit points (gfx950): from G_g = dL/dg and / or G_n = dL/dn at
// the points to dL/dplanes and the decoder-parameter gradients.  It is the "through the normals" branch of
// raymarch_normals_bwd.hip with omega = 1 and d sigma_s = 0, on the tile layout of planes_query_bwd.hip.  Notation of
// include/hfagp.h (hfagp_planes_query_normals_bwd):
//   per 16-point tile (a wave; lane = 16 g + j, j = point, g = channel group, as the forward):
//     plane_taps + gather8 (the forward's bits: scale_rn of planes_query_common.h) -> decoder forward as far as hp ->
//     dH = wsig sigmoid(hp), a = W0'^T dH (fp32) -> g, 1 / r, n (point_density_grad: the forward's lines) ->
//     gamma = G_g - (1 / r)(G_n - n (n . G_n)), gamma_q = coord_scale gamma -> the derivative weights w'_k (normals_second_taps) ->
//     u = sum texel w'_k / 3 (a second gather of the same twelve lines) -> v = W0' u -> e = dH (1 - sigmoid(hp)) v -> dF = W0'^T e;
//   d planes: one run-merged line scatter with two value / weight sets, (dF, w_k / 3) and (a, w'_k / 3)
//     (scatter_tile_runs2<6>: all three planes at their true texels, as planes_query_bwd.hip and for its reason);
//   decoder gradients (PG): dW0' += e F^T + dH u^T, db0' += e, dwsig += sigmoid(hp) v, summed per wave over its tiles, one flush
//     at the end (nrm_grad_* of decoder_adjoint.h); the colour rows of W1 and all of b1 receive nothing.
// The products v, W0'^T e, a and the weight-gradient products run on the exact fp32 MFMA with either decoder: u is not bounded by
// planes_absmax, so the forward's fp16 operand scaling does not carry over.  A point whose two upstream vectors are exactly 0
// publishes weight 0; a tile of such points is skipped; a wave that saw none flushes nothing.
// Schedule: raymarch_common.h ray_schedule over tiles, one round of resident workgroups.
#include "raymarch_normals_common.h"
#include "planes_query_common.h"

namespace hfagp {

constexpr int kQnWaves = 4;

struct QueryNrmBwdParams {
    HfagpRaymarchArgs a;       // planes, decoder, B / H / W, plane_axes, decoder_lr_mul, planes_absmax (the shared helpers' view)
    const float* coords;       // [Bc][M][3]
    const float* g_grad;       // [B][M][3] or NULL
    const float* g_normal;     // [B][M][3] or NULL
    float* d_planes;           // [B][3][H][W][32] or NULL, accumulated into
    long long M, tiles_per_b, total_tiles;
    long long coords_bstride;  // elements between identities in coords (0: broadcast)
    float coord_scale;         // fp32(2 / box_warp), as the forward
};

template <bool DEC16, bool PG>
__global__ void __launch_bounds__(kQnWaves * 64, PG ? 1 : 2)
planes_query_normals_bwd_kernel(const QueryNrmBwdParams p, const DecGrads dg) {
    __shared__ Tile2Lds lds_all[kQnWaves];
    __shared__ __attribute__((aligned(16))) float glds_raw[PG ? kQnWaves * sizeof(NrmGradLds) / sizeof(float) : 1];
    __shared__ float w0t[2 * 16 * 64];                       // fp32 A operands of W0'^T (build_grad_lds)
    __shared__ float w0f[DEC16 ? 32 * 64 : 1];               // fp32 A operands of W0' (fp32 decoder: rows 0-31 of wfwd)
    __shared__ float wfwd[kDecLdsRows * 64];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    build_grad_lds<false>(a, nullptr, w0t, threadIdx.x, kQnWaves * 64);
    if constexpr (DEC16) build_w0_lds(a, w0f, threadIdx.x, kQnWaves * 64);
    __syncthreads();
    const float* w0fwd = DEC16 ? w0f : wfwd;
    Tile2Lds& lds = lds_all[wave];
    NrmGradLds& gl = reinterpret_cast<NrmGradLds*>(glds_raw)[PG ? wave : 0];      // never dereferenced unless PG
    NrmGradAcc acc;
    bool any = false;                               // this wave has a point with a gradient (wave-uniform)
    if constexpr (PG) {
#pragma unroll
        for (int x = 0; x < 4; ++x) {
#pragma unroll
            for (int y = 0; y < 2; ++y) acc.aw0[x][y] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int y = 0; y < 4; ++y) { acc.s_x[x][y] = 0.f; acc.s_sw[x][y] = 0.f; }
        }
        acc.s_ds = 0.f;
    }
    // d pixel / d grid coordinate (plane_pixel); sx, sy: the same times the mean over the planes
    const float hx = (float)a.W * 0.5f, hy = (float)a.H * 0.5f;
    const float sx = hx * 0.3333333333333333f, sy = hy * 0.3333333333333333f;
    const size_t plane_stride = (size_t)a.H * a.W * 32;

    const RaySchedule sch = ray_schedule(p.total_tiles, wave, kQnWaves);
#pragma unroll 1
    for (long long t = sch.begin; t < sch.end; t += sch.stride) {
        const int b = __builtin_amdgcn_readfirstlane((int)(t / p.tiles_per_b));     // wave-uniform
        const long long m0 = (t - (long long)b * p.tiles_per_b) * 16;
        const bool valid = m0 + j < p.M;
        const long long m = min(m0 + j, p.M - 1);            // a lane past M recomputes the last point and contributes nothing
        const long long pt = (long long)b * p.M + m;
        // upstream gradients; a point without one is dead, a tile without a live point is skipped
        float Gg[3] = {0.f, 0.f, 0.f}, Gn[3] = {0.f, 0.f, 0.f};
        if (valid) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (p.g_grad) Gg[k] = p.g_grad[pt * 3 + k];
                if (p.g_normal) Gn[k] = p.g_normal[pt * 3 + k];
            }
        }
        const bool live = Gg[0] != 0.f || Gg[1] != 0.f || Gg[2] != 0.f || Gn[0] != 0.f || Gn[1] != 0.f || Gn[2] != 0.f;
        if (__builtin_amdgcn_ballot_w64(live) == 0) continue;
        any = true;
        float q[3];
        {
            const float* c = p.coords + (long long)b * p.coords_bstride + m * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = scale_rn(p.coord_scale, c[k]);
        }
        PlaneTaps taps[3], dtaps[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            float gx, gy;
            plane_coords(a, q, pl, gx, gy);
            plane_taps(a, gx, gy, taps[pl]);
        }
        float f[8], u[8];
        gather8(a, b, g, taps, f);
        int ln = lane;
        asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
        f32x4 hp[4], h[4], o[2];
        float sigma;
        if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
        else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);
        f32x4 dH[4], av[2];                  // dH = wsig sigmoid(hp); av = a = W0'^T dH (the forward's)
        decoder_dh_lds<DEC16>(wfwd, ln, hp, dH);
        w0t_mul(w0t, ln, dH, av);
        float gw[3];
        const float rs = point_density_grad(a, b, g, q, av, sx, sy, p.coord_scale, gw);
        // gamma_q = coord_scale (G_g - (1 / r)(G_n - n (n . G_n)))
        float gq[3];
        {
            const float n3[3] = {-rs * gw[0], -rs * gw[1], -rs * gw[2]};
            normals_gamma_q(Gn, n3, 1.f, rs, p.coord_scale, gq);
#pragma unroll
            for (int k = 0; k < 3; ++k) gq[k] = fmaf(p.coord_scale, Gg[k], gq[k]);
        }
        // the derivative weights w'_k (and the taps again: the same bits)
        normals_second_taps(a, q, gq, hx, hy, taps, dtaps);
        gather8(a, b, g, dtaps, u);
        f32x4 v[4], x[4];
        w0_mul(w0fwd, ln, u, v);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float sg = sigmoid_f(hp[mt][r]);
                x[mt][r] = dH[mt][r] * (1.f - sg) * v[mt][r];          // e
                if constexpr (PG) {
                    acc.s_x[mt][r] += x[mt][r];
                    acc.s_sw[mt][r] += sg * v[mt][r];
                }
            }
        f32x4 dF[2];
        w0t_mul(w0t, ln, x, dF);
        // (a dead point of a live tile: gamma_q = 0, so w'_k, u, v, e and dF are 0 and it adds nothing below)
        if constexpr (PG) nrm_grad_tile(acc, gl, j, g, f, u, x, dH);
        if (p.d_planes) {                      // (uniform over the launch)
            // d planes: (w_k / 3) dF + (w'_k / 3) a; a dead point publishes weights 0
            float dfc[16], avc[16];
            publish_df2(lds, j, g, dF);
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                if (g == pl) publish_taps2(lds, pl, taps[pl], dtaps[pl], j, live);
            WAVE_SYNC();
            channel_column(lds, lane, dfc);
            WAVE_SYNC();
            publish_df2(lds, j, g, av);
            WAVE_SYNC();
            channel_column(lds, lane, avc);
            scatter_tile_runs2<6>(lds, dfc, avc, p.d_planes + (size_t)b * 3 * plane_stride, plane_stride, lane);
        }
        WAVE_SYNC();                            // the next tile overwrites the wave's LDS tables
    }
    if constexpr (PG) {
        if (any) nrm_grad_flush<false>(acc, dg, a.decoder_lr_mul, lane);
    }
}

template <bool DEC16, bool PG>
static int launch(const QueryNrmBwdParams& p, const DecGrads& dg, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of tiles
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, planes_query_normals_bwd_kernel<DEC16, PG>, kQnWaves * 64, 0) != hipSuccess ||
            n < 1)
            n = 1;
        resident = n;
    }
    long long blocks = (p.total_tiles + kQnWaves - 1) / kQnWaves;
    const long long cap = (long long)kNumCU * resident;
    if (blocks > cap) blocks = cap;
    planes_query_normals_bwd_kernel<DEC16, PG><<<(unsigned)blocks, kQnWaves * 64, 0, s>>>(p, dg);
    return check_launch("planes_query_normals_bwd");
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_planes_query_normals_bwd(const HfagpPlanesQueryBwdArgs* q, const float* g_grad, const float* g_normal,
                                              void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "planes_query_normals_bwd: null pointer");
    HFAGP_REQUIRE(q->planes && q->dec_w0 && q->dec_b0 && q->dec_w1 && q->dec_b1, HFAGP_EBADARG,
                  "planes_query_normals_bwd: null pointer");
    HFAGP_REQUIRE(q->coords, HFAGP_EUNSUPPORTED, "planes_query_normals_bwd: explicit points only (no grid mode)");
    HFAGP_REQUIRE(!q->g_sigma && !q->g_rgb, HFAGP_EBADARG,
                  "planes_query_normals_bwd: g_sigma / g_rgb must be NULL (their gradients are hfagp_planes_query_bwd's)");
    HFAGP_REQUIRE(!q->d_coords, HFAGP_EBADARG, "planes_query_normals_bwd: d_coords must be NULL (no point gradient of the normals)");
    HFAGP_REQUIRE(g_grad || g_normal, HFAGP_EBADARG, "planes_query_normals_bwd: null pointer (g_grad and g_normal: pass at least one)");
    const bool pg = q->d_dec_w0 || q->d_dec_b0 || q->d_dec_w1 || q->d_dec_b1;
    HFAGP_REQUIRE(!pg || (q->d_dec_w0 && q->d_dec_b0 && q->d_dec_w1 && q->d_dec_b1), HFAGP_EBADARG,
                  "planes_query_normals_bwd: the four decoder gradients go together (all or none)");
    HFAGP_REQUIRE(q->d_planes || pg, HFAGP_EBADARG, "planes_query_normals_bwd: null pointer (d_planes, d_dec_*: pass at least one output)");
    HFAGP_REQUIRE(q->B > 0 && q->H > 1 && q->W > 1, HFAGP_EBADARG, "planes_query_normals_bwd: bad dims B=%d H=%d W=%d", q->B, q->H, q->W);
    HFAGP_REQUIRE((long long)q->H * q->W <= (1ll << 25), HFAGP_EUNSUPPORTED,
                  "planes_query_normals_bwd: planes of %d x %d texels (32-bit texel offsets need H * W <= 2^25)", q->H, q->W);
    HFAGP_REQUIRE(q->plane_axes == 0 || q->plane_axes == 1, HFAGP_EBADARG, "planes_query_normals_bwd: plane_axes must be 0 or 1");
    HFAGP_REQUIRE(q->box_warp > 0.0, HFAGP_EBADARG, "planes_query_normals_bwd: box_warp must be > 0");
    HFAGP_REQUIRE(q->M > 0, HFAGP_EBADARG, "planes_query_normals_bwd: M must be > 0");
    HFAGP_REQUIRE(q->Bc == 1 || q->Bc == q->B, HFAGP_EBADARG, "planes_query_normals_bwd: Bc=%d must be 1 or B=%d", q->Bc, q->B);
    QueryNrmBwdParams p = {};
    p.a.planes = q->planes;
    p.a.dec_w0 = q->dec_w0; p.a.dec_b0 = q->dec_b0; p.a.dec_w1 = q->dec_w1; p.a.dec_b1 = q->dec_b1;
    p.a.B = q->B; p.a.H = q->H; p.a.W = q->W;
    p.a.plane_axes = q->plane_axes;
    p.a.box_warp = (float)q->box_warp;
    p.a.decoder_lr_mul = q->decoder_lr_mul;
    p.a.planes_absmax = q->planes_absmax;
    p.coords = q->coords;
    p.g_grad = g_grad;
    p.g_normal = g_normal;
    p.d_planes = q->d_planes;
    p.coord_scale = (float)(2.0 / q->box_warp);
    p.M = q->M;
    p.tiles_per_b = (q->M + 15) / 16;
    p.total_tiles = p.tiles_per_b * q->B;
    p.coords_bstride = q->Bc == 1 ? 0 : q->M * 3;
    const DecGrads dg = {q->d_dec_w0, q->d_dec_b0, q->d_dec_w1, q->d_dec_b1};
    const bool dec16 = q->planes_absmax != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return pg ? launch<true, true>(p, dg, s) : launch<true, false>(p, dg, s);
    return pg ? launch<false, true>(p, dg, s) : launch<false, false>(p, dg, s);
}
