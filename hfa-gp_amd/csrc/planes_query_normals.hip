// Density gradient and unit surface normal at arbitrary 3-D points (gfx950): the point query (planes_query.hip) with the per-sample
// arithmetic of the per-ray normals (raymarch_normals.hip) — a point is a ray sample with compositing weight 1 and no depth.
// Notation of include/hfagp.h (hfagp_planes_query_normals):
//   q = fp32(2 / box_warp) p,  F = plane-mean gather,  hp = W0' F + b0',  sigma / rgb = the decoder of hfagp_planes_query (its bits),
//   a = d sigma / dF = W0'^T (wsig * sigmoid(hp)),  g = (2 / box_warp) J^T a  (J = dF / dq),  n = -g rsqrt(g.g + 1e-12).
// Mapping to the hardware: planes_query_kernel's, explicit points only —
//   * a wave owns one 16-point tile at a time: lane = 16 g + j, j = point in the tile, g = channel octet; ray_schedule gives each
//     XCD one contiguous run of tiles; Bc = 1 broadcasts one point set; a lane past M recomputes the last point and stores nothing;
//   * the decoder lives in registers exactly as in planes_query_kernel (decoder_fwd / decoder_fwd16 with the pre-activations kept):
//     sigma and rgb are that kernel's instruction sequence on the same inputs;
//   * a runs on the exact fp32 matrix instructions with either decoder (w0t_mul on the image of build_grad_lds, 8 KB of LDS): the
//     choice of normals_pass_a, so that the backward (planes_query_normals_bwd.hip) forms the same n;
//   * g: gather_position_grad on the twelve lines the gather has just pulled in, the four channel groups of a point summed with two
//     cross-row shuffles (point_density_grad, raymarch_normals_common.h, shared with the backward).
// One writer per point, plain stores, fixed butterfly order: two calls give the same bits.
#include <type_traits>
#include "raymarch_normals_common.h"
#include "planes_query_common.h"

namespace hfagp {

struct QueryNrmParams {
    HfagpRaymarchArgs a;       // planes, decoder, B / H / W, plane_axes, decoder_lr_mul, planes_absmax (the shared helpers' view)
    const float* coords;       // [Bc][M][3]
    float* sigma;              // NULL or [B] x out_stride floats apart, [M] inside an identity
    float* rgb;                // NULL or the same layout x 32
    float* grad;               // NULL or the same layout x 3: g
    float* normal;             // NULL or the same layout x 3: n
    long long M;               // points per identity
    long long out_stride;      // elements between identities in sigma (rgb: x 32, grad / normal: x 3)
    long long tiles_per_b;     // ceil(M / 16)
    long long total_tiles;
    long long coords_bstride;  // elements between identities in coords (0: broadcast)
    float coord_scale;         // fp32(2 / box_warp), as RayParams::coord_scale
};

template <bool DEC16, bool RGB>
__global__ void __launch_bounds__(256) planes_query_normals_kernel(const QueryNrmParams p) {
    __shared__ float w0t[2 * 16 * 64];                       // fp32 A operands of W0'^T (build_grad_lds)
    const HfagpRaymarchArgs& a = p.a;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (uniform: scalar schedule)
    const int j = lane & 15, g = lane >> 4;
    typename std::conditional<DEC16, Dec16Regs, DecoderRegs>::type dec;
    if constexpr (DEC16) {
        DecoderRegs dec32;
        load_decoder(a, j, g, dec32);
        make_dec16(dec32, a.planes_absmax, lane, dec);
    } else {
        load_decoder(a, j, g, dec);
    }
    build_grad_lds<false>(a, nullptr, w0t, threadIdx.x, 256);
    __syncthreads();
    // d pixel / d grid coordinate (plane_pixel) times the mean over the planes
    const float sx = (float)a.W * 0.5f * 0.3333333333333333f, sy = (float)a.H * 0.5f * 0.3333333333333333f;
    const RaySchedule sch = ray_schedule(p.total_tiles, wave);
#pragma unroll 1
    for (long long t = sch.begin; t < sch.end; t += sch.stride) {
        const int b = __builtin_amdgcn_readfirstlane((int)(t / p.tiles_per_b));     // wave-uniform
        const long long m0 = (t - (long long)b * p.tiles_per_b) * 16;
        const bool valid = m0 + j < p.M;
        const long long m = min(m0 + j, p.M - 1);            // a lane past M recomputes the last point and stores nothing
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
        f32x4 hp[4], h[4], o[2];
        float sigma;
        if constexpr (DEC16) decoder_fwd16<true>(dec, f, hp, h, sigma, o);
        else decoder_fwd<true>(dec, f, hp, h, sigma, o);
        const long long out = (long long)b * p.out_stride + m;                  // 64-bit: B * M * 32 passes 2^31
        if (p.sigma && valid && g == 0) __builtin_nontemporal_store(sigma, p.sigma + out);
        if constexpr (RGB) {
            if (valid) {
#pragma unroll
                for (int ot = 0; ot < 2; ++ot) {
                    f32x4 cv;
#pragma unroll
                    for (int k = 0; k < 4; ++k) cv[k] = sigmoid_f(o[ot][k]) * 1.002f - 0.001f;
                    __builtin_nontemporal_store(cv, reinterpret_cast<f32x4*>(p.rgb + out * 32 + 16 * ot + 4 * g));
                }
            }
        }
        if (p.grad || p.normal) {              // (uniform over the launch)
            // a = W0'^T (wsig * sigmoid(hp)) in fp32 with either decoder, then g and 1 / r
            f32x4 dH[4], av[2];
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) dH[mt][r] = dec.wsig[mt][r] * sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
            w0t_mul(w0t, lane, dH, av);
            float gw[3];
            const float rs = point_density_grad(a, b, g, q, av, sx, sy, p.coord_scale, gw);
            if (valid && g == 0) {
                if (p.grad) {
                    float* dst = p.grad + out * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) dst[k] = gw[k];
                }
                if (p.normal) {
                    float* dst = p.normal + out * 3;
#pragma unroll
                    for (int k = 0; k < 3; ++k) dst[k] = -rs * gw[k];
                }
            }
        }
    }
}

template <bool DEC16, bool RGB>
static int launch(const QueryNrmParams& p, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of tiles (planes_query.hip)
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, planes_query_normals_kernel<DEC16, RGB>, 256, 0) != hipSuccess || n < 1) n = 1;
        resident = n;
    }
    long long blocks = (p.total_tiles + 3) / 4;
    const long long cap = (long long)kNumCU * resident;
    if (blocks > cap) blocks = cap;
    planes_query_normals_kernel<DEC16, RGB><<<(unsigned)blocks, 256, 0, s>>>(p);
    return check_launch("planes_query_normals");
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_planes_query_normals(const HfagpPlanesQueryArgs* q, float* grad, float* normal, void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "planes_query_normals: null pointer");
    HFAGP_REQUIRE(q->planes && q->dec_w0 && q->dec_b0 && q->dec_w1 && q->dec_b1, HFAGP_EBADARG, "planes_query_normals: null pointer");
    HFAGP_REQUIRE(q->coords, HFAGP_EUNSUPPORTED, "planes_query_normals: explicit points only (no grid mode)");
    HFAGP_REQUIRE(q->sigma || q->rgb || grad || normal, HFAGP_EBADARG,
                  "planes_query_normals: null pointer (sigma, rgb, grad, normal: pass at least one output)");
    HFAGP_REQUIRE(q->B > 0 && q->H > 1 && q->W > 1, HFAGP_EBADARG, "planes_query_normals: bad dims B=%d H=%d W=%d", q->B, q->H, q->W);
    HFAGP_REQUIRE((long long)q->H * q->W <= (1ll << 25), HFAGP_EUNSUPPORTED,
                  "planes_query_normals: planes of %d x %d texels (32-bit texel offsets need H * W <= 2^25)", q->H, q->W);
    HFAGP_REQUIRE(q->plane_axes == 0 || q->plane_axes == 1, HFAGP_EBADARG, "planes_query_normals: plane_axes must be 0 or 1");
    HFAGP_REQUIRE(q->box_warp > 0.0, HFAGP_EBADARG, "planes_query_normals: box_warp must be > 0");
    HFAGP_REQUIRE(q->M > 0, HFAGP_EBADARG, "planes_query_normals: M must be > 0");
    HFAGP_REQUIRE(q->Bc == 1 || q->Bc == q->B, HFAGP_EBADARG, "planes_query_normals: Bc=%d must be 1 or B=%d", q->Bc, q->B);
    HFAGP_REQUIRE(q->out_stride == 0 || q->out_stride >= q->M, HFAGP_EBADARG,
                  "planes_query_normals: out_stride %lld < %lld points per identity", (long long)q->out_stride, (long long)q->M);
    QueryNrmParams p = {};
    p.a.planes = q->planes;
    p.a.dec_w0 = q->dec_w0; p.a.dec_b0 = q->dec_b0; p.a.dec_w1 = q->dec_w1; p.a.dec_b1 = q->dec_b1;
    p.a.B = q->B; p.a.H = q->H; p.a.W = q->W;
    p.a.plane_axes = q->plane_axes;
    p.a.box_warp = (float)q->box_warp;
    p.a.decoder_lr_mul = q->decoder_lr_mul;
    p.a.planes_absmax = q->planes_absmax;
    p.coords = q->coords;
    p.sigma = q->sigma;
    p.rgb = q->rgb;
    p.grad = grad;
    p.normal = normal;
    p.coord_scale = (float)(2.0 / q->box_warp);
    p.M = q->M;
    p.tiles_per_b = (q->M + 15) / 16;
    p.coords_bstride = q->Bc == 1 ? 0 : q->M * 3;
    p.out_stride = q->out_stride ? q->out_stride : p.M;
    p.total_tiles = p.tiles_per_b * q->B;
    const bool dec16 = q->planes_absmax != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return q->rgb ? launch<true, true>(p, s) : launch<true, false>(p, s);
    return q->rgb ? launch<false, true>(p, s) : launch<false, false>(p, s);
}
