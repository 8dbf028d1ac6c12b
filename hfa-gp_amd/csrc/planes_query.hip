// Tri-plane point queries (gfx950): raw density and the 32 decoder features at arbitrary 3-D points — the geometry side of
// EG3D's TriPlaneGenerator (sample / sample_mixed) and the density volume of gen_samples.py --shapes, without the ray
// marcher's ray generation, compositing and importance re-sampling.
//
// Mapping to the hardware (the renderer's, raymarch.hip):
//   * a wave owns one 16-point tile at a time: lane = 16*g + j, j = point in the tile, g = channel octet.  Lane (j, g) gathers
//     channels 8g..8g+7 of point j (raymarch_common.h plane_taps + gather8), which is the B-operand image of the decoder's
//     MFMAs (decoder_fwd: exact fp32 matrix instructions; decoder_fwd16: split fp16 operands, given a planes_absmax bound).
//   * sigma is the decoder's raw output 0 (no softplus: that belongs to the ray marcher); rgb = sigmoid(x[1:]) * 1.002 - 0.001.
//     The sigma-only instance never reads the colour logits, so layer 2's colour MFMAs are dead code there and vanish.
//   * point sources: explicit coordinates [Bc][M][3] (Bc = 1: one point set for every identity), or a lattice generated in
//     the kernel (grid mode): tile = 16 consecutive iz of one (ix, iy) row, so the (x,y) taps are shared by the tile and the
//     other two planes are read along a row.
//   * schedule: raymarch_common.h ray_schedule — each XCD walks one contiguous run of tiles (an x range of the lattice), so
//     its 4 MB L2 holds plane bands instead of refetching them.
#include <type_traits>
#include "raymarch_common.h"
#include "planes_query_common.h"

namespace hfagp {

struct QueryParams {
    HfagpRaymarchArgs a;       // planes, decoder, B / H / W, plane_axes, decoder_lr_mul, planes_absmax (the shared helpers' view)
    const float* coords;       // explicit: [Bc][M][3]; NULL: grid mode
    float* sigma;              // [B] x out_stride floats apart; inside an identity: [M] or [x_count][N][N]
    float* rgb;                // NULL or the same layout x 32
    long long M;               // points per identity (grid: x_count * N * N)
    long long out_stride;      // elements between identities in sigma (rgb: x 32)
    long long tiles_per_b;     // explicit: ceil(M / 16); grid: x_count * N * tz
    long long total_tiles;
    long long coords_bstride;  // elements between identities in coords (0: broadcast)
    int N, x_begin, tz;        // grid: points per axis, first x of the slab, tiles per (ix, iy) row = ceil(N / 16)
    float coord_scale;         // fp32(2 / box_warp), as RayParams::coord_scale
    float voxel, origin;       // grid: fp32(cube_length / (N - 1)), fp32(-cube_length / 2)
};

// (scale_rn / lattice_rn, the point normalisation: planes_query_common.h, shared with the backward)

template <bool DEC16, bool RGB, bool GRID>
__global__ void __launch_bounds__(256) planes_query_kernel(const QueryParams p) {
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
    const RaySchedule sch = ray_schedule(p.total_tiles, wave);
#pragma unroll 1
    for (long long t = sch.begin; t < sch.end; t += sch.stride) {
        const int b = __builtin_amdgcn_readfirstlane((int)(t / p.tiles_per_b));     // wave-uniform
        const long long r = t - (long long)b * p.tiles_per_b;
        long long m;          // index of point j inside its identity's output
        bool valid;
        float q[3];
        if constexpr (GRID) {
            const long long row = r / p.tz;                                      // (ix - x_begin) * N + iy
            const int iz0 = (int)(r - row * p.tz) * 16;
            const int iz = min(iz0 + j, p.N - 1);
            valid = iz0 + j < p.N;
            const int ixl = (int)(row / p.N), iy = (int)(row - (long long)ixl * p.N);
            m = row * p.N + iz;
            const int idx[3] = {p.x_begin + ixl, iy, iz};
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = scale_rn(p.coord_scale, lattice_rn(idx[k], p.voxel, p.origin));
        } else {
            const long long m0 = r * 16;
            valid = m0 + j < p.M;
            m = min(m0 + j, p.M - 1);
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
        f32x4 h[4], o[2];
        float sigma;
        if constexpr (DEC16) decoder_fwd16<false>(dec, f, h, h, sigma, o);
        else decoder_fwd<false>(dec, f, h, h, sigma, o);
        const long long out = (long long)b * p.out_stride + m;                  // 64-bit: B * M * 32 passes 2^31
        if (valid && g == 0) __builtin_nontemporal_store(sigma, p.sigma + out);
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
    }
}

template <bool DEC16, bool RGB, bool GRID>
static int launch(const QueryParams& p, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of tiles (the sigma-only instances hold 3 waves per SIMD,
    // the rgb ones 2: a fixed cap would leave a second, partial round of blocks for the tail)
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, planes_query_kernel<DEC16, RGB, GRID>, 256, 0) != hipSuccess || n < 1) n = 2;
        resident = n;
    }
    long long blocks = (p.total_tiles + 3) / 4;
    const long long cap = (long long)kNumCU * resident;
    if (blocks > cap) blocks = cap;
    planes_query_kernel<DEC16, RGB, GRID><<<(unsigned)blocks, 256, 0, s>>>(p);
    return check_launch("planes_query");
}

template <bool DEC16, bool RGB>
static int launch_src(const QueryParams& p, hipStream_t s) {
    return p.coords ? launch<DEC16, RGB, false>(p, s) : launch<DEC16, RGB, true>(p, s);
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_planes_query(const HfagpPlanesQueryArgs* q, void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "planes_query: null pointer");
    HFAGP_REQUIRE(q->planes && q->dec_w0 && q->dec_b0 && q->dec_w1 && q->dec_b1 && q->sigma, HFAGP_EBADARG,
                  "planes_query: null pointer");
    HFAGP_REQUIRE(q->B > 0 && q->H > 1 && q->W > 1, HFAGP_EBADARG, "planes_query: bad dims B=%d H=%d W=%d", q->B, q->H, q->W);
    HFAGP_REQUIRE((long long)q->H * q->W <= (1ll << 25), HFAGP_EUNSUPPORTED,
                  "planes_query: planes of %d x %d texels (32-bit texel offsets need H * W <= 2^25)", q->H, q->W);
    HFAGP_REQUIRE(q->plane_axes == 0 || q->plane_axes == 1, HFAGP_EBADARG, "planes_query: plane_axes must be 0 or 1");
    HFAGP_REQUIRE(q->box_warp > 0.0, HFAGP_EBADARG, "planes_query: box_warp must be > 0");
    QueryParams p = {};
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
    p.coord_scale = (float)(2.0 / q->box_warp);
    if (q->coords) {
        HFAGP_REQUIRE(q->M > 0, HFAGP_EBADARG, "planes_query: M must be > 0");
        HFAGP_REQUIRE(q->Bc == 1 || q->Bc == q->B, HFAGP_EBADARG, "planes_query: Bc=%d must be 1 or B=%d", q->Bc, q->B);
        p.M = q->M;
        p.tiles_per_b = (q->M + 15) / 16;
        p.coords_bstride = q->Bc == 1 ? 0 : q->M * 3;
    } else {
        HFAGP_REQUIRE(q->N >= 2, HFAGP_EBADARG, "planes_query: grid of N=%d points per axis (N >= 2)", q->N);
        HFAGP_REQUIRE(q->x_begin >= 0 && q->x_count > 0 && (long long)q->x_begin + q->x_count <= q->N, HFAGP_EBADARG,
                      "planes_query: x slab [%d, %d + %d) outside [0, %d)", q->x_begin, q->x_begin, q->x_count, q->N);
        HFAGP_REQUIRE(q->cube_length > 0.0, HFAGP_EBADARG, "planes_query: cube_length must be > 0");
        p.N = q->N;
        p.x_begin = q->x_begin;
        p.tz = (q->N + 15) / 16;
        p.M = (long long)q->x_count * q->N * q->N;
        p.tiles_per_b = (long long)q->x_count * q->N * p.tz;
        p.voxel = (float)(q->cube_length / (double)(q->N - 1));
        p.origin = (float)(-q->cube_length / 2.0);
    }
    HFAGP_REQUIRE(q->out_stride == 0 || q->out_stride >= p.M, HFAGP_EBADARG,
                  "planes_query: out_stride %lld < %lld points per identity", (long long)q->out_stride, p.M);
    p.out_stride = q->out_stride ? q->out_stride : p.M;
    p.total_tiles = p.tiles_per_b * q->B;
    const bool dec16 = q->planes_absmax != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return q->rgb ? launch_src<true, true>(p, s) : launch_src<true, false>(p, s);
    return q->rgb ? launch_src<false, true>(p, s) : launch_src<false, false>(p, s);
}
