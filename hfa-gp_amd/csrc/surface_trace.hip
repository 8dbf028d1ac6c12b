// First hit of a ray list with the density iso-surface sigma = level (gfx950): per ray a coarse march over steps + 1 nodes, `refine`
// bisections of the bracketing interval and one secant step, then the point, the raw density, its gradient and the unit normal at the
// hit — the surface that marching cubes exports (`extract_mesh(level=)`), met along a ray.  Notation of include/hfagp.h
// (hfagp_trace_rays); every density is the point query's (planes_query.hip) at x = o + t d, to the bit.
// Mapping to the hardware: planes_query_kernel's —
//   * a wave owns one tile of 16 rays at a time: lane = 16 g + j, j = ray in the tile, g = channel octet; ray_schedule gives each XCD
//     one contiguous run of tiles.  The four lanes of a ray carry the same ray state (the density arrives on all four: decoder_fwd);
//   * the decoder lives in registers (decoder_fwd / decoder_fwd16, the sigma-only form: layer 2's colour rows are dead code);
//   * every loop is wave-uniform: the coarse march leaves when a ballot finds all 16 rays decided, the bisection runs `refine` times
//     for the tile (a ray without a bracket evaluates a dummy point and drops the result), a tile of empty rays is skipped;
//   * NORMALS instances: at the hit, planes_query_normals_kernel's lines from the pre-activations to g and n (a = W0'^T dH on the
//     exact fp32 matrix instructions, 8 KB of LDS for its A operands).  The plain instances use no LDS.
// The ray arithmetic (nodes, points, midpoints, the secant step) is rounded after every operation — no contraction into FMAs — so
// that torch's `o + t[..., None] * d` on the returned t gives the returned point, and a restatement in torch finds the same cell.
// One writer per ray, plain stores: two calls give the same bits.
#include <type_traits>
#include "raymarch_normals_common.h"
#include "planes_query_common.h"

namespace hfagp {

struct TraceParams {
    HfagpRaymarchArgs a;       // planes, decoder, B / H / W, plane_axes, decoder_lr_mul, planes_absmax (the shared helpers' view)
    const float* ray_o, *ray_d;      // [B][R][3]
    const float* t_near, *t_far;     // [B][R]
    unsigned char* hit;        // [B][R] each, NULL = not written
    int* cell;
    float* t, *point, *sigma, *grad, *normal;
    int R;                     // rays per frame (B * R < 2^31)
    int tiles_per_b;           // ceil(R / 16)
    int total_tiles;
    float coord_scale;         // fp32(2 / box_warp), as RayParams::coord_scale
    float level;
    int steps, refine;
};

// the ray arithmetic, each operation rounded on its own (scale_rn / lattice_rn's idiom)
__device__ __forceinline__ float node_rn(float t_near, int i, float dt) {
#pragma clang fp contract(off)
    return t_near + (float)i * dt;
}
__device__ __forceinline__ void point_rn(const float o[3], const float d[3], float t, float x[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = o[k] + t * d[k];
}
__device__ __forceinline__ float mid_rn(float lo, float hi) {
#pragma clang fp contract(off)
    return 0.5f * (lo + hi);
}
__device__ __forceinline__ float secant_rn(float lo, float hi, float s_lo, float s_hi, float level) {
#pragma clang fp contract(off)
    const float den = s_hi - s_lo;
    if (!(den > 0.f)) return hi;                       // (a NaN density too)
    const float t = lo + __fdiv_rn(level - s_lo, den) * (hi - lo);
    return fminf(fmaxf(t, lo), hi);
}

// the point query at the world point x: planes_query_kernel's lines (KEEP_PRE: planes_query_normals_kernel's, with q and hp kept)
template <bool DEC16, bool KEEP_PRE, typename Dec>
__device__ __forceinline__ float density_at(const TraceParams& p, const Dec& dec, int b, int g, const float x[3], float q[3],
                                            f32x4 hp[4]) {
    const HfagpRaymarchArgs& a = p.a;
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = scale_rn(p.coord_scale, x[k]);
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
    if constexpr (DEC16) decoder_fwd16<KEEP_PRE>(dec, f, hp, h, sigma, o);
    else decoder_fwd<KEEP_PRE>(dec, f, hp, h, sigma, o);
    return sigma;
}

template <bool DEC16, bool NORMALS>
__global__ void __launch_bounds__(256) trace_rays_kernel(const TraceParams p) {
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
    [[maybe_unused]] const float* w0t = nullptr;
    if constexpr (NORMALS) {
        __shared__ float w0t_lds[2 * 16 * 64];               // fp32 A operands of W0'^T (build_grad_lds)
        build_grad_lds<false>(a, nullptr, w0t_lds, threadIdx.x, 256);
        __syncthreads();
        w0t = w0t_lds;
    }
    // d pixel / d grid coordinate (plane_pixel) times the mean over the planes
    [[maybe_unused]] const float sx = (float)a.W * 0.5f * 0.3333333333333333f, sy = (float)a.H * 0.5f * 0.3333333333333333f;
    const float fsteps = (float)p.steps;
    // the vector outputs' pointers wait in vector registers for the end of a tile: held in scalar ones across the march they are what
    // the NORMALS instances would spill (plenty of vector registers are free)
    float* out_point = p.point, *out_grad = p.grad, *out_normal = p.normal;
    asm volatile("" : "+v"(out_point), "+v"(out_grad), "+v"(out_normal));
    const RaySchedule sch = ray_schedule(p.total_tiles, wave);
    const int tile_end = (int)sch.end;
#pragma unroll 1
    for (int tile = (int)sch.begin; tile < tile_end; tile += sch.stride) {
        const int b = __builtin_amdgcn_readfirstlane(tile / p.tiles_per_b);            // wave-uniform
        const int r0 = (tile - b * p.tiles_per_b) * 16;
        const bool valid = r0 + j < p.R;
        const int ray = b * p.R + min(r0 + j, p.R - 1);      // a lane past R reads the last ray and stores nothing
        const size_t ray3 = (size_t)ray * 3;
        float o3[3], d3[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) { o3[k] = p.ray_o[ray3 + k]; d3[k] = p.ray_d[ray3 + k]; }
        const float tn = p.t_near[ray], tf = p.t_far[ray];
        // an empty ray (hfagp_raymarch_rays_limits_fwd's rule) is decided before the march: a miss
        const bool live = valid && fabsf(tn) < INFINITY && fabsf(tf) < INFINITY && tf > tn;
        int cell = -1;
        float t_hit = 0.f, lo = 0.f, hi = 0.f, s_lo = 0.f, s_hi = 0.f;
        float q[3];
        f32x4 hp[4];
        if (__builtin_amdgcn_ballot_w64(live) != 0) {
            if (!live) {                                   // every evaluation of this lane is a dummy at the origin of the volume
#pragma unroll
                for (int k = 0; k < 3; ++k) { o3[k] = 0.f; d3[k] = 0.f; }
            }
            const float tn_l = live ? tn : 0.f, tf_l = live ? tf : 0.f;
            const float dt = __fdiv_rn(tf_l - tn_l, fsteps);
            // ---- one loop, one evaluation per trip.  Coarse march: cell = first node i in 0..steps with sigma(t_i) >= level (a NaN
            // never hits); it ends when a ballot finds all 16 rays decided.  Then the bracket [t_{cell-1}, t_cell] of the rays with
            // cell > 0 is bisected `refine` times (a ray without one evaluates the dummy t = 0 and drops the result).
            bool open = live, bracket = false;
            int i = 0, left = 0;            // (uniform) next coarse node; bisections left, once the march is over
            bool marching = true;           // (uniform)
#pragma unroll 1
            for (;;) {
                const float te = marching ? (i < p.steps ? node_rn(tn_l, i, dt) : tf_l) : (bracket ? mid_rn(lo, hi) : 0.f);
                float x[3];
                point_rn(o3, d3, te, x);
                const float s = density_at<DEC16, false>(p, dec, b, g, x, q, hp);
                const bool in = s >= p.level, upd = marching ? open : bracket;
                if (marching) cell = open && in ? i : cell;
                hi = upd && in ? te : hi;    s_hi = upd && in ? s : s_hi;
                lo = upd && !in ? te : lo;   s_lo = upd && !in ? s : s_lo;
                if (marching) {
                    open = open && !in;
                    ++i;
                    if (__builtin_amdgcn_ballot_w64(open) == 0 || i > p.steps) {       // all 16 rays decided: wave-uniform exit
                        marching = false;
                        bracket = cell > 0;
                        left = __builtin_amdgcn_ballot_w64(bracket) != 0 ? p.refine : 0;
                        if (left == 0) break;
                    }
                } else if (--left == 0) {
                    break;
                }
            }
            // ---- one secant step in the final bracket; cell = 0: the origin is inside already
            t_hit = cell == 0 ? tn_l : 0.f;
            if (bracket) t_hit = secant_rn(lo, hi, s_lo, s_hi, p.level);
        }
        // ---- at the hit: the point, the density, and with NORMALS its gradient and the unit normal
        const bool hit = cell >= 0;
        float x[3] = {0.f, 0.f, 0.f}, sigma = 0.f;
        [[maybe_unused]] float gw[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
        if (__builtin_amdgcn_ballot_w64(hit) != 0) {           // (a miss evaluates the dummy point and stores zeros)
            point_rn(o3, d3, hit ? t_hit : 0.f, x);
            const float s = density_at<DEC16, NORMALS>(p, dec, b, g, x, q, hp);
            if constexpr (NORMALS) {
                // a = W0'^T (wsig * sigmoid(hp)) in fp32 with either decoder, then g and 1 / r (planes_query_normals_kernel)
                f32x4 dH[4], av[2];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dH[mt][r] = dec.wsig[mt][r] * sigmoid_f(hp[mt][r]);      // softplus' = sigmoid
                w0t_mul(w0t, lane, dH, av);
                float gv[3];
                const float rs = point_density_grad(a, b, g, q, av, sx, sy, p.coord_scale, gv);
#pragma unroll
                for (int k = 0; k < 3; ++k) { gw[k] = hit ? gv[k] : 0.f; nrm[k] = hit ? -rs * gv[k] : 0.f; }
            }
            sigma = hit ? s : 0.f;
            if (!hit) { x[0] = 0.f; x[1] = 0.f; x[2] = 0.f; }
        }
        if (valid && g == 0) {
            if (p.hit) p.hit[ray] = hit ? 1 : 0;
            if (p.cell) p.cell[ray] = cell;
            if (p.t) p.t[ray] = hit ? t_hit : 0.f;
            if (p.sigma) p.sigma[ray] = sigma;
            if (out_point) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_point[ray3 + k] = x[k];
            }
            if constexpr (NORMALS) {
                if (out_grad) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) out_grad[ray3 + k] = gw[k];
                }
                if (out_normal) {
#pragma unroll
                    for (int k = 0; k < 3; ++k) out_normal[ray3 + k] = nrm[k];
                }
            }
        }
    }
}

template <bool DEC16, bool NORMALS>
static int launch(const TraceParams& p, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of tiles (planes_query.hip)
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, trace_rays_kernel<DEC16, NORMALS>, 256, 0) != hipSuccess || n < 1) n = 1;
        resident = n;
    }
    long long blocks = ((long long)p.total_tiles + 3) / 4;
    const long long cap = (long long)kNumCU * resident;
    if (blocks > cap) blocks = cap;
    trace_rays_kernel<DEC16, NORMALS><<<(unsigned)blocks, 256, 0, s>>>(p);
    return check_launch("trace_rays");
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_trace_rays(const HfagpTraceRaysArgs* q, void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "trace_rays: null pointer");
    HFAGP_REQUIRE(q->planes && q->dec_w0 && q->dec_b0 && q->dec_w1 && q->dec_b1 && q->ray_origins && q->ray_directions && q->t_near &&
                      q->t_far,
                  HFAGP_EBADARG, "trace_rays: null pointer");
    HFAGP_REQUIRE(q->hit || q->cell || q->t || q->point || q->sigma || q->sigma_grad || q->normal, HFAGP_EBADARG,
                  "trace_rays: null pointer (pass at least one output)");
    HFAGP_REQUIRE(q->steps >= 1 && q->steps <= 4096, HFAGP_EBADARG, "trace_rays: steps = %d outside [1, 4096]", q->steps);
    HFAGP_REQUIRE(q->refine >= 0 && q->refine <= 30, HFAGP_EBADARG, "trace_rays: refine = %d outside [0, 30]", q->refine);
    HFAGP_REQUIRE(q->B > 0 && q->H > 1 && q->W > 1 && q->R > 0, HFAGP_EBADARG, "trace_rays: bad dims B=%d H=%d W=%d R=%lld", q->B, q->H,
                  q->W, (long long)q->R);
    HFAGP_REQUIRE((long long)q->H * q->W <= (1ll << 25), HFAGP_EUNSUPPORTED,
                  "trace_rays: planes of %d x %d texels (32-bit texel offsets need H * W <= 2^25)", q->H, q->W);
    HFAGP_REQUIRE((long long)q->B * ((q->R + 15) / 16 * 16) < (1ll << 31), HFAGP_EUNSUPPORTED, "trace_rays: too many rays");
    HFAGP_REQUIRE(q->plane_axes == 0 || q->plane_axes == 1, HFAGP_EBADARG, "trace_rays: plane_axes must be 0 or 1");
    HFAGP_REQUIRE(q->box_warp > 0.0, HFAGP_EBADARG, "trace_rays: box_warp must be > 0");
    TraceParams p = {};
    p.a.planes = q->planes;
    p.a.dec_w0 = q->dec_w0; p.a.dec_b0 = q->dec_b0; p.a.dec_w1 = q->dec_w1; p.a.dec_b1 = q->dec_b1;
    p.a.B = q->B; p.a.H = q->H; p.a.W = q->W;
    p.a.plane_axes = q->plane_axes;
    p.a.box_warp = (float)q->box_warp;
    p.a.decoder_lr_mul = q->decoder_lr_mul;
    p.a.planes_absmax = q->planes_absmax;
    p.ray_o = q->ray_origins; p.ray_d = q->ray_directions;
    p.t_near = q->t_near; p.t_far = q->t_far;
    p.hit = q->hit; p.cell = q->cell; p.t = q->t; p.point = q->point; p.sigma = q->sigma;
    p.grad = q->sigma_grad; p.normal = q->normal;
    p.R = (int)q->R;
    p.tiles_per_b = (int)((q->R + 15) / 16);
    p.total_tiles = p.tiles_per_b * q->B;
    p.coord_scale = (float)(2.0 / q->box_warp);
    p.level = q->level;
    p.steps = q->steps; p.refine = q->refine;
    const bool dec16 = q->planes_absmax != nullptr, normals = q->sigma_grad || q->normal;
    hipStream_t s = (hipStream_t)stream;
    if (dec16) return normals ? launch<true, true>(p, s) : launch<true, false>(p, s);
    return normals ? launch<false, true>(p, s) : launch<false, false>(p, s);
}
