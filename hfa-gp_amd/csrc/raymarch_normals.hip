// Per-ray surface normals of the ray marcher: N = sum_s omega_s n_s over the Sc + Sf samples of the final (merged, depth-sorted)
// pass, with
//   g(x)  = d sigma / d x      the world-space gradient of the RAW decoder density (before softplus(sigma - 1)) at the sample
//   n(x)  = -g rsqrt(g.g + 1e-12)                      unit normal from dense to empty; exactly 0 where g is exactly 0
//   omega = (w_{r-1} + w_r) / 2 at sorted position r   the colour weight of the forward kernel (raymarch.hip)
// so N is what MipRayMarcher2 composites with the per-sample normals as "colours" (before its * 2 - 1); |N| <= sum of weights.
// N is not normalised and white_back does not enter.  Forward only.
//
// Input: the arguments of the forward call and the `state` it filled; of the 35 floats per sample the sorted depths and densities
// are read (the colours are not; the samples are walked in depth order, so the sort index is not needed either).
//
//   raymarch_normals_kernel   one wave per ray.  Per ray the compositing scan of the forward (same formulas, same shuffle scans:
//                             the same omega bits).  Per 16-sample tile, in the lane mapping of raymarch_bwd_camera_kernel
//                             (lane = 16 g + j: sample j of the tile, channel group g): gather -> decoder forward as far as the
//                             hidden pre-activations -> decoder adjoint of d sigma = 1 with no colour gradient = d sigma / dF ->
//                             positional derivative of the bilinear gather (plane_taps_d) -> the four channel groups of a sample
//                             summed with two shuffles -> n_s -> omega_s n_s on the lanes g == 0.  One writer per ray, plain
//                             stores, fixed butterfly order: two calls give the same bits.
//   raymarch_normals_kernel<.., LIST = true>   the same on a caller's ray list (hfagp_raymarch_rays_normals): the state is the one
//                             raymarch_rays_kernel filled.
#include "decoder_adjoint.h"

namespace hfagp {

constexpr int kNrmWaves = 4;

// LIST: the rays of a caller's list (raymarch_common.h ray_fetch; directions as given) instead of the pinhole grid.  With per-ray
// limits (RayParams::t_near / t_far) an EMPTY ray (raymarch.hip's predicate) stores three zeros and reads nothing of its `state`,
// which the forward never wrote.  (The ray fetch is a template parameter of the kernel, not a shared body function: moving the code
// into one changed the grid instantiations' register allocation — DESIGN.md has the table.)
template <int S, bool DEC16, bool LIST = false>
__global__ void __launch_bounds__(kNrmWaves * 64, 2)
raymarch_normals_kernel(const RayParams p, float* __restrict__ normal) {
    __shared__ float w0t[2 * 16 * 64];
    __shared__ float wfwd[kDecLdsRows * 64];
    __shared__ float ray_ts[kNrmWaves][S], ray_ss[kNrmWaves][S], ray_om[kNrmWaves][S];     // by sorted position
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    const int R = LIST ? p.R : a.res * a.res;
    constexpr int NT = S / 16;
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    if constexpr (DEC16) build_grad16_lds<false>(a, nullptr, w0t, lane, wave, kNrmWaves);
    else build_grad_lds<false>(a, nullptr, w0t, threadIdx.x, kNrmWaves * 64);
    __syncthreads();
    float* ts = ray_ts[wave];
    float* ss = ray_ss[wave];
    float* om = ray_om[wave];
    // d pixel / d grid coordinate (plane_pixel) times the mean over the planes
    const float sx = (float)a.W * 0.5f * 0.3333333333333333f, sy = (float)a.H * 0.5f * 0.3333333333333333f;
    const RaySchedule sch = ray_schedule((long long)p.total_rays, wave, kNrmWaves);
    for (long long rp = sch.begin; rp < sch.end; rp += sch.stride) {
        int b, ray;
        float o3[3], d3[3];
        if constexpr (LIST) {
            int ray_v;
            ray_fetch<true>(p, __builtin_amdgcn_readfirstlane((int)rp), R, b, ray_v, o3, d3);
            ray = __builtin_amdgcn_readfirstlane(ray_v);
            if (p.t_near) {                         // (wave-uniform: the limit-less list call never enters)
                const float t_near = p.t_near[ray], t_far = p.t_far[ray];
                if (!(fabsf(t_near) < INFINITY && fabsf(t_far) < INFINITY && t_far > t_near)) {
                    if (lane < 3) normal[(size_t)ray * 3 + lane] = 0.f;
                    continue;
                }
            }
        } else {
            int pi, pj;
            ray_of(__builtin_amdgcn_readfirstlane((int)rp), a.res, b, pi, pj);
            ray = __builtin_amdgcn_readfirstlane(b * R + pi * a.res + pj);
            ray_setup(a, b, pi, pj, o3, d3);
        }
        {
            const float* st = a.state + (size_t)ray * (S * HFAGP_RAYMARCH_STATE_FLOATS_PER_SAMPLE);
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int e = lane + 64 * k;
                if (e < S) {
                    ts[e] = st[S * 32 + e];
                    ss[e] = st[S * 33 + e];
                }
            }
        }
        WAVE_SYNC();
        // ---- the final compositing of the forward over the S-1 midpoints (two per lane) -> omega by sorted position
        {
            float al[2], sh[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int e = lane + 64 * k;
                al[k] = 0.f; sh[k] = 1.f;
                if (e < S - 1) {
                    const float t0 = ts[e], t1 = ts[e + 1];
                    const float dm = softplus_f((ss[e] + ss[e + 1]) * 0.5f - 1.f);
                    al[k] = 1.f - exp_f(-(dm * (t1 - t0)));
                    sh[k] = 1.f - al[k] + 1e-10f;
                }
            }
            const float i0 = wave_scan_mul(sh[0], lane);
            const float tot0 = __shfl(i0, 63);
            float T0 = __shfl_up(i0, 1);
            if (lane == 0) T0 = 1.f;
            const float i1 = wave_scan_mul(sh[1], lane);
            float T1 = __shfl_up(i1, 1);
            if (lane == 0) T1 = 1.f;
            T1 *= tot0;
            const float w0 = al[0] * T0, w1 = al[1] * T1;   // zero beyond S-2
            float p0 = __shfl_up(w0, 1);
            if (lane == 0) p0 = 0.f;
            float p1 = __shfl_up(w1, 1);
            const float w0_63 = __shfl(w0, 63);
            if (lane == 0) p1 = w0_63;
            if (lane < S) om[lane] = 0.5f * (p0 + w0);
            if (lane + 64 < S) om[lane + 64] = 0.5f * (p1 + w1);
        }
        WAVE_SYNC();
        float acc[3] = {0.f, 0.f, 0.f};            // sum of omega n over this lane's samples (lanes g == 0)
#pragma unroll 1
        for (int tt = 0; tt < NT; ++tt) {
            const int s = 16 * tt + j;
            int ln = lane;
            asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
            const float tz = ts[s], om_s = om[s];
            float f[8];
            gather8_mfma(p, b, o3, d3, ts[16 * tt + (lane >> 2)], lane, f);
            // decoder forward: only the hidden pre-activations are used (sigma and the colour logits fall away)
            f32x4 hp[4], h[4], o[2];
            float sigma;
            if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            // decoder adjoint of d sigma = 1, no colour gradient: dH = wsig * softplus'(hp), dF = W0^T dH
            f32x4 dH[4];
            f32x4 dF2[2];
            if constexpr (DEC16) decoder_bwd16_lds<false>(wfwd, nullptr, w0t, ln, o, 1.f, hp, dH, dF2);
            else decoder_bwd_lds<false>(wfwd, nullptr, w0t, ln, o, 1.f, hp, dH, dF2);
            // ---- positional derivative of the gather (as raymarch_bwd_camera_kernel): this lane's share of d sigma / dq
            float q[3], dq[3];
            sample_point(p, o3, d3, tz, q);
            gather_position_grad(a, b, g, q, dF2, sx, sy, dq);
            // the sample's four channel groups -> g = d sigma / d x in world units (q = coord_scale * x), on all four lanes
            float gw[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = dq[k];
                v += __shfl_xor(v, 16);
                v += __shfl_xor(v, 32);
                gw[k] = v * p.coord_scale;
            }
            const float gg2 = fmaf(gw[2], gw[2], fmaf(gw[1], gw[1], gw[0] * gw[0]));
            const float wn = g == 0 ? -om_s * __builtin_amdgcn_rsqf(gg2 + 1e-12f) : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) acc[k] = fmaf(wn, gw[k], acc[k]);
        }
        float out[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = wave_sum(acc[k]);
        if (lane == 0) {
            float* dst = normal + (size_t)ray * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[k] = out[k];
        }
        WAVE_SYNC();       // the next ray overwrites ts / ss / om
    }
}

template <int S, bool LIST>
static void launch_normals(const RayParams& p, float* normal, hipStream_t s) {
    const unsigned blocks = (unsigned)std::min<long long>(((long long)p.total_rays + kNrmWaves - 1) / kNrmWaves, (long long)kNumCU * 6);
    if (p.a.planes_absmax) raymarch_normals_kernel<S, true, LIST><<<blocks, kNrmWaves * 64, 0, s>>>(p, normal);
    else raymarch_normals_kernel<S, false, LIST><<<blocks, kNrmWaves * 64, 0, s>>>(p, normal);
}

}  // namespace hfagp

using namespace hfagp;

#ifndef HFAGP_RAY_LIST_UNIT        // (raymarch_rays_normals.hip compiles this source again for the list entry point alone)
extern "C" int hfagp_raymarch_normals(const HfagpRaymarchArgs* fwd, float* normal, void* stream) {
    HFAGP_REQUIRE(fwd && normal && fwd->state && fwd->planes, HFAGP_EBADARG, "raymarch_normals: null pointer");
    RayParams p;
    const int rc = fill_ray_params(fwd, p, "raymarch_normals");
    if (rc != HFAGP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int S = fwd->Sc + fwd->Sf;
    if (S == 96) launch_normals<96, false>(p, normal, s);
    else if (S == 64) launch_normals<64, false>(p, normal, s);
    else launch_normals<32, false>(p, normal, s);
    return check_launch("raymarch_normals");
}

#else
extern "C" int hfagp_raymarch_rays_normals(const HfagpRayListArgs* a, const HfagpRayLimits* lim, float* normal, void* stream) {
    HFAGP_REQUIRE(a && normal && a->base.state, HFAGP_EBADARG, "raymarch_rays_normals: null pointer");
    HFAGP_REQUIRE(!lim || (lim->t_near && lim->t_far), HFAGP_EBADARG, "raymarch_rays_normals: null pointer (limits)");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->base, p, "raymarch_rays_normals", &rays, lim != nullptr);
    if (rc != HFAGP_OK) return rc;
    if (lim) { p.t_near = lim->t_near; p.t_far = lim->t_far; }
    hipStream_t s = (hipStream_t)stream;
    const int S = a->base.Sc + a->base.Sf;
    if (S == 96) launch_normals<96, true>(p, normal, s);
    else if (S == 64) launch_normals<64, true>(p, normal, s);
    else launch_normals<32, true>(p, normal, s);
    return check_launch("raymarch_rays_normals");
}
#endif
