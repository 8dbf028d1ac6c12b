// Camera gradient of the per-ray surface normals (raymarch_normals.hip): from G^ = dL/dN (3 floats per ray) to the per-ray
// record ray_grad[ray][6] = (dL/d origin, dL/d direction) that camera_reduce_kernel (raymarch_camera.hip) turns into
// d_cam2world and d_intrinsics.  Notation of raymarch_normals_bwd.hip and of include/hfagp.h (hfagp_raymarch_normals_bwd_camera).
// The sample depths carry no gradient, so the camera reaches the normal term through the sample POSITIONS q alone, by three paths:
//   the compositing weights   d sigma_s (the normals as colours)  -> dF = a d sigma_s             -> dq through the tap weights
//   the decoder's curvature   u = second gather with w'_k, v = W0' u, e = wsig sg (1 - sg) v      -> dF += W0'^T e  -> the same
//   the tap weights of J      g = coord_scale J^T a: the mixed second derivative of the bilinear weights times <texel_k, a>
// The first two are gather_position_grad applied to the dF pass B of raymarch_normals_bwd_kernel forms; the third comes from the
// same texels: gather_position_cross_grad (decoder_adjoint.h) forms all three from one read of the twelve lines.
//
//   raymarch_normals_camera_kernel   one wave per ray, four waves per workgroup, ray_schedule; lane = 16 g + j as its siblings.
//     pass A, scan   as raymarch_normals_bwd_kernel (raymarch_normals_common.h: the same code).
//     pass B         per tile: gather (F) and the second gather (u) -> decoder forward as far as hp -> dH, a -> v, e,
//                    x = dH d sigma_s + e, dF = W0'^T x; NO plane scatter, no decoder-gradient sums.  Then this lane's share of
//                    dL/dq = gather_position_cross_grad(dF, a, gamma_q) (one read of the texels), summed along the ray plain and
//                    depth-weighted; wave_sum in the fixed butterfly order, lane 0 stores (or adds to what is there: accumulate).
//   One writer per ray, no atomics: two calls give the same bits.  A ray with G^ == 0 is skipped (its six floats are zeros when
//   not accumulating); a tile whose samples all have omega == 0 and d sigma == 0 is skipped.
//   The second-order products (v, W0'^T x) run on the exact fp32 MFMA with either decoder, as in the sibling.  So does a = W0'^T dH
//   here, in both passes (decoder_dh_lds + w0t_mul; no split-bf16 image of W0'^T is built): with the 16-bit decoder the sibling
//   takes a from the forward normals' split-bf16 product (2^-16 per product) so that n has the forward's bits; that error has one
//   sign over neighbouring rays and the reduction over a frame's rays does not average it out (measured on tiny64, 200 rays:
//   d_cam2world at 1.55 of the gradient bar with the bf16 a, against 0.29 for the fp32 decoder).  The forward products (hp) stay
//   on the split-fp16 pipe (2^-22).
#include "raymarch_normals_common.h"

namespace hfagp {

constexpr int kNcWaves = 4;

// LIST: the rays of a caller's list (raymarch_common.h ray_fetch; directions as given) and the record split into d_origins /
// d_directions [B][R][3] (`ray_grad` / `d_dir`: the layout of launch_ray_list_grads, whose output `accumulate` adds to) — for a list
// the per-ray record IS the answer.  With per-ray limits (RayParams::t_near / t_far) an EMPTY ray (raymarch.hip's predicate) reads
// nothing of its `state`, which the forward never wrote: six zeros when not accumulating, nothing when accumulating.  The body is
// shared by the two kernels below.
template <int S, bool DEC16, bool LIST>
__device__ __forceinline__ void normals_camera_body(const RayParams& p, const float* __restrict__ g_normal, float* __restrict__ ray_grad,
                                                    float* __restrict__ d_dir, const int accumulate) {
    __shared__ float w0t[2 * 16 * 64];                       // fp32 A operands of W0'^T (build_grad_lds)
    __shared__ float w0f[DEC16 ? 32 * 64 : 1];               // fp32 A operands of W0' (fp32 decoder: rows 0-31 of wfwd)
    __shared__ float wfwd[kDecLdsRows * 64];
    // by sorted position: depths, raw densities, omega, n, 1 / r
    __shared__ float ray_ts[kNcWaves][S], ray_ss[kNcWaves][S], ray_om[kNcWaves][S];     // (d sigma overwrites the densities)
    __shared__ float ray_n[kNcWaves][3][S], ray_ri[kNcWaves][S];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    const int R = LIST ? p.R : a.res * a.res;
    constexpr int NT = S / 16;
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    build_grad_lds<false>(a, nullptr, w0t, threadIdx.x, kNcWaves * 64);
    if constexpr (DEC16) {
        const float g0 = a.decoder_lr_mul * 0.17677669529663687f;
        for (int i = threadIdx.x; i < 32 * 64; i += kNcWaves * 64) {
            const int l = i & 63, row = i >> 6;              // row = mt * 8 + t
            w0f[i] = a.dec_w0[(16 * (row >> 3) + (l & 15)) * 32 + 8 * (l >> 4) + (row & 7)] * g0;
        }
    }
    __syncthreads();
    const float* w0fwd = DEC16 ? w0f : wfwd;
    float* ts = ray_ts[wave];
    float* ss = ray_ss[wave];
    float* om = ray_om[wave];
    float* dsg = ss;         // written by the second compositing scan after its last read of ss
    float* nx = ray_n[wave][0];
    float* ny = ray_n[wave][1];
    float* nz = ray_n[wave][2];
    float* ri = ray_ri[wave];
    // d pixel / d grid coordinate (plane_pixel); sx, sy: the same times the mean over the planes
    const float hx = (float)a.W * 0.5f, hy = (float)a.H * 0.5f;
    const float sx = hx * 0.3333333333333333f, sy = hy * 0.3333333333333333f;
    const float sxy = sx * hy;
    const RaySchedule sch = ray_schedule((long long)p.total_rays, wave, kNcWaves);
    for (long long rp = sch.begin; rp < sch.end; rp += sch.stride) {
        int b, pi, pj, ray;
        float o3[3], d3[3];
        bool empty = false;                                               // (LIST with limits; wave-uniform)
        if constexpr (LIST) {
            int ray_v;
            ray_fetch<true>(p, __builtin_amdgcn_readfirstlane((int)rp), R, b, ray_v, o3, d3);
            ray = __builtin_amdgcn_readfirstlane(ray_v);
            if (p.t_near) {                         // (wave-uniform: the limit-less list call never enters)
                const float t_near = p.t_near[ray], t_far = p.t_far[ray];
                empty = !(fabsf(t_near) < INFINITY && fabsf(t_far) < INFINITY && t_far > t_near);
            }
        } else {
            ray_of(__builtin_amdgcn_readfirstlane((int)rp), a.res, b, pi, pj);
            ray = __builtin_amdgcn_readfirstlane(b * R + pi * a.res + pj);
        }
        float* dst = LIST ? ray_grad + (size_t)ray * 3 : ray_grad + (size_t)ray * 6;
        float* dst_d = LIST ? d_dir + (size_t)ray * 3 : dst + 3;
        const float Gh[3] = {g_normal[(size_t)ray * 3], g_normal[(size_t)ray * 3 + 1], g_normal[(size_t)ray * 3 + 2]};
        if (empty || (Gh[0] == 0.f && Gh[1] == 0.f && Gh[2] == 0.f)) {    // (wave-uniform)
            if (!accumulate && lane == 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k] = 0.f;
#pragma unroll
                for (int k = 0; k < 3; ++k) dst_d[k] = 0.f;
            }
            continue;
        }
        if constexpr (!LIST) ray_setup(a, b, pi, pj, o3, d3);
        normals_load_ray<S>(a.state + (size_t)ray * (S * HFAGP_RAYMARCH_STATE_FLOATS_PER_SAMPLE), lane, ts, ss);
        WAVE_SYNC();
        {
            Composite c;
            composite<S>(ts, ss, lane, c);
            midpoints_to_samples<S>(c.w[0], c.w[1], lane, om);
        }
        WAVE_SYNC();
        normals_pass_a<S, DEC16>(p, b, o3, d3, lane, wfwd, w0t, sx, sy, ts, nx, ny, nz, ri);
        WAVE_SYNC();
        normals_weight_adjoint<S>(Gh, ts, ss, nx, ny, nz, lane, dsg);
        WAVE_SYNC();
        // ---- pass B: this lane's share (its 8 channels of its samples) of dL/dq summed along the ray, plain and depth-weighted
        float acc_o[3] = {0.f, 0.f, 0.f}, acc_d[3] = {0.f, 0.f, 0.f};
#pragma unroll 1
        for (int tt = 0; tt < NT; ++tt) {
            const int s = 16 * tt + j;
            const float om_s = om[s], ds_s = dsg[s];
            const bool live = om_s != 0.f || ds_s != 0.f;
            if (__builtin_amdgcn_ballot_w64(live) == 0) continue;
            int ln = lane;
            asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
            const float tz = ts[s];
            float q[3];
            sample_point(p, o3, d3, tz, q);
            float gq[3];
            {
                const float n3[3] = {nx[s], ny[s], nz[s]};
                normals_gamma_q(Gh, n3, om_s, ri[s], p.coord_scale, gq);
            }
            PlaneTaps taps[3], dtaps[3];
            normals_second_taps(a, q, gq, hx, hy, taps, dtaps);
            float f[8], u[8];
            gather8(a, b, g, taps, f);
            gather8(a, b, g, dtaps, u);
            f32x4 hp[4], h[4], o[2];
            float sigma;
            if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            f32x4 dH[4], av[2];                  // dH = wsig sigmoid(hp); av = a = W0'^T dH in fp32 (as pass A)
            decoder_dh_lds<DEC16>(wfwd, ln, hp, dH);
            w0t_mul(w0t, ln, dH, av);
            f32x4 v[4], x[4];
            w0_mul(w0fwd, ln, u, v);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sg = sigmoid_f(hp[mt][r]);
                    const float e = dH[mt][r] * (1.f - sg) * v[mt][r];
                    x[mt][r] = fmaf(dH[mt][r], ds_s, e);
                }
            f32x4 dF[2];
            w0t_mul(w0t, ln, x, dF);
            // a dead sample of a live tile: ds_s = 0 and gamma_q = 0, so u, e, x, dF and the cross term are 0
            float dq[3];
            gather_position_cross_grad(a, b, g, q, dF, av, gq, sx, sy, sxy, dq);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc_o[k] += dq[k];
                acc_d[k] = fmaf(tz, dq[k], acc_d[k]);
            }
        }
        // the ray's 64 lane shares (16 samples per tile x 4 channel groups) in a fixed butterfly order; q = coord_scale * p
        float out[6];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            out[k] = wave_sum(acc_o[k]) * p.coord_scale;
            out[3 + k] = wave_sum(acc_d[k]) * p.coord_scale;
        }
        if (lane == 0) {
            if (accumulate) {
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k] += out[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) dst_d[k] += out[3 + k];
            } else {
#pragma unroll
                for (int k = 0; k < 3; ++k) dst[k] = out[k];
#pragma unroll
                for (int k = 0; k < 3; ++k) dst_d[k] = out[3 + k];
            }
        }
        WAVE_SYNC();       // the next ray overwrites the per-ray tables
    }
}

template <int S, bool DEC16>
__global__ void __launch_bounds__(kNcWaves * 64, 2)
raymarch_normals_camera_kernel(const RayParams p, const float* __restrict__ g_normal, float* __restrict__ ray_grad,
                               const int accumulate) {
    normals_camera_body<S, DEC16, false>(p, g_normal, ray_grad, nullptr, accumulate);
}

// hfagp_raymarch_rays_normals_bwd_rays: one writer per ray, no atomics, no reduction
template <int S, bool DEC16>
__global__ void __launch_bounds__(kNcWaves * 64, 2)
raymarch_normals_camera_rays_kernel(const RayParams p, const float* __restrict__ g_normal, float* __restrict__ d_origins,
                                    float* __restrict__ d_directions, const int accumulate) {
    normals_camera_body<S, DEC16, true>(p, g_normal, d_origins, d_directions, accumulate);
}

// one round of resident workgroups, each wave walking its run of rays
template <typename Kernel>
static long long nc_blocks(const RayParams& p, Kernel kernel, int& resident) {
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, kNcWaves * 64, 0) != hipSuccess || n < 1) n = 1;
        resident = n;
    }
    return std::min<long long>(((long long)p.total_rays + kNcWaves - 1) / kNcWaves, (long long)kNumCU * resident);
}

template <int S, bool DEC16>
static int launch_nc(const RayParams& p, const float* g_normal, float* ray_grad, int accumulate, hipStream_t s) {
    static int resident = 0;
    const long long blocks = nc_blocks(p, raymarch_normals_camera_kernel<S, DEC16>, resident);
    raymarch_normals_camera_kernel<S, DEC16><<<(unsigned)blocks, kNcWaves * 64, 0, s>>>(p, g_normal, ray_grad, accumulate);
    return check_launch("raymarch_normals_bwd_camera");
}

template <int S, bool DEC16>
static int launch_nc_rays(const RayParams& p, const float* g_normal, float* d_origins, float* d_directions, int accumulate,
                          hipStream_t s) {
    static int resident = 0;
    const long long blocks = nc_blocks(p, raymarch_normals_camera_rays_kernel<S, DEC16>, resident);
    raymarch_normals_camera_rays_kernel<S, DEC16><<<(unsigned)blocks, kNcWaves * 64, 0, s>>>(p, g_normal, d_origins, d_directions,
                                                                                            accumulate);
    return check_launch("raymarch_rays_normals_bwd_rays");
}

template <int S>
static int launch_nc_s(const RayParams& p, const float* g_normal, float* ray_grad, int accumulate, hipStream_t s) {
    if (p.a.planes_absmax) return launch_nc<S, true>(p, g_normal, ray_grad, accumulate, s);
    return launch_nc<S, false>(p, g_normal, ray_grad, accumulate, s);
}

template <int S>
static int launch_nc_rays_s(const RayParams& p, const float* g_normal, float* d_origins, float* d_directions, int accumulate,
                            hipStream_t s) {
    if (p.a.planes_absmax) return launch_nc_rays<S, true>(p, g_normal, d_origins, d_directions, accumulate, s);
    return launch_nc_rays<S, false>(p, g_normal, d_origins, d_directions, accumulate, s);
}

}  // namespace hfagp

using namespace hfagp;

#ifndef HFAGP_RAY_LIST_UNIT        // (raymarch_rays_normals.hip compiles this source again for the list entry point alone)
extern "C" int hfagp_raymarch_normals_bwd_camera(const HfagpRaymarchArgs* fwd, const float* g_normal, float* ray_grad, int accumulate,
                                                 float* d_cam2world, float* d_intrinsics, void* stream) {
    HFAGP_REQUIRE(fwd && g_normal && ray_grad && fwd->state && fwd->planes, HFAGP_EBADARG, "raymarch_normals_bwd_camera: null pointer");
    HFAGP_REQUIRE((d_cam2world != nullptr) == (d_intrinsics != nullptr), HFAGP_EBADARG,
                  "raymarch_normals_bwd_camera: d_cam2world and d_intrinsics go together (both or neither)");
    RayParams p;
    int rc = fill_ray_params(fwd, p, "raymarch_normals_bwd_camera");
    if (rc != HFAGP_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int S = fwd->Sc + fwd->Sf;
    const int acc = accumulate != 0;
    if (S == 96) rc = launch_nc_s<96>(p, g_normal, ray_grad, acc, s);
    else if (S == 64) rc = launch_nc_s<64>(p, g_normal, ray_grad, acc, s);
    else rc = launch_nc_s<32>(p, g_normal, ray_grad, acc, s);
    if (rc != HFAGP_OK || !d_cam2world) return rc;
    launch_camera_reduce(p.a, ray_grad, d_cam2world, d_intrinsics, s);
    return check_launch("raymarch_normals_bwd_camera");
}

#else
extern "C" int hfagp_raymarch_rays_normals_bwd_rays(const HfagpRayListArgs* a, const HfagpRayLimits* lim, const float* g_normal,
                                                    float* d_origins, float* d_directions, int accumulate, void* stream) {
    HFAGP_REQUIRE(a && g_normal && d_origins && d_directions && a->base.state, HFAGP_EBADARG,
                  "raymarch_rays_normals_bwd_rays: null pointer");
    HFAGP_REQUIRE(!lim || (lim->t_near && lim->t_far), HFAGP_EBADARG, "raymarch_rays_normals_bwd_rays: null pointer (limits)");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->base, p, "raymarch_rays_normals_bwd_rays", &rays, lim != nullptr);
    if (rc != HFAGP_OK) return rc;
    if (lim) { p.t_near = lim->t_near; p.t_far = lim->t_far; }
    hipStream_t s = (hipStream_t)stream;
    const int S = a->base.Sc + a->base.Sf;
    const int acc = accumulate != 0;
    if (S == 96) return launch_nc_rays_s<96>(p, g_normal, d_origins, d_directions, acc, s);
    if (S == 64) return launch_nc_rays_s<64>(p, g_normal, d_origins, d_directions, acc, s);
    return launch_nc_rays_s<32>(p, g_normal, d_origins, d_directions, acc, s);
}
#endif
