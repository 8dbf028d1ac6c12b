// Camera gradient of the ray marcher: dL/d(cam2world, intrinsics) from the per-sample records pass 1 of the backward leaves
// in `rec` (depth, omega, d sigma per sample: raymarch.hip) and the upstream feature gradient.
//
//   raymarch_bwd_camera_kernel   per 16-sample tile: gather -> decoder forward -> decoder adjoint = dL/dF (the arithmetic of
//                                raymarch_bwd_df_kernel, same shared device functions), then the POSITIONAL derivative of the
//                                bilinear gather,  dL/dp = (2 / box_warp) sum_planes (dL/dix, dL/diy) routed to the two
//                                coordinates the plane projects, summed along the ray:  dL/do = sum_s dL/dp_s,
//                                dL/dd = sum_s t_s dL/dp_s  ->  ray_grad[ray][6].  One writer per ray, plain stores.
//   camera_reduce_kernel         adjoint of ray_setup (raymarch_common.h) summed over a frame's rays in a fixed order
//                                -> d_cam2world[b][16], d_intrinsics[b][9].
// The sample depths carry no gradient (stratified: uniforms and constants; importance: detached as in EG3D), so the camera
// reaches the loss through the sample POSITIONS alone.  A pass of its own, not a flag on the dL/dF producers: it is the same
// whichever pass-2 form ran, and the producers' instantiations stay what they are.
#include "decoder_adjoint.h"

namespace hfagp {

constexpr int kCamWaves = 4;
constexpr int kCamReduceThreads = 256;

// (the decoder adjoint and the positional derivative of the gather: decoder_adjoint.h, shared with raymarch_bwd.hip,
// planes_query_bwd.hip and raymarch_normals.hip)

// LIST: the rays of a caller's list (raymarch_common.h ray_fetch) and the record split into d_origins / d_directions [B][R][3] —
// for a list the per-ray record IS the answer; the body is shared by the two kernels below.
template <int S, bool DEC16, bool LIST>
__device__ __forceinline__ void ray_grad_body(const RayParams& p, float* __restrict__ ray_grad, float* __restrict__ d_dir) {
    __shared__ float w1t[4 * 8 * 64];
    __shared__ float w0t[2 * 16 * 64];
    __shared__ float wfwd[kDecLdsRows * 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    const int R = LIST ? p.R : a.res * a.res;
    constexpr int NT = S / 16;
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    if constexpr (DEC16) build_grad16_lds(a, w1t, w0t, lane, wave, kCamWaves);
    else build_grad_lds(a, w1t, w0t, threadIdx.x, kCamWaves * 64);
    __syncthreads();
    // d pixel / d grid coordinate (plane_pixel) times the mean over the planes
    const float sx = (float)a.W * 0.5f * 0.3333333333333333f, sy = (float)a.H * 0.5f * 0.3333333333333333f;
    const RaySchedule sch = ray_schedule((long long)p.total_rays, wave, kCamWaves);
    for (long long rp = sch.begin; rp < sch.end; rp += sch.stride) {
        int b, ray_v;
        float o3[3], d3[3];
        ray_fetch<LIST>(p, __builtin_amdgcn_readfirstlane((int)rp), R, b, ray_v, o3, d3);
        const int ray = __builtin_amdgcn_readfirstlane(ray_v);
        float4 gfeat[2];
#pragma unroll
        for (int ot = 0; ot < 2; ++ot) gfeat[ot] = load_g_feat4(p, (size_t)ray * 32 + 16 * ot + 4 * g);
        // this lane's share (its 8 channels of its samples) of dL/dq summed along the ray, plain and depth-weighted
        float acc_o[3] = {0.f, 0.f, 0.f}, acc_d[3] = {0.f, 0.f, 0.f};
        float zq = p.rec[((size_t)ray * S + (lane >> 2)) * 4];
#pragma unroll 1
        for (int tt = 0; tt < NT; ++tt) {
            const int s = 16 * tt + j;
            int ln = lane;
            asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
            const float zq_cur = zq;
            zq = p.rec[((size_t)ray * S + 16 * min(tt + 1, NT - 1) + (lane >> 2)) * 4];
            const float4 rec = *reinterpret_cast<const float4*>(p.rec + ((size_t)ray * S + s) * 4);   // depth, omega, dsigma
            float f[8];
            gather8_mfma(p, b, o3, d3, zq_cur, lane, f);
            f32x4 hp[4], h[4], o[2];
            float sigma;
            if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            else decoder_fwd_lds<true>(wfwd, lane, f, hp, h, sigma, o);
            f32x4 dO[2];
            ray_colour_logit_grad(o, rec.y, gfeat, dO);
            f32x4 dH[4];
            f32x4 dF2[2];
            if constexpr (DEC16) decoder_bwd16_lds(wfwd, w1t, w0t, ln, dO, rec.z, hp, dH, dF2);
            else decoder_bwd_lds(wfwd, w1t, w0t, lane, dO, rec.z, hp, dH, dF2);
            // ---- positional derivative of the gather at the sample (depth rec.x): this lane's share
            float q[3], dq[3];
            sample_point(p, o3, d3, rec.x, q);
            gather_position_grad(a, b, g, q, dF2, sx, sy, dq);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                acc_o[k] += dq[k];
                acc_d[k] = fmaf(rec.x, dq[k], acc_d[k]);
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
            if constexpr (LIST) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { ray_grad[(size_t)ray * 3 + k] = out[k]; d_dir[(size_t)ray * 3 + k] = out[3 + k]; }
            } else {
                float* dst = ray_grad + (size_t)ray * 6;
#pragma unroll
                for (int k = 0; k < 6; ++k) dst[k] = out[k];
            }
        }
    }
}

template <int S, bool DEC16>
__global__ void __launch_bounds__(kCamWaves * 64, 2)
raymarch_bwd_camera_kernel(const RayParams p, float* __restrict__ ray_grad) {
    ray_grad_body<S, DEC16, false>(p, ray_grad, nullptr);
}

// hfagp_raymarch_rays_bwd_rays: one writer per ray, no atomics, no reduction
template <int S, bool DEC16>
__global__ void __launch_bounds__(kCamWaves * 64, 2)
raymarch_bwd_rays_kernel(const RayParams p, float* __restrict__ d_origins, float* __restrict__ d_directions) {
    ray_grad_body<S, DEC16, true>(p, d_origins, d_directions);
}

// One workgroup per frame.  Thread t walks rays t, t + 256, ...; 17 partial sums (12 of cam2world rows 0-2, fx, skew, cx, fy, cy),
// then a fixed-order tree over the threads: two calls give the same bits.
__global__ void __launch_bounds__(kCamReduceThreads)
camera_reduce_kernel(const HfagpRaymarchArgs a, const float* __restrict__ ray_grad, float* __restrict__ d_cam2world,
                     float* __restrict__ d_intrinsics) {
    __shared__ float red[17][kCamReduceThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int R = a.res * a.res;
    const float* M = a.cam2world + b * 16;
    const float* K = a.intrinsics + b * 9;
    const float fx = K[0], sk = K[1], cx = K[2], fy = K[4], cy = K[5];
    const float inv_res = 1.0f / (float)a.res, half_res = 0.5f / (float)a.res;
    float acc[17];
#pragma unroll
    for (int k = 0; k < 17; ++k) acc[k] = 0.f;
    for (int i = tid; i < R; i += kCamReduceThreads) {
        const int pi = i / a.res, pj = i % a.res;
        // ray_setup's arithmetic
        const float xc = __fadd_rn(__fmul_rn((float)pj, inv_res), half_res);
        const float yc = __fadd_rn(__fmul_rn((float)pi, inv_res), half_res);
        const float xl = __fdiv_rn(__fsub_rn(__fadd_rn(__fsub_rn(xc, cx), __fdiv_rn(__fmul_rn(cy, sk), fy)),
                                             __fdiv_rn(__fmul_rn(sk, yc), fy)), fx);
        const float yl = __fdiv_rn(__fsub_rn(yc, cy), fy);
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float wv = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(M[4 * k], xl), __fmul_rn(M[4 * k + 1], yl)),
                                                 M[4 * k + 2]), M[4 * k + 3]);
            v[k] = __fsub_rn(wv, M[4 * k + 3]);
        }
        const float nrm = fmaxf(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(v[0], v[0]), __fmul_rn(v[1], v[1])),
                                                     __fmul_rn(v[2], v[2]))), 1e-12f);
        const float d0 = __fdiv_rn(v[0], nrm), d1 = __fdiv_rn(v[1], nrm), d2 = __fdiv_rn(v[2], nrm);
        const float* rg = ray_grad + ((size_t)b * R + i) * 6;
        const float go[3] = {rg[0], rg[1], rg[2]};
        const float gd[3] = {rg[3], rg[4], rg[5]};
        // d = v / |v|:  gv = (g_d - d (d . g_d)) / |v|
        const float dot = d0 * gd[0] + d1 * gd[1] + d2 * gd[2];
        const float inv = 1.f / nrm;
        const float gv[3] = {(gd[0] - d0 * dot) * inv, (gd[1] - d1 * dot) * inv, (gd[2] - d2 * dot) * inv};
        float dxl = 0.f, dyl = 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            acc[4 * k] += gv[k] * xl;
            acc[4 * k + 1] += gv[k] * yl;
            acc[4 * k + 2] += gv[k];
            acc[4 * k + 3] += go[k];            // (column 3 enters v as w - o: its two contributions cancel)
            dxl = fmaf(gv[k], M[4 * k], dxl);
            dyl = fmaf(gv[k], M[4 * k + 1], dyl);
        }
        // xl = (xc - cx - sk yl) / fx,  yl = (yc - cy) / fy
        const float dn = dxl / fx;
        const float dyl_t = dyl - sk * dn;
        acc[12] -= dn * xl;                     // fx
        acc[13] -= dn * yl;                     // skew
        acc[14] -= dn;                          // cx
        acc[15] -= dyl_t * yl / fy;             // fy
        acc[16] -= dyl_t / fy;                  // cy
    }
#pragma unroll
    for (int k = 0; k < 17; ++k) red[k][tid] = acc[k];
    __syncthreads();
    for (int half = kCamReduceThreads / 2; half > 0; half >>= 1) {
        if (tid < half) {
#pragma unroll
            for (int k = 0; k < 17; ++k) red[k][tid] += red[k][tid + half];
        }
        __syncthreads();
    }
    if (tid < 16) d_cam2world[b * 16 + tid] = tid < 12 ? red[tid][0] : 0.f;
    if (tid < 9) {
        const int src = tid == 0 ? 12 : tid == 1 ? 13 : tid == 2 ? 14 : tid == 4 ? 15 : tid == 5 ? 16 : -1;
        d_intrinsics[b * 9 + tid] = src >= 0 ? red[src][0] : 0.f;
    }
}

template <int S>
static void launch_camera(const RayParams& p, float* ray_grad, hipStream_t s) {
    const long long ntiles = (long long)p.total_rays * (S / 16);
    const unsigned blocks = (unsigned)std::min<long long>((ntiles + kCamWaves - 1) / kCamWaves, (long long)kNumCU * 6);
    if (p.a.planes_absmax) raymarch_bwd_camera_kernel<S, true><<<blocks, kCamWaves * 64, 0, s>>>(p, ray_grad);
    else raymarch_bwd_camera_kernel<S, false><<<blocks, kCamWaves * 64, 0, s>>>(p, ray_grad);
}

template <int S>
static void launch_rays(const RayParams& p, float* d_origins, float* d_directions, hipStream_t s) {
    const long long ntiles = (long long)p.total_rays * (S / 16);
    const unsigned blocks = (unsigned)std::min<long long>((ntiles + kCamWaves - 1) / kCamWaves, (long long)kNumCU * 6);
    if (p.a.planes_absmax) raymarch_bwd_rays_kernel<S, true><<<blocks, kCamWaves * 64, 0, s>>>(p, d_origins, d_directions);
    else raymarch_bwd_rays_kernel<S, false><<<blocks, kCamWaves * 64, 0, s>>>(p, d_origins, d_directions);
}

int launch_ray_list_grads(const RayParams& p, float* d_origins, float* d_directions, hipStream_t s) {
    const int S = p.a.Sc + p.a.Sf;
    if (S == 96) launch_rays<96>(p, d_origins, d_directions, s);
    else if (S == 64) launch_rays<64>(p, d_origins, d_directions, s);
    else launch_rays<32>(p, d_origins, d_directions, s);
    return check_launch("raymarch_rays_bwd_rays");
}

// (raymarch_common.h) the reduction alone, for the other producer of ray_grad records: raymarch_normals_camera.hip
void launch_camera_reduce(const HfagpRaymarchArgs& a, const float* ray_grad, float* d_cam2world, float* d_intrinsics, hipStream_t s) {
    camera_reduce_kernel<<<(unsigned)a.B, kCamReduceThreads, 0, s>>>(a, ray_grad, d_cam2world, d_intrinsics);
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_raymarch_bwd_camera(const HfagpRaymarchBwdArgs* a, float* ray_grad, float* d_cam2world, float* d_intrinsics,
                                         void* stream) {
    HFAGP_REQUIRE(a && a->rec && ray_grad, HFAGP_EBADARG, "raymarch_bwd_camera: null pointer");
    HFAGP_REQUIRE((d_cam2world != nullptr) == (d_intrinsics != nullptr), HFAGP_EBADARG,
                  "raymarch_bwd_camera: d_cam2world and d_intrinsics go together (both or neither)");
    RayParams p;
    int rc = fill_ray_params(&a->fwd, p, "raymarch_bwd_camera");
    if (rc != HFAGP_OK) return rc;
    p.g_feat = a->g_feat;
    p.rec = a->rec;
    hipStream_t s = (hipStream_t)stream;
    const int S = a->fwd.Sc + a->fwd.Sf;
    if (S == 96) launch_camera<96>(p, ray_grad, s);
    else if (S == 64) launch_camera<64>(p, ray_grad, s);
    else launch_camera<32>(p, ray_grad, s);
    if (d_cam2world)
        camera_reduce_kernel<<<(unsigned)a->fwd.B, kCamReduceThreads, 0, s>>>(p.a, ray_grad, d_cam2world, d_intrinsics);
    return check_launch("raymarch_bwd_camera");
}
