// What the two backward kernels of the per-ray surface normals share (raymarch_normals_bwd.hip: d planes and the decoder
// gradients; raymarch_normals_camera.hip: the camera gradient), once.  Notation of raymarch_normals_bwd.hip.
//   Composite / composite / midpoints_to_samples    the forward's compositing over the S-1 midpoints (the same bits)
//   normals_load_ray        sorted depths and raw densities of a ray from the forward's state
//   normals_pass_a          pass A: n_s and 1 / r_s of every sample (a in fp32 with either decoder)
//   point_density_grad      g and 1 / r of one point per lane from a (the point queries: planes_query_normals[_bwd].hip)
//   normals_weight_adjoint  the compositing adjoint with the normals as colours: d sigma_s by sorted position
//   normals_gamma_q         gamma_q = coord_scale dL/dg of a sample
//   normals_second_taps     the bilinear taps w_k and their derivative weights w'_k, all three planes
// raymarch_normals_bwd.hip takes the compositing from here (its instantiations keep their instructions) and keeps its own inline
// copy of the rest: moving those lines into functions changed its register allocation and schedule, and its results are pinned.
// Each of those blocks there carries a comment naming its twin here: a change to one belongs in the other.
#pragma once
#include "decoder_adjoint.h"

namespace hfagp {

// the forward's compositing over the S-1 midpoints (raymarch_normals_kernel's lines: the same bits), two midpoints per lane
struct Composite {
    float al[2], sh[2], dl[2], sbar[2], T[2], w[2];
};
template <int S>
__device__ __forceinline__ void composite(const float* ts, const float* ss, int lane, Composite& c) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = lane + 64 * k;
        c.al[k] = 0.f; c.sh[k] = 1.f; c.dl[k] = 0.f; c.sbar[k] = 0.f;
        if (e < S - 1) {
            const float t0 = ts[e], t1 = ts[e + 1];
            c.sbar[k] = (ss[e] + ss[e + 1]) * 0.5f - 1.f;
            const float dm = softplus_f(c.sbar[k]);
            c.dl[k] = t1 - t0;
            c.al[k] = 1.f - exp_f(-(dm * c.dl[k]));
            c.sh[k] = 1.f - c.al[k] + 1e-10f;
        }
    }
    const float i0 = wave_scan_mul(c.sh[0], lane);
    const float tot0 = __shfl(i0, 63);
    float T0 = __shfl_up(i0, 1);
    if (lane == 0) T0 = 1.f;
    const float i1 = wave_scan_mul(c.sh[1], lane);
    float T1 = __shfl_up(i1, 1);
    if (lane == 0) T1 = 1.f;
    T1 *= tot0;
    c.T[0] = T0; c.T[1] = T1;
    c.w[0] = c.al[0] * T0; c.w[1] = c.al[1] * T1;       // zero beyond S-2
}
// v by sorted position = (v_{e-1} + v_e) / 2 of the per-midpoint values (two per lane), into dst[S]
template <int S>
__device__ __forceinline__ void midpoints_to_samples(float v0, float v1, int lane, float* dst) {
    float p0 = __shfl_up(v0, 1);
    if (lane == 0) p0 = 0.f;
    float p1 = __shfl_up(v1, 1);
    const float v0_63 = __shfl(v0, 63);
    if (lane == 0) p1 = v0_63;
    if (lane < S) dst[lane] = 0.5f * (p0 + v0);
    if (lane + 64 < S) dst[lane + 64] = 0.5f * (p1 + v1);
}

// the ray's sorted depths and raw densities from the forward's state (st: the ray's S * 35 floats), into ts[S], ss[S]
template <int S>
__device__ __forceinline__ void normals_load_ray(const float* st, int lane, float* ts, float* ss) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = lane + 64 * k;
        if (e < S) {
            ts[e] = st[S * 32 + e];
            ss[e] = st[S * 33 + e];
        }
    }
}

// ---- pass A: n_s and 1 / r_s of every sample into nx, ny, nz, ri [S] by sorted position.  wfwd: decoder_images_lds; w0t:
// build_grad_lds.  sx, sy: gather_position_grad's.  a = W0'^T dH runs on the exact fp32 matrix instructions with either decoder:
// with the fp32 decoder these are raymarch_normals_kernel's instructions (its n), with the 16-bit decoder that kernel and
// raymarch_normals_bwd_kernel take a from the split-bf16 product (2^-16 per product), which a consumer that sums over a frame's
// rays cannot afford (raymarch_normals_camera.hip), so n is the forward's to ~2^-16 there, not to the bit.
template <int S, bool DEC16>
__device__ __forceinline__ void normals_pass_a(const RayParams& p, int b, const float o3[3], const float d3[3], int lane,
                                               const float* wfwd, const float* w0t, float sx, float sy,
                                               const float* ts, float* nx, float* ny, float* nz, float* ri) {
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
#pragma unroll 1
    for (int tt = 0; tt < S / 16; ++tt) {
        const int s = 16 * tt + j;
        int ln = lane;
        asm volatile("" : "+v"(ln));       // the weight images are read per tile, not hoisted into registers
        const float tz = ts[s];
        float f[8];
        gather8_mfma(p, b, o3, d3, ts[16 * tt + (lane >> 2)], lane, f);
        f32x4 hp[4], h[4], o[2];
        float sigma;
        if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
        else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);
        f32x4 dH[4];
        f32x4 dF2[2];
        decoder_dh_lds<DEC16>(wfwd, ln, hp, dH);
        w0t_mul(w0t, ln, dH, dF2);
        float q[3], dq[3];
        sample_point(p, o3, d3, tz, q);
        gather_position_grad(a, b, g, q, dF2, sx, sy, dq);
        float gw[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float v = dq[k];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            gw[k] = v * p.coord_scale;
        }
        const float gg2 = fmaf(gw[2], gw[2], fmaf(gw[1], gw[1], gw[0] * gw[0]));
        const float rs = __builtin_amdgcn_rsqf(gg2 + 1e-12f);
        if (g == 0) {
            nx[s] = -rs * gw[0];
            ny[s] = -rs * gw[1];
            nz[s] = -rs * gw[2];
            ri[s] = rs;
        }
    }
}

// ---- a point as a ray sample (planes_query_normals.hip and its backward): pass A's lines from a to g and 1 / r for ONE point
// per lane at the normalised position q.  av = a = W0'^T (wsig * sigmoid(hp)) of this lane's channels (w0t_mul); gw = g =
// coord_scale J^T a in world units on all four lanes of the point; returns 1 / r = rsqrt(g.g + 1e-12), so n = -(1 / r) g.
__device__ __forceinline__ float point_density_grad(const HfagpRaymarchArgs& a, int b, int g, const float q[3], const f32x4 av[2],
                                                    float sx, float sy, float coord_scale, float gw[3]) {
    float dq[3];
    gather_position_grad(a, b, g, q, av, sx, sy, dq);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = dq[k];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        gw[k] = v * coord_scale;
    }
    const float gg2 = fmaf(gw[2], gw[2], fmaf(gw[1], gw[1], gw[0] * gw[0]));
    return __builtin_amdgcn_rsqf(gg2 + 1e-12f);
}

// ---- the compositing adjoint (raymarch.hip) with the normals as colours: G_e = G^ . (n_e + n_{e+1}) / 2 -> d sigma_s by sorted
// position into dsg[S].  dsg may be ss: it is written after the last read of ss (every lane's stores depend on its loads).
template <int S>
__device__ __forceinline__ void normals_weight_adjoint(const float Gh[3], const float* ts, const float* ss, const float* nx,
                                                       const float* ny, const float* nz, int lane, float* dsg) {
    Composite c;
    composite<S>(ts, ss, lane, c);
    float G[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = lane + 64 * k;
        G[k] = 0.f;
        if (e < S - 1) {
            const float gn0 = fmaf(Gh[2], nz[e], fmaf(Gh[1], ny[e], Gh[0] * nx[e]));
            const float gn1 = fmaf(Gh[2], nz[e + 1], fmaf(Gh[1], ny[e + 1], Gh[0] * nx[e + 1]));
            G[k] = 0.5f * (gn0 + gn1);
        }
    }
    const float gw0 = G[0] * c.w[0], gw1 = G[1] * c.w[1];
    const float inc0 = wave_scan_add(gw0, lane), inc1 = wave_scan_add(gw1, lane);
    const float tot_a = __shfl(inc0, 63), tot = tot_a + __shfl(inc1, 63);
    const float suf0 = tot - inc0, suf1 = tot - (tot_a + inc1);
    const float da0 = G[0] * c.T[0] - suf0 / c.sh[0], da1 = G[1] * c.T[1] - suf1 / c.sh[1];
    float ds0 = da0 * c.dl[0] * (1.f - c.al[0]) * sigmoid_f(c.sbar[0]);
    float ds1 = da1 * c.dl[1] * (1.f - c.al[1]) * sigmoid_f(c.sbar[1]);
    if (lane >= S - 1) ds0 = 0.f;
    if (lane + 64 >= S - 1) ds1 = 0.f;
    midpoints_to_samples<S>(ds0, ds1, lane, dsg);
}

// gamma_q = coord_scale dL/dg = -coord_scale (omega / r) (G^ - n (n . G^)) of one sample (n3 its normal, rinv = 1 / r)
__device__ __forceinline__ void normals_gamma_q(const float Gh[3], const float n3[3], float om_s, float rinv, float coord_scale,
                                                float gq[3]) {
    const float ndg = fmaf(Gh[2], n3[2], fmaf(Gh[1], n3[1], Gh[0] * n3[0]));
    const float cf = -(om_s * rinv) * coord_scale;
#pragma unroll
    for (int k = 0; k < 3; ++k) gq[k] = cf * (Gh[k] - n3[k] * ndg);
}

// the bilinear taps (w_k) and their derivative weights (w'_k = gamma_q . grad_q w_k), all three planes on every lane.
// hx, hy: d pixel / d grid coordinate (plane_pixel) = W / 2, H / 2.
__device__ __forceinline__ void normals_second_taps(const HfagpRaymarchArgs& a, const float q[3], const float gq[3], float hx,
                                                    float hy, PlaneTaps taps[3], PlaneTaps dtaps[3]) {
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
        float gx, gy;
        plane_coords(a, q, pl, gx, gy);
        plane_taps(a, gx, gy, taps[pl]);
        PlaneTapsD td;
        plane_taps_d(a, gx, gy, td);
        // the components of gamma_q the plane's two coordinates carry (plane_coords), in pixel units
        const float cx = (pl == 2 ? gq[2] : gq[0]) * hx;
        const float cy = (pl == 0 ? gq[1] : pl == 1 ? gq[2] : (a.plane_axes == 0 ? gq[0] : gq[1])) * hy;
        const float ofx = 1.f - td.fx, ofy = 1.f - td.fy;
        const float dw[4] = {-(ofy * cx) - ofx * cy, ofy * cx - td.fx * cy, ofx * cy - td.fy * cx, td.fy * cx + td.fx * cy};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dtaps[pl].idx[k] = td.idx[k];
            dtaps[pl].w[k] = td.ok[k] ? dw[k] : 0.f;
        }
    }
}

}  // namespace hfagp
