// Backward of the per-ray surface normals (raymarch_normals.hip): from G^ = dL/dN (3 floats per ray) to dL/dplanes and the
// decoder-parameter gradients.  Notation of raymarch_normals.hip and of include/hfagp.h (hfagp_raymarch_normals_bwd):
//   F = gathered features, hp = W0' F + b0', sigma = wsig . softplus(hp) + bsig, a = d sigma / dF = W0'^T (wsig * sigmoid(hp)),
//   g = coord_scale J^T a (J = dF / dq), r = sqrt(g.g + 1e-12), n = -g / r, N = sum_s omega_s n_s.
// The gradient has two parts:
//   through the weights   the normals are three "colours" of the compositing: G_e = G^ . (n_e + n_{e+1}) / 2 -> the compositing
//                         adjoint of raymarch.hip -> d sigma_s, then the first-order decoder / gather adjoint  dF = a d sigma_s;
//   through the normals   gamma = dL/dg = -(omega / r) (G^ - n (n . G^)); g is linear in the texels (through J) and in a, so with
//                         w'_k = coord_scale gamma . grad_q w_k  (the derivative weight of tap k)
//                           u = sum_taps texel w'_k / 3     (a second gather of the same twelve lines),    v = W0' u,
//                           e = wsig * sigmoid(hp) (1 - sigmoid(hp)) * v,                                   dF += W0'^T e,
//                         and the texels receive  (w'_k / 3) a  next to  (w_k / 3) dF.
//
//   raymarch_normals_bwd_kernel   one wave per ray, four waves per workgroup, ray_schedule; lane = 16 g + j (sample j of a
//                                 16-sample tile, channel group g) as raymarch_normals_kernel.
//     pass A   the forward's scan (the same omega bits) and, per tile, the forward's n_s (the same instruction sequence: the same
//              bits); n_s and 1 / r_s stay in LDS (4 floats per sample).
//     scan     G_e from G^ . n, the compositing adjoint -> d sigma_s by sorted position, in LDS.
//     pass B   per tile: gather (F) and the second gather (u) -> decoder forward as far as hp -> dH = wsig sigmoid(hp), a -> v, e,
//              x = dH d sigma_s + e, dF = W0'^T x -> one run-merged line scatter with two value / weight sets, (dF, w_k / 3)
//              and (a, w'_k / 3) (scatter_tile_runs2<6>: all three planes at their true texels).  PG: dW0' += x F^T + dH u^T, db0' += x,
//              dwsig += d sigma_s softplus(hp) + sigmoid(hp) v, dbsig += d sigma_s, summed per wave, one flush at the end.
//   The new products (v, W0'^T x, the weight-gradient products) run on the exact fp32 MFMA with either decoder: u is not bounded
//   by planes_absmax, so the forward's fp16 operand scaling does not carry over.  a comes from the decoder adjoint the forward
//   normals use (split bf16 with the 16-bit decoder): n has the forward's bits.
//   A ray with G^ == 0 is skipped; a tile whose samples all have omega == 0 and d sigma == 0 is skipped; a sample like that in
//   a live tile publishes weight 0.  The sample depths carry no gradient.
#include "raymarch_normals_common.h"

namespace hfagp {

constexpr int kNbWaves = 4;

// (Composite, composite, midpoints_to_samples: raymarch_normals_common.h, shared with raymarch_normals_camera.hip.  The blocks
// below marked `twin:` have a copy there as functions, used by that unit: calling them from here changed this unit's register
// allocation and instruction order, so the lines stay inline; keep the two in step.)

// LIST: the rays of a caller's list (raymarch_common.h ray_fetch; directions as given) instead of the pinhole grid.  With per-ray
// limits (RayParams::t_near / t_far) an EMPTY ray (raymarch.hip's predicate) is skipped before anything of it is read: its `state`
// was never written.  (The ray fetch is a template parameter of the kernel, not a shared body function: see the note above on this
// unit's register allocation — DESIGN.md has the table.)
// With the 16-bit decoder the list form takes a = W0'^T dH from the exact fp32 MFMA in both passes (decoder_dh_lds + w0t_mul, the
// choice of raymarch_normals_camera.hip and of normals_pass_a; no split-bf16 image of W0'^T is built), where the grid form takes it
// from the forward normals' split-bf16 product (2^-16 per product): on the 2 x 101 list of non-unit directions that product put
// d_planes at 1.09 of the gradient bar (small128; 0.044 with the fp32 decoder), beyond what the fp32 reference's own error allows.
// n is then the forward's to ~2^-16, not to the bit.  The grid form keeps its arithmetic.
template <int S, bool DEC16, bool PG, bool LIST = false>
__global__ void __launch_bounds__(kNbWaves * 64, PG ? 1 : 2)
raymarch_normals_bwd_kernel(const RayParams p, const float* __restrict__ g_normal, float* __restrict__ d_planes, const DecGrads dg) {
    __shared__ Tile2Lds lds_all[kNbWaves];
    __shared__ __attribute__((aligned(16))) float glds_raw[PG ? kNbWaves * sizeof(NrmGradLds) / sizeof(float) : 1];
    __shared__ float w0t[2 * 16 * 64];                       // fp32 A operands of W0'^T (build_grad_lds)
    constexpr bool A16 = DEC16 && !LIST;                     // a from the split-bf16 product (the grid form with the 16-bit decoder)
    __shared__ float g0img[A16 ? 2 * 16 * 64 : 1];           // split-bf16 A operands of W0'^T: the forward normals' adjoint
    __shared__ float w0f[DEC16 ? 32 * 64 : 1];               // fp32 A operands of W0' (fp32 decoder: rows 0-31 of wfwd)
    __shared__ float wfwd[kDecLdsRows * 64];
    // by sorted position: depths, raw densities, omega, n, 1 / r
    __shared__ float ray_ts[kNbWaves][S], ray_ss[kNbWaves][S], ray_om[kNbWaves][S];     // (d sigma overwrites the densities)
    __shared__ float ray_n[kNbWaves][3][S], ray_ri[kNbWaves][S];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const HfagpRaymarchArgs& a = p.a;
    const int j = lane & 15, g = lane >> 4;
    const int R = LIST ? p.R : a.res * a.res;
    constexpr int NT = S / 16;
    if (wave == 0) decoder_images_lds<DEC16>(a, wfwd, lane, j, g);
    build_grad_lds<false>(a, nullptr, w0t, threadIdx.x, kNbWaves * 64);
    if constexpr (DEC16) {
        if constexpr (A16) build_grad16_lds<false>(a, nullptr, g0img, lane, wave, kNbWaves);
        const float g0 = a.decoder_lr_mul * 0.17677669529663687f;
        for (int i = threadIdx.x; i < 32 * 64; i += kNbWaves * 64) {
            const int l = i & 63, row = i >> 6;              // row = mt * 8 + t
            w0f[i] = a.dec_w0[(16 * (row >> 3) + (l & 15)) * 32 + 8 * (l >> 4) + (row & 7)] * g0;
        }
    }
    __syncthreads();
    const float* w0fwd = DEC16 ? w0f : wfwd;
    float* ts = ray_ts[wave];
    float* ss = ray_ss[wave];
    float* om = ray_om[wave];
    float* dsg = ss;         // written by the second compositing scan after its last read of ss (every lane's stores depend on its loads)
    float* nx = ray_n[wave][0];
    float* ny = ray_n[wave][1];
    float* nz = ray_n[wave][2];
    float* ri = ray_ri[wave];
    Tile2Lds& lds = lds_all[wave];
    NrmGradLds& gl = reinterpret_cast<NrmGradLds*>(glds_raw)[PG ? wave : 0];      // never dereferenced unless PG
    NrmGradAcc acc;
    bool any = false;                               // this wave has a ray with a gradient (wave-uniform)
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
    const RaySchedule sch = ray_schedule((long long)p.total_rays, wave, kNbWaves);
    for (long long rp = sch.begin; rp < sch.end; rp += sch.stride) {
        int b, pi, pj, ray;
        float o3[3], d3[3];
        if constexpr (LIST) {
            int ray_v;
            ray_fetch<true>(p, __builtin_amdgcn_readfirstlane((int)rp), R, b, ray_v, o3, d3);
            ray = __builtin_amdgcn_readfirstlane(ray_v);
            if (p.t_near) {                         // (wave-uniform: the limit-less list call never enters)
                const float t_near = p.t_near[ray], t_far = p.t_far[ray];
                if (!(fabsf(t_near) < INFINITY && fabsf(t_far) < INFINITY && t_far > t_near)) continue;
            }
        } else {
            ray_of(__builtin_amdgcn_readfirstlane((int)rp), a.res, b, pi, pj);
            ray = __builtin_amdgcn_readfirstlane(b * R + pi * a.res + pj);
        }
        const float Gh[3] = {g_normal[(size_t)ray * 3], g_normal[(size_t)ray * 3 + 1], g_normal[(size_t)ray * 3 + 2]};
        if (Gh[0] == 0.f && Gh[1] == 0.f && Gh[2] == 0.f) continue;       // (wave-uniform)
        any = true;
        if constexpr (!LIST) ray_setup(a, b, pi, pj, o3, d3);
        // (twin: normals_load_ray, raymarch_normals_common.h)
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
        {
            Composite c;
            composite<S>(ts, ss, lane, c);
            midpoints_to_samples<S>(c.w[0], c.w[1], lane, om);
        }
        WAVE_SYNC();
        // ---- pass A: n_s and 1 / r_s of every sample, as raymarch_normals_kernel computes them
        // (twin: normals_pass_a, raymarch_normals_common.h, which forms a in fp32; a change here belongs there too)
#pragma unroll 1
        for (int tt = 0; tt < NT; ++tt) {
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
            if constexpr (A16) decoder_bwd16_lds<false>(wfwd, nullptr, g0img, ln, o, 1.f, hp, dH, dF2);
            else if constexpr (DEC16) { decoder_dh_lds<true>(wfwd, ln, hp, dH); w0t_mul(w0t, ln, dH, dF2); }
            else decoder_bwd_lds<false>(wfwd, nullptr, w0t, ln, o, 1.f, hp, dH, dF2);
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
        WAVE_SYNC();
        // ---- the compositing adjoint (raymarch.hip) with the normals as colours: G_e = G^ . (n_e + n_{e+1}) / 2 -> d sigma_s
        // (twin: normals_weight_adjoint, raymarch_normals_common.h)
        {
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
        WAVE_SYNC();
        // ---- pass B
        float* pbase = d_planes + (size_t)b * 3 * plane_stride;
#pragma unroll 1
        for (int tt = 0; tt < NT; ++tt) {
            const int s = 16 * tt + j;
            const float om_s = om[s], ds_s = dsg[s];
            const bool live = om_s != 0.f || ds_s != 0.f;
            if (__builtin_amdgcn_ballot_w64(live) == 0) continue;
            int ln = lane;
            asm volatile("" : "+v"(ln));
            float q[3];
            sample_point(p, o3, d3, ts[s], q);
            // gamma_q = coord_scale dL/dg = -coord_scale (omega / r) (G^ - n (n . G^))   (twin: normals_gamma_q, raymarch_normals_common.h)
            float gq[3];
            {
                const float n3[3] = {nx[s], ny[s], nz[s]};
                const float ndg = fmaf(Gh[2], n3[2], fmaf(Gh[1], n3[1], Gh[0] * n3[0]));
                const float cf = -(om_s * ri[s]) * p.coord_scale;
#pragma unroll
                for (int k = 0; k < 3; ++k) gq[k] = cf * (Gh[k] - n3[k] * ndg);
            }
            // the bilinear taps (w_k) and their derivative weights (w'_k), all three planes on every lane
            // (twin: normals_second_taps, raymarch_normals_common.h)
            PlaneTaps taps[3], dtaps[3];
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
            float f[8], u[8];
            gather8(a, b, g, taps, f);
            gather8(a, b, g, dtaps, u);
            f32x4 hp[4], h[4], o[2];
            float sigma;
            if constexpr (DEC16) decoder_fwd16_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            else decoder_fwd_lds<true>(wfwd, ln, f, hp, h, sigma, o);
            f32x4 dH[4], av[2];                  // dH = wsig sigmoid(hp); av = a = W0'^T dH (as pass A)
            if constexpr (A16) decoder_bwd16_lds<false>(wfwd, nullptr, g0img, ln, o, 1.f, hp, dH, av);
            else if constexpr (DEC16) { decoder_dh_lds<true>(wfwd, ln, hp, dH); w0t_mul(w0t, ln, dH, av); }
            else decoder_bwd_lds<false>(wfwd, nullptr, w0t, ln, o, 1.f, hp, dH, av);
            f32x4 v[4], x[4];
            w0_mul(w0fwd, ln, u, v);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float sg = sigmoid_f(hp[mt][r]);
                    const float e = dH[mt][r] * (1.f - sg) * v[mt][r];
                    x[mt][r] = fmaf(dH[mt][r], ds_s, e);
                    if constexpr (PG) {
                        acc.s_x[mt][r] += x[mt][r];
                        acc.s_sw[mt][r] += fmaf(ds_s, h[mt][r], sg * v[mt][r]);
                    }
                }
            f32x4 dF[2];
            w0t_mul(w0t, ln, x, dF);
            if constexpr (PG) {
                if (g == 0) acc.s_ds += ds_s;
                nrm_grad_tile(acc, gl, j, g, f, u, x, dH);
            }
            // d planes: (w_k / 3) dF + (w'_k / 3) a; a dead sample of a live tile publishes weights 0 (its dF and w' are 0)
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
            scatter_tile_runs2<6>(lds, dfc, avc, pbase, plane_stride, lane);
            WAVE_SYNC();                        // the next tile overwrites the wave's LDS tables
        }
        WAVE_SYNC();       // the next ray overwrites the per-ray tables
    }
    if constexpr (PG) {
        if (any) nrm_grad_flush(acc, dg, a.decoder_lr_mul, lane);
    }
}

template <int S, bool DEC16, bool PG, bool LIST>
static int launch_nb(const RayParams& p, const float* g_normal, float* d_planes, const DecGrads& dg, hipStream_t s) {
    // one round of resident workgroups, each wave walking its run of rays
    static int resident = 0;
    if (resident == 0) {
        int n = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, raymarch_normals_bwd_kernel<S, DEC16, PG, LIST>, kNbWaves * 64, 0) != hipSuccess ||
            n < 1)
            n = 1;
        resident = n;
    }
    const long long blocks = std::min<long long>(((long long)p.total_rays + kNbWaves - 1) / kNbWaves, (long long)kNumCU * resident);
    raymarch_normals_bwd_kernel<S, DEC16, PG, LIST><<<(unsigned)blocks, kNbWaves * 64, 0, s>>>(p, g_normal, d_planes, dg);
    return check_launch(LIST ? "raymarch_rays_normals_bwd" : "raymarch_normals_bwd");
}

template <int S, bool LIST>
static int launch_nb_s(const RayParams& p, const float* g_normal, float* d_planes, const DecGrads& dg, bool pg, hipStream_t s) {
    if (p.a.planes_absmax)
        return pg ? launch_nb<S, true, true, LIST>(p, g_normal, d_planes, dg, s) : launch_nb<S, true, false, LIST>(p, g_normal, d_planes, dg, s);
    return pg ? launch_nb<S, false, true, LIST>(p, g_normal, d_planes, dg, s) : launch_nb<S, false, false, LIST>(p, g_normal, d_planes, dg, s);
}

}  // namespace hfagp

using namespace hfagp;

#ifndef HFAGP_RAY_LIST_UNIT        // (raymarch_rays_normals.hip compiles this source again for the list entry point alone)
extern "C" int hfagp_raymarch_normals_bwd(const HfagpRaymarchArgs* fwd, const float* g_normal, float* d_planes, float* d_dec_w0,
                                          float* d_dec_b0, float* d_dec_w1, float* d_dec_b1, void* stream) {
    HFAGP_REQUIRE(fwd && g_normal && d_planes && fwd->state && fwd->planes, HFAGP_EBADARG, "raymarch_normals_bwd: null pointer");
    const bool pg = d_dec_w0 || d_dec_b0 || d_dec_w1 || d_dec_b1;
    HFAGP_REQUIRE(!pg || (d_dec_w0 && d_dec_b0 && d_dec_w1 && d_dec_b1), HFAGP_EBADARG,
                  "raymarch_normals_bwd: the four decoder gradients go together (all or none)");
    RayParams p;
    const int rc = fill_ray_params(fwd, p, "raymarch_normals_bwd");
    if (rc != HFAGP_OK) return rc;
    const DecGrads dg = {d_dec_w0, d_dec_b0, d_dec_w1, d_dec_b1};
    hipStream_t s = (hipStream_t)stream;
    const int S = fwd->Sc + fwd->Sf;
    if (S == 96) return launch_nb_s<96, false>(p, g_normal, d_planes, dg, pg, s);
    if (S == 64) return launch_nb_s<64, false>(p, g_normal, d_planes, dg, pg, s);
    return launch_nb_s<32, false>(p, g_normal, d_planes, dg, pg, s);
}

#else
extern "C" int hfagp_raymarch_rays_normals_bwd(const HfagpRayListArgs* a, const HfagpRayLimits* lim, const float* g_normal,
                                               float* d_planes, float* d_dec_w0, float* d_dec_b0, float* d_dec_w1, float* d_dec_b1,
                                               void* stream) {
    HFAGP_REQUIRE(a && g_normal && d_planes && a->base.state, HFAGP_EBADARG, "raymarch_rays_normals_bwd: null pointer");
    HFAGP_REQUIRE(!lim || (lim->t_near && lim->t_far), HFAGP_EBADARG, "raymarch_rays_normals_bwd: null pointer (limits)");
    const bool pg = d_dec_w0 || d_dec_b0 || d_dec_w1 || d_dec_b1;
    HFAGP_REQUIRE(!pg || (d_dec_w0 && d_dec_b0 && d_dec_w1 && d_dec_b1), HFAGP_EBADARG,
                  "raymarch_rays_normals_bwd: the four decoder gradients go together (all or none)");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->base, p, "raymarch_rays_normals_bwd", &rays, lim != nullptr);
    if (rc != HFAGP_OK) return rc;
    if (lim) { p.t_near = lim->t_near; p.t_far = lim->t_far; }
    const DecGrads dg = {d_dec_w0, d_dec_b0, d_dec_w1, d_dec_b1};
    hipStream_t s = (hipStream_t)stream;
    const int S = a->base.Sc + a->base.Sf;
    if (S == 96) return launch_nb_s<96, true>(p, g_normal, d_planes, dg, pg, s);
    if (S == 64) return launch_nb_s<64, true>(p, g_normal, d_planes, dg, pg, s);
    return launch_nb_s<32, true>(p, g_normal, d_planes, dg, pg, s);
}
#endif
