// Antialiased bilinear resample of a channels-last image and its adjoint (hfagp.h HfagpResizeAaArgs): the step between the ray
// marcher and the super-resolution blocks when the rays were marched at another resolution than the blocks' input.
// Both directions are ONE gather: destination (y, x) sums  wh[ky] * ww[kx] * src[y0 + ky][x0 + kx]  over the two table rows of its
// coordinates — the forward over the taps of an output, the adjoint over the outputs that read an input (the transposed tables the
// host builds with the forward ones).  No weight is computed here, nothing is accumulated in memory: every destination element is
// written once by one lane, in table order, so two launches give the same bits.
// HBM-streaming: one lane per four channels (16-byte loads and stores; the eight lanes of a 32-channel pixel cover its 128 B and
// a wave covers eight neighbouring pixels of a row), fp32 accumulation, no LDS — the windows of neighbouring destinations overlap
// and the re-reads are served by L2.
#include "common.h"

using namespace hfagp;

namespace {

struct ResizeParams {
    const float4* src;
    float4* dst;
    const float* add3;               // adjoint: [B][3][Hd][Wd] added to channels 0..2, or null
    const int32_t *table_h, *table_w;
    int Hs, Ws, Hd, Wd, C4, kmax;    // source and destination extents, float4s per pixel
    unsigned total;                  // B * Hd * Wd * C4 destination float4s
};

template <bool ADJOINT>
__device__ __forceinline__ void resize_body(const ResizeParams& p) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;
    if (t >= p.total) return;
    const int c4 = (int)(t % (unsigned)p.C4);
    unsigned pix = t / (unsigned)p.C4;
    const int x = (int)(pix % (unsigned)p.Wd);
    pix /= (unsigned)p.Wd;
    const int y = (int)(pix % (unsigned)p.Hd);
    const int b = (int)(pix / (unsigned)p.Hd);
    const int32_t* rh = p.table_h + (size_t)y * (2 + p.kmax);
    const int32_t* rw = p.table_w + (size_t)x * (2 + p.kmax);
    // (a row that does not fit its source is cut, never followed out of bounds: the tables are the caller's)
    const int y0 = min(max(rh[0], 0), p.Hs), ny = min(min(rh[1], p.kmax), p.Hs - y0);
    const int x0 = min(max(rw[0], 0), p.Ws), nx = min(min(rw[1], p.kmax), p.Ws - x0);
    const float* wh = reinterpret_cast<const float*>(rh + 2);
    const float* ww = reinterpret_cast<const float*>(rw + 2);
    const float4* s = p.src + ((size_t)b * p.Hs + y0) * p.Ws * p.C4 + (size_t)x0 * p.C4 + c4;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int ky = 0; ky < ny; ++ky, s += (size_t)p.Ws * p.C4) {
        float4 row = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int kx = 0; kx < nx; ++kx) {
            const float4 v = s[(size_t)kx * p.C4];
            const float w = ww[kx];
            row.x = fmaf(w, v.x, row.x);
            row.y = fmaf(w, v.y, row.y);
            row.z = fmaf(w, v.z, row.z);
            row.w = fmaf(w, v.w, row.w);
        }
        const float w = wh[ky];
        acc.x = fmaf(w, row.x, acc.x);
        acc.y = fmaf(w, row.y, acc.y);
        acc.z = fmaf(w, row.z, acc.z);
        acc.w = fmaf(w, row.w, acc.w);
    }
    if (ADJOINT && p.add3 && c4 == 0) {
        const size_t plane = (size_t)p.Hd * p.Wd;
        const float* g = p.add3 + (size_t)b * 3 * plane + (size_t)y * p.Wd + x;
        acc.x += g[0];
        acc.y += g[plane];
        acc.z += g[2 * plane];
    }
    p.dst[t] = acc;
}

__global__ __launch_bounds__(256) void resize_aa_kernel(const ResizeParams p) { resize_body<false>(p); }

__global__ __launch_bounds__(256) void resize_aa_bwd_kernel(const ResizeParams p) { resize_body<true>(p); }

int resize_run(const HfagpResizeAaArgs* a, bool adjoint, const char* who, hipStream_t stream) {
    HFAGP_REQUIRE(a && a->src && a->dst && a->table_h && a->table_w, HFAGP_EBADARG, "%s: null pointer", who);
    HFAGP_REQUIRE(a->B > 0 && a->Hi > 0 && a->Wi > 0 && a->Ho > 0 && a->Wo > 0 && a->C > 0, HFAGP_EUNSUPPORTED,
                  "%s: empty extent (B %d, %d x %d -> %d x %d, C %d)", who, a->B, a->Hi, a->Wi, a->Ho, a->Wo, a->C);
    HFAGP_REQUIRE(a->C % 4 == 0, HFAGP_EUNSUPPORTED, "%s: C=%d must be a multiple of 4", who, a->C);
    HFAGP_REQUIRE(a->kmax >= 1 && a->kmax <= HFAGP_RESIZE_AA_KMAX, HFAGP_EUNSUPPORTED,
                  "%s: kmax=%d is outside 1..%d, what the kernel was compiled for", who, a->kmax, HFAGP_RESIZE_AA_KMAX);
    HFAGP_REQUIRE(4ll * a->Hi >= a->Ho && a->Hi <= 4ll * a->Ho && 4ll * a->Wi >= a->Wo && a->Wi <= 4ll * a->Wo, HFAGP_EUNSUPPORTED,
                  "%s: %d x %d -> %d x %d is outside the supported ratios n_out / 4 <= n_in <= 4 n_out", who, a->Hi, a->Wi, a->Ho,
                  a->Wo);
    ResizeParams p;
    p.src = reinterpret_cast<const float4*>(a->src);
    p.dst = reinterpret_cast<float4*>(a->dst);
    p.add3 = adjoint ? a->add_nchw3 : nullptr;
    p.table_h = a->table_h;
    p.table_w = a->table_w;
    p.Hs = adjoint ? a->Ho : a->Hi;
    p.Ws = adjoint ? a->Wo : a->Wi;
    p.Hd = adjoint ? a->Hi : a->Ho;
    p.Wd = adjoint ? a->Wi : a->Wo;
    p.C4 = a->C / 4;
    p.kmax = a->kmax;
    const long long total = (long long)a->B * p.Hd * p.Wd * p.C4;
    HFAGP_REQUIRE(total < (1ll << 31), HFAGP_EUNSUPPORTED, "%s: too many outputs (%lld float4s)", who, total);
    p.total = (unsigned)total;
    const unsigned blocks = (unsigned)((total + 255) / 256);
    if (adjoint)
        resize_aa_bwd_kernel<<<blocks, 256, 0, stream>>>(p);
    else
        resize_aa_kernel<<<blocks, 256, 0, stream>>>(p);
    return check_launch(who);
}

}  // namespace

extern "C" int hfagp_resize_aa_fwd(const HfagpResizeAaArgs* a, void* stream) {
    return resize_run(a, false, "resize_aa_fwd", (hipStream_t)stream);
}

extern "C" int hfagp_resize_aa_bwd(const HfagpResizeAaArgs* a, void* stream) {
    return resize_run(a, true, "resize_aa_bwd", (hipStream_t)stream);
}
