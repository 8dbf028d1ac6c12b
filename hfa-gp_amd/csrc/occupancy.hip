// Occupancy grids for ray lists: hfagp_occupancy_pack (a density lattice -> one bit per cell) and hfagp_ray_limits_grid (per ray the
// [first entry, last exit] of the occupied cells it passes through — tight limits and a correct miss test for
// hfagp_raymarch_rays_limits_*, where hfagp_ray_limits_box only knows the tri-plane cube).
//
// The grid: G^3 cells over the cube [-L/2, L/2]^3, cell (ix, iy, iz) the box [plane(i), plane(i + 1)] per axis with
//   plane(i) = -L/2 + float(i) * (L / float(G))      (fp32, every operation rounded on its own; plane(0) = -L/2 exactly)
// bits [B][G][G][W] int32, W = ceil(G / 32): bit (iz & 31) of word (iz >> 5) at [b][ix][iy]; padding bits are 0.
//
// Ray limits.  A cell counts for a ray iff its bit is set and its slab interval has a POSITIVE chord at t >= 0:
//   per axis k with d_k != 0:  inv = 1 / d_k,  ta = (plane(i_k) - o_k) * inv,  tb = (plane(i_k + 1) - o_k) * inv   (the formula of
//                              ray_limits_box_kernel, on the cell's planes),  in_k = min(ta, tb),  out_k = max(ta, tb)
//   per axis k with d_k == 0:  the ray lies in the half-open slab plane(i) <= o_k < plane(i + 1) of exactly one i (in = -inf,
//                              out = +inf there); o_k <= plane(0) or o_k >= plane(G) — the box kernel's 0 * inf — empties the ray
//   near_c = max_k in_k,  far_c = min_k out_k,  the cell counts iff far_c > max(near_c, 0)  (any NaN: it does not)
//   t_near = min over the counting cells of max(near_c, 0),   t_far = max over them of far_c.
// No counting cell, a zero direction, or a result that is not finite: (+inf, -inf), an EMPTY ray to the list kernels.
// cam_utils.ray_limits_grid evaluates exactly this over EVERY occupied cell (no traversal); the kernel finds the cells with a 3-D
// DDA (Amanatides & Woo) and must agree with it to rounding, so:
//   * every t that is compared or reported is RECOMPUTED from the integer plane index with the formula above — never an
//     accumulated tMax += tDelta; the DDA decides only which cells are looked at, each cell's verdict is the formula's;
//   * the start cell of a ray that enters from outside has index 0 or G-1 on the crossed axis BY CONSTRUCTION (not the floor of a
//     rounded position); the other indices are floored, clamped to [0, G-1] and moved so that plane(i) <= p < plane(i + 1) holds in
//     the kernel's own plane arithmetic; an origin inside the cube starts at its own cell.  A start cell that rounding put one cell
//     back has a non-positive chord: it is not counted and the DDA steps out of it at once;
//   * an axis with d_k == 0 never steps;
//   * the walk is bounded at 3 G + 3 steps whatever the arithmetic does (NaN / inf inputs included): nothing here can spin.
// One thread per ray; the bits are read through the caches (at G = 64 a frame's grid is 32 KB and a block's 256 rays touch a few
// hundred of its words, so staging all of it in LDS per block would read more than it saves — see profiles/occupancy/README.md).
// Plain vector stores, no atomics.
#include "common.h"

// "every operation rounded on its own" needs more than the _rn intrinsics: inlined from their header, __fmul_rn and __fadd_rn still
// carry its contraction flag, and hipcc fused plane(i)'s multiply and add into one v_fma_f32 (seen in this unit's ISA), which
// moves the planes of a grid whose L / G is inexact (G = 40) off the reference's by an ulp.  So the products, sums and differences
// below are plain operators compiled with contraction OFF; only the division keeps its intrinsic (correctly rounded).
#pragma clang fp contract(off)

namespace hfagp {

__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }
__device__ __forceinline__ float sub_rn(float a, float b) { return a - b; }
__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }

__device__ __forceinline__ float grid_plane(int i, float half, float cell) { return add_rn(-half, mul_rn((float)i, cell)); }

__global__ void __launch_bounds__(256) ray_limits_grid_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                             const int* __restrict__ bits, float* __restrict__ t_near,
                                                             float* __restrict__ t_far, int B, int R, int G, int W, float half,
                                                             float cell, float inv_cell) {
    const long long ray = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray >= (long long)B * R) return;
    const int* __restrict__ grid = bits + (size_t)(ray / R) * G * G * W;
    float best_near = INFINITY, best_far = -INFINITY;
    float ok[3], dir[3], inv[3], t_in[3], t_out[3];
    int step[3], idx[3];
    bool empty = false;
    // the cube's own slabs: does the ray meet the grid at all, and where does it enter
    float enter = -INFINITY, leave = INFINITY;
    int crossed = -1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok[k] = o[ray * 3 + k];
        const float dk = dir[k] = d[ray * 3 + k];
        inv[k] = __fdiv_rn(1.f, dk);
        step[k] = dk > 0.f ? 1 : dk < 0.f ? -1 : 0;
        const float lo = grid_plane(0, half, cell), hi = grid_plane(G, half, cell);
        if (dk != dk || ok[k] != ok[k]) empty = true;
        if (step[k] == 0) {
            if (!(ok[k] > lo && ok[k] < hi)) empty = true;          // parallel and outside, or exactly on a face: 0 * inf
            continue;
        }
        const float ta = mul_rn(sub_rn(lo, ok[k]), inv[k]), tb = mul_rn(sub_rn(hi, ok[k]), inv[k]);
        const float a_in = step[k] > 0 ? ta : tb, a_out = step[k] > 0 ? tb : ta;
        if (a_in != a_in || a_out != a_out) empty = true;
        if (a_in > enter) { enter = a_in; crossed = k; }
        leave = fminf(leave, a_out);
    }
    if (step[0] == 0 && step[1] == 0 && step[2] == 0) empty = true;
    if (!(leave > fmaxf(enter, 0.f))) empty = true;
    if (!empty) {
        const bool outside = enter > 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int i;
            if (outside && k == crossed) {
                i = step[k] > 0 ? 0 : G - 1;
            } else {
                const float p = outside ? add_rn(ok[k], mul_rn(enter, dir[k])) : ok[k];
                const float f = fminf(fmaxf(floorf(mul_rn(add_rn(p, half), inv_cell)), 0.f), (float)(G - 1));   // (NaN -> 0)
                i = (int)f;
                for (int fix = 0; fix < 2; ++fix) {                 // the floor, held to the kernel's own planes
                    if (i > 0 && p < grid_plane(i, half, cell)) --i;
                    else if (i < G - 1 && p >= grid_plane(i + 1, half, cell)) ++i;
                }
            }
            idx[k] = i;
            if (step[k] == 0) {
                t_in[k] = -INFINITY;
                t_out[k] = INFINITY;
            } else {
                const float ta = mul_rn(sub_rn(grid_plane(i, half, cell), ok[k]), inv[k]);
                const float tb = mul_rn(sub_rn(grid_plane(i + 1, half, cell), ok[k]), inv[k]);
                t_in[k] = step[k] > 0 ? ta : tb;
                t_out[k] = step[k] > 0 ? tb : ta;
            }
        }
        const int max_steps = 3 * G + 3;                            // HARD bound: at most 3 (G - 1) + 1 cells lie on a ray
        for (int it = 0; it < max_steps; ++it) {
            const int word = grid[((size_t)idx[0] * G + idx[1]) * W + (idx[2] >> 5)];
            if ((word >> (idx[2] & 31)) & 1) {
                const bool nan = t_in[0] != t_in[0] || t_in[1] != t_in[1] || t_in[2] != t_in[2] || t_out[0] != t_out[0] ||
                                 t_out[1] != t_out[1] || t_out[2] != t_out[2];
                const float near_c = fmaxf(fmaxf(fmaxf(t_in[0], t_in[1]), t_in[2]), 0.f);
                const float far_c = fminf(fminf(t_out[0], t_out[1]), t_out[2]);
                if (!nan && far_c > near_c) {
                    best_near = fminf(best_near, near_c);
                    best_far = fmaxf(best_far, far_c);
                }
            }
            int a = 0;                                              // the axis whose exit plane comes first (ties: x, y, z)
            float first = t_out[0];
            if (t_out[1] < first) { first = t_out[1]; a = 1; }
            if (t_out[2] < first) a = 2;
            // (a is written out per axis: dynamic indexing of the small arrays would put them in scratch)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k != a) continue;
                if (step[k] == 0) { it = max_steps; break; }        // only NaN / inf exits are left: stop
                idx[k] += step[k];
                if (idx[k] < 0 || idx[k] >= G) { it = max_steps; break; }
                t_in[k] = t_out[k];                                 // the plane just crossed: the same index, the same formula
                t_out[k] = mul_rn(sub_rn(grid_plane(idx[k] + (step[k] > 0 ? 1 : 0), half, cell), ok[k]), inv[k]);
            }
        }
    }
    const bool hit = best_far > best_near && best_near >= 0.f && best_far < INFINITY;
    t_near[ray] = hit ? best_near : INFINITY;
    t_far[ray] = hit ? best_far : -INFINITY;
}

// One wave per output column [b][ix][iy][:].  Pass 1: lane p (a z index of the lattice, coalesced along z) ORs !(v < level) over
// the x / y lattice rows of the cell's dilated extent -> one ballot per 64 z points, kept in LDS.  Pass 2: lane iz ORs the bits of
// its dilated z extent -> one ballot per 64 cells = two output words, written by lane 0 with plain stores.
constexpr int kPackMaxLattice = 1025;                               // G * k + 1 <= 1025
constexpr int kPackMaxDilate = 8;

__global__ void __launch_bounds__(64) occupancy_pack_kernel(const float* __restrict__ vol, int* __restrict__ bits, int G, int k,
                                                           int W, float level, int dil) {
    __shared__ unsigned long long hot[(kPackMaxLattice + 63) / 64];
    const int lane = threadIdx.x;
    const int iy = blockIdx.x % G, ix = (blockIdx.x / G) % G, b = blockIdx.x / (G * G);
    const int n = G * k + 1;
    const int x0 = max(ix - dil, 0) * k, x1 = (min(ix + dil, G - 1) + 1) * k;
    const int y0 = max(iy - dil, 0) * k, y1 = (min(iy + dil, G - 1) + 1) * k;
    const float* __restrict__ frame = vol + (size_t)b * n * n * n;
    for (int c = 0; c * 64 < n; ++c) {
        const int p = c * 64 + lane;
        bool h = false;
        if (p < n)
            for (int x = x0; x <= x1; ++x)
                for (int y = y0; y <= y1; ++y) h = h || !(frame[((size_t)x * n + y) * n + p] < level);      // (NaN: occupied)
        const unsigned long long m = __ballot(h);
        if (lane == 0) hot[c] = m;
    }
    __syncthreads();
    int* __restrict__ out = bits + (size_t)blockIdx.x * W;
    for (int c = 0; c * 64 < G; ++c) {
        const int iz = c * 64 + lane;
        bool occ = false;
        if (iz < G) {
            const int p0 = max(iz - dil, 0) * k, p1 = (min(iz + dil, G - 1) + 1) * k;
            for (int p = p0; p <= p1; ++p) occ = occ || ((hot[p >> 6] >> (p & 63)) & 1ull);
        }
        const unsigned long long m = __ballot(occ);
        if (lane == 0) {
            out[2 * c] = (int)(unsigned)(m & 0xffffffffull);
            if (2 * c + 1 < W) out[2 * c + 1] = (int)(unsigned)(m >> 32);
        }
    }
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_ray_limits_grid(const float* ray_origins, const float* ray_directions, const int32_t* bits, float* t_near,
                                     float* t_far, int32_t B, int32_t R, int32_t G, float box_side, void* stream) {
    HFAGP_REQUIRE(ray_origins && ray_directions && bits && t_near && t_far, HFAGP_EBADARG, "ray_limits_grid: null pointer");
    HFAGP_REQUIRE(B > 0 && R > 0 && (long long)B * R < (1ll << 31), HFAGP_EBADARG, "ray_limits_grid: B = %d, R = %d", B, R);
    HFAGP_REQUIRE(G >= 2 && G <= 256, HFAGP_EBADARG, "ray_limits_grid: G = %d (2 .. 256)", G);
    HFAGP_REQUIRE(box_side > 0.f && box_side < INFINITY, HFAGP_EBADARG, "ray_limits_grid: box_side = %g", (double)box_side);
    const unsigned blocks = (unsigned)(((long long)B * R + 255) / 256);
    ray_limits_grid_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(ray_origins, ray_directions, bits, t_near, t_far, B, R, G,
                                                                   (G + 31) / 32, box_side * 0.5f, box_side / (float)G,
                                                                   (float)G / box_side);
    return check_launch("ray_limits_grid");
}

extern "C" int hfagp_occupancy_pack(const float* volume, int32_t* bits, int32_t B, int32_t G, int32_t oversample, float level,
                                    int32_t dilate, void* stream) {
    HFAGP_REQUIRE(volume && bits, HFAGP_EBADARG, "occupancy_pack: null pointer");
    HFAGP_REQUIRE(B > 0 && B <= 4096, HFAGP_EBADARG, "occupancy_pack: B = %d", B);
    HFAGP_REQUIRE(G >= 2 && G <= 256, HFAGP_EBADARG, "occupancy_pack: G = %d (2 .. 256)", G);
    HFAGP_REQUIRE(oversample >= 1 && (long long)G * oversample + 1 <= kPackMaxLattice, HFAGP_EBADARG,
                  "occupancy_pack: oversample = %d (>= 1, G * oversample + 1 <= %d)", oversample, kPackMaxLattice);
    HFAGP_REQUIRE(dilate >= 0 && dilate <= kPackMaxDilate, HFAGP_EBADARG, "occupancy_pack: dilate = %d (0 .. %d)", dilate, kPackMaxDilate);
    HFAGP_REQUIRE(level == level, HFAGP_EBADARG, "occupancy_pack: level is NaN");
    occupancy_pack_kernel<<<(unsigned)B * G * G, 64, 0, (hipStream_t)stream>>>(volume, bits, G, oversample, (G + 31) / 32, level, dilate);
    return check_launch("occupancy_pack");
}
