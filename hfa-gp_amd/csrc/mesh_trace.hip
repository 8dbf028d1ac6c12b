// First hit of a ray list with a triangle mesh (gfx950): per ray the nearest face, t, the barycentric weights, the point, the
// geometric normal and the facing.  Notation and the arithmetic of include/hfagp.h (hfagp_trace_mesh); mesh.trace_mesh_reference
// states the same in torch, and both kernels must give its float32 bits.
//
// One intersection function (`intersect`) serves both kernels and the final evaluation of the winner (`finish`), so a face gives
// the same (candidate, t) wherever it is tested, and the outputs are those of the winning face's own evaluation:
//   * the three edge functions U, V, W are scalar triple products of the SAME vectors a - o, b - o, c - o in a fixed operand order:
//     the face across an edge computes the negated bits, so one of the two accepts a ray through the edge — no cracks along the
//     edges of a consistently wound mesh (DESIGN.md has the argument and the one leak, rays aimed exactly at a vertex);
//   * every operation is rounded on its own: contraction is OFF for the whole unit (occupancy.hip's note on why the _rn
//     intrinsics alone do not do it); the division and the square root are the correctly rounded ones.
// Brute force (trace_mesh_brute_kernel): a lane owns a ray, a block of 256 rays streams the faces of its frame through LDS in tiles
//   of kMeshTile records of 36 bytes; every lane reads the same record at the same time (an LDS broadcast: no bank conflicts) and tests
//   it.  9 KB of LDS per block: the tile does not limit occupancy; a larger one would only add to the barrier's latency.
// Grid (trace_mesh_grid_kernel): a lane owns a ray and walks the cells of a uniform grid with occupancy.hip's DDA — every t that is
//   compared is recomputed from the integer plane index, an axis with d = 0 never steps, at most 3 G + 3 cells — testing the faces
//   of each cell's list.  It keeps the lexicographic minimum of (t, face) over everything tested and stops once that t lies before
//   the exit of the current cell, or past t_far, or outside the box.  Offsets and face indices read from the lists are clamped.
// Nothing spins, no atomics, one writer per ray with plain stores: two calls give the same bits.
#include <climits>
#include "common.h"

#pragma clang fp contract(off)

namespace hfagp {

constexpr int kMeshTile = 256;                  // faces per LDS tile (tests/test_gpu_mesh_trace.py runs F = kMeshTile - 1, +0, +1)

struct MeshParams {
    const float* tri;                           // [tri_frames][F][9]
    const float* ray_o, *ray_d;                 // [B][R][3]
    const float* t_near, *t_far;                // [B][R]
    const int* cell_start;                      // [tri_frames][G^3 + 1]
    const int* cell_faces;                      // [n_pairs]
    const float* box;                           // [tri_frames][6]
    unsigned char* hit, *front;                 // outputs, NULL = not written
    int* face;
    float* t, *bary, *point, *normal;
    int B, R, F, G;
    int per_frame;                              // 1: tri / grid per ray frame, 0: one for all
    int n_pairs;
    int tiles_per_b;                            // ceil(R / 256) (brute force)
};

struct MeshRay {
    float o[3], d[3], tn, tf;
};

struct FaceHit {
    float U, V, W, det, N[3], dn, t;
    bool cand;
};

__device__ __forceinline__ void cross3(const float x[3], const float y[3], float r[3]) {
    r[0] = x[1] * y[2] - x[2] * y[1];
    r[1] = x[2] * y[0] - x[0] * y[2];
    r[2] = x[0] * y[1] - x[1] * y[0];
}
__device__ __forceinline__ float dot3(const float x[3], const float y[3]) { return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]; }

// the one definition of a ray against a face; v = (a, b, c), 9 floats in LDS or global memory
__device__ __forceinline__ FaceHit intersect(const MeshRay& r, const float* __restrict__ v) {
    float a[3], b[3], c[3], A[3], Bv[3], Cv[3], e1[3], e2[3], x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a[k] = v[k]; b[k] = v[3 + k]; c[k] = v[6 + k];
        A[k] = a[k] - r.o[k]; Bv[k] = b[k] - r.o[k]; Cv[k] = c[k] - r.o[k];
        e1[k] = b[k] - a[k]; e2[k] = c[k] - a[k];
    }
    FaceHit h;
    cross3(Bv, Cv, x); h.U = dot3(r.d, x);
    cross3(Cv, A, x);  h.V = dot3(r.d, x);
    cross3(A, Bv, x);  h.W = dot3(r.d, x);
    h.det = (h.U + h.V) + h.W;
    cross3(e1, e2, h.N);
    h.dn = dot3(r.d, h.N);
    h.t = __fdiv_rn(dot3(A, h.N), h.dn);
    const bool pos = h.U >= 0.f && h.V >= 0.f && h.W >= 0.f, neg = h.U <= 0.f && h.V <= 0.f && h.W <= 0.f;
    h.cand = (pos || neg) && h.det != 0.f && h.dn != 0.f && r.tn <= h.t && h.t <= r.tf;
    return h;
}

// the lexicographic minimum of (t, face)
__device__ __forceinline__ void keep(const FaceHit& h, int f, float& best_t, int& best_f) {
    const bool better = h.cand && (h.t < best_t || (h.t == best_t && f < best_f));
    best_t = better ? h.t : best_t;
    best_f = better ? f : best_f;
}

__device__ __forceinline__ void load_ray(const MeshParams& p, size_t ray, MeshRay& r) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { r.o[k] = p.ray_o[ray * 3 + k]; r.d[k] = p.ray_d[ray * 3 + k]; }
    r.tn = p.t_near[ray];
    r.tf = p.t_far[ray];
}

// a ray that cannot hit whatever the mesh is: a NaN anywhere, a zero direction, t_far < t_near — a miss before any face is read
__device__ __forceinline__ bool dead_ray(const MeshRay& r) {
    bool nan = r.tn != r.tn || r.tf != r.tf;
#pragma unroll
    for (int k = 0; k < 3; ++k) nan = nan || r.o[k] != r.o[k] || r.d[k] != r.d[k];
    const bool zero = r.d[0] == 0.f && r.d[1] == 0.f && r.d[2] == 0.f;
    return nan || zero || !(r.tn <= r.tf);
}

// the winner's own evaluation -> the outputs (a miss: zeros)
__device__ __forceinline__ void finish(const MeshParams& p, size_t ray, const MeshRay& r, const float* __restrict__ tri_b, int best_f) {
    const bool hit = best_f != INT_MAX;
    float t = 0.f, bary[3] = {0.f, 0.f, 0.f}, x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    bool front = false;
    if (hit) {
        const FaceHit h = intersect(r, tri_b + (size_t)best_f * 9);
        t = h.t;
        bary[0] = __fdiv_rn(h.U, h.det); bary[1] = __fdiv_rn(h.V, h.det); bary[2] = __fdiv_rn(h.W, h.det);
        const float len = sqrtf(dot3(h.N, h.N));        // correctly rounded (__fsqrt_rn is the 1-ulp native instruction here)
#pragma unroll
        for (int k = 0; k < 3; ++k) { x[k] = r.o[k] + t * r.d[k]; n[k] = __fdiv_rn(h.N[k], len); }
        front = h.dn < 0.f;
    }
    if (p.hit) p.hit[ray] = hit ? 1 : 0;
    if (p.front) p.front[ray] = front ? 1 : 0;
    if (p.face) p.face[ray] = hit ? best_f : -1;
    if (p.t) p.t[ray] = t;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (p.bary) p.bary[ray * 3 + k] = bary[k];
        if (p.point) p.point[ray * 3 + k] = x[k];
        if (p.normal) p.normal[ray * 3 + k] = n[k];
    }
}

__global__ void __launch_bounds__(256) trace_mesh_brute_kernel(const MeshParams p) {
    __shared__ float tile[kMeshTile * 9];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / p.tiles_per_b;                               // block-uniform
    const int r_in_b = (blockIdx.x - b * p.tiles_per_b) * 256 + tid;
    const bool valid = r_in_b < p.R;
    const size_t ray = (size_t)b * p.R + min(r_in_b, p.R - 1);              // a lane past R reads the last ray and stores nothing
    const float* __restrict__ tri_b = p.tri + (p.per_frame ? (size_t)b * p.F * 9 : 0);
    MeshRay r;
    load_ray(p, ray, r);
    const bool live = valid && !dead_ray(r);
    float best_t = INFINITY;
    int best_f = INT_MAX;
#pragma unroll 1
    for (int f0 = 0; f0 < p.F; f0 += kMeshTile) {                           // block-uniform trip count: the barriers are met by all
        const int n = min(kMeshTile, p.F - f0);
        __syncthreads();                                                    // the previous tile has been read
        for (int i = tid; i < n * 9; i += 256) tile[i] = tri_b[(size_t)f0 * 9 + i];
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int j = 0; j < n; ++j) keep(intersect(r, tile + j * 9), f0 + j, best_t, best_f);
        }
    }
    if (valid) finish(p, ray, r, tri_b, best_f);
}

__device__ __forceinline__ float plane_at(int i, float lo, float cell) { return lo + (float)i * cell; }

__global__ void __launch_bounds__(256) trace_mesh_grid_kernel(const MeshParams p) {
    const long long ray_ll = (long long)blockIdx.x * 256 + threadIdx.x;
    if (ray_ll >= (long long)p.B * p.R) return;                             // (no barrier in this kernel)
    const size_t ray = (size_t)ray_ll;
    const int G = p.G;
    const size_t frame = p.per_frame ? (size_t)(ray_ll / p.R) : 0;
    const float* __restrict__ tri_b = p.tri + frame * p.F * 9;
    const int* __restrict__ cs = p.cell_start + frame * ((size_t)G * G * G + 1);
    const float* __restrict__ box = p.box + frame * 6;
    MeshRay r;
    load_ray(p, ray, r);
    float best_t = INFINITY;
    int best_f = INT_MAX;
    if (!dead_ray(r)) {
        // ---- the box's own slabs: does the ray meet the grid, and where does it enter
        float lo[3], cell[3], inv[3], t_out[3];
        int step[3], idx[3];
        bool miss = false, every = false;                                   // every: test all faces (nothing below can be trusted)
        float enter = -INFINITY, leave = INFINITY;
        int crossed = -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = box[k];
            cell[k] = box[3 + k];
            const float dk = r.d[k], ok = r.o[k];
            if (!(fabsf(dk) < INFINITY) || !(fabsf(ok) < INFINITY)) every = true;
            inv[k] = __fdiv_rn(1.f, dk);
            step[k] = dk > 0.f ? 1 : dk < 0.f ? -1 : 0;
            const float p0 = plane_at(0, lo[k], cell[k]), p1 = plane_at(G, lo[k], cell[k]);
            if (step[k] == 0) {
                if (!(ok >= p0 && ok <= p1)) miss = true;                  // parallel to the slab and outside it
                continue;
            }
            const float ta = (p0 - ok) * inv[k], tb = (p1 - ok) * inv[k];
            const float a_in = step[k] > 0 ? ta : tb, a_out = step[k] > 0 ? tb : ta;
            if (a_in != a_in || a_out != a_out) every = true;
            if (a_in > enter) { enter = a_in; crossed = k; }
            leave = fminf(leave, a_out);
        }
        const bool outside = enter > r.tn;                                  // the box is entered after t_near
        const float t0 = outside ? enter : r.tn;
        if (!(fabsf(t0) < INFINITY)) every = true;
        if (every) {
            // bounded by F; the brute-force kernel's loop on this lane alone
            for (int f = 0; f < p.F; ++f) keep(intersect(r, tri_b + (size_t)f * 9), f, best_t, best_f);
        } else if (!miss && fminf(leave, r.tf) >= t0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                int i;
                if (outside && k == crossed) {
                    i = step[k] > 0 ? 0 : G - 1;                            // by construction, not the floor of a rounded position
                } else {
                    const float pk = r.o[k] + t0 * r.d[k];
                    const float f = fminf(fmaxf(floorf(__fdiv_rn(pk - lo[k], cell[k])), 0.f), (float)(G - 1));      // (NaN -> 0)
                    i = (int)f;
                    for (int fix = 0; fix < 2; ++fix) {                     // the floor, held to the kernel's own planes
                        if (i > 0 && pk < plane_at(i, lo[k], cell[k])) --i;
                        else if (i < G - 1 && pk >= plane_at(i + 1, lo[k], cell[k])) ++i;
                    }
                }
                idx[k] = i;
                t_out[k] = step[k] == 0 ? INFINITY : (plane_at(i + (step[k] > 0 ? 1 : 0), lo[k], cell[k]) - r.o[k]) * inv[k];
            }
            const int max_steps = 3 * G + 3;                                // HARD bound: at most 3 (G - 1) + 1 cells lie on a ray
#pragma unroll 1
            for (int it = 0; it < max_steps; ++it) {
                const size_t c = ((size_t)idx[0] * G + idx[1]) * G + idx[2];
                const int s = max(cs[c], 0), e = min(cs[c + 1], p.n_pairs);
#pragma unroll 1
                for (int j = s; j < e; ++j) {
                    const int f = min(max(p.cell_faces[j], 0), p.F - 1);
                    keep(intersect(r, tri_b + (size_t)f * 9), f, best_t, best_f);
                }
                int a = 0;                                                  // the axis whose exit plane comes first (ties: x, y, z)
                float first = t_out[0];
                if (t_out[1] < first) { first = t_out[1]; a = 1; }
                if (t_out[2] < first) { first = t_out[2]; a = 2; }
                if (best_t < first) break;                                  // nothing beyond this cell can come before the best
                if (!(first <= r.tf)) break;                                // the next cell begins past t_far (or at a NaN)
                bool out = false;
                // (a is written out per axis: dynamic indexing of the small arrays would put them in scratch)
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (k != a) continue;
                    if (step[k] == 0) { out = true; continue; }
                    idx[k] += step[k];
                    if (idx[k] < 0 || idx[k] >= G) { out = true; continue; }
                    t_out[k] = (plane_at(idx[k] + (step[k] > 0 ? 1 : 0), lo[k], cell[k]) - r.o[k]) * inv[k];
                }
                if (out) break;
            }
        }
    }
    finish(p, ray, r, tri_b, best_f);
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_trace_mesh(const HfagpTraceMeshArgs* q, void* stream) {
    HFAGP_REQUIRE(q, HFAGP_EBADARG, "trace_mesh: null pointer");
    HFAGP_REQUIRE(q->B >= 0 && q->R >= 0 && q->F >= 0 && q->n_pairs >= 0, HFAGP_EBADARG,
                  "trace_mesh: negative count B=%d R=%lld F=%d n_pairs=%lld", q->B, (long long)q->R, q->F, (long long)q->n_pairs);
    HFAGP_REQUIRE(q->ray_origins && q->ray_directions && q->t_near && q->t_far && (q->tri || q->F == 0), HFAGP_EBADARG,
                  "trace_mesh: null pointer");
    HFAGP_REQUIRE(q->hit || q->face || q->t || q->bary || q->point || q->normal || q->front, HFAGP_EBADARG,
                  "trace_mesh: null pointer (pass at least one output)");
    HFAGP_REQUIRE(q->tri_frames == 1 || q->tri_frames == q->B, HFAGP_EBADARG, "trace_mesh: tri_frames = %d (1 or B = %d)",
                  q->tri_frames, q->B);
    const bool any_grid = q->cell_start || q->cell_faces || q->grid_box, grid = q->cell_start && q->cell_faces && q->grid_box;
    HFAGP_REQUIRE(!any_grid || grid, HFAGP_EBADARG, "trace_mesh: cell_start, cell_faces and grid_box go together");
    HFAGP_REQUIRE(!grid || (q->G >= 1 && q->G <= 256), HFAGP_EBADARG, "trace_mesh: G = %d (1 .. 256)", q->G);
    HFAGP_REQUIRE(q->n_pairs < (1ll << 31), HFAGP_EBADARG, "trace_mesh: n_pairs = %lld (< 2^31)", (long long)q->n_pairs);
    HFAGP_REQUIRE((long long)q->B * ((q->R + 255) / 256 * 256) < (1ll << 31), HFAGP_EUNSUPPORTED, "trace_mesh: too many rays");
    if (q->B == 0 || q->R == 0) return HFAGP_OK;
    MeshParams p = {};
    p.tri = q->tri;
    p.ray_o = q->ray_origins; p.ray_d = q->ray_directions;
    p.t_near = q->t_near; p.t_far = q->t_far;
    p.cell_start = q->cell_start; p.cell_faces = q->cell_faces; p.box = q->grid_box;
    p.hit = q->hit; p.front = q->front; p.face = q->face;
    p.t = q->t; p.bary = q->bary; p.point = q->point; p.normal = q->normal;
    p.B = q->B; p.R = (int)q->R; p.F = q->F; p.G = q->G;
    p.per_frame = q->tri_frames == q->B && q->B > 1 ? 1 : 0;
    p.n_pairs = (int)q->n_pairs;
    p.tiles_per_b = (int)((q->R + 255) / 256);
    hipStream_t s = (hipStream_t)stream;
    if (grid && q->F > 0) {
        const unsigned blocks = (unsigned)(((long long)q->B * q->R + 255) / 256);
        trace_mesh_grid_kernel<<<blocks, 256, 0, s>>>(p);
    } else {
        trace_mesh_brute_kernel<<<(unsigned)(p.tiles_per_b * q->B), 256, 0, s>>>(p);
    }
    return check_launch("trace_mesh");
}
