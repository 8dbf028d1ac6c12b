// The ray marcher on caller-given ray lists (hfagp.h HfagpRayListArgs): the entry points.  The kernels are the list instantiations
// of the grid's — raymarch_rays_kernel (raymarch.hip), raymarch_bwd_tiles_kernel / raymarch_bwd_df_kernel <.., LIST>
// (raymarch_bwd.hip), raymarch_bwd_bins_kernel <.., LIST> (raymarch_rows.hip), raymarch_bwd_rays_kernel (raymarch_camera.hip) — which
// differ from them in the ray fetch alone (raymarch_common.h ray_fetch).  Here: argument checks and the hand-over to the launchers
// those units share with their grid entry points.  (The normals of a list — hfagp_raymarch_rays_normals / _normals_bwd /
// _normals_bwd_rays — have their entry points next to their kernels, in raymarch_normals.hip, raymarch_normals_bwd.hip and
// raymarch_normals_camera.hip, compiled by raymarch_rays_normals.hip.)
#include "raymarch_common.h"

using namespace hfagp;

extern "C" int hfagp_raymarch_rays_fwd(const HfagpRayListArgs* a, void* stream) {
    HFAGP_REQUIRE(a, HFAGP_EBADARG, "raymarch_rays_fwd: null pointer");
    const HfagpRaymarchArgs* f = &a->base;
    HFAGP_REQUIRE(f->feat && f->depth && f->wsum && f->tminmax, HFAGP_EBADARG, "raymarch_rays_fwd: null pointer");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(f, p, "raymarch_rays_fwd", &rays);
    if (rc != HFAGP_OK) return rc;
    return launch_raymarch(p, false, (hipStream_t)stream);
}

extern "C" int hfagp_raymarch_rays_bwd(const HfagpRayListBwdArgs* a, const HfagpRaymarchGeomGrads* geom, void* stream) {
    HFAGP_REQUIRE(a && a->bwd.d_planes && a->bwd.rec, HFAGP_EBADARG, "raymarch_rays_bwd: null pointer");
    const float* g_depth = geom ? geom->g_depth : nullptr;
    const float* g_wsum = geom ? geom->g_wsum : nullptr;
    HFAGP_REQUIRE(a->bwd.g_feat || g_depth || g_wsum, HFAGP_EBADARG,
                  "raymarch_rays_bwd: no upstream gradient (g_feat, g_depth and g_wsum are all null)");
    HFAGP_REQUIRE(!g_depth || geom->depth_range, HFAGP_EBADARG, "raymarch_rays_bwd: g_depth needs depth_range");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->bwd.fwd, p, "raymarch_rays_bwd", &rays);
    if (rc != HFAGP_OK) return rc;
    return raymarch_bwd_run(&a->bwd, p, geom, (hipStream_t)stream);
}

extern "C" size_t hfagp_raymarch_rays_bwd_rows_bytes(const HfagpRayListArgs* a) {
    if (!a || a->base.B <= 0 || a->base.H <= 1 || a->base.W <= 1 || a->R <= 0) return 0;
    if ((long long)a->base.B * a->R >= (1ll << 31)) return 0;
    return rows_scratch_bytes(a->base, a->R);
}

extern "C" int hfagp_raymarch_rays_bwd_rays(const HfagpRayListBwdArgs* a, float* d_origins, float* d_directions, void* stream) {
    HFAGP_REQUIRE(a && a->bwd.rec && d_origins && d_directions, HFAGP_EBADARG, "raymarch_rays_bwd_rays: null pointer");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->bwd.fwd, p, "raymarch_rays_bwd_rays", &rays);
    if (rc != HFAGP_OK) return rc;
    p.g_feat = a->bwd.g_feat;
    p.rec = a->bwd.rec;
    return launch_ray_list_grads(p, d_origins, d_directions, (hipStream_t)stream);
}

// ---- the same three with per-ray depth limits (hfagp.h HfagpRayLimits): the limits reach the list instantiations of raymarch_body
// (the forward and pass 1 of the backward) through RayParams::t_near / t_far; pass 2 and the rays' pass read the depths from the
// records and need none.  base.ray_start / ray_end are neither read nor checked.
extern "C" int hfagp_raymarch_rays_limits_fwd(const HfagpRayListArgs* a, const HfagpRayLimits* lim, void* stream) {
    HFAGP_REQUIRE(lim && lim->t_near && lim->t_far, HFAGP_EBADARG, "raymarch_rays_limits_fwd: null pointer (limits)");
    HFAGP_REQUIRE(a, HFAGP_EBADARG, "raymarch_rays_limits_fwd: null pointer");
    const HfagpRaymarchArgs* f = &a->base;
    HFAGP_REQUIRE(f->feat && f->depth && f->wsum && f->tminmax, HFAGP_EBADARG, "raymarch_rays_limits_fwd: null pointer");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(f, p, "raymarch_rays_limits_fwd", &rays, true);
    if (rc != HFAGP_OK) return rc;
    p.t_near = lim->t_near;
    p.t_far = lim->t_far;
    return launch_raymarch(p, false, (hipStream_t)stream);
}

extern "C" int hfagp_raymarch_rays_limits_bwd(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim,
                                              const HfagpRaymarchGeomGrads* geom, void* stream) {
    HFAGP_REQUIRE(lim && lim->t_near && lim->t_far, HFAGP_EBADARG, "raymarch_rays_limits_bwd: null pointer (limits)");
    HFAGP_REQUIRE(a && a->bwd.d_planes && a->bwd.rec, HFAGP_EBADARG, "raymarch_rays_limits_bwd: null pointer");
    const float* g_depth = geom ? geom->g_depth : nullptr;
    const float* g_wsum = geom ? geom->g_wsum : nullptr;
    HFAGP_REQUIRE(a->bwd.g_feat || g_depth || g_wsum, HFAGP_EBADARG,
                  "raymarch_rays_limits_bwd: no upstream gradient (g_feat, g_depth and g_wsum are all null)");
    HFAGP_REQUIRE(!g_depth || geom->depth_range, HFAGP_EBADARG, "raymarch_rays_limits_bwd: g_depth needs depth_range");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->bwd.fwd, p, "raymarch_rays_limits_bwd", &rays, true);
    if (rc != HFAGP_OK) return rc;
    p.t_near = lim->t_near;
    p.t_far = lim->t_far;
    return raymarch_bwd_run(&a->bwd, p, geom, (hipStream_t)stream);
}

extern "C" int hfagp_raymarch_rays_limits_bwd_rays(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim, float* d_origins,
                                                   float* d_directions, void* stream) {
    HFAGP_REQUIRE(lim && lim->t_near && lim->t_far, HFAGP_EBADARG, "raymarch_rays_limits_bwd_rays: null pointer (limits)");
    HFAGP_REQUIRE(a && a->bwd.rec && d_origins && d_directions, HFAGP_EBADARG, "raymarch_rays_limits_bwd_rays: null pointer");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->bwd.fwd, p, "raymarch_rays_limits_bwd_rays", &rays, true);
    if (rc != HFAGP_OK) return rc;
    p.g_feat = a->bwd.g_feat;
    p.rec = a->bwd.rec;
    p.t_near = lim->t_near;          // (not read: the depths of the records are the limits' already)
    p.t_far = lim->t_far;
    return launch_ray_list_grads(p, d_origins, d_directions, (hipStream_t)stream);
}

// ---- per-sample compositing weights (hfagp.h HfagpRaySamples): the forward with two more outputs, the backward with one more
// addend in pass 1's adjoint (RayParams::samples_w / samples_t / g_weights, raymarch.hip), with or without per-ray limits.  Pass 2
// and the rays' pass (hfagp_raymarch_rays_bwd_rays / _limits_bwd_rays above) read the records, into which the term is folded.
extern "C" int hfagp_raymarch_rays_samples_fwd(const HfagpRayListArgs* a, const HfagpRayLimits* lim, const HfagpRaySamples* out,
                                               void* stream) {
    HFAGP_REQUIRE(!lim || (lim->t_near && lim->t_far), HFAGP_EBADARG, "raymarch_rays_samples_fwd: null pointer (limits)");
    HFAGP_REQUIRE(out && out->weights && out->depths, HFAGP_EBADARG, "raymarch_rays_samples_fwd: null pointer (samples)");
    HFAGP_REQUIRE(a, HFAGP_EBADARG, "raymarch_rays_samples_fwd: null pointer");
    const HfagpRaymarchArgs* f = &a->base;
    HFAGP_REQUIRE(f->feat && f->depth && f->wsum && f->tminmax, HFAGP_EBADARG, "raymarch_rays_samples_fwd: null pointer");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(f, p, "raymarch_rays_samples_fwd", &rays, lim != nullptr);
    if (rc != HFAGP_OK) return rc;
    if (lim) { p.t_near = lim->t_near; p.t_far = lim->t_far; }
    p.samples_w = out->weights;
    p.samples_t = out->depths;
    return launch_raymarch(p, false, (hipStream_t)stream);
}

extern "C" int hfagp_raymarch_rays_samples_bwd(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim,
                                               const HfagpRaymarchGeomGrads* geom, const float* g_weights, void* stream) {
    HFAGP_REQUIRE(!lim || (lim->t_near && lim->t_far), HFAGP_EBADARG, "raymarch_rays_samples_bwd: null pointer (limits)");
    HFAGP_REQUIRE(g_weights, HFAGP_EBADARG, "raymarch_rays_samples_bwd: null pointer (g_weights)");
    HFAGP_REQUIRE(a && a->bwd.d_planes && a->bwd.rec, HFAGP_EBADARG, "raymarch_rays_samples_bwd: null pointer");
    HFAGP_REQUIRE(!(geom && geom->g_depth) || geom->depth_range, HFAGP_EBADARG, "raymarch_rays_samples_bwd: g_depth needs depth_range");
    const RayList rays{a->ray_origins, a->ray_directions, a->R};
    RayParams p;
    const int rc = fill_ray_params(&a->bwd.fwd, p, "raymarch_rays_samples_bwd", &rays, lim != nullptr);
    if (rc != HFAGP_OK) return rc;
    if (lim) { p.t_near = lim->t_near; p.t_far = lim->t_far; }
    p.g_weights = g_weights;          // (g_feat, g_depth and g_wsum may all be null: this gradient alone is an upstream gradient)
    return raymarch_bwd_run(&a->bwd, p, geom, (hipStream_t)stream);
}
