// Ray–box depth limits for a ray list (hfagp_ray_limits_box): the [t_near, t_far] of every ray against the cube
// [-box_side/2, box_side/2]^3 the tri-planes cover — EG3D's ray_start == ray_end == 'auto' (math_utils.get_ray_limits_box) as the
// input of hfagp_raymarch_rays_limits_* (raymarch_rays.hip).
//
// Slab method, every operation rounded on its own (cam_utils.ray_limits_box is the same formula in torch and the reference):
//   per axis k:  inv = 1 / d_k (IEEE: +-inf for a zero component),  t0 = (-h - o_k) * inv,  t1 = (h - o_k) * inv
//   near = max_k min(t0, t1), clamped below at 0;   far = min_k max(t0, t1)
// A ray misses the box iff far <= near (the list kernels treat it as EMPTY).  0 * inf — the origin exactly on a slab of an axis the
// ray is parallel to — is NaN and makes BOTH limits NaN (fminf / fmaxf would drop it): the ray is empty as well.
// The clamp at 0 diverges from EG3D on purpose: an origin inside the box starts at the origin, which is what a shadow ray needs.
// One thread per ray, three 4-byte loads per vector, plain vector stores.
#include "common.h"

namespace hfagp {

__global__ void __launch_bounds__(256) ray_limits_box_kernel(const float* __restrict__ o, const float* __restrict__ d,
                                                            float* __restrict__ t_near, float* __restrict__ t_far, long long n,
                                                            float half) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float near = -INFINITY, far = INFINITY;
    bool nan = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float ok = o[i * 3 + k], dk = d[i * 3 + k];
        const float inv = __fdiv_rn(1.f, dk);
        const float t0 = __fmul_rn(__fsub_rn(-half, ok), inv), t1 = __fmul_rn(__fsub_rn(half, ok), inv);
        nan = nan || t0 != t0 || t1 != t1;
        near = fmaxf(near, fminf(t0, t1));
        far = fminf(far, fmaxf(t0, t1));
    }
    near = fmaxf(near, 0.f);
    if (nan) near = far = __int_as_float(0x7fc00000);
    t_near[i] = near;
    t_far[i] = far;
}

}  // namespace hfagp

using namespace hfagp;

extern "C" int hfagp_ray_limits_box(const float* ray_origins, const float* ray_directions, float* t_near, float* t_far,
                                    int64_t n_rays, float box_side, void* stream) {
    HFAGP_REQUIRE(ray_origins && ray_directions && t_near && t_far, HFAGP_EBADARG, "ray_limits_box: null pointer");
    HFAGP_REQUIRE(n_rays > 0 && n_rays < (1ll << 31), HFAGP_EBADARG, "ray_limits_box: n_rays = %lld", (long long)n_rays);
    HFAGP_REQUIRE(box_side > 0.f && box_side < INFINITY, HFAGP_EBADARG, "ray_limits_box: box_side = %g", (double)box_side);
    const unsigned blocks = (unsigned)((n_rays + 255) / 256);
    ray_limits_box_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(ray_origins, ray_directions, t_near, t_far, (long long)n_rays,
                                                                  box_side * 0.5f);
    return check_launch("ray_limits_box");
}
