/*
 * hfagp.h — C ABI of libhfagp_hip.so: the MI355X (gfx950) implementation of the
 * EG3D tri-plane generator hot path that HFA-GP calls as
 *   generator.synthesis(ws, c=label, noise_mode='const')['image']
 * (/root/reference/code/networks/headnerf.py:112,118,133,207,218,267,277).
 *
 * The reference has no FFI of its own (it is pure Python).  The
 * interfaces these entry points replace are the EG3D operator API one level
 * below that call (NVlabs/eg3d, not shipped in the reference tree):
 *   hfagp_raymarch_fwd      <- ImportanceRenderer.forward + RaySampler + OSGDecoder + MipRayMarcher2
 *   hfagp_modconv_fwd       <- modulated_conv2d(...) + bias_act(...) (SynthesisLayer / ToRGBLayer)
 *   hfagp_style_fwd         <- FullyConnectedLayer affine + demodulation coefficients
 *   hfagp_upfir_epilogue_fwd<- upfirdn2d(pad [1,1,1,1], gain 4) after the transposed conv + bias_act
 *   hfagp_upfirdn2d_fwd     <- upfirdn2d.upfirdn2d(x, f, up, down, padding, gain)
 *                              (in-repo twin: upfirdn2d_native, code/networks/encoder3d.py:23-45)
 *   hfagp_bias_act_fwd      <- bias_act.bias_act(x, b, act, alpha, gain, clamp)
 *                              (in-repo twin: fused_leaky_relu, code/networks/encoder3d.py:7-8)
 *   hfagp_torgb_fwd         <- ToRGBLayer for img_channels=3 + upsample2d(img) skip add
 *   hfagp_skip_upsample_add <- img = upsample2d(img, resample_filter) + y   (SynthesisBlock 'skip')
 *   hfagp_torgb_skip_fwd    <- ToRGBLayer (96 tri-plane channels) + the skip add, one streaming pass
 *   hfagp_torgb_finish_fwd  <- bias + clamp + skip add of a 3-channel ToRGBLayer whose sums rode in the conv's epilogue
 *   hfagp_upconv_fir_fwd    <- conv2d_resample(up=2) + bias_act of a SynthesisLayer in one pass (+ _scratch_bytes)
 *   hfagp_style_batch_fwd   <- the affine + demodulation of EVERY layer of one synthesis() call, one launch
 *   hfagp_fc_fwd            <- FullyConnectedLayer (MappingNetwork; EqualLinear twin: code/networks/encoder3d.py:112-139)
 *   hfagp_weight_prep[_split|_prec] <- (no reference counterpart: MFMA operand images of a conv weight, per weight version)
 *   hfagp_qr_gram_fwd / hfagp_qr_refine_fwd <- torch.qr(bases.T) of get_latent (code/networks/headnerf.py:91,187,246)
 *   hfagp_planes_query      <- TriPlaneGenerator.sample / sample_mixed (sample_from_planes + OSGDecoder at given points) and the
 *                              density volume of gen_samples.py --shapes (create_samples lattice), one launch (ABI 13)
 *   hfagp_planes_query_normals[_bwd] <- (no reference counterpart: autograd of sample_mixed's sigma w.r.t. the points, i.e. the
 *                              density gradient and surface normal at a point, and what a loss on them back-propagates)
 *   hfagp_trace_rays        <- (no reference counterpart: the first hit of a ray list with the density iso-surface that marching
 *                              cubes exports — t, point, density gradient and normal per ray)
 *   hfagp_trace_mesh        <- (no reference counterpart: the first hit of a ray list with a triangle mesh — face, t, barycentric
 *                              weights, point and geometric normal per ray; brute force or through a uniform grid of face lists)
 *   hfagp_marching_cubes_count / _emit (+ _workspace_bytes) <- the .ply mesh of gen_samples.py --shapes
 *                              (skimage.measure.marching_cubes + plyfile in EG3D's shape_utils), on the GPU (ABI 14)
 *   hfagp_raymarch_normals  <- (no reference counterpart: the per-ray surface normal map of EG3D-family geometry renders — the
 *                              density gradient of every sample composited with MipRayMarcher2's weights)
 *   hfagp_raymarch_normals_bwd <- (none either: what autograd would do with a normal-map loss on such a render)
 *   hfagp_raymarch_normals_bwd_camera <- (none either: the same loss's gradient w.r.t. the camera label)
 *   hfagp_raymarch_rays_normals / _normals_bwd / _normals_bwd_rays <- (none either: the three above on explicit ray lists, with
 *                              optional per-ray depth limits)
 *   hfagp_depth_clamp       <- MipRayMarcher2's torch.clamp(depth, min sample depth, max sample depth) over the batch, one launch (ABI 10)
 *   hfagp_resize_aa_fwd / _bwd <- SuperresolutionHybrid8XDC.forward's antialiased bilinear F.interpolate of rgb and x to its input
 *                              resolution (synthesis(neural_rendering_resolution=N), N != the configured one) and its autograd
 *   hfagp_planes_to_nhwc    <- planes.view(N, 3, 32, H, W) of TriPlaneGenerator.synthesis (layout change for the gather)
 *   hfagp_planes_sum_to_nhwc <- (no reference counterpart: the same layout change with autograd's sum over the V frames that
 *                              share one identity's planes in front of it — synthesis(ws [B], c [B,V,25]))
 *   hfagp_nchw_to_nhwc / hfagp_nhwc_to_nchw <- tensor layout at the module boundary (reference tensors are NCHW)
 *   hfagp_pool_mse_fwd/_bwd <- face_pool (AdaptiveAvgPool2d) + MSELoss of gen_update (code/trainer_rgb.py:63,84-85) and its backward
 *   hfagp_pool_wmse_fwd/_bwd <- the same under a per-pixel weight, normalised per frame: the unused `mask=None` slot of gen_update
 *                              (code/trainer_rgb.py:73)
 *   hfagp_blur_down_fwd/_bwd<- Blur + stride-2 sampling in front of the ResBlock skip (code/networks/encoder3d.py:59-73,142-199)
 *   hfagp_allreduce_f32     <- the gradient all-reduce DistributedDataParallel does for the reference
 *                              (code/trainer_rgb.py:56, code/trainer_3dmm.py:29, code/trainer_audio.py:30-34; NCCL group: code/train_rgb.py:57)
 * backward (the reference gets these from torch.autograd through EG3D's custom ops; g_loss.backward(), code/trainer_rgb.py:93):
 *   hfagp_raymarch_bwd      <- autograd of the renderer: grid_sample / decoder / compositing adjoints
 *   hfagp_raymarch_bwd_geom <- the same with gradients of the expected depth and the opacity (silhouette / depth losses)
 *   hfagp_raymarch_bwd_camera <- autograd of RaySampler + grid_sample w.r.t. the sample positions: the gradient of the camera label
 *   hfagp_raymarch_rays_fwd / _rays_bwd / _rays_bwd_rays <- ImportanceRenderer.forward on explicit (ray_origins, ray_directions) and
 *                              its autograd w.r.t. planes, decoder and the rays (crops, multi-view lists, arbitrary camera models)
 *   hfagp_raymarch_rays_limits_fwd / _limits_bwd / _limits_bwd_rays, hfagp_ray_limits_box <- the same with per-ray depth limits:
 *                              ImportanceRenderer.forward with ray_start == ray_end == 'auto' (math_utils.get_ray_limits_box)
 *   hfagp_raymarch_rays_samples_fwd / _samples_bwd <- MipRayMarcher2's `weights` and the sorted depths of unify_samples, which
 *                              ImportanceRenderer.forward drops, as outputs of the list renderer, and autograd through the weights
 *   hfagp_planes_query_bwd  <- autograd of sample_mixed (grid_sample + OSGDecoder at given points) w.r.t. planes, decoder and points
 *   hfagp_modconv_fwd modes HFAGP_CONV3X3_BWD / HFAGP_CONVS2_BWD <- conv2d_gradfix data gradients (the same GEMM kernel)
 *   hfagp_conv_wgrad (+ _workspace_bytes) <- conv2d_gradfix weight gradients
 *   hfagp_pointwise_bwd     <- bias_act backward + noise-strength / bias gradients + demodulation adjoint of a SynthesisLayer
 *   hfagp_upfir_bwd, hfagp_upsample2d_bwd, hfagp_upfirdn2d_bwd, hfagp_bias_act_bwd <- upfirdn2d / bias_act backward
 *   hfagp_style_bwd / hfagp_style_batch_bwd, hfagp_affine_grad, hfagp_channel_sum <- affine / demodulation / bias gradients
 *
 * Contract:
 *   - plain pointers and sizes only; all pointers are DEVICE pointers owned by the caller;
 *     the library never allocates, frees or retains them past the call;
 *   - all work is enqueued asynchronously on the hipStream_t passed in (void* here so that
 *     callers need no HIP headers); no internal synchronisation;
 *   - return 0 on success, <0 on error: -1 bad arguments, -2 unsupported shape/dtype,
 *     -3 HIP launch failure; hfagp_last_error() returns a thread-local message;
 *   - never aborts, never throws across the boundary.
 *
 * Activation layout inside the path is channels-last fp32:  x[b][y][x][c].
 * The tri-plane volume is plane-major channels-last:        planes[b][plane][y][x][32].
 */
#ifndef HFAGP_H_
#define HFAGP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HFAGP_ABI_VERSION 15

enum { HFAGP_OK = 0, HFAGP_EBADARG = -1, HFAGP_EUNSUPPORTED = -2, HFAGP_ELAUNCH = -3 };

int hfagp_abi_version(void);
const char* hfagp_last_error(void);

/* ------------------------------------------------------------------ ray march
 * One launch: ray generation -> stratified depths -> tri-plane bilinear gather
 * -> decoder MLP -> coarse compositing -> importance re-sampling -> second
 * gather+MLP -> depth merge -> final compositing.                              */
#define HFAGP_RAYMARCH_STATE_FLOATS_PER_SAMPLE 35   /* HfagpRaymarchArgs::state: 32 colours, depth, density, sort index */

typedef struct {
    const float* planes;      /* [B][3][H][W][32] fp32                                        */
    const float* cam2world;   /* [B][16] row-major 4x4 (label[:, :16])                        */
    const float* intrinsics;  /* [B][9]  row-major 3x3 (label[:, 16:25])                      */
    const float* u_strat;     /* [B][R][Sc]  uniforms of the stratified jitter                */
    const float* u_imp;       /* [B][R][Sf]  uniforms of the inverse-CDF draw                 */
    const float* dec_w0;      /* decoder.net.0.weight [64][32]  (raw parameter)               */
    const float* dec_b0;      /* decoder.net.0.bias   [64]                                    */
    const float* dec_w1;      /* decoder.net.2.weight [33][64]                                */
    const float* dec_b1;      /* decoder.net.2.bias   [33]                                    */
    float*       feat;        /* out [B][R][32]  composited features, scaled to (-1,1)        */
    float*       depth;       /* out [B][R]      expected depth, NaN->inf, NOT yet clamped    */
    float*       wsum;        /* out [B][R]      sum of weights                               */
    float*       tminmax;     /* out [B][R][2]   per-ray min / max sample depth               */
    int32_t B, H, W;          /* plane height/width                                           */
    int32_t res;              /* rays per side; R = res*res                                   */
    int32_t Sc, Sf;           /* coarse / importance samples per ray: 16,32 or 48 each        */
    int32_t plane_axes;       /* 0: (x,y),(x,z),(z,x) [eg3d original]; 1: third = (z,y)       */
    int32_t white_back;
    double ray_start, ray_end;/* python floats of rendering_kwargs (kept double: linspace/delta rounding) */
    float box_warp, decoder_lr_mul;
    /* optional: HFAGP_ABSMAX_FLOATS floats (64 slots, HFAGP_ABSMAX_STRIDE apart) whose maximum bounds |planes| (published by the kernel that wrote the planes,
     * hfagp_skip_upsample_add, or any upper bound).  With it the decoder MLP runs on the 16-bit matrix pipe with split
     * operands (fp16 hi + lo parts, 3 MFMAs per product as HFAGP_PREC_F16X3: ~2^-22, fp32-class; gradients: bf16 parts),
     * every operand scaled into fp16's range by an exact power of two derived from this bound and the weights.
     * NULL: the decoder runs on the exact fp32 matrix instructions (5x the matrix-pipe time).                      */
    const float* planes_absmax;
    /* optional [B][R][(Sc + Sf) * HFAGP_RAYMARCH_STATE_FLOATS_PER_SAMPLE] floats: in hfagp_raymarch_fwd the per-sample colours,
     * densities, depths and sort order of every ray are LEFT here (13.4 KB per ray at 48+48 samples); hfagp_raymarch_bwd
     * given the same buffer (fwd.state) reads them instead of gathering and decoding every sample again for the
     * compositing adjoint.  NULL: nothing is saved / everything is recomputed.                                       */
    float*       state;
} HfagpRaymarchArgs;

int hfagp_raymarch_fwd(const HfagpRaymarchArgs* a, void* stream);

/* Per-ray surface normals (additive to ABI 15).  After hfagp_raymarch_fwd on the same arguments and stream with fwd->state given:
 * the sorted sample depths and densities are read from the state (the output pointers of `fwd` are not touched).  Per sample
 *   g = d sigma / d x   the WORLD-space gradient of the raw decoder density (channel 0 of the decoder, before softplus(sigma - 1))
 *                       of the function the forward evaluated: plane mean of the three bilinear gathers, zeros padding,
 *                       align_corners = False; the 2 / box_warp factor and the routing of plane_axes included
 *   n = -g * rsqrt(g.g + 1e-12)   the unit normal from dense to empty; exactly 0 where g is exactly 0 (outside every plane)
 * and per ray  normal[b][r][0..2] = sum_s omega_s n_s  over the Sc + Sf samples of the final depth-sorted pass with the colour
 * weights of the forward, omega = (w_{r-1} + w_r) / 2 at sorted position r (MipRayMarcher2's midpoint rule with the normals as
 * colours, before its * 2 - 1).  |normal| <= wsum; not normalised; white_back does not enter.  Decoder arithmetic as the forward:
 * split 16-bit operands given planes_absmax (gradient products: bf16 parts), exact fp32 without it.  One writer per ray, no
 * atomics: two calls give the same bits.  Its backward is hfagp_raymarch_normals_bwd.
 * HFAGP_EBADARG, nothing launched: fwd, normal, fwd->state or fwd->planes NULL (then the checks of hfagp_raymarch_fwd on the
 * inputs); HFAGP_EUNSUPPORTED: sample counts the forward does not support.                                                    */
int hfagp_raymarch_normals(const HfagpRaymarchArgs* fwd, float* normal /* [B][R][3] */, void* stream);

/* Backward of hfagp_raymarch_normals (additive to ABI 15): from g_normal = dL/d normal to the plane gradient and the decoder-
 * parameter gradients, one launch, same arguments and state as the forward call.  With F the 32 gathered features of a sample at
 * q = (2 / box_warp) x, hp = W0' F + b0' (the lr_mul gains folded in as in the forward), sigma = wsig . softplus(hp) + bsig,
 * a = d sigma / dF = W0'^T (wsig * sigmoid(hp)), J = dF / dq, g = (2 / box_warp) J^T a, r = sqrt(g.g + 1e-12), n = -g / r:
 *   through the weights   G_e = g_normal . (n_e + n_{e+1}) / 2 is dL/dw_e of the midpoint weights (the normals are three colours
 *                         of the compositing, no * 2 - 1, no white_back); the compositing adjoint of hfagp_raymarch_bwd gives
 *                         d sigma_s of the raw densities.  The sample depths carry no gradient.
 *   through the normals   gamma = dL/dg_s = -(omega_s / r)(g_normal - n (n . g_normal)); per tap k of every plane, with w_k its
 *                         bilinear weight, w'_k = (2 / box_warp) gamma . grad_q w_k (0 for a tap outside the plane),
 *                         u = sum_planes sum_k texel w'_k / 3,  v = W0' u,  e = wsig * sigmoid(hp) * (1 - sigmoid(hp)) * v,
 *                         dF = a d sigma_s + W0'^T e.
 *   d_planes    += (w_k / 3) dF + (w'_k / 3) a at every tap, all three planes at their true texels (fp32 atomics): on mirrored
 *                  planes call it AFTER hfagp_raymarch_bwd on the same buffer, which overwrites plane 2.
 *   d_dec_w0    += [(d sigma_s dH + e) F^T + dH u^T] * gain, dH = wsig * sigmoid(hp);   d_dec_b0 += (d sigma_s dH + e) * gain;
 *   d_dec_w1[0] += [d sigma_s softplus(hp) + sigmoid(hp) * v] * gain;   d_dec_b1[0] += d sigma_s * gain; the colour rows get
 *                  nothing.  The four go together (all or none); gains as hfagp_raymarch_bwd.
 * The second-order products run on the exact fp32 matrix instructions with either decoder.  A ray whose g_normal is exactly 0
 * touches nothing.  HFAGP_EBADARG, nothing launched: fwd, fwd->state, fwd->planes, g_normal or d_planes NULL, or only some of the
 * four decoder outputs given (then the checks of hfagp_raymarch_fwd); HFAGP_EUNSUPPORTED: sample counts.                       */
int hfagp_raymarch_normals_bwd(const HfagpRaymarchArgs* fwd, const float* g_normal /* [B][R][3] */,
                               float* d_planes /* [B][3][H][W][32], accumulated into */,
                               float* d_dec_w0, float* d_dec_b0, float* d_dec_w1, float* d_dec_b1 /* all four or none; accumulated */,
                               void* stream);

/* Camera gradient of hfagp_raymarch_normals (additive to ABI 15): from g_normal = dL/d normal to the per-ray record
 * ray_grad[b][r][0..5] = (dL/d origin, dL/d direction) of hfagp_raymarch_bwd_camera and, through the same reduction, to
 * d_cam2world [B][16] and d_intrinsics [B][9].  Call it after hfagp_raymarch_fwd with fwd->state given, on the same stream.  The
 * sample depths t carry no gradient; per sample q = (2 / box_warp)(o + t d).  With a, g, r, n, d sigma_s, gamma, w'_k, u, v, e of
 * hfagp_raymarch_normals_bwd, gamma_q = (2 / box_warp) gamma, (cx, cy) the components of gamma_q a plane's two grid coordinates
 * (gx, gy) carry, x = wsig * sigmoid(hp) * d sigma_s + e and dF = W0'^T x, the positional gradient is, per plane in grid units,
 *   dL/dgx = sum_k (texel_k . dF) dw_k/dgx / 3 + m cy,      dL/dgy = sum_k (texel_k . dF) dw_k/dgy / 3 + m cx,
 *   m = (W / 2)(H / 2) sum_k s_k ok_k (texel_k . a) / 3,    s = (+1, -1, -1, +1) for the taps nw, ne, sw, se
 * (bilinear weights have no pure second derivative, only d2 w_k / dgx dgy = s_k; ok_k = 0 for a tap outside the plane), routed to
 * the three axes of q as plane_axes projects them; dL/dp = (2 / box_warp) dL/dq, and per ray
 *   ray_grad = (sum_s dL/dp_s, sum_s t_s dL/dp_s).
 * accumulate != 0: the six floats are ADDED to what ray_grad holds (one plain load, add, store per ray) -- after
 * hfagp_raymarch_bwd_camera on the same buffer, so that one reduction serves the whole loss; 0: they are written (zeros for a ray
 * whose g_normal is exactly 0, which is otherwise skipped).  d_cam2world and d_intrinsics: both or neither; when given,
 * the reduction of hfagp_raymarch_bwd_camera runs on the final ray_grad.  One writer per ray, no atomics: two calls give the same
 * bits.  Decoder arithmetic: the forward products (hp) as hfagp_raymarch_fwd (split 16-bit operands given planes_absmax, exact fp32
 * without it); the second-order products AND a = W0'^T (wsig * sigmoid(hp)) on the exact fp32 matrix instructions with either
 * decoder.  Unlike hfagp_raymarch_normals / hfagp_raymarch_normals_bwd, which take a from split-bf16 parts (2^-16 per product)
 * with the 16-bit decoder, the n this entry forms there is the forward's to ~2^-16, not to the bit: that error has one sign over
 * neighbouring rays and would not average out in the reduction over a frame.
 * HFAGP_EBADARG, nothing launched: fwd, fwd->state, fwd->planes, g_normal or ray_grad NULL, or only one of d_cam2world /
 * d_intrinsics given (then the checks of hfagp_raymarch_fwd); HFAGP_EUNSUPPORTED: sample counts.                               */
int hfagp_raymarch_normals_bwd_camera(const HfagpRaymarchArgs* fwd, const float* g_normal /* [B][R][3] */,
                                      float* ray_grad /* [B][R][6] */, int accumulate,
                                      float* d_cam2world, float* d_intrinsics, void* stream);

/* ------------------------------------------------------------------ point queries (ABI 13)
 * The decoder at arbitrary points, no compositing: per point the same tri-plane gather and OSGDecoder the ray marcher runs,
 *   sigma = raw decoder output 0 (NO softplus: EG3D's sample() returns x[..., 0:1])
 *   rgb   = sigmoid(x[..., 1:]) * 1.002 - 0.001 (32 channels)
 * of the points q = fp32(2 / box_warp) * p.  Decoder arithmetic as hfagp_raymarch_fwd: split fp16 given planes_absmax, exact fp32
 * without it, so a query reports the densities the renderer sees.  Two point sources:
 *   explicit  coords != NULL: points [Bc][M][3]; Bc = 1 queries one point set for every identity; out [B][M] (rgb [B][M][32])
 *   grid      coords == NULL: the lattice of EG3D's create_samples, generated in the kernel (nothing materialised): N points per
 *             axis over a cube of side cube_length centred at the origin, coordinate k = fp32(i_k) * fp32(cube_length / (N-1))
 *             + fp32(-cube_length / 2) (two fp32 roundings, as torch computes it).  Only x in [x_begin, x_begin + x_count) is
 *             evaluated; out [B][x_count][N][N] indexed (ix - x_begin, iy, iz), iz fastest (rgb: x 32).
 * Identity b's outputs start at sigma + b * out_stride (rgb + b * out_stride * 32); out_stride 0 = dense.  Offsets are 64-bit. */
typedef struct {
    const float* planes;      /* [B][3][H][W][32] fp32 (as HfagpRaymarchArgs::planes)                                     */
    const float* coords;      /* [Bc][M][3] points in world units, or NULL: grid mode                                     */
    const float* dec_w0;      /* decoder.net.0.weight [64][32]  (raw parameter)                                           */
    const float* dec_b0;      /* decoder.net.0.bias   [64]                                                                */
    const float* dec_w1;      /* decoder.net.2.weight [33][64]                                                            */
    const float* dec_b1;      /* decoder.net.2.bias   [33]                                                                */
    const float* planes_absmax; /* optional [HFAGP_ABSMAX_FLOATS] bound on |planes| (HfagpRaymarchArgs::planes_absmax):
                               * given, the split-fp16 decoder; NULL, the exact fp32 decoder                              */
    float*       sigma;       /* out: raw density, layout above                                                           */
    float*       rgb;         /* optional out: the 32 decoder features; NULL = sigma only (layer 2's colour rows skipped) */
    int64_t M;                /* explicit: points per identity                                                            */
    int64_t out_stride;       /* elements between identities in sigma (0: M, grid x_count * N * N)                      */
    int32_t B, H, W;          /* identities, plane height / width (> 1)                                                   */
    int32_t Bc;               /* explicit: identities in coords, 1 (broadcast) or B                                       */
    int32_t N;                /* grid: points per axis (>= 2)                                                             */
    int32_t x_begin, x_count; /* grid: the slab of x evaluated by this launch, inside [0, N)                              */
    int32_t plane_axes;       /* 0: (x,y),(x,z),(z,x) [eg3d original]; 1: third = (z,y)                                   */
    float decoder_lr_mul;
    double box_warp;          /* python float of rendering_kwargs (kept double: 2 / box_warp rounds once, to fp32)        */
    double cube_length;       /* grid: side of the cube (EG3D: box_warp)                                                  */
} HfagpPlanesQueryArgs;

int hfagp_planes_query(const HfagpPlanesQueryArgs* a, void* stream);

/* Backward of hfagp_planes_query for explicit points (additive to ABI 15; grid mode has no backward: HFAGP_EUNSUPPORTED).
 * Given dL/dsigma [B][M] and / or dL/drgb [B][M][32] (at least one), recomputes gather and decoder per point in the precision
 * the forward ran (planes_absmax given: split fp16 forward, split bf16 adjoint; NULL: exact fp32) and writes, each optional
 * (at least one):
 *   d_planes  [B][3][H][W][32]  ACCUMULATED INTO with fp32 atomics (the caller zeroes it, or hands over a gradient to add
 *             to).  Every plane is scattered at its true texels.  hfagp_raymarch_bwd OVERWRITES plane 2 of its d_planes
 *             with plane 1 transposed on square planes with plane_axes 0, so a caller sharing one d_planes between the two
 *             must call this entry AFTER hfagp_raymarch_bwd on the same stream.
 *   d_coords  [B][M][3]  plain stores, one writer per point, in world units (the 2 / box_warp scale included).  With Bc = 1
 *             the gradient of the shared point set is the caller's sum over B.  Points outside the box get exact zeros.
 *   d_dec_*   the decoder-parameter gradients (all four or none), ACCUMULATED INTO with one set of atomics per wavefront.
 * The bilinear gather is not differentiable where a pixel coordinate is an integer; there the one-sided derivative of the
 * cell the forward's floor() picked is returned.                                                                        */
typedef struct {
    const float* planes;      /* [B][3][H][W][32] fp32                                                                    */
    const float* coords;      /* [Bc][M][3] points in world units (required)                                              */
    const float* dec_w0;      /* decoder.net.0.weight [64][32]  (raw parameter)                                           */
    const float* dec_b0;      /* decoder.net.0.bias   [64]                                                                */
    const float* dec_w1;      /* decoder.net.2.weight [33][64]                                                            */
    const float* dec_b1;      /* decoder.net.2.bias   [33]                                                                */
    const float* planes_absmax; /* optional, as HfagpPlanesQueryArgs::planes_absmax: pass what the forward call passed    */
    const float* g_sigma;     /* optional [B][M]     dL/d sigma (the raw density)                                         */
    const float* g_rgb;       /* optional [B][M][32] dL/d rgb                                                             */
    float*       d_planes;    /* optional, accumulated into                                                               */
    float*       d_coords;    /* optional out [B][M][3]                                                                   */
    float*       d_dec_w0;    /* optional [64][32], accumulated into (the four go together)                               */
    float*       d_dec_b0;    /* [64]                                                                                     */
    float*       d_dec_w1;    /* [33][64]                                                                                 */
    float*       d_dec_b1;    /* [33]                                                                                     */
    int64_t M;                /* points per identity (> 0)                                                                */
    int32_t B, H, W;          /* identities, plane height / width (> 1)                                                   */
    int32_t Bc;               /* identities in coords, 1 (broadcast) or B                                                 */
    int32_t plane_axes;       /* 0: (x,y),(x,z),(z,x) [eg3d original]; 1: third = (z,y)                                   */
    float decoder_lr_mul;
    double box_warp;
} HfagpPlanesQueryBwdArgs;

int hfagp_planes_query_bwd(const HfagpPlanesQueryBwdArgs* a, void* stream);

/* Density gradient and unit surface normal at explicit points (additive to ABI 15): hfagp_planes_query with two more outputs, one
 * launch.  A point is a ray sample of hfagp_raymarch_normals with compositing weight 1 and no depth.  Per point, with
 * q = fp32(2 / box_warp) p, F the plane mean of the three bilinear gathers, hp = W0' F + b0' (the lr_mul gains folded in):
 *   sigma, rgb   exactly as hfagp_planes_query computes them (split fp16 given planes_absmax, exact fp32 without it): its bits
 *   a = d sigma / dF = W0'^T (wsig * sigmoid(hp))   on the exact fp32 matrix instructions with EITHER decoder, so that this entry
 *                and hfagp_planes_query_normals_bwd form the same n
 *   grad   = g = (2 / box_warp) J^T a   the WORLD-space gradient of the raw density; J = dF / dq with zeros padding and
 *                align_corners = False; where a pixel coordinate is an integer, the one-sided derivative of the cell the
 *                forward's floor() picked
 *   normal = n = -g * rsqrt(g.g + 1e-12)   the unit normal from dense to empty
 * Outputs, each optional (at least one): a->sigma [B][M], a->rgb [B][M][32], grad [B][M][3], normal [B][M][3]; identity b's start
 * at b * out_stride elements (x 32, x 3, x 3; out_stride 0 = M).  A point outside every plane gets exact zeros in grad and normal.
 * One writer per point, no atomics: two calls give the same bits.  The grid fields of `a` are not read.
 * HFAGP_EBADARG, nothing launched: a, the planes or a decoder tensor NULL; no output given; bad B / H / W / M / Bc / plane_axes /
 * box_warp / out_stride.  HFAGP_EUNSUPPORTED, nothing launched: a->coords NULL (no grid mode); H * W > 2^25.                   */
int hfagp_planes_query_normals(const HfagpPlanesQueryArgs* a, float* grad /* [B][M][3] or NULL */,
                               float* normal /* [B][M][3] or NULL */, void* stream);

/* Backward of the grad / normal outputs of hfagp_planes_query_normals (additive to ABI 15): from g_grad = dL/d grad and / or
 * g_normal = dL/d normal, both [B][M][3] (at least one), to the plane gradient and the decoder-parameter gradients, one launch.
 * The gradients of sigma / rgb are NOT formed here: they stay with hfagp_planes_query_bwd, and a caller with both launches both
 * entries into the same buffers.  The forward is recomputed per point (a, g, n as the forward entry forms them); then, with
 * r = sqrt(g.g + 1e-12), it is the "through the normals" branch of hfagp_raymarch_normals_bwd with omega = 1 and d sigma_s = 0:
 *   gamma = dL/dg = g_grad - (1 / r)(g_normal - n (n . g_normal));   per tap k of every plane, with w_k its bilinear weight,
 *   w'_k = (2 / box_warp) gamma . grad_q w_k (0 for a tap outside the plane),   u = sum_planes sum_k texel w'_k / 3,   v = W0' u,
 *   e = wsig * sigmoid(hp) * (1 - sigmoid(hp)) * v,   dF = W0'^T e.
 *   a->d_planes    += (w_k / 3) dF + (w'_k / 3) a at every tap, all three planes at their true texels (fp32 atomics): as
 *                     hfagp_planes_query_bwd, call it AFTER hfagp_raymarch_bwd on a shared buffer, which overwrites plane 2 on
 *                     mirrored planes.
 *   a->d_dec_w0    += (e F^T + dH u^T) * gain, dH = wsig * sigmoid(hp);   a->d_dec_b0 += e * gain;
 *   a->d_dec_w1[0] += sigmoid(hp) * v * gain;   the colour rows of d_dec_w1 and ALL of d_dec_b1 receive nothing.  The four go
 *                     together (all or none), one set of atomics per wavefront; gains as hfagp_raymarch_bwd.
 * At least one of d_planes and the decoder gradients is given.  The second-order products (and a) run on the exact fp32 matrix
 * instructions with either decoder; hp as the forward ran it (pass the planes_absmax the forward call got).  A point whose two
 * upstream vectors are exactly 0 touches nothing.  There is no gradient w.r.t. the points for these two outputs.
 * HFAGP_EBADARG, nothing launched: a, the planes or a decoder tensor NULL; a->g_sigma, a->g_rgb or a->d_coords not NULL; g_grad
 * and g_normal both NULL; only some of the four decoder outputs given; no output given; bad B / H / W / M / Bc / plane_axes /
 * box_warp.  HFAGP_EUNSUPPORTED, nothing launched: a->coords NULL (no grid mode); H * W > 2^25.                                */
int hfagp_planes_query_normals_bwd(const HfagpPlanesQueryBwdArgs* a /* g_sigma, g_rgb, d_coords must be NULL */,
                                   const float* g_grad, const float* g_normal, void* stream);

/* ------------------------------------------------------------------ surface tracing (additive to ABI 15)
 * The first hit of every ray of a list with the iso-surface sigma = level of the raw density (the surface hfagp_marching_cubes
 * extracts from a density lattice at the same level), one launch.  Rays as hfagp_raymarch_rays_limits_fwd takes them: origins and
 * directions [B][R][3] in world units, directions NOT normalised (a point is o + t d), per-ray limits [B][R].  sigma(x) below is the
 * raw density of hfagp_planes_query at the world point x, to the bit (split fp16 decoder given planes_absmax, exact fp32 without).
 * Every operation of the ray arithmetic is rounded to fp32 on its own (no fused multiply-add), as torch evaluates the expressions:
 *   empty ray   unless both limits are finite and t_far > t_near: a miss, nothing is evaluated for it
 *   nodes       dt = (t_far - t_near) / fp32(steps);  t_i = t_near + fp32(i) * dt for i < steps, t_steps = t_far;  x = o + t * d
 *   coarse      cell = the first i in 0..steps with sigma(x(t_i)) >= level (a NaN density never hits); none: a miss, cell = -1;
 *               cell = 0: the origin is inside already, t = t_near
 *   refine      for cell > 0: lo = t_{cell-1}, hi = t_cell with their densities s_lo, s_hi; `refine` times mid = 0.5 * (lo + hi) and
 *               sigma(x(mid)) >= level replaces (hi, s_hi), anything else (lo, s_lo); then one secant step
 *               t = lo + (level - s_lo) / (s_hi - s_lo) * (hi - lo) clamped into [lo, hi], or t = hi unless s_hi - s_lo > 0
 *   at the hit  point = o + t * d;  sigma, sigma_grad = g and normal = n of hfagp_planes_query_normals at that point (its bits)
 * Outputs, each optional (at least one), [B][R] (x 3 for point, sigma_grad, normal): hit (0 / 1), cell, t, point, sigma, sigma_grad,
 * normal.  A miss (empty rays included) writes hit = 0, cell = -1 and exact zeros everywhere else: never NaN or inf.  One writer
 * per ray, no atomics: two calls give the same bits, whichever outputs are asked for.  About cell + 1 + refine + 1 density
 * evaluations per hit, steps + 1 per miss (a tile of 16 rays marches until its last ray is decided).
 * HFAGP_EBADARG, nothing launched: a, the planes, a decoder tensor, the rays or a limit NULL; no output given; steps outside
 * [1, 4096]; refine outside [0, 30]; bad B / H / W / R / plane_axes / box_warp.  HFAGP_EUNSUPPORTED: H * W > 2^25.              */
typedef struct {
    const float* planes;         /* [B][3][H][W][32] fp32 (as HfagpRaymarchArgs::planes)                                    */
    const float* ray_origins;    /* [B][R][3]                                                                               */
    const float* ray_directions; /* [B][R][3], taken as given                                                               */
    const float* t_near;         /* [B][R]                                                                                  */
    const float* t_far;          /* [B][R]                                                                                  */
    const float* dec_w0;         /* decoder.net.0.weight [64][32]  (raw parameter)                                          */
    const float* dec_b0;         /* decoder.net.0.bias   [64]                                                               */
    const float* dec_w1;         /* decoder.net.2.weight [33][64]                                                           */
    const float* dec_b1;         /* decoder.net.2.bias   [33]                                                               */
    const float* planes_absmax;  /* optional, as HfagpPlanesQueryArgs::planes_absmax                                        */
    uint8_t*     hit;            /* optional out [B][R]                                                                     */
    int32_t*     cell;           /* optional out [B][R]                                                                     */
    float*       t;              /* optional out [B][R]                                                                     */
    float*       point;          /* optional out [B][R][3]                                                                  */
    float*       sigma;          /* optional out [B][R]                                                                     */
    float*       sigma_grad;     /* optional out [B][R][3]                                                                  */
    float*       normal;         /* optional out [B][R][3]                                                                  */
    int64_t R;                   /* rays per frame (> 0)                                                                    */
    int32_t B, H, W;             /* frames, plane height / width (> 1)                                                      */
    int32_t plane_axes;          /* 0: (x,y),(x,z),(z,x) [eg3d original]; 1: third = (z,y)                                  */
    int32_t steps;               /* coarse intervals per ray, 1 .. 4096                                                     */
    int32_t refine;              /* bisections of the bracket, 0 .. 30                                                      */
    float level;                 /* raw density of the surface (the unit of hfagp_planes_query's sigma)                     */
    float decoder_lr_mul;
    double box_warp;
} HfagpTraceRaysArgs;

int hfagp_trace_rays(const HfagpTraceRaysArgs* a, void* stream);

/* ------------------------------------------------------------------ mesh tracing (additive to ABI 15)
 * The first hit of every ray of a list with a triangle mesh, one launch.  Rays as hfagp_trace_rays takes them (directions NOT
 * normalised, a point is o + t d, per-ray limits [B][R]).  The mesh arrives as per-face vertex records tri [Bt][F][9] = (a, b, c)
 * of every face, Bt = tri_frames = 1 (one mesh for all frames) or B.  Per ray and face, every operation rounded to fp32 on its own
 * (no fused multiply-add; the division and the square root correctly rounded), as torch evaluates the expressions:
 *   A = a - o, B = b - o, C = c - o;   cross(x, y) = (x1 y2 - x2 y1, x2 y0 - x0 y2, x0 y1 - x1 y0);   dot(x, y) = (x0 y0 + x1 y1) + x2 y2
 *   U = dot(d, cross(B, C)), V = dot(d, cross(C, A)), W = dot(d, cross(A, B)), det = (U + V) + W
 *   N = cross(b - a, c - a), dn = dot(d, N), t = dot(A, N) / dn
 *   candidate iff ((U >= 0 & V >= 0 & W >= 0) | (U <= 0 & V <= 0 & W <= 0)) & det != 0 & dn != 0 & t_near <= t & t <= t_far
 *   winner = the candidate of smallest t, equal t: the smallest face index      (a NaN fails every comparison; hits are two-sided)
 * Outputs, each optional (at least one), [B][R] (x 3 for bary, point, normal): hit (0 / 1), face (-1 for a miss), t, bary =
 * (U, V, W) / det (the weights of a, b, c), point = o + t d, normal = N / sqrt(dot(N, N)) (the winding's, not flipped), front =
 * (dn < 0).  A miss writes hit = 0, face = -1, front = 0 and exact zeros everywhere else.  One writer per ray, no atomics: two
 * calls give the same bits.
 * cell_start == NULL: brute force, every ray against every face (the faces stream through LDS in tiles of 256 records).
 * cell_start != NULL: a uniform grid of G^3 cells per mesh frame.  grid_box [Bt][6] = the lower corner and the cell size per axis;
 * cell (ix, iy, iz) spans [plane_k(i), plane_k(i + 1)], plane_k(i) = lo_k + fp32(i) * cell_k; cell_start [Bt][G^3 + 1] holds
 * offsets into cell_faces [n_pairs] (the faces of cell (ix G + iy) G + iz of frame f are cell_faces[cell_start[f][c] ..
 * cell_start[f][c + 1])).  The ray walks the cells with a 3-D DDA of at most 3 G + 3 steps, tests the faces of every list with the
 * arithmetic above, keeps the minimum of (t, face) and stops once that t lies before the exit of the current cell.  Offsets and face
 * indices are clamped into [0, n_pairs] and [0, F): no content of the lists can make the kernel read out of bounds.  A ray whose
 * origin, direction or grid entry is not finite is tested against every face instead.
 * HFAGP_EBADARG, nothing launched: a, tri, the rays or a limit NULL; no output given; B, R, F or n_pairs negative; tri_frames not 1
 * or B; only some of cell_start / cell_faces / grid_box given; G outside [1, 256].  HFAGP_EUNSUPPORTED: B * R >= 2^31.
 * B = 0 or R = 0 launches nothing; F = 0 writes misses.                                                                           */
typedef struct {
    const float*   tri;            /* [tri_frames][F][9]                                                                      */
    const float*   ray_origins;    /* [B][R][3]                                                                               */
    const float*   ray_directions; /* [B][R][3], taken as given                                                               */
    const float*   t_near;         /* [B][R]                                                                                  */
    const float*   t_far;          /* [B][R]                                                                                  */
    const int32_t* cell_start;     /* optional [tri_frames][G^3 + 1]; NULL = brute force                                      */
    const int32_t* cell_faces;     /* [n_pairs], with cell_start                                                              */
    const float*   grid_box;       /* [tri_frames][6], with cell_start                                                        */
    uint8_t*       hit;            /* optional out [B][R]                                                                     */
    int32_t*       face;           /* optional out [B][R]                                                                     */
    float*         t;              /* optional out [B][R]                                                                     */
    float*         bary;           /* optional out [B][R][3]                                                                  */
    float*         point;          /* optional out [B][R][3]                                                                  */
    float*         normal;         /* optional out [B][R][3]                                                                  */
    uint8_t*       front;          /* optional out [B][R]                                                                     */
    int64_t R;                     /* rays per frame                                                                          */
    int64_t n_pairs;               /* entries of cell_faces                                                                   */
    int32_t B, F;                  /* ray frames, faces                                                                       */
    int32_t tri_frames;            /* 1 or B                                                                                  */
    int32_t G;                     /* cells per axis, 1 .. 256 (with cell_start)                                              */
} HfagpTraceMeshArgs;

int hfagp_trace_mesh(const HfagpTraceMeshArgs* a, void* stream);

/* ------------------------------------------------------------------ marching cubes (ABI 14)
 * The iso-surface of a fp32 volume V[n0][n1][n2] (last axis fastest, each extent >= 2) as a welded triangle mesh.
 *   inside:   a lattice point is inside iff V > level (strict; NaN is outside).
 *   vertices: one per crossed edge (two lattice points one step apart along one axis, exactly one inside), at
 *             p0 + t (p1 - p0), t = (level - v0) / (v1 - v0), p0 the lower-index end, output origin + spacing * p (fp32).
 *             ORDER: ascending by the owning (lower-index) point's linear index (i n1 + j) n2 + k, then axis 0, 1, 2.
 *   faces:    int32 vertex index triples from a 256-case table over the 8 corners of each cube (corner c at offset
 *             (c >> 2 & 1, c >> 1 & 1, c & 1)); ORDER: ascending by cube (i, j, k), k fastest, then the table's order.
 *             WINDING: counter-clockwise seen from outside, the geometric normal points toward decreasing values.
 *             Ambiguous cube faces are cut the same way from both sides (inside corners never connect across a face
 *             diagonal): the mesh of a volume whose boundary layer is all outside is closed and edge-manifold.
 * The output is bit-identical from run to run and independent of the launch: positions come from prefix sums, no atomics.
 * Two phases, so that the caller can allocate in between:
 *   hfagp_marching_cubes_count  fills the workspace (per lattice row offsets) and counts[0] = vertices, counts[1] = faces;
 *   hfagp_marching_cubes_emit   writes verts / faces.  It reads counts back and SYNCHRONISES the stream (the one entry point
 *                               that does): capacities below the counts return HFAGP_EBADARG, counts >= 2^31 return
 *                               HFAGP_EUNSUPPORTED, and nothing is written; an empty mesh launches nothing.
 * Both take the same arguments; the workspace must survive from count to emit.  Offsets are 64-bit. */
typedef struct {
    const float* volume;      /* [n0][n1][n2] fp32                                                                     */
    void*        workspace;   /* >= hfagp_marching_cubes_workspace_bytes(n0, n1, n2) bytes, 8-byte aligned            */
    int64_t*     counts;      /* [2]: vertices, faces (written by _count)                                              */
    float*       verts;       /* out [vert_capacity][3] (emit)                                                         */
    int32_t*     faces;       /* out [face_capacity][3] (emit)                                                         */
    int64_t workspace_bytes;
    int64_t vert_capacity;
    int64_t face_capacity;
    int32_t n0, n1, n2;       /* extents, each >= 2                                                                    */
    float level;              /* iso level                                                                             */
    float origin[3];          /* position of lattice point (0, 0, 0)                                                   */
    float spacing[3];         /* lattice step per axis                                                                 */
} HfagpMarchingCubesArgs;

size_t hfagp_marching_cubes_workspace_bytes(int32_t n0, int32_t n1, int32_t n2);
int hfagp_marching_cubes_count(const HfagpMarchingCubesArgs* a, void* stream);
int hfagp_marching_cubes_emit(const HfagpMarchingCubesArgs* a, void* stream);

/* ------------------------------------------------------------------ styles
 * styles[b][i] = (w[b] . A[i]) / sqrt(w_dim) * 1 + bias[i]   (then * style_gain)
 * dcoef[b][o]  = rsqrt( sum_i styles[b][i]^2 * wsq[o][i] + eps )   if wsq != NULL */
typedef struct {
    const float* w;           /* [B][w_stride] one latent row per sample                      */
    const float* affine_w;    /* [Cin][w_dim]                                                 */
    const float* affine_b;    /* [Cin]                                                        */
    const float* wsq;         /* [Cout][Cin] = sum_k weight[o][i][k]^2, or NULL (no demod)    */
    float*       styles;      /* out [B][Cin]                                                 */
    float*       dcoef;       /* out [B][Cout] or NULL                                        */
    int32_t B, w_dim, w_stride, Cin, Cout;
    float style_gain, eps;
} HfagpStyleArgs;

int hfagp_style_fwd(const HfagpStyleArgs* a, void* stream);
/* the same for n <= 32 layers in one launch per kernel (styles, then demodulation): the styles of a whole
 * synthesis pass depend only on ws, so the host computes them up front                                    */
int hfagp_style_batch_fwd(const HfagpStyleArgs* items, int32_t n, void* stream);

/* Householder QR of the latent basis A = (bases + 1e-8)^T [m x n], n <= 64 (headnerf.py:85-91), split as
 *   gram = A^T A [n][n] and top = A[0:n, 0:n] [n][n] (row-major, formed by the caller with one GEMM / one copy)
 *   -> R [n][n] upper triangular with LAPACK geqrf's sign convention, Rinv = R^-1;  the caller forms Q = A . Rinv.
 * One small kernel instead of the ~250 launches of a library geqrf + orgqr on a 7168 x 50 panel.            */
int hfagp_qr_gram_fwd(const float* gram, const float* top, float* R, float* Rinv, int32_t n, void* stream);
/* Re-orthogonalisation pass (CholeskyQR2's second step) that removes the cond(A)^2 eps orthogonality defect of the
 * Gram-matrix factorisation: gram = Q1^T Q1 [n][n] of the first pass' Q1 -> upper Cholesky factor R [n][n] (positive
 * diagonal, so the signs of pass 1 = LAPACK's are kept) and Rinv; the caller forms Q = Q1 . Rinv.
 * status (optional, device float[2]): [0] = max |gram - I| = the defect of pass 1 (the host's conditioning monitor:
 * HeadNeRF_* falls back to a library Householder QR when it grows), [1] = 1 when a pivot was not positive — the
 * outputs are then NaN, never silently wrong.                                                                   */
int hfagp_qr_refine_fwd(const float* gram, float* R, float* Rinv, float* status, int32_t n, void* stream);
/* ABI 12: out[n][n] = scale * X^T Y for tall-skinny X, Y [m x n], n <= 64, element (k, i) at k * rs + i * cs (row- or
 * column-major operands): the Gram matrices of the two passes above (A^T A, Q1^T Q1) and -Q^T dQ of the QR's backward, where a
 * GEMM library runs one macro-tile.  workspace: hfagp_tall_gram_workspace_bytes(m, n); fixed summation order.                */
size_t hfagp_tall_gram_workspace_bytes(int32_t m, int32_t n);
int hfagp_tall_gram(const float* X, int64_t x_rs, int64_t x_cs, const float* Y, int64_t y_rs, int64_t y_cs, float* workspace,
                    float* out, int32_t m, int32_t n, float scale, void* stream);

/* FullyConnectedLayer (mapping network): y = act((x . W^T) * lr_mul/sqrt(In) + bias*lr_mul) * gain   [B][Out] */
int hfagp_fc_fwd(const float* x, const float* weight, const float* bias, float* y, int32_t B, int32_t In, int32_t Out,
                 float lr_mul, int32_t act, float alpha, float gain, void* stream);

/* weight preparation (cached by the host while the generator is frozen)
 *   wt  [taps][Cin/4][Cout][4]  <- weight [Cout][Cin][kh][kw]      (MFMA B-operand image)
 *   wsq [Cout][Cin]             <- sum over taps of weight^2                           */
int hfagp_weight_prep(const float* weight, float* wt, float* wsq,
                      int32_t Cout, int32_t Cin, int32_t taps, void* stream);

/* split-bf16 weight image for the HFAGP_PREC_BF16X3 / _BF16X6 conv path:
 *   wb [nparts][taps][Cin/8][Cout][8] bf16  <- weight [Cout][Cin][kh][kw],  w = part0 + part1 (+ part2),
 *   each part the round-to-nearest bf16 of the residual left by the parts before it (nparts = 2 or 3).
 *   nparts = 1: the HFAGP_PREC_F16 image, same layout, elements rounded to IEEE fp16.
 *   When Cout % 128 != 0 (the 96-channel toRGB) the buffer must extend 512 bytes past the image: the 128-wide
 *   tile reads (and discards) one partial row beyond it.                                                   */
int hfagp_weight_prep_split(const float* weight, void* wb, int32_t Cout, int32_t Cin, int32_t taps,
                            int32_t nparts, void* stream);
/* the same image selected by HFAGP_PREC_* (F16: 1 fp16 part, BF16X3 / BF16X6: 2 / 3 bf16 parts,
 * F16X3: 2 fp16 parts = round-to-nearest fp16 of the weight and of its residual)                           */
int hfagp_weight_prep_prec(const float* weight, void* wb, int32_t Cout, int32_t Cin, int32_t taps,
                           int32_t precision, void* stream);
/* Weight images (ABI 15).  A bfloat16 image holds the weight itself: bfloat16 has fp32's exponent range, so BF16X3 / BF16X6 keep
 * their class for ANY finite fp32 weight tensor.  A float16 image of the RAW weight (the two calls above) keeps its class only
 * while the parts are fp16 normals: F16X3 has its 22 bits for 2^-3 <= |w| <= 65504 and loses one bit per factor of two below
 * (4e-6 of max |y| is crossed near |w| ~ 4e-3), F16 for 2^-14 <= |w| <= 65504; beyond 65504 the image holds infinities.
 * hfagp_weight_prep_scaled (F16, F16X3 / F16X2 only) lifts that: it finds max |w| of the tensor on the device, writes it to
 * *w_absmax (one float, device memory, no host synchronisation) and stores the parts of  w * 2^-e,  e = 8 floor((ex + 3) / 8)
 * where max |w| = f 2^ex, f in [0.5, 1)  — the multiple of 8 that brings the image's maximum into [2^-4, 2^4); e = 0 for an
 * all-zero or non-finite tensor, and |e| <= 120.  For 2^-4 <= max |w| < 2^4 (unit-scale and 1/sqrt(fan-in) weights) e is 0 and
 * the image has the bits of the raw one.  Every consumer of the image is given the same pointer (HfagpModconvArgs::w_absmax,
 * HfagpTorgbSkipArgs::w_absmax), recomputes e from it and folds 2^e into the power of two it already applies to its fp32
 * accumulators for the style / x_absmax scaling: exact, and no work in the main loops.  Contract: for any finite weight tensor
 * with 2^-116 <= max |w| the image is off the weight by at most 2^-21 max |w| per element (F16X3; the low part's step 2^-24
 * against a maximum of at least 2^-4; F16: 2^-11 |w| down to 2^-10 max |w|), nothing overflows, and the result is that of the
 * same arithmetic at unit scale while the combined power of two 2^(e_styles + e_x + e_w) stays within [2^-126, 2^127] (it is
 * clamped there); y(w 2^8j) = 2^8j y(w) bit for bit.  What remains is the spread INSIDE one tensor: elements far below the
 * maximum have fewer bits of their own — against the products of the tensor's large elements in the same sum that is below
 * the class's error.                                                                                                    */
int hfagp_weight_prep_scaled(const float* weight, void* wb, float* w_absmax, int32_t Cout, int32_t Cin, int32_t taps,
                             int32_t precision, void* stream);

/* ABI 11: everything a step needs of a set of conv weights in ONE launch — for each item the forward image (layout of
 * hfagp_weight_prep_prec, `precision`), the image of the Cin/Cout TRANSPOSE (`precision_t`; the bwd-data GEMM's operand) and
 * wsq[Cout][Cin] = sum over taps of w^2; any of the three outputs may be NULL.  Cout, Cin multiples of 32; at most 48 items.
 * For a generator that is being tuned: its weights change every step (trainer_rgb.py:69-71), its images with them. */
typedef struct {
    const float* weight;      /* [Cout][Cin][taps] */
    void*        image;       /* [parts][taps][Cin/8][Cout][8] or NULL */
    void*        image_t;     /* [parts][taps][Cout/8][Cin][8] or NULL */
    float*       wsq;         /* [Cout][Cin] or NULL */
    int32_t Cout, Cin, taps;
    int32_t precision, precision_t;
    float*       w_absmax;    /* ABI 15: one float, receives max |w|; the item's float16 images (either side) are then SCALED images
                               * (hfagp_weight_prep_scaled; the transpose has the same maximum).  NULL: raw images */
} HfagpWeightPrepItem;
int hfagp_weight_prep_batch(const HfagpWeightPrepItem* items, int32_t n, void* stream);

/* ------------------------------------------------------------------ modulated conv
 * Implicit-GEMM on v_mfma_f32_32x32x2_f32 (exact fp32).  Input is scaled by
 * styles on the way into LDS; demodulation, noise, bias, leaky-ReLU, gain and
 * clamp are applied in the epilogue (mode 0/2) or by hfagp_upfir_epilogue_fwd
 * (mode 1, which writes the raw transposed-conv result).                          */
enum {
    HFAGP_CONV3X3 = 0,      /* y = corr3x3(x*s, W), padding 1, fused epilogue                               */
    HFAGP_CONVT3X3_UP2 = 1, /* y_t = conv_transpose2d(x*s, W, stride 2): RAW [B][2H+1][2W+1][Cout]          */
    HFAGP_CONV1X1 = 2,      /* y = x*s . W (toRGB with many output channels), fused epilogue               */
    HFAGP_CONV3X3_BWD = 3,  /* adjoint of mode 0 w.r.t. (x*s): x = grad [B][H][W][Cout_fwd], wt = prep of   */
                            /* weight^T (Cin/Cout swapped), Cin = Cout_fwd, Cout = Cin_fwd                  */
    HFAGP_CONVS2_BWD = 4    /* adjoint of mode 1 w.r.t. (x*s): x = 4 parity images of the y_t gradient      */
                            /* [2][2][B][H+1][W+1][Cin] (hfagp_upfir_bwd), H, W = resolution of dx          */
};
enum { HFAGP_ACT_LINEAR = 0, HFAGP_ACT_LRELU = 1 };
/* arithmetic of the GEMM (accumulation is always fp32):
 *   F32     v_mfma_f32_32x32x2_f32, exact fp32 products
 *   BF16X3  operands split into 2 bf16 parts (hi+lo), 3 v_mfma_f32_32x32x16_bf16 per product
 *           (hi.hi + lo.hi + hi.lo): relative product error ~2^-16
 *   BF16X6  3 parts, 6 MFMAs per product: relative product error ~2^-23 (fp32 class)
 *   F16X3   operands split into 2 fp16 parts (11 + 11 mantissa bits), 3 v_mfma_f32_32x32x16_f16 per product
 *           (hi.hi + lo.hi + hi.lo): relative product error ~2^-22 — fp32 class at the cost of BF16X3
 *           (at any weight scale with a scaled image, hfagp_weight_prep_scaled; a raw float16 image: "Weight images" above)
 *   F16     operands rounded to fp16, ONE v_mfma_f32_32x32x16_f16 per product: relative product error ~2^-11.
 *           The arithmetic EG3D's CUDA path uses in its fp16 blocks (super-resolution, sr_num_fp16_res = 4:
 *           SURVEY.md U4) except that tensors stay fp32 in HBM and accumulation is fp32.  The caller keeps
 *           The fp16 kinds keep |x * style| <= |x| inside the kernel (styles scaled by a power of two per sample,
 *           undone on the accumulators: EG3D's fp16 pre-normalisation, exact); |x| itself must stay below 65504 unless
 *           the tensor's maximum is passed in x_absmax (then any fp32 magnitude is taken, see HfagpModconvArgs).
 * The 16-bit paths need Cin % 16 == 0 and Cout % 128 == 0 — or, except for HFAGP_CONVT3X3_UP2, Cout % 128 >= 96
 * (the 96-channel toRGB: computed on a 128-wide tile whose last columns are discarded) — HFAGP_EUNSUPPORTED otherwise.
 * HFAGP_PREC_F16X2 (ABI 9): the F16X3 weight image (two fp16 parts, 22 bits) against activations rounded to ONE fp16 part —
 *           two MFMAs per product.  The class of TF32 (11-bit x 11-bit), which the reference's cuDNN convolutions use on
 *           Ampere-class GPUs; NOT the default.  hfagp_torgb_skip_fwd / hfagp_upconv_fir_fwd run it as F16X3.               */
enum { HFAGP_PREC_F32 = 0, HFAGP_PREC_BF16X3 = 1, HFAGP_PREC_BF16X6 = 2, HFAGP_PREC_F16 = 3, HFAGP_PREC_F16X3 = 4,
       HFAGP_PREC_F16X2 = 5 };

typedef struct {
    const float* x;           /* [B][H][W][Cin]; x_batch_stride (elements) may be 0 (const)   */
    const void*  wt;          /* hfagp_weight_prep (F32) or hfagp_weight_prep_prec (16-bit precisions) */
    const float* styles;      /* [B][Cin] or NULL                                             */
    const float* dcoef;       /* [B][Cout] or NULL                                            */
    const float* noise;       /* [Ho][Wo] or NULL                                             */
    const float* bias;        /* [Cout] or NULL                                               */
    float*       y;           /* mode 0/2: [B][H][W][Cout]; mode 1: [B][2H+1][2W+1][Cout] raw */
    float*       workspace;   /* split-K partials, >= hfagp_modconv_workspace_bytes()          */
    int64_t x_batch_stride;
    int32_t B, H, W, Cin, Cout;
    int32_t mode, act;
    int32_t ksplit;           /* 0 = let the library choose                                   */
    float noise_strength, alpha, gain, clamp;   /* clamp < 0: none                            */
    int32_t precision;        /* HFAGP_PREC_*                                                 */
    /* fp16 range tracking (optional, both may be NULL).  A tensor without a clamp (EG3D's fp32 backbone,
     * conv_clamp = None) has no bound, and fp16 parts saturate at 65504 and lose bits below 2^-14: the producer of
     * such a tensor publishes max |y| into y_absmax (HFAGP_ABSMAX_FLOATS floats = 64 slots, zeroed by the caller before the
     * launch; blocks write different slots, the maximum over the slots is the tensor's), and the fp16 kinds (F16X3,
     * F16) that consume it read x_absmax and scale the operand by the power of two that brings max |x| to 2^15 —
     * undone on the accumulators, so the result is that of un-scaled arithmetic and nothing saturates.            */
    const float* x_absmax;    /* [HFAGP_ABSMAX_FLOATS] max |x| of the input tensor, or NULL (then |x| <= 65504 is the caller's promise) */
    float*       y_absmax;    /* [HFAGP_ABSMAX_FLOATS] receives max |y| of the fused-epilogue output, or NULL */
    /* fused toRGB of a block's last conv (optional, both or none; 16-bit precisions, modes 0 / 2 without split-K —
     * hfagp_modconv_workspace_bytes() == 0): while the output tile is still in registers the block also forms
     *   rgb[r] = sum_co y[co] * rgb_w[b][r][co]     (r < 3; rgb_w = toRGB weight * its styles, Cout entries per r)
     * over ITS output channels and writes the partial sums to rgb_part; hfagp_torgb_finish_fwd adds the parts, the
     * bias, the clamp and the up-sampled previous image.  Saves the separate toRGB pass over the activation.    */
    /* (with rgb_part, y may be NULL: the activation itself is not stored — the last super-resolution layer of a
     *  forward-only call, whose output feeds nothing but this toRGB)                                                */
    const float* rgb_w;       /* [B][3][Cout] or NULL */
    float*       rgb_part;    /* [hfagp_modconv_rgb_parts()][B][H][W][4] floats (3 used), written, or NULL */
    /* fp16 STORAGE of the activations (EG3D's fp16 blocks keep them in fp16: super-resolution, sr_num_fp16_res = 4):
     * x_f16 = 1: x holds IEEE fp16 values (same shape; pass the pointer as x), y_f16 = 1: y is written as fp16.
     * Only with precision HFAGP_PREC_F16, modes 0 and 1, no split-K (hfagp_modconv_workspace_bytes() == 0); the styles
     * are applied with packed fp16 multiplies and staging is a copy instead of a conversion.                        */
    int32_t x_f16, y_f16;
    /* ABI 15: max |w| as hfagp_weight_prep_scaled / hfagp_weight_prep_batch left it for a SCALED float16 image (see "Weight
     * images"); NULL: wt is an image of the raw weight (bfloat16 images always are).  Also read by hfagp_upconv_fir_fwd. */
    const float* w_absmax;
} HfagpModconvArgs;
/* number of partial-sum images a call with rgb_part writes: (Cout / 128) x 2 */
int32_t hfagp_modconv_rgb_parts(const HfagpModconvArgs* a);
#define HFAGP_ABSMAX_SLOTS 64
/* an absmax buffer is HFAGP_ABSMAX_FLOATS floats: slot i lives at float index i * HFAGP_ABSMAX_STRIDE (one 128-byte
 * line per slot, so the publishing waves' atomics spread over the L2 channels instead of queueing on two lines) */
#define HFAGP_ABSMAX_STRIDE 32
#define HFAGP_ABSMAX_FLOATS (HFAGP_ABSMAX_SLOTS * HFAGP_ABSMAX_STRIDE)

size_t hfagp_modconv_workspace_bytes(const HfagpModconvArgs* a);
int hfagp_modconv_fwd(const HfagpModconvArgs* a, void* stream);

/* FIR (4x4 [1,3,3,1]^2/64, pad [1,1,1,1], gain 4) over the raw transposed-conv
 * output + demod + noise + bias + act.  yt [B][2H+1][2W+1][C] -> y [B][2H][2W][C] */
typedef struct {
    const void*  yt;          /* fp32, or fp16 when io_f16 */
    const float* dcoef;       /* [B][C] or NULL */
    const float* noise;       /* [2H][2W] or NULL */
    const float* bias;        /* [C] or NULL */
    void*        y;           /* fp32, or fp16 when io_f16 */
    int32_t B, H, W, C;       /* H, W = INPUT resolution of the up-conv */
    int32_t act;
    float noise_strength, alpha, gain, clamp;
    float*       y_absmax;    /* optional [HFAGP_ABSMAX_FLOATS]: max |y| (see HfagpModconvArgs); io_f16: of the halves as stored */
    int32_t      io_f16;      /* 1: yt and y are IEEE fp16 tensors (same shapes; HfagpModconvArgs::x_f16 / y_f16), math stays fp32 */
} HfagpUpfirEpilogueArgs;

int hfagp_upfir_epilogue_fwd(const HfagpUpfirEpilogueArgs* a, void* stream);

/* The whole up-sampling layer in ONE pass over its output (EG3D conv2d_resample(up = 2) + bias_act; replaces
 * hfagp_modconv_fwd(mode HFAGP_CONVT3X3_UP2) + hfagp_upfir_epilogue_fwd):
 *   y [B][2H][2W][Cout] = act(FIR(conv_transpose2d(x * styles, W, stride 2)) * dcoef + noise + bias) * gain, clamp
 * The raw transposed-conv result never goes to HBM: a block owns a strip of 32 y_t columns, walks down a segment of
 * tiles and filters each y_t tile in LDS; the three output columns at every strip boundary and the three output rows at
 * every segment boundary are finished by a second, small kernel from raw strips in `scratch`.
 * `a` as for hfagp_modconv_fwd with mode = HFAGP_CONVT3X3_UP2, except that y is the FINAL tensor, dcoef / noise / bias / act /
 * alpha / gain / clamp / y_absmax apply (as in HfagpUpfirEpilogueArgs), workspace and ksplit are ignored and there is no
 * fused toRGB.  Precisions BF16X3, F16X3, F16 (x_f16 / y_f16 storage allowed with F16); Cin % 16 == 0, Cin <= 512,
 * Cout % 128 == 0; the launch must fill the chip (B * ceil((W+1)/16) * Cout/128 >= 256 strips).
 * Cin == 32 (the first super-resolution layer; Cout % 64 == 0, fp32 storage, precisions F16 / BF16X3 / F16X3 / F16X2) takes a
 * STREAMING kernel instead (round 6, csrc/upfir_lean.hip: FIR in registers, no scratch use, no strip kernel) at any batch.
 * hfagp_upconv_fir_scratch_bytes(): bytes of `scratch` the call needs (a non-zero token size where the streaming kernel runs:
 * the pointer must still be non-NULL), or 0 when the shape is not supported — the caller then uses the two-call form.        */
size_t hfagp_upconv_fir_scratch_bytes(const HfagpModconvArgs* a);
int hfagp_upconv_fir_fwd(const HfagpModconvArgs* a, void* scratch, void* stream);

/* skip connection: img_out = upsample2d(img_in) + y  (both channels-last, C channels;
 * img_in may be NULL -> img_out = y).  Optional plane-major output for the last block:
 * planes_out [B][3][2H][2W][C/3] when plane_major != 0.                              */
typedef struct {
    const float* img_in;      /* [B][H][W][C] or NULL */
    const float* y;           /* [B][2H][2W][C] (or [B][H][W][C] when img_in is NULL) */
    float*       img_out;
    int32_t B, H, W, C;       /* H, W = resolution of img_in */
    int32_t plane_major;
    float*       out_absmax;  /* optional [HFAGP_ABSMAX_FLOATS]: receives max |img_out| (HfagpRaymarchArgs::planes_absmax) */
} HfagpSkipArgs;

int hfagp_skip_upsample_add(const HfagpSkipArgs* a, void* stream);

/* toRGB of a backbone block with its skip connection in ONE streaming pass (EG3D SynthesisBlock.forward, architecture
 * 'skip': `img = upsample2d(img); y = self.torgb(x, ws); img = img.add_(y)`), for the 96-channel tri-plane image:
 *   img_out[b][p][co] = sum_i x[b][p][i] styles[b][i] w[co][i] + bias[co] + upsample2d(img_in)[b][p][co]
 * on the 16-bit matrix pipe with split operands (precision = HFAGP_PREC_F16X3 / BF16X3 / BF16X6 / F16, as hfagp_modconv_fwd),
 * every wave streaming 32 positions x Cin channels straight from HBM into MFMA operands; the toRGB output never
 * goes through memory.  Cout a multiple of 32 (<= 128), Cin a multiple of 16 (<= 512), W a multiple of 32, H*W of 128;
 * other shapes: hfagp_modconv_fwd (HFAGP_CONV1X1) + hfagp_skip_upsample_add.                                         */
typedef struct {
    const float* x;           /* [B][H][W][Cin] channels-last */
    const void*  wt;          /* hfagp_weight_prep_prec image of the [Cout][Cin][1][1] weight (taps = 1) */
    const float* styles;      /* [B][Cin] (already * 1/sqrt(Cin)) */
    const float* bias;        /* [Cout] */
    const float* img_in;      /* [B][H/2][W/2][Cout] channels-last, or NULL (first block: img_out = toRGB) */
    float*       img_out;     /* [B][H][W][Cout], or [B][3][H][W][Cout/3] when plane_major (needs Cout = 96) */
    const float* x_absmax;    /* optional [HFAGP_ABSMAX_FLOATS]: max |x| as published by x's producer (fp16 kinds) */
    float*       out_absmax;  /* optional [HFAGP_ABSMAX_FLOATS]: receives max |img_out| */
    int32_t B, H, W, Cin, Cout;
    int32_t precision;        /* HFAGP_PREC_* of the weight image (not F32) */
    int32_t plane_major;
    const float* w_absmax;    /* ABI 15: as HfagpModconvArgs::w_absmax (scaled float16 image), or NULL */
} HfagpTorgbSkipArgs;

int hfagp_torgb_skip_fwd(const HfagpTorgbSkipArgs* a, void* stream);

/* toRGB with few output channels (super-resolution, img_channels = 3):
 * rgb_out[b][c][y][x] (NCHW) = sum_i x[b][y][x][i]*styles[b][i]*w[c][i] + bias[c]
 *                              (clamped) + upsample2d(rgb_in)[b][c][y][x]           */
typedef struct {
    const float* x;           /* [B][H][W][Cin] channels-last */
    const float* weight;      /* [Cout][Cin] (1x1) */
    const float* styles;      /* [B][Cin] (already * 1/sqrt(Cin)) */
    const float* bias;        /* [Cout] */
    const float* rgb_in;      /* NCHW [B][Cout][H/2][W/2] or NULL */
    float*       rgb_out;     /* NCHW [B][Cout][H][W] */
    float*       y_pre;       /* optional NCHW [B][Cout][H][W]: toRGB output before the skip add (for backward) */
    int32_t B, H, W, Cin, Cout;
    float clamp;
} HfagpTorgbArgs;

int hfagp_torgb_fwd(const HfagpTorgbArgs* a, void* stream);

/* second half of the fused toRGB (HfagpModconvArgs::rgb_part): rgb_out[b][c][y][x] (NCHW) =
 * clamp(sum_p part[p][b][y][x][c] + bias[c]) + upsample2d(rgb_in)[b][c][y][x]                         */
typedef struct {
    const float* part;        /* [nparts][B][H][W][4] */
    const float* bias;        /* [Cout] */
    const float* rgb_in;      /* NCHW [B][Cout][H/2][W/2] or NULL */
    float*       rgb_out;     /* NCHW [B][Cout][H][W] */
    float*       y_pre;       /* optional NCHW [B][Cout][H][W]: value before the clamp (backward mask) */
    int32_t nparts, B, H, W, Cout;   /* Cout <= 3 */
    float clamp;
} HfagpTorgbFinishArgs;
int hfagp_torgb_finish_fwd(const HfagpTorgbFinishArgs* a, void* stream);

/* ------------------------------------------------------------------ backward pass (generator frozen: d/d ws)
 * GEMM-shaped parts reuse hfagp_modconv_fwd (modes 3, 4 and 2 with transposed weights).               */

/* One fused streaming pass per activation tensor X [B][H][W][C] (output of layer P, input of its
 * consumers): sums the consumers' input gradients, reduces their style gradients, and pushes the result
 * through P's clamp / gain / leaky-ReLU / demodulation.
 *   gX      = dxs_conv*s_conv + dxs_rgb*s_rgb + s_small * (w_rgb_small^T g_rgb_small) + g_direct + [c < 3] (g_nchw3_a + g_nchw3_b)
 *             (g_rgb_small is masked with [|y_rgb_small| < clamp_rgb_small] when y_rgb_small is given: the clamp of the small toRGB)
 *   g_out   = has_producer ? gX * gain * lrelu'(X) * [|X|<clamp] * dcoef_p : gX
 *   sums[b][0] = sum_pix dxs_conv*X   sums[b][1] = sum_pix dxs_rgb*X   sums[b][2] = sum_pix (w^T g)*X
 *   sums[b][3] = sum_pix g_pre * conv_p      (gradient of P's demodulation coefficients)
 * and, when param_grads != 0 (generator being tuned):
 *   sums[b][4] = sum_pix g_pre (bias of P)   sums[b][5] = sum_pix g_pre * noise_p (per channel: d noise_strength)
 *   sums[b][6+c] = sum_pix g_rgb_small[c] * X   (small-toRGB weight gradient before the style factor)
 * sums is [B][10][C].                                                                                    */
typedef struct {
    const float* dxs_conv;    /* [B][H][W][C] or NULL */
    const float* s_conv;      /* [B][C] */
    const float* dxs_rgb;     /* [B][H][W][C] or NULL */
    const float* s_rgb;       /* [B][C] */
    const float* g_rgb_small; /* NCHW [B][Co][H][W] (already clamp-masked) or NULL; ABI 12: exclusive with dxs_rgb (a layer has one toRGB) */
    const float* w_rgb_small; /* [Co][C] */
    const float* s_small;     /* [B][C] */
    const float* g_direct;    /* [B][H][W][C] extra gradient added as is, or NULL */
    const float* x;           /* [B][H][W][C] saved activation */
    const float* dcoef_p;     /* [B][C] or NULL */
    const float* bias_p;      /* [C] or NULL */
    const float* noise_p;     /* [H][W] or NULL */
    float*       g_out;       /* [B][H][W][C] */
    float*       partial;     /* workspace [B][nchunks][10][C] */
    float*       sums;        /* out [B][10][C] */
    int32_t B, H, W, C, Co, nchunks, has_producer, act_p, param_grads;
    float noise_strength_p, alpha, gain, clamp;
    /* ABI 10 (all optional): */
    const float* y_rgb_small; /* NCHW [B][Co][H][W]: the small toRGB's pre-clamp output; with clamp_rgb_small >= 0 the kernel masks
                                 g_rgb_small itself (the caller then passes the UN-masked gradient) */
    const float* g_nchw3_a;   /* NCHW [B][3][H][W] gradients added to channels 0..2 of gX (image_raw = first three channels of  */
    const float* g_nchw3_b;   /* the feature image: the super-resolution skip path and the caller's d image_raw), or NULL          */
    float clamp_rgb_small;
    /* ABI 11 (optional): the producer's noise strength read from DEVICE memory (one float) instead of `noise_strength_p` — a generator
     * that is being tuned changes it every step, and a host copy would cost a device-to-host synchronisation per step */
    const float* noise_strength_dev;
} HfagpPointwiseBwdArgs;

int hfagp_pointwise_bwd(const HfagpPointwiseBwdArgs* a, void* stream);

/* ABI 12: hfagp_pointwise_bwd with sums = NULL leaves its per-chunk partial sums un-reduced; this reduces up to 32 such buffers in
 * one launch: sums[b][k] = sum over chunks of partial[b][chunk][k], k < n = 10 * C, in a fixed order (not the single-pass reducer's: the last bits may
 * differ) (a backward pass with the generator frozen consumes the sums only at its end: 19 launches -> 1).                               */
typedef struct {
    const float* partial;     /* [B][nchunks][n] */
    float*       sums;        /* [B][n] */
    int32_t B, nchunks, n;
} HfagpReducePartialsItem;
int hfagp_reduce_partials_batch(const HfagpReducePartialsItem* items, int32_t n, void* stream);

/* MipRayMarcher2's depth clamp (EG3D: `torch.clamp(depth, min(sample depths), max(sample depths))` over the WHOLE batch) in one
 * launch: depth [n] is clamped in place to [min_i tminmax[i][0], max_i tminmax[i][1]] (tminmax as hfagp_raymarch_fwd writes it).
 * Up to 64 workgroups, each reducing all of tminmax itself (L2-resident) and clamping its slice; any batch since ABI 11. */
int hfagp_depth_clamp(float* depth, const float* tminmax, int64_t n, void* stream);

/* adjoint of hfagp_upfir_epilogue_fwd's FIR: g_y [B][2H][2W][C] -> four parity images of the y_t gradient,
 * gph [2][2][B][H+1][W+1][C] (input of hfagp_modconv_fwd mode HFAGP_CONVS2_BWD)                          */
int hfagp_upfir_bwd(const float* gy, float* gph, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);

/* adjoint of upsample2d: g [outer][2H][2W][inner] -> gin [outer][H][W][inner] (inner = C for channels-last,
 * 1 for NCHW with outer = B*C)                                                                           */
int hfagp_upsample2d_bwd(const float* g, float* gin, int64_t outer, int32_t H, int32_t W, int32_t inner, void* stream);

/* plane-major [B][3][H][W][Cp] -> channels-last [B][H][W][3*Cp] */
int hfagp_planes_to_nhwc(const float* pm, float* y, int32_t B, int32_t H, int32_t W, int32_t Cp, void* stream);

/* the same with the sum over the V views of an identity fused in: pm [B][V][3][H][W][Cp] (frame b*V + v plane-major) ->
 * y [B][H][W][3*Cp], y[b,h,w,pl*Cp+ch] = sum_v pm[b,v,pl,h,w,ch] in fp32, in the fixed order v = 0 .. V-1 (no atomics: the same
 * bits on every call); V = 1 gives hfagp_planes_to_nhwc's bits.  HFAGP_EBADARG: a null pointer or B, V, H, W < 1;
 * HFAGP_EUNSUPPORTED: Cp % 4 != 0.  (additive within ABI 15)                                                */
int hfagp_planes_sum_to_nhwc(const float* pm, float* y, int32_t B, int32_t V, int32_t H, int32_t W, int32_t Cp, void* stream);

/* styles -> latent: dstot = (ds - styles * sum_o dd_o d_o^3 wsq[o][i]) * style_gain;
 * dw[b][:] (+)= dstot[b] . affine_w / sqrt(w_dim)                                                         */
typedef struct {
    const float* ds;          /* [B][Cin] gradient w.r.t. the styles (data path) */
    const float* dd;          /* [B][Cout] gradient w.r.t. the demod coefficients, or NULL */
    const float* styles;      /* [B][Cin] */
    const float* dcoef;       /* [B][Cout] */
    const float* wsq;         /* [Cout][Cin] */
    const float* affine_w;    /* [Cin][w_dim] */
    float*       dstot;       /* workspace [B][Cin] */
    float*       dw;          /* [B][dw_stride] row of d ws */
    int32_t B, Cin, Cout, w_dim, dw_stride, accumulate;
    float style_gain;
} HfagpStyleBwdArgs;

int hfagp_style_bwd(const HfagpStyleBwdArgs* a, void* stream);

/* the same for every affine layer of a backward pass in two launches (at most 32 items, sorted by `dw`: layers that
 * share a row of d ws are accumulated in item order by one block, so the result is deterministic).  ds / dd are read
 * with a row stride (elements), so the reductions of hfagp_pointwise_bwd can be passed without a copy; every dw row
 * is accumulated into (+=).                                                                                  */
typedef struct {
    const float* ds;          /* [B][Cin], row stride ds_stride */
    const float* dd;          /* [B][Cout], row stride dd_stride, or NULL (no demodulation) */
    const float* styles;      /* [B][Cin] */
    const float* dcoef;       /* [B][Cout] or NULL */
    const float* wsq;         /* [Cout][Cin] or NULL */
    const float* affine_w;    /* [Cin][w_dim] */
    float*       dstot;       /* out [B][Cin] */
    float*       dw;          /* row of d ws: dw[b * dw_stride + k] += ... */
    int32_t B, Cin, Cout, w_dim, dw_stride, ds_stride, dd_stride;
    float style_gain;
} HfagpStyleBwdItem;
int hfagp_style_batch_bwd(const HfagpStyleBwdItem* items, int32_t n, void* stream);

/* backward of hfagp_raymarch_fwd w.r.t. the tri-plane volume: recomputes the forward per ray, then
 * scatters d feat -> d planes with fp32 atomics (d_planes must be zero-initialised by the caller).
 * With plane_axes = 0 on square planes, planes 1 (x,z) and 2 (z,x) receive mirrored gradients: only plane 1
 * is scattered and plane 2 is WRITTEN as its transpose (a third fewer atomics).                            */
typedef struct {
    HfagpRaymarchArgs fwd;    /* same inputs as the forward call (feat/depth/wsum/tminmax unused) */
    const float* g_feat;      /* [B][R][32] gradient of the composited features */
    float*       d_planes;    /* [B][3][H][W][32], accumulated into */
    float*       rec;         /* workspace [B][R][Sc+Sf][4] floats (per-sample depth, omega, d sigma) */
    /* optional (all four or none): gradients of the decoder parameters, zero-initialised, accumulated into */
    float*       d_dec_w0;    /* [64][32] */
    float*       d_dec_b0;    /* [64] */
    float*       d_dec_w1;    /* [33][64] */
    float*       d_dec_b1;    /* [33] */
    /* optional (ABI 10): scratch [B][R][Sc+Sf][32] floats.  Given (and the column variant applies: plane_axes = 0, square planes
     * up to 256^2), pass 2 runs as two kernels — dL/dF of every sample into the scratch buffer, then the scatter alone — instead
     * of one whose waves alternate between the two in lock step; same arithmetic, the atomic order differs as it does run to run. */
    float*       df_scratch;
    /* optional (ABI 12): scratch of hfagp_raymarch_bwd_rows_bytes(&fwd) bytes.  Given, pass 2 runs as SORT + GATHER instead of
     * a per-sample scatter: the samples are counting-sorted by (frame, plane, 32-texel column strip, texel row), dL/dF of every
     * sample goes to its sorted slot, and every output row tile is a dense product  W[32 texels x 16 samples] . dL/dF[16 x 32]
     * on the 16-bit matrix pipe (split bf16 operands), W being grid_sample's bilinear weights.  d_planes receives two adds per
     * element and bin chunk instead of ~12 atomics per sample; takes precedence over df_scratch.  Decoder gradients (d_dec_*)
     * come from the same pass as dL/dF.  The buffer's contents are undefined before and after the call.                       */
    void*        rows_scratch;
    uint64_t     rows_scratch_bytes;
} HfagpRaymarchBwdArgs;

int hfagp_raymarch_bwd(const HfagpRaymarchBwdArgs* a, void* stream);

/* Depth and opacity gradients through the same backward (additive to ABI 15: HfagpRaymarchBwdArgs keeps its layout).
 * With the kernel's notation — midpoints e = 0 .. S-2 of the depth-sorted samples, compositing weights w_e = alpha_e T_e,
 * midpoint depths tbar_e, W = sum_e w_e (the `wsum` output), D = sum_e w_e tbar_e, d = D / W (the `depth` output) — the
 * per-midpoint adjoint that pass 1 forms becomes
 *     G_e = dL/dw_e = g . cbar_e  -  white_back * sum(g)  +  gamma_W  +  gamma_d * (tbar_e - d) / W
 * gamma_W = g_wsum[ray].  gamma_d = g_depth[ray] taken back through what follows d in the forward (NaN -> inf, then the clamp
 * to the batch-global range [lo, hi] = depth_range): it is 0 where W == 0, where d is not finite and where d lies outside
 * [lo, hi] (a depth ON a bound passes, as torch.clamp's gradient does).  The sample depths carry no gradient (stratified
 * depths come from the uniforms, importance depths are detached as in EG3D), so everything after G_e — d alpha, d sigma, the
 * per-sample records, all of pass 2 — is what the image gradient alone goes through.  On a ray list a per-sample gradient is one
 * more addend (hfagp_raymarch_rays_samples_bwd below):
 *     G_e = g . cbar_e  -  white_back * sum(g)  +  gamma_W  +  gamma_d * (tbar_e - d) / W  +  g_weights[e]
 * hfagp_raymarch_bwd(a, s) == hfagp_raymarch_bwd_geom(a, NULL, s).  a->g_feat may be NULL (zeros) when g_depth or g_wsum is
 * given.  HFAGP_EBADARG, nothing launched: g_depth without depth_range; no upstream gradient at all.                        */
typedef struct {
    const float* g_depth;      /* [B][R] dL/d image_depth (the CLAMPED depth), or NULL            */
    const float* g_wsum;       /* [B][R] dL/d opacity, or NULL                                     */
    const float* depth_range;  /* 2 floats ON THE DEVICE: the batch-global clamp range lo, hi;    */
                               /* required with g_depth                                            */
} HfagpRaymarchGeomGrads;
int hfagp_raymarch_bwd_geom(const HfagpRaymarchBwdArgs* a, const HfagpRaymarchGeomGrads* g, void* stream);
/* bytes of HfagpRaymarchBwdArgs::rows_scratch for this forward configuration (B, H, W, res, Sc, Sf, plane_axes are read);
 * 0 = the sort + gather form does not apply (more than 8192 bins per frame: planes beyond ~256 x 341 texels, or more than
 * 2^31 slots): leave rows_scratch NULL.  At 2 frames x 128^2 rays x 96 samples on mirrored 256^2 planes: 1.8 GB.            */
size_t hfagp_raymarch_bwd_rows_bytes(const HfagpRaymarchArgs* fwd);

/* Camera gradient (additive to ABI 15).  After hfagp_raymarch_bwd[_geom] on the same arguments and stream: a->rec holds pass 1's
 * records (the depth, opacity and white_back terms are folded into them).  a->d_planes, rows_scratch, df_scratch and d_dec_* are
 * ignored.  Per sample the positional derivative of the tri-plane gather (the function the forward evaluated: grid_sample
 * bilinear, zeros padding, a tap outside the plane contributes nothing), summed along the ray:
 * ray_grad: [B][R][6] floats, written (d origin, d direction per ray; the sample depths carry no gradient, as in EG3D).
 * d_cam2world [B][16], d_intrinsics [B][9]: written, both or neither (NULL: only ray_grad) — the adjoint of the ray generation
 * summed over each frame's rays; row 3 of cam2world and intrinsics entries 3, 6, 7, 8 are written as 0.  No atomics: two calls
 * give the same bits.  HFAGP_EBADARG, nothing launched: a, a->rec or ray_grad NULL; one of the two camera outputs alone.     */
int hfagp_raymarch_bwd_camera(const HfagpRaymarchBwdArgs* a, float* ray_grad, float* d_cam2world, float* d_intrinsics, void* stream);

/* ------------------------------------------------------------------ ray lists (additive to ABI 15)
 * The same renderer on R caller-given rays per frame instead of the res x res pinhole grid of a label: EG3D's
 * ImportanceRenderer.forward(planes, decoder, ray_origins, ray_directions, rendering_kwargs) — crops and zoomed windows,
 * several cameras of one identity as one longer list, random ray batches, camera models that are no 25-float label.
 * Directions are taken as given and NOT normalised: sample s of a ray is origin + t_s * direction.  Everything after the ray
 * fetch — depths, gather, decoder, compositing, the per-sample state and records — is the arithmetic of hfagp_raymarch_fwd /
 * hfagp_raymarch_bwd_geom: the list ray_grid-of-a-label in row order renders what the grid call renders.
 * In `base` (and `bwd.fwd`) cam2world, intrinsics and res are IGNORED and may be NULL / 0; u_strat, u_imp, the outputs, state,
 * g_feat, rec and the geometry gradients are sized by R where the grid forms say res * res.  The rays of the launch are walked in
 * list order, cut into eight contiguous parts (one per XCD): locality is the caller's order.
 * HFAGP_EBADARG, nothing launched: a NULL struct, ray_origins or ray_directions NULL, R <= 0, then the checks of the grid entry
 * point; HFAGP_EUNSUPPORTED: sample counts, B * R >= 2^31.                                                                     */
typedef struct {
    HfagpRaymarchArgs base;
    const float* ray_origins;     /* [B][R][3] */
    const float* ray_directions;  /* [B][R][3] */
    int32_t R;                    /* rays per frame */
} HfagpRayListArgs;

typedef struct {
    HfagpRaymarchBwdArgs bwd;     /* as for hfagp_raymarch_bwd; df_scratch is ignored (the column variant is image-shaped) */
    const float* ray_origins;     /* [B][R][3] */
    const float* ray_directions;  /* [B][R][3] */
    int32_t R;
} HfagpRayListBwdArgs;

int hfagp_raymarch_rays_fwd(const HfagpRayListArgs* a, void* stream);
/* d_planes (accumulated into), optional decoder gradients and rec, as hfagp_raymarch_bwd_geom (g may be NULL).  With
 * bwd.rows_scratch of hfagp_raymarch_rays_bwd_rows_bytes bytes pass 2 is sort + gather (a workgroup of the sort takes 32
 * consecutive rays of a frame's list); without it the per-sample scatter kernels run.                                         */
int hfagp_raymarch_rays_bwd(const HfagpRayListBwdArgs* a, const HfagpRaymarchGeomGrads* g, void* stream);
/* bytes of bwd.rows_scratch for this list (B, H, W, R, Sc, Sf, plane_axes are read); 0 = sort + gather does not apply           */
size_t hfagp_raymarch_rays_bwd_rows_bytes(const HfagpRayListArgs* a);
/* The rays' gradient.  After hfagp_raymarch_rays_bwd on the same arguments and stream (a->bwd.rec holds pass 1's records;
 * d_planes, the scratch buffers and d_dec_* are ignored): d_origins, d_directions [B][R][3] are WRITTEN — per ray the positional
 * derivative of the gather summed over its samples, plain and depth-weighted (the record hfagp_raymarch_bwd_camera forms before
 * its reduction; the sample depths carry no gradient).  One writer per ray, no atomics, no reduction: two calls give the same
 * bits.  HFAGP_EBADARG also for a->bwd.rec, d_origins or d_directions NULL.                                                  */
int hfagp_raymarch_rays_bwd_rays(const HfagpRayListBwdArgs* a, float* d_origins, float* d_directions, void* stream);

/* ------------------------------------------------------------------ per-ray depth limits for ray lists (additive to ABI 15)
 * The three list entry points above with a [t_near, t_far] per ray instead of the one interval base.ray_start / ray_end (which
 * is then neither read nor checked): EG3D's ImportanceRenderer with ray_start == ray_end == 'auto' (hfagp_ray_limits_box gives
 * the limits of the tri-plane cube), a camera at any distance, directions of any length, a visibility ray from a surface point
 * (t_near = 0, t_far = the distance to the light), depth-guided sampling (depth -+ delta).
 * Coarse sample s of S = Sc, in fp32 with every operation rounded on its own (math_utils.linspace + sample_stratified for tensor
 * limits):   span = far - near,   t_s = near + (float(s) / float(S-1)) * span + u_s * (span / float(S-1)).
 * Everything after the coarse depths — importance pass, merge, compositing, state, records — is unchanged.
 * A ray is VALID iff both limits are finite and far > near; any other ray is EMPTY and is not marched (no gather, no decoder):
 *   forward: feat = -1 in all 32 channels (+1 with white_back), wsum = 0, depth = +inf, tminmax = (+inf, -inf) — so it does not
 *            enter a min / max over the call's rays; its slice of `state` is not written (unspecified);
 *   backward: its S records are zero, and with them d_planes, the decoder gradients, d_origins and d_directions receive exactly
 *            zero from it; g_depth / g_wsum of an empty ray are not read.
 * The limits carry no gradient (as the sample depths carry none).                                                             */
typedef struct {
    const float* t_near;          /* [B][R] */
    const float* t_far;           /* [B][R] */
} HfagpRayLimits;

/* Slab intersection of n_rays rays ([n][3] origins / directions, any layout of B and R) with the cube [-box_side/2, box_side/2]^3:
 * per axis inv = 1 / d (IEEE, +-inf for a zero component), t0 = (-h - o) * inv, t1 = (h - o) * inv; t_near = max over the axes of
 * min(t0, t1), clamped below at 0 (an origin inside the cube starts at the origin: NOT EG3D's value there); t_far = min over
 * the axes of max(t0, t1).  A miss has t_far <= t_near; a NaN (origin exactly on a slab of an axis the ray is parallel to) makes
 * both limits NaN: either way the ray is empty for the entry points below.  t_near, t_far [n]: written.
 * HFAGP_EBADARG: a NULL pointer, n_rays <= 0 or >= 2^31, box_side not positive and finite.                                      */
int hfagp_ray_limits_box(const float* ray_origins, const float* ray_directions, float* t_near, float* t_far,
                         int64_t n_rays, float box_side, void* stream);
/* HFAGP_EBADARG, nothing launched: lim or one of its members NULL; then the checks of the entry point without limits, minus
 * ray_end > ray_start.                                                                                                        */
int hfagp_raymarch_rays_limits_fwd(const HfagpRayListArgs* a, const HfagpRayLimits* lim, void* stream);
int hfagp_raymarch_rays_limits_bwd(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim,
                                   const HfagpRaymarchGeomGrads* g, void* stream);
/* (reads the depths from the records of hfagp_raymarch_rays_limits_bwd; lim is checked, its arrays are not read)               */
int hfagp_raymarch_rays_limits_bwd_rays(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim,
                                        float* d_origins, float* d_directions, void* stream);

/* ------------------------------------------------------------------ occupancy grids for ray lists (additive to ABI 15)
 * Tight per-ray limits and a miss test from a bit grid of the occupied space, as the input of the limits entry points above.
 * The grid: G^3 cells (2 <= G <= 256) over the cube [-box_side/2, box_side/2]^3 in the world frame; cell (ix, iy, iz) is the box
 * [plane(i), plane(i+1)] per axis, plane(i) = -box_side/2 + float(i) * (box_side / float(G)) in fp32, every operation rounded on
 * its own.  bits [B][G][G][W] int32, W = (G + 31) / 32: bit (iz & 31) of word (iz >> 5) at [b][ix][iy]; padding bits are 0.
 *
 * hfagp_ray_limits_grid: rays [B][R][3] (directions of any length, t in units of d) against grid b of bits.  A cell COUNTS for a ray
 * iff its bit is set and the ray's slab interval with it — the formula of hfagp_ray_limits_box on the cell's planes — has a positive
 * chord at t >= 0: far_c > max(near_c, 0).  On an axis with d_k == 0 the ray lies in the half-open slab plane(i) <= o_k < plane(i+1)
 * of one i; o_k <= plane(0) or o_k >= plane(G) there empties the ray (the box entry's 0 * inf case included).
 *   t_near = min over the counting cells of max(near_c, 0)  — the entry of the FIRST occupied cell, 0 for an origin inside one;
 *   t_far  = max over the counting cells of far_c           — the exit of the LAST occupied cell.
 * A ray without a counting cell, with a zero direction, with a NaN component or with a limit that is not finite gets
 * (+inf, -inf): an EMPTY ray.  Cells are found by a 3-D DDA bounded at 3 G + 3 steps; every reported t is recomputed from its
 * integer plane index, never accumulated.  One launch, one thread per ray.  To use ONE grid for several frames pass B = 1 and
 * R = the total ray count.
 * HFAGP_EBADARG: a NULL pointer, B or R <= 0, B * R >= 2^31, G outside 2 .. 256, box_side not positive and finite.                */
int hfagp_ray_limits_grid(const float* ray_origins, const float* ray_directions, const int32_t* bits, float* t_near, float* t_far,
                          int32_t B, int32_t R, int32_t G, float box_side, void* stream);
/* A density lattice -> bits.  volume [B][n][n][n] fp32, n = G * oversample + 1 lattice points per axis over the cube (z fastest;
 * lattice point i * oversample lies on plane(i)): cell (ix, iy, iz) is occupied iff one of the (oversample + 1)^3 lattice points of
 * its closed extent has !(v < level) — faces are shared with the neighbours (conservative), a NaN is occupied — and its bit is
 * set iff a cell within Chebyshev distance `dilate` of it (clipped at the cube) is occupied.  bits as above: written, padding 0.
 * One launch, no atomics: a wave owns the words of one [b][ix][iy] column and writes them with plain stores.
 * HFAGP_EBADARG: a NULL pointer, B <= 0, G outside 2 .. 256, oversample < 1 or G * oversample + 1 > 1025, dilate outside 0 .. 8,
 * level NaN.                                                                                                                   */
int hfagp_occupancy_pack(const float* volume, int32_t* bits, int32_t B, int32_t G, int32_t oversample, float level,
                         int32_t dilate, void* stream);

/* ------------------------------------------------------------------ per-sample compositing weights of ray lists (additive to ABI 15)
 * The distribution along every ray of a list, which the entry points above compute and reduce to one number per ray: with
 * S = Sc + Sf samples sorted by depth, t_0 <= .. <= t_{S-1}, the compositing weight w_e = alpha_e T_e of interval [t_e, t_{e+1}],
 * e = 0 .. S-2 — for distortion and depth-distribution losses, median / quantile depth, depth variance, transmittance at a depth.
 *   weights[ray][e] = w_e, the very values the kernel composites feat, wsum (= sum_e w_e) and depth (= sum_e w_e tbar_e / wsum,
 *                     tbar_e = (t_e + t_{e+1}) / 2) with; white_back does not enter;
 *   depths[ray][s]  = t_s, by SORTED position (not sample id).
 * hfagp_raymarch_rays_samples_fwd is hfagp_raymarch_rays_fwd (lim NULL) or hfagp_raymarch_rays_limits_fwd (lim given) with these two
 * more outputs; every other output has the bits of that call.  An EMPTY ray (see HfagpRayLimits) gets S-1 zeros and S zeros.
 * hfagp_raymarch_rays_samples_bwd is hfagp_raymarch_rays_bwd / _limits_bwd with g_weights [B][R][Sc+Sf-1] = dL/d weights as one more
 * addend of pass 1's per-interval adjoint (see HfagpRaymarchGeomGrads):
 *     G_e = g . cbar_e  -  white_back * sum(g)  +  gamma_W  +  gamma_d * (tbar_e - d) / W  +  g_weights[e]
 * The depths carry no gradient (importance depths are detached as in EG3D, stratified ones are constants), so all that follows
 * G_e is unchanged, and the rays' gradient of the term comes from hfagp_raymarch_rays_bwd_rays / _limits_bwd_rays on the records
 * this call wrote.  g_weights of an empty ray is not read.  g_weights alone is an upstream gradient: a->bwd.g_feat and g (or its
 * members) may all be NULL.
 * HFAGP_EBADARG, nothing launched: out or one of its members NULL; g_weights NULL; lim non-NULL with a NULL member; then the checks
 * of the list entry point with (lim given) or without limits.                                                                  */
typedef struct {
    float* weights;               /* [B][R][Sc+Sf-1] */
    float* depths;                /* [B][R][Sc+Sf]   */
} HfagpRaySamples;
int hfagp_raymarch_rays_samples_fwd(const HfagpRayListArgs* a, const HfagpRayLimits* lim /* NULL: config interval */,
                                    const HfagpRaySamples* out, void* stream);
int hfagp_raymarch_rays_samples_bwd(const HfagpRayListBwdArgs* a, const HfagpRayLimits* lim /* NULL ok */,
                                    const HfagpRaymarchGeomGrads* g /* NULL ok */, const float* g_weights, void* stream);

/* ------------------------------------------------------------------ surface normals along ray lists (additive to ABI 15)
 * hfagp_raymarch_normals, hfagp_raymarch_normals_bwd and the per-ray part of hfagp_raymarch_normals_bwd_camera on the rays of a
 * list: the formulas are those entries', with sample s of ray i at origin_i + t_s * direction_i (directions as given) and R rays
 * per frame.  list->base.state is the state hfagp_raymarch_rays_fwd / hfagp_raymarch_rays_limits_fwd filled on the same list
 * ([B][R][(Sc + Sf) * HFAGP_RAYMARCH_STATE_FLOATS_PER_SAMPLE]); the forward's outputs in `base` are not read.  The sample depths
 * and the limits carry no gradient.  (One difference in arithmetic: with the 16-bit decoder hfagp_raymarch_rays_normals_bwd forms
 * a = W0'^T dH in fp32, as hfagp_raymarch_normals_bwd_camera does, not from split-bf16 parts as hfagp_raymarch_normals_bwd.)
 * lim: NULL = the list was marched on the config's [ray_start, ray_end]; else the limits of that forward call, and a ray that is
 * EMPTY by them (see HfagpRayLimits) has no state: nothing of it is read,
 *   hfagp_raymarch_rays_normals            writes three zeros for it,
 *   hfagp_raymarch_rays_normals_bwd        skips it (its g_normal is not read),
 *   hfagp_raymarch_rays_normals_bwd_rays   writes six zeros for it, or leaves its six floats alone when accumulating.
 * normal [B][R][3]: written.  d_planes and the four decoder gradients (all or none): ACCUMULATED into, as in the grid entry — after
 * hfagp_raymarch_rays_bwd where they share d_planes (that call overwrites plane 2 on mirrored planes).  d_origins, d_directions
 * [B][R][3] (the layout of hfagp_raymarch_rays_bwd_rays): written, or with accumulate != 0 added to, so that the normal term joins
 * the colour term's; no reduction follows.  One writer per ray in the first and the third: two calls give the same bits.
 * HFAGP_EBADARG, nothing launched: list, its state or an output NULL; lim non-NULL with a NULL member; one decoder gradient without
 * the others; then the checks of hfagp_raymarch_rays_fwd (with lim: minus ray_end > ray_start).                                */
int hfagp_raymarch_rays_normals(const HfagpRayListArgs* list, const HfagpRayLimits* lim, float* normal /* [B][R][3] */, void* stream);
int hfagp_raymarch_rays_normals_bwd(const HfagpRayListArgs* list, const HfagpRayLimits* lim, const float* g_normal /* [B][R][3] */,
                                    float* d_planes, float* d_dec_w0, float* d_dec_b0, float* d_dec_w1, float* d_dec_b1, void* stream);
int hfagp_raymarch_rays_normals_bwd_rays(const HfagpRayListArgs* list, const HfagpRayLimits* lim, const float* g_normal /* [B][R][3] */,
                                         float* d_origins, float* d_directions, int accumulate, void* stream);

/* ------------------------------------------------------------------ antialiased resample (additive to ABI 15)
 * SuperresolutionHybrid8XDC's F.interpolate(mode='bilinear', align_corners=False, antialias=True) of the feature image and the
 * raw RGB when the rays were marched at another resolution than the super-resolution input (neural_rendering_resolution), on
 * the channels-last feature image, and its adjoint.  The resize is separable; per axis n_in -> n_out, with s = n_in / n_out,
 * support = max(s, 1) and inv = 1 / max(s, 1), output i reads the inputs
 *     j in [lo, hi),  lo = max(0, (int)(c - support + 0.5)),  hi = min(n_in, (int)(c + support + 0.5)),  c = s (i + 0.5)
 * with the weights  w_j = max(0, 1 - |(j - c + 0.5) inv|)  divided by their sum (torch's _upsample_bilinear2d_aa).
 * The kernels compute NO weights: the caller builds one table per axis (in double, stored as fp32) and passes them in.
 * A table has one row of 2 + kmax 32-bit words per DESTINATION index of its axis: int32 start, int32 count, then kmax floats —
 * destination d sums  weight[k] * source[start + k]  over k < count.  Forward: Ho rows (table_h) and Wo rows (table_w) as above.
 * Adjoint: the TRANSPOSED tables, Hi and Wi rows — per input index the consecutive outputs that read it and the same
 * (normalised) weights: a gather, every element of dst written exactly once, no atomics, no memset, a fixed summation order
 * (two calls give the same bits).  Supported ratios per axis: n_out / 4 <= n_in <= 4 n_out (at most HFAGP_RESIZE_AA_KMAX taps
 * per output and readers per input).  Rows must satisfy 0 <= start, start + count <= source extent (a count is cut to what
 * fits: nothing is read out of bounds).
 * HFAGP_EBADARG, nothing launched: a, src, dst or a table NULL.  HFAGP_EUNSUPPORTED: C not a multiple of 4, an empty extent
 * (B, Hi, Wi, Ho, Wo or C <= 0), a ratio outside the range, kmax < 1 or > HFAGP_RESIZE_AA_KMAX, 2^31 or more float4 outputs.    */
#define HFAGP_RESIZE_AA_KMAX 9
typedef struct {
    const float* src;          /* forward: x [B][Hi][Wi][C];  adjoint: g_y [B][Ho][Wo][C] */
    float* dst;                /* forward: y [B][Ho][Wo][C];  adjoint: g_x [B][Hi][Wi][C] (written, not accumulated) */
    const float* add_nchw3;    /* adjoint only, may be NULL: [B][3][Hi][Wi], added to channels 0..2 of g_x in the same pass (the
                                  gradient of image_raw = those channels of the unresampled feature image); forward: ignored */
    const int32_t* table_h;    /* rows of the vertical axis:   forward [Ho][2 + kmax], adjoint [Hi][2 + kmax] */
    const int32_t* table_w;    /* rows of the horizontal axis: forward [Wo][2 + kmax], adjoint [Wi][2 + kmax] */
    int32_t B, Hi, Wi, Ho, Wo, C;
    int32_t kmax;              /* weights per table row */
} HfagpResizeAaArgs;

int hfagp_resize_aa_fwd(const HfagpResizeAaArgs* a, void* stream);
int hfagp_resize_aa_bwd(const HfagpResizeAaArgs* a, void* stream);

/* ------------------------------------------------------------------ gradients w.r.t. the generator weights
 * (needed once HFA-GP calls tune_generator(), trainer_rgb.py:69-71)                                       */

/* dweight[Cout][Cin][k][k] = conv-weight-gradient( x * styles , g )  -  weight * sum_b dd d^3 styles^2
 * (second term: through the demodulation coefficients; dd may be NULL).
 *   mode HFAGP_CONV3X3      : g = gradient w.r.t. the raw conv output            [B][H][W][Cout]
 *   mode HFAGP_CONVT3X3_UP2 : g = parity images from hfagp_upfir_bwd             [2][2][B][H+1][W+1][Cout]
 *   mode HFAGP_CONV1X1      : g = gradient w.r.t. the toRGB output               [B][H][W][Cout]            */
typedef struct {
    const float* x;           /* [B][H][W][Cin] layer input */
    const float* styles;      /* [B][Cin] or NULL */
    const float* g;
    const float* weight;      /* [Cout][Cin][k][k] */
    const float* dd;          /* [B][Cout] or NULL */
    const float* dcoef;       /* [B][Cout] */
    float*       dweight;     /* out [Cout][Cin][k][k] (overwritten) */
    float*       workspace;   /* >= hfagp_wgrad_workspace_bytes() */
    int32_t B, H, W, Cin, Cout, mode;
    int32_t ksplit;           /* number of split-K slabs over (b, position tiles); >= 1 */
    int32_t precision;        /* HFAGP_PREC_F32 (exact fp32 MFMA) or HFAGP_PREC_BF16X3: modes 0 and 1 with Cin, Cout    */
                              /* multiples of 64 (mode 1 also Cin = 32) then run on the split-bf16 MFMA kernels, the rest fp32 */
                              /* (the one predicate: wgrad_split16, csrc/wgrad_plan.h; hfagp_wgrad_ksplit follows it)          */
    int32_t accumulate;       /* ABI 11: 1 = dweight += (the parameter's .grad slice: no separate add pass), 0 = overwrite */
    int32_t dd_stride;        /* ABI 12: row stride of dd in elements (0 = Cout): row 3 of hfagp_pointwise_bwd's sums without a copy */
} HfagpWgradArgs;

/* ABI 11: the library's split-K choice for this layer (everything but `ksplit` / `workspace` filled in): one block per CU for the
 * kernel that will run (64 x 64 (ci, co) tiles), never more slabs than position tiles */
int32_t hfagp_wgrad_ksplit(const HfagpWgradArgs* a);
size_t hfagp_wgrad_workspace_bytes(const HfagpWgradArgs* a);
int hfagp_conv_wgrad(const HfagpWgradArgs* a, void* stream);

/* affine layer: dA[Cin][w_dim] += dstot^T . w / sqrt(w_dim);  db[Cin] += sum_b dstot   (dstot from hfagp_style_bwd) */
int hfagp_affine_grad(const float* dstot, const float* w, float* dA, float* db, int32_t B, int32_t Cin, int32_t w_dim,
                      int32_t w_stride, void* stream);

/* ABI 12: the same for up to 32 affine layers in one launch (every dA / db accumulated into: the .grad slices themselves) */
typedef struct {
    const float* dstot;       /* [B][Cin] */
    const float* w;           /* row view [B][w_dim] of ws, row stride w_stride */
    float*       dA;          /* [Cin][w_dim] += */
    float*       db;          /* [Cin] += */
    int32_t B, Cin, w_dim, w_stride;
} HfagpAffineGradItem;
int hfagp_affine_grad_batch(const HfagpAffineGradItem* items, int32_t n, void* stream);

/* ABI 12: bias and noise-strength gradients of up to 32 synthesis layers in one launch, from the reductions hfagp_pointwise_bwd
 * (param_grads = 1) left in sums [B][10][C]:  dbias[c] += sum_b sums[b][4][c],  dnoise[0] += sum_{b,c} sums[b][5][c]
 * (either pointer may be NULL); fixed summation order.  Replaces two framework reductions + adds per layer.                  */
typedef struct {
    const float* sums;
    float*       dbias;
    float*       dnoise;
    int32_t B, C;
} HfagpBiasNoiseGradItem;
int hfagp_bias_noise_grads(const HfagpBiasNoiseGradItem* items, int32_t n, void* stream);

/* out[c] (+)= sum over npix rows of a [npix][C] channels-last tensor (C <= 256); partial: [nblocks][C] workspace;
 * ABI 11: nblocks * 256 must be a multiple of C (the tensor is walked as a flat array and a thread keeps its channel) */
int hfagp_channel_sum(const float* g, float* partial, float* out, int64_t npix, int32_t C, int32_t nblocks,
                      int32_t accumulate, void* stream);

/* ------------------------------------------------------------------ loss side of the fitting step
 * trainer_rgb.py:84-86 / trainer_3dmm.py:51-53 / trainer_audio.py:97-99:
 *   pooled = AdaptiveAvgPool2d((h, w))(img)  with img [BC][f*h][f*w] (NCHW, BC = B*C, integer factor f),
 *   loss   = mean((real - pooled)^2)          (MSELoss(reduction='mean'); deterministic reduction order)
 * and its adjoint  d_img = g_loss * 2 (pooled - real) / (BC*h*w * f^2)  (every element of d_img is written).
 * workspace: hfagp_pool_mse_workspace_bytes() bytes; loss, g_loss: one float on the device.              */
size_t hfagp_pool_mse_workspace_bytes(void);

/* ABI 11: torch.optim.Adam's update (trainer_rgb.py:58; no weight decay, no amsgrad) of MANY tensors in one call.
 *   tensor_table: device memory, ntensors x 6 64-bit words {param*, grad*, exp_avg*, exp_avg_sq*, step* (ONE float, advanced by
 *                 this call), numel};   chunk_table: device memory, nchunks x {int32 tensor index, int32 first element}, one entry
 *                 per hfagp_adam_chunk() elements of every tensor.  All tensors fp32, contiguous. */
int hfagp_adam_step(const void* tensor_table, const void* chunk_table, int32_t ntensors, int32_t nchunks, double lr, double beta1,
                    double beta2, double eps, void* stream);      /* (doubles: torch forms 1 - beta and the bias corrections in double) */
int32_t hfagp_adam_chunk(void);
int hfagp_pool_mse_fwd(const float* img, const float* real, float* pooled, float* loss, float* workspace,
                       int32_t BC, int32_t h, int32_t w, int32_t f, void* stream);
int hfagp_pool_mse_bwd(const float* pooled, const float* real, const float* g_loss, float* d_img,
                       int32_t BC, int32_t h, int32_t w, int32_t f, void* stream);

/* The same pass with a per-pixel weight at the loss resolution (masked / region-weighted fits; additive to ABI 15):
 *   img [B][C][f*h][f*w], real and pooled [B][C][h][w], weight [B][1][h][w] (finite, >= 0, values above 1 allowed; broadcast over C)
 *   pooled = AdaptiveAvgPool2d((h, w))(img)                       (written unmasked)
 *   N_b    = sum over c, y, x of weight_b(y,x) (real - pooled)^2,   D_b = C * sum over y, x of weight_b(y,x)
 *   loss   = (1/B) sum over b of (D_b > 0 ? N_b / D_b : 0)         (normalised PER FRAME; deterministic reduction order, no atomics)
 *   d_img[b,c,Y,X] = g_loss * 2 weight_b(y,x) (pooled - real) / (B D_b f^2)      (every element of d_img is written)
 * Where weight == 0 or D_b == 0 the pixel adds exactly 0 to N_b and its d_img is exactly +0.0 — a branch, not a product: NaN / inf
 * in img or real under zero weight reach neither.  A negative or non-finite weight is not checked (no host sync): undefined loss.
 * inv_d: B floats on the device, written by _fwd (1 / D_b, 0 for a frame without weight) and read by _bwd;
 * workspace: hfagp_pool_wmse_workspace_bytes(B) bytes; loss, g_loss: one float on the device; 1 <= B <= 65535.
 * hfagp_pool_wmse_sweep_elements(): elements of ONE frame (C*h*w) that one sweep of the forward launch covers; a larger frame takes
 * further sweeps of the same blocks. */
size_t hfagp_pool_wmse_workspace_bytes(int32_t B);
int64_t hfagp_pool_wmse_sweep_elements(void);
int hfagp_pool_wmse_fwd(const float* img, const float* real, const float* weight, float* pooled, float* loss, float* inv_d,
                        float* workspace, int32_t B, int32_t C, int32_t h, int32_t w, int32_t f, void* stream);
int hfagp_pool_wmse_bwd(const float* pooled, const float* real, const float* weight, const float* inv_d, const float* g_loss,
                        float* d_img, int32_t B, int32_t C, int32_t h, int32_t w, int32_t f, void* stream);

/* ------------------------------------------------------------------ standalone ops (NCHW, test surface) */
int hfagp_upfirdn2d_fwd(const float* x, const float* f, float* y,
                        int32_t N, int32_t C, int32_t H, int32_t W, int32_t fh, int32_t fw,
                        int32_t up, int32_t down, int32_t px0, int32_t px1, int32_t py0, int32_t py1,
                        float gain, void* stream);

int hfagp_bias_act_fwd(const float* x, const float* b, float* y, int64_t n, int32_t C, int64_t inner,
                       int32_t act, float alpha, float gain, float clamp, void* stream);
/* adjoints of the two operators above (EG3D's upfirdn2d / bias_act are differentiable):
 *   hfagp_upfirdn2d_bwd: dx [N][C][H][W] from dy [N][C][Ho][Wo]; H, W, up, down, padding: those of the FORWARD call
 *   hfagp_bias_act_bwd:  dx = dy * gain * (y < 0 ? alpha : 1) where |y| < clamp, else 0, from the forward OUTPUT y
 *                        (d bias = sum of dx over everything but the channel: the caller's reduction)               */
int hfagp_upfirdn2d_bwd(const float* dy, const float* f, float* dx, int32_t N, int32_t C, int32_t H, int32_t W,
                        int32_t fh, int32_t fw, int32_t up, int32_t down, int32_t px0, int32_t px1, int32_t py0,
                        int32_t py1, float gain, void* stream);
int hfagp_bias_act_bwd(const float* dy, const float* y, float* dx, int64_t n, int32_t act, float alpha, float gain,
                       float clamp, void* stream);

/* Blur(pad (1,1)) of the FIR [1,3,3,1] x [1,3,3,1] / 64 followed by stride-2 sampling, channels-last — the front of the 1x1
 * skip convolution of the RGB driver's ResBlock (/root/reference/code/networks/encoder3d.py:215, ConvLayer(..., 1,
 * downsample=True)): y[b][i][j][c] = sum_ab f[a] f[b] x[b][2i + a - 1][2j + b - 1][c], zero outside; H, W even, C % 4 == 0.
 * hfagp_blur_down_bwd is its adjoint (gx [B][H][W][C] from gy [B][H/2][W/2][C]).                                     */
int hfagp_blur_down_fwd(const float* x, float* y, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int hfagp_blur_down_bwd(const float* gy, float* gx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);

/* layout helpers */
int hfagp_nchw_to_nhwc(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);
int hfagp_nhwc_to_nchw(const float* x, float* y, int32_t B, int32_t C, int32_t H, int32_t W, void* stream);

/* ------------------------------------------------------------------ the path's one exchange step, for non-PyTorch hosts
 * In-place all-reduce (sum, or mean when average != 0) of n floats at `buf` over the ranks of `comm`, an RCCL communicator
 * (ncclComm_t) the HOST created, enqueued on `stream`: the per-step reduction of the shared gradient buffer
 * [bases | delta | driver net | generator when tuned] that HFA-GP gets from DistributedDataParallel
 * (/root/reference/code/train_rgb.py:53-57,196-202; trainer_3dmm.py:29).  PyTorch hosts use torch.distributed instead
 * (hfa_gp_amd.trainer.FlatGrads / BucketedAllReduce).  The library does not link RCCL: ncclAllReduce is resolved from the
 * running process (or librccl.so on the loader path) at the first call; HFAGP_EUNSUPPORTED when it cannot be found.     */
int hfagp_allreduce_f32(void* buf, size_t n, void* comm, int32_t average, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HFAGP_H_ */
