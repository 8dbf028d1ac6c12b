"""The weighted pool + MSE pass (hfagp_pool_wmse_fwd / _bwd, ops.pool_wmse) against its definition in float64 on the CPU, its
properties (bit-repeatable, zero weight is a branch, +0.0 gradients), and `mask=` / `matte=` through the trainer on the device.
Definition, weights and bounds: tests/test_masked_fit_cpu.py.  Needs an MI355X:  python -m pytest tests -m gpu"""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from tests.test_masked_fit_cpu import KINDS, SHAPES, case, disc_matte, ref_wmse, soft_mask, within

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def run(dev, img, real, weight, scale=1.7):
    from hfa_gp_amd import ops
    img_d = img.to(dev).requires_grad_(True)
    loss, pooled = ops.pool_wmse(img_d, real.to(dev), weight.to(dev))
    (grad,) = torch.autograd.grad(loss * scale, img_d)
    return loss.detach(), grad / scale, pooled


def check_against_float64(dev, b, c, h, f, kind):
    img, real, weight = case(b, c, h, f, kind)
    loss, grad, pooled = run(dev, img, real, weight)
    assert not pooled.requires_grad
    assert float((pooled.cpu() - F.adaptive_avg_pool2d(img, h)).abs().max()) <= 1e-6
    within(loss, grad, *ref_wmse(img, real, weight))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,c,h,f", SHAPES + [(2, 3, 256, 2)])          # + the fitting step's own shape
def test_pool_wmse_matches_float64(dev, b, c, h, f, kind):
    check_against_float64(dev, b, c, h, f, kind)


@pytest.mark.parametrize("kind", ["soft", "zero_frame"])
def test_frame_larger_than_one_sweep_of_the_launch(dev, kind):
    """A frame of more elements than the forward launch covers in one sweep (its blocks per frame x threads per block): the
    grid-stride loop runs more than once, and with two frames so does the per-frame partial layout."""
    from hfa_gp_amd import _lib
    sweep = _lib.lib().hfagp_pool_wmse_sweep_elements()
    h = math.isqrt(sweep) + 1                                          # c = 1, f = 1: h * h elements per frame
    assert h * h > sweep and h < 1024
    check_against_float64(dev, 2, 1, h, 1, kind)


@pytest.mark.parametrize("b,c,h,f", [(2, 3, 19, 3), (2, 3, 256, 2)])
def test_second_call_returns_the_same_bits(dev, b, c, h, f):
    img, real, weight = case(b, c, h, f, "soft")
    l1, g1, p1 = run(dev, img, real, weight)
    l2, g2, p2 = run(dev, img, real, weight)
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and torch.equal(p1, p2)


@pytest.mark.parametrize("b,c,h,f", [(3, 3, 17, 1), (2, 3, 16, 4), (2, 3, 256, 2)])
def test_all_ones_weights_against_pool_mse(dev, b, c, h, f):
    from hfa_gp_amd import ops
    img, real, weight = case(b, c, h, f, "ones")
    loss, _, pooled = run(dev, img, real, weight)
    want, pooled_u = ops.pool_mse(img.to(dev), real.to(dev))
    assert abs(float(loss) - float(want)) <= 1e-6 + 1e-5 * abs(float(want))
    assert torch.equal(pooled, pooled_u)


@pytest.mark.parametrize("b,c,h,f", [(2, 3, 16, 2), (2, 3, 19, 3), (3, 3, 17, 1)])
def test_nan_and_inf_under_zero_weight_reach_nothing(dev, b, c, h, f):
    img, real, weight = case(b, c, h, f, "binary")
    weight[-1] = 0                                                      # an empty frame too
    clean_loss, clean_grad, _ = run(dev, img, real, weight)
    off = (weight == 0).expand(-1, c, -1, -1)
    off_img = off.repeat_interleave(f, -1).repeat_interleave(f, -2)
    bad_img, bad_real = img.clone(), real.clone()
    bad_img[off_img] = float("nan")
    bad_real[off] = float("inf")
    bad_img[-1, 0, 0, 0] = float("-inf")
    loss, grad, _ = run(dev, bad_img, bad_real, weight)
    assert torch.isfinite(loss) and torch.equal(loss, clean_loss)
    grad, clean_grad = grad.cpu(), clean_grad.cpu()
    assert torch.equal(grad[~off_img], clean_grad[~off_img])
    assert torch.equal(grad[off_img], torch.zeros_like(grad[off_img])) and not torch.signbit(grad[off_img]).any()


@pytest.mark.parametrize("b,c,h,f", [(2, 3, 16, 2), (2, 3, 19, 3)])
def test_all_zero_weights(dev, b, c, h, f):
    img, real, weight = case(b, c, h, f, "soft")
    loss, grad, _ = run(dev, img, real, torch.zeros_like(weight), scale=-3.0)
    assert float(loss) == 0.0
    from hfa_gp_amd import ops
    img_d = img.to(dev).requires_grad_(True)
    loss, _ = ops.pool_wmse(img_d, real.to(dev), torch.zeros_like(weight).to(dev))
    (-3.0 * loss).backward()                                            # (the sign of the incoming gradient does not leak either)
    assert torch.equal(img_d.grad, torch.zeros_like(img_d.grad)) and not torch.signbit(img_d.grad).any()


def test_bad_weights_raise_and_null_pointers_return_a_code(dev):
    from hfa_gp_amd import _lib, ops
    img, real, weight = case(2, 3, 16, 2, "soft")
    img, real, wd = img.to(dev), real.to(dev), weight.to(dev)
    for bad in (wd[:, :, :8].contiguous(), wd.expand(-1, 3, -1, -1).contiguous(), wd[:1].contiguous(),      # shape
                wd.double(), wd.half(),                                                                       # dtype
                weight,                                                                                       # device
                wd.transpose(-1, -2)):                                                                        # not contiguous
        with pytest.raises((RuntimeError, ValueError, TypeError)):
            ops.pool_wmse(img, real, bad)
    with pytest.raises(RuntimeError, match="requires grad"):
        ops.pool_wmse(img, real, wd.clone().requires_grad_(True))
    h = _lib.lib()
    assert h.hfagp_pool_wmse_fwd(None, None, None, None, None, None, None, 2, 3, 16, 16, 2, None) == -1      # HFAGP_EBADARG
    assert b"null pointer" in h.hfagp_last_error()
    assert h.hfagp_pool_wmse_bwd(None, None, None, None, None, None, 2, 3, 16, 16, 2, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    assert h.hfagp_pool_wmse_fwd(1, 1, 1, 1, 1, 1, 1, 0, 3, 16, 16, 2, None) == -1                           # dims are rejected first
    assert b"bad dims" in h.hfagp_last_error()
    assert h.hfagp_pool_wmse_workspace_bytes(2) >= 2 * 4 * (2 * (h.hfagp_pool_wmse_sweep_elements() // 256) + 1)


# ----------------------------------------------------------------------------- the trainer on the device
class A:
    out_pose = False; person_2 = False; params_len = 76; size = 32; batch_size = 2; lr = 1e-3
    latent_dim_style = 512; latent_dim_shape = 8; generator_preset = "tiny14"; generator_seed = 0      # 64^2 image -> 32^2 loss


def make_trainer(dev, lpips="none"):
    from hfa_gp_amd.trainer import Trainer
    torch.manual_seed(0)
    return Trainer(A(), dev, mode="rgb", lpips=lpips)


def frames(dev):
    from hfa_gp_amd.synthetic import gaussian_labels
    g = torch.Generator().manual_seed(5)
    real = (0.5 * torch.randn(2, 3, 32, 32, generator=g)).clamp(-1, 1).to(dev)
    return real, gaussian_labels(2, dev, seed=3)


def uniforms(tr, dev, b=2):
    cfg = tr.gen.generator.cfg
    g = torch.Generator().manual_seed(9)
    r = cfg.neural_rendering_resolution ** 2
    return dict(u_strat=torch.rand(b, r, cfg.depth_resolution, generator=g).to(dev),
                u_imp=torch.rand(b * r, cfg.depth_resolution_importance, generator=g).to(dev))


def masked_step(tr, dev, fused, **kw):
    """One `gen_update(mask=...)`; → (its return, the gradient that arrived at the generated image, whether ops.pool_wmse ran).
    `fused=False`: ops.pool_wmse is replaced by the torch form of the same definition (`pooled_l2` made to take its fallback)."""
    from hfa_gp_amd import ops
    from hfa_gp_amd.trainer import pooled_l2
    arrived, used = [], {}
    get_image = tr.gen.get_image

    def hooked(*a, **k):
        out = get_image(*a, **k)
        (out["image"] if isinstance(out, dict) else out).register_hook(lambda g: arrived.append(g.detach().clone()))
        return out
    tr.gen.get_image = hooked
    orig = ops.pool_wmse

    def torch_form(img, real, weight):
        used["fused"] = True
        return pooled_l2(nn.AdaptiveAvgPool2d(real.shape[-2:]), real, img, True, weight)
    ops.pool_wmse = (lambda *a, **k: (used.setdefault("fused", True), orig(*a, **k))[1]) if fused else torch_form
    real, label = frames(dev)
    try:
        out = tr.gen_update(real, label, mask=soft_mask(3, 2).to(dev), **uniforms(tr, dev), **kw)
    finally:
        ops.pool_wmse = orig
        del tr.gen.get_image
    assert len(arrived) == 1
    return out, arrived[0], used.get("fused", False)


@pytest.mark.parametrize("with_lpips", [False, True])
def test_gen_update_with_a_mask_runs_the_fused_pass(dev, with_lpips):
    """`gen_update(mask=)` keeps the L2 term on ops.pool_wmse — without LPIPS and with the 2 x 2 pool folded into LPIPSAlex — and
    the gradient that arrives at the generated image is the one the torch form of the definition sends there (compared at the
    image: the ray-march backward behind it is not bit-repeatable)."""
    from hfa_gp_amd.lpips_alex import LPIPSAlex

    def lp():
        torch.manual_seed(1234)
        return LPIPSAlex().to(dev) if with_lpips else "none"
    (l2, lpv, img), got, used = masked_step(make_trainer(dev, lp()), dev, fused=True)
    assert used, "the masked L2 term must stay on the fused weighted pool + MSE pass"
    assert img.shape == (2, 3, 32, 32) and torch.isfinite(l2) and torch.isfinite(lpv) and (float(lpv) > 0) == with_lpips
    real, _ = frames(dev)
    want_l2, _ = ref_wmse(img.cpu(), real.cpu(), soft_mask(3, 2))
    assert abs(float(l2) - float(want_l2)) <= 1e-6 + 1e-5 * abs(float(want_l2))
    (l2_t, _, _), want, used_t = masked_step(make_trainer(dev, lp()), dev, fused=False)
    assert used_t and got.shape == want.shape == (2, 3, 64, 64)
    err, bound = float((got - want).abs().max()), 1e-9 + 1e-5 * float(want.abs().max())
    print(f"d image: max err {err:.3e} (bound {bound:.3e}), l2 {float(l2):.6e} / {float(l2_t):.6e}")
    assert float(want.abs().max()) > 0 and err <= bound


def test_gen_update_with_mask_and_matte_frozen_and_tuned(dev):
    tr = make_trainer(dev)
    real, label = frames(dev)
    mask, matte = soft_mask(3, 2).to(dev), disc_matte(2).to(dev)
    l2, lpv, img = tr.gen_update(real, label, mask=mask, matte=matte)
    sil = tr.last_silhouette
    assert sil.shape == () and sil.is_cuda and not sil.requires_grad and torch.isfinite(sil) and float(sil) > 0
    assert torch.isfinite(l2) and img.shape == (2, 3, 32, 32) and float(tr.gen.bases.grad.abs().sum()) > 0
    tr.tune_generator()
    w0 = tr.gen.generator.backbone.synthesis.b8.conv1.weight.detach().clone()
    _, label = frames(dev)
    l2, _, _ = tr.gen_update(real, label, mask=mask, matte=matte)
    assert torch.isfinite(l2) and torch.isfinite(tr.last_silhouette) and float(tr.gen.bases.grad.abs().sum()) > 0
    assert not torch.equal(tr.gen.generator.backbone.synthesis.b8.conv1.weight.detach(), w0)
    tr.gen_update(real, frames(dev)[1])
    assert tr.last_silhouette is None


def test_fit_frames_with_masks_and_mattes(dev):
    from hfa_gp_amd import ops
    from hfa_gp_amd.trainer import fit_frames
    tr = make_trainer(dev)
    real, label = frames(dev)
    reals, labels = torch.cat([real, real.flip(0)]), torch.cat([label, label.flip(0)])
    calls = []
    orig = ops.pool_wmse
    ops.pool_wmse = lambda *a, **k: (calls.append(1), orig(*a, **k))[1]
    try:
        losses = fit_frames(tr, reals, labels, epochs=1, batch=2, masks=soft_mask(3, 4).to(dev), mattes=disc_matte(4).to(dev))
    finally:
        ops.pool_wmse = orig
    assert len(losses) == 2 and len(calls) == 2 and all(torch.isfinite(v) for v in losses)
    assert float(tr.last_silhouette) > 0
