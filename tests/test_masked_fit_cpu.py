"""Masked fits on the CPU: the torch form of the per-pixel-weighted, per-frame-normalised L2 (`trainer.pooled_l2(weight=)`), the
matte compositing in front of LPIPS, the silhouette term, and `mask=` / `matte=` through the trainers and `fit_frames`.

The definition every check here evaluates in float64 (`ref_wmse`):
    pooled = AdaptiveAvgPool2d((h, w))(img),  N_b = sum_{c,y,x} weight_b (real - pooled)^2,  D_b = C sum_{y,x} weight_b,
    loss = (1/B) sum_b (D_b > 0 ? N_b / D_b : 0);   zero weight is a branch (NaN / inf under it never enter).
Bounds: those of tests/test_gpu_backward.py::test_pool_mse_fused_loss — loss 1e-6 + 1e-5 |ref|, gradient 1e-9 + 1e-5 max|ref|
(float32 torch against float64 stays below 2.1e-7 relative on these shapes and weights: a margin of about 50)."""
import os

import pytest
import torch
import torch.multiprocessing as mp
import torch.nn.functional as F
from torch import nn

from hfa_gp_amd.trainer import fit_frames, matte_composite, pooled_l2
from oracle import eg3d_oracle as O
from tests.test_trainer_cpu import (OracleGenerator, _frame_set, _free_port, frame, make_audio_trainer, make_rgb_trainer,
                                    make_trainer)

SHAPES = [(1, 1, 1, 2), (3, 3, 17, 1), (2, 3, 19, 3), (2, 3, 16, 4), (1, 3, 32, 2)]       # (b, c, h, f)
KINDS = ["soft", "binary", "lip", "ones", "zero_frame"]


def make_weight(kind, b, h, g):
    """[b,1,h,h] float32: uniform-random soft; binary at 0.5; 'lip' (1, and 5 on 10 % of the pixels); all ones; soft with frame 0
    all zero."""
    u = torch.rand(b, 1, h, h, generator=g)
    if kind == "soft":
        return u
    if kind == "binary":
        return (u > 0.5).float()
    if kind == "lip":
        return torch.where(u < 0.1, torch.full_like(u, 5.0), torch.ones_like(u))
    if kind == "ones":
        return torch.ones_like(u)
    assert kind == "zero_frame"
    u[0] = 0
    return u


def case(b, c, h, f, kind, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 31 * h + f)
    img = torch.randn(b, c, h * f, h * f, generator=g)
    real = torch.randn(b, c, h, h, generator=g)
    return img, real, make_weight(kind, b, h, g)


def ref_wmse(img, real, weight):
    """The definition in float64 → (loss, d loss / d img), both float64."""
    img = img.double().requires_grad_(True)
    real, weight = real.double(), weight.double()
    b, c, h, w = real.shape
    pooled = F.adaptive_avg_pool2d(img, (h, w))
    on = weight > 0
    diff = torch.where(on, real - pooled, torch.zeros((), dtype=torch.float64))
    n_b = (weight * diff * diff).sum(dim=(1, 2, 3))
    d_b = c * weight.sum(dim=(1, 2, 3))
    loss = sum(n_b[i] / d_b[i] if float(d_b[i]) > 0 else n_b[i] * 0 for i in range(b)) / b
    (grad,) = torch.autograd.grad(loss, img)
    return loss.detach(), grad


def within(loss, grad, ref_loss, ref_grad):
    el, eg = abs(float(loss) - float(ref_loss)), float((grad.double().cpu() - ref_grad).abs().max())
    bl, bg = 1e-6 + 1e-5 * abs(float(ref_loss)), 1e-9 + 1e-5 * float(ref_grad.abs().max())
    print(f"loss err {el:.3e} (bound {bl:.3e})  grad err {eg:.3e} (bound {bg:.3e})")
    assert el <= bl, (el, bl)
    assert eg <= bg, (eg, bg)


def fallback(img, real, weight):
    img = img.clone().requires_grad_(True)
    pool = nn.AdaptiveAvgPool2d(real.shape[-2:])
    loss, pooled = pooled_l2(pool, real, img, False, weight)
    (grad,) = torch.autograd.grad(loss, img)
    return loss.detach(), grad, pooled.detach()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("b,c,h,f", SHAPES)
def test_fallback_matches_float64(b, c, h, f, kind):
    img, real, weight = case(b, c, h, f, kind)
    loss, grad, pooled = fallback(img, real, weight)
    within(loss, grad, *ref_wmse(img, real, weight))
    assert torch.allclose(pooled, F.adaptive_avg_pool2d(img, h), atol=1e-6)           # returned unmasked


@pytest.mark.parametrize("b,c,h,f", SHAPES)
def test_all_ones_is_the_unweighted_loss(b, c, h, f):
    img, real, weight = case(b, c, h, f, "ones")
    loss, _, _ = fallback(img, real, weight)
    want = F.mse_loss(real.double(), F.adaptive_avg_pool2d(img.double(), h))
    assert abs(float(loss) - float(want)) <= 1e-6 + 1e-5 * abs(float(want))


def test_zero_weight_frame_contributes_zero_and_still_counts_in_the_mean():
    img, real, weight = case(3, 3, 17, 1, "soft")
    full, _, _ = fallback(img[1:], real[1:], weight[1:])                                # frames 1, 2 alone: mean over 2
    weight[0] = 0
    loss, grad, _ = fallback(img, real, weight)
    assert abs(float(loss) - float(full) * 2 / 3) <= 1e-6 + 1e-5 * abs(float(full))     # divided by B = 3
    assert torch.equal(grad[0], torch.zeros_like(grad[0]))
    zero, gz, _ = fallback(img, real, torch.zeros_like(weight))
    assert float(zero) == 0.0 and torch.equal(gz, torch.zeros_like(gz))


@pytest.mark.parametrize("b,c,h,f", [(2, 3, 16, 2), (2, 3, 19, 3), (3, 3, 17, 1)])
def test_nan_and_inf_under_zero_weight_reach_nothing(b, c, h, f):
    img, real, weight = case(b, c, h, f, "binary")
    weight[-1] = 0                                                                      # an empty frame too
    clean_loss, clean_grad, _ = fallback(img, real, weight)
    off = (weight == 0).expand(-1, c, -1, -1)
    off_img = off.repeat_interleave(f, -1).repeat_interleave(f, -2)
    bad_img, bad_real = img.clone(), real.clone()
    bad_img[off_img] = float("nan")
    bad_real[off] = float("inf")
    bad_img[-1, 0, 0, 0] = float("-inf")
    loss, grad, _ = fallback(bad_img, bad_real, weight)
    assert torch.equal(loss, clean_loss)
    assert torch.equal(grad[~off_img], clean_grad[~off_img])
    assert torch.equal(grad[off_img], torch.zeros_like(grad[off_img]))


def test_weight_is_validated():
    img, real, weight = case(2, 3, 16, 2, "soft")
    pool = nn.AdaptiveAvgPool2d(16)
    with pytest.raises(ValueError):
        pooled_l2(pool, real, img, False, weight[:, :, :8])
    with pytest.raises(ValueError):
        pooled_l2(pool, real, img, False, weight.double())
    with pytest.raises(RuntimeError, match="requires grad"):
        pooled_l2(pool, real, img, False, weight.clone().requires_grad_(True))


# ----------------------------------------------------------------------------- trainers
class GeometryOracle(OracleGenerator):
    """TEST INFRASTRUCTURE: the CPU oracle generator of test_trainer_cpu with the `geometry=True` key the product generator has —
    'image_mask' [B,1,r,r] is the opacity the oracle's renderer returns next to colour and depth (differentiable)."""

    def synthesis(self, ws, c=None, geometry=False, **kw):
        seen, orig = [], O.importance_renderer

        def spy(*a, **k):
            out = orig(*a, **k)
            seen.append(out[2])
            return out
        O.importance_renderer = spy
        try:
            out = super().synthesis(ws, c, **kw)
        finally:
            O.importance_renderer = orig
        if geometry:
            r = self.cfg.neural_rendering_resolution
            out["image_mask"] = seen[0].permute(0, 2, 1).reshape(ws.shape[0], 1, r, r)
        return out


def with_geometry(tr):
    tr.gen.generator.__class__ = GeometryOracle
    return tr


def soft_mask(seed, n=1, s=32):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(n, 1, s, s, generator=g)
    m[:, :, : s // 4] = 0                      # a band without weight
    m[:, :, -4:, -4:] = 3.0                    # and a region above 1
    return m


def disc_matte(n=1, s=32):
    y, x = torch.meshgrid(torch.linspace(-1, 1, s), torch.linspace(-1, 1, s), indexing="ij")
    return ((x * x + y * y) < 0.5).float()[None, None].repeat(n, 1, 1, 1)


def test_gen_update_takes_mask():
    tr = make_trainer()
    real, label, params = frame(2)
    mask = soft_mask(3)
    out = tr.gen_update(real, label, params, mask=mask)
    assert len(out) == 4 and out[0].shape == (1,) and out[3].shape == (1, 3, 32, 32)          # arity unchanged (3dmm mode)
    want, _ = ref_wmse(out[3], real, mask)
    assert abs(float(out[1]) - float(want)) <= 1e-6 + 1e-5 * abs(float(want))
    assert tr.last_silhouette is None
    assert tr.gen.bases.grad.abs().sum() > 0


def test_gen_update_takes_mask_and_matte():
    tr = with_geometry(make_trainer())
    real, label, params = frame(2)
    mask, matte = soft_mask(3), disc_matte()
    b0 = tr.gen.bases.detach().clone()
    out = tr.gen_update(real, label, params, mask=mask, matte=matte)
    assert len(out) == 4
    want, _ = ref_wmse(out[3], real, mask)
    assert abs(float(out[1]) - float(want)) <= 1e-6 + 1e-5 * abs(float(want))
    sil = tr.last_silhouette
    assert sil.shape == () and not sil.requires_grad and torch.isfinite(sil) and float(sil) > 0
    assert not torch.equal(tr.gen.bases.detach(), b0)
    # the term is in the loss: the same step without it leaves another gradient
    g_with = tr.gen.bases.grad.clone()
    tr2 = with_geometry(make_trainer())
    real, label, params = frame(2)
    tr2.gen_update(real, label, params, mask=mask, matte=matte, silhouette_weight=0.0)
    assert tr2.last_silhouette is None
    assert not torch.equal(tr2.gen.bases.grad, g_with)
    # matte alone, and the step after it without keywords forgets the value
    tr.gen_update(real, label.clone(), params, matte=matte)
    assert float(tr.last_silhouette) > 0
    tr.gen_update(real, label.clone(), params)
    assert tr.last_silhouette is None


def test_return_arity_in_rgb_mode_and_the_audio_trainer():
    tr = with_geometry(make_rgb_trainer())
    real, label, _ = frame(2)
    out = tr.gen_update(real, label, mask=soft_mask(3), matte=disc_matte())
    assert len(out) == 3 and out[2].shape == (1, 3, 32, 32) and float(tr.last_silhouette) > 0
    out = tr.gen_update(real[:0], label[:0], mask=soft_mask(3)[:0], matte=disc_matte()[:0])   # an empty batch ignores both
    assert len(out) == 3 and tr.last_silhouette is None
    at = make_audio_trainer()
    with_geometry(at)
    for step in (0, 5):                                                                        # both smoothing branches
        out = at.gen_update(real, label.clone(), None, global_step=step, img_i=3, mask=soft_mask(3), matte=disc_matte())
        assert len(out) == 4 and float(out[0]) == 0.0 and out[3].shape == (1, 3, 32, 32)
        want, _ = ref_wmse(out[3], real, soft_mask(3))
        assert abs(float(out[1]) - float(want)) <= 1e-6 + 1e-5 * abs(float(want))
        assert torch.isfinite(at.last_silhouette) and float(at.last_silhouette) > 0


def test_no_keywords_is_the_old_step():
    a, b = make_trainer(seed=4), make_trainer(seed=4)
    real, label, params = frame(6)
    oa = a.gen_update(real, label.clone(), params)
    ob = b.gen_update(real, label.clone(), params, mask=None, matte=None)
    assert all(torch.equal(x, y) for x, y in zip(oa, ob))
    for (n, p), q in zip(a.gen.named_parameters(), b.gen.parameters()):
        assert torch.equal(p, q), n


class RecordingLPIPS:
    """Stands in for an LPIPS callable: keeps what it was handed, returns a differentiable per-frame value."""

    def __init__(self, accepts_unpooled):
        self.accepts_unpooled = accepts_unpooled
        self.calls = []

    def __call__(self, real, fake):
        self.calls.append((real.detach().clone(), fake.detach().clone()))
        if fake.shape[-1] != real.shape[-1]:
            fake = F.adaptive_avg_pool2d(fake, real.shape[-2:])
        return ((real - fake) ** 2).mean(dim=(1, 2, 3))


@pytest.mark.parametrize("folded", [False, True])
def test_lpips_sees_the_image_composited_under_the_matte(folded):
    tr = make_trainer()
    tr.lpips_loss = RecordingLPIPS(folded)
    real, label, params = frame(2)
    mask = soft_mask(3)
    tr.gen_update(real, label, params, mask=mask)
    (seen_real, fake), = tr.lpips_loss.calls
    assert torch.equal(seen_real, real)
    f = 2 if folded else 1
    assert fake.shape == (1, 3, 32 * f, 32 * f)                   # folded: the image at 2x the loss size is handed over
    up = lambda t: t.repeat_interleave(f, -1).repeat_interleave(f, -2)
    off = (up(mask) == 0).expand(-1, 3, -1, -1)
    assert off.any() and torch.equal(fake[off], up(real)[off])
    assert not torch.equal(fake[~off], up(real)[~off])
    assert tr.gen.bases.grad.abs().sum() > 0


def test_composite_commutes_with_the_pool():
    g = torch.Generator().manual_seed(0)
    gen, real, mask = torch.randn(2, 3, 32, 32, generator=g), torch.randn(2, 3, 16, 16, generator=g), soft_mask(1, 2, 16)
    m = mask.clamp(max=1)
    want = m * F.adaptive_avg_pool2d(gen, 16) + (1 - m) * real
    assert torch.allclose(F.adaptive_avg_pool2d(matte_composite(real, gen, mask), 16), want, atol=1e-6)


# ----------------------------------------------------------------------------- ragged shards over two ranks
def _masks(n):
    m = soft_mask(7, n)
    m[2] = 0                      # frame 2 (rank 1's only frame, in the step frame 0 is trained on) carries no weight
    return m


def _masked_fit_worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    try:
        tr = make_trainer(seed=10 + rank, world_size=world, rank=rank)
        tr.optimizer = torch.optim.SGD(tr.gen.parameters(), lr=0.05)
        start = tr.gen.bases.detach().clone()
        reals, labels, params = _frame_set(3)
        losses = fit_frames(tr, reals, labels, params, epochs=1, batch=1, masks=_masks(3))
        out[rank] = {"bases": tr.gen.bases.detach().clone(), "n": len(losses), "start": start,
                     "fc0": tr.gen.weights_3dmm.fc[0].weight.detach().clone(), "l2": [float(v) for v in losses]}
    finally:
        dist.destroy_process_group()


def test_masked_fit_frames_two_ranks_ragged_equals_single_rank_global_batch():
    """test_fit_frames_two_ranks_ragged_equals_single_rank_global_batch with `masks=`, frame 2 without any weight: step 0 trains on
    frames {0, 2}, step 1 on frame 1 alone.  The per-frame normalisation makes the loss a mean over frames, which is what the
    weighted all-reduce mean reproduces: the ranks are bit-equal and agree with a single process on the global batches."""
    world, port = 2, _free_port()
    with mp.Manager() as mgr:
        out = mgr.dict()
        mp.spawn(_masked_fit_worker, args=(world, port, out), nprocs=world, join=True)
        r0, r1 = out[0], out[1]
    assert r0["n"] == 2 and r1["n"] == 2
    assert torch.equal(r0["bases"], r1["bases"]) and torch.equal(r0["fc0"], r1["fc0"])
    assert r1["l2"][0] == 0.0                                                          # the frame without weight
    tr = make_trainer(seed=10)
    tr.optimizer = torch.optim.SGD(tr.gen.parameters(), lr=0.05)
    start = tr.gen.bases.detach().clone()
    assert torch.equal(start, r0["start"])
    reals, labels, params = _frame_set(3)
    masks = _masks(3)
    for idx in ([0, 2], [1]):
        tr.gen_update(reals[idx], labels[idx].clone(), params[idx], mask=masks[idx])
    want, got = tr.gen.bases.detach() - start, r0["bases"] - start
    assert want.abs().max() > 1e-4
    assert (got - want).abs().max() <= 2e-3 * want.abs().max(), ((got - want).abs().max(), want.abs().max())
