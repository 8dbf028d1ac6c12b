"""Host side of multi-view synthesis (no GPU): the turntable cameras, the label flip on a [B,V,25] label, a 3-D label through
HeadNeRF_*.get_image, and the trainer step's flattening on the CPU oracle."""
import math

import pytest
import torch

from hfa_gp_amd import cam_utils, headnerf


@pytest.mark.parametrize("n", [1, 2, 8])
def test_orbit_labels(n):
    r, yaw, pitch, off = 2.3, 0.4, 0.2, -0.1
    lab = cam_utils.orbit_labels(n, r=r, yaw_range=yaw, pitch_range=pitch, pitch_offset=off)
    assert lab.shape == (n, 25) and lab.dtype == torch.float32
    pos = lab[:, :16].reshape(n, 4, 4)[:, :3, 3]
    assert torch.allclose(pos.norm(dim=-1), torch.full((n,), r), atol=1e-5)
    assert torch.equal(lab[:, 16:], torch.tensor(cam_utils.FFHQ_INTRINSICS).expand(n, -1))
    for i in range(n):
        h = math.pi / 2 + yaw * math.sin(2 * math.pi * i / n)
        v = math.pi / 2 + off + pitch * math.cos(2 * math.pi * i / n)
        p = r * torch.tensor([[math.sin(v) * math.cos(h), math.cos(v), math.sin(v) * math.sin(h)]])
        want = cam_utils.make_label(cam_utils.create_cam2world_matrix(-cam_utils.normalize_vecs(p), p))
        assert torch.allclose(lab[i:i + 1], want, atol=1e-5), i
        # the camera looks at the origin: its forward axis (third column; un-flipped labels have it pointing away) is along p
        fwd = lab[i, :16].reshape(4, 4)[:3, 2]
        assert torch.allclose(fwd, p[0] / r, atol=1e-5)
    k = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5, 0.0, 0.0, 1.0)
    assert torch.equal(cam_utils.orbit_labels(2, intrinsics=k)[:, 16:], torch.tensor(k).expand(2, -1))
    with pytest.raises(ValueError):
        cam_utils.orbit_labels(0)


def test_flip_label_on_a_multi_view_label():
    lab = torch.randn(2, 3, 25, generator=torch.Generator().manual_seed(0))
    before = lab.clone()
    out = headnerf.flip_label_(lab)
    assert out is lab
    want = before.clone()
    want[..., headnerf.FLIP_COLUMNS] *= -1
    assert torch.equal(lab, want)
    assert torch.equal(lab[..., [0, 3, 4, 7, 8, 11, 24]], before[..., [0, 3, 4, 7, 8, 11, 24]])


class _Args:
    out_pose = False
    person_2 = False
    params_len = 76
    size = 32
    batch_size = 1
    lr = 3e-4
    latent_dim_style = 512
    latent_dim_shape = 8
    generator_preset = "tiny14"
    generator_seed = 0


def test_get_image_passes_a_multi_view_label_through():
    torch.manual_seed(0)
    gen = headnerf.HeadNeRF_3DMM(_Args(), _Args.size, "cpu", 512, _Args.latent_dim_shape)
    seen = {}

    def stub(ws, c=None, noise_mode="const", **kw):
        seen.update(ws=ws, c=c, kw=kw)
        out = {"image": torch.zeros(c.shape[0], c.shape[1], 3, 8, 8)}
        if kw.get("geometry"):
            out["image_mask"] = torch.zeros(c.shape[0], c.shape[1], 1, 4, 4)
        return out

    gen.generator.synthesis = stub
    lab = cam_utils.orbit_labels(3)[None].repeat(2, 1, 1)
    before = lab.clone()
    latent = gen.get_latent(gen.get_weights(torch.randn(2, 76)))
    img = gen.get_image(latent, lab)
    assert img.shape == (2, 3, 3, 8, 8)
    assert seen["c"] is lab and seen["c"].shape == (2, 3, 25) and seen["ws"].shape == (2, 14, 512)
    assert torch.equal(lab[..., headnerf.FLIP_COLUMNS], -before[..., headnerf.FLIP_COLUMNS])
    out = gen(torch.randn(2, 76), before.clone(), geometry=True)
    assert out["image_mask"].shape == (2, 3, 1, 4, 4)


def test_trainer_step_flattens_views_on_the_cpu_oracle():
    """`gen_update(real [B,V,3,s,s], label [B,V,25], params [B,P])` on the CPU oracle: the loss and the gradients of the step over the
    B·V flattened frames with repeated driver inputs, the image back with the view axis, 4-D inputs untouched."""
    from hfa_gp_amd.trainer import Trainer
    from tests.test_trainer_cpu import Args, OracleGenerator
    from tests.util import look_at_label

    class MultiViewOracle(OracleGenerator):
        def synthesis(self, ws, c=None, noise_mode="const", u_strat=None, u_imp=None, **kw):
            if c.dim() != 3:
                return super().synthesis(ws, c, noise_mode, u_strat, u_imp)
            b, v = c.shape[:2]
            out = super().synthesis(ws.repeat_interleave(v, 0), c.flatten(0, 1), noise_mode, u_strat, u_imp)
            return {k: t.unflatten(0, (b, v)) for k, t in out.items() if k in ("image", "image_raw", "image_depth")}

    def build():
        torch.manual_seed(0)
        gen = headnerf.HeadNeRF_3DMM(Args(), Args.size, "cpu", 512, Args.latent_dim_shape)
        MultiViewOracle.adopt(gen.generator)
        tr = Trainer(Args(), "cpu", mode="3dmm", gen=gen, lpips="none")
        tr.optimizer = torch.optim.SGD(tr.gen.parameters(), lr=0.0)
        return tr

    g = torch.Generator().manual_seed(2)
    real = (0.5 * torch.randn(2, 2, 3, 32, 32, generator=g)).clamp(-1, 1)
    params = torch.randn(2, 76, generator=g)
    label = look_at_label(torch.tensor([1.5, 1.7, 1.4, 1.6]), torch.tensor([1.6, 1.5, 1.55, 1.65]), flipped=False).reshape(2, 2, 25)
    mv, flat = build(), build()
    lab = label.clone()
    _, l2_mv, _, img = mv.gen_update(real, lab, params)
    _, l2_flat, _, img_flat = flat.gen_update(real.flatten(0, 1), label.clone().flatten(0, 1), params.repeat_interleave(2, 0))
    assert img.shape == (2, 2, 3, 32, 32) and img_flat.shape == (4, 3, 32, 32)
    assert torch.equal(lab[..., headnerf.FLIP_COLUMNS], -label[..., headnerf.FLIP_COLUMNS])
    assert torch.allclose(img.flatten(0, 1), img_flat, atol=1e-6)
    assert abs(float(l2_mv) - float(l2_flat)) <= 1e-6 * abs(float(l2_flat))
    for name in ("bases", "delta"):
        a, b = getattr(mv.gen, name).grad, getattr(flat.gen, name).grad
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-5 * float(b.abs().max())), name
    with pytest.raises(ValueError):
        mv.gen_update(real.flatten(0, 1), label.clone(), params)          # a 3-D label needs 5-D images
