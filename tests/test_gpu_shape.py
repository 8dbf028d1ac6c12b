"""Tri-plane point queries (csrc/planes_query.hip, ops.planes_query, TriPlaneGenerator.sample / sample_mixed / density_grid,
HeadNeRF get_shape) against the CPU oracle's sample_from_planes + osg_decoder.  Needs an MI355X:  python -m pytest tests -m gpu

Tolerance as tests/test_gpu_parity.py's renderer cases: max abs <= 2e-5 * max(1, |ref|.max()) for both decoder precisions."""
import dataclasses

import pytest
import torch

from tests.util import perturb_state, state_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def close(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    atol = 2e-5 * max(1.0, float(b.abs().max()))
    err = (a - b).abs().max().item()
    assert err <= atol, f"max err {err:.3e} > {atol:.3e}"


def _decoder(g, lr_mul):
    return {"decoder.net.0.weight": torch.randn(64, 32, generator=g) / lr_mul,
            "decoder.net.0.bias": 0.3 * torch.randn(64, generator=g) / lr_mul,
            "decoder.net.2.weight": torch.randn(33, 64, generator=g) / lr_mul,
            "decoder.net.2.bias": 0.3 * torch.randn(33, generator=g) / lr_mul}


def _query(dev, planes, P, coords=None, **kw):
    from hfa_gp_amd import ops
    d = {k: v.to(dev) for k, v in P.items()}
    return ops.planes_query(planes, coords, dec_w0=d["decoder.net.0.weight"], dec_b0=d["decoder.net.0.bias"],
                            dec_w1=d["decoder.net.2.weight"], dec_b1=d["decoder.net.2.bias"], **kw)


def _oracle(P, planes_nchw, coords, box_warp, axes, lr_mul):
    from oracle import eg3d_oracle as O
    b = planes_nchw.shape[0]
    coords = coords.expand(b, -1, -1)
    return O.osg_decoder(P, O.sample_from_planes(O.plane_axes(axes), planes_nchw, coords, box_warp), lr_mul)


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("axes", ["eg3d_original", "eg3d_fixed"])
def test_planes_query_vs_oracle(dev, prec, axes):
    g = torch.Generator().manual_seed(5)
    b, h, w, box_warp, lr_mul = 2, 20, 28, 0.8, 0.5
    P = _decoder(g, lr_mul)
    pn = torch.randn(b, 3, 32, h, w, generator=g)                     # oracle layout [B,3,C,H,W]
    planes = pn.permute(0, 1, 3, 4, 2).contiguous().to(dev)
    m = 16 * 37 + 5                                                   # not a multiple of 16
    coords = (torch.rand(b, m, 3, generator=g) - 0.5) * (1.3 * box_warp)     # ~1/3 of the points outside the box
    coords[:, :7] = torch.tensor([[3.0, -3.0, 2.0], [-9.0, 9.0, 9.0], [0.6, 0.0, 0.0], [0.0, -0.41, 0.0],
                                  [0.4, 0.4, 0.4], [-0.4, -0.4, -0.4], [0.0, 0.0, 0.0]]) * box_warp
    kw = dict(box_warp=box_warp, plane_axes=axes, decoder_lr_mul=lr_mul, decoder_precision=prec)
    want_rgb, want_sig = _oracle(P, pn, coords, box_warp, axes, lr_mul)
    sig, rgb = _query(dev, planes, P, coords.to(dev), **kw)
    close(sig, want_sig)
    close(rgb, want_rgb)
    # points outside the box see zero features: sigma = decoder(0)
    z_rgb, z_sig = _oracle(P, torch.zeros(1, 3, 32, h, w), torch.zeros(1, 1, 3), box_warp, axes, lr_mul)
    close(sig[:, :2], z_sig.expand(b, 2, 1))
    # the sigma-only instance: the same bits
    sig_only, none = _query(dev, planes, P, coords.to(dev), want_rgb=False, **kw)
    assert none is None and torch.equal(sig_only, sig)
    # one point set broadcast to every identity (Bc = 1)
    sig1, rgb1 = _query(dev, planes, P, coords[:1].to(dev), **kw)
    want_rgb1, want_sig1 = _oracle(P, pn, coords[:1], box_warp, axes, lr_mul)
    close(sig1, want_sig1)
    close(rgb1, want_rgb1)
    assert torch.equal(sig1[0], sig[0])


def _lattice(n, cube):
    """EG3D create_samples on the exact integer lattice, torch fp32: samples * voxel_size + voxel_origin."""
    i = torch.arange(n, dtype=torch.float32)
    ax = i * (cube / (n - 1)) + (-cube / 2)
    x, y, z = torch.meshgrid(ax, ax, ax, indexing="ij")
    return torch.stack([x, y, z], -1).reshape(1, -1, 3)


@pytest.mark.parametrize("n", [33, 64])
def test_grid_mode_equals_explicit(dev, n):
    g = torch.Generator().manual_seed(7)
    P = _decoder(g, 1.0)
    planes = torch.randn(2, 3, 24, 24, 32, generator=g).to(dev)
    for prec in ("f16x3", "fp32"):
        kw = dict(box_warp=1.0, plane_axes=0, decoder_lr_mul=1.0, decoder_precision=prec)
        cube = 1.1
        sig_g, rgb_g = _query(dev, planes, P, grid=(n, cube, 0, n), **kw)
        sig_e, rgb_e = _query(dev, planes, P, _lattice(n, cube).to(dev), **kw)
        assert torch.equal(sig_g, sig_e.view(2, n, n, n)), (sig_g - sig_e.view(2, n, n, n)).abs().max()
        assert torch.equal(rgb_g, rgb_e.view(2, n, n, n, 32))
        # x slabs concatenate to the whole grid; a slab written into a view of the whole volume
        parts = [_query(dev, planes, P, grid=(n, cube, x0, xc), want_rgb=False, **kw)[0] for x0, xc in ((0, 10), (10, n - 10))]
        assert torch.equal(torch.cat(parts, 1), sig_g)
        vol = torch.full((2, n, n, n), float("nan"), device=dev)
        for x0, xc in ((0, 5), (5, n - 5)):
            _query(dev, planes, P, grid=(n, cube, x0, xc), want_rgb=False, out=vol[:, x0:x0 + xc], **kw)
        assert torch.equal(vol, sig_g)
        # default cube = box_warp
        assert torch.equal(_query(dev, planes, P, grid=n, want_rgb=False, **kw)[0],
                           _query(dev, planes, P, grid=(n, 1.0, 0, n), want_rgb=False, **kw)[0])


def _gen(dev, preset):
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS[preset](), conv_precision="fp32")     # planes at fp32 accuracy: the query is under test
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False)
    P = state_cpu(gen)
    return cfg, gen.to(dev), P


@pytest.mark.parametrize("preset", ["tiny64", "ffhq512_128"])
def test_sample_mixed_vs_oracle_chain(dev, preset):
    from oracle import eg3d_oracle as O
    cfg, gen, P = _gen(dev, preset)
    g = torch.Generator().manual_seed(11)
    b, m = 2, 3000
    ws = torch.randn(b, cfg.num_ws, cfg.w_dim, generator=g)
    coords = (torch.rand(b, m, 3, generator=g) - 0.5) * 1.1 * cfg.box_warp
    r = cfg.plane_resolution
    with torch.no_grad():
        out = gen.sample_mixed(coords.to(dev), torch.zeros(b, m, 3, device=dev), ws.to(dev))
        pn = O.backbone_synthesis(P, cfg, ws).view(b, 3, 32, r, r)
    want_rgb, want_sig = _oracle(P, pn, coords, cfg.box_warp, cfg.plane_axes, cfg.decoder_lr_mul)
    assert set(out) == {"rgb", "sigma"}
    close(out["sigma"], want_sig)
    close(out["rgb"], want_rgb)
    # sample(z, c) == sample_mixed(mapping(z, c))
    z = torch.randn(b, cfg.z_dim, generator=g).to(dev)
    c = torch.randn(b, cfg.c_dim, generator=g).to(dev)
    with torch.no_grad():
        s1 = gen.sample(coords.to(dev), None, z, c, truncation_psi=0.7)
        s2 = gen.sample_mixed(coords.to(dev), None, gen.mapping(z, c, truncation_psi=0.7))
    assert torch.equal(s1["sigma"], s2["sigma"]) and torch.equal(s1["rgb"], s2["rgb"])


def test_density_grid_and_get_shape(dev):
    from hfa_gp_amd.headnerf import _LatentBasis
    cfg, gen, _ = _gen(dev, "tiny64")
    g = torch.Generator().manual_seed(13)
    ws = torch.randn(2, cfg.num_ws, cfg.w_dim, generator=g).to(dev)
    n = 64
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        want = gen.sample_mixed(_lattice(n, cfg.box_warp).to(dev), None, ws)["sigma"].view(2, n, n, n)
        assert torch.equal(vol, want)
        assert torch.equal(gen.density_grid(ws, resolution=n, max_points=2 * n * n * 7), vol)     # 7-plane x slabs
        basis = _LatentBasis()
        basis.generator = gen
        assert torch.equal(basis.get_shape(ws, resolution=n), vol)


def test_density_grid_512_spot_check(dev):
    """One 512^3 grid (134 M points, 537 MB of sigma): voxels past 2^31 rgb-sized offsets checked against the explicit path."""
    cfg, gen, _ = _gen(dev, "ffhq512_128")
    g = torch.Generator().manual_seed(17)
    ws = torch.randn(1, cfg.num_ws, cfg.w_dim, generator=g).to(dev)
    n = 512
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        idx = torch.randint(0, n, (4096, 3), generator=g)
        idx[:4] = torch.tensor([[n - 1, n - 1, n - 1], [0, 0, 0], [n - 1, 0, n - 1], [300, 511, 17]])
        voxel, origin = torch.tensor(cfg.box_warp / (n - 1)), torch.tensor(-cfg.box_warp / 2)
        pts = idx.float() * voxel + origin
        want = gen.sample_mixed(pts[None].to(dev), None, ws)["sigma"][0, :, 0]
    got = vol[0, idx[:, 0], idx[:, 1], idx[:, 2]]
    assert torch.equal(got, want)


def test_query_guards(dev):
    cfg, gen, _ = _gen(dev, "tiny64")
    ws = torch.randn(2, cfg.num_ws, cfg.w_dim, device=dev)
    pts = torch.rand(2, 40, 3, device=dev) - 0.5
    with pytest.raises(RuntimeError, match="no_grad"):
        gen.sample_mixed(pts, None, ws.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no_grad"):
        gen.density_grid(ws.clone().requires_grad_(True), resolution=8)
    with pytest.raises(ValueError, match="directions"):
        gen.sample_mixed(pts, torch.zeros(2, 41, 3, device=dev), ws)
    with pytest.raises(NotImplementedError):
        gen.sample_mixed(pts, None, ws, noise_mode="random")
    with pytest.raises(NotImplementedError):
        gen.sample(pts, None, torch.randn(2, cfg.z_dim, device=dev), torch.randn(2, cfg.c_dim, device=dev), truncation_cutoff=14)
    with torch.no_grad():
        e = gen.sample_mixed(torch.zeros(0, 40, 3, device=dev), None, ws[:0])
        assert e["sigma"].shape == (0, 40, 1) and e["rgb"].shape == (0, 40, 32)
        e = gen.sample_mixed(torch.zeros(2, 0, 3, device=dev), None, ws)
        assert e["sigma"].shape == (2, 0, 1) and e["rgb"].shape == (2, 0, 32)
        assert gen.density_grid(ws[:0], resolution=8).shape == (0, 8, 8, 8)
