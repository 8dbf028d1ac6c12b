"""Density gradient and unit normal at query points on the GPU (csrc/planes_query_normals.hip, csrc/planes_query_normals_bwd.hip,
ops.planes_query_normals[_bwd], sample_mixed(normals=True), synthesis(query_normals=True), extract_mesh(normals=True),
tools/extract_shapes.py --normals) against the float64 reference of tests/query_normals_ref.py.
Needs an MI355X:  python -m pytest tests -m gpu

Bar: the project's gradient bar, normal_grad_ref.bar_ratio (|err| <= 2e-5 max(1, max|ref|) + 1e-3 |ref| per element).  The points of
tests/query_ref.base_case() keep 1e-3 texel clear of every texel edge, so EVERY point is compared."""
import dataclasses
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import normal_grad_ref as NG
from tests import query_normals_ref as R
from tests import query_ref as Q
from tests.test_gpu_geometry_grad import close, close_grad
from tests.util import ROOT, make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "f16x3")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _planes_dev(pn, dev):
    return pn.permute(0, 1, 3, 4, 2).contiguous().to(dev)          # oracle [B,3,C,H,W] -> [B,3,H,W,C]


def _dec_kw(dev, P, prec, axes, box_warp=Q.BOX_WARP, lr_mul=Q.LR_MUL):
    d = {k: P[k].to(dev) for k in Q.DEC_KEYS}
    return dict(dec_w0=d[Q.DEC_KEYS[0]], dec_b0=d[Q.DEC_KEYS[1]], dec_w1=d[Q.DEC_KEYS[2]], dec_b1=d[Q.DEC_KEYS[3]], box_warp=box_warp,
                plane_axes=axes, decoder_lr_mul=lr_mul, decoder_precision=prec)


# ----------------------------------------------------------------------------- 1. the forward kernel
@pytest.mark.parametrize("broadcast", (False, True), ids=("Bc=B", "Bc=1"))
@pytest.mark.parametrize("axes", Q.AXES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_forward_vs_reference(dev, prec, axes, broadcast):
    from hfa_gp_amd import ops
    cs = Q.base_case()
    ref = R.base_forward(axes, broadcast)
    planes = _planes_dev(cs["pn"], dev)
    coords = (cs["coords"][:1] if broadcast else cs["coords"]).to(dev)
    kw = _dec_kw(dev, cs["P"], prec, axes)
    out = ops.planes_query_normals(planes, coords, **kw)
    assert set(out) == {"sigma", "rgb", "grad", "normal"}
    sigma, rgb = ops.planes_query(planes, coords, **kw)
    assert torch.equal(out["sigma"], sigma) and torch.equal(out["rgb"], rgb)
    what = f"{prec}/{axes}/{'Bc=1' if broadcast else 'Bc=B'}"
    assert R.worst(out["grad"], ref["g"], f"{what} grad") <= 1.0
    assert R.worst(out["normal"], ref["n"], f"{what} normal") <= 1.0
    # the first two SPECIAL points lie outside every plane: exact zeros
    assert bool((out["grad"][:, :2] == 0).all()) and bool((out["normal"][:, :2] == 0).all())
    # one writer per point, no atomics: the same bits again; and every subset of the outputs gives the same bits
    again = ops.planes_query_normals(planes, coords, **kw)
    assert all(torch.equal(out[k], again[k]) for k in out)
    for want in (("normal",), ("grad",), ("sigma", "grad"), ("rgb", "normal")):
        part = ops.planes_query_normals(planes, coords, want=want, **kw)
        assert set(part) == set(want) and all(torch.equal(part[k], out[k]) for k in want), want


@pytest.mark.parametrize("m,hw,axes", [(1, (20, 28), "eg3d_original"), (32, (20, 28), "eg3d_original"), (53, (36, 20), "eg3d_fixed")],
                         ids=("M=1", "M=32", "36x20-fixed"))
def test_forward_extra_shapes(dev, m, hw, axes):
    from hfa_gp_amd import ops
    cs = Q.base_case()
    g = torch.Generator().manual_seed(50 + m)
    pn = torch.randn(Q.B, 3, 32, hw[0], hw[1], generator=g)
    coords = Q.make_points(g, Q.B, m, h=hw[0], w=hw[1], special=False, spread=1.1)
    ref = R.forward(cs["P"], pn, coords, axes)
    for prec in PRECISIONS:
        kw = _dec_kw(dev, cs["P"], prec, axes)
        out = ops.planes_query_normals(_planes_dev(pn, dev), coords.to(dev), **kw)
        sigma, rgb = ops.planes_query(_planes_dev(pn, dev), coords.to(dev), **kw)
        assert torch.equal(out["sigma"], sigma) and torch.equal(out["rgb"], rgb)
        assert R.worst(out["grad"], ref["g"], f"M={m}/{hw}/{prec} grad") <= 1.0
        assert R.worst(out["normal"], ref["n"], f"M={m}/{hw}/{prec} normal") <= 1.0


def test_ops_checks(dev):
    from hfa_gp_amd import ops
    cs = Q.base_case()
    planes, coords = _planes_dev(cs["pn"], dev), cs["coords"].to(dev)
    kw = _dec_kw(dev, cs["P"], "fp32", "eg3d_original")
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.planes_query_normals(planes, cs["coords"], **kw)
    with pytest.raises(RuntimeError, match="coords must be"):
        ops.planes_query_normals(planes, coords[:, :, :2].contiguous(), **kw)
    with pytest.raises(ValueError, match="want"):
        ops.planes_query_normals(planes, coords, want=("sigma", "depth"), **kw)
    with pytest.raises(ValueError, match="want"):
        ops.planes_query_normals(planes, coords, want=(), **kw)
    empty = ops.planes_query_normals(planes, coords[:, :0].contiguous(), **kw)
    assert empty["grad"].shape == (Q.B, 0, 3) and empty["rgb"].shape == (Q.B, 0, 32)
    gg = torch.zeros(Q.B, Q.M, 3, device=dev)
    with pytest.raises(ValueError, match="g_grad"):
        ops.planes_query_normals_bwd(planes, coords, None, None, **kw)
    with pytest.raises(RuntimeError, match=r"\[B, M, 3\]"):
        ops.planes_query_normals_bwd(planes, coords, gg[:, :5].contiguous(), None, **kw)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.planes_query_normals_bwd(planes, coords, gg.cpu(), None, **kw)
    with pytest.raises(ValueError, match="nothing to compute"):
        ops.planes_query_normals_bwd(planes, coords, gg, None, d_planes=False, **kw)
    d_pl, dec = ops.planes_query_normals_bwd(planes, coords[:, :0].contiguous(), gg[:, :0].contiguous(), None, decoder_grads=True, **kw)
    assert bool((d_pl == 0).all()) and all(bool((t == 0).all()) for t in dec)


# ----------------------------------------------------------------------------- 2. the backward kernel
def _bwd(dev, cs, which, prec, axes, **kw):
    from hfa_gp_amd import ops
    use_g, use_n = R.UPSTREAM[which]
    gg, gn = R.upstream()
    return ops.planes_query_normals_bwd(_planes_dev(cs["pn"], dev), cs["coords"].to(dev), gg.to(dev) if use_g else None,
                                        gn.to(dev) if use_n else None, **_dec_kw(dev, cs["P"], prec, axes), **kw)


@pytest.mark.parametrize("which", list(R.UPSTREAM))
@pytest.mark.parametrize("axes", Q.AXES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_backward_vs_reference(dev, prec, axes, which):
    cs = Q.base_case()
    ref = R.base_backward(axes, which)
    what = f"{prec}/{axes}/{which}"
    d_pl, dec = _bwd(dev, cs, which, prec, axes, decoder_grads=True)
    assert R.rho(d_pl.permute(0, 1, 4, 2, 3), dec, ref, what) <= 1.0
    assert bool((dec[2][1:] == 0).all()) and bool((dec[3] == 0).all())         # the colour rows and the second bias: nothing
    only, none = _bwd(dev, cs, which, prec, axes)
    assert none is None
    assert R.rho(only.permute(0, 1, 4, 2, 3), None, ref, what + " planes only") <= 1.0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_backward_accumulates_into_prefilled_buffers(dev, prec):
    cs = Q.base_case()
    axes = "eg3d_fixed"
    ref = R.base_backward(axes, "both")
    g = torch.Generator().manual_seed(21)
    pre_pl = torch.randn(Q.B, 3, Q.H, Q.W, 32, generator=g).to(dev)
    pre_dec = tuple(torch.randn(cs["P"][k].shape, generator=g).to(dev) for k in Q.DEC_KEYS)
    d_pl, dec = pre_pl.clone(), tuple(t.clone() for t in pre_dec)
    out_pl, out_dec = _bwd(dev, cs, "both", prec, axes, d_planes=d_pl, decoder_grads=True, dec_out=dec)
    assert out_pl is d_pl and all(a is b for a, b in zip(out_dec, dec))
    want = dict(planes=ref["planes"] + pre_pl.cpu().double().permute(0, 1, 4, 2, 3),
                dec=tuple(r + p.cpu().double() for r, p in zip(ref["dec"], pre_dec)))
    assert R.rho(d_pl.permute(0, 1, 4, 2, 3), dec, want, f"accumulate/{prec}") <= 1.0
    # the colour rows of d_dec_w1 and all of d_dec_b1 keep their prefilled bits
    assert torch.equal(dec[2][1:], pre_dec[2][1:]) and torch.equal(dec[3], pre_dec[3])
    assert not torch.equal(dec[2][0], pre_dec[2][0]) and not torch.equal(dec[0], pre_dec[0])
    # d_planes=False: the decoder gradients alone, within the bar of the same reference
    none_pl, dec2 = _bwd(dev, cs, "both", prec, axes, d_planes=False, decoder_grads=True)
    assert none_pl is None
    for k, a, b in zip(Q.DEC_KEYS, dec2, ref["dec"]):
        assert R.worst(a, b, f"decoder only/{prec}/{k}") <= 1.0


@pytest.mark.parametrize("prec", PRECISIONS)
def test_zero_upstream_leaves_every_buffer_alone(dev, prec):
    from hfa_gp_amd import ops
    cs = Q.base_case()
    g = torch.Generator().manual_seed(22)
    pre_pl = torch.randn(Q.B, 3, Q.H, Q.W, 32, generator=g).to(dev)
    pre_dec = tuple(torch.randn(cs["P"][k].shape, generator=g).to(dev) for k in Q.DEC_KEYS)
    d_pl, dec = pre_pl.clone(), tuple(t.clone() for t in pre_dec)
    zero = torch.zeros(Q.B, Q.M, 3, device=dev)
    ops.planes_query_normals_bwd(_planes_dev(cs["pn"], dev), cs["coords"].to(dev), zero, zero.clone(), d_planes=d_pl, decoder_grads=True,
                                 dec_out=dec, **_dec_kw(dev, cs["P"], prec, "eg3d_original"))
    assert torch.equal(d_pl.view(torch.int32), pre_pl.view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(dec, pre_dec))
    # a single live point in a tile of dead ones: only its twelve lines per identity are touched
    one = zero.clone()
    one[:, 6] = 1.0                              # SPECIAL[6]: the origin, inside every plane
    d_pl2, _ = ops.planes_query_normals_bwd(_planes_dev(cs["pn"], dev), cs["coords"].to(dev), None, one,
                                            **_dec_kw(dev, cs["P"], prec, "eg3d_original"))
    assert 0 < int((d_pl2.abs().sum(-1) != 0).sum()) <= Q.B * 12


# ----------------------------------------------------------------------------- 3 - 5. through the generator (tiny64)
M_E2E = 37


def _cfg():
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")


def _gen(dev, tuned=False):
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = perturb_state(TriPlaneGenerator(_cfg(), seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    return gen


TUNED_KEYS = Q.DEC_KEYS + ("backbone.synthesis.b32.conv1.weight",)


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """float64 autograd through the oracle backbone and the reference's twice-differentiable gather: loss <n, Gn> + <g, Gg> at
    points on the planes of ws; gradients w.r.t. ws, the decoder tensors and one backbone conv weight."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    for k in TUNED_KEYS:
        P[k].requires_grad_(True)
    ws, c, us, ui = make_inputs(cfg, 2)
    g = torch.Generator().manual_seed(31)
    r = cfg.plane_resolution
    coords = Q.make_points(g, 2, M_E2E, cfg.box_warp, r, r, special=False, spread=1.1)
    Gn = torch.randn(2, M_E2E, 3, generator=g) / 8
    Gg = torch.randn(2, M_E2E, 3, generator=g) / 64
    G = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution, generator=g) / cfg.img_resolution
    ws_ref = ws.double().requires_grad_(True)
    pn = O.backbone_synthesis(P, cfg, ws_ref).reshape(2, 3, 32, r, r)
    x = coords.double().requires_grad_(True)
    _, sigma = O.osg_decoder(P, NG.gather_from_planes(cfg.plane_axes, pn, x, cfg.box_warp), cfg.decoder_lr_mul)
    gr, = torch.autograd.grad(sigma.sum(), x, create_graph=True)
    n = -gr * torch.rsqrt((gr * gr).sum(-1, keepdim=True) + 1e-12)
    norm = gr.detach().norm(dim=-1)
    print(f"e2e reference: smallest non-zero |g| {float(norm[norm > 0].min()):.3e}, {int((norm == 0).sum())} points outside")
    loss = (n * Gn.double()).sum() + (gr * Gg.double()).sum()
    grads = torch.autograd.grad(loss, [ws_ref] + [P[k] for k in TUNED_KEYS], allow_unused=True)
    grads = [torch.zeros_like(t) if gv is None else gv for gv, t in zip(grads, [ws_ref] + [P[k] for k in TUNED_KEYS])]
    return dict(inputs=(ws, c, us, ui), coords=coords, Gn=Gn, Gg=Gg, G=G, d_ws=grads[0], d_params=dict(zip(TUNED_KEYS, grads[1:])),
                g=gr.detach(), n=n.detach())


def _normal_term(out, rf, dev, keys=("sigma_grad", "normal")):
    return (out[keys[1]] * rf["Gn"].to(dev)).sum() + (out[keys[0]] * rf["Gg"].to(dev)).sum()


def test_sample_mixed_normals_forward_bits(dev):
    from hfa_gp_amd import ops
    gen = _gen(dev)
    rf = e2e_reference()
    ws, co = rf["inputs"][0].to(dev), rf["coords"].to(dev)
    with torch.no_grad():
        out = gen.sample_mixed(co, None, ws, normals=True)
        plain = gen.sample_mixed(co, None, ws)
        planes, pam = gen._query_planes(ws)
        want = ops.planes_query_normals(planes, co, planes_absmax=pam, **gen._query_kwargs())
    assert set(out) == {"rgb", "sigma", "sigma_grad", "normal"} and set(plain) == {"rgb", "sigma"}
    assert torch.equal(out["sigma"], want["sigma"]) and torch.equal(out["rgb"], want["rgb"])
    assert torch.equal(out["sigma_grad"], want["grad"]) and torch.equal(out["normal"], want["normal"])
    assert torch.equal(out["sigma"], plain["sigma"]) and torch.equal(out["rgb"], plain["rgb"])
    assert R.worst(out["sigma_grad"], rf["g"], "tiny64 sigma_grad") <= 1.0
    assert R.worst(out["normal"], rf["n"], "tiny64 normal") <= 1.0
    # under grad the same bits, as differentiable outputs
    ws_g = ws.clone().requires_grad_(True)
    diff = gen.sample_mixed(co, None, ws_g, normals=True, differentiable=True)
    assert all(diff[k].requires_grad for k in diff)
    assert torch.equal(diff["sigma_grad"], want["grad"]) and torch.equal(diff["normal"], want["normal"])
    empty = gen.sample_mixed(co[:, :0], None, ws, normals=True)
    assert empty["sigma_grad"].shape == (2, 0, 3) and empty["normal"].shape == (2, 0, 3)


def test_sample_mixed_normals_backward_frozen(dev):
    gen = _gen(dev)
    rf = e2e_reference()
    ws_d = rf["inputs"][0].to(dev).requires_grad_(True)
    out = gen.sample_mixed(rf["coords"].to(dev), None, ws_d, normals=True, differentiable=True)
    _normal_term(out, rf, dev).backward()
    scale = rf["d_ws"].abs().max().item()
    close(ws_d.grad, rf["d_ws"].float(), atol=2e-4 * scale, rtol=2e-3, what="sample_mixed(normals) d ws")
    # sigma / rgb next to the normal term: the sum of the two stand-alone gradients (both kernels into the same buffers)
    ws_a = rf["inputs"][0].to(dev).requires_grad_(True)
    o = gen.sample_mixed(rf["coords"].to(dev), None, ws_a, normals=True, differentiable=True)
    (_normal_term(o, rf, dev) + o["sigma"].mean() + o["rgb"].mean()).backward()
    ws_b = rf["inputs"][0].to(dev).requires_grad_(True)
    o = gen.sample_mixed(rf["coords"].to(dev), None, ws_b, differentiable=True)
    (o["sigma"].mean() + o["rgb"].mean()).backward()
    want = ws_d.grad + ws_b.grad
    close(ws_a.grad, want, atol=1e-4 * float(want.abs().max()), rtol=1e-3, what="normal term + sigma / rgb")


def test_sample_mixed_normals_backward_tuned(dev):
    from tests.test_gpu_round4 import rel_l2
    gen = _gen(dev, tuned=True)
    rf = e2e_reference()
    ws_d = rf["inputs"][0].to(dev).requires_grad_(True)
    out = gen.sample_mixed(rf["coords"].to(dev), None, ws_d, normals=True, differentiable=True)
    _normal_term(out, rf, dev).backward()
    scale = rf["d_ws"].abs().max().item()
    close(ws_d.grad, rf["d_ws"].float(), atol=2e-4 * scale, rtol=2e-3, what="sample_mixed(normals) d ws (tuned)")
    prm = dict(gen.named_parameters())
    for k in Q.DEC_KEYS:
        assert R.worst(prm[k].grad, rf["d_params"][k], k) <= 1.0
    k = TUNED_KEYS[-1]
    err = rel_l2(prm[k].grad, rf["d_params"][k].float())
    print(f"{k}: rel-L2 {err:.3e}")
    assert err <= 2e-3


def test_synthesis_query_normals_forward(dev):
    gen = _gen(dev)
    rf = e2e_reference()
    ws, c, us, ui = (t.to(dev) for t in rf["inputs"])
    co = rf["coords"].to(dev)
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui)
    with torch.no_grad():
        want = gen.sample_mixed(co, None, ws, normals=True)
        plain = gen.synthesis(ws, c, query=co, **kw)
        out = gen.synthesis(ws, c, query=co, query_normals=True, **kw)
        geo = gen.synthesis(ws, c, query=co, query_normals=True, geometry=True, normals=True, **kw)
    plain_grad = gen.synthesis(ws.clone().requires_grad_(True), c, query=co, **kw)
    under_grad = gen.synthesis(ws.clone().requires_grad_(True), c, query=co, query_normals=True, **kw)
    assert set(out) == {"image", "image_raw", "image_depth", "query_sigma", "query_rgb", "query_sigma_grad", "query_normal"}
    assert set(geo) == set(out) | {"image_mask", "image_normal"}
    for o, base in ((out, plain), (geo, plain), (under_grad, plain_grad)):
        assert torch.equal(o["query_sigma_grad"], want["sigma_grad"]) and torch.equal(o["query_normal"], want["normal"])
        assert torch.equal(o["query_sigma"], want["sigma"]) and torch.equal(o["query_rgb"], want["rgb"])
        for k in ("image", "image_raw", "image_depth"):
            assert torch.equal(o[k], base[k]), k
    assert under_grad["query_normal"].requires_grad and under_grad["query_sigma_grad"].requires_grad
    assert not out["query_normal"].requires_grad
    empty = gen.synthesis(ws, c, query=co[:, :0], query_normals=True, **kw)
    assert empty["query_normal"].shape == (2, 0, 3) and empty["query_sigma_grad"].shape == (2, 0, 3)


def test_synthesis_query_normals_backward_is_image_plus_normal_term(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen = _gen(dev)
    rf = e2e_reference()
    ws, c, us, ui = (t.to(dev) for t in rf["inputs"])
    co = rf["coords"].to(dev)
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui)
    target = torch.randn(rf["G"].shape, generator=torch.Generator().manual_seed(7)).to(dev) * 0.5
    keys = ("query_sigma_grad", "query_normal")
    calls = []
    real = ops.planes_query_normals_bwd
    monkeypatch.setattr(ops, "planes_query_normals_bwd", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # image only (with the keyword: the new keys are ignored by the loss, nothing extra is launched)
    ws_i = ws.clone().requires_grad_(True)
    out = gen.synthesis(ws_i, c, query=co, query_normals=True, geometry=True, **kw)
    torch.nn.functional.mse_loss(out["image"], target).backward()
    assert calls == []
    # the stand-alone normal term
    ws_n = ws.clone().requires_grad_(True)
    _normal_term(gen.sample_mixed(co, None, ws_n, normals=True, differentiable=True), rf, dev).backward()
    assert calls == [1]
    # both in one pass
    ws_j = ws.clone().requires_grad_(True)
    out = gen.synthesis(ws_j, c, query=co, query_normals=True, **kw)
    (torch.nn.functional.mse_loss(out["image"], target) + _normal_term(out, rf, dev, keys)).backward()
    assert calls == [1, 1]
    want = ws_i.grad + ws_n.grad
    scale = float(want.abs().max())
    print(f"image + normal term: max |d ws| {scale:.3e}, image part {float(ws_i.grad.abs().max()):.3e}, "
          f"normal part {float(ws_n.grad.abs().max()):.3e}, max diff {float((ws_j.grad - want).abs().max()):.3e}")
    close(ws_j.grad, want, atol=2e-4 * scale, rtol=2e-3, what="image + normal term d ws")
    # the tuned generator composes with geometry=True: every decoder gradient is finite and the sigma row moved
    gen_t = _gen(dev, tuned=True)
    out = gen_t.synthesis(ws.clone().requires_grad_(True), c, query=co, query_normals=True, geometry=True, **kw)
    (out["image_mask"].mean() + _normal_term(out, rf, dev, keys)).backward()
    assert calls == [1, 1, 1]
    prm = dict(gen_t.named_parameters())
    assert all(bool(torch.isfinite(prm[k].grad).all()) for k in Q.DEC_KEYS) and float(prm[Q.DEC_KEYS[0]].grad.abs().max()) > 0


def test_refusals_come_before_any_launch(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen = _gen(dev)
    rf = e2e_reference()
    ws, c, us, ui = (t.to(dev) for t in rf["inputs"])
    co = rf["coords"].to(dev)
    launched = []
    for name in ("planes_query", "planes_query_normals", "planes_query_bwd", "planes_query_normals_bwd", "raymarch", "modconv",
                 "styles_demod_batch"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui)
    with pytest.raises(NotImplementedError, match="points"):
        gen.synthesis(ws.clone().requires_grad_(True), c, query=co.clone().requires_grad_(True), query_normals=True, **kw)
    with pytest.raises(NotImplementedError, match="points"):
        gen.sample_mixed(co.clone().requires_grad_(True), None, ws.clone().requires_grad_(True), normals=True, differentiable=True)
    for extra in (dict(normal_grad=True), dict(normal_camera_grad=True)):
        with pytest.raises(NotImplementedError, match="normal_grad"):
            gen.synthesis(ws.clone().requires_grad_(True), c, query=co, query_normals=True, **extra, **kw)
    with pytest.raises(ValueError, match="query"):
        gen.synthesis(ws, c, query_normals=True, **kw)
    with pytest.raises(ValueError, match="device"):
        gen.synthesis(ws, c, query=co.cpu(), query_normals=True, **kw)
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="CUDA"):
            gen.sample_mixed(co.cpu(), None, ws, normals=True)
    # the trainer-step-scope rule of sample_mixed(differentiable=True), unchanged
    gen._grad_sink = lambda p, g: None
    try:
        with pytest.raises(RuntimeError, match=r"synthesis\(.*query="):
            gen.sample_mixed(co, None, ws.clone().requires_grad_(True), normals=True, differentiable=True)
    finally:
        gen._grad_sink = None
    with pytest.raises(RuntimeError, match="no_grad"):
        gen.sample_mixed(co, None, ws.clone().requires_grad_(True), normals=True)
    assert launched == []


# ----------------------------------------------------------------------------- 6. meshes
def _level(vol):
    n = vol.shape[-1]
    p = int(30 * n / 256)
    return float(vol[..., p:n - p, p:n - p, p:n - p].median())


def _agreeing_share(verts, faces, normals):
    """share of the vertices whose normal has a positive dot product with the area-weighted mean of their adjacent face normals"""
    v, f, n = verts.double().cpu(), faces.long().cpu(), normals.double().cpu()
    fn = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])        # length = 2 x area
    acc = torch.zeros_like(v)
    for k in range(3):
        acc.index_add_(0, f[:, k], fn)
    return float(((acc * n).sum(-1) > 0).double().mean())


def test_mesh_vertex_normals(dev):
    from hfa_gp_amd import ops
    from hfa_gp_amd.headnerf import _LatentBasis
    gen = _gen(dev)
    cfg = gen.cfg
    n = 48
    ws = torch.randn(2, cfg.num_ws, cfg.w_dim, generator=torch.Generator().manual_seed(21)).to(dev)
    with torch.no_grad():
        level = _level(gen.density_grid(ws, resolution=n))
        base = gen.extract_mesh(ws, resolution=n, level=level, colors=True)
        meshes = gen.extract_mesh(ws, resolution=n, level=level, colors=True, normals=True)
        planes, pam = gen._query_planes(ws)
        P = {k: v.double() for k, v in state_cpu(gen).items() if k in Q.DEC_KEYS}
        for b, (m, m0) in enumerate(zip(meshes, base)):
            assert set(m) == {"vertices", "faces", "colors", "normals"} and set(m0) == {"vertices", "faces", "colors"}
            for k in m0:
                assert torch.equal(m[k], m0[k]), k
            verts = m["vertices"]
            assert verts.shape[0] > 100 and m["normals"].shape == verts.shape and m["normals"].dtype == torch.float32
            q = ops.planes_query_normals(planes[b:b + 1], verts[None], want=("grad", "normal"), planes_absmax=pam, **gen._query_kwargs())
            assert torch.equal(m["normals"], q["normal"][0])
            live = q["grad"][0].abs().sum(-1) != 0
            assert float((m["normals"].norm(dim=-1)[live] - 1).abs().max()) <= 1e-5
            ref = R.forward(P, planes[b:b + 1].permute(0, 1, 4, 2, 3).cpu(), verts[None].cpu(), cfg.plane_axes, cfg.box_warp,
                            cfg.decoder_lr_mul)
            got, want = _agreeing_share(verts, m["faces"], m["normals"]), _agreeing_share(verts, m["faces"], ref["n"][0])
            print(f"mesh {b}: {verts.shape[0]} vertices, share of normals on the faces' side {got:.4f} (float64 reference {want:.4f})")
            assert got >= want - 0.01
        basis = _LatentBasis()
        basis.generator = gen
        again = basis.get_mesh(ws, resolution=n, level=level, normals=True)
        assert torch.equal(again[1]["normals"], meshes[1]["normals"]) and "colors" not in again[1]


def test_extract_shapes_cli_normals(dev, tmp_path):
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import load_G_official
    from hfa_gp_amd.render import shape_mesh_eg3d
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import extract_shapes as X
    finally:
        sys.path.pop(0)
    n = 40
    cfg = tiny64()
    gen = load_G_official(cfg=cfg, seed=0, weights=None, device=dev)
    with torch.no_grad():
        z = torch.from_numpy(np.random.RandomState(3).randn(1, cfg.z_dim)).float().to(dev)
        ws = gen.mapping(z, X.frontal_label(dev))
        grid = gen.density_grid(ws, resolution=n)[0]
        level = _level(grid)
        verts, faces = shape_mesh_eg3d(grid, level=level)
        want = X.world_to_eg3d_dir(gen.sample_mixed(X.eg3d_to_world(verts, n, cfg.box_warp)[None], None, ws, normals=True)["normal"][0])
    nv = verts.shape[0]
    assert nv > 0
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "extract_shapes.py"), "--preset", "tiny64", "--seeds", "3",
                          "--resolution", str(n), "--format", "ply", "--level", repr(level), "--normals", "--outdir", str(tmp_path)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    raw = (tmp_path / "seed0003.ply").read_bytes()
    head, body = raw.split(b"end_header\n", 1)
    header = head.decode().splitlines()
    assert f"element vertex {nv}" in header
    props = [ln.split()[-1] for ln in header if ln.startswith("property float")]
    assert props == ["x", "y", "z", "nx", "ny", "nz"] and "property uchar red" not in header
    vert = np.frombuffer(body[:nv * 24], dtype="<f4").reshape(nv, 6)
    assert np.array_equal(vert[:, :3], verts.cpu().numpy())
    assert np.array_equal(vert[:, 3:], want.cpu().numpy())
    # in the lattice frame too the normals point to the side the faces are wound toward: a wrong flip or permutation of the axes
    # would leave the complement of this share, below one half
    share = _agreeing_share(verts, faces, torch.from_numpy(vert[:, 3:].copy()))
    print(f"CLI mesh: share of normals on the faces' side {share:.4f}")
    assert share > 0.5
