"""Depth and opacity gradients through the fused ray marcher (hfagp_raymarch_bwd_geom, ops.raymarch_bwd g_depth / g_wsum,
synthesis(geometry=True)) against autograd through the CPU oracle, whose importance_renderer returns (feat, depth, wsum).
Needs an MI355X:  python -m pytest tests -m gpu"""
import dataclasses
import functools

import pytest
import torch

from tests.util import look_at_label, make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

DEC_KEYS = ("decoder.net.0.weight", "decoder.net.0.bias", "decoder.net.2.weight", "decoder.net.2.bias")
COMBOS = {"wsum": (False, False, True), "depth": (False, True, False), "all": (True, True, True)}     # (g_feat, g_depth, g_wsum)
# The depth term carries 1 / W: the inputs are chosen so that the ORACLE's opacity stays above this on every ray (asserted)
MIN_OPACITY = 0.05
SEED = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def close(a, b, atol, rtol, what=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    assert torch.isfinite(a).all()
    err = (a - b).abs()
    print(f"{what}: max err {err.max().item():.3e}, ref max {b.abs().max().item():.3e}, "
          f"worst err / bound {(err / (atol + rtol * b.abs())).max().item():.3f}")
    assert bool((err <= atol + rtol * b.abs()).all()), f"{what}: max err {err.max().item():.3e} (ref max {b.abs().max().item():.3e})"


def close_grad(a, b, what=""):
    """test_raymarch_bwd_vs_oracle_autograd's bar, its atol scaled by max(1, max|ref|)."""
    close(a, b, atol=2e-5 * max(1.0, float(b.abs().max())), rtol=1e-3, what=what)


@functools.lru_cache(maxsize=None)
def case(preset, axes="eg3d_original", white_back=False):
    """The set-up of test_raymarch_bwd_vs_oracle_autograd (100 rays per frame: the last 4-ray block is partial; B = 2; 20 x 20
    planes) and ONE oracle pass per configuration; every gradient combination is a `torch.autograd.grad` on its graph."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = dataclasses.replace(PRESETS[preset](), neural_rendering_resolution=10, img_resolution=40, plane_axes=axes,
                              white_back=white_back)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0))
    P = state_cpu(gen)
    for k in DEC_KEYS:
        P[k].requires_grad_(True)
    c = look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7]))
    g = torch.Generator().manual_seed(SEED)
    b, res = 2, cfg.neural_rendering_resolution
    r = res * res
    planes = torch.randn(b, 3, 32, 20, 20, generator=g, requires_grad=True)
    us = torch.rand(b, r, cfg.depth_resolution, 1, generator=g)
    ui = torch.rand(b * r, cfg.depth_resolution_importance, generator=g)
    ups = dict(g_feat=torch.randn(b, r, 32, generator=g), g_depth=torch.randn(b, r, generator=g),
               g_wsum=torch.randn(b, r, generator=g))
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    feat, depth, wsum = O.importance_renderer(P, cfg, planes, o, d, us, ui)
    assert float(wsum.detach().min()) >= MIN_OPACITY, f"oracle opacity down to {float(wsum.detach().min()):.3e}: pick other inputs"
    return dict(cfg=cfg, gen=gen, P=P, c=c, planes=planes, us=us, ui=ui, ups=ups, out=(feat, depth[..., 0], wsum[..., 0]), b=b, r=r,
                refs={})


def reference(cs, combo):
    """(d planes, (d decoder parameters)) of sum over the combination's outputs of <output, upstream>."""
    if combo not in cs["refs"]:
        loss = sum((out * cs["ups"][k]).sum() for use, out, k in zip(COMBOS[combo], cs["out"], ("g_feat", "g_depth", "g_wsum")) if use)
        grads = torch.autograd.grad(loss, [cs["planes"]] + [cs["P"][k] for k in DEC_KEYS], retain_graph=True)
        cs["refs"][combo] = (grads[0], grads[1:])
    return cs["refs"][combo]


def device_call(cs, dev, combo, precision=None, use_state=False, auto_range=True, **kw):
    """ops.raymarch_bwd on the case's inputs with the combination's upstream gradients."""
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    b = cs["b"]
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = gen._render_args(cs["c"].to(dev))
    if precision is not None:
        args["decoder_precision"] = precision
    cfg = cs["cfg"]
    state = ops.raymarch_state(b, cfg.neural_rendering_resolution, cfg.depth_resolution, cfg.depth_resolution_importance, dev) \
        if use_state else None
    _, depth_raw, _, tmm = ops.raymarch(pl, u_strat=u_s, u_imp=u_i, state=state, **args)
    use = COMBOS[combo]
    ups = {k: (cs["ups"][k].to(dev) if u else None) for u, k in zip(use, ("g_feat", "g_depth", "g_wsum"))}
    rng = kw.pop("depth_range", None)
    if rng is None and use[1] and auto_range:
        rng = ops.depth_range(tmm)
    out = ops.raymarch_bwd(ups["g_feat"], pl, u_strat=u_s, u_imp=u_i, state=state, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                           depth_range=rng, **args, **kw)
    return out, depth_raw, tmm


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("preset", ["tiny64", "small128", "ffhq512_128"])
def test_geometry_grads_vs_oracle_autograd(dev, preset, combo):
    """16+16 (one midpoint per lane), 32+32 (the e < S-1 edge on lane 63), 48+48 samples (two midpoints per lane)."""
    cs = case(preset)
    dpl, _, _ = device_call(cs, dev, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), reference(cs, combo)[0], f"{preset}/{combo}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("variant", ["fp32", "f16x3", "state_fp32", "state_f16x3", "scatter", "eg3d_fixed", "white_back"])
def test_geometry_grads_variants_small128(dev, variant, combo):
    """Both decoder precisions, the FROM_STATE adjoint (state= of a forward call), pass 2 as scatter, three scattered planes,
    white_back (whose own term in G_e is dL/dW of rgb + 1 - W and stays)."""
    cs = case("small128", "eg3d_fixed" if variant == "eg3d_fixed" else "eg3d_original", variant == "white_back")
    kw = {}
    if variant.endswith("fp32") or variant.endswith("f16x3"):
        kw["precision"] = variant.split("_")[-1]
    if variant.startswith("state"):
        kw["use_state"] = True
    if variant == "scatter":
        kw["rows"] = False
    dpl, _, _ = device_call(cs, dev, combo, **kw)
    close_grad(dpl.permute(0, 1, 4, 2, 3), reference(cs, combo)[0], f"{variant}/{combo}")


@pytest.mark.parametrize("combo", list(COMBOS))
def test_geometry_grads_decoder_parameters(dev, combo):
    cs = case("small128")
    (dpl, dec), _, _ = device_call(cs, dev, combo, decoder_grads=True)
    ref_pl, ref_dec = reference(cs, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref_pl, f"dec/{combo}/planes")
    for got, ref, k in zip(dec, ref_dec, DEC_KEYS):
        close_grad(got, ref, f"dec/{combo}/{k}")


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_image_only_path_untouched(dev, precision):
    """Zero-filled g_depth / g_wsum through the new entry add exactly zero: the pass-1 record (depth, omega, d sigma per sample)
    equals the plain call's bit for bit — the W guard forms no 0 * inf and the image-only arithmetic is what it was."""
    cs = case("small128")
    (_, rec0), _, tmm = device_call(cs, dev, "all", precision=precision, return_rec=True)      # (warm; also the non-zero run)
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(cs["b"], dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = dict(gen._render_args(cs["c"].to(dev)), decoder_precision=precision)
    gf = cs["ups"]["g_feat"].to(dev)
    _, plain = ops.raymarch_bwd(gf, pl, u_strat=u_s, u_imp=u_i, return_rec=True, **args)
    z = torch.zeros(cs["b"], cs["r"], device=dev)
    _, geom = ops.raymarch_bwd(gf, pl, u_strat=u_s, u_imp=u_i, return_rec=True, g_depth=z, g_wsum=z.clone(),
                               depth_range=ops.depth_range(tmm), **args)
    assert torch.isfinite(plain).all()
    assert torch.equal(plain, geom)
    assert not torch.equal(plain, rec0), "non-zero geometry gradients change d sigma"


def test_clamp_adjoint(dev):
    """A depth_range whose `hi` cuts through the rays' depths: rays inside get the depth gradient of the oracle's formula with
    that range (torch.clamp's autograd), rays outside contribute exactly what the g_depth=None run gives."""
    from hfa_gp_amd import ops
    from oracle import eg3d_oracle as O
    cs = case("small128")
    _, depth_raw, tmm = device_call(cs, dev, "wsum")
    rng = ops.depth_range(tmm)
    srt = depth_raw.flatten().sort().values
    n = srt.numel()
    hi = 0.5 * (srt[n // 2 - 1] + srt[n // 2])          # between the two middle depths: no ray sits on the bound
    rng_cut = torch.stack((rng[0], hi))
    # reference: the oracle's unclamped depth D / W through torch.clamp(lo, hi)
    feat, depth, wsum = cs["out"]
    d_ref = depth.detach()
    # (the oracle's own clamp range excludes no ray here, so its `depth` is the unclamped one)
    assert float(d_ref.min()) > float(rng[0]) and float(d_ref.max()) < float(rng[1])
    inside = d_ref <= hi.cpu()
    assert torch.equal(depth_raw.cpu() <= hi.cpu(), inside), "oracle and kernel put a ray on different sides of the cut"
    assert 0.4 < float(inside.float().mean()) < 0.6
    ups = cs["ups"]
    loss = (feat * ups["g_feat"]).sum() + (wsum * ups["g_wsum"]).sum() + \
        (torch.clamp(depth, float(rng[0]), float(hi)) * ups["g_depth"]).sum()
    ref, = torch.autograd.grad(loss, cs["planes"], retain_graph=True)
    dpl, _, _ = device_call(cs, dev, "all", depth_range=rng_cut)
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref, "clamp/all")
    # every ray excluded (hi below every depth of the batch): exactly the run without g_depth
    below = torch.stack((rng[0], srt[0] - 0.01))
    (_, rec_none), _, _ = device_call(cs, dev, "wsum", return_rec=True)
    gd = cs["ups"]["g_depth"].to(dev)
    gen = cs["gen"].to(dev)
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(cs["b"], dev, cs["us"].to(dev), cs["ui"].to(dev))
    _, rec_out = ops.raymarch_bwd(None, pl, u_strat=u_s, u_imp=u_i, return_rec=True, g_depth=gd, g_wsum=cs["ups"]["g_wsum"].to(dev),
                                  depth_range=below, **gen._render_args(cs["c"].to(dev)))
    assert torch.equal(rec_out, rec_none)
    # ... and with the cut range, the excluded rays' records are those of the g_depth=None run, the others are not
    _, rec_cut = ops.raymarch_bwd(None, pl, u_strat=u_s, u_imp=u_i, return_rec=True, g_depth=gd, g_wsum=cs["ups"]["g_wsum"].to(dev),
                                  depth_range=rng_cut, **gen._render_args(cs["c"].to(dev)))
    same = (rec_cut == rec_none).flatten(2).all(-1).cpu()
    assert torch.equal(same, ~inside), (int(same.sum()), int((~inside).sum()))


def _oracle_synthesis_geom(P, cfg, ws, c, us, ui):
    """O.synthesis with the opacity kept (it drops wsum): backbone_synthesis -> importance_renderer -> superresolution."""
    from oracle import eg3d_oracle as O
    b, res = ws.shape[0], cfg.neural_rendering_resolution
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:25].reshape(-1, 3, 3), res)
    planes = O.backbone_synthesis(P, cfg, ws)
    planes5 = planes.reshape(b, 3, cfg.plane_channels, planes.shape[-2], planes.shape[-1])
    feat, depth, wsum = O.importance_renderer(P, cfg, planes5, o, d, us, ui)
    feat_img = feat.permute(0, 2, 1).reshape(b, feat.shape[-1], res, res).contiguous()
    img = O.superresolution(P, cfg, feat_img[:, :3], feat_img, ws)
    return {"image": img, "image_raw": feat_img[:, :3], "image_depth": depth.permute(0, 2, 1).reshape(b, 1, res, res),
            "image_mask": wsum.permute(0, 2, 1).reshape(b, 1, res, res)}


@pytest.mark.parametrize("tuned", [False, True])
def test_synthesis_geometry_end_to_end(dev, tuned):
    """tiny64, B = 2: mse(image, target) + 0.5 mean(image_mask m) + 0.5 mean(image_depth k) -> d ws and (generator tuned) every
    generator-parameter gradient, at the bars of test_synthesis_backward_vs_oracle_autograd (fp32 convs: k = 1)."""
    import torch.nn.functional as F
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False)
    P = state_cpu(gen)
    gen = gen.to(dev)
    if tuned:
        for k, v in P.items():
            if v.is_floating_point() and not k.startswith("backbone.mapping."):
                v.requires_grad_(True)
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    ws, c, us, ui = make_inputs(cfg, 2)
    g = torch.Generator().manual_seed(6)
    r = cfg.neural_rendering_resolution
    target = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution, generator=g).clamp(-1, 1)
    m = torch.randn(2, 1, r, r, generator=g)
    kd = torch.randn(2, 1, r, r, generator=g)

    def loss_of(out, dv=None):
        t = (lambda x: x) if dv is None else (lambda x: x.to(dv))
        return F.mse_loss(out["image"], t(target)) + 0.5 * (out["image_mask"] * t(m)).mean() + 0.5 * (out["image_depth"] * t(kd)).mean()

    ws_ref = ws.clone().requires_grad_(True)
    ref = _oracle_synthesis_geom(P, cfg, ws_ref, c, us, ui)
    assert float(ref["image_mask"].detach().min()) >= MIN_OPACITY
    loss_of(ref).backward()
    ws_d = ws.to(dev).requires_grad_(True)
    out = gen.synthesis(ws_d, c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True)
    assert set(out) == {"image", "image_raw", "image_depth", "image_mask"}
    assert out["image_depth"].requires_grad and out["image_mask"].requires_grad
    close(out["image"], ref["image"], atol=1e-4, rtol=1e-4, what="image")
    close(out["image_mask"], ref["image_mask"], atol=1e-5, rtol=0.0, what="image_mask")
    loss_of(out, dev).backward()
    scale = ws_ref.grad.abs().max().item()
    close(ws_d.grad, ws_ref.grad, atol=2e-4 * scale, rtol=2e-3, what="d ws")
    if tuned:
        for n, p in gen.named_parameters():
            if n.startswith("backbone.mapping."):
                continue
            refg = P[n].grad
            if p.grad is None:          # a parameter the forward does not read (noise strength of a layer without noise)
                assert refg is None or not bool(refg.any()), n
                continue
            refg = torch.zeros_like(P[n]) if refg is None else refg
            close(p.grad, refg, atol=2e-4 * max(refg.abs().max().item(), 1e-30), rtol=2e-3, what=n)


def test_default_contract(dev):
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = PRESETS["tiny64"]()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui)
    out = gen.synthesis(ws.clone().requires_grad_(True), c, **kw)
    assert set(out) == {"image", "image_raw", "image_depth"}
    assert out["image"].requires_grad and out["image_depth"].requires_grad is False
    with torch.no_grad():
        out_ng = gen.synthesis(ws, c, geometry=True, **kw)
    assert set(out_ng) == {"image", "image_raw", "image_depth", "image_mask"}
    assert not any(v.requires_grad for v in out_ng.values())
    r = cfg.neural_rendering_resolution
    assert out_ng["image_mask"].shape == (2, 1, r, r)
    assert torch.equal(out_ng["image_depth"], out["image_depth"])
    empty = gen.synthesis(ws[:0], c[:0], geometry=True, noise_mode="const")
    assert empty["image_mask"].shape == (0, 1, r, r)
    assert set(gen.synthesis(ws[:0], c[:0], noise_mode="const")) == {"image", "image_raw", "image_depth"}


def test_entry_point_errors(dev):
    """The library's own messages; nothing is launched."""
    cs = case("tiny64")
    with pytest.raises(RuntimeError, match="g_depth needs depth_range"):
        device_call(cs, dev, "depth", auto_range=False)
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(cs["b"], dev, cs["us"].to(dev), cs["ui"].to(dev))
    with pytest.raises(RuntimeError, match="no upstream gradient"):
        ops.raymarch_bwd(None, pl, u_strat=u_s, u_imp=u_i, **gen._render_args(cs["c"].to(dev)))
    with pytest.raises(RuntimeError, match=r"g_wsum must be \[B, R\]"):
        ops.raymarch_bwd(None, pl, u_strat=u_s, u_imp=u_i, g_wsum=torch.zeros(cs["b"], cs["r"], 1, device=dev),
                         **gen._render_args(cs["c"].to(dev)))
    torch.cuda.synchronize()
