"""Explicit ray lists on the device (hfagp_raymarch_rays_*, ops.raymarch_rays / raymarch_rays_bwd / raymarch_rays_bwd_rays,
TriPlaneGenerator.render_rays, cam_utils.ray_grid) against the CPU oracle, whose importance_renderer takes the rays as given.
Needs an MI355X:  python -m pytest tests -m gpu

The list: B = 2, R = 101 rays per frame (odd, no square: the last 4-ray block of a workgroup is partial), origins scattered around
(0, 0, 2.7), directions towards a cloud around the centre and NOT of unit length.  In the oracle the opacity of these rays stays
far above the floor the depth gradient needs (asserted per case)."""
import dataclasses
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_camera_grad import MAX_EDGE_RAYS, check_rays
from tests.test_gpu_geometry_grad import DEC_KEYS, MIN_OPACITY, close, close_grad
from tests.util import make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

ATOL_FWD = 2e-5            # tests/test_gpu_parity.py _render_case
B, R = 2, 101
KEYS = ("g_feat", "g_depth", "g_wsum")
COMBOS = {"feat": (True, False, False), "depth": (False, True, False), "wsum": (False, False, True), "all": (True, True, True)}
PRESETS3 = ["tiny64", "small128", "ffhq512_128"]                 # 16+16, 32+32, 48+48 samples


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def ray_list():
    g = torch.Generator().manual_seed(7)
    n = torch.randn(B, R, 2, generator=g)
    o = 2.7 * F.normalize(torch.cat((0.5 * n, torch.ones(B, R, 1)), -1), dim=-1)
    d = F.normalize(0.15 * torch.randn(B, R, 3, generator=g) - o, dim=-1) * (0.95 + 0.1 * torch.rand(B, R, 1, generator=g))
    return o.contiguous(), d.contiguous()


@functools.lru_cache(maxsize=None)
def case(preset, axes="eg3d_original", white_back=False, box_warp=None, r=R):
    """ONE fp32 oracle pass on the first r rays of the list per configuration, its graph kept: every reference gradient is a
    `torch.autograd.grad` on it (planes, decoder parameters, origins, directions)."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = dataclasses.replace(PRESETS[preset](), plane_axes=axes, white_back=white_back)
    if box_warp is not None:
        cfg = dataclasses.replace(cfg, box_warp=box_warp)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0))
    P = state_cpu(gen)
    for k in DEC_KEYS:
        P[k].requires_grad_(True)
    g = torch.Generator().manual_seed(8)
    planes = torch.randn(B, 3, 32, 20, 20, generator=g, requires_grad=True)
    us = torch.rand(B, R, cfg.depth_resolution, 1, generator=g)[:, :r].contiguous()
    ui = torch.rand(B, R, cfg.depth_resolution_importance, generator=g)[:, :r].reshape(B * r, -1).contiguous()
    ups = dict(g_feat=torch.randn(B, R, 32, generator=g)[:, :r].contiguous(), g_depth=torch.randn(B, R, generator=g)[:, :r].contiguous(),
               g_wsum=torch.randn(B, R, generator=g)[:, :r].contiguous())
    o, d = (t[:, :r].clone().requires_grad_(True) for t in ray_list())
    feat, depth, wsum = O.importance_renderer(P, cfg, planes, o, d, us, ui)
    lo, hi = float(wsum.detach().min()), float(wsum.detach().max())
    print(f"{preset}/{axes}/{white_back}/{box_warp}/{r}: oracle opacity in [{lo:.3f}, {hi:.3f}]")
    assert lo >= MIN_OPACITY, f"oracle opacity down to {lo:.3e}: pick other inputs"
    return dict(cfg=cfg, gen=gen, P=P, planes=planes, us=us, ui=ui, ups=ups, od=(o, d), out=(feat, depth[..., 0], wsum[..., 0]), r=r,
                refs={})


def reference(cs, combo):
    """(d planes, (d decoder parameters), [B,R,6] = (d origin, d direction)) of sum over the combination of <output, upstream>."""
    if combo not in cs["refs"]:
        loss = sum((out * cs["ups"][k]).sum() for use, out, k in zip(COMBOS[combo], cs["out"], KEYS) if use)
        grads = torch.autograd.grad(loss, [cs["planes"]] + [cs["P"][k] for k in DEC_KEYS] + list(cs["od"]), retain_graph=True)
        cs["refs"][combo] = (grads[0], grads[1:5], torch.cat(grads[5:], -1))
    return cs["refs"][combo]


def device_inputs(cs, dev, precision=None):
    gen = cs["gen"].to(dev)
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    o, d = (t.detach().to(dev) for t in cs["od"])
    args = gen._rays_kwargs()
    if precision is not None:
        args["decoder_precision"] = precision
    return pl, o, d, cs["us"][..., 0].contiguous().to(dev), cs["ui"].to(dev), args


def device_forward(cs, dev, precision=None, state=None):
    from hfa_gp_amd import ops
    pl, o, d, us, ui, args = device_inputs(cs, dev, precision)
    return ops.raymarch_rays(pl, o, d, us, ui, state=state, **args)


def device_backward(cs, dev, combo, precision=None, use_state=False, rays=False, **kw):
    """ops.raymarch_rays (for the clamp range and the state), ops.raymarch_rays_bwd, and with `rays` ops.raymarch_rays_bwd_rays."""
    from hfa_gp_amd import ops
    pl, o, d, us, ui, args = device_inputs(cs, dev, precision)
    cfg = cs["cfg"]
    state = ops.raymarch_rays_state(B, cs["r"], cfg.depth_resolution, cfg.depth_resolution_importance, dev) if use_state else None
    _, _, _, tmm = ops.raymarch_rays(pl, o, d, us, ui, state=state, **args)
    ups = {k: (cs["ups"][k].to(dev) if use else None) for use, k in zip(COMBOS[combo], KEYS)}
    rec = []
    out = ops.raymarch_rays_bwd(ups["g_feat"], pl, o, d, us, ui, state=state, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                                depth_range=ops.depth_range(tmm) if ups["g_depth"] is not None else None, rec_out=rec, **args, **kw)
    assert len(rec) == 1 and rec[0].shape == (B, cs["r"], cfg.depth_resolution + cfg.depth_resolution_importance, 4)
    if not rays:
        return out
    return out, ops.raymarch_rays_bwd_rays(ups["g_feat"], pl, rec[0], o, d, us, ui, **args)


def check_forward(cs, dev, precision, what):
    feat, depth, wsum, tmm = device_forward(cs, dev, precision)
    depth = torch.clamp(depth, tmm[..., 0].min(), tmm[..., 1].max())
    for got, want, name in zip((feat, depth, wsum), cs["out"], ("feat", "depth", "wsum")):
        close(got, want, atol=ATOL_FWD, rtol=0.0, what=f"{what}/{name}")


# ----------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("preset", PRESETS3)
def test_forward_vs_oracle(dev, preset, precision):
    check_forward(case(preset), dev, precision, f"{preset}/{precision}")


@pytest.mark.parametrize("kw", [dict(axes="eg3d_fixed", white_back=True), dict(box_warp=2.0)], ids=["fixed-white_back", "box_warp2"])
def test_forward_other_configurations(dev, kw):
    check_forward(case("small128", **kw), dev, None, str(kw))


@pytest.mark.parametrize("r", [1, 4])
def test_forward_tiny_lists(dev, r):
    """One ray per frame (a single wave of one block has work) and one full 4-ray block."""
    check_forward(case("small128", r=r), dev, None, f"R={r}")


def test_forward_state_and_repeat(dev):
    """`state=` changes no output bit, and two calls agree bit for bit."""
    from hfa_gp_amd import ops
    cs = case("small128")
    a = device_forward(cs, dev)
    cfg = cs["cfg"]
    st = ops.raymarch_rays_state(B, R, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
    b = device_forward(cs, dev, state=st)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert torch.isfinite(st).all()


# ----------------------------------------------------------------------------- 2. the grid as a list
def _grid_setup(dev):
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = PRESETS["tiny64"]()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    return cfg, gen


def _as_list(img):
    return img.flatten(2).permute(0, 2, 1)            # [B,C,r,r] -> [B,R,C]


def test_grid_rays_render_what_synthesis_renders(dev):
    """render_rays on ray_grid(c, res) in row order against synthesis(geometry=True): 4e-5 = twice the forward bar (each side is
    within 2e-5 of the oracle on the same rays: ray_grid on the CPU is the oracle's RaySampler bit for bit)."""
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _grid_setup(dev)
    res = cfg.neural_rendering_resolution
    ws, c, us, ui = make_inputs(cfg, 2)
    o, d = (t.to(dev) for t in ray_grid(c, res))
    with torch.no_grad():
        ref = gen.synthesis(ws.to(dev), c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True)
        out = gen.render_rays(ws.to(dev), o, d, us[..., 0].to(dev), ui.to(dev))
    assert set(out) == {"feature", "rgb", "depth", "mask"} and out["feature"].shape == (2, res * res, 32)
    assert torch.equal(out["rgb"], out["feature"][..., :3])
    close(out["rgb"], _as_list(ref["image_raw"]), atol=2 * ATOL_FWD, rtol=0.0, what="rgb")
    close(out["depth"], _as_list(ref["image_depth"])[..., 0], atol=2 * ATOL_FWD, rtol=0.0, what="depth")
    close(out["mask"], _as_list(ref["image_mask"])[..., 0], atol=2 * ATOL_FWD, rtol=0.0, what="mask")


def test_two_views_in_one_list(dev):
    """Two labels' rays as ONE list of 2 R rays per frame against two synthesis calls on the same ws."""
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _grid_setup(dev)
    res = cfg.neural_rendering_resolution
    r = res * res
    ws, ca, usa, uia = make_inputs(cfg, 2)
    _, cb, usb, uib = make_inputs(cfg, 2, seed=11)
    o, d = (torch.cat(t, 1).to(dev) for t in zip(ray_grid(ca, res), ray_grid(cb, res)))
    us = torch.cat((usa, usb), 1)[..., 0].to(dev)
    ui = torch.cat((uia.reshape(2, r, -1), uib.reshape(2, r, -1)), 1).reshape(4 * r, -1).to(dev)
    with torch.no_grad():
        out = gen.render_rays(ws.to(dev), o, d, us, ui)
        for k, (c, u_s, u_i) in enumerate(((ca, usa, uia), (cb, usb, uib))):
            ref = gen.synthesis(ws.to(dev), c.to(dev), noise_mode="const", u_strat=u_s.to(dev), u_imp=u_i.to(dev), geometry=True)
            sl = slice(k * r, (k + 1) * r)
            close(out["rgb"][:, sl], _as_list(ref["image_raw"]), atol=2 * ATOL_FWD, rtol=0.0, what=f"view {k}: rgb")
            close(out["depth"][:, sl], _as_list(ref["image_depth"])[..., 0], atol=2 * ATOL_FWD, rtol=0.0, what=f"view {k}: depth")
            close(out["mask"][:, sl], _as_list(ref["image_mask"])[..., 0], atol=2 * ATOL_FWD, rtol=0.0, what=f"view {k}: mask")


# ----------------------------------------------------------------------------- 3. plane and decoder gradients
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("preset", PRESETS3)
def test_plane_grads_vs_oracle_autograd(dev, preset, combo):
    cs = case(preset)
    dpl = device_backward(cs, dev, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), reference(cs, combo)[0], f"{preset}/{combo}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("variant", ["fp32", "f16x3", "scatter", "state", "state_scatter", "eg3d_fixed"])
def test_plane_grads_variants_small128(dev, variant, combo):
    """Both decoder precisions; pass 2 as sort + gather (default) and as scatter (rows=False); the compositing adjoint from the
    forward's state; three sorted planes instead of two + the mirror."""
    cs = case("small128", "eg3d_fixed" if variant == "eg3d_fixed" else "eg3d_original")
    kw = {}
    if variant in ("fp32", "f16x3"):
        kw["precision"] = variant
    if variant.startswith("state"):
        kw["use_state"] = True
    if variant.endswith("scatter"):
        kw["rows"] = False
    dpl = device_backward(cs, dev, combo, **kw)
    close_grad(dpl.permute(0, 1, 4, 2, 3), reference(cs, combo)[0], f"{variant}/{combo}")


@pytest.mark.parametrize("rows", [None, False], ids=["sort", "scatter"])
@pytest.mark.parametrize("combo", list(COMBOS))
def test_decoder_grads_vs_oracle_autograd(dev, combo, rows):
    cs = case("small128")
    dpl, dec = device_backward(cs, dev, combo, decoder_grads=True, rows=rows)
    ref_pl, ref_dec, _ = reference(cs, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref_pl, f"dec/{combo}/planes")
    for got, ref, k in zip(dec, ref_dec, DEC_KEYS):
        close_grad(got, ref, f"dec/{combo}/{k}")


def rel_l2(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dec", [False, True])
@pytest.mark.parametrize("preset", PRESETS3)
def test_sort_gather_equals_the_scatter_kernels(dev, preset, dec):
    """The two pass-2 forms against each other, at the bars of test_raymarch_backward_sort_gather_equals_the_scatter_kernels."""
    from hfa_gp_amd import ops
    cs = case(preset)
    ref = device_backward(cs, dev, "all", rows=False, decoder_grads=dec)
    out = device_backward(cs, dev, "all", rows=True, decoder_grads=dec)
    assert ops.ROWS_STATS["path"] == "rows" and ops.ROWS_STATS["chunks"] == 1
    dref, dout = (ref[0], out[0]) if dec else (ref, out)
    scale = dref.abs().max().item()
    assert scale > 0 and torch.isfinite(dout).all()
    assert (dout - dref).abs().max().item() <= 2e-5 * scale
    assert rel_l2(dout, dref) <= 2e-5
    if dec:
        for x, y in zip(out[1], ref[1]):
            assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item()


def test_scratch_cap_cuts_the_list_at_ray_boundaries(dev, monkeypatch):
    """A cap below one frame's scratch: the call runs in ray chunks of a frame and gives what the whole call gives."""
    from hfa_gp_amd import ops
    cs = case("small128")
    whole, dec_w = device_backward(cs, dev, "all", decoder_grads=True)
    need = ops.ROWS_STATS["bytes"]
    monkeypatch.setenv("HFAGP_RAYBWD_SCRATCH_GIB", repr(need / 3 / 2 ** 30))
    cut, dec_c = device_backward(cs, dev, "all", decoder_grads=True)
    assert ops.ROWS_STATS["path"] == "rows" and ops.ROWS_STATS["chunks"] >= 4, ops.ROWS_STATS      # at least two per frame
    scale = whole.abs().max().item()
    assert (cut - whole).abs().max().item() <= 2e-5 * scale and rel_l2(cut, whole) <= 2e-5
    for x, y in zip(dec_c, dec_w):
        assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item()
    close_grad(cut.permute(0, 1, 4, 2, 3), reference(cs, "all")[0], "chunked/all")


# ----------------------------------------------------------------------------- 4. ray gradients
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("preset", PRESETS3)
def test_ray_grads_vs_oracle_autograd(dev, preset, combo):
    cs = case(preset)
    _, (d_o, d_d) = device_backward(cs, dev, combo, rays=True)
    assert d_o.shape == d_d.shape == (B, R, 3) and MAX_EDGE_RAYS == 4
    check_rays(torch.cat((d_o, d_d), -1), reference(cs, combo)[2], f"{preset}/{combo}")


@pytest.mark.parametrize("variant", ["fp32", "state", "scatter", "decoder_grads", "eg3d_fixed", "box_warp2"])
def test_ray_grads_variants_small128(dev, variant):
    kw, ckw = {}, {}
    if variant == "fp32":
        kw["precision"] = "fp32"
    if variant == "state":
        kw["use_state"] = True
    if variant == "scatter":
        kw["rows"] = False
    if variant == "decoder_grads":
        kw["decoder_grads"] = True
    if variant == "eg3d_fixed":
        ckw["axes"] = "eg3d_fixed"
    if variant == "box_warp2":
        ckw["box_warp"] = 2.0
    cs = case("small128", **ckw)
    _, (d_o, d_d) = device_backward(cs, dev, "all", rays=True, **kw)
    check_rays(torch.cat((d_o, d_d), -1), reference(cs, "all")[2], variant)


def test_ray_grads_are_deterministic_and_independent_of_pass2(dev):
    cs = case("small128")
    a = device_backward(cs, dev, "all", rays=True)[1]
    b = device_backward(cs, dev, "all", rays=True)[1]
    c = device_backward(cs, dev, "all", rays=True, rows=False)[1]
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


# ----------------------------------------------------------------------------- 5. end to end
E2E_RES = 9                # 81 rays per frame


def _e2e_cfg():
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")


def _e2e_inputs(cfg):
    ws, c, _, _ = make_inputs(cfg, 2)
    g = torch.Generator().manual_seed(6)
    r = E2E_RES * E2E_RES
    us = torch.rand(2, r, cfg.depth_resolution, 1, generator=g)
    ui = torch.rand(2 * r, cfg.depth_resolution_importance, generator=g)
    terms = (torch.randn(2, r, 32, generator=g), torch.randn(2, r, generator=g), torch.randn(2, r, generator=g))
    return ws, c, us, ui, terms


def _e2e_loss(feat, depth, mask, terms, dv=None):
    gf, kd, m = (t if dv is None else t.to(dv) for t in terms)
    return (feat * gf).mean() + 0.5 * (mask * m).mean() + 0.5 * (depth * kd).mean()


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """The oracle-backed graph: backbone_synthesis -> ray_sampler (a crop window's worth of rays would do as well) ->
    importance_renderer, every generator parameter, ws and c leaves."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = _e2e_cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    for k, v in P.items():
        if v.is_floating_point() and not k.startswith("backbone.mapping."):
            v.requires_grad_(True)
    ws, c, us, ui, terms = _e2e_inputs(cfg)
    ws_ref, c_ref = ws.clone().requires_grad_(True), c.clone().requires_grad_(True)
    o, d = O.ray_sampler(c_ref[:, :16].reshape(-1, 4, 4), c_ref[:, 16:25].reshape(-1, 3, 3), E2E_RES)
    planes = O.backbone_synthesis(P, cfg, ws_ref)
    planes5 = planes.reshape(2, 3, cfg.plane_channels, planes.shape[-2], planes.shape[-1])
    feat, depth, wsum = O.importance_renderer(P, cfg, planes5, o, d, us, ui)
    assert float(wsum.detach().min()) >= MIN_OPACITY
    _e2e_loss(feat, depth[..., 0], wsum[..., 0], terms).backward()
    return P, ws_ref.grad, c_ref.grad, (feat.detach(), depth.detach()[..., 0], wsum.detach()[..., 0])


def test_render_rays_end_to_end(dev):
    """tiny64, fp32 convs, generator tuned, ws and c leaves (c through ray_grid on the device): d ws, every generator-parameter
    gradient and d c at the bars of test_synthesis_geometry_end_to_end / test_synthesis_camera_grad_configurations; a second
    backward raises."""
    from hfa_gp_amd.cam_utils import ray_grid
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = _e2e_cfg()
    P, ws_g, c_g, fwd = e2e_reference()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    for n, p in gen.named_parameters():
        if not n.startswith("backbone.mapping."):
            p.requires_grad_(True)
    ws, c, us, ui, terms = _e2e_inputs(cfg)
    ws_d, c_d = ws.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
    o, d = ray_grid(c_d, E2E_RES)
    out = gen.render_rays(ws_d, o, d, us.to(dev), ui.to(dev))
    assert all(out[k].requires_grad for k in ("feature", "rgb", "depth", "mask"))
    close(out["feature"], fwd[0], atol=1e-4, rtol=1e-4, what="feature")
    close(out["mask"], fwd[2], atol=1e-5, rtol=0.0, what="mask")
    loss = _e2e_loss(out["feature"], out["depth"], out["mask"], terms, dev)
    loss.backward(retain_graph=True)
    close(ws_d.grad, ws_g, atol=2e-4 * ws_g.abs().max().item(), rtol=2e-3, what="d ws")
    assert c_d.grad is not None and c_d.grad.shape == (2, 25)
    close(c_d.grad, c_g, atol=2e-4 * c_g.abs().max().item(), rtol=2e-3, what="d c")
    for n, p in gen.named_parameters():
        if n.startswith("backbone.mapping."):
            continue
        refg = P[n].grad
        if p.grad is None:              # a parameter the forward does not read (the super-resolution blocks: render_rays has none)
            assert refg is None or not bool(refg.any()), n
            continue
        refg = torch.zeros_like(P[n]) if refg is None else refg
        close(p.grad, refg, atol=2e-4 * max(refg.abs().max().item(), 1e-30), rtol=2e-3, what=n)
    assert gen.decoder.net["0"].weight.grad is not None
    with pytest.raises(RuntimeError, match="backward called a second time"):
        loss.backward()


# ----------------------------------------------------------------------------- 6. contract
def test_grid_path_launches_no_list_entry_and_rays_pass_is_opt_in(dev, monkeypatch):
    from hfa_gp_amd import ops
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _grid_setup(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))

    def boom(name):
        def f(*a, **k):
            raise AssertionError(f"{name} called")
        return f

    with monkeypatch.context() as m:
        for name in ("raymarch_rays", "raymarch_rays_bwd", "raymarch_rays_bwd_rays"):
            m.setattr(ops, name, boom(name))
        ws.requires_grad_(True)
        c_g = c.clone().requires_grad_(True)
        out = gen.synthesis(ws, c_g, noise_mode="const", u_strat=us, u_imp=ui, geometry=True)
        (out["image"].square().mean() + out["image_depth"].mean() + out["image_mask"].mean()).backward()
        assert ws.grad is not None and c_g.grad is not None
    monkeypatch.setattr(ops, "raymarch_rays_bwd_rays", boom("raymarch_rays_bwd_rays"))
    o, d = ray_grid(c, 6)
    ws.grad = None
    out = gen.render_rays(ws, o, d)
    (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()
    assert ws.grad is not None and bool(ws.grad.abs().sum() > 0)
    out = gen.render_rays(ws, o.clone().requires_grad_(True), d)
    with pytest.raises(AssertionError, match="raymarch_rays_bwd_rays called"):
        out["feature"].square().mean().backward()
    # under no_grad nothing requires grad, whatever the inputs say
    with torch.no_grad():
        out = gen.render_rays(ws, o.clone().requires_grad_(True), d)
    assert not any(v.requires_grad for v in out.values())


def test_empty_lists_and_guards(dev, monkeypatch):
    from hfa_gp_amd import ops
    cfg, gen = _grid_setup(dev)
    ws = make_inputs(cfg, 2)[0].to(dev)
    for name in ("raymarch_rays", "raymarch_rays_bwd"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    for b, r in ((2, 0), (0, 5), (0, 0)):
        out = gen.render_rays(ws[:b], torch.zeros(b, r, 3, device=dev), torch.zeros(b, r, 3, device=dev))
        assert out["feature"].shape == (b, r, 32) and out["rgb"].shape == (b, r, 3)
        assert out["depth"].shape == (b, r) and out["mask"].shape == (b, r)
    o = torch.zeros(2, 0, 3, device=dev, requires_grad=True)
    out = gen.render_rays(ws.clone().requires_grad_(True), o, torch.zeros(2, 0, 3, device=dev))
    out["feature"].sum().backward()
    assert o.grad is not None and o.grad.shape == (2, 0, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gen.render_rays(ws, torch.zeros(2, 3, 3), torch.zeros(2, 3, 3))
    with pytest.raises(ValueError, match=r"\[B, R, 3\]"):
        gen.render_rays(ws, torch.zeros(1, 3, 3, device=dev), torch.zeros(1, 3, 3, device=dev))


def test_ops_refuse_mis_shaped_tensors(dev):
    from hfa_gp_amd import ops
    cs = case("small128")
    pl, o, d, us, ui, args = device_inputs(cs, dev)
    with pytest.raises(RuntimeError, match="ray_origins"):
        ops.raymarch_rays(pl, o[:1], d[:1], us, ui, **args)
    with pytest.raises(RuntimeError, match="differ"):
        ops.raymarch_rays(pl, o, d[:, :50].contiguous(), us, ui, **args)
    with pytest.raises(RuntimeError, match="wrong number of elements"):
        ops.raymarch_rays(pl, o, d, us[:, :50].contiguous(), ui, **args)
    with pytest.raises(RuntimeError, match="g_feat"):
        ops.raymarch_rays_bwd(torch.zeros(B, R - 1, 32, device=dev), pl, o, d, us, ui, **args)
    with pytest.raises(RuntimeError, match="rec must be"):
        ops.raymarch_rays_bwd_rays(None, pl, torch.zeros(B, R, 8, 4, device=dev), o, d, us, ui, **args)
