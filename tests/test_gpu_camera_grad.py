"""The camera gradient of the renderer on the device (hfagp_raymarch_bwd_camera, ops.raymarch_bwd_camera, synthesis with
`c.requires_grad`) against autograd through the CPU oracle.  Needs an MI355X:  python -m pytest tests -m gpu

The positional derivative of a bilinear gather is discontinuous at texel edges: a sample whose pixel coordinate rounds across an
edge in one implementation and not in the other changes one ray by up to a few percent.  The per-ray comparisons therefore allow
a fixed number of rays (4 of 200; the fp32 oracle alone has 0 or 1 against the float64 oracle on these inputs) beyond the bar,
and print the count; everything downstream of the per-ray gradients is continuous and compared without exclusions."""
import ctypes
import dataclasses
import functools
import math

import pytest
import torch

from tests import camera_ref as R
from tests.test_gpu_geometry_grad import MIN_OPACITY, SEED, _oracle_synthesis_geom, close, close_grad
from tests.util import FLIP_COLUMNS, look_at_label, make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

MAX_EDGE_RAYS = 4            # of 200 per case
UPSTREAMS = {"feat": ("g_feat",), "all": ("g_feat", "g_depth", "g_wsum")}
ZERO_COLUMNS = [k for k in range(25) if k not in R.NONZERO_COLUMNS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def case(preset, axes="eg3d_original", hw=(20, 20), box_warp=None, white_back=False):
    """test_gpu_geometry_grad.case with the plane size and box_warp open: 100 rays per frame (the last 4-ray block of a workgroup
    is partial), B = 2, random planes (seed 4), ONE fp32 oracle pass whose graph keeps the rays' origins and directions."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = dataclasses.replace(PRESETS[preset](), neural_rendering_resolution=10, img_resolution=40, plane_axes=axes,
                              white_back=white_back)
    if box_warp is not None:
        cfg = dataclasses.replace(cfg, box_warp=box_warp)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0))
    P = state_cpu(gen)
    c = look_at_label(torch.tensor([1.3, 1.8]), torch.tensor([1.5, 1.7])).requires_grad_(True)
    g = torch.Generator().manual_seed(SEED)
    b, res = 2, cfg.neural_rendering_resolution
    r = res * res
    planes = torch.randn(b, 3, 32, hw[0], hw[1], generator=g)
    us = torch.rand(b, r, cfg.depth_resolution, 1, generator=g)
    ui = torch.rand(b * r, cfg.depth_resolution_importance, generator=g)
    ups = dict(g_feat=torch.randn(b, r, 32, generator=g), g_depth=torch.randn(b, r, generator=g),
               g_wsum=torch.randn(b, r, generator=g))
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), res)
    o.retain_grad(), d.retain_grad()
    feat, depth, wsum = O.importance_renderer(P, cfg, planes, o, d, us, ui)
    return dict(cfg=cfg, gen=gen, c=c, planes=planes, us=us, ui=ui, ups=ups, od=(o, d), out=(feat, depth[..., 0], wsum[..., 0]),
                b=b, r=r, refs={})


def reference(cs, up):
    """[B,R,6] = (dL/d origin, dL/d direction) per ray of sum over the upstream set of <output, upstream>, fp32 oracle autograd."""
    if up not in cs["refs"]:
        loss = sum((out * cs["ups"][k]).sum() for out, k in zip(cs["out"], ("g_feat", "g_depth", "g_wsum")) if k in UPSTREAMS[up])
        cs["refs"][up] = torch.cat(torch.autograd.grad(loss, cs["od"], retain_graph=True), -1)
    return cs["refs"][up]


def device_call(cs, dev, up, precision=None, use_state=False, **kw):
    """ops.raymarch_bwd (pass 1 leaves `rec`) then ops.raymarch_bwd_camera -> (d_cam2world, d_intrinsics, ray_grad)."""
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    b, cfg = cs["b"], cs["cfg"]
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = gen._render_args(cs["c"].detach().to(dev))
    if precision is not None:
        args["decoder_precision"] = precision
    state = ops.raymarch_state(b, cfg.neural_rendering_resolution, cfg.depth_resolution, cfg.depth_resolution_importance, dev) \
        if use_state else None
    _, _, _, tmm = ops.raymarch(pl, u_strat=u_s, u_imp=u_i, state=state, **args)
    ups = {k: (cs["ups"][k].to(dev) if k in UPSTREAMS[up] else None) for k in ("g_feat", "g_depth", "g_wsum")}
    rec = []
    ops.raymarch_bwd(ups["g_feat"], pl, u_strat=u_s, u_imp=u_i, state=state, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                     depth_range=ops.depth_range(tmm) if ups["g_depth"] is not None else None, rec_out=rec, **args, **kw)
    assert len(rec) == 1 and rec[0].shape == (b, cs["r"], cfg.depth_resolution + cfg.depth_resolution_importance, 4)
    return ops.raymarch_bwd_camera(ups["g_feat"], pl, rec[0], u_strat=u_s, u_imp=u_i, **args)


def check_rays(ray_grad, ref, what):
    """close_grad's bar per ray; at most MAX_EDGE_RAYS rays beyond it, every ray finite."""
    got = ray_grad.detach().float().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    atol, rtol = 2e-5 * max(1.0, float(ref.abs().max())), 1e-3
    err = (got - ref).abs()
    bad = (err > atol + rtol * ref.abs()).flatten(2).any(-1)
    good = ~bad[..., None].expand_as(err)
    worst = float((err / (atol + rtol * ref.abs()))[good].max()) if bool(good.any()) else 0.0
    print(f"{what}: {int(bad.sum())} of {bad.numel()} rays beyond the bar (allowed {MAX_EDGE_RAYS}); ref max {float(ref.abs().max()):.3e}, "
          f"max err {float(err.max()):.3e}, worst err / bound of the other rays {worst:.3f}")
    assert int(bad.sum()) <= MAX_EDGE_RAYS, f"{what}: {int(bad.sum())} rays beyond the bar"


CASES = [("tiny64", "eg3d_original", (20, 20), None), ("small128", "eg3d_original", (20, 20), None),
         ("ffhq512_128", "eg3d_original", (20, 20), None), ("small128", "eg3d_fixed", (36, 20), None),
         ("small128", "eg3d_fixed", (24, 24), None), ("small128", "eg3d_original", (20, 36), 0.6),
         ("small128", "eg3d_original", (40, 72), 0.45)]


@pytest.mark.parametrize("up", list(UPSTREAMS))
@pytest.mark.parametrize("preset,axes,hw,box_warp", CASES, ids=[f"{p}-{a}-{h[0]}x{h[1]}-{b}" for p, a, h, b in CASES])
def test_ray_grad_vs_oracle_autograd(dev, preset, axes, hw, box_warp, up):
    """16+16, 32+32, 48+48 samples; both axis conventions; planes that are not square either way; points outside the box."""
    cs = case(preset, axes, hw, box_warp)
    _, _, rg = device_call(cs, dev, up)
    check_rays(rg, reference(cs, up), f"{preset}/{axes}/{hw}/{box_warp}/{up}")


@pytest.mark.parametrize("up", list(UPSTREAMS))
@pytest.mark.parametrize("variant", ["fp32", "f16x3", "state", "scatter", "decoder_grads", "white_back"])
def test_ray_grad_variants_small128(dev, variant, up):
    cs = case("small128", white_back=variant == "white_back")
    kw = {}
    if variant in ("fp32", "f16x3"):
        kw["precision"] = variant
    if variant == "state":
        kw["use_state"] = True
    if variant == "scatter":
        kw["rows"] = False
    if variant == "decoder_grads":
        kw["decoder_grads"] = True
    _, _, rg = device_call(cs, dev, up, **kw)
    check_rays(rg, reference(cs, up), f"{variant}/{up}")


def test_ray_grad_independent_of_pass2_form(dev):
    cs = case("small128")
    a = device_call(cs, dev, "all")
    b = device_call(cs, dev, "all", rows=False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("preset,axes,hw,box_warp", [CASES[0], CASES[2], CASES[3], CASES[6]],
                         ids=["tiny64", "ffhq512_128", "fixed-36x20", "40x72-0.45"])
def test_ray_setup_adjoint_and_reduction(dev, preset, axes, hw, box_warp):
    """The device's own ray_grad through the float64 oracle's ray_sampler autograd = d_cam2world / d_intrinsics (no discontinuity
    here: no exclusions); the slots without a gradient are exactly 0; two calls return the same bits."""
    from oracle import eg3d_oracle as O
    cs = case(preset, axes, hw, box_warp)
    d_m, d_k, rg = device_call(cs, dev, "all")
    d_m2, d_k2, rg2 = device_call(cs, dev, "all")
    assert torch.equal(d_m, d_m2) and torch.equal(d_k, d_k2) and torch.equal(rg, rg2)
    c = cs["c"].detach().double().requires_grad_(True)
    o, d = O.ray_sampler(c[:, :16].reshape(-1, 4, 4), c[:, 16:].reshape(-1, 3, 3), cs["cfg"].neural_rendering_resolution)
    rg64 = rg.cpu().double()
    ref, = torch.autograd.grad((o, d), c, (rg64[..., :3], rg64[..., 3:]))
    got = torch.cat((d_m, d_k), 1).cpu()
    close_grad(got[:, :16], ref[:, :16].float(), f"{preset}/d_cam2world")
    close_grad(got[:, 16:], ref[:, 16:].float(), f"{preset}/d_intrinsics")
    assert bool((got[:, ZERO_COLUMNS] == 0).all()) and bool((ref[:, ZERO_COLUMNS] == 0).all())
    # ... and the closed form of tests/camera_ref.py says the same
    close_grad(got, R.ray_setup_adjoint(c.detach(), cs["cfg"].neural_rendering_resolution, rg64).float(), f"{preset}/camera_ref")


def test_ray_setup_adjoint_with_skew(dev):
    """A label with skew, cx != cy and fx != fy (the look-at labels have none): ray_grad handed to the entry directly."""
    from hfa_gp_amd import ops
    from oracle import eg3d_oracle as O
    cs = case("tiny64")
    gen = cs["gen"].to(dev)
    b, cfg = cs["b"], cs["cfg"]
    c = cs["c"].detach().clone()
    c[:, 16], c[:, 17], c[:, 18], c[:, 21] = torch.tensor([4.1, 4.4]), torch.tensor([0.07, -0.11]), torch.tensor([0.47, 0.52]), \
        torch.tensor([0.55, 0.44])
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = gen._render_args(c.to(dev))
    gf = cs["ups"]["g_feat"].to(dev)
    rec = []
    ops.raymarch_bwd(gf, pl, u_strat=u_s, u_imp=u_i, rec_out=rec, **args)
    d_m, d_k, rg = ops.raymarch_bwd_camera(gf, pl, rec[0], u_strat=u_s, u_imp=u_i, **args)
    c64 = c.double().requires_grad_(True)
    o, d = O.ray_sampler(c64[:, :16].reshape(-1, 4, 4), c64[:, 16:].reshape(-1, 3, 3), cfg.neural_rendering_resolution)
    rg64 = rg.cpu().double()
    ref, = torch.autograd.grad((o, d), c64, (rg64[..., :3], rg64[..., 3:]))
    got = torch.cat((d_m, d_k), 1).cpu()
    assert bool((ref[:, R.NONZERO_COLUMNS] != 0).all())
    close_grad(got[:, :16], ref[:, :16].float(), "skew/d_cam2world")
    close_grad(got[:, 16:], ref[:, 16:].float(), "skew/d_intrinsics")
    assert bool((got[:, ZERO_COLUMNS] == 0).all())


# ----------------------------------------------------------------------------- end to end
def _e2e_cfg():
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")


def _e2e_terms(cfg):
    g = torch.Generator().manual_seed(6)
    r = cfg.neural_rendering_resolution
    target = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution, generator=g).clamp(-1, 1)
    return target, torch.randn(2, 1, r, r, generator=g), torch.randn(2, 1, r, r, generator=g)


def _e2e_loss(out, terms, dv=None):
    """test_synthesis_geometry_end_to_end's loss: mse + mask + depth terms."""
    import torch.nn.functional as F
    target, m, kd = (t if dv is None else t.to(dv) for t in terms)
    return F.mse_loss(out["image"], target) + 0.5 * (out["image_mask"] * m).mean() + 0.5 * (out["image_depth"] * kd).mean()


@functools.lru_cache(maxsize=None)
def e2e_reference(seed):
    """(inputs, d ws, d c) of the oracle for make_inputs(cfg, 2, seed); one CPU pass per seed, shared by the tests below."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = _e2e_cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    ws, c, us, ui = make_inputs(cfg, 2, seed)
    ws_ref, c_ref = ws.clone().requires_grad_(True), c.clone().requires_grad_(True)
    ref = _oracle_synthesis_geom(P, cfg, ws_ref, c_ref, us, ui)
    assert float(ref["image_mask"].detach().min()) >= MIN_OPACITY
    _e2e_loss(ref, _e2e_terms(cfg)).backward()
    return (ws, c, us, ui), ws_ref.grad, c_ref.grad


def _e2e_device(dev, seed, ws_grad=True, tuned=False):
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = _e2e_cfg()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    (ws, c, us, ui), _, _ = e2e_reference(seed)
    ws_d = ws.to(dev).requires_grad_(ws_grad)
    c_d = c.to(dev).requires_grad_(True)
    out = gen.synthesis(ws_d, c_d, noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True)
    assert all(out[k].requires_grad for k in ("image", "image_depth", "image_mask"))
    _e2e_loss(out, _e2e_terms(cfg), dev).backward()
    assert c_d.grad is not None and c_d.grad.shape == (2, 25) and c_d.grad.dtype == c_d.dtype
    return ws_d.grad, c_d.grad, gen


def _within(got, ref, atol, rtol):
    got = got.detach().float().cpu()
    return bool(torch.isfinite(got).all()) and bool(((got - ref).abs() <= atol + rtol * ref.abs()).all())


def test_synthesis_camera_grad_end_to_end(dev):
    """tiny64, B = 2, fp32 convs, ws and c both leaves that require grad; seeds 10, 11, 12.  d c at the bar of d ws
    (2e-4 scale, 2e-3 relative); one seed may exceed it (a single-sample edge flip) but must stay within 1e-2 scale.  d ws meets
    its bar in the same call."""
    beyond = []
    for seed in (10, 11, 12):
        _, ws_ref, c_ref = e2e_reference(seed)
        d_ws, d_c, _ = _e2e_device(dev, seed)
        close(d_ws, ws_ref, atol=2e-4 * ws_ref.abs().max().item(), rtol=2e-3, what=f"seed {seed}: d ws")
        scale = c_ref.abs().max().item()
        err = (d_c.cpu() - c_ref).abs()
        print(f"seed {seed}: d c max err {err.max().item():.3e}, scale {scale:.3e}, err / scale {err.max().item() / scale:.3e}")
        assert bool((d_c.cpu()[:, ZERO_COLUMNS] == 0).all())
        if not _within(d_c, c_ref, 2e-4 * scale, 2e-3):
            beyond.append(seed)
            assert _within(d_c, c_ref, 1e-2 * scale, 0.0), f"seed {seed}: d c off by {err.max().item() / scale:.3e} of its scale"
    print(f"seeds beyond the 2e-4 bar: {beyond}")
    assert len(beyond) <= 1, beyond


@pytest.mark.parametrize("mode", ["c_only", "tuned"])
def test_synthesis_camera_grad_configurations(dev, mode):
    """Only c requires grad (generator and ws frozen); generator tuned + c."""
    seed = 10
    _, ws_ref, c_ref = e2e_reference(seed)
    d_ws, d_c, gen = _e2e_device(dev, seed, ws_grad=mode == "tuned", tuned=mode == "tuned")
    scale = c_ref.abs().max().item()
    close(d_c, c_ref, atol=2e-4 * scale, rtol=2e-3, what=f"{mode}: d c")
    if mode == "c_only":
        assert d_ws is None and all(p.grad is None for p in gen.parameters())
    else:
        close(d_ws, ws_ref, atol=2e-4 * ws_ref.abs().max().item(), rtol=2e-3, what="tuned: d ws")
        assert gen.decoder.net["0"].weight.grad is not None


# ----------------------------------------------------------------------------- contract
def test_no_camera_pass_without_camera_grad(dev, monkeypatch):
    from hfa_gp_amd import ops
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = PRESETS["tiny64"]()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))

    def boom(*a, **k):
        raise AssertionError("raymarch_bwd_camera called although c needs no gradient")

    monkeypatch.setattr(ops, "raymarch_bwd_camera", boom)
    ws.requires_grad_(True)
    gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)["image"].square().mean().backward()
    assert ws.grad is not None and c.grad is None
    # under no_grad a label that requires grad is just a label
    with torch.no_grad():
        out = gen.synthesis(ws.detach(), c.clone().requires_grad_(True), noise_mode="const", u_strat=us, u_imp=ui, geometry=True)
    assert not any(v.requires_grad for v in out.values())
    # ... and with it the pass runs
    with pytest.raises(AssertionError, match="raymarch_bwd_camera called"):
        gen.synthesis(ws.detach(), c.clone().requires_grad_(True), noise_mode="const", u_strat=us,
                      u_imp=ui)["image"].square().mean().backward()


def test_get_image_with_non_leaf_label(dev):
    """label = base + delta (non-leaf): the in-place flip is an autograd-tracked mul_, so delta.grad is the generator-level c.grad
    with the flipped columns negated; a LEAF that requires grad fails in PyTorch's own in-place check, as in the reference."""
    from hfa_gp_amd import headnerf

    class A:
        out_pose = False; person_2 = False; params_len = 76; generator_preset = "tiny14"; generator_seed = 0

    torch.manual_seed(0)
    m = headnerf.HeadNeRF_3DMM(A(), 64, dev, 512, 8).to(dev)
    cfg = m.generator.cfg
    r = cfg.neural_rendering_resolution ** 2
    g = torch.Generator().manual_seed(2)
    us = torch.rand(2, r, cfg.depth_resolution, generator=g).to(dev)
    ui = torch.rand(2 * r, cfg.depth_resolution_importance, generator=g).to(dev)
    latent = m.get_latent(torch.randn(2, 8, generator=g).to(dev)).detach()
    base = look_at_label(torch.tensor([1.5, 1.7]), torch.tensor([1.6, 1.5]), flipped=False).to(dev)
    delta = (1e-3 * torch.randn(2, 25, generator=g)).to(dev).requires_grad_(True)
    m.get_image(latent, base + delta, u_strat=us, u_imp=ui).square().mean().backward()
    c = (base + delta.detach()).clone()
    c[:, FLIP_COLUMNS] *= -1
    c.requires_grad_(True)
    m.generator.synthesis(latent, c, noise_mode="const", u_strat=us, u_imp=ui)["image"].square().mean().backward()
    want = c.grad.clone()
    want[:, FLIP_COLUMNS] *= -1
    assert bool(want.abs().max() > 0)
    close(delta.grad, want, atol=1e-6 * want.abs().max().item(), rtol=1e-5, what="d delta")
    with pytest.raises(RuntimeError, match="in-place"):
        m.get_image(latent, base.clone().requires_grad_(True), u_strat=us, u_imp=ui)


def test_entry_errors_and_empty_batch(dev):
    from hfa_gp_amd import _lib, ops
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cs = case("tiny64")
    gen = cs["gen"].to(dev)
    b, r = cs["b"], cs["r"]
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    args = gen._render_args(cs["c"].detach().to(dev))
    gf = cs["ups"]["g_feat"].to(dev)
    # the library's own message: 24 + 24 samples are not a supported count
    us, ui = torch.rand(b, r, 24, device=dev), torch.rand(b * r, 24, device=dev)
    with pytest.raises(RuntimeError, match="raymarch_bwd_camera: unsupported sample counts"):
        ops.raymarch_bwd_camera(gf, pl, torch.zeros(b, r, 48, 4, device=dev), u_strat=us, u_imp=ui, **args)
    a = _lib.RaymarchBwdArgs()
    a.rec = 8
    with pytest.raises(RuntimeError, match="d_cam2world and d_intrinsics go together"):
        _lib.check(_lib.lib().hfagp_raymarch_bwd_camera(ctypes.byref(a), 8, 8, None, None), "raymarch_bwd_camera")
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    with pytest.raises(RuntimeError, match=r"rec must be \[B, R, Sc \+ Sf, 4\]"):
        ops.raymarch_bwd_camera(gf, pl, torch.zeros(b, r, 7, 4, device=dev), u_strat=u_s, u_imp=u_i, **args)
    # the empty batch: nothing launched, shapes kept
    e_args = dict(args, cam2world=args["cam2world"][:0], intrinsics=args["intrinsics"][:0])
    d_m, d_k, rg = ops.raymarch_bwd_camera(None, pl[:0], torch.zeros(0, r, 32, 4, device=dev), u_strat=u_s[:0], u_imp=u_i[:0], **e_args)
    assert d_m.shape == (0, 16) and d_k.shape == (0, 9) and rg.shape == (0, r, 6)
    cfg = PRESETS["tiny64"]()
    g2 = TriPlaneGenerator(cfg, seed=0).requires_grad_(False).to(dev)
    ws, c, _, _ = (t.to(dev) for t in make_inputs(cfg, 2))
    c0 = c[:0].clone().requires_grad_(True)
    out = g2.synthesis(ws[:0], c0, noise_mode="const")
    out["image"].sum().backward()
    assert c0.grad is not None and c0.grad.shape == (0, 25)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- what it is for
@pytest.mark.parametrize("start", [(0.08, -0.05), (-0.06, 0.04)])
def test_recovers_a_camera(dev, start):
    """tiny64, B = 1, fixed uniforms: the target is the render at (h, v) = (1.45, 1.62); Adam (lr 0.01, 40 steps) on (h, v)
    through look_at_label (differentiable torch) brings the loss to <= 5 % of its start and both angles to within 0.02 (the CPU
    oracle on these inputs: loss ratios 0.002 and 0.006, largest final angle error 0.0054)."""
    import torch.nn.functional as F
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = PRESETS["tiny64"]()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws, _, us, ui = (t.to(dev) for t in make_inputs(cfg, 1))
    h0, v0 = 1.45, 1.62

    def render(h, v):
        c = look_at_label(h, v).to(dev)
        return gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)["image"]

    with torch.no_grad():
        target = render(torch.tensor([h0]), torch.tensor([v0]))
    h = torch.tensor([h0 + start[0]], requires_grad=True)
    v = torch.tensor([v0 + start[1]], requires_grad=True)
    opt = torch.optim.Adam([h, v], lr=0.01)
    first = None
    for _ in range(40):
        opt.zero_grad()
        loss = F.mse_loss(render(h, v), target)
        loss.backward()
        first = loss.item() if first is None else first
        opt.step()
    with torch.no_grad():
        last = F.mse_loss(render(h, v), target).item()
    dh, dv = abs(h.item() - h0), abs(v.item() - v0)
    print(f"start {start}: loss {first:.4e} -> {last:.4e} (ratio {last / first:.4f}), |dh| {dh:.4f}, |dv| {dv:.4f}")
    assert math.isfinite(last) and last <= 0.05 * first, (first, last)
    assert dh <= 0.02 and dv <= 0.02, (dh, dv)
