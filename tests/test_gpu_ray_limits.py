"""Per-ray depth limits for ray lists on the device (hfagp_ray_limits_box, hfagp_raymarch_rays_limits_*, ops.ray_limits_box,
ops.raymarch_rays* with t_near / t_far, TriPlaneGenerator.render_rays(t_near=, t_far=, ray_limits=)) against the CPU reference of
tests/ray_limits_ref.py — the oracle's importance_renderer restated with a [t_near, t_far] per ray.
Needs an MI355X:  python -m pytest tests -m gpu

The lists (ray_limits_ref): "mixed" — B = 2, R = 101, origins at radii 0.9 ... 4.5, direction lengths 0.5 ... 2, every ray hits the
box at box_warp 1 and 2, smallest span 0.39, reference opacity >= 0.146 (asserted per case); "miss" — the same with every ray
i % 5 == 2 turned away from the box: 40 empty rays.  Tolerances are the ray-list tests' (imported)."""
import functools

import pytest
import torch

from tests import ray_limits_ref as RL
from tests import test_gpu_render_rays as TR
from tests.test_gpu_camera_grad import MAX_EDGE_RAYS, check_rays
from tests.test_gpu_geometry_grad import DEC_KEYS, MIN_OPACITY, close, close_grad
from tests.test_gpu_render_rays import ATOL_FWD, B, COMBOS, KEYS, PRESETS3, R
from tests.util import make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def device_inputs(cs, dev, precision=None):
    """planes, origins, directions, u_strat, u_imp, (t_near, t_far) from ops.ray_limits_box or the case's constant range, args."""
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    pl = cs["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    o, d = (t.detach().to(dev) for t in cs["od"])
    args = gen._rays_kwargs()
    if precision is not None:
        args["decoder_precision"] = precision
    if "lim_dev" not in cs:
        tn, tf = (t.to(dev) for t in cs["lim"])
        box = ops.ray_limits_box(o, d, cs["cfg"].box_warp)
        # (the device's limits where the case's are the box's: test 1 holds them to 1e-6 of the reference's)
        cs["lim_dev"] = box if cs["box"] else (tn.contiguous(), tf.contiguous())
    return pl, o, d, cs["us"][..., 0].contiguous().to(dev), cs["ui"].to(dev), cs["lim_dev"], args


def case(*a, **k):
    cs = RL.case(*a, **k)
    cs.setdefault("box", k.get("limits", "box") == "box")
    return cs


def device_forward(cs, dev, precision=None, state=None):
    from hfa_gp_amd import ops
    pl, o, d, us, ui, (tn, tf), args = device_inputs(cs, dev, precision)
    return ops.raymarch_rays(pl, o, d, us, ui, state=state, t_near=tn, t_far=tf, **args)


def device_backward(cs, dev, combo, precision=None, use_state=False, rays=False, **kw):
    from hfa_gp_amd import ops
    pl, o, d, us, ui, (tn, tf), args = device_inputs(cs, dev, precision)
    cfg = cs["cfg"]
    state = ops.raymarch_rays_state(B, cs["r"], cfg.depth_resolution, cfg.depth_resolution_importance, dev) if use_state else None
    _, _, _, tmm = ops.raymarch_rays(pl, o, d, us, ui, state=state, t_near=tn, t_far=tf, **args)
    ups = {k: (cs["ups"][k].to(dev) if use else None) for use, k in zip(COMBOS[combo], KEYS)}
    rec = []
    out = ops.raymarch_rays_bwd(ups["g_feat"], pl, o, d, us, ui, state=state, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                                depth_range=ops.depth_range(tmm, empty_rays=True) if ups["g_depth"] is not None else None, rec_out=rec,
                                t_near=tn, t_far=tf, **args, **kw)
    assert len(rec) == 1 and rec[0].shape == (B, cs["r"], cfg.depth_resolution + cfg.depth_resolution_importance, 4)
    if not rays:
        return out
    return out, ops.raymarch_rays_bwd_rays(ups["g_feat"], pl, rec[0], o, d, us, ui, t_near=tn, t_far=tf, **args)


def check_forward(cs, dev, precision, what, want=None):
    from hfa_gp_amd import ops
    feat, depth, wsum, tmm = device_forward(cs, dev, precision)
    depth = ops.depth_clamp_(depth, tmm, empty_rays=True)
    for got, ref, name in zip((feat, depth, wsum), want or cs["out"], ("feat", "depth", "wsum")):
        close(got, ref, atol=ATOL_FWD, rtol=0.0, what=f"{what}/{name}")


# ----------------------------------------------------------------------------- 1. the ray-box kernel
@pytest.mark.parametrize("side", [1.0, 2.0])
@pytest.mark.parametrize("name", ["mixed", "miss"])
def test_ray_limits_box_vs_torch(dev, name, side):
    from hfa_gp_amd import cam_utils, ops
    o, d = RL.LISTS[name]()
    axis = (torch.tensor([[[0.0, 0.0, 2.7]]]).expand(B, 1, 3), torch.tensor([[[0.0, 0.0, -1.0]]]).expand(B, 1, 3))
    o, d = torch.cat((o, axis[0]), 1).contiguous(), torch.cat((d, axis[1]), 1).contiguous()      # + one axis-parallel ray per frame
    want_n, want_f = cam_utils.ray_limits_box(o, d, side)
    want_v = cam_utils.ray_limits_valid(want_n, want_f)
    assert float((want_f - want_n)[want_v].min()) >= RL.MIN_SPAN          # no ray near the edge of validity
    tn, tf = ops.ray_limits_box(o.to(dev), d.to(dev), side)
    assert tn.shape == tf.shape == (B, R + 1) and tn.dtype == tf.dtype == torch.float32
    assert torch.equal(cam_utils.ray_limits_valid(tn, tf).cpu(), want_v)
    torch.testing.assert_close(tn.cpu(), want_n, rtol=1e-6, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(tf.cpu(), want_f, rtol=1e-6, atol=1e-6, equal_nan=True)
    torch.testing.assert_close(tn[:, R].cpu(), torch.full((B,), 2.7 - side / 2), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(tf[:, R].cpu(), torch.full((B,), 2.7 + side / 2), rtol=1e-6, atol=1e-6)


def test_ray_limits_box_nan_and_inside(dev):
    """0 * inf (origin on a slab of a parallel axis) gives NaN limits; an origin inside starts at 0."""
    from hfa_gp_amd import ops
    o = torch.tensor([[[0.5, 0.0, 2.0], [0.1, -0.2, 0.3], [0.0, 0.0, 2.7]]], device=dev)
    d = torch.tensor([[[0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]], device=dev)
    tn, tf = (t.cpu()[0] for t in ops.ray_limits_box(o, d, 1.0))
    assert bool(torch.isnan(tn[0])) and bool(torch.isnan(tf[0]))
    assert float(tn[1]) == 0.0 and abs(float(tf[1]) - 0.4) <= 1e-6
    assert float(tf[2]) < float(tn[2])


# ----------------------------------------------------------------------------- 2. forward: the constant range as limits
@pytest.mark.parametrize("rays", ["r27", "mixed"])
def test_forward_constant_limits_vs_oracle(dev, rays):
    """Explicit limits filled with cfg.ray_start / ray_end against the UNTOUCHED oracle (the linspace formulas differ in the last
    bit only: tests/test_ray_limits_cpu.py)."""
    from oracle import eg3d_oracle as O
    cs = case("small128", rays=rays, limits="config")
    o, d = cs["od"]
    with torch.no_grad():
        feat, depth, wsum = O.importance_renderer(cs["P"], cs["cfg"], cs["planes"], o, d, cs["us"], cs["ui"])
    assert float(wsum.min()) >= MIN_OPACITY
    check_forward(cs, dev, None, f"const/{rays}", want=(feat, depth[..., 0], wsum[..., 0]))


# ----------------------------------------------------------------------------- 3. forward: box limits
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("preset", PRESETS3)
def test_forward_box_vs_reference(dev, preset, precision):
    check_forward(case(preset), dev, precision, f"{preset}/{precision}")


@pytest.mark.parametrize("kw", [dict(axes="eg3d_fixed", white_back=True), dict(box_warp=2.0)], ids=["fixed-white_back", "box_warp2"])
def test_forward_box_other_configurations(dev, kw):
    cs = case("small128", **kw)
    if "box_warp" in kw:
        assert bool((cs["lim"][0] == 0).any())            # origins inside the box: near = 0
    check_forward(cs, dev, None, str(kw))


@pytest.mark.parametrize("r", [1, 4])
def test_forward_box_tiny_lists(dev, r):
    check_forward(case("small128", r=r), dev, None, f"R={r}")


# ----------------------------------------------------------------------------- 4. empty rays
def test_empty_rays_forward(dev):
    from hfa_gp_amd import ops
    cs = case("small128", rays="miss")
    valid = cs["valid"]
    assert torch.equal(valid, ~RL.MISS) and int((~valid).sum()) == 40
    pl, o, d, us, ui, (tn, tf), args = device_inputs(cs, dev)
    feat, depth, wsum, tmm = ops.raymarch_rays(pl, o, d, us, ui, t_near=tn, t_far=tf, **args)
    e = (~valid).to(dev)
    assert bool((feat[e] == -1).all()) and bool((wsum[e] == 0).all()) and bool((depth[e] == INF).all())
    assert bool((tmm[e][:, 0] == INF).all()) and bool((tmm[e][:, 1] == -INF).all())
    assert torch.isfinite(feat).all() and torch.isfinite(tmm[~e]).all()
    rng = ops.depth_range(tmm, empty_rays=True)
    assert torch.equal(rng, torch.stack((tmm[~e][:, 0].min(), tmm[~e][:, 1].max())))
    clamped = ops.depth_clamp_(depth.clone(), tmm, empty_rays=True)
    assert torch.isfinite(clamped).all() and bool((clamped[e] == rng[1]).all())
    for got, ref, name in zip((feat, clamped, wsum), cs["out"], ("feat", "depth", "wsum")):
        close(got, ref, atol=ATOL_FWD, rtol=0.0, what=f"miss/{name}")
    # the 81 valid rays of each frame alone: the same bits
    keep = (~RL.MISS[0]).nonzero()[:, 0].to(dev)
    sf = ui.shape[-1]
    sub = ops.raymarch_rays(pl, o[:, keep].contiguous(), d[:, keep].contiguous(), us[:, keep].contiguous(),
                            ui.reshape(B, R, sf)[:, keep].reshape(-1, sf).contiguous(), t_near=tn[:, keep].contiguous(),
                            t_far=tf[:, keep].contiguous(), **args)
    assert torch.equal(sub[0], feat[:, keep]) and torch.equal(sub[2], wsum[:, keep]) and torch.equal(sub[1], depth[:, keep])
    # white_back: the background is +1
    wb = dict(args, white_back=True)
    feat_w = ops.raymarch_rays(pl, o, d, us, ui, t_near=tn, t_far=tf, **wb)[0]
    assert bool((feat_w[e] == 1).all())
    # an explicit NaN limit and far == near on two rays that were valid; the others keep their bits
    tn2, tf2 = tn.clone(), tf.clone()
    tn2[0, 0] = float("nan")
    tf2[1, 3] = tn2[1, 3]
    assert bool(valid[0, 0]) and bool(valid[1, 3])
    feat2, depth2, wsum2, tmm2 = ops.raymarch_rays(pl, o, d, us, ui, t_near=tn2, t_far=tf2, **args)
    for b, i in ((0, 0), (1, 3)):
        assert bool((feat2[b, i] == -1).all()) and float(wsum2[b, i]) == 0 and float(depth2[b, i]) == INF
        assert tmm2[b, i].tolist() == [INF, -INF]
    same = torch.ones(B, R, dtype=torch.bool, device=dev)
    same[0, 0] = same[1, 3] = False
    assert torch.equal(feat2[same], feat[same]) and torch.equal(wsum2[same], wsum[same])


def test_all_empty_call(dev):
    from hfa_gp_amd import ops
    cs = case("small128")
    assert bool(cs["valid"].all())
    pl, o, d, us, ui, (tn, tf), args = device_inputs(cs, dev)
    state = ops.raymarch_rays_state(B, R, us.shape[-1], ui.shape[-1], dev)
    feat, depth, wsum, tmm = ops.raymarch_rays(pl, o, d, us, ui, t_near=tf, t_far=tn, state=state, **args)      # swapped: far < near
    assert bool((feat == -1).all()) and bool((wsum == 0).all())
    assert ops.depth_range(tmm, empty_rays=True).tolist() == [0.0, 0.0]
    assert bool((ops.depth_clamp_(depth, tmm, empty_rays=True) == 0).all())
    # and its backward: zero planes gradient, zero records, zero ray gradients — with and without the (unwritten) state
    ups = {k: cs["ups"][k].to(dev) for k in KEYS}
    for st in (None, state):
        rec = []
        dpl = ops.raymarch_rays_bwd(ups["g_feat"], pl, o, d, us, ui, state=st, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                                    depth_range=ops.depth_range(tmm, empty_rays=True), rec_out=rec, t_near=tf, t_far=tn, **args)
        assert bool((dpl == 0).all()) and bool((rec[0] == 0).all())
        d_o, d_d = ops.raymarch_rays_bwd_rays(ups["g_feat"], pl, rec[0], o, d, us, ui, t_near=tf, t_far=tn, **args)
        assert bool((d_o == 0).all()) and bool((d_d == 0).all())


# ----------------------------------------------------------------------------- 5. plane and decoder gradients
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("preset", PRESETS3)
def test_plane_grads_vs_reference_autograd(dev, preset, combo):
    cs = case(preset)
    dpl = device_backward(cs, dev, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), RL.reference(cs, combo)[0], f"{preset}/{combo}")


@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("variant", ["scatter", "state", "state_scatter", "decoder"])
def test_plane_grads_variants_small128(dev, variant, combo):
    """Pass 2 as scatter (rows=False) instead of sort + gather; the compositing adjoint from the forward's state (the FROM_STATE
    instantiation reads the limits as well); the decoder-parameter gradients."""
    cs = case("small128")
    kw = dict(use_state=variant.startswith("state"), decoder_grads=variant == "decoder")
    if variant.endswith("scatter"):
        kw["rows"] = False
    out = device_backward(cs, dev, combo, **kw)
    ref_pl, ref_dec, _ = RL.reference(cs, combo)
    dpl, dec = out if variant == "decoder" else (out, None)
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref_pl, f"{variant}/{combo}")
    if dec is not None:
        for got, ref, k in zip(dec, ref_dec, DEC_KEYS):
            close_grad(got, ref, f"{variant}/{combo}/{k}")


@pytest.mark.parametrize("variant", ["sort", "scatter", "state"])
def test_grads_with_empty_rays(dev, variant):
    """The miss list: 40 empty rays contribute nothing to the planes and the decoder (their upstream gradients are random, not
    zero), and their records are zero."""
    cs = case("small128", rays="miss")
    kw = dict(use_state=variant == "state", decoder_grads=True)
    if variant == "scatter":
        kw["rows"] = False
    dpl, dec = device_backward(cs, dev, "all", **kw)
    ref_pl, ref_dec, _ = RL.reference(cs, "all")
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref_pl, f"miss/{variant}/planes")
    for got, ref, k in zip(dec, ref_dec, DEC_KEYS):
        close_grad(got, ref, f"miss/{variant}/{k}")


# ----------------------------------------------------------------------------- 6. ray gradients
@pytest.mark.parametrize("combo", list(COMBOS))
@pytest.mark.parametrize("preset", PRESETS3)
def test_ray_grads_vs_reference_autograd(dev, preset, combo):
    """d origins / d directions with the limits held fixed (the reference computes the limits under no_grad)."""
    cs = case(preset)
    _, (d_o, d_d) = device_backward(cs, dev, combo, rays=True)
    assert d_o.shape == d_d.shape == (B, R, 3) and MAX_EDGE_RAYS == 4
    check_rays(torch.cat((d_o, d_d), -1), RL.reference(cs, combo)[2], f"{preset}/{combo}")


def test_ray_grads_empty_rays_and_determinism(dev):
    cs = case("small128", rays="miss")
    a = device_backward(cs, dev, "all", rays=True)[1]
    b = device_backward(cs, dev, "all", rays=True)[1]
    c = device_backward(cs, dev, "all", rays=True, rows=False, use_state=True)[1]
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    e = (~cs["valid"]).to(dev)
    assert bool((a[0][e] == 0).all()) and bool((a[1][e] == 0).all())
    check_rays(torch.cat(a, -1), RL.reference(cs, "all")[2], "miss/all")


# ----------------------------------------------------------------------------- 7. end to end
E2E_RADIUS = 4.0


def _e2e_label(c):
    """The label's camera moved along its viewing axis to E2E_RADIUS from the centre (it keeps looking at it)."""
    c = c.clone()
    pos = c[:, [3, 7, 11]]
    c[:, [3, 7, 11]] = pos * (E2E_RADIUS / pos.norm(dim=-1, keepdim=True))
    return c


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """backbone_synthesis -> ray_sampler at radius 4 -> box limits (no_grad) -> the reference renderer; every generator parameter,
    ws and c leaves."""
    from hfa_gp_amd.cam_utils import ray_limits_box
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = TR._e2e_cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    for k, v in P.items():
        if v.is_floating_point() and not k.startswith("backbone.mapping."):
            v.requires_grad_(True)
    ws, c, us, ui, terms = TR._e2e_inputs(cfg)
    ws_ref, c_ref = ws.clone().requires_grad_(True), _e2e_label(c).requires_grad_(True)
    o, d = O.ray_sampler(c_ref[:, :16].reshape(-1, 4, 4), c_ref[:, 16:25].reshape(-1, 3, 3), TR.E2E_RES)
    tn, tf = ray_limits_box(o.detach(), d.detach(), cfg.box_warp)
    planes = O.backbone_synthesis(P, cfg, ws_ref)
    planes5 = planes.reshape(2, 3, cfg.plane_channels, planes.shape[-2], planes.shape[-1])
    feat, depth, wsum, valid = RL.importance_renderer_limits(P, cfg, planes5, o, d, us, ui, tn, tf)
    print(f"e2e: {int(valid.sum())} of {valid.numel()} rays valid, limits in [{float(tn.min()):.3f}, {float(tf.max()):.3f}], reference "
          f"opacity >= {float(wsum.detach().min()):.3f}")
    assert bool(valid.all()) and float(wsum.detach().min()) >= MIN_OPACITY
    assert float(tn.min()) > cfg.ray_end              # the config's interval would end in front of the box
    TR._e2e_loss(feat, depth[..., 0], wsum[..., 0], terms).backward()
    return P, ws_ref.grad, c_ref.grad, (feat.detach(), depth.detach()[..., 0], wsum.detach()[..., 0])


def test_render_rays_box_end_to_end(dev):
    """tiny64, fp32 convs, generator tuned, a camera at radius 4.0 through ray_grid with ray_limits="box": d ws, every
    generator-parameter gradient and d c (limits detached on both sides) at the bars of test_render_rays_end_to_end."""
    from hfa_gp_amd.cam_utils import ray_grid
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = TR._e2e_cfg()
    P, ws_g, c_g, fwd = e2e_reference()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    for n, p in gen.named_parameters():
        if not n.startswith("backbone.mapping."):
            p.requires_grad_(True)
    ws, c, us, ui, terms = TR._e2e_inputs(cfg)
    ws_d, c_d = ws.to(dev).requires_grad_(True), _e2e_label(c).to(dev).requires_grad_(True)
    o, d = ray_grid(c_d, TR.E2E_RES)
    out = gen.render_rays(ws_d, o, d, us.to(dev), ui.to(dev), ray_limits="box")
    assert set(out) == {"feature", "rgb", "depth", "mask", "valid"}
    assert out["valid"].dtype == torch.bool and bool(out["valid"].all()) and not out["valid"].requires_grad
    assert all(out[k].requires_grad for k in ("feature", "rgb", "depth", "mask"))
    close(out["feature"], fwd[0], atol=1e-4, rtol=1e-4, what="feature")
    close(out["mask"], fwd[2], atol=1e-5, rtol=0.0, what="mask")
    close(out["depth"], fwd[1], atol=1e-4, rtol=1e-4, what="depth")
    loss = TR._e2e_loss(out["feature"], out["depth"], out["mask"], terms, dev)
    loss.backward()
    close(ws_d.grad, ws_g, atol=2e-4 * ws_g.abs().max().item(), rtol=2e-3, what="d ws")
    assert c_d.grad is not None and c_d.grad.shape == (2, 25)
    close(c_d.grad, c_g, atol=2e-4 * c_g.abs().max().item(), rtol=2e-3, what="d c")
    for n, p in gen.named_parameters():
        if n.startswith("backbone.mapping."):
            continue
        refg = P[n].grad
        if p.grad is None:              # a parameter the forward does not read (the super-resolution blocks)
            assert refg is None or not bool(refg.any()), n
            continue
        refg = torch.zeros_like(P[n]) if refg is None else refg
        close(p.grad, refg, atol=2e-4 * max(refg.abs().max().item(), 1e-30), rtol=2e-3, what=n)


def test_render_rays_limits_forms_and_empty_rays(dev):
    """Python floats expand; explicit tensors; empty rays in the dict: background, mask 0, depth = the range's upper end, nothing
    NaN or inf; an all-empty call has depth 0; under grad an empty ray's gradient is exactly zero."""
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = PRESETS["tiny64"]()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws = make_inputs(cfg, B)[0].to(dev)
    o, d = (t.to(dev) for t in RL.miss_list())
    g = torch.Generator().manual_seed(3)
    us = torch.rand(B, R, cfg.depth_resolution, generator=g).to(dev)
    ui = torch.rand(B * R, cfg.depth_resolution_importance, generator=g).to(dev)
    with torch.no_grad():
        ref = gen.render_rays(ws, o, d, us, ui)
        assert set(ref) == {"feature", "rgb", "depth", "mask"}
        flt = gen.render_rays(ws, o, d, us, ui, t_near=cfg.ray_start, t_far=cfg.ray_end)
        ten = gen.render_rays(ws, o, d, us, ui, t_near=torch.full((B, R), cfg.ray_start, device=dev, dtype=torch.float64),
                              t_far=torch.full((B, R), cfg.ray_end, device=dev))
        box = gen.render_rays(ws, o, d, us, ui, ray_limits="box")
        none = gen.render_rays(ws, o, d, us, ui, t_near=1.0, t_far=1.0)
    assert bool(flt["valid"].all()) and torch.equal(flt["feature"], ten["feature"]) and torch.equal(flt["depth"], ten["depth"])
    e = RL.MISS.to(dev)
    assert torch.equal(box["valid"], ~e)
    assert all(bool(torch.isfinite(v).all()) for k, v in box.items() if k != "valid")
    assert bool((box["feature"][e] == -1).all()) and bool((box["mask"][e] == 0).all())
    assert bool((box["depth"][e] == box["depth"].max()).all()) and bool((box["depth"][~e] <= box["depth"].max()).all())
    assert not bool(none["valid"].any()) and bool((none["depth"] == 0).all()) and bool((none["feature"] == -1).all())
    o_g, d_g = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    out = gen.render_rays(ws, o_g, d_g, us, ui, ray_limits="box")
    (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()
    assert bool((o_g.grad[e] == 0).all()) and bool((d_g.grad[e] == 0).all())
    assert torch.isfinite(o_g.grad).all() and bool((o_g.grad[~e] != 0).any())


# ----------------------------------------------------------------------------- 8. guards and the untouched default
def test_guards_raise_before_a_launch(dev, monkeypatch):
    from hfa_gp_amd import ops
    cfg, gen = TR._grid_setup(dev)
    ws = make_inputs(cfg, 2)[0].to(dev)
    o, d = (t[:, :6].contiguous().to(dev) for t in RL.mixed_list())
    for name in ("raymarch_rays", "raymarch_rays_bwd", "ray_limits_box"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    monkeypatch.setattr(gen, "_query_planes", lambda *a, **k: (_ for _ in ()).throw(AssertionError("backbone launched")))
    lim = torch.ones(2, 6, device=dev)
    with pytest.raises(ValueError, match="mutually exclusive"):
        gen.render_rays(ws, o, d, t_near=lim, t_far=2 * lim, ray_limits="box")
    with pytest.raises(ValueError, match="both or neither"):
        gen.render_rays(ws, o, d, t_near=lim)
    with pytest.raises(ValueError, match="both or neither"):
        gen.render_rays(ws, o, d, t_far=2.0)
    with pytest.raises(ValueError, match=r"t_far must be \[B, R\]"):
        gen.render_rays(ws, o, d, t_near=lim, t_far=torch.ones(2, 5, device=dev))
    with pytest.raises(ValueError, match="ray_limits must be None or 'box'"):
        gen.render_rays(ws, o, d, ray_limits="auto")
    with pytest.raises(NotImplementedError, match="not differentiated"):
        gen.render_rays(ws, o, d, t_near=lim.clone().requires_grad_(True), t_far=2 * lim)


def test_ops_refuse_mis_shaped_limits(dev):
    from hfa_gp_amd import ops
    cs = case("small128")
    pl, o, d, us, ui, (tn, tf), args = device_inputs(cs, dev)
    with pytest.raises(RuntimeError, match="both or neither"):
        ops.raymarch_rays(pl, o, d, us, ui, t_near=tn, **args)
    with pytest.raises(RuntimeError, match=r"t_far must be \[B, R\]"):
        ops.raymarch_rays(pl, o, d, us, ui, t_near=tn, t_far=tf[:, :50].contiguous(), **args)
    with pytest.raises(RuntimeError, match="float32"):
        ops.raymarch_rays(pl, o, d, us, ui, t_near=tn.double(), t_far=tf, **args)
    with pytest.raises(RuntimeError, match="t_near"):
        ops.raymarch_rays_bwd(torch.zeros(B, R, 32, device=dev), pl, o, d, us, ui, t_near=tn.cpu(), t_far=tf, **args)


def test_without_the_keywords_no_limits_entry_point_runs(dev, monkeypatch):
    """synthesis and the limit-less render_rays (forward and backward, rays' gradient included) call none of the four new entry
    points, and the dict has its four keys."""
    from hfa_gp_amd import _lib, ops
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = TR._grid_setup(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    new = ("hfagp_ray_limits_box", "hfagp_raymarch_rays_limits_fwd", "hfagp_raymarch_rays_limits_bwd",
           "hfagp_raymarch_rays_limits_bwd_rays")
    calls = {n: 0 for n in new}
    real = _lib.lib()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if name not in calls:
                return fn

            def counted(*a, **k):
                calls[name] += 1
                return fn(*a, **k)
            return counted

    monkeypatch.setattr(ops.L, "lib", lambda: Counting())
    ws.requires_grad_(True)
    out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, geometry=True)
    (out["image"].square().mean() + out["image_depth"].mean() + out["image_mask"].mean()).backward()
    o, d = ray_grid(c, 6)
    out = gen.render_rays(ws, o.clone().requires_grad_(True), d)
    assert set(out) == {"feature", "rgb", "depth", "mask"}
    (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()
    with torch.no_grad():
        assert set(gen.render_rays(ws, o, d)) == {"feature", "rgb", "depth", "mask"}
    assert calls == {n: 0 for n in new}, calls
    # ... and with them, they do
    out = gen.render_rays(ws, o.clone().requires_grad_(True), d, ray_limits="box")
    (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()
    assert calls == {n: 1 for n in new}, calls
