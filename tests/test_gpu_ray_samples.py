"""Per-sample compositing weights of ray lists on the device (hfagp_raymarch_rays_samples_fwd / _samples_bwd,
ops.raymarch_rays(samples=True) / raymarch_rays_bwd(g_weights=), TriPlaneGenerator.render_rays(samples=True)) against
tests/ray_samples_ref.py.  Needs an MI355X:  python -m pytest tests -m gpu

Depths are compared with the fp32 reference per ray (a fine sample may fall into the neighbouring CDF bin: at most 2 % of the valid
rays may be left out, a condition); weights and every gradient are compared with float64 `weights_at` evaluated AT THE DEVICE'S OWN
depths, every ray, none left out."""
import dataclasses
import functools

import pytest
import torch

from tests import ray_samples_ref as SR
from tests import test_gpu_ray_limits as TL
from tests import test_gpu_render_rays as TR
from tests.test_gpu_camera_grad import MAX_EDGE_RAYS, check_rays
from tests.test_gpu_geometry_grad import DEC_KEYS, MIN_OPACITY, close, close_grad
from tests.test_gpu_render_rays import ATOL_FWD, B, COMBOS, KEYS, PRESETS3, R
from tests.util import make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

G_SEED = 21


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def device_inputs(cs, dev, precision=None):
    """planes, o, d, u_strat, u_imp, dict of limits (empty without), args — of a test_gpu_render_rays or a ray_limits_ref case."""
    if "lim" in cs:
        cs.setdefault("box", True)
        pl, o, d, us, ui, (tn, tf), args = TL.device_inputs(cs, dev, precision)
        return pl, o, d, us, ui, dict(t_near=tn, t_far=tf), args
    pl, o, d, us, ui, args = TR.device_inputs(cs, dev, precision)
    return pl, o, d, us, ui, {}, args


def device_samples(cs, dev, precision=None, state=None):
    """ops.raymarch_rays(samples=True) -> feat, depth (unclamped), wsum, tminmax, sample_weights, sample_depths."""
    from hfa_gp_amd import ops
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev, precision)
    return ops.raymarch_rays(pl, o, d, us, ui, state=state, samples=True, **lim, **args)


def g_weights(cs):
    s = cs["cfg"].depth_resolution + cs["cfg"].depth_resolution_importance
    return torch.randn(B, cs["r"], s - 1, generator=torch.Generator().manual_seed(G_SEED))


def check_depths(ts, preset, limits, r, what):
    """Non-decreasing; per valid ray within TOL_T of the fp32 reference, at most 2 % of the valid rays left out; empty rays zero."""
    ref = SR.reference(preset, limits, r)
    ts = ts.cpu()
    assert ts.shape == ref["t"].shape and torch.isfinite(ts).all()
    assert bool((ts[..., 1:] >= ts[..., :-1]).all()), f"{what}: sample_depths not sorted"
    tol = SR.tol_t(preset, limits, r)
    dev_t = (ts - ref["t"]).abs().amax(-1)
    valid = ref["valid"]
    out = valid & (dev_t > tol)
    worst = float(dev_t[valid & ~out].max()) if bool((valid & ~out).any()) else 0.0
    print(f"{what}: {int(out.sum())} of {int(valid.sum())} valid rays beyond TOL_T = {tol:.3e} (allowed "
          f"{SR.MAX_UNMATCHED_DEV * int(valid.sum()):.1f}); largest deviation of the others {worst:.3e}")
    assert int(out.sum()) <= SR.MAX_UNMATCHED_DEV * int(valid.sum()), f"{what}: {int(out.sum())} rays left out"
    assert not bool(ts[~valid].any())


def check_weights(cs, out, preset, limits, r, what):
    """sample_weights against float64 weights_at at the device's depths, every ray; their sum against wsum and their mean depth
    against the unclamped depth at the forward bar."""
    feat, depth, wsum, tmm, sw, ts = out
    s = ts.shape[-1]
    assert sw.shape == (B, r, s - 1) and ts.shape == (B, r, s) and sw.dtype == ts.dtype == torch.float32
    want, _ = SR.weights64(cs, ts)
    close(sw, want.float(), atol=SR.tol_w(preset, limits, r), rtol=0.0, what=f"{what}/weights")
    valid = SR.reference(preset, limits, r)["valid"]
    assert not bool(sw.cpu()[~valid].any())
    w64, t64 = sw.double().cpu(), ts.double().cpu()
    close(wsum, w64.sum(-1).float(), atol=ATOL_FWD, rtol=0.0, what=f"{what}/sum w vs mask")
    tot = w64.sum(-1)
    d64 = (w64 * 0.5 * (t64[..., 1:] + t64[..., :-1])).sum(-1) / tot
    close(depth.cpu()[valid], d64[valid].float(), atol=ATOL_FWD, rtol=0.0, what=f"{what}/sum w t / sum w vs depth")


# ----------------------------------------------------------------------------- 1, 2. depths and weights
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
@pytest.mark.parametrize("preset", PRESETS3)
def test_depths_and_weights(dev, preset, precision):
    """S = 32, 64, 96: one half-wave, the lane-63 boundary, the carry between the two halves of the scan."""
    cs = SR.inputs(preset)
    out = device_samples(cs, dev, precision)
    check_depths(out[5], preset, None, R, f"{preset}/{precision}")
    check_weights(cs, out, preset, None, R, f"{preset}/{precision}")


# ----------------------------------------------------------------------------- 3. shapes and edges
@pytest.mark.parametrize("r", [1, 3])
def test_short_lists(dev, r):
    """Fewer rays than a workgroup has waves (R = 101, a partial last block, is test 1's)."""
    cs = SR.inputs("small128", r=r)
    out = device_samples(cs, dev)
    check_depths(out[5], "small128", None, r, f"R={r}")
    check_weights(cs, out, "small128", None, r, f"R={r}")


def test_white_back_leaves_the_weights_alone(dev):
    a = device_samples(SR.inputs("small128"), dev)
    b = device_samples(SR.inputs("small128", white_back=True), dev)
    assert torch.equal(a[4], b[4]) and torch.equal(a[5], b[5])
    assert not torch.equal(a[0], b[0])


def test_box_limits_and_empty_rays(dev):
    """ray_limits_ref.miss_list(): the 40 empty rays give exact zeros in both outputs, the valid ones match as in 1 and 2."""
    cs = SR.inputs("small128", "box")
    out = device_samples(cs, dev)
    empty = ~SR.reference("small128", "box")["valid"]
    assert int(empty.sum()) == 40
    assert not bool(out[4].cpu()[empty].any()) and not bool(out[5].cpu()[empty].any())
    check_depths(out[5], "small128", "box", R, "box")
    check_weights(cs, out, "small128", "box", R, "box")


@pytest.mark.parametrize("limits", [None, "box"])
@pytest.mark.parametrize("use_state", [False, True])
def test_other_outputs_keep_their_bits(dev, limits, use_state):
    from hfa_gp_amd import ops
    cs = SR.inputs("small128", limits)
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev)
    cfg = cs["cfg"]
    mk = lambda: ops.raymarch_rays_state(B, R, cfg.depth_resolution, cfg.depth_resolution_importance, dev) if use_state else None
    sa, sb = mk(), mk()
    a = ops.raymarch_rays(pl, o, d, us, ui, state=sa, **lim, **args)
    b = ops.raymarch_rays(pl, o, d, us, ui, state=sb, samples=True, **lim, **args)
    assert len(a) == 4 and len(b) == 6
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if use_state and limits is None:
        assert torch.equal(sa, sb)


# ----------------------------------------------------------------------------- 4, 5. gradients through ops
def device_backward(cs, dev, combo, precision=None, use_state=False, rays=False, **kw):
    """ops.raymarch_rays(samples=True), ops.raymarch_rays_bwd(g_weights=, + the upstreams of `combo` or none), and with `rays`
    ops.raymarch_rays_bwd_rays on its records -> (result of the backward, device depths, (d_o, d_d) or None)."""
    from hfa_gp_amd import ops
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev, precision)
    cfg = cs["cfg"]
    state = ops.raymarch_rays_state(B, cs["r"], cfg.depth_resolution, cfg.depth_resolution_importance, dev) if use_state else None
    _, _, _, tmm, _, ts = ops.raymarch_rays(pl, o, d, us, ui, state=state, samples=True, **lim, **args)
    ups = {k: (cs["ups"][k].to(dev) if combo and use else None) for use, k in zip(COMBOS[combo or "all"], KEYS)}
    rec = []
    out = ops.raymarch_rays_bwd(ups["g_feat"], pl, o, d, us, ui, state=state, g_depth=ups["g_depth"], g_wsum=ups["g_wsum"],
                                depth_range=ops.depth_range(tmm, empty_rays=bool(lim)) if ups["g_depth"] is not None else None,
                                rec_out=rec, g_weights=g_weights(cs).to(dev), **lim, **args, **kw)
    dod = ops.raymarch_rays_bwd_rays(ups["g_feat"], pl, rec[0], o, d, us, ui, **lim, **args) if rays else None
    return out, ts, dod


def reference_grads(cs, ts, combo, limits=None):
    """float64 autograd through weights_at at the device's depths, plus the existing fp32 reference terms of `combo`."""
    pl, dec, rays = SR.weight_grads(cs, ts, g_weights(cs))
    if combo:
        epl, edec, erays = (TL.RL if limits else TR).reference(cs, combo)
        pl, dec, rays = pl + epl, tuple(a + b for a, b in zip(dec, edec)), rays + erays
    return pl, dec, rays


@pytest.mark.parametrize("combo", [None, "all"], ids=["alone", "with-feat-depth-wsum"])
@pytest.mark.parametrize("preset", PRESETS3)
def test_plane_grads(dev, preset, combo):
    cs = SR.inputs(preset)
    dpl, ts, _ = device_backward(cs, dev, combo)
    close_grad(dpl.permute(0, 1, 4, 2, 3), reference_grads(cs, ts, combo)[0], f"{preset}/{combo}")


@pytest.mark.parametrize("combo", [None, "all"], ids=["alone", "with-feat-depth-wsum"])
@pytest.mark.parametrize("variant", ["state", "scatter", "state_scatter", "decoder_grads", "decoder_grads_scatter", "fp32", "box"])
def test_plane_and_decoder_grads_variants_small128(dev, variant, combo):
    """The compositing adjoint from the forward's state; pass 2 as scatter instead of sort + gather; the decoder gradients in both
    forms; the fp32 decoder; per-ray limits with empty rays (whose g_weights must not be read: it is NaN there)."""
    limits = "box" if variant == "box" else None
    cs = SR.inputs("small128", limits)
    kw = dict(use_state=variant.startswith("state"), decoder_grads=variant.startswith("decoder_grads"))
    if variant.endswith("scatter"):
        kw["rows"] = False
    if variant == "fp32":
        kw["precision"] = "fp32"
    out, ts, _ = device_backward(cs, dev, combo, **kw)
    ref_pl, ref_dec, _ = reference_grads(cs, ts, combo, limits)
    dpl, dec = out if kw["decoder_grads"] else (out, None)
    close_grad(dpl.permute(0, 1, 4, 2, 3), ref_pl, f"{variant}/{combo}/planes")
    if dec is not None:
        for got, ref, k in zip(dec, ref_dec, DEC_KEYS):
            close_grad(got, ref, f"{variant}/{combo}/{k}")


def test_state_against_recompute(dev):
    """Pass 1 from the forward's state and pass 1 recomputing the forward: the records to close_grad's bar (the two paths may
    differ in the last bit), so everything after them agrees as it does for the other upstream gradients."""
    from hfa_gp_amd import ops
    cs = SR.inputs("small128")
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev)
    cfg = cs["cfg"]
    state = ops.raymarch_rays_state(B, R, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
    ops.raymarch_rays(pl, o, d, us, ui, state=state, **args)
    gw = g_weights(cs).to(dev)
    recs = []
    for st in (None, state):
        ops.raymarch_rays_bwd(None, pl, o, d, us, ui, state=st, g_weights=gw, rec_out=recs, **args)
    assert bool(recs[0][..., 2].abs().sum() > 0)
    close_grad(recs[1], recs[0].cpu(), "records: state vs recompute")


def test_empty_rays_g_weights_is_not_read(dev):
    from hfa_gp_amd import ops
    cs = SR.inputs("small128", "box")
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev)
    empty = ~SR.reference("small128", "box")["valid"]
    gw = g_weights(cs)
    ref = ops.raymarch_rays_bwd(None, pl, o, d, us, ui, g_weights=gw.to(dev), **lim, **args)
    gw[empty] = float("nan")
    rec = []
    got = ops.raymarch_rays_bwd(None, pl, o, d, us, ui, g_weights=gw.to(dev), rec_out=rec, **lim, **args)
    assert torch.isfinite(got).all() and not bool(rec[0].cpu()[empty].any())
    scale = ref.abs().max().item()
    assert scale > 0 and (got - ref).abs().max().item() <= 2e-5 * scale          # (atomics: the order of the sums is not fixed)


def test_scratch_cap_slices_g_weights_with_the_chunk(dev, monkeypatch):
    from hfa_gp_amd import ops
    cs = SR.inputs("small128")
    (whole, dec_w), ts, _ = device_backward(cs, dev, "all", decoder_grads=True)
    need = ops.ROWS_STATS["bytes"]
    monkeypatch.setenv("HFAGP_RAYBWD_SCRATCH_GIB", repr(need / 3 / 2 ** 30))
    (cut, dec_c), _, _ = device_backward(cs, dev, "all", decoder_grads=True)
    assert ops.ROWS_STATS["path"] == "rows" and ops.ROWS_STATS["chunks"] >= 4, ops.ROWS_STATS
    ref_pl, ref_dec, _ = reference_grads(cs, ts, "all")
    close_grad(cut.permute(0, 1, 4, 2, 3), ref_pl, "chunked/planes")
    for got, ref, k in zip(dec_c, ref_dec, DEC_KEYS):
        close_grad(got, ref, f"chunked/{k}")
    scale = whole.abs().max().item()
    assert (cut - whole).abs().max().item() <= 2e-5 * scale


@pytest.mark.parametrize("combo", [None, "all"], ids=["alone", "with-feat-depth-wsum"])
@pytest.mark.parametrize("preset", PRESETS3)
def test_ray_grads(dev, preset, combo):
    """d origins / d directions through the EXISTING rays' pass on the records of the samples backward."""
    cs = SR.inputs(preset)
    _, ts, (d_o, d_d) = device_backward(cs, dev, combo, rays=True)
    assert d_o.shape == d_d.shape == (B, R, 3) and MAX_EDGE_RAYS == 4
    check_rays(torch.cat((d_o, d_d), -1), reference_grads(cs, ts, combo)[2], f"{preset}/{combo}")


def test_ray_grads_with_limits(dev):
    cs = SR.inputs("small128", "box")
    _, ts, (d_o, d_d) = device_backward(cs, dev, "all", rays=True)
    empty = ~SR.reference("small128", "box")["valid"]
    assert not bool(d_o.cpu()[empty].any()) and not bool(d_d.cpu()[empty].any())
    check_rays(torch.cat((d_o, d_d), -1), reference_grads(cs, ts, "all", "box")[2], "box/all")


# ----------------------------------------------------------------------------- launches
RAY_ENTRIES = ("hfagp_raymarch_rays_fwd", "hfagp_raymarch_rays_bwd", "hfagp_raymarch_rays_bwd_rays", "hfagp_raymarch_rays_limits_fwd",
               "hfagp_raymarch_rays_limits_bwd", "hfagp_raymarch_rays_limits_bwd_rays", "hfagp_raymarch_rays_samples_fwd",
               "hfagp_raymarch_rays_samples_bwd", "hfagp_raymarch_rays_normals", "hfagp_raymarch_rays_normals_bwd",
               "hfagp_raymarch_rays_normals_bwd_rays")


def count_entries(monkeypatch):
    """Wraps the list entry points of the loaded library; returns the list their names are appended to, call by call."""
    from hfa_gp_amd import _lib
    handle, calls = _lib.lib(), []
    for name in RAY_ENTRIES:
        fn = getattr(handle, name)

        def wrapped(*a, _fn=fn, _name=name):
            calls.append(_name.replace("hfagp_raymarch_rays_", ""))
            return _fn(*a)
        monkeypatch.setattr(handle, name, wrapped)
    return calls


def _tiny_gen(dev, tuned=False, **kw):
    from hfa_gp_amd.config import PRESETS
    from hfa_gp_amd.generator import TriPlaneGenerator
    cfg = dataclasses.replace(PRESETS["tiny64"](), **kw)
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    return cfg, gen


def test_launches_and_keys(dev, monkeypatch):
    """Without samples= the call launches what it launched and returns its four keys; with it the samples entries replace the
    forward and the backward launch, and the rays get their gradient from the existing rays' pass — no launch of its own."""
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _tiny_gen(dev)
    ws, c, _, _ = (t.to(dev) for t in make_inputs(cfg, 2))
    o, d = ray_grid(c, 6)
    s = cfg.depth_resolution + cfg.depth_resolution_importance
    calls = count_entries(monkeypatch)
    ws.requires_grad_(True)
    o_g = o.clone().requires_grad_(True)
    out = gen.render_rays(ws, o_g, d)
    assert set(out) == {"feature", "rgb", "depth", "mask"}
    (out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()).backward()
    assert calls == ["fwd", "bwd", "bwd_rays"], calls
    del calls[:]
    with torch.no_grad():
        assert set(gen.render_rays(ws, o, d, ray_limits="box")) == {"feature", "rgb", "depth", "mask", "valid"}
    assert calls == ["limits_fwd"], calls
    del calls[:]
    ws.grad = o_g.grad = None
    out = gen.render_rays(ws, o_g, d, samples=True)
    assert set(out) == {"feature", "rgb", "depth", "mask", "sample_weights", "sample_depths"}
    assert out["sample_weights"].shape == (2, 36, s - 1) and out["sample_depths"].shape == (2, 36, s)
    assert out["sample_weights"].requires_grad and not out["sample_depths"].requires_grad
    out["sample_weights"].square().sum().backward()          # only the weights carry a gradient: the launch runs for them alone
    assert calls == ["samples_fwd", "samples_bwd", "bwd_rays"], calls
    assert bool(ws.grad.abs().sum() > 0) and bool(o_g.grad.abs().sum() > 0)
    del calls[:]
    out = gen.render_rays(ws, o_g, d, samples=True, ray_limits="box")
    out["rgb"].square().sum().backward()                     # a loss that ignores the weights: the launch it ran before
    assert calls == ["samples_fwd", "limits_bwd", "limits_bwd_rays"], calls
    del calls[:]
    with torch.no_grad():
        out = gen.render_rays(ws, o, d, samples=True, normals=True)
    assert calls == ["samples_fwd", "normals"] and not any(v.requires_grad for v in out.values())


def test_guards(dev):
    from hfa_gp_amd import ops
    cs = SR.inputs("small128")
    pl, o, d, us, ui, lim, args = device_inputs(cs, dev)
    with pytest.raises(RuntimeError, match="g_weights must be"):
        ops.raymarch_rays_bwd(None, pl, o, d, us, ui, g_weights=torch.zeros(B, R, 64, device=dev), **args)
    with pytest.raises(RuntimeError, match="g_weights must be"):
        ops.raymarch_rays_bwd(None, pl, o, d, us, ui, g_weights=torch.zeros(B, R - 1, 63, device=dev), **args)
    with pytest.raises(RuntimeError, match="no upstream gradient"):
        ops.raymarch_rays_bwd(None, pl, o, d, us, ui, **args)
    cfg, gen = _tiny_gen(dev)
    ws = make_inputs(cfg, 2)[0].to(dev)
    s = cfg.depth_resolution + cfg.depth_resolution_importance
    out = gen.render_rays(ws, torch.zeros(2, 0, 3, device=dev), torch.zeros(2, 0, 3, device=dev), samples=True)
    assert out["sample_depths"].shape == (2, 0, s) and out["sample_weights"].shape == (2, 0, s - 1)
    o = torch.zeros(2, 5, 3, device=dev)
    o[..., 2] = 2.7
    d = torch.zeros(2, 5, 3, device=dev)
    d[..., 2] = -1.0
    out = gen.render_rays(ws.clone().requires_grad_(True), o, d, samples=True)
    loss = out["sample_weights"].sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="backward called a second time"):
        loss.backward()


def test_above_the_state_cap(dev, monkeypatch):
    """No per-sample state is kept above RAY_STATE_CAP_BYTES: the same weights, and their gradient from the recomputing pass 1."""
    from hfa_gp_amd import generator
    cfg, gen = _tiny_gen(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    from hfa_gp_amd.cam_utils import ray_grid
    o, d = ray_grid(c, 6)
    us, ui = us[:, :36, :, 0].contiguous(), ui.reshape(2, -1, ui.shape[-1])[:, :36].reshape(72, -1).contiguous()
    res = []
    for cap in (None, 1000):
        if cap is not None:
            monkeypatch.setattr(generator, "RAY_STATE_CAP_BYTES", cap)
        w = ws.clone().requires_grad_(True)
        out = gen.render_rays(w, o, d, us, ui, samples=True)
        out["sample_weights"].square().sum().backward()
        with torch.no_grad():
            nog = gen.render_rays(w, o, d, us, ui, samples=True, normals=True)
        assert torch.equal(nog["sample_weights"], out["sample_weights"]) and torch.equal(nog["sample_depths"], out["sample_depths"])
        res.append((out["sample_weights"].detach(), out["sample_depths"], w.grad))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    close_grad(res[1][2], res[0][2].cpu(), "d ws: recompute vs state")


# ----------------------------------------------------------------------------- 6. end to end
def _e2e_loss(rgb, sample_depths, sample_weights, target, t_range):
    from hfa_gp_amd.ray_losses import distortion_loss
    return distortion_loss(sample_depths, sample_weights, t_range).mean() + (rgb - target).square().mean()


@functools.lru_cache(maxsize=None)
def e2e_reference():
    """The oracle-backed step: backbone_synthesis -> ray_sampler -> the restated renderer, every generator parameter, ws and c
    leaves; the inputs of test_render_rays_end_to_end."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = TR._e2e_cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    for k, v in P.items():
        if v.is_floating_point() and not k.startswith("backbone.mapping."):
            v.requires_grad_(True)
    ws, c, us, ui, terms = TR._e2e_inputs(cfg)
    ws_ref, c_ref = ws.clone().requires_grad_(True), c.clone().requires_grad_(True)
    o, d = O.ray_sampler(c_ref[:, :16].reshape(-1, 4, 4), c_ref[:, 16:25].reshape(-1, 3, 3), TR.E2E_RES)
    planes = O.backbone_synthesis(P, cfg, ws_ref)
    planes5 = planes.reshape(2, 3, cfg.plane_channels, planes.shape[-2], planes.shape[-1])
    out = SR.render(P, cfg, planes5, o, d, us, ui)
    assert float(out["wsum"].detach().min()) >= MIN_OPACITY
    _e2e_loss(out["feat"][..., :3], out["t"], out["w"], terms[0][..., :3], (cfg.ray_start, cfg.ray_end)).backward()
    return P, ws_ref.grad, c_ref.grad, out["w"].detach()


def test_render_rays_samples_end_to_end(dev):
    """tiny64, fp32 convs, generator tuned, ws and c leaves (c through ray_grid): distortion loss + L2 on 'rgb' through
    render_rays(samples=True) against the oracle-backed step, at the bars of test_render_rays_end_to_end."""
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _tiny_gen(dev, tuned=True, conv_precision="fp32")
    P, ws_g, c_g, w_ref = e2e_reference()
    ws, c, us, ui, terms = TR._e2e_inputs(cfg)
    ws_d, c_d = ws.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
    o, d = ray_grid(c_d, TR.E2E_RES)
    out = gen.render_rays(ws_d, o, d, us.to(dev), ui.to(dev), samples=True)
    close(out["sample_weights"].sum(-1), w_ref.sum(-1), atol=1e-5, rtol=0.0, what="sum of the weights")
    _e2e_loss(out["rgb"], out["sample_depths"], out["sample_weights"], terms[0][..., :3].to(dev), (cfg.ray_start, cfg.ray_end)).backward()
    close(ws_d.grad, ws_g, atol=2e-4 * ws_g.abs().max().item(), rtol=2e-3, what="d ws")
    close(c_d.grad, c_g, atol=2e-4 * c_g.abs().max().item(), rtol=2e-3, what="d c")
    n = "decoder.net.0.weight"
    refg = P[n].grad
    close(dict(gen.named_parameters())[n].grad, refg, atol=2e-4 * refg.abs().max().item(), rtol=2e-3, what=n)


def test_samples_with_normal_grad_is_the_sum_of_its_terms(dev):
    """samples=True with normal_grad=True (and the rays' opt-in): the gradients of a loss on both equal the sum of the two
    single-term calls'."""
    from hfa_gp_amd.cam_utils import ray_grid
    cfg, gen = _tiny_gen(dev, tuned=True, conv_precision="fp32")
    ws, c, us, ui, _ = TR._e2e_inputs(cfg)
    g = torch.Generator().manual_seed(G_SEED)
    r = TR.E2E_RES ** 2
    gn = torch.randn(2, r, 3, generator=g).to(dev)
    gw = torch.randn(2, r, cfg.depth_resolution + cfg.depth_resolution_importance - 1, generator=g).to(dev)
    dec = dict(gen.named_parameters())["decoder.net.0.weight"]

    def run(use_w, use_n):
        ws_d, c_d = ws.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
        o, d = ray_grid(c_d, TR.E2E_RES)
        out = gen.render_rays(ws_d, o, d, us.to(dev), ui.to(dev), samples=True, normal_ray_grad=True)
        loss = (out["sample_weights"] * gw).sum() * float(use_w) + (out["normal"] * gn).sum() * float(use_n)
        gen.zero_grad(set_to_none=True)
        loss.backward(inputs=[ws_d, c_d, dec])
        return ws_d.grad.cpu(), c_d.grad.cpu(), dec.grad.cpu().clone()

    def only(use_w):
        ws_d, c_d = ws.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
        o, d = ray_grid(c_d, TR.E2E_RES)
        out = gen.render_rays(ws_d, o, d, us.to(dev), ui.to(dev), samples=use_w, normal_ray_grad=not use_w)
        loss = (out["sample_weights"] * gw).sum() if use_w else (out["normal"] * gn).sum()
        gen.zero_grad(set_to_none=True)
        loss.backward(inputs=[ws_d, c_d, dec])
        return ws_d.grad.cpu(), c_d.grad.cpu(), dec.grad.cpu().clone()

    both, a, b = run(True, True), only(True), only(False)
    for got, x, y, name in zip(both, a, b, ("d ws", "d c", "d decoder.net.0.weight")):
        assert bool(x.abs().sum() > 0) and bool(y.abs().sum() > 0)
        close_grad(got, x + y, name)
