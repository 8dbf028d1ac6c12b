"""Surface normals along ray lists on the device (hfagp_raymarch_rays_normals*, ops.raymarch_rays_normals / _bwd / _bwd_rays,
TriPlaneGenerator.render_rays(normals=, normal_grad=, normal_ray_grad=)) against the float64 references of
tests/rays_normals_ref.py.  Needs an MI355X:  python -m pytest tests -m gpu

B = 2, planes 20 x 20 (36 x 20 once), R <= 101: a partial 4-wave block, all three tile counts, both decoders.  The forward is held
to normals_ref's per-ray bar with at most MAX_EDGE_RAYS rays beyond it (each side draws its own fine depths).  The backward
references take the DEVICE's sorted depths (read from the state), the upstream gradient is multiplied by the reference's edge mask,
and the tolerance is the project's gradient bar times max(1, 4 rho), rho = the fp32 reference's own worst err / bar on the same
inputs, recomputed in the run (the rule and factor of tests/test_gpu_normal_grad.py).  Every comparison prints its figures."""
import functools

import pytest
import torch

from tests import normal_camera_ref as NC
from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests import rays_normals_ref as RN
from tests.test_gpu_normal_grad import _cfg, _gen, _gen_cpu, _inputs, _within, state_depths
from tests.util import make_inputs, state_cpu

pytestmark = pytest.mark.gpu

B, R = RN.B, RN.R
MISS = RN.RL.MISS
NEW_OPS = ("raymarch_rays_normals", "raymarch_rays_normals_bwd", "raymarch_rays_normals_bwd_rays")
# (preset, axes, plane (H, W), list, limits), decoder precision
FWD_CASES = [(("tiny64", "eg3d_original", (20, 20), "r27", None), None), (("small128", "eg3d_original", (20, 20), "r27", None), None),
             (("small128", "eg3d_original", (20, 20), "r27", None), "fp32"), (("ffhq512_128", "eg3d_original", (20, 20), "r27", None), None),
             (("small128", "eg3d_fixed", (36, 20), "r27", None), None)]
FWD_IDS = ["tiny64", "small128", "small128-fp32", "ffhq512_128", "small128-fixed-36x20"]
MISS_KEY = ("small128", "eg3d_original", (20, 20), "miss", "box")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def device_inputs(cs, dev, precision=None, keep=None):
    """(planes, the keyword arguments of the three list normals ops) on the device; `keep` [R] bool: that subset of the rays."""
    cut = (lambda t: t) if keep is None else (lambda t: t[:, keep].contiguous())
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    sf = cs["ui"].shape[-1]
    kw = dict(cs["gen"].to(dev)._rays_kwargs(), ray_origins=cut(cs["o"]).to(dev), ray_directions=cut(cs["d"]).to(dev),
              u_strat=cut(cs["us"][..., 0]).to(dev), u_imp=cut(cs["ui"].view(B, -1, sf)).reshape(-1, sf).to(dev))
    if cs["lim"] is not None:
        kw.update(t_near=cut(cs["lim"][0]).to(dev), t_far=cut(cs["lim"][1]).to(dev))
    if precision is not None:
        kw["decoder_precision"] = precision
    return pl, kw


def forward(pl, kw, dev, nan_state=False):
    """ops.raymarch_rays with a state (pre-filled with NaN on request), then the normals -> (state, wsum, normal)."""
    from hfa_gp_amd import ops
    b, r = kw["ray_origins"].shape[:2]
    state = ops.raymarch_rays_state(b, r, kw["u_strat"].shape[-1], kw["u_imp"].shape[-1], dev)
    if nan_state:
        state.fill_(float("nan"))
    march = {k: v for k, v in kw.items() if k not in ("ray_origins", "ray_directions", "u_strat", "u_imp")}
    _, _, wsum, _ = ops.raymarch_rays(pl, kw["ray_origins"], kw["ray_directions"], kw["u_strat"], kw["u_imp"], state=state, **march)
    return state, wsum, ops.raymarch_rays_normals(pl, state, **kw)


@functools.lru_cache(maxsize=None)
def device_case(dev, key, precision=None, nan_state=False):
    """One forward, one call of each backward op and the float64 references on the device's depths (computed once, left unchanged)."""
    from hfa_gp_amd import ops
    cs = RN.case(*key)
    pl, kw = device_inputs(cs, dev, precision)
    state, wsum, normal = forward(pl, kw, dev, nan_state)
    s = kw["u_strat"].shape[-1] + kw["u_imp"].shape[-1]
    valid = None if cs["lim"] is None else RN.RL.valid_rays(*cs["lim"])
    depths = state_depths(state, s)
    g_hat, mask = RN.masked_upstream(cs, depths, valid)
    g_dev = g_hat.float().to(dev)
    d_planes, dec = ops.raymarch_rays_normals_bwd(g_dev, pl, state, decoder_grads=True, **kw)
    d_o, d_d = ops.raymarch_rays_normals_bwd_rays(g_dev, pl, state, **kw)
    ref = RN.grad_reference(cs["P"], cs["cfg"], cs["planes"], cs["o"], cs["d"], depths, g_hat, valid=valid)
    low = RN.grad_reference(cs["P"], cs["cfg"], cs["planes"], cs["o"], cs["d"], depths, g_hat, dtype=torch.float32, valid=valid)
    rho = G.rho(low, ref, f"{key}: fp32 reference")[0]
    rho_rays = G.bar_ratio(low["rays"], ref["rays"])
    got = dict(planes=d_planes.permute(0, 1, 4, 2, 3), dec=dec, rays=torch.cat((d_o, d_d), -1))
    return dict(cs=cs, pl=pl, kw=kw, state=state, wsum=wsum, normal=normal, valid=valid, g_hat=g_dev, mask=mask, got=got, ref=ref,
                factor=max(1.0, 4.0 * rho), factor_rays=max(1.0, 4.0 * rho_rays))


# ----------------------------------------------------------------------------- 1. forward against float64
@pytest.mark.parametrize("key,precision", FWD_CASES, ids=FWD_IDS)
def test_forward_vs_float64_reference(dev, key, precision):
    cs = RN.case(*key)
    pl, kw = device_inputs(cs, dev, precision)
    _, wsum, normal = forward(pl, kw, dev)
    ref = RN.case_reference(*key)
    assert normal.shape == (B, R, 3) and float(ref["normal"].norm(dim=-1).max()) > 0.05
    bad = N.rays_beyond(normal, ref["normal"], f"{key}/{precision}: device")
    assert bad <= N.MAX_EDGE_RAYS, bad
    over = float((normal.norm(dim=-1) - wsum).max())
    print(f"max (|N| - wsum) {over:.3e}")
    assert over <= 1e-6
    _, _, again = forward(pl, kw, dev)
    assert torch.equal(_bits(normal), _bits(again))


@pytest.mark.parametrize("r", [1, 4, 5])
def test_forward_short_lists(dev, r):
    """One ray, one full 4-wave block, one block and a ray.  MAX_EDGE_RAYS is 4 rays of 200 — one in 50 — so among at most 10 rays
    none is allowed beyond the bar."""
    key = ("tiny64", "eg3d_original", (20, 20), "r27", None, r)
    pl, kw = device_inputs(RN.case(*key), dev)
    _, wsum, normal = forward(pl, kw, dev)
    assert normal.shape == (B, r, 3)
    assert N.rays_beyond(normal, RN.case_reference(*key)["normal"], f"R = {r}") == 0
    assert float((normal.norm(dim=-1) - wsum).max()) <= 1e-6


# ----------------------------------------------------------------------------- 2. limits and empty rays
def test_limits_empty_rays_are_zero_and_read_no_state(dev):
    """The "miss" list under box limits on a state pre-filled with NaN: the 40 missed rays' state stays unwritten, so a kernel that
    read any of it would hand back something that is not finite."""
    dc = device_case(dev, MISS_KEY, None, True)
    normal, state = dc["normal"], dc["state"]
    assert torch.equal(dc["valid"], ~MISS)
    assert bool(torch.isnan(state[MISS.to(dev)]).all()), "the forward wrote an empty ray's state"
    s = dc["kw"]["u_strat"].shape[-1] + dc["kw"]["u_imp"].shape[-1]
    assert bool(torch.isfinite(state[(~MISS).to(dev)][..., 32 * s: 34 * s]).all())          # (depths and densities of the valid rays)
    assert bool((_bits(normal)[MISS.to(dev)] == 0).all()), "an empty ray's normal is not three +0.0"
    ref = RN.case_reference(*MISS_KEY)
    bad = N.rays_beyond(normal, ref["normal"], "miss list, box limits: device")
    assert bad <= N.MAX_EDGE_RAYS, bad
    assert float(normal[(~MISS).to(dev)].norm(dim=-1).max()) > 0.05
    for t in (dc["got"]["planes"], dc["got"]["rays"]) + tuple(dc["got"]["dec"]):
        assert bool(torch.isfinite(t).all())
    assert bool((_bits(dc["got"]["rays"])[MISS.to(dev)] == 0).all()), "an empty ray's gradient is not six +0.0"


def test_limits_on_the_mixed_list(dev):
    """The "mixed" list under box limits (cameras nearer and farther than the config's interval, directions of lengths 0.5 ... 2):
    every ray valid; the float64 reference with limits at the bar."""
    key = ("small128", "eg3d_original", (20, 20), "mixed", "box")
    pl, kw = device_inputs(RN.case(*key), dev)
    _, wsum, normal = forward(pl, kw, dev, nan_state=True)
    bad = N.rays_beyond(normal, RN.case_reference(*key)["normal"], "mixed list, box limits: device")
    assert bad <= N.MAX_EDGE_RAYS and float((normal.norm(dim=-1) - wsum).max()) <= 1e-6


# ----------------------------------------------------------------------------- 3. the grid as a list
def test_grid_as_a_list_is_image_normal(dev):
    from hfa_gp_amd.cam_utils import ray_grid
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    res = cfg.neural_rendering_resolution
    with torch.no_grad():
        grid = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, normals=True)["image_normal"]
        o, d = ray_grid(c, res)
        out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True)
    assert set(out) == {"feature", "rgb", "depth", "mask", "normal"} and out["normal"].shape == (B, res * res, 3)
    want = grid.permute(0, 2, 3, 1).reshape(B, res * res, 3)
    bad = N.rays_beyond(out["normal"], want, "render_rays(ray_grid) against synthesis")
    print(f"{bad} rays beyond the bar (allowed {2 * N.MAX_EDGE_RAYS}); bit-equal: {torch.equal(out['normal'], want)}")
    assert bad <= 2 * N.MAX_EDGE_RAYS and float(want.norm(dim=-1).max()) > 0


# ----------------------------------------------------------------------------- 4. plane and decoder gradients
@pytest.mark.parametrize("key,precision", FWD_CASES, ids=FWD_IDS)
def test_plane_and_decoder_gradients_vs_float64(dev, key, precision):
    """Measured on an MI355X, worst err / bar (d_planes, then the worst decoder gradient) against the allowed max(1, 4 rho):
    tiny64 0.059 / 0.032 (1.00); small128 0.064 / 0.077 (1.06); small128-fp32 0.044 / 0.070 (1.07); ffhq512_128 0.030 / 0.063
    (1.00); small128-fixed-36x20 0.066 / 0.050 (1.00).  With the decoder adjoint a = W0'^T dH taken from split-bf16 products, as the
    grid kernel takes it with the 16-bit decoder, the small128 case stood at 1.094 / 0.94 and missed its allowance; the list form
    therefore forms a on the exact fp32 MFMA with either decoder (raymarch_normals_bwd.hip's note)."""
    dc = device_case(dev, key, precision)
    worst, _ = G.rho(dc["got"], dc["ref"], f"{key}/{precision}: device")
    print(f"tolerance factor {dc['factor']:.2f}, {int(dc['mask'].sum())} of {dc['mask'].numel()} rays kept")
    assert float(dc["ref"]["planes"].abs().max()) > 1e-3
    assert worst <= dc["factor"], f"worst err / bar {worst:.3f} > {dc['factor']:.2f}"


def test_gradients_accumulate_and_zero_upstream_touches_nothing(dev):
    from hfa_gp_amd import ops
    dc = device_case(dev, FWD_CASES[0][0])
    g = torch.Generator().manual_seed(21)
    pre = torch.randn(dc["pl"].shape, generator=g).to(dev)
    pre[0, 0, 0, 0, :4] = -0.0
    pre_dec = tuple(torch.randn(t.shape, generator=g).to(dev) for t in dc["got"]["dec"])
    acc, acc_dec = pre.clone(), tuple(t.clone() for t in pre_dec)
    ops.raymarch_rays_normals_bwd(torch.zeros_like(dc["g_hat"]), dc["pl"], dc["state"], d_planes=acc, decoder_grads=True,
                                  dec_out=acc_dec, **dc["kw"])
    assert torch.equal(_bits(acc), _bits(pre)) and all(torch.equal(_bits(a), _bits(p)) for a, p in zip(acc_dec, pre_dec))
    out, dec = ops.raymarch_rays_normals_bwd(dc["g_hat"], dc["pl"], dc["state"], d_planes=acc, decoder_grads=True, dec_out=acc_dec,
                                             **dc["kw"])
    assert out is acc and all(a is b for a, b in zip(dec, acc_dec))

    def summed(got, pre_t, fresh_t, what):       # (tests/test_gpu_normal_grad.py: the bar with its atol scaled by what is summed)
        err = (got - pre_t - fresh_t).abs()
        bound = 2e-5 * max(1.0, float(pre_t.abs().max() + fresh_t.abs().max())) + 1e-3 * fresh_t.abs()
        print(f"{what}: worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), what

    summed(out, pre, dc["got"]["planes"].permute(0, 1, 3, 4, 2), "d_planes")
    for got, p, f, k in zip(dec, pre_dec, dc["got"]["dec"], G.DEC_KEYS):
        summed(got, p, f, k)
    frozen, none = ops.raymarch_rays_normals_bwd(dc["g_hat"], dc["pl"], dc["state"], **dc["kw"])
    assert none is None and G.bar_ratio(frozen.permute(0, 1, 4, 2, 3), dc["got"]["planes"]) <= 1.0


def test_missed_rays_contribute_nothing(dev):
    """The "miss" list's gradients against those of the same list with the 40 missed rays removed: the bar, no factor."""
    from hfa_gp_amd import ops
    dc = device_case(dev, MISS_KEY, None, True)
    keep = ~MISS[0]
    pl, kw = device_inputs(dc["cs"], dev, keep=keep)
    state, _, normal = forward(pl, kw, dev)
    assert torch.equal(_bits(normal), _bits(dc["normal"][:, keep.to(dev)]))
    g_cut = dc["g_hat"][:, keep.to(dev)].contiguous()
    d_planes, dec = ops.raymarch_rays_normals_bwd(g_cut, pl, state, decoder_grads=True, **kw)
    part = dict(planes=d_planes.permute(0, 1, 4, 2, 3), dec=dec)
    worst, _ = G.rho(dc["got"], part, "miss list against the list without the missed rays")
    assert float(d_planes.abs().max()) > 1e-3 and worst <= 1.0
    d_o, d_d = ops.raymarch_rays_normals_bwd_rays(g_cut, pl, state, **kw)
    assert torch.equal(_bits(torch.cat((d_o, d_d), -1)), _bits(dc["got"]["rays"][:, keep.to(dev)]))


# ----------------------------------------------------------------------------- 5. ray gradients
@pytest.mark.parametrize("key,precision", FWD_CASES, ids=FWD_IDS)
def test_ray_gradients_vs_float64(dev, key, precision):
    from hfa_gp_amd import ops
    dc = device_case(dev, key, precision)
    got, ref = dc["got"]["rays"], dc["ref"]["rays"]
    ratio = G.bar_ratio(got, ref)
    print(f"{key}/{precision}: rays' gradient worst err / bar {ratio:.3f} (allowed {dc['factor_rays']:.2f}), max |ref| "
          f"{float(ref.abs().max()):.3e}")
    assert float(ref.abs().max()) > 1e-3 and ratio <= dc["factor_rays"]
    d_o, d_d = ops.raymarch_rays_normals_bwd_rays(dc["g_hat"], dc["pl"], dc["state"], **dc["kw"])
    assert torch.equal(_bits(torch.cat((d_o, d_d), -1)), _bits(got))
    dropped = ~dc["mask"].to(dev)                       # G^ = 0 there: six zero floats
    assert bool((got[dropped] == 0).all())


def test_ray_gradients_accumulate_onto_the_colour_terms(dev):
    """accumulate=1 on top of what ops.raymarch_rays_bwd_rays wrote = the sum (one fp32 addition per float: exact); an empty ray's
    six floats are left alone."""
    from hfa_gp_amd import ops
    dc = device_case(dev, MISS_KEY, None, True)
    pl, kw = dc["pl"], dc["kw"]
    rays = (kw["ray_origins"], kw["ray_directions"], kw["u_strat"], kw["u_imp"])
    rest = {k: v for k, v in kw.items() if k not in ("ray_origins", "ray_directions", "u_strat", "u_imp")}
    g_feat = torch.randn(B, R, 32, generator=torch.Generator().manual_seed(5)).to(dev)
    rec = []
    ops.raymarch_rays_bwd(g_feat, pl, *rays, rec_out=rec, **rest)
    c_o, c_d = ops.raymarch_rays_bwd_rays(g_feat, pl, rec[0], *rays, **rest)
    assert float(c_o.abs().max()) > 0 and bool((c_o[MISS.to(dev)] == 0).all())
    marked = c_o.clone(), c_d.clone()
    marked[0][MISS.to(dev)] = 7.0                        # (an accumulating call must not touch an empty ray)
    marked[1][MISS.to(dev)] = -7.0
    want = torch.cat(marked, -1) + dc["got"]["rays"]
    a_o, a_d = ops.raymarch_rays_normals_bwd_rays(dc["g_hat"], pl, dc["state"], d_origins=marked[0], d_directions=marked[1], **kw)
    assert a_o is marked[0] and a_d is marked[1]
    assert torch.equal(_bits(torch.cat((a_o, a_d), -1)), _bits(want))
    with pytest.raises(RuntimeError, match="d_origins and d_directions go together"):
        ops.raymarch_rays_normals_bwd_rays(dc["g_hat"], pl, dc["state"], d_origins=marked[0], **kw)
    with pytest.raises(RuntimeError, match="g_normal must be"):
        ops.raymarch_rays_normals_bwd_rays(dc["g_hat"][:, :7].contiguous(), pl, dc["state"], **kw)
    with pytest.raises(RuntimeError, match="state must be"):
        ops.raymarch_rays_normals(pl, dc["state"][:, :7].contiguous(), **kw)


# ----------------------------------------------------------------------------- 6. end to end: tiny64
def _list_inputs(dev, grad_rays=False):
    """ws, the 2 x 101 list and its uniforms for the tiny64 generator of tests/test_gpu_normal_grad.py."""
    cfg = _cfg()
    ws = _inputs(dev)[0].requires_grad_(True)
    o, d = (t.to(dev).requires_grad_(grad_rays) for t in RN.RL.ray_list())
    g = torch.Generator().manual_seed(31)
    us = torch.rand(B, R, cfg.depth_resolution, generator=g).to(dev)
    ui = torch.rand(B * R, cfg.depth_resolution_importance, generator=g).to(dev)
    return ws, o, d, us, ui


def _recorded_states(monkeypatch, ops):
    states, inner = [], ops.raymarch_rays
    monkeypatch.setattr(ops, "raymarch_rays", lambda *a, **k: states.append(k.get("state")) or inner(*a, **k))
    return states


def _float64_chain(o, d, depths, g_hat):
    """The oracle's backbone in float64 autograd feeding rays_normals_ref.grad_reference on the device's depths ->
    (d ws, the reference, rho of the fp32 reference on this set-up)."""
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in state_cpu(_gen_cpu()).items()}
    ws = make_inputs(cfg, B)[0].double().requires_grad_(True)
    planes = O.backbone_synthesis(P, cfg, ws).reshape(B, 3, 32, cfg.plane_resolution, cfg.plane_resolution)
    ref = RN.grad_reference(P, cfg, planes, o, d, depths, g_hat)
    d_ws, = torch.autograd.grad((planes * ref["planes"]).sum(), ws)
    low = RN.grad_reference(P, cfg, planes, o, d, depths, g_hat, dtype=torch.float32)
    return d_ws, ref, G.rho(low, ref, "tiny64 generator, list: fp32 reference")[0]


def test_render_rays_normal_grad_d_ws_vs_float64(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    hw = (cfg.plane_resolution, cfg.plane_resolution)
    states = _recorded_states(monkeypatch, ops)
    ws, o, d, us, ui = _list_inputs(dev)
    out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normal_grad=True)
    assert set(out) == {"feature", "rgb", "depth", "mask", "normal"} and out["normal"].requires_grad and len(states) == 1
    depths = state_depths(states[0], cfg.depth_resolution + cfg.depth_resolution_importance)
    o_cpu, d_cpu = RN.RL.ray_list()
    mask = RN.edge_mask(cfg, hw, o_cpu, d_cpu, depths)
    assert RN.kept(mask) >= G.MIN_KEPT
    g_hat = RN.upstream(B, R, 23) * mask[..., None]
    (out["normal"] * g_hat.float().to(dev)).sum().backward()
    with torch.no_grad():
        plain = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True)
    assert not plain["normal"].requires_grad
    for k in plain:
        assert torch.equal(out[k].detach(), plain[k]), k
    d_ws, ref, rho = _float64_chain(o_cpu, d_cpu, depths, g_hat)
    assert float(ref["normal"].norm(dim=-1).max()) > 0.01
    _within(ws.grad, d_ws, max(1.0, 4.0 * rho), "d ws of a normals-only loss on a list")


def test_render_rays_feature_and_normal_loss_is_the_sum(dev):
    gen = _gen(dev)
    t_f = torch.randn(B, R, 32, generator=torch.Generator().manual_seed(6)).to(dev) / R
    t_n = torch.randn(B, R, 3, generator=torch.Generator().manual_seed(7)).to(dev) / R

    def step(feature, normal):
        ws, o, d, us, ui = _list_inputs(dev)
        out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normal_grad=True)
        loss = 0
        if feature:
            loss = loss + (out["feature"] * t_f).sum()
        if normal:
            loss = loss + (out["normal"] * t_n).sum()
        loss.backward()
        return ws.grad

    both, f_only, n_only = step(True, True), step(True, False), step(False, True)
    assert float(f_only.abs().max()) > 0 and float(n_only.abs().max()) > 0
    _within(both, f_only + n_only, 1.0, "d ws of the joint loss against the sum of its parts")


def test_label_gradient_through_ray_grid_and_synthesis(dev, monkeypatch):
    """c.grad of a normals-only loss two ways — render_rays(normal_ray_grad=True) on ray_grid(c, res), torch autograd carrying the
    rays' gradient to the label, and synthesis(normal_camera_grad=True) — each against normal_camera_ref's float64 dL/dc on the
    depths of its own forward, under that file's factor rule."""
    from hfa_gp_amd import ops
    from hfa_gp_amd.cam_utils import ray_grid
    gen, cfg = _gen(dev), _cfg()
    res = cfg.neural_rendering_resolution
    s = cfg.depth_resolution + cfg.depth_resolution_importance
    hw = (cfg.plane_resolution, cfg.plane_resolution)
    c_cpu = make_inputs(cfg, B)[1]
    t = torch.randn(B, res * res, 3, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    P = state_cpu(_gen_cpu())

    def check(c_grad, planes, depths, g_hat, what):
        dc, dx = NC.reference(P, cfg, planes, c_cpu, depths, g_hat)
        dc32, dx32 = NC.reference(P, cfg, planes, c_cpu, depths, g_hat, dtype=torch.float32)
        factor = max(1.0, 4.0 * max(G.bar_ratio(dx32, dx), G.bar_ratio(dc32, dc)))
        ratio = G.bar_ratio(c_grad, dc)
        print(f"{what}: c.grad worst err / bar {ratio:.3f} (allowed {factor:.2f}), max |ref| {float(dc.abs().max()):.3e}")
        assert float(dc.abs().max()) > 1e-3 and ratio <= factor, what

    # the list
    list_states = _recorded_states(monkeypatch, ops)
    ws, c, us, ui = _inputs(dev)
    ws.requires_grad_(True)
    c.requires_grad_(True)
    out = gen.render_rays(ws, *ray_grid(c, res), u_strat=us, u_imp=ui, normal_ray_grad=True)
    depths = state_depths(list_states[0], s)
    mask = G.edge_mask(cfg, hw, c_cpu, depths)
    assert float(mask.double().mean()) >= G.MIN_KEPT
    (out["normal"] * (t * mask[..., None]).float().to(dev)).sum().backward()
    assert c.grad is not None and ws.grad is not None
    # the grid, and the planes of the call
    grid_states, inner = [], ops.raymarch
    monkeypatch.setattr(ops, "raymarch", lambda *a, **k: grid_states.append(k.get("state")) or inner(*a, **k))
    ws2, c2, us, ui = _inputs(dev)
    ws2.requires_grad_(True)
    c2.requires_grad_(True)
    img = gen.synthesis(ws2, c2, noise_mode="const", u_strat=us, u_imp=ui, normal_camera_grad=True, return_planes=True)
    depths2 = state_depths(grid_states[0], s)
    mask2 = G.edge_mask(cfg, hw, c_cpu, depths2)
    assert float(mask2.double().mean()) >= G.MIN_KEPT
    t_img = (t * mask2[..., None]).float().reshape(B, res, res, 3).permute(0, 3, 1, 2).to(dev)
    (img["image_normal"] * t_img).sum().backward()
    planes = img["planes"].detach().permute(0, 1, 4, 2, 3).cpu()
    print(f"the two forwards left bit-equal depths: {torch.equal(depths, depths2)}")
    check(c.grad, planes, depths, t * mask[..., None], "render_rays(normal_ray_grad=True) on ray_grid(c)")
    check(c2.grad, planes, depths2, t * mask2[..., None], "synthesis(normal_camera_grad=True)")
    assert bool((c.grad[:, NC.ZERO_COLUMNS] == 0).all())


# ----------------------------------------------------------------------------- 7. launch accounting, refusals, edges
def _counters(monkeypatch, ops):
    calls = {k: 0 for k in NEW_OPS}

    def wrap(name):
        inner = getattr(ops, name)

        def counted(*a, **k):
            calls[name] += 1
            return inner(*a, **k)
        return counted

    for name in NEW_OPS:
        monkeypatch.setattr(ops, name, wrap(name))
    return calls


def test_launch_accounting(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen = _gen(dev)
    calls = _counters(monkeypatch, ops)
    fwd, bwd, rays = NEW_OPS

    def step(use_normal, grad_rays=False, **kw):
        ws, o, d, us, ui = _list_inputs(dev, grad_rays)
        out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, **kw)
        loss = out["feature"].sum()
        if use_normal:
            loss = loss + out["normal"].square().sum()
        loss.backward()
        return out, ws, o

    out, ws_plain, _ = step(False)
    assert set(out) == {"feature", "rgb", "depth", "mask"} and sum(calls.values()) == 0
    with torch.no_grad():
        ws, o, d, us, ui = _list_inputs(dev)
        assert set(gen.render_rays(ws, o, d, u_strat=us, u_imp=ui)) == {"feature", "rgb", "depth", "mask"} and sum(calls.values()) == 0
        out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True)
    assert calls == {fwd: 1, bwd: 0, rays: 0} and not out["normal"].requires_grad
    out, _, _ = step(False, normals=True)                       # a detached map inside a differentiable call
    assert calls == {fwd: 2, bwd: 0, rays: 0} and not out["normal"].requires_grad and out["normal"].grad_fn is None
    out, ws_ignored, _ = step(False, normal_grad=True)          # a loss that ignores 'normal'
    assert calls == {fwd: 3, bwd: 0, rays: 0} and out["normal"].requires_grad
    _within(ws_ignored.grad, ws_plain.grad, 1.0, "d ws with 'normal' ignored against the plain step")
    step(True, normal_grad=True)
    assert calls == {fwd: 4, bwd: 1, rays: 0}
    step(True, normal_ray_grad=True)                            # the rays do not require grad: no rays' pass
    assert calls == {fwd: 5, bwd: 2, rays: 0}
    _, _, o = step(True, grad_rays=True, normal_ray_grad=True)
    assert calls == {fwd: 6, bwd: 3, rays: 1} and o.grad is not None and float(o.grad.abs().max()) > 0
    _, _, o = step(False, grad_rays=True, normal_ray_grad=True)  # rays with grad, a loss that ignores 'normal'
    assert calls == {fwd: 7, bwd: 3, rays: 1} and o.grad is not None


def test_refusals_come_before_any_launch(dev, monkeypatch):
    from hfa_gp_amd import generator as Gn
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    ws, o, d, us, ui = _list_inputs(dev)
    with torch.no_grad():
        whole = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True, ray_limits="box")
    per_ray = B * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    monkeypatch.setattr(Gn, "RAY_STATE_CAP_BYTES", 17 * per_ray)
    with torch.no_grad():                                        # above the cap without grad: chunks of 17 rays, the same bits
        parts = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True, ray_limits="box")
    for k in whole:
        assert torch.equal(whole[k], parts[k]), k
    # a detached map inside a differentiable call above the cap: the colours keep their graph, the normals come in chunks
    mixed = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normals=True, ray_limits="box")
    assert mixed["feature"].requires_grad and not mixed["normal"].requires_grad
    for k in whole:
        assert torch.equal(whole[k], mixed[k].detach()), k

    def boom(*a, **k):
        raise AssertionError("launched before the refusal")

    monkeypatch.setattr(ops, "raymarch_rays", boom)
    monkeypatch.setattr(ops, "ray_limits_box", boom)
    with pytest.raises(RuntimeError, match=rf"RAY_STATE_CAP_BYTES = {17 * per_ray}; 34 rays fit"):
        gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, normal_grad=True, ray_limits="box")
    monkeypatch.setattr(Gn, "RAY_STATE_CAP_BYTES", 8 << 30)
    with pytest.raises(NotImplementedError, match="rays' gradient of the normal term is opt-in"):
        gen.render_rays(ws, o.detach().requires_grad_(True), d, u_strat=us, u_imp=ui, normal_grad=True)


def test_empty_calls_and_empty_rays_through_render_rays(dev):
    gen = _gen(dev)
    ws, o, d, us, ui = _list_inputs(dev, grad_rays=True)
    for sl_b, sl_r in ((slice(0, 0), slice(None)), (slice(None), slice(0, 0))):
        out = gen.render_rays(ws[sl_b], o[sl_b, sl_r], d[sl_b, sl_r], normal_ray_grad=True)
        b, r = o[sl_b, sl_r].shape[:2]
        assert out["normal"].shape == (b, r, 3) and out["normal"].requires_grad
        out["normal"].sum().backward()
        assert ws.grad is not None and bool((ws.grad == 0).all()) and bool((o.grad == 0).all())
        assert not gen.render_rays(ws[sl_b], o[sl_b, sl_r], d[sl_b, sl_r], normals=True)["normal"].requires_grad
    # the "miss" list under box limits: an invalid ray's normal is exactly 0 and so is every gradient it gets
    ws, _, _, us, ui = _list_inputs(dev)
    o, d = (t.to(dev).requires_grad_(True) for t in RN.RL.miss_list())
    out = gen.render_rays(ws, o, d, u_strat=us, u_imp=ui, ray_limits="box", normal_ray_grad=True)
    miss = MISS.to(dev)
    assert torch.equal(out["valid"], ~miss) and bool((_bits(out["normal"].detach())[miss] == 0).all())
    assert bool(torch.isfinite(out["normal"]).all())
    (out["normal"].square().sum() + out["feature"].sum()).backward()
    for t in (o.grad, d.grad):
        assert bool(torch.isfinite(t).all()) and bool((t[miss] == 0).all()) and float(t[~miss].abs().max()) > 0
    assert bool(torch.isfinite(ws.grad).all()) and float(ws.grad.abs().max()) > 0
