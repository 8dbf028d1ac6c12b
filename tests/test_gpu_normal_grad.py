"""The gradient of the per-ray surface normals on the device (hfagp_raymarch_normals_bwd, ops.raymarch_normals_bwd,
synthesis(normal_grad=True)) against the float64 reference of tests/normal_grad_ref.py.  Needs an MI355X:  python -m pytest tests -m gpu

The reference takes the DEVICE's sorted sample depths (read from the ray marcher's state), so importance sampling drops out, and
the upstream gradient is multiplied by the reference's edge mask (rays with a sample within 1e-4 pixels of a texel edge, where the
density gradient jumps).  Tolerance per case: the project's gradient bar (atol 2e-5 max(1, max|ref|), rtol 1e-3) times
max(1, 4 rho), rho = the fp32 reference's own worst err / bar on that case, recomputed in the same run
(normal_grad_ref.oracle_rho); the factor 4 allows for the device's summation and atomic order, the split-operand decoder and the
hardware reciprocal square root.  Every comparison prints its worst err / bar."""
import dataclasses
import functools

import pytest
import torch

from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests.util import FLIP_COLUMNS, SYNTHESIS_CALL_STATE, make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def state_depths(state, s):
    """The sorted sample depths [B,R,S,1] (float64, CPU) the forward left in its state [B,R,35 S]."""
    return state[..., 32 * s: 33 * s].double().cpu()[..., None]


def forward_state(cs, dev, precision=None, c=None):
    """ops.raymarch with a state -> (planes on the device, state, the keyword arguments of the renderer's ops)."""
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    b, cfg = cs["b"], cs["cfg"]
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = dict(gen._render_args((cs["c"] if c is None else c).to(dev)), u_strat=u_s, u_imp=u_i)
    if precision is not None:
        args["decoder_precision"] = precision
    state = ops.raymarch_state(b, cfg.neural_rendering_resolution, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
    ops.raymarch(pl, state=state, **args)
    return pl, state, args


@functools.lru_cache(maxsize=None)
def device_case(dev, case, precision=None):
    """One forward + backward call and the float64 reference on the device's depths (computed once and left unchanged) ->
    dict(pl, state, args, g_hat [device], got, ref, mask)."""
    from hfa_gp_amd import ops
    cs = N.case(*case)
    cfg = cs["cfg"]
    pl, state, args = forward_state(cs, dev, precision)
    depths = state_depths(state, cfg.depth_resolution + cfg.depth_resolution_importance)
    _, _, g_hat, mask = G.masked_case(*case, depths=depths)
    g_dev = g_hat.float().to(dev)
    d_planes, dec = ops.raymarch_normals_bwd(g_dev, pl, state, decoder_grads=True, **args)
    ref = G.reference(cs["P"], cfg, cs["planes"], cs["c"], depths, g_hat)
    got = dict(planes=d_planes.permute(0, 1, 4, 2, 3), dec=dec)
    return dict(pl=pl, state=state, args=args, g_hat=g_dev, got=got, ref=ref, mask=mask, depths=depths)


def tolerance_factor(case):
    return max(1.0, 4.0 * G.oracle_rho(*case))


# ----------------------------------------------------------------------------- 6. the op against float64
@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_op_vs_float64_reference(dev, preset, axes, hw, box_warp):
    """16+16, 32+32, 48+48 samples; both axis conventions; planes that are not square either way; points outside the box; 100 rays
    per frame (the last 4-ray workgroup is partial), B = 2.  The default decoder precision (split 16-bit)."""
    case = (preset, axes, hw, box_warp)
    dc = device_case(dev, case)
    worst, _ = G.rho(dc["got"], dc["ref"], f"{N.CASE_IDS[N.CASES.index(case)]}: device")
    factor = tolerance_factor(case)
    print(f"tolerance factor {factor:.2f}, {int(dc['mask'].sum())} of {dc['mask'].numel()} rays kept")
    assert float(dc["ref"]["planes"].abs().max()) > 1e-3
    assert worst <= factor, f"worst err / bar {worst:.3f} > {factor:.2f}"


@pytest.mark.parametrize("preset,axes,hw,box_warp", [N.CASES[0], N.CASES[5], N.CASES[2]],
                         ids=[N.CASE_IDS[0], N.CASE_IDS[5], N.CASE_IDS[2]])
def test_op_fp32_decoder_vs_float64_reference(dev, preset, axes, hw, box_warp):
    """One case per sample count with decoder_precision='fp32' (the exact fp32 matrix instructions throughout)."""
    case = (preset, axes, hw, box_warp)
    dc = device_case(dev, case, "fp32")
    worst, _ = G.rho(dc["got"], dc["ref"], f"{N.CASE_IDS[N.CASES.index(case)]}: device, fp32 decoder")
    factor = tolerance_factor(case)
    print(f"tolerance factor {factor:.2f}")
    assert worst <= factor, f"worst err / bar {worst:.3f} > {factor:.2f}"


def test_op_without_decoder_gradients_gives_the_same_planes(dev):
    """The kernel without the parameter-gradient sums (generator frozen) against the one with them: the same arithmetic per texel,
    another atomic order."""
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[1])
    d_planes, dec = ops.raymarch_normals_bwd(dc["g_hat"], dc["pl"], dc["state"], **dc["args"])
    assert dec is None
    ratio = G.bar_ratio(d_planes.permute(0, 1, 4, 2, 3), dc["got"]["planes"])
    print(f"frozen against tuned kernel: worst err / bar {ratio:.3f}")
    assert ratio <= 1.0


# ----------------------------------------------------------------------------- 7. accumulation
def test_op_accumulates_into_every_plane(dev):
    """A pre-filled d_planes comes back as pre-fill + gradient (summed in fp32 in whatever order the atomics land: the bar with its
    atol scaled by the magnitude of what is summed); pre-filled decoder tensors likewise.  Square eg3d_original planes, where
    raymarch_bwd mirrors plane 1 into plane 2: here planes 1 and 2 each receive their own true-texel contribution."""
    from hfa_gp_amd import ops
    case = N.CASES[0]
    dc = device_case(dev, case)
    g = torch.Generator().manual_seed(21)
    pre = torch.randn(dc["pl"].shape, generator=g).to(dev)
    pre_dec = tuple(torch.randn(t.shape, generator=g).to(dev) for t in dc["got"]["dec"])
    acc = pre.clone()
    acc_dec = tuple(t.clone() for t in pre_dec)
    out, dec = ops.raymarch_normals_bwd(dc["g_hat"], dc["pl"], dc["state"], d_planes=acc, decoder_grads=True, dec_out=acc_dec,
                                        **dc["args"])
    assert out is acc and all(a is b for a, b in zip(dec, acc_dec))
    fresh = dc["got"]["planes"].permute(0, 1, 3, 4, 2)

    def summed(got, pre_t, fresh_t, what):
        err = (got - pre_t - fresh_t).abs()
        bound = 2e-5 * max(1.0, float(pre_t.abs().max() + fresh_t.abs().max())) + 1e-3 * fresh_t.abs()
        print(f"{what}: worst err / bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), what

    summed(out, pre, fresh, "d_planes")
    for got, p, f, k in zip(dec, pre_dec, dc["got"]["dec"], G.DEC_KEYS):
        summed(got, p, f, k)
    factor = tolerance_factor(case)
    ref = dc["ref"]["planes"]
    for pl in (1, 2):
        ratio = G.bar_ratio(dc["got"]["planes"][:, pl], ref[:, pl])
        print(f"plane {pl}: worst err / bar {ratio:.3f}, max |ref| {float(ref[:, pl].abs().max()):.3e}")
        assert float(ref[:, pl].abs().max()) > 1e-3 and ratio <= factor
    # (on these planes the true-texel gradient of plane 2 IS the mirror image of plane 1's — what raymarch_bwd exploits — so a
    # kernel that left plane 2 to a mirror pass would show as a plane 2 of zeros here, not as a wrong value)
    assert float((ref[:, 2] - ref[:, 1].transpose(-1, -2)).abs().max()) <= 1e-12
    assert float(dc["got"]["planes"][:, 2].abs().max()) > 0.5 * float(ref[:, 2].abs().max())


# ----------------------------------------------------------------------------- 8. zero upstream
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_zero_upstream_touches_nothing(dev, precision):
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[1], None if precision == "f16x3" else "fp32")
    g = torch.Generator().manual_seed(22)
    pre = torch.randn(dc["pl"].shape, generator=g).to(dev)
    pre[0, 0, 0, 0, :4] = -0.0
    pre_dec = tuple(torch.randn(t.shape, generator=g).to(dev) for t in dc["got"]["dec"])
    acc, acc_dec = pre.clone(), tuple(t.clone() for t in pre_dec)
    ops.raymarch_normals_bwd(torch.zeros_like(dc["g_hat"]), dc["pl"], dc["state"], d_planes=acc, decoder_grads=True, dec_out=acc_dec,
                             **dc["args"])
    assert torch.equal(acc.view(torch.int32), pre.view(torch.int32))
    for a, p in zip(acc_dec, pre_dec):
        assert torch.equal(a.view(torch.int32), p.view(torch.int32))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_camera_looking_away_gives_exact_zeros(dev, precision):
    from hfa_gp_amd import ops
    cs = N.case(*N.CASES[0])
    c = cs["c"].clone()
    m = c[:, :16].view(-1, 4, 4)
    m[:, :3, 0] *= -1                             # half a turn about the camera's up axis: every ray leaves the box behind
    m[:, :3, 2] *= -1
    pl, state, args = forward_state(cs, dev, precision, c=c)
    d_planes, dec = ops.raymarch_normals_bwd(G.upstream(cs).float().to(dev), pl, state, decoder_grads=True, **args)
    assert bool((d_planes == 0).all()) and all(bool((t == 0).all()) for t in dec)


def test_op_argument_checks(dev):
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[0])
    with pytest.raises(RuntimeError, match="raymarch_normals_bwd: state must be"):
        ops.raymarch_normals_bwd(dc["g_hat"], dc["pl"], None, **dc["args"])
    with pytest.raises(RuntimeError, match="g_normal must be"):
        ops.raymarch_normals_bwd(dc["g_hat"][:, :7].contiguous(), dc["pl"], dc["state"], **dc["args"])
    with pytest.raises(RuntimeError, match="d_planes must be shaped like planes"):
        ops.raymarch_normals_bwd(dc["g_hat"], dc["pl"], dc["state"], d_planes=dc["pl"][:, :2].contiguous(), **dc["args"])


# ----------------------------------------------------------------------------- 9 - 13. synthesis(normal_grad=True): tiny64, 10 x 10 rays
B = 2
TUNED_KEYS = G.DEC_KEYS + ("backbone.synthesis.b32.conv1.weight",)


def _cfg():
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS["tiny64"](), neural_rendering_resolution=10, img_resolution=40, conv_precision="fp32")


@functools.lru_cache(maxsize=None)
def _gen_cpu():
    from hfa_gp_amd.generator import TriPlaneGenerator
    return perturb_state(TriPlaneGenerator(_cfg(), seed=0)).requires_grad_(False)


def _gen(dev, tuned=False):
    if not tuned:
        return _gen_cpu().to(dev)
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = perturb_state(TriPlaneGenerator(_cfg(), seed=0)).requires_grad_(False).to(dev)
    for n, p in gen.named_parameters():
        if not n.startswith("backbone.mapping."):
            p.requires_grad_(True)
    return gen


def _inputs(dev):
    return tuple(t.to(dev) for t in make_inputs(_cfg(), B))


def _target(shape, seed, dev):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


def _normal_step(gen, dev):
    """A differentiable step with a loss on 'image_normal' alone: L = <image_normal, T * edge mask>, the mask taken from the depths
    the forward left in the tape's state -> (outputs, ws, depths, T * mask [B,R,3] float64 on the CPU)."""
    from hfa_gp_amd import ops
    cfg = _cfg()
    ws, c, us, ui = _inputs(dev)
    ws.requires_grad_(True)
    states, inner = [], ops.raymarch

    def recording(*a, **k):
        states.append(k.get("state"))
        return inner(*a, **k)

    ops.raymarch = recording
    try:
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, normal_grad=True, return_planes=True)
    finally:
        ops.raymarch = inner
    assert len(states) == 1 and states[0] is not None
    r = cfg.neural_rendering_resolution
    depths = state_depths(states[0], cfg.depth_resolution + cfg.depth_resolution_importance)
    mask = G.edge_mask(cfg, (cfg.plane_resolution, cfg.plane_resolution), make_inputs(cfg, B)[1], depths)
    assert float(mask.double().mean()) >= G.MIN_KEPT
    g_hat = torch.randn(B, r * r, 3, generator=torch.Generator().manual_seed(23), dtype=torch.float64) * mask[..., None]
    t_img = g_hat.float().reshape(B, r, r, 3).permute(0, 3, 1, 2).to(dev)
    (out["image_normal"] * t_img).sum().backward()
    return out, ws, depths, g_hat


def _float64_chain(depths, g_hat, keys=()):
    """The oracle's backbone in float64 autograd feeding normal_grad_ref.reference on the device's depths ->
    (d ws, {key: gradient} of the decoder tensors and backbone parameters asked for, rho of the fp32 reference on this set-up)."""
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in state_cpu(_gen_cpu()).items()}
    ws, c, _, _ = make_inputs(cfg, B)
    ws = ws.double().requires_grad_(True)
    bb = [k for k in keys if k not in G.DEC_KEYS]
    for k in bb:
        P[k].requires_grad_(True)
    planes = O.backbone_synthesis(P, cfg, ws).reshape(B, 3, 32, cfg.plane_resolution, cfg.plane_resolution)
    ref = G.reference(P, cfg, planes, c, depths, g_hat)
    grads = torch.autograd.grad((planes * ref["planes"]).sum(), [ws] + [P[k] for k in bb])
    out = dict(zip(G.DEC_KEYS, ref["dec"]))
    out.update(zip(bb, grads[1:]))
    low = G.reference(P, cfg, planes, c, depths, g_hat, dtype=torch.float32)
    return grads[0], out, G.rho(low, ref, "tiny64 generator: fp32 reference")[0]


def _within(got, ref, factor, what):
    ratio = G.bar_ratio(got, ref)
    print(f"{what}: worst err / bar {ratio:.3f} (allowed {factor:.2f}), max |ref| {float(ref.abs().max()):.3e}")
    assert float(ref.abs().max()) > 0 and ratio <= factor, what


def test_synthesis_normal_grad_d_ws_vs_float64(dev):
    gen = _gen(dev)
    out, ws, depths, g_hat = _normal_step(gen, dev)
    assert set(out) == {"image", "image_raw", "image_depth", "image_normal", "planes", "feature_image"}
    assert out["image_normal"].requires_grad and out["image"].requires_grad and not out["image_depth"].requires_grad
    ws2, c, us, ui = _inputs(dev)
    with torch.no_grad():
        plain = gen.synthesis(ws2, c, noise_mode="const", u_strat=us, u_imp=ui, normals=True)
    assert not plain["image_normal"].requires_grad
    assert torch.equal(out["image_normal"].detach(), plain["image_normal"])
    for k in ("image", "image_raw", "image_depth"):
        assert torch.equal(out[k].detach(), plain[k]), k
    d_ws, _, rho = _float64_chain(depths, g_hat)
    _within(ws.grad, d_ws, max(1.0, 4.0 * rho), "d ws of a normals-only loss")


def test_synthesis_normal_grad_tuned_generator(dev):
    """With the generator tuned: the decoder parameters' .grad and one backbone conv's .grad against the float64 chain."""
    gen = _gen(dev, tuned=True)
    _, ws, depths, g_hat = _normal_step(gen, dev)
    d_ws, ref, rho = _float64_chain(depths, g_hat, TUNED_KEYS)
    factor = max(1.0, 4.0 * rho)
    _within(ws.grad, d_ws, factor, "d ws (tuned)")
    prm = dict(gen.named_parameters())
    for k in TUNED_KEYS:
        assert prm[k].grad is not None, k
        _within(prm[k].grad, ref[k], factor, k)


def test_synthesis_normal_grad_composes(dev):
    """d ws of loss_img + loss_depth + loss_mask + loss_normal + a query term = the sum of the separately computed ones."""
    gen, cfg = _gen(dev), _cfg()
    r = cfg.neural_rendering_resolution
    coords = (torch.rand(B, 21, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(dev)
    t_img = _target((B, 3, cfg.img_resolution, cfg.img_resolution), 6, dev) / cfg.img_resolution
    t_geo, t_nrm, t_q = _target((B, 1, r, r), 7, dev) / r, _target((B, 3, r, r), 8, dev) / r, _target((B, 21, 1), 9, dev) / 8

    def step(image, normal, **kw):
        ws, c, us, ui = _inputs(dev)
        ws.requires_grad_(True)
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, geometry=True, query=coords, **kw)
        loss = 0
        if image:
            loss = (out["image"] * t_img).sum() + (out["image_depth"] * t_geo).sum() + (out["image_mask"] * t_geo).sum() + \
                (out["query_sigma"] * t_q).sum()
        if normal:
            loss = loss + (out["image_normal"] * t_nrm).sum()
        loss.backward()
        return out, ws.grad

    out, both = step(True, True, normal_grad=True)
    assert set(out) == {"image", "image_raw", "image_depth", "image_mask", "query_sigma", "query_rgb", "image_normal"}
    assert all(out[k].requires_grad for k in ("image", "image_depth", "image_mask", "query_sigma", "image_normal"))
    _, image_only = step(True, False)
    _, normal_only = step(False, True, normal_grad=True)
    assert float(normal_only.abs().max()) > 0 and float(image_only.abs().max()) > 0
    _within(both, image_only + normal_only, 1.0, "d ws of the joint loss against the sum of its parts")


# ----------------------------------------------------------------------------- 11. unchanged paths
def test_new_op_is_not_called_unless_the_loss_uses_the_normals(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    calls, inner = [], ops.raymarch_normals_bwd
    monkeypatch.setattr(ops, "raymarch_normals_bwd", lambda *a, **k: calls.append(1) or inner(*a, **k))
    t_img = _target((B, 3, cfg.img_resolution, cfg.img_resolution), 6, dev)

    def step(use_normal, **kw):
        ws, c, us, ui = _inputs(dev)
        ws.requires_grad_(True)
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, **kw)
        loss = (out["image"] * t_img).sum()
        if use_normal:
            loss = loss + out["image_normal"].sum()
        loss.backward()
        return out, ws.grad

    out, _ = step(False, normals=True)
    assert not out["image_normal"].requires_grad and out["image_normal"].grad_fn is None and calls == []
    out, d_ignored = step(False, normal_grad=True)          # a loss that ignores image_normal
    assert out["image_normal"].requires_grad and calls == []
    _, d_plain = step(False)
    _within(d_ignored, d_plain, 1.0, "d ws with image_normal ignored against the plain step")
    step(True, normal_grad=True)
    assert calls == [1]


# ----------------------------------------------------------------------------- 12. refusals
def test_refusals(dev, monkeypatch):
    from hfa_gp_amd import generator as Gn
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    with torch.no_grad():
        before = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)

    def boom(*a, **k):
        raise AssertionError("launched before the refusal")

    monkeypatch.setattr(ops, "raymarch", boom)
    with pytest.raises(NotImplementedError, match="camera gradient of the normal term"):
        gen.synthesis(ws.clone().requires_grad_(True), c.clone().requires_grad_(True), noise_mode="const", u_strat=us, u_imp=ui,
                      normal_grad=True)
    frame = cfg.neural_rendering_resolution ** 2 * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    monkeypatch.setattr(Gn, "RAY_STATE_CAP_BYTES", frame)
    with pytest.raises(RuntimeError, match=rf"RAY_STATE_CAP_BYTES = {frame}; 1 frames fit"):
        gen.synthesis(ws.clone().requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui, normal_grad=True)
    assert not SYNTHESIS_CALL_STATE & set(vars(gen))          # (the request lives in the call's record, not on the module)
    monkeypatch.undo()
    with torch.no_grad():
        plain = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
    assert list(plain) == ["image", "image_raw", "image_depth"]
    for k in plain:
        assert torch.equal(plain[k], before[k]), k
    monkeypatch.setattr(Gn, "RAY_STATE_CAP_BYTES", frame)
    with torch.no_grad():                                     # without grad it is `normals=True`: rendered in frame chunks
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, normal_grad=True)
    assert not out["image_normal"].requires_grad and out["image_normal"].shape[0] == B


# ----------------------------------------------------------------------------- 13. pass-through and edges
def test_empty_batch_has_the_key_with_its_edge(dev):
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    ws.requires_grad_(True)
    out = gen.synthesis(ws[:0], c[:0], noise_mode="const", normal_grad=True, geometry=True)
    r = cfg.neural_rendering_resolution
    assert out["image_normal"].shape == (0, 3, r, r) and out["image_mask"].shape == (0, 1, r, r)
    assert out["image_normal"].requires_grad
    out["image_normal"].sum().backward()
    assert ws.grad is not None and bool((ws.grad == 0).all())


def test_get_image_passes_normal_grad_through(dev):
    from hfa_gp_amd import headnerf

    class A:
        out_pose = False; person_2 = False; params_len = 76; generator_preset = "tiny14"; generator_seed = 0

    torch.manual_seed(0)
    m = headnerf.HeadNeRF_3DMM(A(), 64, dev, 512, 50).to(dev)
    cfg = m.generator.cfg
    _, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    data = c.clone()
    data[:, FLIP_COLUMNS] *= -1                    # the label as the data set yields it: get_image flips it in place
    ws = m.get_latent(torch.randn(2, 50, device=dev))
    assert ws.requires_grad
    label = data.clone()
    out = m.get_image(ws, label, normal_grad=True, u_strat=us, u_imp=ui)
    assert torch.equal(label, c), "the label flip side effect is gone"
    assert isinstance(out, dict) and set(out) == {"image", "image_raw", "image_depth", "image_normal"}
    assert out["image_normal"].requires_grad
    with torch.no_grad():
        want = m.get_image(ws, data.clone(), normals=True, u_strat=us, u_imp=ui)
    assert torch.equal(out["image_normal"].detach(), want["image_normal"])
    d_latent, = torch.autograd.grad(out["image_normal"].square().sum(), ws)
    assert float(d_latent.abs().max()) > 0 and bool(torch.isfinite(d_latent).all())
    fwd = m(torch.randn(2, 76, device=dev), data.clone(), normal_grad=True, geometry=True)
    assert isinstance(fwd, dict) and fwd["image_normal"].requires_grad and fwd["image_mask"].requires_grad
