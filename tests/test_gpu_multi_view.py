"""Multi-view synthesis: `synthesis(ws [B,14,512], c [B,V,25])` renders V cameras of every latent on one backbone pass.  The view-sum
kernel (hfagp_planes_sum_to_nhwc) to the bit; the multi-view call against the single-view path (bits) and against the oracle on the
flattened call `O.synthesis(ws.repeat_interleave(V, 0), c.flatten(0, 1))` (forward, d ws, generator parameters, d c); the trainer step.
Needs an MI355X:  python -m pytest tests -m gpu"""
import dataclasses
import functools

import pytest
import torch

from tests import resample_ref
from tests.test_gpu_parity import E2E_ATOL, close
from tests.util import look_at_label, make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _cfg(preset="tiny64", prec="fp32"):
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS[preset](), conv_precision=prec)


@functools.lru_cache(maxsize=None)
def _gen_and_state(preset="tiny64", prec="fp32"):
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = perturb_state(TriPlaneGenerator(_cfg(preset, prec), seed=0)).requires_grad_(False)
    return gen, state_cpu(gen)


def _device_gen(dev, preset="tiny64", prec="fp32", tuned=False):
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = perturb_state(TriPlaneGenerator(_cfg(preset, prec), seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for n, p in gen.named_parameters():
            if not n.startswith("backbone.mapping."):
                p.requires_grad_(True)
    return gen


def mv_inputs(cfg, b, v, n=None, seed=10):
    """ws [B,14,512] of make_inputs(cfg, B); c [B,V,25], u_strat [B·V,r,Sc,1], u_imp [B·V·r,Sf] of make_inputs(cfg, B·V) at n x n rays:
    frame f = b·V + v."""
    ws = make_inputs(cfg, b, seed)[0]
    _, c, us, ui = resample_ref.inputs(cfg, b * v, cfg.neural_rendering_resolution if n is None else n, seed + 1)
    return ws, c.reshape(b, v, 25), us, ui


def _timed(gen, fn):
    gen.timing = {}
    try:
        out = fn()
        return out, {k: len(t) for k, t in gen.timing.items()}
    finally:
        gen.timing = None


# ----------------------------------------------------------------------------- the kernel
def test_planes_sum_to_nhwc_is_the_ordered_sum(dev):
    """[2,3,3,5,7,32]: 1680 float4 outputs, the last block of 256 is partial.  The running sum in the order v = 0, 1, 2, to the bit."""
    from hfa_gp_amd import ops
    pm = torch.randn(2, 3, 3, 5, 7, 32, generator=torch.Generator().manual_seed(1)).to(dev)
    got = ops.planes_sum_to_nhwc(pm)
    assert got.shape == (2, 5, 7, 96)
    assert torch.equal(got, ops.planes_to_nhwc(((pm[:, 0] + pm[:, 1]) + pm[:, 2]).contiguous()))
    one = pm[:, :1].contiguous()
    assert torch.equal(ops.planes_sum_to_nhwc(one), ops.planes_to_nhwc(one[:, 0].contiguous()))
    assert torch.equal(ops.planes_sum_to_nhwc(pm), got), "two calls, the same bits"


def test_planes_sum_to_nhwc_argument_codes(dev):
    from hfa_gp_amd import _lib
    h = _lib.lib()
    assert h.hfagp_planes_sum_to_nhwc(None, None, 1, 1, 8, 8, 32, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    assert h.hfagp_planes_sum_to_nhwc(1, None, 1, 1, 8, 8, 32, None) == -1
    assert h.hfagp_planes_sum_to_nhwc(1, 1, 1, 0, 8, 8, 32, None) == -1          # (non-null, never dereferenced: V = 0 is rejected first)
    assert h.hfagp_planes_sum_to_nhwc(1, 1, 0, 1, 8, 8, 32, None) == -1
    assert h.hfagp_planes_sum_to_nhwc(1, 1, 1, 1, 8, 8, 6, None) == -2           # Cp % 4 != 0
    assert b"Cp=6" in h.hfagp_last_error()


# ----------------------------------------------------------------------------- against the single-view path, bits
def test_one_view_is_the_single_view_call(dev):
    cfg = _cfg()
    gen = _device_gen(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui, geometry=True, normals=True, return_planes=True)
    single, ran_single = _timed(gen, lambda: gen.synthesis(ws, c, **kw))
    multi, ran_multi = _timed(gen, lambda: gen.synthesis(ws, c[:, None], **kw))
    assert set(multi) == set(single) == {"image", "image_raw", "image_depth", "image_mask", "image_normal", "planes", "feature_image"}
    for k in single:
        got = multi[k] if k == "planes" else multi[k][:, 0]
        assert multi[k].shape == (single[k].shape if k == "planes" else (2, 1) + single[k].shape[1:]), k
        assert torch.equal(got, single[k]), k
    assert ran_multi == ran_single and ran_single, (ran_multi, ran_single)


def test_planes_once_and_per_view_bits(dev):
    cfg = _cfg()
    gen = _device_gen(dev)
    b, v, r = 2, 3, cfg.neural_rendering_resolution
    ws, c, us, ui = (t.to(dev) for t in mv_inputs(cfg, b, v))
    kw = dict(noise_mode="const", geometry=True, normals=True, return_planes=True)
    multi, ran_multi = _timed(gen, lambda: gen.synthesis(ws, c, u_strat=us, u_imp=ui, **kw))
    assert multi["image"].shape == (b, v, 3, cfg.img_resolution, cfg.img_resolution)
    assert multi["image_raw"].shape == multi["image_normal"].shape == (b, v, 3, r, r)
    assert multi["image_depth"].shape == multi["image_mask"].shape == (b, v, 1, r, r)
    assert multi["feature_image"].shape == (b, v, r, r, 32)
    assert multi["planes"].shape[0] == b
    us_v, ui_v = us.view(b, v, *us.shape[1:]), ui.view(b, v, r * r, -1)
    for i in range(v):
        one, ran_one = _timed(gen, lambda: gen.synthesis(ws, c[:, i].contiguous(), u_strat=us_v[:, i].contiguous(),
                                                         u_imp=ui_v[:, i].reshape(b * r * r, -1), **kw))
        assert torch.equal(multi["planes"], one["planes"])
        for k in ("image_raw", "image_mask", "image_normal"):
            assert torch.equal(multi[k][:, i], one[k]), (k, i)
        assert torch.equal(multi["feature_image"][:, i], one["feature_image"])
        # the backbone convs (and every other timed launch) run as often as in a B = 2 call
        assert ran_multi == ran_one, (ran_multi, ran_one)
    assert any(k.startswith("modconv") for k in ran_multi)


# ----------------------------------------------------------------------------- against the oracle
CASES = {"tiny64": ("tiny64", "fp32", 2, 3, None), "small128": ("small128", "f16x3", 1, 2, 16)}      # preset, prec, B, V, N (None: r0)


@functools.lru_cache(maxsize=None)
def reference(case):
    """One oracle pass per case on the flattened call, shared by the forward and the backward test: the outputs reshaped to the view
    axis and d ws of L = <image, G> + <image_raw, G_raw> (the oracle's autograd sums over the repeated rows)."""
    from oracle import eg3d_oracle as O
    preset, prec, b, v, n = CASES[case]
    cfg = _cfg(preset, prec)
    _, P = _gen_and_state(preset, prec)
    ws, c, us, ui = mv_inputs(cfg, b, v, n)
    r = cfg.neural_rendering_resolution if n is None else n
    g = torch.Generator().manual_seed(6)
    G = torch.randn(b, v, 3, cfg.img_resolution, cfg.img_resolution, generator=g) / cfg.img_resolution
    G_raw = torch.randn(b, v, 3, r, r, generator=g) / 64
    ws_ref = ws.clone().requires_grad_(True)
    ws_rep, c_flat = ws_ref.repeat_interleave(v, 0), c.flatten(0, 1)
    if n is None:
        ref = O.synthesis(P, cfg, ws_rep, c_flat, us, ui)
    else:       # (the oracle has no resample: composed from its functions, as tests/test_gpu_resample.py does)
        ref = resample_ref.synthesis(P, cfg, ws_rep, c_flat, us, ui, n)
    ref = {k: ref[k].unflatten(0, (b, v)) for k in ("image", "image_raw", "image_depth")}
    ((ref["image"] * G).sum() + (ref["image_raw"] * G_raw).sum()).backward()
    return dict(cfg=cfg, inputs=(ws, c, us, ui), n=n, G=G, G_raw=G_raw, out={k: t.detach() for k, t in ref.items()}, d_ws=ws_ref.grad)


@pytest.mark.parametrize("case", list(CASES))
def test_forward_vs_oracle(dev, case):
    ref = reference(case)
    preset, prec, b, v, n = CASES[case]
    gen = _device_gen(dev, preset, prec)
    ws, c, us, ui = (t.to(dev) for t in ref["inputs"])
    with torch.no_grad():
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=n)
    for k in ("image", "image_raw", "image_depth"):
        print(f"{case} {k}: max err {(out[k].cpu() - ref['out'][k]).abs().max().item():.3e} (bar {E2E_ATOL[prec]:.0e})")
    for k in ("image_raw", "image_depth", "image"):           # (image_depth: the clamp range is global over the B·V frames)
        close(out[k], ref["out"][k], atol=E2E_ATOL[prec])


@pytest.mark.parametrize("case", list(CASES))
def test_backward_vs_oracle(dev, case):
    ref = reference(case)
    preset, prec, b, v, n = CASES[case]
    k = {"fp32": 1.0, "f16x3": 5.0}[prec]
    gen = _device_gen(dev, preset, prec)
    ws, c, us, ui = (t.to(dev) for t in ref["inputs"])
    ws.requires_grad_(True)
    out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=n)
    ((out["image"] * ref["G"].to(dev)).sum() + (out["image_raw"] * ref["G_raw"].to(dev)).sum()).backward()
    scale = ref["d_ws"].abs().max().item()
    err = (ws.grad.cpu() - ref["d_ws"]).abs().max().item()
    print(f"{case} d ws: max err {err:.3e}, scale {scale:.3e}, err / scale {err / scale:.3e}")
    assert ws.grad.shape == (b, ref["cfg"].num_ws, 512)
    close(ws.grad, ref["d_ws"], atol=2e-4 * k * scale, rtol=2e-3 * k)


def test_generator_parameter_gradients_vs_oracle(dev):
    """tiny64, fp32, B = 1, V = 2, generator tuned: every generator-parameter gradient and d ws at the bars of
    test_generator_parameter_gradients_vs_oracle_autograd (noise strengths against their cancellation scale)."""
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    b, v, k = 1, 2, 1.0
    gen, _ = _gen_and_state()
    P = {n: t.detach().clone() for n, t in gen.state_dict().items()}
    names = [n for n, _ in gen.named_parameters() if not n.startswith("backbone.mapping.")]
    for n in names:
        P[n].requires_grad_(True)
    ws, c, us, ui = mv_inputs(cfg, b, v)
    G = torch.randn(b, v, 3, cfg.img_resolution, cfg.img_resolution, generator=torch.Generator().manual_seed(8)) / cfg.img_resolution
    ws_ref = ws.clone().requires_grad_(True)
    (O.synthesis(P, cfg, ws_ref.repeat_interleave(v, 0), c.flatten(0, 1), us, ui)["image"] * G.flatten(0, 1)).sum().backward()
    P2 = {n: t.detach().clone() for n, t in P.items()}
    spread = {}
    for n in names:
        if n.endswith(".noise_strength"):
            spread[n] = torch.full_like(P2[n[:-len("noise_strength")] + "noise_const"], float(P2[n])).requires_grad_(True)
            P2[n] = spread[n]
    (O.synthesis(P2, cfg, ws.repeat_interleave(v, 0), c.flatten(0, 1), us, ui)["image"] * G.flatten(0, 1)).sum().backward()
    cancel = {n: float(t.grad.abs().sum()) for n, t in spread.items() if t.grad is not None}
    dgen = _device_gen(dev, tuned=True)
    ws_d = ws.to(dev).requires_grad_(True)
    out = dgen.synthesis(ws_d, c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev))
    (out["image"] * G.to(dev)).sum().backward()
    close(ws_d.grad, ws_ref.grad, atol=2e-4 * k * ws_ref.grad.abs().max().item(), rtol=2e-3 * k)
    params = dict(dgen.named_parameters())
    bad = []
    for n in names:
        ref, got = P[n].grad, params[n].grad
        if ref is None:
            assert got is None or float(got.abs().max()) == 0.0, n
            continue
        assert got is not None, n
        scale, tol = max(ref.abs().max().item(), 1e-12), 5e-4 * k
        if n in cancel:
            scale, tol = max(cancel[n], 1e-12), 1e-4 * k
        err = (got.cpu() - ref).abs().max().item()
        if not err <= tol * scale + 1e-7:
            bad.append((n, err, scale))
    assert not bad, bad[:8]


def test_geometry_and_camera_gradients_vs_oracle(dev):
    """tiny64, fp32, B = 2, V = 2, geometry=True, ws and c [B,V,25] both leaves: L = <image, G> + <image_raw, G_raw> + <image_mask, M> +
    <image_depth, K>.  d ws at tests/test_gpu_geometry_grad.py::close_grad's bar; c.grad [B,V,25] against the oracle's autograd
    w.r.t. the flattened labels at the bar of test_gpu_camera_grad's end-to-end case (2e-4 of its scale, 2e-3 relative)."""
    from tests.test_gpu_camera_grad import ZERO_COLUMNS
    from tests.test_gpu_geometry_grad import MIN_OPACITY, _oracle_synthesis_geom, close_grad
    cfg = _cfg()
    b, v, r = 2, 2, cfg.neural_rendering_resolution
    _, P = _gen_and_state()
    ws, c, us, ui = mv_inputs(cfg, b, v)
    g = torch.Generator().manual_seed(7)
    G = torch.randn(b, v, 3, cfg.img_resolution, cfg.img_resolution, generator=g) / cfg.img_resolution
    G_raw = torch.randn(b, v, 3, r, r, generator=g) / 64
    M, K = torch.randn(b, v, 1, r, r, generator=g) / (r * r), torch.randn(b, v, 1, r, r, generator=g) / (r * r)

    def loss_of(out, dv="cpu"):
        return sum((out[k].reshape(b, v, *t.shape[2:]) * t.to(dv)).sum()
                   for k, t in (("image", G), ("image_raw", G_raw), ("image_mask", M), ("image_depth", K)))

    ws_ref, c_ref = ws.clone().requires_grad_(True), c.clone().requires_grad_(True)
    ref = _oracle_synthesis_geom(P, cfg, ws_ref.repeat_interleave(v, 0), c_ref.flatten(0, 1), us, ui)
    assert float(ref["image_mask"].detach().min()) >= MIN_OPACITY, "pick other inputs: the depth term carries 1 / opacity"
    loss_of(ref).backward()
    gen = _device_gen(dev)
    ws_d, c_d = ws.to(dev).requires_grad_(True), c.to(dev).requires_grad_(True)
    out = gen.synthesis(ws_d, c_d, noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True)
    assert out["image_mask"].shape == (b, v, 1, r, r) and out["image_mask"].requires_grad and out["image_depth"].requires_grad
    loss_of(out, dev).backward()
    assert c_d.grad is not None and c_d.grad.shape == (b, v, 25) and c_d.grad.dtype == c_d.dtype
    close_grad(ws_d.grad, ws_ref.grad, "d ws")
    scale = c_ref.grad.abs().max().item()
    err = (c_d.grad.cpu() - c_ref.grad).abs()
    print(f"d c: max err {err.max().item():.3e}, scale {scale:.3e}, err / scale {err.max().item() / scale:.3e}")
    assert bool((c_d.grad[..., ZERO_COLUMNS] == 0).all())
    close(c_d.grad, c_ref.grad, atol=2e-4 * scale, rtol=2e-3)


def test_query_and_normal_terms_compose(dev):
    """`query=` points belong to the identity: [B,M,·], evaluated once — the bits of `sample_mixed` — and their plane gradient joins
    the identity's, next to a differentiable 'image_normal' per view.  d ws of image + normal + query terms is the sum of d ws of the
    multi-view call without the points and d ws of the points alone (`sample_mixed(differentiable=True)`): the same terms in another
    order, held to the d ws bar of the oracle tests (2e-4 of the scale, 2e-3 relative)."""
    cfg = _cfg()
    gen = _device_gen(dev)
    b, v, m, r = 2, 2, 37, cfg.neural_rendering_resolution
    ws, c, us, ui = (t.to(dev) for t in mv_inputs(cfg, b, v))
    g = torch.Generator().manual_seed(9)
    pts = ((torch.rand(b, m, 3, generator=g) - 0.5) * 0.8 * cfg.box_warp).to(dev)
    qs, qr = torch.randn(b, m, 1, generator=g).to(dev), torch.randn(b, m, 32, generator=g).to(dev)
    nrm = torch.randn(b, v, 3, r, r, generator=g).to(dev)

    def image_terms(out):
        return out["image"].square().mean() + (out["image_normal"] * nrm).mean()

    def query_terms(sigma, rgb):
        return (sigma * qs).mean() + (rgb * qr).mean()

    kw = dict(noise_mode="const", u_strat=us, u_imp=ui, normal_grad=True)
    w_all, w_img, w_pts = (ws.clone().requires_grad_(True) for _ in range(3))
    out = gen.synthesis(w_all, c, query=pts, **kw)
    assert out["query_sigma"].shape == (b, m, 1) and out["query_rgb"].shape == (b, m, 32)
    assert out["image_normal"].shape == (b, v, 3, r, r) and out["image_normal"].requires_grad
    (image_terms(out) + query_terms(out["query_sigma"], out["query_rgb"])).backward()
    image_terms(gen.synthesis(w_img, c, **kw)).backward()
    alone = gen.sample_mixed(pts, None, w_pts, differentiable=True)
    assert torch.equal(out["query_sigma"], alone["sigma"]) and torch.equal(out["query_rgb"], alone["rgb"])
    query_terms(alone["sigma"], alone["rgb"]).backward()
    want = (w_img.grad + w_pts.grad).cpu()
    assert float(w_pts.grad.abs().max()) > 1e-3 * float(want.abs().max()), "the point term must matter in the sum"
    err = (w_all.grad.cpu() - want).abs().max().item()
    print(f"d ws with points: max err {err:.3e}, scale {want.abs().max().item():.3e}, points alone {w_pts.grad.abs().max().item():.3e}")
    close(w_all.grad, want, atol=2e-4 * want.abs().max().item(), rtol=2e-3)


# ----------------------------------------------------------------------------- determinism
def test_two_calls_give_the_same_ws_grad(dev, monkeypatch):
    """Pass 2 of ops.raymarch_bwd sums in the arrival order of an atomic cursor; everything else of the backward — the early flush of
    the SR styles, the view sums — is deterministic: with the first step's ray-march adjoint replayed (tests/test_gpu_resample.py), the
    second step must hand it the same bits and arrive at the same d ws."""
    from hfa_gp_amd import ops
    from tests.test_gpu_resample import _replay_raymarch_bwd
    cfg = _cfg()
    gen = _device_gen(dev)
    ws, c, us, ui = (t.to(dev) for t in mv_inputs(cfg, 2, 2))
    first = _replay_raymarch_bwd(monkeypatch, ops)
    grads = []
    for _ in range(2):
        w = ws.clone().requires_grad_(True)
        out = gen.synthesis(w, c, noise_mode="const", u_strat=us, u_imp=ui, geometry=True)
        (out["image"].square().mean() + out["image_raw"].mean() + out["image_mask"].mean()).backward()
        grads.append(w.grad)
    assert first["result"].shape[0] == 4, "the ray-march adjoint runs at B·V frames"
    assert torch.equal(grads[0], grads[1]) and bool(grads[0].abs().max() > 0)


# ----------------------------------------------------------------------------- errors and empties
def test_errors_and_empty_views(dev):
    cfg = _cfg()
    gen = _device_gen(dev)
    b, v, r, s = 2, 2, cfg.neural_rendering_resolution, cfg.img_resolution
    ws, c, us, ui = (t.to(dev) for t in mv_inputs(cfg, b, v))
    gen.timing = {}
    try:
        with pytest.raises(ValueError):
            gen.synthesis(ws, c[:, :, None])                                  # 4-D label
        with pytest.raises(ValueError):
            gen.synthesis(ws, torch.cat((c, c[:1])))                          # [B+1, V, 25]
        with pytest.raises(ValueError):
            gen.synthesis(ws, c[..., :24])
        with pytest.raises(ValueError):
            gen.synthesis(ws, c, u_strat=us[:b])                              # sized for B frames, not B·V
        with pytest.raises(ValueError):
            gen.synthesis(ws, c, u_imp=ui[:b * r * r])
        w = ws.clone().requires_grad_(True)
        out = gen.synthesis(w, c[:, :0], geometry=True, normals=True)
        assert out["image"].shape == (b, 0, 3, s, s) and out["image_raw"].shape == out["image_normal"].shape == (b, 0, 3, r, r)
        assert out["image_depth"].shape == out["image_mask"].shape == (b, 0, 1, r, r)
        assert out["image"].requires_grad, "the autograd edges are kept"
        out["image"].sum().backward()
        assert w.grad is not None and not bool(w.grad.any())
        none = gen.synthesis(ws[:0], c[:0])
        assert none["image"].shape == (0, v, 3, s, s)
        assert gen.timing == {}, "nothing may be launched"
    finally:
        gen.timing = None


# ----------------------------------------------------------------------------- the trainer step
def _trainer(device, oracle, tuned=False):
    from hfa_gp_amd import headnerf
    from hfa_gp_amd.trainer import Trainer
    from tests.test_trainer_cpu import Args, OracleGenerator

    class MultiViewOracle(OracleGenerator):
        """The CPU oracle behind `synthesis` with a 3-D label flattened: the B·V frames rendered with repeated latents."""

        def synthesis(self, ws, c=None, noise_mode="const", u_strat=None, u_imp=None, **kw):
            if c.dim() != 3:
                return super().synthesis(ws, c, noise_mode, u_strat, u_imp)
            b, v = c.shape[:2]
            out = super().synthesis(ws.repeat_interleave(v, 0), c.flatten(0, 1), noise_mode, u_strat, u_imp)
            return {k: t.unflatten(0, (b, v)) for k, t in out.items() if k in ("image", "image_raw", "image_depth")}

    torch.manual_seed(0)
    gen = headnerf.HeadNeRF_3DMM(Args(), Args.size, device, 512, Args.latent_dim_shape)
    if oracle:
        MultiViewOracle.adopt(gen.generator)
    tr = Trainer(Args(), device, mode="3dmm", gen=gen, lpips="none")
    if tuned:
        tr.tune_generator()
    tr.optimizer = torch.optim.SGD(tr.gen.parameters(), lr=0.0)     # compare gradients, not Adam's first step
    return tr


def _rig_frames():
    g = torch.Generator().manual_seed(2)
    real = (0.5 * torch.randn(2, 2, 3, 32, 32, generator=g)).clamp(-1, 1)
    params = torch.randn(2, 76, generator=g)
    label = look_at_label(torch.tensor([1.5, 1.7, 1.4, 1.6]), torch.tensor([1.6, 1.5, 1.55, 1.65]), flipped=False).reshape(2, 2, 25)
    return real, label, params


def _oracle_uniforms(cfg, frames, dev):
    """What OracleGenerator draws (seed 0): one frame's uniforms, the same for every frame."""
    g = torch.Generator().manual_seed(0)
    r = cfg.neural_rendering_resolution ** 2
    us = torch.rand(1, r, cfg.depth_resolution, 1, generator=g).expand(frames, -1, -1, -1).contiguous().to(dev)
    ui = torch.rand(r, cfg.depth_resolution_importance, generator=g).repeat(frames, 1).to(dev)
    return us, ui


def test_trainer_multi_view_step_matches_oracle_step(dev):
    """One `gen_update` (3DMM-driven, L2 only, tiny14) with real [2,2,3,s,s] and label [2,2,25] on the MI355X against the CPU step that
    renders the four frames with repeated latents: loss, d bases, d delta at test_trainer_step_on_gpu_matches_oracle_step's bars."""
    from tests.test_gpu_backward import close as close_b
    real, label, params = _rig_frames()
    cpu = _trainer("cpu", True)
    _, l2_cpu, _, img_cpu = cpu.gen_update(real, label.clone(), params)
    assert img_cpu.shape == (2, 2, 3, 32, 32)
    gpu = _trainer(dev, False)
    us, ui = _oracle_uniforms(gpu.gen.generator.cfg, 4, dev)
    lab = label.clone().to(dev)
    _, l2_gpu, _, img = gpu.gen_update(real.to(dev), lab, params.to(dev), u_strat=us, u_imp=ui)
    assert img.shape == (2, 2, 3, 32, 32)
    assert torch.equal(lab.cpu()[..., [1, 2, 5, 6, 9, 10]], -label[..., [1, 2, 5, 6, 9, 10]]), "the label flip side effect"
    print(f"l2 gpu {float(l2_gpu):.6e} cpu {float(l2_cpu):.6e}")
    assert abs(float(l2_gpu) - float(l2_cpu)) < 1e-5
    for name in ("bases", "delta"):
        a, bref = getattr(gpu.gen, name).grad, getattr(cpu.gen, name).grad
        close_b(a, bref, atol=2e-4 * bref.abs().max().item(), rtol=2e-3)


def test_trainer_multi_view_tuned_step_releases_every_parameter_once(dev):
    """The same step with tune_generator(): it completes inside the trainer's step scope, and every generator parameter carries ONE
    gradient — that of the step over the four flattened frames with repeated driver inputs.  The two are the same sums in another
    order (fp32, ~1e-6 relative to the sum of magnitudes; a noise strength cancels to ~1e-3 of that): held to 1e-3 of the tensor's
    scale + 1e-2 relative, against which a parameter handed to the sink twice, at twice the gradient, is off by 100 %."""
    from tests.test_gpu_backward import close as close_b
    real, label, params = _rig_frames()
    mv = _trainer(dev, False, tuned=True)
    us, ui = _oracle_uniforms(mv.gen.generator.cfg, 4, dev)
    mv.gen_update(real.to(dev), label.clone().to(dev), params.to(dev), u_strat=us, u_imp=ui)
    flat = _trainer(dev, False, tuned=True)
    flat.gen_update(real.flatten(0, 1).to(dev), label.clone().flatten(0, 1).to(dev), params.repeat_interleave(2, 0).to(dev),
                    u_strat=us, u_imp=ui)
    seen = 0
    for (n, p), (_, q) in zip(mv.gen.generator.named_parameters(), flat.gen.generator.named_parameters()):
        if n.startswith("backbone.mapping."):
            continue
        assert (p.grad is None) == (q.grad is None), n
        if p.grad is None:
            continue
        assert torch.isfinite(p.grad).all(), n
        scale = q.grad.abs().max().item()
        if scale > 0:
            seen += 1
            close_b(p.grad, q.grad, atol=1e-3 * scale, rtol=1e-2)
    assert seen > 20
