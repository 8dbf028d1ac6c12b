"""Backward of the tri-plane point query (csrc/planes_query_bwd.hip, ops.planes_query_bwd, synthesis(query=),
sample_mixed(differentiable=True)) against float64 autograd through the CPU oracle (tests/query_ref.py).
Needs an MI355X:  python -m pytest tests -m gpu

Bar: `close_grad` of tests/test_gpu_geometry_grad.py (atol 2e-5 * max(1, max|ref|), rtol 1e-3 per element), the project's
own for renderer gradients against oracle autograd.  The test points keep 1e-3 of a texel clear of every texel edge (where the
bilinear gather has no derivative), so EVERY point is compared."""
import dataclasses
import functools

import pytest
import torch

from tests import query_ref as Q
from tests.test_gpu_geometry_grad import close, close_grad
from tests.util import make_inputs, perturb_state, state_cpu

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


def _bwd(dev, P, planes, coords, g_sigma, g_rgb, prec, axes, box_warp=Q.BOX_WARP, lr_mul=Q.LR_MUL, **kw):
    from hfa_gp_amd import ops
    d = {k: v.to(dev) for k, v in P.items()}
    return ops.planes_query_bwd(planes, coords.to(dev), None if g_sigma is None else g_sigma.to(dev),
                                None if g_rgb is None else g_rgb.to(dev), dec_w0=d[Q.DEC_KEYS[0]], dec_b0=d[Q.DEC_KEYS[1]],
                                dec_w1=d[Q.DEC_KEYS[2]], dec_b1=d[Q.DEC_KEYS[3]], box_warp=box_warp, plane_axes=axes,
                                decoder_lr_mul=lr_mul, decoder_precision=prec, **kw)


def _check_all(got, ref, what):
    d_planes, d_coords, dec = got
    close_grad(d_planes.permute(0, 1, 4, 2, 3), ref["planes"], f"{what}/planes")
    close_grad(d_coords, ref["coords"], f"{what}/coords")
    for g, r, k in zip(dec, ref["dec"], Q.DEC_KEYS):
        close_grad(g, r, f"{what}/{k}")


# ----------------------------------------------------------------------------- 1. the op against the reference
@pytest.mark.parametrize("which", list(Q.UPSTREAM))
@pytest.mark.parametrize("axes", Q.AXES)
@pytest.mark.parametrize("prec", PRECISIONS)
def test_op_vs_reference(dev, prec, axes, which):
    cs = Q.base_case()
    use_s, use_r = Q.UPSTREAM[which]
    ref = Q.base_reference(axes, which)
    got = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), cs["coords"], cs["ups"]["g_sigma"] if use_s else None,
               cs["ups"]["g_rgb"] if use_r else None, prec, axes, coords_grad=True, decoder_grads=True)
    _check_all(got, ref, f"{prec}/{axes}/{which}")
    # the first two special points lie outside every plane: exact zeros
    assert bool((got[1][:, :2] == 0).all())
    assert bool((ref["coords"][:, :2] == 0).all())
    # the instances without the point gradient / the decoder gradients give the same plane gradient within the bar
    only = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), cs["coords"], cs["ups"]["g_sigma"] if use_s else None,
                cs["ups"]["g_rgb"] if use_r else None, prec, axes)
    assert only[1] is None and only[2] is None
    close_grad(only[0].permute(0, 1, 4, 2, 3), ref["planes"], f"{prec}/{axes}/{which}/planes only")


# ----------------------------------------------------------------------------- 2. broadcast
@pytest.mark.parametrize("prec", PRECISIONS)
def test_broadcast_points_sum_over_identities(dev, prec):
    cs = Q.base_case()
    ref = Q.base_reference("eg3d_original", "both", True)
    got = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), cs["coords"][:1], cs["ups"]["g_sigma"], cs["ups"]["g_rgb"], prec,
               "eg3d_original", coords_grad=True, decoder_grads=True)
    assert got[1].shape == (Q.B, Q.M, 3)
    _check_all((got[0], got[1].sum(0, keepdim=True), got[2]), ref, f"broadcast/{prec}")


# ----------------------------------------------------------------------------- 3. accumulate contract
def test_accumulates_into_d_planes_and_dec_out(dev):
    cs = Q.base_case()
    ref = Q.base_reference("eg3d_fixed", "both")
    g = torch.Generator().manual_seed(21)
    planes = _planes_dev(cs["pn"], dev)
    pre_pl = torch.randn(planes.shape, generator=g).to(dev)
    pre_dec = tuple(torch.randn(cs["P"][k].shape, generator=g).to(dev) for k in Q.DEC_KEYS)
    d_pl, dec = pre_pl.clone(), tuple(t.clone() for t in pre_dec)
    out_pl, d_co, out_dec = _bwd(dev, cs["P"], planes, cs["coords"], cs["ups"]["g_sigma"], cs["ups"]["g_rgb"], "f16x3", "eg3d_fixed",
                                 d_planes=d_pl, coords_grad=True, decoder_grads=True, dec_out=dec)
    assert out_pl is d_pl and all(a is b for a, b in zip(out_dec, dec))
    _check_all((d_pl - pre_pl, d_co, tuple(a - b for a, b in zip(dec, pre_dec))), ref, "accumulate")
    # d_planes=False: the point gradient alone
    none_pl, d_co2, none_dec = _bwd(dev, cs["P"], planes, cs["coords"], cs["ups"]["g_sigma"], cs["ups"]["g_rgb"], "f16x3",
                                    "eg3d_fixed", d_planes=False, coords_grad=True)
    assert none_pl is None and none_dec is None
    assert torch.equal(d_co2, d_co)           # no atomics on this path: the same bits
    with pytest.raises(ValueError):
        _bwd(dev, cs["P"], planes, cs["coords"], cs["ups"]["g_sigma"], None, "f16x3", "eg3d_fixed", d_planes=False)
    with pytest.raises(ValueError):
        _bwd(dev, cs["P"], planes, cs["coords"], None, None, "f16x3", "eg3d_fixed")


# ----------------------------------------------------------------------------- 4. collisions
@pytest.mark.parametrize("prec", PRECISIONS)
def test_identical_points_collide_on_twelve_lines(dev, prec):
    cs = Q.base_case()
    g = torch.Generator().manual_seed(22)
    m = 64
    pt = torch.tensor([[0.11, -0.23, 0.07], [-0.31, 0.05, 0.19]])
    coords = pt[:, None].expand(Q.B, m, 3).contiguous()
    assert not Q.near_edge(coords, Q.BOX_WARP, Q.H, Q.W).any()
    gs, gr = torch.randn(Q.B, m, 1, generator=g), torch.randn(Q.B, m, 32, generator=g)
    ref = Q.reference(cs["P"], cs["pn"], coords, gs, gr, Q.BOX_WARP, "eg3d_original", Q.LR_MUL)
    assert int((ref["planes"].abs().sum(2) != 0).sum()) == Q.B * 12
    got = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), coords, gs, gr, prec, "eg3d_original", coords_grad=True, decoder_grads=True)
    _check_all(got, ref, f"collisions/{prec}")


# ----------------------------------------------------------------------------- 5. ragged sizes
@pytest.mark.parametrize("m", [1, 16, 17])
def test_ragged_point_counts(dev, m):
    cs = Q.base_case()
    g = torch.Generator().manual_seed(23 + m)
    coords = Q.make_points(g, Q.B, m, special=False, spread=0.9)
    gs, gr = torch.randn(Q.B, m, 1, generator=g), torch.randn(Q.B, m, 32, generator=g)
    ref = Q.reference(cs["P"], cs["pn"], coords, gs, gr, Q.BOX_WARP, "eg3d_fixed", Q.LR_MUL)
    for prec in PRECISIONS:
        got = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), coords, gs, gr, prec, "eg3d_fixed", coords_grad=True, decoder_grads=True)
        _check_all(got, ref, f"M={m}/{prec}")


# ----------------------------------------------------------------------------- 6. zero upstream gradient
def test_zero_upstream_gives_exact_zeros(dev):
    cs = Q.base_case()
    for prec in PRECISIONS:
        got = _bwd(dev, cs["P"], _planes_dev(cs["pn"], dev), cs["coords"], torch.zeros(Q.B, Q.M, 1), torch.zeros(Q.B, Q.M, 32), prec,
                   "eg3d_original", coords_grad=True, decoder_grads=True)
        for t in (got[0], got[1]) + tuple(got[2]):
            assert bool(torch.isfinite(t).all()) and bool((t == 0).all())


# ----------------------------------------------------------------------------- 7. after the ray marcher, into its d_planes
def test_query_gradient_joins_the_ray_marchers_on_mirrored_planes(dev):
    """eg3d_original axes on square planes: ops.raymarch_bwd scatters planes 0 and 1 and OVERWRITES plane 2 with plane 1 transposed;
    the query kernel, launched after it into the same d_planes, adds to all three planes.  What is checked: joined = ray marcher +
    query within the bar, and (joined - ray marcher) = the float64 reference of the query, plane 2 included.
    What is NOT checked: that plane 2 is "no transpose of plane 1", nor the launch order.  On these planes a free point's plane-2
    gradient is itself the transpose of its plane-1 gradient (same taps with row and column swapped, one dL/dF for the three planes),
    so the joined plane 2 is the transpose of the joined plane 1 up to atomic order, and query-first-then-mirror would give the same
    sum: no assertion on the result can tell the two orders apart.  The order is fixed in autograd.SynthesisFn.backward."""
    from tests.test_gpu_geometry_grad import case, device_call
    rc = case("small128")
    assert rc["cfg"].plane_axes == "eg3d_original" and rc["planes"].shape[-2:] == (20, 20)
    cfg = rc["cfg"]
    ray_alone, _, _ = device_call(rc, dev, "all")
    joined, _, _ = device_call(rc, dev, "all")
    planes = rc["planes"].detach().permute(0, 1, 3, 4, 2).contiguous().to(dev)
    P = {k: rc["P"][k].detach() for k in Q.DEC_KEYS}
    g = torch.Generator().manual_seed(24)
    m = 16 * 5 + 3
    coords = Q.make_points(g, rc["b"], m, cfg.box_warp, 20, 20, special=False, spread=1.1)
    gs, gr = torch.randn(rc["b"], m, 1, generator=g), torch.randn(rc["b"], m, 32, generator=g)
    kw = dict(box_warp=cfg.box_warp, lr_mul=cfg.decoder_lr_mul)
    q_alone, _, _ = _bwd(dev, P, planes, coords, gs, gr, cfg.decoder_precision, "eg3d_original", **kw)
    out, _, _ = _bwd(dev, P, planes, coords, gs, gr, cfg.decoder_precision, "eg3d_original", d_planes=joined, **kw)
    assert out is joined
    close_grad(joined, ray_alone + q_alone, "joined")
    ref = Q.reference(P, rc["planes"].detach(), coords, gs, gr, cfg.box_warp, "eg3d_original", cfg.decoder_lr_mul)
    close_grad((joined - ray_alone).permute(0, 1, 4, 2, 3), ref["planes"], "joined - ray marcher")
    assert float(q_alone[:, 2].abs().max()) > 0
    assert not torch.equal(joined[:, 2], ray_alone[:, 2])


# ----------------------------------------------------------------------------- 8 - 13. through the generator
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
    """One oracle pass (fp32, as test_synthesis_backward_vs_oracle_autograd): O.synthesis plus the query on the planes of the
    same ws; loss <image, G> + <query_sigma, Gs> + <query_rgb, Gr>; gradients w.r.t. ws, the points, the decoder tensors and one
    backbone conv weight."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    for k in TUNED_KEYS:
        P[k].requires_grad_(True)
    ws, c, us, ui = make_inputs(cfg, 2)
    g = torch.Generator().manual_seed(31)
    r = cfg.plane_resolution
    coords = Q.make_points(g, 2, M_E2E, cfg.box_warp, r, r, special=False, spread=1.1)
    G = torch.randn(2, 3, cfg.img_resolution, cfg.img_resolution, generator=g) / cfg.img_resolution
    Gs = torch.randn(2, M_E2E, 1, generator=g) / 8
    Gr = torch.randn(2, M_E2E, 32, generator=g) / 8
    ws_ref, co_ref = ws.clone().requires_grad_(True), coords.clone().requires_grad_(True)
    ref = O.synthesis(P, cfg, ws_ref, c, us, ui, return_planes=True)
    pn = ref["planes"].reshape(2, 3, 32, r, r)
    rgb, sigma = O.osg_decoder(P, O.sample_from_planes(O.plane_axes(cfg.plane_axes), pn, co_ref, cfg.box_warp), cfg.decoder_lr_mul)
    loss = (ref["image"] * G).sum() + (sigma * Gs).sum() + (rgb * Gr).sum()
    grads = torch.autograd.grad(loss, [ws_ref, co_ref] + [P[k] for k in TUNED_KEYS])
    return dict(inputs=(ws, c, us, ui), coords=coords, G=G, Gs=Gs, Gr=Gr, d_ws=grads[0], d_coords=grads[1],
                d_params=dict(zip(TUNED_KEYS, grads[2:])))


def _e2e_device(dev, gen, coords_grad=False, ws_grad=True, image=True):
    rf = e2e_reference()
    ws, c, us, ui = rf["inputs"]
    ws_d = ws.to(dev).requires_grad_(ws_grad)
    co_d = rf["coords"].to(dev).requires_grad_(coords_grad)
    out = gen.synthesis(ws_d, c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), query=co_d)
    loss = (out["query_sigma"] * rf["Gs"].to(dev)).sum() + (out["query_rgb"] * rf["Gr"].to(dev)).sum()
    if image:
        loss = loss + (out["image"] * rf["G"].to(dev)).sum()
    loss.backward()
    return out, ws_d, co_d


def test_synthesis_query_end_to_end_frozen(dev):
    rf = e2e_reference()
    out, ws_d, co_d = _e2e_device(dev, _gen(dev), coords_grad=True)
    assert set(out) == {"image", "image_raw", "image_depth", "query_sigma", "query_rgb"}
    assert out["query_sigma"].shape == (2, M_E2E, 1) and out["query_rgb"].shape == (2, M_E2E, 32)
    scale = rf["d_ws"].abs().max().item()
    close(ws_d.grad, rf["d_ws"], atol=2e-4 * scale, rtol=2e-3, what="d ws")
    close_grad(co_d.grad, rf["d_coords"], "d coords")


def test_synthesis_query_end_to_end_tuned(dev):
    from tests.test_gpu_round4 import rel_l2
    rf = e2e_reference()
    gen = _gen(dev, tuned=True)
    _, ws_d, _ = _e2e_device(dev, gen)
    scale = rf["d_ws"].abs().max().item()
    close(ws_d.grad, rf["d_ws"], atol=2e-4 * scale, rtol=2e-3, what="d ws (tuned)")
    prm = dict(gen.named_parameters())
    for k in Q.DEC_KEYS:
        close_grad(prm[k].grad, rf["d_params"][k], k)
    k = TUNED_KEYS[-1]
    err = rel_l2(prm[k].grad, rf["d_params"][k])
    print(f"{k}: rel-L2 {err:.3e}")
    assert err <= 2e-3


def test_geometry_and_camera_compose_with_query(dev):
    gen = _gen(dev)
    rf = e2e_reference()
    ws, c, us, ui = rf["inputs"]
    c_d = c.to(dev).requires_grad_(True)
    ws_d = ws.to(dev).requires_grad_(True)
    out = gen.synthesis(ws_d, c_d, noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True, query=rf["coords"].to(dev))
    assert set(out) == {"image", "image_raw", "image_depth", "image_mask", "query_sigma", "query_rgb"}
    (out["image_mask"].mean() + out["image_depth"].mean() + out["query_sigma"].mean()).backward()
    assert c_d.grad is not None and bool(torch.isfinite(c_d.grad).all()) and float(c_d.grad.abs().max()) > 0
    # the same loss without the query term + the query term alone = the joint gradient (one pass instead of two)
    ws_a = ws.to(dev).requires_grad_(True)
    o = gen.synthesis(ws_a, c.to(dev), noise_mode="const", u_strat=us.to(dev), u_imp=ui.to(dev), geometry=True)
    (o["image_mask"].mean() + o["image_depth"].mean()).backward()
    ws_b = ws.to(dev).requires_grad_(True)
    gen.sample_mixed(rf["coords"].to(dev), None, ws_b, differentiable=True)["sigma"].mean().backward()
    want = ws_a.grad + ws_b.grad
    close(ws_d.grad, want, atol=1e-4 * float(want.abs().max()), rtol=1e-3, what="geometry + query")


# ----------------------------------------------------------------------------- 9. query-only loss
def test_query_only_loss_matches_stand_alone_sample_mixed(dev):
    """The image outputs are unused (their gradients arrive as None).  The two forms differ only in atomic order."""
    gen = _gen(dev)
    rf = e2e_reference()
    _, ws_d, co_d = _e2e_device(dev, gen, coords_grad=True, image=False)
    ws_s = rf["inputs"][0].to(dev).requires_grad_(True)
    co_s = rf["coords"].to(dev).requires_grad_(True)
    o = gen.sample_mixed(co_s, None, ws_s, differentiable=True)
    assert o["sigma"].requires_grad and o["rgb"].requires_grad
    ((o["sigma"] * rf["Gs"].to(dev)).sum() + (o["rgb"] * rf["Gr"].to(dev)).sum()).backward()
    scale = float(ws_s.grad.abs().max())
    err = float((ws_d.grad - ws_s.grad).abs().max())
    print(f"query-only: d ws max diff {err:.3e}, scale {scale:.3e}, ratio {err / scale:.3e}")
    assert scale > 0 and err <= 1e-5 * scale
    assert torch.equal(co_d.grad, co_s.grad)                  # the point gradient has one writer per point: the same bits
    # and the stand-alone form against the oracle's query-only gradient
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = state_cpu(gen)
    ws_ref = rf["inputs"][0].clone().requires_grad_(True)
    r = cfg.plane_resolution
    pn = O.backbone_synthesis(P, cfg, ws_ref).reshape(2, 3, 32, r, r)
    rgb, sigma = O.osg_decoder(P, O.sample_from_planes(O.plane_axes(cfg.plane_axes), pn, rf["coords"], cfg.box_warp), cfg.decoder_lr_mul)
    ((sigma * rf["Gs"]).sum() + (rgb * rf["Gr"]).sum()).backward()
    close(ws_s.grad, ws_ref.grad, atol=2e-4 * float(ws_ref.grad.abs().max()), rtol=2e-3, what="sample_mixed d ws")


# ----------------------------------------------------------------------------- 10. forward consistency
def test_forward_is_the_bits_of_sample_mixed_and_leaves_the_image_alone(dev):
    gen = _gen(dev)
    rf = e2e_reference()
    ws, c, us, ui = (t.to(dev) for t in rf["inputs"])
    co = rf["coords"].to(dev)
    # the public call without the keyword still refuses a gradient, and now names the keyword
    with pytest.raises(RuntimeError, match="no_grad") as refusal:
        gen.sample_mixed(co, None, ws.clone().requires_grad_(True))
    assert "differentiable=True" in str(refusal.value)
    with torch.no_grad():
        want = gen.sample_mixed(co, None, ws)
        plain = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
        with_q = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, query=co)
    plain_grad = gen.synthesis(ws.clone().requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui)
    under_grad = gen.synthesis(ws.clone().requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui, query=co)
    for out, base in ((with_q, plain), (under_grad, plain_grad)):      # (each against the call without query= in the same mode)
        assert torch.equal(out["query_sigma"], want["sigma"]) and torch.equal(out["query_rgb"], want["rgb"])
        for k in ("image", "image_raw", "image_depth"):
            assert torch.equal(out[k], base[k]), k
    assert under_grad["query_sigma"].requires_grad and not with_q["query_sigma"].requires_grad
    one = gen.synthesis(ws.clone().requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui, query=co[:1])
    assert torch.equal(one["query_sigma"][0], want["sigma"][0])
    with pytest.raises(ValueError, match="query"):
        gen.synthesis(ws, c, noise_mode="const", query=co[:, :, :2])


# ----------------------------------------------------------------------------- 11. the image-only path is untouched
def test_synthesis_without_query_never_calls_the_query_backward(dev, monkeypatch):
    from hfa_gp_amd import ops
    calls = []
    monkeypatch.setattr(ops, "planes_query_bwd", lambda *a, **k: calls.append(1))
    real_query = ops.planes_query
    monkeypatch.setattr(ops, "planes_query", lambda *a, **k: (calls.append(2), real_query(*a, **k))[1])
    gen = _gen(dev, tuned=True)
    ws, c, us, ui = (t.to(dev) for t in e2e_reference()["inputs"])
    ws.requires_grad_(True)
    for geometry in (False, True):
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, geometry=geometry)
        assert "query_sigma" not in out
        out["image"].mean().backward()
    assert calls == []


# ----------------------------------------------------------------------------- 12. the sink invariant
def test_every_parameter_reaches_the_gradient_sink_once(dev):
    rf = e2e_reference()
    gen = _gen(dev, tuned=True)
    names = {id(p): n for n, p in gen.named_parameters()}

    def run(query):
        counts = {}
        for p in gen.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None

        def sink(p, g):
            if g is not None:
                p.grad.add_(g.view_as(p.grad))
            counts[names[id(p)]] = counts.get(names[id(p)], 0) + 1
        gen._grad_sink = sink
        try:
            ws, c, us, ui = (t.to(dev) for t in rf["inputs"])
            out = gen.synthesis(ws.requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui,
                                query=rf["coords"].to(dev) if query else None)
            loss = (out["image"] * rf["G"].to(dev)).sum()
            if query:
                loss = loss + (out["query_sigma"] * rf["Gs"].to(dev)).sum() + (out["query_rgb"] * rf["Gr"].to(dev)).sum()
            loss.backward()
            if query:
                with pytest.raises(RuntimeError, match=r"synthesis\(.*query="):
                    gen.sample_mixed(rf["coords"].to(dev), None, ws, differentiable=True)
        finally:
            gen._grad_sink = None
        return counts, {n: p.grad.clone() for n, p in gen.named_parameters() if p.requires_grad}

    base, _ = run(False)
    counts, grads = run(True)
    # every parameter the image-only pass releases (all but those its forward never reads: the noise strengths of the
    # super-resolution blocks, which run without noise) is released by the joined pass too, each exactly once
    assert set(Q.DEC_KEYS) <= set(base) and len(base) > 50
    assert counts == base and set(counts.values()) == {1}
    for k in Q.DEC_KEYS:             # the sink received the joint gradient (image + query)
        close_grad(grads[k], rf["d_params"][k], f"sink/{k}")


# ----------------------------------------------------------------------------- 13. density regularisation descends
def test_density_regularisation_descends(dev):
    """EG3D's recipe (loss.py): random points and copies perturbed by 0.004 * box_warp, L1 between the two densities; ten Adam steps
    on ws alone lower it — a check of sign and scale, not of a rate."""
    gen = _gen(dev)
    cfg = gen.cfg
    ws, c, us, ui = (t.to(dev) for t in e2e_reference()["inputs"])
    g = torch.Generator().manual_seed(41)
    pts = (torch.rand(2, 200, 3, generator=g) * 2 - 1) * (cfg.box_warp / 2)
    pert = pts + torch.randn(2, 200, 3, generator=g) * (0.004 * cfg.box_warp)
    coords = torch.cat([pts, pert], 1).to(dev)
    ws = ws.clone().requires_grad_(True)
    opt = torch.optim.Adam([ws], lr=2e-3)
    losses = []
    for _ in range(11):
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, query=coords)
        sigma = out["query_sigma"]
        loss = torch.nn.functional.l1_loss(sigma[:, :200], sigma[:, 200:])
        losses.append(loss.item())
        opt.zero_grad()
        loss.backward()
        opt.step()
    print("density regularisation:", " ".join(f"{v:.4e}" for v in losses))
    assert losses[-1] < losses[0]
