"""Surface tracing on the GPU (csrc/surface_trace.hip, ops.trace_rays, TriPlaneGenerator.trace_rays, ray_losses.implicit_depth)
against the torch restatement of tests/trace_ref.py and the float64 oracle.  Needs an MI355X:  python -m pytest tests -m gpu

1. logic, exact: the restatement in fp32 on the device with `ops.planes_query` as its density sees the kernel's density bits, so
   `hit` and `cell` agree for EVERY ray and t to 1e-6 max(1, |t|); what the kernel reports at the hit is `ops.planes_query_normals`
   at the returned point, to the bit.
2. accuracy: the float64 density at the returned point is within bar_sigma + w max|d sigma / dt| of the level (w: the final
   bracket; bar_sigma = 2e-5 max(1, max|sigma|): tests/test_gpu_shape.py's bar for 'sigma', both decoder precisions).
3. the generator's call, with every kind of limits.
4. the implicit gradient against the float64 formula on the oracle, under the project's gradient bar (normal_grad_ref.bar_ratio)."""
import dataclasses
import functools

import pytest
import torch

from tests import normal_grad_ref as NG
from tests import query_ref as Q
from tests import trace_ref as T
from tests.util import make_inputs, perturb_state, state_cpu

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "f16x3")
CASES = {"20x28": ((Q.H, Q.W), "eg3d_original"), "36x20-fixed": ((36, 20), "eg3d_fixed")}
RAYS = (1, 16, 53)                                    # one ray, one full tile, three tiles and a tail of 5
PLANS = ((1, 0), (7, 5), (64, 8))                     # (steps, refine)
LEVEL_STEPS = 64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _planes_dev(pn, dev):
    return pn.permute(0, 1, 3, 4, 2).contiguous().to(dev)          # oracle [B,3,C,H,W] -> [B,3,H,W,C]


def _dec_kw(dev, P, prec, axes):
    d = {k: P[k].to(dev) for k in Q.DEC_KEYS}
    return dict(dec_w0=d[Q.DEC_KEYS[0]], dec_b0=d[Q.DEC_KEYS[1]], dec_w1=d[Q.DEC_KEYS[2]], dec_b1=d[Q.DEC_KEYS[3]],
                box_warp=Q.BOX_WARP, plane_axes=axes, decoder_lr_mul=Q.LR_MUL, decoder_precision=prec)


def _dev_sigma(planes, kw):
    """The kernel's own density as the restatement's callable: `ops.planes_query`, sigma only."""
    from hfa_gp_amd import ops
    b = planes.shape[0]

    def sigma(x):
        return ops.planes_query(planes, x.reshape(b, -1, 3).contiguous(), want_rgb=False, **kw)[0].reshape(x.shape[:-1])
    return sigma


@functools.lru_cache(maxsize=None)
def ray_case(name, r):
    """The rays of a case on the CPU (fp32), the float64 oracle density, and the level: the 0.9 quantile of the reference's node
    densities.  For r = 53 four special rays stand at the end of the list: t_far <= t_near, a NaN limit, a ray outside every
    plane, and an origin at the densest node of its frame (inside: cell 0, t = t_near)."""
    hw, axes = CASES[name]
    P, pn = T.planes_case(hw)
    o, d, tn, tf = T.sphere_rays(torch.Generator().manual_seed(100 + r), Q.B, r)
    sig64 = T.oracle_sigma(P, pn.double(), axes)
    with torch.no_grad():
        nodes = T.node_sigmas(sig64, o.double(), d.double(), tn.double(), tf.double(), LEVEL_STEPS)
    level = float(torch.quantile(nodes[torch.isfinite(nodes)], 0.9))
    if r >= 53:
        tf[:, -4] = tn[:, -4]
        tn[:, -3] = float("nan")
        o[:, -2] = torch.tensor([3.0, -3.0, 2.0]) * Q.BOX_WARP
        d[:, -2] = torch.tensor([0.3, -0.2, 0.1])
        tn[:, -2], tf[:, -2] = 0.0, 1.0
        flat = torch.where(torch.isfinite(nodes), nodes, torch.full_like(nodes, -1e30)).reshape(Q.B, -1)
        best = flat.argmax(1)
        ray, node = best // (LEVEL_STEPS + 1), best % (LEVEL_STEPS + 1)
        for b in range(Q.B):
            t_best = tn[b, ray[b]] + (tf[b, ray[b]] - tn[b, ray[b]]) * float(node[b]) / LEVEL_STEPS
            o[b, -1] = o[b, ray[b]] + t_best * d[b, ray[b]]
            d[b, -1] = torch.tensor([0.4, 0.5, -0.3])
        tn[:, -1], tf[:, -1] = 0.0, 0.3
    return dict(P=P, pn=pn, axes=axes, rays=(o, d, tn, tf), level=level, sig64=sig64, max_node=float(nodes[torch.isfinite(nodes)].max()))


def _trace(dev, cs, prec, steps, refine, level=None, **kw):
    from hfa_gp_amd import ops
    planes = _planes_dev(cs["pn"], dev)
    o, d, tn, tf = (t.to(dev) for t in cs["rays"])
    dk = _dec_kw(dev, cs["P"], prec, cs["axes"])
    out = ops.trace_rays(planes, o, d, tn, tf, cs["level"] if level is None else level, steps, refine, **kw, **dk)
    return out, planes, (o, d, tn, tf), dk


# ----------------------------------------------------------------------------- 1. logic, exact
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_logic_is_the_restatement_on_the_kernels_density(dev, name, prec):
    from hfa_gp_amd import ops
    for r in RAYS:
        cs = ray_case(name, r)
        for steps, refine in PLANS:
            what = f"{name}/{prec}/R={r}/steps={steps}/refine={refine}"
            out, planes, (o, d, tn, tf), dk = _trace(dev, cs, prec, steps, refine)
            assert set(out) == set(ops._TRACE_OUT) and out["hit"].dtype == torch.uint8 and out["cell"].dtype == torch.int32
            ref = T.trace(_dev_sigma(planes, dk), o, d, tn, tf, cs["level"], steps, refine)
            hit = out["hit"].bool()
            assert torch.equal(hit, ref["hit"]), what
            assert torch.equal(out["cell"], ref["cell"]), what
            err = (out["t"] - ref["t"]).abs() / out["t"].abs().clamp_min(1.0)
            print(f"{what}: {int(hit.sum())} of {hit.numel()} rays hit, {int((out['cell'] > 0).sum())} with a bracket, "
                  f"max |t - t_ref| / max(1, |t|) = {float(err.max()):.3e}")
            assert bool((err <= 1e-6).all()), what
            assert all(bool(torch.isfinite(out[k]).all()) for k in ("t", "point", "sigma", "sigma_grad", "normal")), what
            # the point is torch's o + t d, and what is reported there is the point query's at that point: the same bits
            assert torch.equal(out["point"][hit], (o + out["t"][..., None] * d)[hit]), what
            q = ops.planes_query_normals(planes, out["point"], want=("sigma", "grad", "normal"), **dk)
            assert torch.equal(out["sigma"][hit], q["sigma"][..., 0][hit]), what
            assert torch.equal(out["sigma_grad"][hit], q["grad"][hit]) and torch.equal(out["normal"][hit], q["normal"][hit]), what
            # a miss: exact zeros everywhere
            for k in ("t", "point", "sigma", "sigma_grad", "normal"):
                assert bool((out[k][~hit] == 0).all()), (what, k)
            assert bool((out["cell"][~hit] == -1).all())
            if r >= 53:
                assert not bool(hit[:, -4:-2].any())                                    # the two empty rays
                assert bool((out["cell"][:, -1] == 0).all()) and bool((out["t"][:, -1] == 0).all())        # inside: t = t_near = 0
                assert torch.equal(out["point"][:, -1], o[:, -1])
                if bool(hit[:, -2].any()):                                               # outside every plane: no gradient there
                    assert bool((out["sigma_grad"][:, -2] == 0).all()) and bool((out["normal"][:, -2] == 0).all())
    # (on the last plan) one writer per ray: a second call gives the same bits, and so does every subset of the outputs
    again, *_ = _trace(dev, cs, prec, steps, refine)
    assert all(torch.equal(out[k], again[k]) for k in out)
    for want in (("t",), ("hit", "cell"), ("point", "normal"), ("sigma",), ("sigma_grad",), ("hit", "t", "point", "sigma")):
        part, *_ = _trace(dev, cs, prec, steps, refine, want=want)
        assert set(part) == set(want) and all(torch.equal(part[k], out[k]) for k in want), want
    # a level above every density: everything misses, every output is an exact zero
    none, *_ = _trace(dev, cs, prec, steps, refine, level=cs["max_node"] + 1e4)
    assert not bool(none["hit"].any()) and bool((none["cell"] == -1).all())
    assert all(bool((none[k] == 0).all()) for k in ("t", "point", "sigma", "sigma_grad", "normal"))


def test_ops_checks(dev):
    from hfa_gp_amd import ops
    cs = ray_case("20x28", 16)
    planes = _planes_dev(cs["pn"], dev)
    o, d, tn, tf = (t.to(dev) for t in cs["rays"])
    dk = _dec_kw(dev, cs["P"], "fp32", cs["axes"])
    with pytest.raises(ValueError, match="want"):
        ops.trace_rays(planes, o, d, tn, tf, 1.0, want=("t", "depth"), **dk)
    with pytest.raises(ValueError, match="steps"):
        ops.trace_rays(planes, o, d, tn, tf, 1.0, steps=4097, **dk)
    with pytest.raises(ValueError, match="refine"):
        ops.trace_rays(planes, o, d, tn, tf, 1.0, refine=-1, **dk)
    with pytest.raises(RuntimeError, match="t_near must be"):
        ops.trace_rays(planes, o, d, tn[:, :5].contiguous(), tf, 1.0, **dk)
    with pytest.raises(RuntimeError, match="CUDA"):
        ops.trace_rays(planes, o.cpu(), d, tn, tf, 1.0, **dk)
    empty = ops.trace_rays(planes, o[:, :0].contiguous(), d[:, :0].contiguous(), tn[:, :0].contiguous(), tf[:, :0].contiguous(), 1.0, **dk)
    assert empty["point"].shape == (Q.B, 0, 3) and empty["hit"].shape == (Q.B, 0)


# ----------------------------------------------------------------------------- 2. accuracy
@pytest.mark.parametrize("prec", PRECISIONS)
@pytest.mark.parametrize("name", list(CASES))
def test_returned_point_lies_on_the_float64_surface(dev, name, prec):
    cs = ray_case(name, 53)
    o, d, tn, tf = (t.double() for t in cs["rays"])
    for steps, refine in PLANS:
        out, *_ = _trace(dev, cs, prec, steps, refine)
        keep = (out["cell"] > 0).cpu()                                   # every ray with a bracket, none left out
        t = out["t"].cpu().double()
        w = torch.where(keep, T.bracket_width(tn, tf, steps, refine), torch.zeros_like(t))
        slopes = []
        for off in (-1.0, 0.0, 1.0):
            tt = (t + off * w).requires_grad_(True)
            s = cs["sig64"](o + tt[..., None] * d)
            slopes.append(torch.autograd.grad(s.sum(), tt)[0].abs())
            if off == 0.0:
                s_hit = s.detach()
        slope = torch.stack(slopes).amax(0)
        bar = 2e-5 * max(1.0, float(s_hit[keep].abs().max())) if bool(keep.any()) else 0.0
        ratio = ((s_hit - cs["level"]).abs() / (bar + w * slope))[keep]
        print(f"{name}/{prec}/steps={steps}/refine={refine}: {int(keep.sum())} rays, bar_sigma {bar:.3e}, "
              f"worst |sigma64(x*) - level| / bound = {float(ratio.max()) if ratio.numel() else 0.0:.3f}")
        assert bool((ratio <= 1.0).all())
    assert int(keep.sum()) >= 20                                         # (64, 8): the level lets most rays march to a crossing


# ----------------------------------------------------------------------------- 3, 4. through the generator (tiny64)
E2E_RES, E2E_STEPS, E2E_REFINE = 16, 32, 8


def _cfg():
    from hfa_gp_amd.config import PRESETS
    return dataclasses.replace(PRESETS["tiny64"](), conv_precision="fp32")


def _gen(dev, tuned=False):
    from hfa_gp_amd.generator import TriPlaneGenerator
    gen = perturb_state(TriPlaneGenerator(_cfg(), seed=0)).requires_grad_(False).to(dev)
    if tuned:
        for k in Q.DEC_KEYS:
            dict(gen.named_parameters())[k].requires_grad_(True)
    return gen


@functools.lru_cache(maxsize=None)
def e2e_case():
    """tiny64 in float64 on the CPU: the oracle's planes of ws, the rays of `ray_grid(c, 16)`, and the level — the 0.9 quantile of
    the oracle's node densities on the config's interval."""
    from hfa_gp_amd.cam_utils import ray_grid
    from hfa_gp_amd.generator import TriPlaneGenerator
    from oracle import eg3d_oracle as O
    cfg = _cfg()
    P = state_cpu(perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False))
    P = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    ws, c, us, ui = make_inputs(cfg, 2)
    o, d = ray_grid(c, E2E_RES)
    r = cfg.plane_resolution
    with torch.no_grad():
        pn = O.backbone_synthesis(P, cfg, ws.double()).reshape(2, 3, 32, r, r)
        sig = _oracle_sigma(P, pn, cfg)
        tn = torch.full(o.shape[:2], float(cfg.ray_start), dtype=torch.float64)
        tf = torch.full(o.shape[:2], float(cfg.ray_end), dtype=torch.float64)
        nodes = T.node_sigmas(sig, o.double(), d.double(), tn, tf, E2E_STEPS)
    return dict(cfg=cfg, P=P, inputs=(ws, c, us, ui), rays=(o, d), level=float(torch.quantile(nodes, 0.9)))


def _oracle_sigma(P, pn, cfg):
    from oracle import eg3d_oracle as O

    def sigma(x):
        flat = x.reshape(pn.shape[0], -1, 3)
        return O.osg_decoder(P, O.sample_from_planes(O.plane_axes(cfg.plane_axes), pn, flat, cfg.box_warp),
                             cfg.decoder_lr_mul)[1].reshape(x.shape[:-1])
    return sigma


def test_generator_trace_rays_with_every_kind_of_limits(dev, monkeypatch):
    from hfa_gp_amd import ops
    from hfa_gp_amd.cam_utils import ray_limits_valid
    cs = e2e_case()
    gen = _gen(dev)
    ws, c, us, ui = (t.to(dev) for t in cs["inputs"])
    o, d = (t.to(dev) for t in cs["rays"])
    kw = dict(level=cs["level"], steps=E2E_STEPS, refine=E2E_REFINE)
    with torch.no_grad():
        occ = gen.occupancy_grid(ws, resolution=16, level=cs["level"] - 5.0)
        seen = 0
        for limits in (None, "box", occ):
            out = gen.trace_rays(ws, o, d, ray_limits=limits, **kw)
            keys = {"hit", "cell", "t", "point", "sigma", "sigma_grad", "normal"} | ({"valid"} if limits is not None else set())
            assert set(out) == keys and out["hit"].dtype == torch.bool and out["t"].shape == (2, E2E_RES ** 2)
            hit = out["hit"]
            print(f"limits {limits if not hasattr(limits, 'bits') else 'occupancy grid'}: {int(hit.sum())} of {hit.numel()} rays hit, "
                  f"{int((out['cell'] > 0).sum())} with a bracket")
            seen += int((out["cell"] > 0).sum())
            q = gen.sample_mixed(out["point"], None, ws, normals=True)
            assert torch.equal(q["sigma"][..., 0][hit], out["sigma"][hit])
            assert torch.equal(q["sigma_grad"][hit], out["sigma_grad"][hit]) and torch.equal(q["normal"][hit], out["normal"][hit])
            assert torch.equal(out["point"][hit], (o + out["t"][..., None] * d)[hit])
            for k in ("t", "point", "sigma", "sigma_grad", "normal"):
                assert bool((out[k][~hit] == 0).all()), k
            plain = gen.trace_rays(ws, o, d, ray_limits=limits, normals=False, **kw)
            assert "normal" not in plain and "sigma_grad" not in plain
            assert all(torch.equal(plain[k], out[k]) for k in plain)
            if limits is not None:
                rr = gen.render_rays(ws, o, d, ray_limits=limits)
                assert torch.equal(out["valid"], rr["valid"])
                assert not bool(hit[~out["valid"]].any())
                tn, tf = (ops.ray_limits_box(o, d, gen.cfg.box_warp) if limits == "box" else ops.ray_limits_grid(o, d, limits))
                assert torch.equal(out["valid"], ray_limits_valid(tn, tf))
                explicit = gen.trace_rays(ws, o, d, t_near=tn, t_far=tf, **kw)
                assert all(torch.equal(explicit[k], out[k]) for k in out)
        assert seen > 0
        # explicit floats are the config's interval when they are its ends
        a = gen.trace_rays(ws, o, d, **kw)
        b = gen.trace_rays(ws, o, d, t_near=gen.cfg.ray_start, t_far=gen.cfg.ray_end, **kw)
        assert all(torch.equal(a[k], b[k]) for k in a) and bool(b["valid"].all())
        # no rays: empty tensors, nothing launched
        calls = []
        real = ops.trace_rays
        monkeypatch.setattr(ops, "trace_rays", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
        for ob, db, wb in ((o[:, :0], d[:, :0], ws), (o[:0], d[:0], ws[:0])):
            e = gen.trace_rays(wb, ob, db, ray_limits="box", **kw)
            assert e["point"].shape == ob.shape and e["hit"].dtype == torch.bool and e["valid"].shape == ob.shape[:2]
        assert calls == []
        gen.trace_rays(ws, o, d, **kw)
        assert calls == [1]
    with pytest.raises(RuntimeError, match="no_grad"):
        gen.trace_rays(ws.clone().requires_grad_(True), o, d, **kw)
    with pytest.raises(NotImplementedError, match="requires grad"):
        gen.trace_rays(ws, o, d, t_near=torch.zeros(2, E2E_RES ** 2, device=dev, requires_grad=True), t_far=1.0, **kw)


def _reference_grads(cs, t_star, mask, c_t, c_p, probe=False):
    """float64: d/d(ws, decoder tensors, o, d) of L = sum c_t t + sum c_p . point by the implicit formula on the oracle, at the
    device's t*.  ``probe``: only the float64 slope decisions and cosines (no gradient w.r.t. ws or the decoder)."""
    from oracle import eg3d_oracle as O
    cfg = cs["cfg"]
    P = dict(cs["P"])
    for k in Q.DEC_KEYS:
        P[k] = P[k].detach().clone().requires_grad_(not probe)
    ws_ref = cs["inputs"][0].double().requires_grad_(not probe)
    r = cfg.plane_resolution
    with torch.set_grad_enabled(not probe):
        pn = O.backbone_synthesis(P, cfg, ws_ref).reshape(2, 3, 32, r, r)
    with torch.enable_grad():
        params = [] if probe else [ws_ref] + [P[k] for k in Q.DEC_KEYS]
        grads, d_o, d_d, carries, cos = T.implicit_grads(_oracle_sigma(P, pn, cfg), params, cs["rays"][0], cs["rays"][1], t_star, mask,
                                                          c_t, c_p)
    return dict(ws=grads[0] if grads else None, dec=grads[1:], o=d_o, d=d_d, carries=carries, cos=cos)


def test_implicit_gradient_against_the_float64_formula(dev):
    """L = sum c_r t_r + sum C_r . point_r through trace_rays(differentiable=True): d ws, the decoder gradients and the rays'
    gradients against the float64 implicit formula on the oracle, fed the device's t*, each under normal_grad_ref.bar_ratio <= 1.
    Rays on which the fp32 and the float64 slope-floor decisions differ leave both sides (at most 2 % of the rays)."""
    from hfa_gp_amd.ray_losses import implicit_depth, transversal
    cs = e2e_case()
    gen = _gen(dev, tuned=True)
    ws, c, us, ui = (t.to(dev) for t in cs["inputs"])
    n = E2E_RES ** 2
    g = torch.Generator().manual_seed(17)
    c_t, c_p = torch.randn(2, n, generator=g), torch.randn(2, n, 3, generator=g)
    kw = dict(level=cs["level"], steps=E2E_STEPS, refine=E2E_REFINE)
    with torch.no_grad():
        tr = gen.trace_rays(ws, cs["rays"][0].to(dev), cs["rays"][1].to(dev), **kw)
    mask = (tr["hit"] & (tr["cell"] > 0)).cpu()
    on32 = mask & transversal(tr["sigma_grad"], cs["rays"][1].to(dev)).cpu()
    probe = _reference_grads(cs, tr["t"].cpu(), mask, c_t, c_p, probe=True)
    cos = probe["cos"][mask]
    clear = float(((cos - 0.01).abs() > 1e-3).double().mean())
    differ = on32 != probe["carries"]
    print(f"{int(mask.sum())} of {mask.numel()} rays with a bracket, {int(on32.sum())} above the slope floor in fp32; "
          f"{clear:.4f} of them keep the cosine clear of 0.01 +- 1e-3; the decisions differ on {int(differ.sum())} rays")
    assert int(on32.sum()) >= 32 and clear >= 0.98 and float(differ.double().mean()) <= 0.02
    c_t, c_p = c_t * (~differ), c_p * (~differ)[..., None]
    ref = _reference_grads(cs, tr["t"].cpu(), mask & ~differ, c_t, c_p)
    # --- the device
    ws_d = ws.clone().requires_grad_(True)
    o_d, d_d = cs["rays"][0].to(dev).requires_grad_(True), cs["rays"][1].to(dev).requires_grad_(True)
    out = gen.trace_rays(ws_d, o_d, d_d, differentiable=True, **kw)
    assert out["t"].requires_grad and out["point"].requires_grad and not out["sigma"].requires_grad
    assert torch.equal(out["t"].detach(), tr["t"]) and torch.equal(out["point"].detach(), tr["point"])
    assert all(torch.equal(out[k], tr[k]) for k in ("hit", "cell", "sigma", "sigma_grad", "normal"))
    ((out["t"] * c_t.to(dev)).sum() + (out["point"] * c_p.to(dev)).sum()).backward()
    prm = dict(gen.named_parameters())
    ratios = {"ws": NG.bar_ratio(ws_d.grad, ref["ws"]), "o": NG.bar_ratio(o_d.grad, ref["o"]), "d": NG.bar_ratio(d_d.grad, ref["d"])}
    for k, want in zip(Q.DEC_KEYS, ref["dec"]):
        ratios[k] = NG.bar_ratio(prm[k].grad, want)
    print("differentiable=True, err / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          f"; ref max |d ws| {float(ref['ws'].abs().max()):.3e}")
    assert max(ratios.values()) <= 1.0, ratios
    # rays off the formula: exactly zero gradient
    off = ~(on32 & ~differ).to(dev)
    assert bool((o_d.grad[off] == 0).all()) and bool((d_d.grad[off] == 0).all())
    assert float(o_d.grad[~off].abs().max()) > 0
    # --- the same depth term on an image pass: trace under no_grad, the points through synthesis(query=), implicit_depth
    for p in gen.parameters():
        p.grad = None
    ws_q = ws.clone().requires_grad_(True)
    syn = gen.synthesis(ws_q, c, noise_mode="const", u_strat=us, u_imp=ui, query=tr["point"])
    t = implicit_depth(tr["t"], syn["query_sigma"], tr["sigma_grad"], cs["rays"][1].to(dev), mask=mask.to(dev))
    assert torch.equal(t.detach(), tr["t"])
    pt = cs["rays"][0].to(dev) + t[..., None] * cs["rays"][1].to(dev)
    ((t * c_t.to(dev)).sum() + (pt * c_p.to(dev)).sum()).backward()
    ratios = {"ws": NG.bar_ratio(ws_q.grad, ref["ws"])}
    for k, want in zip(Q.DEC_KEYS, ref["dec"]):
        ratios[k] = NG.bar_ratio(prm[k].grad, want)
    print("synthesis(query=) + implicit_depth, err / bar: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # --- inside a trainer step scope the stand-alone differentiable call raises
    gen._grad_sink = lambda p, g_: None
    try:
        with pytest.raises(RuntimeError, match="trainer step scope"):
            gen.trace_rays(ws.clone().requires_grad_(True), cs["rays"][0].to(dev), cs["rays"][1].to(dev), differentiable=True, **kw)
    finally:
        gen._grad_sink = None
