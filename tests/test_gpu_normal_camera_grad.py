"""The camera gradient of the per-ray surface normals on the device (hfagp_raymarch_normals_bwd_camera,
ops.raymarch_normals_bwd_camera, synthesis(normal_camera_grad=True)) against the float64 reference of tests/normal_camera_ref.py.
Needs an MI355X:  python -m pytest tests -m gpu

As in tests/test_gpu_normal_grad.py the reference takes the DEVICE's sorted sample depths (read from the ray marcher's state) and the
upstream gradient is multiplied by the reference's edge mask.  Tolerance per case: the project's gradient bar (atol 2e-5 max(1,
max|ref|), rtol 1e-3) times max(1, 4 rho), rho = the fp32 reference's own worst err / bar on that case (d x and d c), recomputed in
the same run (normal_camera_ref.oracle_rho); the factor 4 allows for the device's summation order, the split-operand decoder and the
hardware reciprocal square root.  Every comparison prints its worst err / bar."""
import functools

import pytest
import torch

from tests import camera_ref as CR
from tests import normal_camera_ref as NC
from tests import normal_grad_ref as G
from tests import normals_ref as N
from tests.test_gpu_normal_grad import B, _cfg, _gen, _gen_cpu, _inputs, _target, forward_state, state_depths
from tests.util import FLIP_COLUMNS, SYNTHESIS_CALL_STATE, make_inputs, state_cpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def device_case(dev, case, precision=None):
    """One forward + one call of the op and the float64 reference on the device's depths (computed once, left unchanged)."""
    from hfa_gp_amd import ops
    cs = N.case(*case)
    cfg = cs["cfg"]
    pl, state, args = forward_state(cs, dev, precision)
    depths = state_depths(state, cfg.depth_resolution + cfg.depth_resolution_importance)
    _, _, g_hat, mask = G.masked_case(*case, depths=depths)
    g_dev = g_hat.float().to(dev)
    d_m, d_k, rg = ops.raymarch_normals_bwd_camera(g_dev, pl, state, **args)
    dc, dx = NC.reference(cs["P"], cfg, cs["planes"], cs["c"], depths, g_hat)
    return dict(cs=cs, pl=pl, state=state, args=args, g_hat=g_dev, d_c=torch.cat((d_m, d_k), 1), ray_grad=rg, ref_c=dc,
                ref_rg=NC.ray_records(dx, depths), mask=mask, depths=depths)


def tolerance_factor(case):
    return max(1.0, 4.0 * NC.oracle_rho(*case))


def _check_case(dc, factor, what):
    r_rg = G.bar_ratio(dc["ray_grad"], dc["ref_rg"])
    r_m = G.bar_ratio(dc["d_c"][:, :16], dc["ref_c"][:, :16])
    r_k = G.bar_ratio(dc["d_c"][:, 16:], dc["ref_c"][:, 16:])
    print(f"{what}: ray_grad {r_rg:.3f}, d_cam2world {r_m:.3f}, d_intrinsics {r_k:.3f} (allowed {factor:.2f}); ref max |d c| "
          f"{float(dc['ref_c'].abs().max()):.3e}, {int(dc['mask'].sum())} of {dc['mask'].numel()} rays kept")
    assert float(dc["ref_c"].abs().max()) > 1e-3
    assert bool((dc["d_c"][:, NC.ZERO_COLUMNS] == 0).all())
    assert max(r_rg, r_m, r_k) <= factor, f"{what}: worst err / bar {max(r_rg, r_m, r_k):.3f} > {factor:.2f}"


# ----------------------------------------------------------------------------- 1. the op against float64
@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_op_vs_float64_reference(dev, preset, axes, hw, box_warp):
    """16+16, 32+32, 48+48 samples; both axis conventions; planes that are not square; points outside the box; 100 rays per frame,
    B = 2.  The default decoder precision (split 16-bit)."""
    case = (preset, axes, hw, box_warp)
    _check_case(device_case(dev, case), tolerance_factor(case), f"{N.CASE_IDS[N.CASES.index(case)]}: device")


@pytest.mark.parametrize("preset,axes,hw,box_warp", [N.CASES[0], N.CASES[5], N.CASES[2]],
                         ids=[N.CASE_IDS[0], N.CASE_IDS[5], N.CASE_IDS[2]])
def test_op_fp32_decoder_vs_float64_reference(dev, preset, axes, hw, box_warp):
    """One case per sample count with decoder_precision='fp32' (the exact fp32 matrix instructions throughout)."""
    case = (preset, axes, hw, box_warp)
    _check_case(device_case(dev, case, "fp32"), tolerance_factor(case), f"{N.CASE_IDS[N.CASES.index(case)]}: device, fp32 decoder")


# ----------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_two_calls_give_the_same_bits(dev, precision):
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[2], None if precision == "f16x3" else "fp32")
    d_m, d_k, rg = ops.raymarch_normals_bwd_camera(dc["g_hat"], dc["pl"], dc["state"], **dc["args"])
    assert torch.equal(_bits(rg), _bits(dc["ray_grad"]))
    assert torch.equal(_bits(torch.cat((d_m, d_k), 1)), _bits(dc["d_c"]))


# ----------------------------------------------------------------------------- 3. accumulation
def test_op_accumulates_into_ray_grad(dev):
    """A pre-filled ray_grad comes back as pre-fill + fresh (one fp32 add per float: the bar with its atol scaled by the summed
    magnitudes); with the reduction, the label gradient is the float64 ray_setup adjoint of the returned records, at the bar."""
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[5])
    pre = torch.randn(dc["ray_grad"].shape, generator=torch.Generator().manual_seed(31)).to(dev)
    acc = pre.clone()
    d_m, d_k, out = ops.raymarch_normals_bwd_camera(dc["g_hat"], dc["pl"], dc["state"], ray_grad=acc, **dc["args"])
    assert out is acc
    fresh = dc["ray_grad"]
    err = (out - pre - fresh).abs()
    bound = 2e-5 * max(1.0, float(pre.abs().max() + fresh.abs().max())) + 1e-3 * fresh.abs()
    print(f"ray_grad: worst err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    want = CR.ray_setup_adjoint(dc["cs"]["c"].double(), dc["cs"]["cfg"].neural_rendering_resolution, out.double().cpu())
    ratio = G.bar_ratio(torch.cat((d_m, d_k), 1), want)
    print(f"reduction of the accumulated records: worst err / bar {ratio:.3f}")
    assert ratio <= 1.0
    none_m, none_k, rg = ops.raymarch_normals_bwd_camera(dc["g_hat"], dc["pl"], dc["state"], reduce=False, **dc["args"])
    assert none_m is None and none_k is None and torch.equal(_bits(rg), _bits(fresh))


# ----------------------------------------------------------------------------- 4. zero upstream
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_zero_upstream(dev, precision):
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[1], None if precision == "f16x3" else "fp32")
    zero = torch.zeros_like(dc["g_hat"])
    d_m, d_k, rg = ops.raymarch_normals_bwd_camera(zero, dc["pl"], dc["state"], **dc["args"])
    assert bool((_bits(rg) == 0).all()) and bool((d_m == 0).all()) and bool((d_k == 0).all())
    pre = torch.randn(rg.shape, generator=torch.Generator().manual_seed(32)).to(dev)
    pre[0, 0, :4] = -0.0
    acc = pre.clone()
    ops.raymarch_normals_bwd_camera(zero, dc["pl"], dc["state"], ray_grad=acc, reduce=False, **dc["args"])
    assert torch.equal(_bits(acc), _bits(pre))
    # a ray with a zero upstream among live ones: its record is zeros, the others are what the full call gave them
    part = dc["g_hat"].clone()
    part[:, ::3] = 0
    _, _, rg_part = ops.raymarch_normals_bwd_camera(part, dc["pl"], dc["state"], reduce=False, **dc["args"])
    assert bool((_bits(rg_part[:, ::3]) == 0).all())
    keep = torch.ones(rg.shape[1], dtype=torch.bool)
    keep[::3] = False
    assert torch.equal(_bits(rg_part[:, keep]), _bits(dc["ray_grad"][:, keep]))


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_camera_looking_away_gives_exact_zeros(dev, precision):
    from hfa_gp_amd import ops
    cs = N.case(*N.CASES[0])
    c = cs["c"].clone()
    m = c[:, :16].view(-1, 4, 4)
    m[:, :3, 0] *= -1                             # half a turn about the camera's up axis: every ray leaves the box behind
    m[:, :3, 2] *= -1
    pl, state, args = forward_state(cs, dev, precision, c=c)
    d_m, d_k, rg = ops.raymarch_normals_bwd_camera(G.upstream(cs).float().to(dev), pl, state, **args)
    assert bool((rg == 0).all()) and bool((d_m == 0).all()) and bool((d_k == 0).all())


# ----------------------------------------------------------------------------- 5. skew
def test_reduction_with_skew(dev):
    """A label with skew, cx != cy and fx != fy: the op's records against float64 on that label, and its reduction against the
    float64 adjoint of the oracle's ray sampler applied to the returned records."""
    from hfa_gp_amd import ops
    from oracle import eg3d_oracle as O
    case = N.CASES[0]
    cs = N.case(*case)
    cfg = cs["cfg"]
    c = cs["c"].detach().clone()
    c[:, 16], c[:, 17], c[:, 18], c[:, 21] = torch.tensor([4.1, 4.4]), torch.tensor([0.07, -0.11]), torch.tensor([0.47, 0.52]), \
        torch.tensor([0.55, 0.44])
    pl, state, args = forward_state(cs, dev, c=c)
    depths = state_depths(state, cfg.depth_resolution + cfg.depth_resolution_importance)
    mask = G.edge_mask(cfg, case[2], c, depths)
    assert float(mask.double().mean()) >= G.MIN_KEPT
    g_hat = G.upstream(cs) * mask[..., None]
    d_m, d_k, rg = ops.raymarch_normals_bwd_camera(g_hat.float().to(dev), pl, state, **args)
    dc, dx = NC.reference(cs["P"], cfg, cs["planes"], c, depths, g_hat)
    dc32, dx32 = NC.reference(cs["P"], cfg, cs["planes"], c, depths, g_hat, dtype=torch.float32)
    factor = max(1.0, 4.0 * max(G.bar_ratio(dx32, dx), G.bar_ratio(dc32, dc)))
    got = torch.cat((d_m, d_k), 1)
    r_rg, r_c = G.bar_ratio(rg, NC.ray_records(dx, depths)), G.bar_ratio(got, dc)
    c64 = c.double().requires_grad_(True)
    o, d = O.ray_sampler(c64[:, :16].reshape(-1, 4, 4), c64[:, 16:].reshape(-1, 3, 3), cfg.neural_rendering_resolution)
    rg64 = rg.cpu().double()
    want, = torch.autograd.grad((o, d), c64, (rg64[..., :3], rg64[..., 3:]))
    r_red = G.bar_ratio(got, want)
    print(f"skew: ray_grad {r_rg:.3f}, d c {r_c:.3f} (allowed {factor:.2f}); reduction of the device's records {r_red:.3f} (allowed 1)")
    assert bool((dc[:, CR.NONZERO_COLUMNS] != 0).all()) and bool((got[:, NC.ZERO_COLUMNS] == 0).all())
    assert r_rg <= factor and r_c <= factor and r_red <= 1.0


# ----------------------------------------------------------------------------- 6. argument checks
def test_op_argument_checks(dev):
    from hfa_gp_amd import ops
    dc = device_case(dev, N.CASES[0])
    with pytest.raises(RuntimeError, match="raymarch_normals_bwd_camera: state must be"):
        ops.raymarch_normals_bwd_camera(dc["g_hat"], dc["pl"], None, **dc["args"])
    with pytest.raises(RuntimeError, match="raymarch_normals_bwd_camera: g_normal must be"):
        ops.raymarch_normals_bwd_camera(dc["g_hat"][:, :7].contiguous(), dc["pl"], dc["state"], **dc["args"])
    with pytest.raises(RuntimeError, match="raymarch_normals_bwd_camera: ray_grad must be"):
        ops.raymarch_normals_bwd_camera(dc["g_hat"], dc["pl"], dc["state"], ray_grad=dc["ray_grad"][:, :9].contiguous(), **dc["args"])


# ----------------------------------------------------------------------------- 7 - 10. synthesis(normal_camera_grad=True)
def _step(gen, dev, image=False, normal=True, c_grad=True, t_nrm=None, replay=None, record=None, **kw):
    """One differentiable step of tiny64 at 10 x 10 rays -> (out, ws, c, the ray marcher's state of the call).

    `record` (a dict) receives what the two calls of the backward that sum with atomics were handed and what they left:
    ops.raymarch_bwd (pass 2 fills its bins in the arrival order of an atomic cursor) and ops.raymarch_normals_bwd (its plane
    scatter).  Everything else of the backward is deterministic.  With `replay` (the record of an earlier step) both calls must be
    handed bit-identical tensors, still run their kernels, and the step continues from the RECORDED results: its `d ws` is then
    comparable with `torch.equal` (the mechanism of tests/test_gpu_normals.py)."""
    from hfa_gp_amd import ops
    cfg = _cfg()
    ws, c, us, ui = _inputs(dev)
    ws.requires_grad_(True)
    c.requires_grad_(c_grad)
    states, inner = [], ops.raymarch

    def recording(*a, **k):
        states.append(k.get("state"))
        return inner(*a, **k)

    ops.raymarch = recording
    try:
        out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, return_planes=True, **kw)
    finally:
        ops.raymarch = inner
    loss = 0
    if image:
        loss = loss + (out["image"] * _target((B, 3, cfg.img_resolution, cfg.img_resolution), 6, dev) / cfg.img_resolution).sum()
    if normal:
        loss = loss + (out["image_normal"] * t_nrm).sum()
    rec = {} if record is None else record
    inner_rb, inner_nb = ops.raymarch_bwd, ops.raymarch_normals_bwd

    def same(handed, want, who):
        assert set(handed) == set(want)
        for name, t in handed.items():
            assert torch.equal(t, want[name]), f"{who} was handed another {name}"

    def rb(g_feat, planes, *a, **k):
        handed = dict(g_feat=g_feat.clone(), planes=planes.clone(), state=k["state"].clone(), u_strat=k["u_strat"].clone(),
                      u_imp=k["u_imp"].clone(), cam2world=k["cam2world"].clone(), intrinsics=k["intrinsics"].clone())
        result = inner_rb(g_feat, planes, *a, **k)                 # (with c.requires_grad it also fills rec_out for the camera pass)
        assert isinstance(result, torch.Tensor), "the generator is frozen: d_planes alone"
        rec["rb"] = dict(handed=handed, result=result.clone())
        if replay is None:
            return result
        same(handed, replay["rb"]["handed"], "ops.raymarch_bwd")
        return replay["rb"]["result"].clone()

    def nb(g_normal, planes, state, **k):
        handed = dict(g_normal=g_normal.clone(), planes=planes.clone(), state=state.clone(), d_planes=k["d_planes"].clone())
        if replay is None:
            result = inner_nb(g_normal, planes, state, **k)
            rec["nb"] = dict(handed=handed, after=result[0].clone())
            return result
        same(handed, replay["nb"]["handed"], "ops.raymarch_normals_bwd")
        own = inner_nb(g_normal, planes, state, **dict(k, d_planes=k["d_planes"].clone()))
        rec["nb"] = dict(handed=handed, after=own[0].clone())
        k["d_planes"].copy_(replay["nb"]["after"])
        return k["d_planes"], own[1]

    if record is not None or replay is not None:
        ops.raymarch_bwd, ops.raymarch_normals_bwd = rb, nb
    try:
        loss.backward()
    finally:
        ops.raymarch_bwd, ops.raymarch_normals_bwd = inner_rb, inner_nb
    return out, ws, c, states[0]


def _masked_target(dev, state):
    """T * edge mask [B,R,3] float64 (CPU) for the depths in `state`, and the same as the NCHW device tensor the loss multiplies."""
    cfg = _cfg()
    r = cfg.neural_rendering_resolution
    depths = state_depths(state, cfg.depth_resolution + cfg.depth_resolution_importance)
    mask = G.edge_mask(cfg, (cfg.plane_resolution, cfg.plane_resolution), make_inputs(cfg, B)[1], depths)
    assert float(mask.double().mean()) >= G.MIN_KEPT
    g_hat = torch.randn(B, r * r, 3, generator=torch.Generator().manual_seed(23), dtype=torch.float64) * mask[..., None]
    return depths, g_hat, g_hat.float().reshape(B, r, r, 3).permute(0, 3, 1, 2).contiguous().to(dev)


@functools.lru_cache(maxsize=None)
def _probe_state(dev):
    """The state of the forward (bit-reproducible: the same depths in every step of these inputs)."""
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    states, inner = [], ops.raymarch

    def recording(*a, **k):
        states.append(k.get("state"))
        return inner(*a, **k)

    ops.raymarch = recording
    try:
        gen.synthesis(ws.requires_grad_(True), c, noise_mode="const", u_strat=us, u_imp=ui, normal_grad=True)
    finally:
        ops.raymarch = inner
    return states[0]


def test_synthesis_normals_only_loss(dev):
    """c.grad of a loss on image_normal alone = the op called by hand on the call's planes and state, bit for bit (the photometric
    records it is added to are zeros), and within test 1's tolerance of the float64 reference on those planes."""
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    depths, g_hat, t_nrm = _masked_target(dev, _probe_state(dev))
    out, ws, c, state = _step(gen, dev, t_nrm=t_nrm, normal_camera_grad=True)
    assert out["image_normal"].requires_grad and c.grad is not None and ws.grad is not None
    assert torch.equal(state_depths(state, depths.shape[2]), depths), "the forward is bit-reproducible"
    _, c_in, us, ui = _inputs(dev)
    u_s, u_i = gen._uniforms(B, dev, us, ui)
    d_m, d_k, _ = ops.raymarch_normals_bwd_camera(g_hat.float().to(dev), out["planes"], state, u_strat=u_s, u_imp=u_i,
                                                  planes_absmax=getattr(gen, "_planes_absmax", None), **gen._render_args(c_in))
    by_hand = torch.cat((d_m, d_k), 1)
    assert float(by_hand.abs().max()) > 0
    assert torch.equal(_bits(c.grad), _bits(by_hand))
    P = state_cpu(_gen_cpu())
    planes = out["planes"].detach().permute(0, 1, 4, 2, 3).cpu()
    c_cpu = make_inputs(cfg, B)[1]
    dc, dx = NC.reference(P, cfg, planes, c_cpu, depths, g_hat)
    dc32, dx32 = NC.reference(P, cfg, planes, c_cpu, depths, g_hat, dtype=torch.float32)
    factor = max(1.0, 4.0 * max(G.bar_ratio(dx32, dx), G.bar_ratio(dc32, dc)))
    ratio = G.bar_ratio(c.grad, dc)
    print(f"c.grad of a normals-only loss: worst err / bar {ratio:.3f} (allowed {factor:.2f}), max |ref| {float(dc.abs().max()):.3e}")
    assert float(dc.abs().max()) > 1e-3 and ratio <= factor
    assert bool((c.grad[:, NC.ZERO_COLUMNS] == 0).all())


def test_synthesis_image_and_normal_loss(dev):
    """c.grad of the joint loss = photometric-only c.grad + normals-only c.grad at the bar.  d ws does not depend on asking for
    c.grad: the step with c.requires_grad hands ops.raymarch_bwd and ops.raymarch_normals_bwd (the two calls of the backward that
    sum in the arrival order of atomics) bit-identical tensors to the step with c detached, and continued from that step's results
    its d ws is `torch.equal` to it.  Each call's own result in the two steps agrees at the gradient bar.  Printed, not asserted:
    the spread of d ws between two c-detached steps (the run-to-run level of a step with `normal_grad`) and between the steps with
    and without c.grad, both without replay."""
    gen = _gen(dev)
    _, _, t_nrm = _masked_target(dev, _probe_state(dev))
    _, ws_both, c_both, _ = _step(gen, dev, image=True, t_nrm=t_nrm, normal_camera_grad=True)
    _, _, c_img, _ = _step(gen, dev, image=True, normal=False)
    _, _, c_nrm, _ = _step(gen, dev, t_nrm=t_nrm, normal_camera_grad=True)
    assert float(c_img.grad.abs().max()) > 0 and float(c_nrm.grad.abs().max()) > 0
    ratio = G.bar_ratio(c_both.grad, (c_img.grad + c_nrm.grad).double())
    print(f"c.grad of the joint loss against the sum of its parts: worst err / bar {ratio:.3f}")
    assert ratio <= 1.0
    det, rep = {}, {}
    _, ws_det, c_det, _ = _step(gen, dev, image=True, c_grad=False, t_nrm=t_nrm, record=det, normal_camera_grad=True)
    assert c_det.grad is None and set(det) == {"rb", "nb"}
    _, ws_rep, c_rep, _ = _step(gen, dev, image=True, t_nrm=t_nrm, replay=det, record=rep, normal_camera_grad=True)
    assert c_rep.grad is not None and float(ws_det.grad.abs().max()) > 0
    assert torch.equal(ws_rep.grad, ws_det.grad), f"d ws max diff {float((ws_rep.grad - ws_det.grad).abs().max()):.3e}"
    assert torch.equal(_bits(c_rep.grad), _bits(c_both.grad)), "the camera passes are deterministic"
    r_rb = G.bar_ratio(rep["rb"]["result"], det["rb"]["result"])
    r_nb = G.bar_ratio(rep["nb"]["after"], det["nb"]["after"])
    print(f"own results of the two steps: raymarch_bwd d_planes {r_rb:.4f}, after raymarch_normals_bwd {r_nb:.4f} of the bar")
    assert r_rb <= 1.0 and r_nb <= 1.0
    _, ws_det2, _, _ = _step(gen, dev, image=True, c_grad=False, t_nrm=t_nrm, normal_camera_grad=True)
    top = float(ws_det.grad.abs().max())
    print(f"d ws, no replay: two c-detached steps differ by {float((ws_det2.grad - ws_det.grad).abs().max()) / top:.2e} of max |d ws|; "
          f"with against without c.grad {float((ws_both.grad - ws_det.grad).abs().max()) / top:.2e}")


def test_refusal_and_silence(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    with torch.no_grad():
        before = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
    with pytest.raises(NotImplementedError, match="camera gradient of the normal term.*normal_camera_grad"):
        gen.synthesis(ws.clone().requires_grad_(True), c.clone().requires_grad_(True), noise_mode="const", u_strat=us, u_imp=ui,
                      normal_grad=True)
    calls, inner = [], ops.raymarch_normals_bwd_camera
    monkeypatch.setattr(ops, "raymarch_normals_bwd_camera", lambda *a, **k: calls.append(1) or inner(*a, **k))
    _, _, t_nrm = _masked_target(dev, _probe_state(dev))
    out, _, c1, _ = _step(gen, dev, image=True, normal=False, normal_camera_grad=True)      # the loss ignores image_normal
    assert out["image_normal"].requires_grad and c1.grad is not None and calls == []
    _, _, c2, _ = _step(gen, dev, image=True, normal=False)
    assert torch.equal(_bits(c1.grad), _bits(c2.grad)), "raymarch_bwd_camera is deterministic: the same label gradient"
    _step(gen, dev, image=True, c_grad=False, t_nrm=t_nrm, normal_camera_grad=True)         # the label is detached
    assert calls == []
    _step(gen, dev, image=True, t_nrm=t_nrm, normal_camera_grad=True, geometry=True)
    assert calls == [1]
    assert not SYNTHESIS_CALL_STATE & set(vars(gen))          # (the request lives in the call's record, not on the module)
    with torch.no_grad():
        plain = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui)
    assert list(plain) == ["image", "image_raw", "image_depth"]
    for k in plain:
        assert torch.equal(plain[k], before[k]), k


def test_get_image_with_non_leaf_label(dev):
    """label = base + delta (non-leaf) through get_image(normal_camera_grad=True): delta.grad is the generator-level c.grad with the
    flipped columns negated (the in-place flip is an autograd-tracked mul_)."""
    from hfa_gp_amd import headnerf
    from tests.util import look_at_label

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
    out = m.get_image(latent, base + delta, normal_camera_grad=True, u_strat=us, u_imp=ui)
    assert isinstance(out, dict) and out["image_normal"].requires_grad
    out["image_normal"].square().sum().backward()
    c = (base + delta.detach()).clone()
    c[:, FLIP_COLUMNS] *= -1
    c.requires_grad_(True)
    m.generator.synthesis(latent, c, noise_mode="const", u_strat=us, u_imp=ui, normal_camera_grad=True)["image_normal"] \
        .square().sum().backward()
    want = c.grad.clone()
    want[:, FLIP_COLUMNS] *= -1
    assert bool(want.abs().max() > 0)
    assert torch.equal(_bits(delta.grad), _bits(want))
