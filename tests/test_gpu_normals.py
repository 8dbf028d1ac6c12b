"""The per-ray surface normals on the device (hfagp_raymarch_normals, ops.raymarch_normals, synthesis(normals=True)) against the
float64 reference of tests/normals_ref.py.  Needs an MI355X:  python -m pytest tests -m gpu

The normal of a sample is the positional derivative of a bilinear gather, which is discontinuous at texel edges: a sample whose
pixel coordinate rounds across an edge on one side only changes its ray discontinuously.  The per-ray comparisons therefore allow
4 of 200 rays beyond the bar (tests/test_gpu_camera_grad.py's cap; the fp32 oracle alone needs at most 1:
tests/test_normals_cpu.py::test_fp32_oracle_edge_rays), print the count and require every ray to be finite."""
import functools

import pytest
import torch

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


def device_call(cs, dev, precision=None, c=None):
    """ops.raymarch (leaves the state) then ops.raymarch_normals -> (normal [B,R,3], wsum [B,R])."""
    from hfa_gp_amd import ops
    gen = cs["gen"].to(dev)
    b, cfg = cs["b"], cs["cfg"]
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = gen._render_args((cs["c"] if c is None else c).to(dev))
    if precision is not None:
        args["decoder_precision"] = precision
    state = ops.raymarch_state(b, cfg.neural_rendering_resolution, cfg.depth_resolution, cfg.depth_resolution_importance, dev)
    _, _, wsum, _ = ops.raymarch(pl, u_strat=u_s, u_imp=u_i, state=state, **args)
    normal = ops.raymarch_normals(pl, state, u_strat=u_s, u_imp=u_i, **args)
    assert normal.shape == (b, cs["r"], 3) and not normal.requires_grad
    return normal, wsum


@pytest.mark.parametrize("preset,axes,hw,box_warp", N.CASES, ids=N.CASE_IDS)
def test_normals_vs_float64_reference(dev, preset, axes, hw, box_warp):
    """16+16, 32+32, 48+48 samples; both axis conventions; planes that are not square either way; points outside the box."""
    cs = N.case(preset, axes, hw, box_warp)
    ref = N.case_reference(preset, axes, hw, box_warp)
    normal, _ = device_call(cs, dev)
    bad = N.rays_beyond(normal, ref["normal"], f"{preset}/{axes}/{hw}/{box_warp}")
    assert bad <= N.MAX_EDGE_RAYS, f"{bad} rays beyond the bar"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_normals_decoder_precisions_small128(dev, precision):
    cs = N.case("small128")
    normal, _ = device_call(cs, dev, precision=precision)
    bad = N.rays_beyond(normal, N.case_reference("small128")["normal"], f"small128/{precision}")
    assert bad <= N.MAX_EDGE_RAYS, f"{bad} rays beyond the bar"


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_rays_that_miss_the_box_are_exact_zeros(dev, precision):
    cs = N.case("tiny64")
    c = cs["c"].clone()
    m = c[:, :16].view(-1, 4, 4)
    m[:, :3, 0] *= -1                             # half a turn about the camera's up axis: every ray leaves the box behind
    m[:, :3, 2] *= -1
    normal, _ = device_call(cs, dev, precision=precision, c=c)
    assert bool((normal.view(torch.int32) == 0).all())


@pytest.mark.parametrize("preset,axes,hw,box_warp", [N.CASES[0], N.CASES[2], N.CASES[6]], ids=["tiny64", "ffhq512_128", "40x72-0.45"])
def test_norm_bounded_by_opacity_and_two_calls_equal(dev, preset, axes, hw, box_warp):
    cs = N.case(preset, axes, hw, box_warp)
    normal, wsum = device_call(cs, dev)
    assert bool((normal.norm(dim=-1) <= wsum + 1e-6).all())
    assert float(normal.norm(dim=-1).max()) > 0.05
    again, _ = device_call(cs, dev)
    assert torch.equal(normal, again)


def test_op_argument_checks(dev):
    from hfa_gp_amd import ops
    cs = N.case("tiny64")
    gen = cs["gen"].to(dev)
    b, cfg = cs["b"], cs["cfg"]
    pl = cs["planes"].permute(0, 1, 3, 4, 2).contiguous().to(dev)
    u_s, u_i = gen._uniforms(b, dev, cs["us"].to(dev), cs["ui"].to(dev))
    args = gen._render_args(cs["c"].to(dev))
    with pytest.raises(RuntimeError, match="raymarch_normals: state must be"):
        ops.raymarch_normals(pl, torch.zeros(b, cs["r"], 7, device=dev), u_strat=u_s, u_imp=u_i, **args)
    e_args = dict(args, cam2world=args["cam2world"][:0], intrinsics=args["intrinsics"][:0])
    empty = ops.raymarch_normals(pl[:0], torch.zeros(0, cs["r"], 32 * 35, device=dev), u_strat=u_s[:0], u_imp=u_i[:0], **e_args)
    assert empty.shape == (0, cs["r"], 3)


# ----------------------------------------------------------------------------- synthesis(normals=True): tiny64's own size, B = 3
B = 3


def _cfg():
    from hfa_gp_amd.config import PRESETS
    return PRESETS["tiny64"]()


@functools.lru_cache(maxsize=None)
def _gen_cpu():
    from hfa_gp_amd.generator import TriPlaneGenerator
    return perturb_state(TriPlaneGenerator(_cfg(), seed=0)).requires_grad_(False)


def _gen(dev):
    return _gen_cpu().to(dev)


def _inputs(dev):
    return tuple(t.to(dev) for t in make_inputs(_cfg(), B))


def _call(gen, dev, **kw):
    ws, c, us, ui = _inputs(dev)
    return gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, **kw)


@functools.lru_cache(maxsize=None)
def _plain(dev):
    """The call without `normals` under no_grad (computed once and left unchanged)."""
    with torch.no_grad():
        return _call(_gen(dev), dev)


def _same_images(out, ref):
    for k in ("image", "image_raw", "image_depth"):
        assert torch.equal(out[k], ref[k]), k


def test_synthesis_normals_match_reference_on_own_planes(dev):
    """256 rays per frame (the strip order of the ray schedule; the res-10 cases take the row order).  At most 4 of the call's 768
    rays beyond the bar: the kernel tests' count, not their rate — a localised error would show."""
    gen, cfg = _gen(dev), _cfg()
    with torch.no_grad():
        out = _call(gen, dev, normals=True, return_planes=True)
    r = cfg.neural_rendering_resolution
    assert set(out) == {"image", "image_raw", "image_depth", "image_normal", "planes", "feature_image"}
    assert out["image_normal"].shape == (B, 3, r, r) and not out["image_normal"].requires_grad
    _same_images(out, _plain(dev))
    _, c, us, ui = make_inputs(cfg, B)
    planes = out["planes"].cpu().permute(0, 1, 4, 2, 3).contiguous()              # [B,3,H,W,32] -> the oracle's [B,3,32,H,W]
    ref = N.reference(state_cpu(gen), cfg, planes, c, us, ui)
    got = out["image_normal"].permute(0, 2, 3, 1).reshape(B, r * r, 3)
    bad = N.rays_beyond(got, ref["normal"], "synthesis(normals=True)")
    assert bad <= N.MAX_EDGE_RAYS, f"{bad} rays beyond the bar"
    assert float(ref["normal"].norm(dim=-1).max()) > 0.05


def test_synthesis_normals_compose_under_no_grad(dev):
    gen = _gen(dev)
    coords = (torch.rand(1, 37, 3, generator=torch.Generator().manual_seed(2)) - 0.5).to(dev)
    with torch.no_grad():
        base = _call(gen, dev, normals=True)
        out = _call(gen, dev, normals=True, geometry=True, query=coords)
        want = _call(gen, dev, geometry=True, query=coords)
    assert set(out) == set(want) | {"image_normal"}
    for k in want:
        assert torch.equal(out[k], want[k]), k
    assert torch.equal(out["image_normal"], base["image_normal"])
    assert bool((out["image_normal"].norm(dim=1, keepdim=True) <= out["image_mask"] + 1e-6).all())
    _same_images(out, _plain(dev))


def _clone(x):
    if isinstance(x, torch.Tensor):
        return x.clone()
    if isinstance(x, (tuple, list)):
        return type(x)(_clone(v) for v in x)
    return x


def _step(gen, dev, replay=None, **kw):
    """One differentiable step with an image loss -> (outputs, d ws, record of the renderer's backward: what `ops.raymarch_bwd` was
    handed and what it returned).

    Two steps of this project do not give the same bits of `d ws`, with or without `normals`: pass 2 of the ray marcher's backward
    (sort + gather, raymarch_rows.hip) fills its bins in the arrival order of an atomic cursor, so the fp32 sums of a bin are taken
    in another order every run (measured on one MI355X on these inputs: two steps WITHOUT normals differ by 3.7e-9 = 4.5e-8 of
    max |d ws|).  Everything before and after that one call is deterministic.  So with `replay` (the record of an earlier step) this
    step's call must be handed bit-identical tensors — the image gradient that reaches it, planes, saved state, uniforms, camera —
    still runs the kernel, and then continues from the RECORDED result: its `d ws` is comparable with `torch.equal`."""
    from hfa_gp_amd import ops
    ws, c, us, ui = _inputs(dev)
    ws.requires_grad_(True)
    out = gen.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, **kw)
    target = torch.randn(out["image"].shape, generator=torch.Generator().manual_seed(6)).clamp(-1, 1).to(dev)
    records = []
    inner = ops.raymarch_bwd

    def recording(g_feat, planes, *a, **k):
        handed = dict(g_feat=g_feat.clone(), planes=planes.clone(), state=None if k.get("state") is None else k["state"].clone(),
                      u_strat=k["u_strat"].clone(), u_imp=k["u_imp"].clone(), cam2world=k["cam2world"].clone(),
                      intrinsics=k["intrinsics"].clone())
        result = inner(g_feat, planes, *a, **k)
        records.append(dict(handed=handed, result=_clone(result)))
        if replay is None:
            return result
        assert set(handed) == set(replay["handed"])
        for name, t in handed.items():
            want = replay["handed"][name]
            assert (t is None) == (want is None), name
            assert t is None or torch.equal(t, want), f"the renderer's backward was handed another {name}"
        return _clone(replay["result"])

    ops.raymarch_bwd = recording
    try:
        torch.nn.functional.mse_loss(out["image"], target).backward()
    finally:
        ops.raymarch_bwd = inner
    assert len(records) == 1
    return out, ws.grad, records[0]


def _same_backward(step, plain, what):
    """`d ws` of a step with `normals` that replayed `plain`'s renderer backward (`_step`) is `torch.equal` to `plain`'s: together
    with the bit-identical inputs of that call (asserted inside the replay) nothing of the backward depends on `normals`."""
    (_, d_ws, _), (_, d_ws_plain, _) = step, plain
    assert d_ws is not None and float(d_ws_plain.abs().max()) > 0 and bool(torch.isfinite(d_ws).all())
    assert torch.equal(d_ws, d_ws_plain), f"{what}: d ws max diff {float((d_ws - d_ws_plain).abs().max()):.3e}"


def test_synthesis_normals_in_a_differentiable_step(dev):
    gen = _gen(dev)
    with torch.no_grad():
        base = _call(gen, dev, normals=True)
    plain = _step(gen, dev)
    step = _step(gen, dev, replay=plain[2], normals=True)
    out = step[0]
    assert out["image"].requires_grad and not out["image_normal"].requires_grad
    assert torch.equal(out["image_normal"], base["image_normal"])
    _same_images(out, plain[0])
    _same_images(out, _plain(dev))
    assert step[2]["handed"]["state"] is not None, "the tape's ray_state is reused"
    _same_backward(step, plain, "differentiable step")
    coords = (torch.rand(B, 21, 3, generator=torch.Generator().manual_seed(3)) - 0.5).to(dev).requires_grad_(True)
    both = _step(gen, dev, normals=True, geometry=True, query=coords)[0]
    assert set(both) == {"image", "image_raw", "image_depth", "image_mask", "query_sigma", "query_rgb", "image_normal"}
    assert both["image_mask"].requires_grad and both["query_sigma"].requires_grad and not both["image_normal"].requires_grad
    assert torch.equal(both["image_normal"], base["image_normal"])


def test_chunked_path_equals_unchunked(dev, monkeypatch):
    """The cap on the ray marcher's state lowered to one frame: no_grad renders in one-frame chunks, and the differentiable step
    (whose tape then skips the state) does too."""
    from hfa_gp_amd import generator as G
    from hfa_gp_amd import ops
    gen, cfg = _gen(dev), _cfg()
    with torch.no_grad():
        base = _call(gen, dev, normals=True, geometry=True)
    frame = cfg.neural_rendering_resolution ** 2 * (cfg.depth_resolution + cfg.depth_resolution_importance) * 140
    monkeypatch.setattr(G, "RAY_STATE_CAP_BYTES", frame)
    calls = []
    inner = ops.raymarch_normals
    monkeypatch.setattr(ops, "raymarch_normals", lambda planes, *a, **k: calls.append(planes.shape[0]) or inner(planes, *a, **k))
    with torch.no_grad():
        out = _call(gen, dev, normals=True, geometry=True)
    assert calls == [1] * B
    for k in base:
        assert torch.equal(out[k], base[k]), k
    plain = _step(gen, dev)                       # (the plain step under the same cap)
    step = _step(gen, dev, replay=plain[2], normals=True)
    assert calls == [1] * (2 * B)
    assert step[2]["handed"]["state"] is None     # the tape skipped the state: the backward marches again
    _same_backward(step, plain, "chunked differentiable step")
    assert torch.equal(step[0]["image_normal"], base["image_normal"])
    _same_images(step[0], base)
    monkeypatch.setattr(G, "RAY_STATE_CAP_BYTES", 2 * frame)       # two frames, then the ragged last one
    with torch.no_grad():
        out = _call(gen, dev, normals=True, geometry=True)
    assert calls[2 * B:] == [2, 1]
    for k in base:
        assert torch.equal(out[k], base[k]), k


def test_empty_batch_has_the_key(dev):
    gen, cfg = _gen(dev), _cfg()
    ws, c, us, ui = _inputs(dev)
    out = gen.synthesis(ws[:0], c[:0], noise_mode="const", normals=True, geometry=True)
    r = cfg.neural_rendering_resolution
    assert out["image_normal"].shape == (0, 3, r, r) and out["image_mask"].shape == (0, 1, r, r)


def test_get_image_passes_normals_through(dev):
    """HeadNeRF_*.get_image / forward(..., normals=True) return the dict and keep the in-place label flip."""
    from hfa_gp_amd import headnerf

    class A:
        out_pose = False; person_2 = False; params_len = 76; generator_preset = "tiny14"; generator_seed = 0

    torch.manual_seed(0)
    m = headnerf.HeadNeRF_3DMM(A(), 64, dev, 512, 50).to(dev)
    cfg = m.generator.cfg
    _, c, us, ui = (t.to(dev) for t in make_inputs(cfg, 2))
    ws = m.get_latent(torch.randn(2, 50, device=dev)).detach()
    data = c.clone()
    data[:, FLIP_COLUMNS] *= -1                    # the label as the data set yields it: get_image flips it in place
    with torch.no_grad():
        label = data.clone()
        out = m.get_image(ws, label, normals=True, u_strat=us, u_imp=ui)
        assert torch.equal(label, c), "the label flip side effect is gone"
        img = m.get_image(ws, data.clone(), u_strat=us, u_imp=ui)
        want = m.generator.synthesis(ws, c, noise_mode="const", u_strat=us, u_imp=ui, normals=True)
        full = m.get_image(ws, data.clone(), normals=True, geometry=True, u_strat=us, u_imp=ui)
        label = data.clone()
        fwd = m(torch.randn(2, 76, device=dev), label, normals=True)
        assert torch.equal(label, c)
    r = cfg.neural_rendering_resolution
    assert isinstance(out, dict) and set(out) == {"image", "image_raw", "image_depth", "image_normal"}
    assert isinstance(img, torch.Tensor) and torch.equal(img, out["image"])
    assert torch.equal(out["image_normal"], want["image_normal"]) and float(out["image_normal"].abs().max()) > 0
    assert set(full) == set(out) | {"image_mask"} and torch.equal(full["image_normal"], out["image_normal"])
    assert isinstance(fwd, dict) and fwd["image_normal"].shape == (2, 3, r, r)


def test_no_normal_pass_without_normals(dev, monkeypatch):
    from hfa_gp_amd import ops
    gen = _gen(dev)

    def boom(*a, **k):
        raise AssertionError("raymarch_normals called although normals was not asked for")

    monkeypatch.setattr(ops, "raymarch_normals", boom)
    with torch.no_grad():
        out = _call(gen, dev, geometry=True)
    assert "image_normal" not in out
    _same_images(out, _plain(dev))
    assert "image_normal" not in _step(gen, dev)[0]
    with pytest.raises(AssertionError, match="raymarch_normals called"), torch.no_grad():
        _call(gen, dev, normals=True)
    assert not SYNTHESIS_CALL_STATE & set(vars(gen))          # (the request lives in the call's record, not on the module)
    with torch.no_grad():
        after = _call(gen, dev)
    assert list(after) == ["image", "image_raw", "image_depth"]
    _same_images(after, _plain(dev))
