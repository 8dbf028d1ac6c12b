"""Occupancy grids on the device: ops.occupancy_pack (hfagp_occupancy_pack) against its torch reference, ops.ray_limits_grid
(hfagp_ray_limits_grid) against the brute-force float64 reference cam_utils.ray_limits_grid, TriPlaneGenerator.occupancy_grid, and
render_rays(ray_limits=occ, compact=) against the explicit-limits path it is built on.

Tolerance of the limits: tests/occupancy_ref.atol_gpu(G) = 4 x the float32 reference's own largest deviation from float64 at that G
(tests/test_occupancy_cpu.py measures and pins it).  Grazing rays — an occupied cell with a chord below 1e-3 of a cell — are left
out of the comparison and capped at 2 % of a list."""
import functools
import math

import pytest
import torch

from tests import occupancy_ref as OR
from tests import test_gpu_render_rays as TR
from tests.test_gpu_camera_grad import check_rays
from tests.test_gpu_geometry_grad import close
from tests.util import look_at_label, make_inputs, perturb_state

pytestmark = pytest.mark.gpu

INF = float("inf")
RES = 12                    # 144 rays per frame: two full waves and a partial one
G_RENDER = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- 1. the pack kernel
@pytest.mark.parametrize("g,k,dilate", [(8, 1, 0), (8, 2, 1), (40, 2, 1), (33, 1, 2)])
def test_occupancy_pack_vs_reference(dev, g, k, dilate):
    from hfa_gp_amd import ops
    from hfa_gp_amd.occupancy import OccupancyGrid, occupancy_reference
    gen = torch.Generator().manual_seed(11)
    n = g * k + 1
    vol = torch.randn(2, n, n, n, generator=gen)
    vol[1, n // 2, k, n - 1] = float("nan")
    level = 2.0 if dilate < 2 else 3.0               # inside the data's range: 2 % / 0.1 % of the points reach it
    want = occupancy_reference(vol, g, k, level, dilate)
    assert 0 < int(want.sum()) < want.numel()
    bits = ops.occupancy_pack(vol.to(dev), g, k, level, dilate)
    assert bits.dtype == torch.int32 and bits.shape == (2, g, g, (g + 31) // 32)
    assert torch.equal(OccupancyGrid(bits, g, 1.0).dense().cpu(), want)
    assert torch.equal(bits.cpu(), OccupancyGrid.from_dense(want, 1.0).bits)          # the padding bits too
    assert torch.equal(ops.occupancy_pack(vol.to(dev), g, k, level, dilate), bits)   # no atomics: the same bits again
    lo, hi = torch.full((1, n, n, n), -1.0, device=dev), torch.full((1, n, n, n), 1.0, device=dev)
    assert not bool(ops.occupancy_pack(lo, g, k, 0.0, dilate).any())
    assert bool(OccupancyGrid(ops.occupancy_pack(hi, g, k, 0.0, dilate), g, 1.0).dense().all())


# ----------------------------------------------------------------------------- 2. the ray kernel
@functools.lru_cache(maxsize=None)
def limits_case(g):
    """B = 2 masks, R = 1000 rays per frame (990 of the recipe + 10 special rows), the float64 and float32 references and the
    grazing rays — computed once."""
    from hfa_gp_amd.cam_utils import ray_limits_grid
    dense = OR.random_mask(g, seed=300 + g, b=2)
    o, d = OR.recipe_rays(990, seed=400 + g, b=2)
    so, sd = OR.special_rays(g, dense)
    so = so.expand(2, -1, -1).clone()
    so[1, -2:] = (dense[1].nonzero()[0].double() + 0.5) / g - 0.5      # frame 1: the centre of one of ITS occupied cells
    o, d = torch.cat((o, so.float().double()), 1), torch.cat((d, sd.expand(2, -1, -1)), 1)
    ref = ray_limits_grid(o, d, dense, OR.CUBE)
    ref32 = ray_limits_grid(o.float(), d.float(), dense, OR.CUBE)
    return dense, o, d, ref, ref32, OR.grazing(o, d, dense)


def check_limits(tn, tf, ref, graz, atol, what):
    tn, tf = tn.cpu(), tf.cpu()
    hit, want = torch.isfinite(tn), torch.isfinite(ref[0])
    share = graz.float().mean().item()
    both = hit & want & ~graz
    dev_n, dev_f = (tn.double() - ref[0])[both].abs().max().item(), (tf.double() - ref[1])[both].abs().max().item()
    print(f"{what}: {int(want.sum())} of {want.numel()} rays hit, grazing {100 * share:.2f} %, max |d t_near| {dev_n:.3e}, "
          f"|d t_far| {dev_f:.3e} (atol {atol:.2e})")
    assert share <= OR.GRAZING_CAP
    assert bool(((tn == INF) & (tf == -INF))[~hit].all()) and bool(torch.isfinite(tf[hit]).all())     # finite, or exactly (+inf, -inf)
    assert torch.equal(hit[~graz], want[~graz]), f"{what}: hit / miss differs on {int((hit != want)[~graz].sum())} rays"
    assert dev_n <= atol and dev_f <= atol


@pytest.mark.parametrize("g", [8, 40])
def test_ray_limits_grid_vs_float64_twin(dev, g):
    from hfa_gp_amd import ops
    from hfa_gp_amd.occupancy import OccupancyGrid
    dense, o, d, ref, ref32, graz = limits_case(g)
    assert o.shape == (2, 1000, 3) and not torch.equal(dense[0], dense[1])
    od, dd = o.float().to(dev), d.float().to(dev)
    tn, tf = ops.ray_limits_grid(od, dd, OccupancyGrid.from_dense(dense.to(dev), OR.CUBE))
    assert tn.shape == (2, 1000) and tn.dtype == torch.float32
    check_limits(tn, tf, ref, graz, OR.atol_gpu(g), f"G = {g}")
    # the special rows: the misses and the zero direction are empty, an origin in an occupied cell starts at 0
    assert bool((tn[:, -6:-2] == INF).all()) and bool((tf[:, -6:-2] == -INF).all()) and bool((tn[:, -2:] == 0).all())
    # every reported t is the float32 formula on a plane index, so the float32 reference is met exactly — grazing rays included
    diff = int((tn.cpu() != ref32[0]).sum() + (tf.cpu() != ref32[1]).sum())
    print(f"G = {g}: {diff} limits differ from the float32 reference")
    assert diff == 0
    # one grid for both frames
    one = OccupancyGrid.from_dense(dense[1:].to(dev), OR.CUBE)
    bn, bf = ops.ray_limits_grid(od, dd, one)
    assert torch.equal(bn[1], tn[1]) and torch.equal(bf[1], tf[1])
    sn, sf = ops.ray_limits_grid(od[:1].contiguous(), dd[:1].contiguous(), one)
    assert torch.equal(bn[0], sn[0]) and torch.equal(bf[0], sf[0])


def test_all_ones_grid_is_the_box(dev):
    from hfa_gp_amd import cam_utils, ops
    from hfa_gp_amd.occupancy import OccupancyGrid
    g = 8
    _, o, d, _, _, _ = limits_case(g)
    od, dd = o.float().to(dev), d.float().to(dev)
    occ = OccupancyGrid.from_dense(torch.ones(1, g, g, g, dtype=torch.bool, device=dev), OR.CUBE)
    tn, tf = ops.ray_limits_grid(od, dd, occ)
    bn, bf = ops.ray_limits_box(od, dd, OR.CUBE)
    valid = cam_utils.ray_limits_valid(bn, bf)
    assert torch.equal(cam_utils.ray_limits_valid(tn, tf), valid) and 0 < int(valid.sum()) < valid.numel()
    atol = OR.atol_gpu(g)
    assert float((tn - bn)[valid].abs().max()) <= atol and float((tf - bf)[valid].abs().max()) <= atol
    inside = (o.abs().amax(-1) < 0.5).to(dev) & valid
    assert int(inside.sum()) > 100 and bool((tn[inside] == 0).all())


# ----------------------------------------------------------------------------- 3. render_rays
@pytest.fixture(scope="module")
def scene(dev):
    """tiny64 with fp32 convs, B = 2, cameras at radius 4 through ray_grid (the config's interval would end in front of the cube),
    caller-given uniforms, and two ball masks of different radii: about half of the rays are empty, differently many per frame."""
    from hfa_gp_amd.cam_utils import ray_grid
    from hfa_gp_amd.generator import TriPlaneGenerator
    from hfa_gp_amd.occupancy import OccupancyGrid
    cfg = TR._e2e_cfg()
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws = make_inputs(cfg, 2)[0].to(dev)
    c = look_at_label(torch.tensor([math.pi / 2 + 0.3, math.pi / 2 - 0.2]), torch.tensor([math.pi / 2 - 0.1, math.pi / 2 + 0.15]),
                      r=4.0).to(dev)
    o, d = ray_grid(c, RES)
    rng = torch.Generator().manual_seed(21)
    r = RES * RES
    us = torch.rand(2, r, cfg.depth_resolution, generator=rng).to(dev)
    ui = torch.rand(2 * r, cfg.depth_resolution_importance, generator=rng).to(dev)
    x = (torch.arange(G_RENDER) + 0.5) / G_RENDER - 0.5
    rad = torch.stack(torch.meshgrid(x, x, x, indexing="ij"), -1).norm(dim=-1)
    balls = torch.stack((rad < 0.38, rad < 0.30))
    occ = OccupancyGrid.from_dense(balls.to(dev), cfg.box_warp)
    return dict(cfg=cfg, gen=gen, ws=ws, o=o, d=d, us=us, ui=ui, occ=occ, balls=balls)


def loss_of(out):
    return out["feature"].square().mean() + out["depth"].mean() + out["mask"].mean()


def test_render_rays_with_a_grid_is_the_explicit_limits_path(dev, scene):
    from hfa_gp_amd import ops
    s = scene
    gen, ws, o, d, us, ui, occ = (s[k] for k in ("gen", "ws", "o", "d", "us", "ui", "occ"))
    tn, tf = ops.ray_limits_grid(o, d, occ)
    nv = torch.isfinite(tn).sum(1).tolist()
    print(f"valid rays per frame: {nv} of {RES * RES}")
    assert 0.25 * RES * RES < nv[1] < nv[0] < 0.75 * RES * RES
    grads = []
    for kw in (dict(ray_limits=occ), dict(t_near=tn, t_far=tf), dict(t_near=tn, t_far=tf)):
        w = ws.clone().requires_grad_(True)
        out = gen.render_rays(w, o, d, us, ui, **kw)
        loss_of(out).backward()
        grads.append((out, w.grad))
    (a, ga), (b, gb), (_, gb2) = grads
    assert set(a) == set(b) == {"feature", "rgb", "depth", "mask", "valid"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # d ws: the same launches on the same inputs.  The plane gradient is accumulated with float atomics, so two IDENTICAL calls of
    # the explicit-limits path need not agree to the bit; the grid's call is held to the explicit one as tightly as that path is to
    # itself — bit-equal when it is — and in any case to the d ws bar of tests/test_gpu_ray_limits.py
    same = torch.equal(gb, gb2)
    print(f"d ws: two explicit-limits calls bit-equal: {same}; grid against explicit max |diff| {float((ga - gb).abs().max()):.3e}, "
          f"explicit against itself {float((gb - gb2).abs().max()):.3e}, max |d ws| {float(gb.abs().max()):.3e}")
    assert bool(ga.abs().max() > 0)
    if same:
        assert torch.equal(ga, gb)
    close(ga, gb, atol=2e-4 * gb.abs().max().item(), rtol=2e-3, what="d ws, grid against explicit limits")
    assert torch.equal(a["valid"], torch.isfinite(tn)) and not a["valid"].requires_grad
    e = ~a["valid"]
    assert bool((a["feature"][e] == -1).all()) and bool((a["mask"][e] == 0).all()) and bool((a["depth"][e] == a["depth"].max()).all())
    assert all(bool(torch.isfinite(v).all()) for k, v in a.items() if k != "valid")
    # it composes: samples and normals, under no_grad
    with torch.no_grad():
        full = gen.render_rays(ws, o, d, us, ui, ray_limits=occ, samples=True, normals=True)
        ref = gen.render_rays(ws, o, d, us, ui, t_near=tn, t_far=tf, samples=True, normals=True)
    for k in ref:
        assert torch.equal(full[k], ref[k]), k
    for k in ("feature", "depth", "mask"):
        assert torch.equal(full[k], a[k].detach()), k
    close(full["sample_weights"].sum(-1), full["mask"], atol=1e-5, rtol=0.0, what="sum of the weights against the mask")
    assert not bool(full["normal"][e].any()) and not bool(full["sample_weights"][e].any()) and not bool(full["sample_depths"][e].any())
    assert bool(full["normal"][~e].any())
    # the rays' gradient: exactly zero for an empty ray
    og, dg = o.clone().requires_grad_(True), d.clone().requires_grad_(True)
    loss_of(gen.render_rays(ws, og, dg, us, ui, ray_limits=occ)).backward()
    assert not bool(og.grad[e].any()) and not bool(dg.grad[e].any()) and bool(og.grad[~e].any())
    # one grid for both frames
    one = type(occ)(occ.bits[:1].contiguous(), occ.resolution, occ.cube_length)
    with torch.no_grad():
        shared = gen.render_rays(ws, o, d, us, ui, ray_limits=one)
    assert torch.equal(shared["feature"][0], a["feature"][0].detach()) and int(shared["valid"][1].sum()) > nv[1]


def test_all_zero_grid_renders_the_background(dev, scene):
    from hfa_gp_amd.occupancy import OccupancyGrid
    s = scene
    empty = OccupancyGrid.from_dense(torch.zeros_like(s["balls"]).to(dev), s["cfg"].box_warp)
    for compact in (False, True):
        with torch.no_grad():
            out = s["gen"].render_rays(s["ws"], s["o"], s["d"], s["us"], s["ui"], ray_limits=empty, compact=compact)
        assert not bool(out["valid"].any()) and bool((out["feature"] == -1).all()) and bool((out["rgb"] == -1).all())
        assert bool((out["mask"] == 0).all()) and bool((out["depth"] == 0).all())


class Counting:
    """ops.L.lib() with every entry point counted by name."""
    def __init__(self, real):
        self.real, self.calls = real, {}

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def counted(*a, **k):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a, **k)
        return counted


def test_compact_is_bit_identical_and_skips_the_empty_rays(dev, scene, monkeypatch):
    from hfa_gp_amd import _lib, ops
    from hfa_gp_amd.occupancy import OccupancyGrid
    s = scene
    gen, ws, o, d, us, ui, occ, cfg = (s[k] for k in ("gen", "ws", "o", "d", "us", "ui", "occ", "cfg"))
    kw = dict(ray_limits=occ, samples=True, normals=True)
    res = []
    for compact in (False, True):
        w, og, dg = ws.clone().requires_grad_(True), o.clone().requires_grad_(True), d.clone().requires_grad_(True)
        out = gen.render_rays(w, og, dg, us, ui, compact=compact, **kw)
        (loss_of(out) + out["sample_weights"].square().sum(-1).mean()).backward()
        res.append((out, w.grad, og.grad, dg.grad))
    (a, wa, oa, da), (b, wb, ob, db) = res
    nv = a["valid"].sum(1).tolist()
    assert nv[0] != nv[1] and set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), k
    close(wb, wa, atol=2e-4 * wa.abs().max().item(), rtol=2e-3, what="d ws, compact against not")
    check_rays(ob, oa.cpu(), "d origins, compact against not")
    check_rays(db, da.cpu(), "d directions, compact against not")
    e = ~a["valid"]
    assert not bool(ob[e].any()) and not bool(db[e].any())
    # only R' + 1 rays per frame reach the launch, in their original order
    seen = []
    real = ops.raymarch_rays
    monkeypatch.setattr(ops, "raymarch_rays", lambda planes, ro, *a_, **k_: (seen.append(ro.clone()), real(planes, ro, *a_, **k_))[1])
    with torch.no_grad():
        c = gen.render_rays(ws, o, d, us, ui, ray_limits=occ, compact=True)
        p = gen.render_rays(ws, o, d, us, ui, ray_limits=occ)
    monkeypatch.setattr(ops, "raymarch_rays", real)
    assert [t.shape[1] for t in seen] == [max(nv) + 1, RES * RES]
    assert torch.equal(seen[0][0, :nv[0]], o[0][a["valid"][0]])
    for k in p:
        assert torch.equal(c[k], p[k]), k
    # explicit limits compact as well; a frame without a valid ray; a call without one launches nothing
    tn, tf = ops.ray_limits_grid(o, d, occ)
    tn0, tf0 = tn.clone(), tf.clone()
    tn0[1], tf0[1] = INF, -INF
    with torch.no_grad():
        c = gen.render_rays(ws, o, d, us, ui, t_near=tn0, t_far=tf0, compact=True)
        p = gen.render_rays(ws, o, d, us, ui, t_near=tn0, t_far=tf0)
    assert not bool(c["valid"][1].any()) and bool(c["valid"][0].any())
    for k in p:
        assert torch.equal(c[k], p[k]), k
    counting = Counting(_lib.lib())
    monkeypatch.setattr(ops.L, "lib", lambda: counting)
    nothing = OccupancyGrid.from_dense(torch.zeros_like(s["balls"]).to(dev), cfg.box_warp)
    w = ws.clone().requires_grad_(True)
    out = gen.render_rays(w, o, d, us, ui, ray_limits=nothing, compact=True, samples=True, normal_grad=True)
    loss_of(out).backward()
    assert counting.calls == {"hfagp_ray_limits_grid": 1}, counting.calls
    assert not bool(w.grad.any()) and out["sample_weights"].shape == (2, RES * RES, cfg.depth_resolution +
                                                                       cfg.depth_resolution_importance - 1)
    assert not bool(out["normal"].any()) and bool((out["feature"] == -1).all())


def test_box_and_limitless_calls_launch_what_they_did(dev, scene, monkeypatch):
    from hfa_gp_amd import _lib, ops
    s = scene
    counting = Counting(_lib.lib())
    monkeypatch.setattr(ops.L, "lib", lambda: counting)
    with torch.no_grad():
        s["gen"].render_rays(s["ws"], s["o"], s["d"], s["us"], s["ui"])
        s["gen"].render_rays(s["ws"], s["o"], s["d"], s["us"], s["ui"], ray_limits="box")
    assert "hfagp_ray_limits_grid" not in counting.calls and "hfagp_occupancy_pack" not in counting.calls
    assert counting.calls["hfagp_raymarch_rays_fwd"] == 1 and counting.calls["hfagp_raymarch_rays_limits_fwd"] == 1
    assert counting.calls["hfagp_ray_limits_box"] == 1
    with torch.no_grad():
        s["gen"].render_rays(s["ws"], s["o"], s["d"], s["us"], s["ui"], ray_limits=s["occ"])
    assert counting.calls["hfagp_ray_limits_grid"] == 1 and counting.calls["hfagp_raymarch_rays_limits_fwd"] == 2
    assert counting.calls["hfagp_ray_limits_box"] == 1


# ----------------------------------------------------------------------------- 4. occupancy_grid
def test_occupancy_grid_is_conservative(dev, scene):
    """Every lattice point of the G k + 1 lattice with sigma >= level lies in a cell whose bit is set (all up to eight cells that
    share it, before any dilation); a level below the volume's minimum fills the grid."""
    s = scene
    gen, ws = s["gen"], s["ws"]
    g, k = 12, 2
    n = g * k + 1
    with torch.no_grad():
        vol = gen.density_grid(ws, resolution=n)
        level = vol.float().quantile(0.9).item()
        occ = gen.occupancy_grid(ws, resolution=g, level=level, oversample=k, dilate=0)
        wide = gen.occupancy_grid(ws, resolution=g, level=level, oversample=k, dilate=1, max_points=n * n * 2 * 5)
        full = gen.occupancy_grid(ws, resolution=g, level=vol.min().item() - 1.0, oversample=k)
    assert occ.resolution == g and occ.cube_length == s["cfg"].box_warp and occ.batch == 2
    dense = occ.dense()
    hot = (vol >= level).nonzero()                      # [N, 4]: b, x, y, z lattice indices
    assert hot.shape[0] > 100
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):                           # the cells that own lattice point p: ceil(p / k) - 1 and floor(p / k), clipped
                cell = [((hot[:, i + 1] + (k - 1) * dlt) // k - dlt).clamp(0, g - 1) for i, dlt in enumerate((dx, dy, dz))]
                assert bool(dense[hot[:, 0], cell[0], cell[1], cell[2]].all())
    assert 0 < int(dense.sum()) < dense.numel()
    assert bool((wide.dense() | ~dense).all()) and int(wide.dense().sum()) > int(dense.sum())
    assert bool(full.dense().all())
    from hfa_gp_amd.occupancy import occupancy_reference
    assert torch.equal(dense, occupancy_reference(vol, g, k, level, 0))
    assert torch.equal(wide.dense(), occupancy_reference(vol, g, k, level, 1))


# ----------------------------------------------------------------------------- 5. guards
def test_guards_raise_before_a_launch(dev, scene, monkeypatch):
    from hfa_gp_amd import ops
    from hfa_gp_amd.occupancy import OccupancyGrid
    s = scene
    gen, ws, o, d, occ = (s[k] for k in ("gen", "ws", "o", "d", "occ"))
    for name in ("raymarch_rays", "raymarch_rays_bwd", "ray_limits_box", "ray_limits_grid", "occupancy_pack", "planes_query"):
        monkeypatch.setattr(ops, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("launched")))
    monkeypatch.setattr(gen, "_query_planes", lambda *a, **k: (_ for _ in ()).throw(AssertionError("backbone launched")))
    three = OccupancyGrid(torch.zeros(3, G_RENDER, G_RENDER, 1, device=dev, dtype=torch.int32), G_RENDER, occ.cube_length)
    with pytest.raises(ValueError, match="batch must be B = 2 or 1"):
        gen.render_rays(ws, o, d, ray_limits=three)
    with pytest.raises(ValueError, match="cube_length"):
        gen.render_rays(ws, o, d, ray_limits=OccupancyGrid(occ.bits, occ.resolution, 2.0 * occ.cube_length))
    with pytest.raises(ValueError, match="mutually exclusive"):
        gen.render_rays(ws, o, d, ray_limits=occ, t_near=0.0, t_far=1.0)
    with pytest.raises(ValueError, match="compact=True needs ray limits"):
        gen.render_rays(ws, o, d, compact=True)
    with pytest.raises(ValueError, match="ray_limits must be None or 'box'"):
        gen.render_rays(ws, o, d, ray_limits=occ.bits)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gen.render_rays(ws, o, d, ray_limits=OccupancyGrid(occ.bits.cpu(), occ.resolution, occ.cube_length))
    for g in (1, 257):
        with pytest.raises(ValueError, match=r"resolution must be in \[2, 256\]"):
            gen.occupancy_grid(ws, resolution=g)
    with pytest.raises(ValueError, match="oversample"):
        gen.occupancy_grid(ws, resolution=64, oversample=0)
    with pytest.raises(ValueError, match="dilate"):
        gen.occupancy_grid(ws, resolution=64, dilate=-1)
    with pytest.raises(RuntimeError, match="wrap in `torch.no_grad"):
        gen.occupancy_grid(ws.clone().requires_grad_(True))
