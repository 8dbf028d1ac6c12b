"""Occupancy grids, the parts that need no GPU: OccupancyGrid's bit layout, the torch reference of hfagp_occupancy_pack, the
brute-force reference of hfagp_ray_limits_grid (cam_utils.ray_limits_grid) — float32 against float64, which is where the GPU test's
tolerance comes from, and closed-form cases — the argument checks of the two C entry points and the unit's resources."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import occupancy_ref as OR
from tests.util import ROOT

INF = float("inf")


# ----------------------------------------------------------------------------- 1. the bits
@pytest.mark.parametrize("g", [8, 33, 40])
def test_from_dense_round_trip_and_bit_layout(g):
    from hfa_gp_amd.occupancy import OccupancyGrid
    dense = OR.random_mask(g, seed=g, b=2)
    occ = OccupancyGrid.from_dense(dense, 1.0)
    w = (g + 31) // 32
    assert occ.bits.dtype == torch.int32 and occ.bits.shape == (2, g, g, w) and occ.resolution == g and occ.cube_length == 1.0
    assert torch.equal(occ.dense(), dense)
    # bit iz & 31 of word iz >> 5 at [b, ix, iy]; padding bits are 0
    bits = occ.bits.to(torch.int64) & 0xffffffff
    for ix, iy, iz in ((0, 0, 0), (1, 2, g - 1), (g - 1, 0, min(31, g - 1)), (3, g - 1, min(32, g - 1))):
        assert bool((bits[1, ix, iy, iz >> 5] >> (iz & 31)) & 1) == bool(dense[1, ix, iy, iz])
    if g % 32:
        assert not bool((bits[..., -1] >> (g % 32)).any())
    one = torch.zeros(g, g, g, dtype=torch.bool)
    one[2, 5, g - 1] = True
    single = OccupancyGrid.from_dense(one, 2.0)             # a [G, G, G] mask is one frame
    assert single.batch == 1 and int((single.bits != 0).sum()) == 1
    assert int(single.bits[0, 2, 5, (g - 1) >> 5]) & 0xffffffff == 1 << ((g - 1) & 31)


def test_grid_refuses_bad_shapes():
    from hfa_gp_amd.occupancy import OccupancyGrid
    with pytest.raises(ValueError, match="resolution must be in"):
        OccupancyGrid.from_dense(torch.ones(1, 1, 1, 1, dtype=torch.bool), 1.0)
    with pytest.raises(ValueError, match="resolution must be in"):
        OccupancyGrid(torch.zeros(1, 257, 257, 9, dtype=torch.int32), 257, 1.0)
    with pytest.raises(ValueError, match="bits must be int32"):
        OccupancyGrid(torch.zeros(1, 8, 8, 2, dtype=torch.int32), 8, 1.0)
    with pytest.raises(ValueError, match="cube_length"):
        OccupancyGrid(torch.zeros(1, 8, 8, 1, dtype=torch.int32), 8, 0.0)
    with pytest.raises(ValueError, match=r"\[B, G, G, G\]"):
        OccupancyGrid.from_dense(torch.ones(1, 8, 8, 4, dtype=torch.bool), 1.0)


# ----------------------------------------------------------------------------- 2. pooling, threshold, dilation
def _occupancy_loops(vol, g, k, level, dilate):
    """occupancy_reference by its definition, cell by cell."""
    raw = torch.zeros(vol.shape[0], g, g, g, dtype=torch.bool)
    for b in range(vol.shape[0]):
        for ix in range(g):
            for iy in range(g):
                for iz in range(g):
                    blk = vol[b, ix * k:(ix + 1) * k + 1, iy * k:(iy + 1) * k + 1, iz * k:(iz + 1) * k + 1]
                    raw[b, ix, iy, iz] = bool((~(blk < level)).any())
    out = torch.zeros_like(raw)
    for ix in range(g):
        for iy in range(g):
            for iz in range(g):
                s = [slice(max(i - dilate, 0), min(i + dilate, g - 1) + 1) for i in (ix, iy, iz)]
                out[:, ix, iy, iz] = raw[:, s[0], s[1], s[2]].flatten(1).any(1)
    return out


@pytest.mark.parametrize("g,k,dilate", [(4, 1, 0), (5, 2, 1), (6, 3, 2)])
def test_occupancy_reference_is_its_definition(g, k, dilate):
    from hfa_gp_amd.occupancy import occupancy_reference
    gen = torch.Generator().manual_seed(7)
    n = g * k + 1
    vol = torch.randn(2, n, n, n, generator=gen)
    vol[0, k, 2 * k, n - 1] = float("nan")                 # a lattice point on shared faces: occupied, with every cell that owns it
    level = 2.0                                             # inside the data's range: about 2 % of the points
    got = occupancy_reference(vol, g, k, level, dilate)
    assert got.dtype == torch.bool and got.shape == (2, g, g, g)
    assert torch.equal(got, _occupancy_loops(vol, g, k, level, dilate))
    assert 0 < int(got.sum()) and (dilate or int(got.sum()) < got.numel())
    assert bool(got[0, 0, 1, g - 1]) and bool(got[0, 1, 2, g - 1])            # the NaN's cells
    assert not bool(occupancy_reference(torch.full((1, n, n, n), -1.0), g, k, 0.0, dilate).any())
    assert bool(occupancy_reference(torch.full((1, n, n, n), 1.0), g, k, 0.0, dilate).all())


# ----------------------------------------------------------------------------- 3. the torch twin, float32 against float64
@pytest.mark.parametrize("g", [8, 16, 40])
def test_twin_float32_vs_float64(g):
    """cam_utils.ray_limits_grid in float32 (the arithmetic of the kernel) against float64 on the recipe of the issue: R = 4096,
    30 % occupancy.  The grazing share stays under its cap; off the grazing rays the hit / miss sets agree; the largest deviation
    of a limit is what tests/occupancy_ref.TWIN_F32_DEVIATION records per G, and 4 x that is the GPU tests' atol.  G = 8 and 16
    have planes that are exact in float32; G = 40 does not (L / G is rounded), which a ray with a small direction component on its
    deciding axis amplifies — so it carries its own, larger figure."""
    from hfa_gp_amd.cam_utils import ray_limits_grid
    dense = OR.random_mask(g, seed=100 + g)
    o, d = OR.recipe_rays(4096, seed=200 + g)
    n64, f64 = ray_limits_grid(o, d, dense, OR.CUBE)
    n32, f32 = ray_limits_grid(o.float(), d.float(), dense, OR.CUBE)
    assert n32.dtype == torch.float32 and n64.dtype == torch.float64
    graz = OR.grazing(o, d, dense)
    share = graz.float().mean().item()
    hit64, hit32 = torch.isfinite(n64), torch.isfinite(n32)
    both = hit64 & hit32 & ~graz
    dev = max((n32.double() - n64)[both].abs().max().item(), (f32.double() - f64)[both].abs().max().item())
    print(f"G = {g}: grazing {100 * share:.2f} %, hits {int(hit64.sum())} of {hit64.numel()}, largest float32 deviation {dev:.3e} "
          f"at t <= {f64[hit64].max().item():.2f}")
    assert share <= OR.GRAZING_CAP
    assert 0.3 < hit64.float().mean().item() < 0.9           # the recipe has both kinds
    assert torch.equal(hit32[~graz], hit64[~graz])
    for tn, tf, hit in ((n64, f64, hit64), (n32, f32, hit32)):
        assert bool(((tn == INF) & (tf == -INF))[~hit].all()) and bool((tf > tn)[hit].all()) and bool((tn >= 0)[hit].all())
    assert dev <= OR.TWIN_F32_DEVIATION[g]


# ----------------------------------------------------------------------------- 4. closed forms
def _limits(o, d, dense, dtype=torch.float64, cube=OR.CUBE):
    from hfa_gp_amd.cam_utils import ray_limits_grid
    tn, tf = ray_limits_grid(torch.tensor([o], dtype=dtype), torch.tensor([d], dtype=dtype), dense, cube)
    return tn[0].tolist(), tf[0].tolist()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_closed_forms(dtype):
    g = 8                                     # cells of side 1/8: every plane is exact in float32
    dense = torch.zeros(1, g, g, g, dtype=torch.bool)
    dense[0, 2, 3, 4] = dense[0, 6, 3, 4] = True
    cy, cz = -0.5 + 3.5 / 8, -0.5 + 4.5 / 8
    rows_o = [(-2.0, cy, cz),                 # along +x through the centres of both cells: enters x = -0.25, leaves x = 0.375
              (2.0, cy, cz),                  # the same line backwards
              (-0.2, cy, cz),                 # origin inside occupied cell (2, 3, 4): t_near == 0
              (0.05, cy, cz),                 # origin inside the cube in an EMPTY cell, between the two
              (0.05, cy, cz),                 # ... looking the other way
              (-2.0, -0.5 + 3.0 / 8, cz),     # parallel to x with the origin exactly on a cell plane: the half-open slab, row 3
              (-2.0, -0.5 + 4.0 / 8, cz),     # ... on the next plane: row 4, which is empty
              (-0.2, cy, cz),                 # zero direction
              (-2.0, 0.7, cz),                # parallel and beside the cube
              (-2.0, cy, cz),                 # points away from the cube
              (-2.0, cy, cz),                 # a direction of length 4: t scales by 1 / 4
              (-2.0, 0.5, cz)]                # parallel, exactly on the cube's face: the box kernel's 0 * inf
    rows_d = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 0.0, 0.0),
              (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (4.0, 0.0, 0.0), (1.0, 0.0, 0.0)]
    tn, tf = _limits(rows_o, rows_d, dense, dtype)
    want = [(1.75, 2.375), (1.625, 2.25), (0.0, 0.575), (0.2, 0.325), (0.175, 0.3), (1.75, 2.375), (INF, -INF), (INF, -INF),
            (INF, -INF), (INF, -INF), (1.75 / 4, 2.375 / 4), (INF, -INF)]
    for i, (a, b) in enumerate(want):
        assert tn[i] == pytest.approx(a, abs=1e-6) and tf[i] == pytest.approx(b, abs=1e-6), (i, tn[i], tf[i])
    assert tn[0] == 1.75 and tf[0] == 2.375 and tn[2] == 0.0            # exact: planes and differences are dyadic
    # a diagonal through the cube's centre with every cell set: the box's limits
    full = torch.ones(1, g, g, g, dtype=torch.bool)
    tn, tf = _limits([(-1.0, -1.0, -1.0)], [(1.0, 1.0, 1.0)], full, dtype)
    assert tn[0] == 0.5 and tf[0] == 1.5
    # the grid's batch of 1 is broadcast; an all-zero grid empties everything
    from hfa_gp_amd.cam_utils import ray_limits_grid
    o, d = OR.recipe_rays(64, seed=5, b=2, dtype=dtype)
    a = ray_limits_grid(o, d, full, OR.CUBE)
    b = ray_limits_grid(o, d, full.expand(2, -1, -1, -1), OR.CUBE)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].shape == (2, 64)
    tn, tf = ray_limits_grid(o, d, ~full, OR.CUBE)
    assert bool((tn == INF).all()) and bool((tf == -INF).all())


def test_all_ones_grid_is_the_box():
    """With every cell set the limits are the cube's (cam_utils.ray_limits_box) wherever that has a valid interval."""
    from hfa_gp_amd.cam_utils import ray_limits_box, ray_limits_grid, ray_limits_valid
    o, d = OR.recipe_rays(1024, seed=9)
    full = torch.ones(1, 8, 8, 8, dtype=torch.bool)
    tn, tf = ray_limits_grid(o, d, full, OR.CUBE)
    bn, bf = ray_limits_box(o, d, OR.CUBE)
    valid = ray_limits_valid(bn, bf)
    assert torch.equal(torch.isfinite(tn), valid) and 0 < int(valid.sum()) < valid.numel()
    assert torch.allclose(tn[valid], bn[valid], atol=1e-12, rtol=0) and torch.allclose(tf[valid], bf[valid], atol=1e-12, rtol=0)


# ----------------------------------------------------------------------------- 5. the C entry points and the compiled unit
@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_entry_points_check_their_arguments(lib):
    h = lib.lib()
    EBADARG = -1
    grid = lambda *a: h.hfagp_ray_limits_grid(*a, None)          # noqa: E731
    assert grid(1, 1, None, 1, 1, 1, 4, 8, 1.0) == EBADARG and b"null pointer" in h.hfagp_last_error()
    assert grid(1, 1, 1, 1, 1, 1, 0, 8, 1.0) == EBADARG and b"R = 0" in h.hfagp_last_error()
    assert grid(1, 1, 1, 1, 1, 65536, 65536, 8, 1.0) == EBADARG and b"B = 65536" in h.hfagp_last_error()
    for g in (1, 257):
        assert grid(1, 1, 1, 1, 1, 1, 4, g, 1.0) == EBADARG and b"G = " in h.hfagp_last_error()
    assert grid(1, 1, 1, 1, 1, 1, 4, 8, float("inf")) == EBADARG and b"box_side" in h.hfagp_last_error()
    pack = lambda *a: h.hfagp_occupancy_pack(*a, None)           # noqa: E731
    assert pack(None, 1, 1, 8, 1, 0.0, 0) == EBADARG and b"null pointer" in h.hfagp_last_error()
    assert pack(1, 1, 0, 8, 1, 0.0, 0) == EBADARG and b"B = 0" in h.hfagp_last_error()
    assert pack(1, 1, 1, 300, 1, 0.0, 0) == EBADARG and b"G = 300" in h.hfagp_last_error()
    assert pack(1, 1, 1, 8, 0, 0.0, 0) == EBADARG and b"oversample" in h.hfagp_last_error()
    assert pack(1, 1, 1, 256, 5, 0.0, 0) == EBADARG and b"oversample" in h.hfagp_last_error()
    assert pack(1, 1, 1, 8, 1, 0.0, 9) == EBADARG and b"dilate" in h.hfagp_last_error()
    assert pack(1, 1, 1, 8, 1, float("nan"), 0) == EBADARG and b"NaN" in h.hfagp_last_error()
    assert C.sizeof(C.c_int32) == 4


def test_python_guards_need_no_device():
    from hfa_gp_amd import ops
    from hfa_gp_amd.occupancy import OccupancyGrid
    occ = OccupancyGrid.from_dense(torch.ones(1, 8, 8, 8, dtype=torch.bool), 1.0)
    o = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ray_limits_grid(o, o, occ)
    with pytest.raises(ValueError, match="resolution must be in"):
        ops.occupancy_pack(torch.zeros(1, 2, 2, 2), 1, 1, 0.0, 0)
    with pytest.raises(ValueError, match="dilate"):
        ops.occupancy_pack(torch.zeros(1, 9, 9, 9), 8, 1, 0.0, 9)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.occupancy_pack(torch.zeros(1, 9, 9, 9), 8, 1, 0.0, 0)


HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_occupancy_unit_resources(tmp_path):
    """occupancy.hip is in build.sh's list and, compiled with its flags: two kernels without scratch or spill, the ray kernel without
    LDS, and none of the packed fp32 arithmetic build.sh keeps out of the library."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    assert re.search(r"^units\+=\(.*\boccupancy\b", build, re.M), "occupancy.hip is not in build.sh's unit list"
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / "occupancy.s"
    out = subprocess.run([HIPCC, *flags, "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", "occupancy.hip"),
                          "-o", str(asm), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=1800)
    assert out.returncode == 0, out.stderr[-2000:]
    res, name = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs|LDS Size \[bytes/block\]): (\d+)", line)
        if m and name:
            res.setdefault(name, {})[m.group(1)] = int(m.group(2))
    assert len(res) == 2, res
    for kernel, r in res.items():
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0 and r["VGPRs"] <= 64, (kernel, r)
    ray = next(r for k, r in res.items() if "ray_limits_grid_kernel" in k)
    pack = next(r for k, r in res.items() if "occupancy_pack_kernel" in k)
    assert ray["LDS Size [bytes/block]"] == 0 and 0 < pack["LDS Size [bytes/block]"] <= 256
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", asm.read_text())
