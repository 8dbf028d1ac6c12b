"""The forward ray marcher's bilinear taps, one plane per quad lane exchanged by DPP (csrc/raymarch_common.h sample_taps_quad),
against the form it replaces — all three planes' taps on every lane of a gather quad (developer switch
HFAGP_DEV_RAY_TAPS_LEGACY=1).  Every tap is produced by the same instructions on the same inputs, only on another lane, so the two
forms must give the SAME BITS: feat, depth, wsum, tminmax, the saved per-sample state, and the records of the recomputing
backward pass.  Identical outputs cannot show that the switch switched anything: the CPU test at the end looks at the compiled
unit for that (both instantiations present, quad-permute moves in one and not in the other)."""
import itertools
import math
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests.util import ROOT, look_at_label

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SWITCH = "HFAGP_DEV_RAY_TAPS_LEGACY"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(new, old, what):
    """the same bits (stricter than torch.equal: tells -0 from +0 and compares NaN payloads), and torch.equal itself"""
    assert torch.equal(_bits(new), _bits(old)), what
    assert torch.isnan(new).any() or torch.equal(new, old), what


# scenes: (cameras(b) -> labels, box_warp, ray_start, ray_end)
def _cams(b, flipped=True):
    h = math.pi / 2 + torch.linspace(-0.35, 0.3, b)
    v = math.pi / 2 + torch.linspace(0.12, -0.2, b)
    return look_at_label(h, v, flipped=flipped)


SCENES = {
    # unit box seen from 2.7 away, depths 2.25 .. 3.3: the rays enter and leave the box, so tiles mix samples inside, outside and on
    # the faces (quads whose three planes differ in validity, clamped indices, zero weights)
    "box1": (lambda b: _cams(b), 1.0, 2.25, 3.3),
    # wider box and ray range (test_raymarch_edge_cases): most samples inside
    "box2": (lambda b: _cams(b), 2.0, 2.0, 3.6),
    # camera looking away (the un-flipped label): zero-padding taps only
    "away": (lambda b: _cams(b, flipped=False), 1.0, 2.25, 3.3),
}
PLANES_HW = [(24, 24), (5, 7), (17, 9)]            # non-square: the index stride (W) and the two clamps (W - 1, H - 1) differ
RES_B = [(8, 1), (12, 3)]


def _inputs(dev, seed, b, res, s, hw, scene):
    g = torch.Generator().manual_seed(seed)
    cams, box_warp, t0, t1 = SCENES[scene]
    c = cams(b)
    r = res * res
    t = dict(planes=torch.randn(b, 3, hw[0], hw[1], 32, generator=g),       # a distinct value per plane, texel and channel
             cam2world=c[:, :16].contiguous(), intrinsics=c[:, 16:25].contiguous(),
             u_strat=torch.rand(b, r, s, generator=g), u_imp=torch.rand(b * r, s, generator=g),
             dec_w0=torch.randn(64, 32, generator=g), dec_b0=0.1 * torch.randn(64, generator=g),
             dec_w1=torch.randn(33, 64, generator=g), dec_b1=0.1 * torch.randn(33, generator=g))
    kw = {k: v.to(dev) for k, v in t.items()}
    kw.update(res=res, ray_start=t0, ray_end=t1, box_warp=box_warp)
    return kw


def _both(monkeypatch, fn):
    monkeypatch.setenv(SWITCH, "1")
    old = fn(float("nan"))
    monkeypatch.delenv(SWITCH)
    new = fn(1.0)
    return new, old


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [16, 48], ids=["16+16", "48+48"])          # one and three tiles per pass: <1,1> and <3,3>
@pytest.mark.parametrize("decoder", ["f16x3", "fp32"])                         # the two gather paths: eval_pass's loop, eval_tile
def test_forward_outputs_and_state_are_bit_identical(dev, monkeypatch, decoder, samples):
    from hfa_gp_amd import ops
    n = 0
    for (res, b), hw, axes, scene in itertools.product(RES_B, PLANES_HW, (0, 1), SCENES):
        n += 1
        kw = _inputs(dev, 100 * n + samples, b, res, samples, hw, scene)

        def run(fill):
            state = ops.raymarch_state(b, res, samples, samples, dev).fill_(fill)      # (different garbage per arm: all of it is written)
            return ops.raymarch(plane_axes=axes, white_back=bool(n & 1), decoder_precision=decoder, state=state, **kw) + (state,)

        new, old = _both(monkeypatch, run)
        what = f"res {res} B {b} planes {hw} plane_axes {axes} scene {scene}"
        for name, x, y in zip(("feat", "depth", "wsum", "tminmax", "state"), new, old):
            _same(x, y, f"{name}: {what}")
        assert torch.isfinite(new[0]).all() and torch.isfinite(new[2]).all(), what
    assert n == 36


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", ["f16x3", "fp32"])
def test_gen_render_is_bit_identical(dev, monkeypatch, decoder):
    """the same through the generator's own call (gen.render: its camera split, uniforms and decoder parameters)"""
    import dataclasses
    from hfa_gp_amd.config import tiny64
    from hfa_gp_amd.generator import TriPlaneGenerator
    from hfa_gp_amd.synthetic import perturb_state
    cfg = dataclasses.replace(tiny64(), neural_rendering_resolution=12, img_resolution=48, decoder_precision=decoder,
                              plane_axes="eg3d_fixed")
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).to(dev)
    g = torch.Generator().manual_seed(5)
    b = 3
    planes = torch.randn(b, 3, 17, 9, 32, generator=g).to(dev)
    c = _cams(b).to(dev)
    us = torch.rand(b, 144, cfg.depth_resolution, generator=g).to(dev)
    ui = torch.rand(b * 144, cfg.depth_resolution_importance, generator=g).to(dev)
    new, old = _both(monkeypatch, lambda fill: gen.render(planes, c, us, ui))
    for name, x, y in zip(("feat", "depth", "wsum", "tminmax"), new, old):
        _same(x, y, name)


@pytest.mark.gpu
@pytest.mark.parametrize("decoder", ["f16x3", "fp32"])
def test_recomputing_backward_is_bit_identical(dev, monkeypatch, decoder):
    """raymarch_kernel<GRADS> without a saved state gathers and decodes every sample again (eval_tile): its per-sample records
    (depth, omega, d sigma) must be the same bits under both switch settings.  d planes comes from pass 2, whose float atomics sum
    in an order that may differ between two runs of the SAME code: it must be torch.equal whenever two runs of the legacy form are,
    and within the bound test_raymarch_backward_from_saved_state sets for that summation order otherwise."""
    from hfa_gp_amd import ops
    res, b, samples, hw = 12, 3, 48, (17, 9)
    kw = _inputs(dev, 7, b, res, samples, hw, "box1")
    g = torch.Generator().manual_seed(8)
    g_feat = torch.randn(b, res * res, 32, generator=g).to(dev)

    def run():
        return ops.raymarch_bwd(g_feat, return_rec=True, plane_axes=1, decoder_precision=decoder, **kw)

    monkeypatch.setenv(SWITCH, "1")
    d_old, rec_old = run()
    d_old2, rec_old2 = run()
    monkeypatch.delenv(SWITCH)
    d_new, rec_new = run()
    assert torch.equal(_bits(rec_old2[..., :3]), _bits(rec_old[..., :3]))
    _same(rec_new[..., :3], rec_old[..., :3], "records")
    assert torch.isfinite(d_new).all() and float(d_new.abs().max()) > 0
    print(f"d planes: legacy run to run {(d_old2 - d_old).abs().max().item():.3e}, new vs legacy {(d_new - d_old).abs().max().item():.3e}, "
          f"max |d| {d_old.abs().max().item():.3e}")
    if torch.equal(d_old2, d_old):
        assert torch.equal(d_new, d_old)
    else:
        assert (d_new - d_old).abs().max().item() <= 2e-6 * d_old.abs().max().item()


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_raymarch_forward_kernel_resources_and_tap_forms(tmp_path):
    """raymarch.hip compiled for gfx950 with build.sh's flags: the forward <3, 3, false, true, false> kernel — both tap forms — uses
    no scratch, spills no vector register and stays within 256 VGPRs (two workgroups per CU); the unit has no packed fp32
    arithmetic (build.sh's note on v_pk_*_f32); the default form exchanges its taps with quad-permute DPP moves and the legacy
    form (last template argument true) has none, so the developer switch selects different code."""
    build = open(os.path.join(ROOT, "hfa-gp_amd", "csrc", "build.sh")).read()
    flags = re.search(r"^FLAGS=\((.*)\)", build, re.M).group(1).split()
    asm = tmp_path / "raymarch.s"
    out = subprocess.run([HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc"), *flags, "-S", "--cuda-device-only",
                          "-Rpass-analysis=kernel-resource-usage", os.path.join(ROOT, "hfa-gp_amd", "csrc", "raymarch.hip"),
                          "-o", str(asm)], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    fwd = "raymarch_kernelILi3ELi3ELb0ELb1ELb0E"                # <3, 3, GRADS false, DEC16 true, FROM_STATE false, ...>
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"remark:\s+(ScratchSize \[bytes/lane\]|VGPRs Spill|VGPRs|AGPRs): (\d+)", line)
        if m and name and fwd in name:
            seen.setdefault(name, {})[m.group(1)] = int(m.group(2))
    new = [k for k in seen if k.endswith("Lb0ELb1ELb0ELb0EEEvNS_9RayParamsE")]
    legacy = [k for k in seen if k.endswith("Lb0ELb1ELb0ELb1EEEvNS_9RayParamsE")]
    assert len(seen) == 2 and len(new) == 1 and len(legacy) == 1, list(seen)
    for k, r in seen.items():
        print(k, r)
        assert r["ScratchSize [bytes/lane]"] == 0 and r["VGPRs Spill"] == 0, (k, r)
        assert r["VGPRs"] + r["AGPRs"] <= 256, (k, r)
    text = asm.read_text()
    assert not re.findall(r"v_pk_(fma|mul|add)_f32", text)

    def body(sym):
        a = text.index("\n" + sym + ":")
        return text[a:text.index("s_endpgm", a)]
    assert "quad_perm:[2,2,2,2]" in body(new[0])
    assert "quad_perm" not in body(legacy[0])
