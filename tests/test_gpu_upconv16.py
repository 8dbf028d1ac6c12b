"""The 32-channel 16x16x32 loop of the merged up-conv at F16X3 (csrc/modconv_bf16.hip, upconv_bf16_kernel<4, 4, 0, 2>) against
the 16-channel loop it replaces for those layers (developer switch HFAGP_DEV_UP_LEGACY_LOOP=1) and the exact-fp32 kernel.  Same
operands and precision class: only the summation order changes, so the new loop's error against fp32 must stay within 1.25x
the old loop's (max-abs and relative L2), per sample — the style magnitudes differ by 1e4 across a batch."""
import math
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests.util import ROOT

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
BAR = 1.25
CLASS = 4e-6        # the f16x3 bound of tests/test_gpu_round6.py, relative to max |ref|
SWITCH = "HFAGP_DEV_UP_LEGACY_LOOP"


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _layer(dev, B, H, W, cin, cout, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, H, W, cin, device=dev, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)
    s = torch.randn(B, cin, device=dev, generator=g) * torch.logspace(-2, 2, B, device=dev)[:, None]
    return x, w, s


def _three(monkeypatch, fn):
    """(new loop, 16-channel loop, exact fp32) outputs of fn(precision image kind)"""
    monkeypatch.delenv(SWITCH, raising=False)
    new = fn("f16x3")
    monkeypatch.setenv(SWITCH, "1")
    old = fn("f16x3")
    monkeypatch.delenv(SWITCH)
    ref = fn("fp32")
    return new, old, ref


def _errs(y, ref):
    d = y.double() - ref.double()
    return d.abs().max().item(), math.sqrt(float((d * d).sum()) / max(float((ref.double() ** 2).sum()), 1e-300))


def _check(new, old, ref):
    """per sample: within BAR x the old loop's error in both measures, or within a quarter of the class bound (with one or two
    chunks the ratio of two tiny errors is noise)"""
    assert torch.isfinite(new).all()
    assert new.shape == old.shape == ref.shape
    assert not torch.equal(new, old)       # the two loops sum in different orders: identical bits would mean the new loop never ran
    for i in range(new.shape[0]):
        e_new, e_old = _errs(new[i], ref[i]), _errs(old[i], ref[i])
        scale = ref[i].abs().max().item()
        print(f"sample {i}: new max {e_new[0]:.3e} l2 {e_new[1]:.3e} | old max {e_old[0]:.3e} l2 {e_old[1]:.3e} | max|ref| {scale:.3e}")
        within = e_new[0] <= BAR * e_old[0] + 1e-30 and e_new[1] <= BAR * e_old[1] + 1e-30
        assert within or e_new[0] <= 0.25 * CLASS * scale, (i, e_new, e_old, scale)


def _run(x, w, s, cout, ksplit=0):
    from hfa_gp_amd import ops
    wts = {"fp32": ops.weight_prep(w)[0], "f16x3": ops.weight_prep_prec(w, "f16x3")}

    def fn(prec):
        return ops.modconv(x, wts[prec], cout, ops.CONVT3X3_UP2, styles=s, ksplit=ksplit if prec != "fp32" else 0)
    return fn


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cin,cout,ksplit", [
    (3, 16, 32, 32, 128, 0),      # fringe tiles, tiles straddling samples, ragged last row tile, one chunk
    (5, 8, 16, 64, 128, 0),       # one fringe tile over all samples
    (2, 24, 40, 64, 64, 0),       # W % 16 != 0 (no fringe tiles), Cout = 64
    (9, 4, 4, 32, 128, 0),        # a patch touching three samples
    (33, 16, 16, 32, 128, 0),     # more samples than a block stages
    (2, 32, 32, 256, 128, 3),     # 8 chunks over 3 slices
    (2, 32, 32, 128, 128, 8),     # more slices than 32-channel chunks: empty slices store zeros
    (4, 32, 48, 512, 512, 0),     # styles beyond the default dynamic LDS (of the 16-channel loop; 8 samples x 512 styles here)
    (1, 64, 64, 256, 128, 0),     # batch 1, plan-chosen split
])
def test_upconv16_shapes(dev, monkeypatch, B, H, W, cin, cout, ksplit):
    x, w, s = _layer(dev, B, H, W, cin, cout, seed=B * 7 + H + cin)
    new, old, ref = _three(monkeypatch, _run(x, w, s, cout, ksplit=ksplit))
    assert new.shape == (B, 2 * H + 1, 2 * W + 1, cout)
    _check(new, old, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("xscale,sscale,tol", [(200.0, 40.0, 4e-6), (1e-3, 1.0, 1e-4), (1.0, 1e-4, 4e-6), (3e4, 1e3, 4e-6)])
def test_upconv16_range_guard(dev, monkeypatch, xscale, sscale, tol):
    """test_conv9_f16x3_range_guard's extremes on the up-conv, against a float64 conv_transpose2d, with and without x_absmax as a
    producer would publish it."""
    from hfa_gp_amd import ops
    g = torch.Generator().manual_seed(23)
    b, cin, cout, h = 2, 64, 128, 24
    x = torch.randn(b, cin, h, h, generator=g) * xscale
    if xscale > 1e4:
        x = x.clamp(-6e4, 6e4)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    s = (torch.randn(b, cin, generator=g) + 1.5) * sscale
    want = F.conv_transpose2d((x * s[:, :, None, None]).double(), w.transpose(0, 1).double(), stride=2)
    wb = ops.weight_prep_prec(w.to(dev), "f16x3")
    xd = ops.nchw_to_nhwc(x.to(dev))
    xam = xd.abs().amax().expand(64 * 32).contiguous()
    outs = {}
    for legacy in (False, True):
        if legacy:
            monkeypatch.setenv(SWITCH, "1")
        else:
            monkeypatch.delenv(SWITCH, raising=False)
        for name, am in (("guard", None), ("absmax", xam)):
            y = ops.nhwc_to_nchw(ops.modconv(xd, wb, cout, ops.CONVT3X3_UP2, styles=s.to(dev), x_absmax=am)).cpu().double()
            assert torch.isfinite(y).all()
            err = (y - want).abs().max().item()
            print(legacy, name, err, want.abs().max().item())
            assert err <= tol * want.abs().max().item(), (legacy, name, err, want.abs().max().item())
            outs[(legacy, name)] = err
    monkeypatch.delenv(SWITCH)
    for name in ("guard", "absmax"):
        assert outs[(False, name)] <= BAR * outs[(True, name)] + 1e-30 or outs[(False, name)] <= 0.25 * tol * want.abs().max().item(), outs


@pytest.mark.gpu
def test_upconv16_sample_alone_equals_sample_in_batch(dev, monkeypatch):
    """Sample i of a batch of 6 equals the same sample run alone, bit for bit, at four 32-channel chunks (same K order, same
    scales: only the tile it lands in and the resource it is read through differ)."""
    from hfa_gp_amd import ops
    monkeypatch.delenv(SWITCH, raising=False)
    g = torch.Generator().manual_seed(62)
    b, h, cin, cout = 6, 16, 128, 128
    x = torch.randn(b, h, h, cin, generator=g).to(dev)
    s = (torch.randn(b, cin, generator=g) * torch.logspace(-1, 1, b)[:, None]).to(dev)
    wb = ops.weight_prep_prec(torch.randn(cout, cin, 3, 3, generator=g).to(dev), "f16x3")
    full = ops.modconv(x, wb, cout, ops.CONVT3X3_UP2, styles=s)
    for i in (0, 3, 5):
        one = ops.modconv(x[i:i + 1].contiguous(), wb, cout, ops.CONVT3X3_UP2, styles=s[i:i + 1].contiguous())
        assert torch.equal(one[0], full[i]), i


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16x3", "bf16x3", "f16"])
@pytest.mark.parametrize("B,H,W", [(2, 24, 40), (3, 16, 32)])      # without / with fringe tiles
def test_upconv_legacy_loop_cout_64(dev, monkeypatch, prec, B, H, W):
    """Cout = 64, which the launcher admits for the 4-wave merged up-conv since the 32-channel loop, on the 16-channel loop of
    every kind that reaches it (f16x3 by the switch), against a float64 conv_transpose2d at the class bounds of
    tests/test_gpu_round6.py's test_upconv_stacked_rows_and_fringe_tiles."""
    from hfa_gp_amd import ops
    monkeypatch.setenv(SWITCH, "1")
    cin, cout = 64, 64
    g = torch.Generator().manual_seed(64)
    x = torch.randn(B, cin, H, W, generator=g)
    w3 = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)
    s = torch.randn(B, cin, generator=g) * torch.logspace(-2, 2, B)[:, None]
    tol = {"f16x3": 4e-6, "bf16x3": 5e-5, "f16": 6e-3}[prec]
    want = F.conv_transpose2d((x * s[:, :, None, None]).double(), w3.transpose(0, 1).double(), stride=2)
    y = ops.modconv(ops.nchw_to_nhwc(x.to(dev)), ops.weight_prep_prec(w3.to(dev), prec), cout, ops.CONVT3X3_UP2, styles=s.to(dev))
    y = ops.nhwc_to_nchw(y).cpu().double()
    assert y.shape == want.shape == (B, cout, 2 * H + 1, 2 * W + 1)
    for i in range(B):
        err, scale = (y[i] - want[i]).abs().max().item(), want[i].abs().max().item()
        print(f"{prec} sample {i}: err {err:.3e} max|ref| {scale:.3e}")
        assert err <= tol * scale + 1e-12, (i, err, scale)


@pytest.mark.gpu
def test_upconv16_layer_with_fir_epilogue(dev, monkeypatch):
    """The whole up-sampling layer, modconv(UP2) + upfir_epilogue, under both loops and on the exact-fp32 kernel."""
    from hfa_gp_amd import ops
    B, H, cin, cout = 2, 32, 128, 128
    x, w, s = _layer(dev, B, H, H, cin, cout, seed=77)
    g = torch.Generator(device=dev).manual_seed(78)
    dcoef = torch.rand(B, cout, device=dev, generator=g) + 0.5
    bias = torch.randn(cout, device=dev, generator=g)
    noise = torch.randn(2 * H, 2 * H, device=dev, generator=g)
    raw = _run(x, w, s, cout)

    def fn(prec):
        return ops.upfir_epilogue(raw(prec), dcoef, noise, 0.3, bias, act="lrelu", gain=math.sqrt(2))
    new, old, ref = _three(monkeypatch, fn)
    assert new.shape == (B, 2 * H, 2 * H, cout)
    _check(new, old, ref)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_upconv16_loop_does_not_spill(tmp_path):
    """CPU check: the 32-channel loop compiles with build.sh's flags to 0 scratch at 2 waves per SIMD (two
    blocks per CU), without packed fp32 arithmetic, with 2 x 216 MFMAs and no 64-bit VALU address arithmetic in the K loop."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-fno-vectorize",
                          "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", "modconv_bf16.hip"),
                          "-o", str(tmp_path / "x.s"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    isa = open(tmp_path / "x.s").read()
    for loop_id in (2,):
        tag = f"upconv_bf16_kernelILi4ELi4ELi0ELi{loop_id}E"
        name, seen = None, {}
        for line in out.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            if name and tag in name:
                for key in ("VGPRs Spill", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]"):
                    m = re.search(key + r": (\d+)", line)
                    if m:
                        seen[key] = int(m.group(1))
        assert seen.get("VGPRs Spill") == 0 and seen.get("ScratchSize \\[bytes/lane\\]") == 0, (loop_id, seen)
        assert seen.get("Occupancy \\[waves/SIMD\\]", 0) >= 2, (loop_id, seen)
        body = isa[isa.index(f"_ZN5hfagp18{tag}EEvNS_10ConvParamsE:"):]
        body = body[:body.index("s_endpgm")]
        assert not re.search(r"v_pk_(fma|mul|add)_f32", body), "packed fp32 arithmetic (build.sh, lanes 48-63)"
        # the K loop (the pairs of chunks): the loop, from its header to the branch back to it, that holds the MFMAs
        loops = []
        for h in re.finditer(r"^(\.LBB\w+):[^\n]*Loop Header", body, re.M):
            back = re.search(r"s_cbranch\w* " + re.escape(h.group(1)) + r"\s", body[h.start():])
            if back:
                loops.append(body[h.start():h.start() + back.end()])
        loop = max(loops, key=lambda t: t.count("v_mfma"))
        assert loop.count("v_mfma_f32_16x16x32_f16") == 2 * 9 * 8 * 3, loop_id
        assert "v_lshl_add_u64" not in loop, "64-bit address arithmetic in the 32-channel loop"
