"""The 32-channel 16x16x32 loop of the forward 3x3 conv at F16X3 (csrc/modconv_bf16.hip, modconv_bf16_kernel<4, 2, 9, 0, 1>)
against the 16-channel loop it replaces for those layers (developer switch HFAGP_DEV_CONV9_LEGACY=1) and the exact-fp32
kernel.  Same operands and precision class: only the summation order inside the MFMA changes, so the new loop's error
against fp32 must stay within 1.25x the old loop's (max-abs and relative L2)."""
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


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


def _errs(y, ref):
    """max |y - ref| and ||y - ref|| / ||ref||, accumulated in float64 one sample at a time"""
    mx, num, den = 0.0, 0.0, 0.0
    for i in range(y.shape[0]):
        d = (y[i].double() - ref[i].double())
        mx = max(mx, d.abs().max().item())
        num += float((d * d).sum())
        den += float((ref[i].double() ** 2).sum())
    return mx, math.sqrt(num / max(den, 1e-300))


def _layer(dev, B, H, W, cin, cout, seed, xscale=1.0, sscale=1.0):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn(B, H, W, cin, device=dev, generator=g) * xscale
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g) / math.sqrt(9 * cin)
    s = (torch.randn(B, cin, device=dev, generator=g) + 1.0) * sscale
    dcoef = torch.rand(B, cout, device=dev, generator=g) + 0.5
    bias = torch.randn(cout, device=dev, generator=g)
    noise = torch.randn(H, W, device=dev, generator=g)
    return x, w, s, dcoef, bias, noise


def _three(monkeypatch, fn):
    """(new loop, 16-channel loop, exact fp32) outputs of fn(precision image kind)"""
    monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY", raising=False)
    new = fn("f16x3")
    monkeypatch.setenv("HFAGP_DEV_CONV9_LEGACY", "1")
    old = fn("f16x3")
    monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY")
    ref = fn("fp32")
    return new, old, ref


def _check(new, old, ref, distinct=True):
    assert torch.isfinite(new).all()
    e_new, e_old = _errs(new, ref), _errs(old, ref)
    assert e_new[0] <= BAR * e_old[0] + 1e-30, (e_new, e_old)
    assert e_new[1] <= BAR * e_old[1] + 1e-30, (e_new, e_old)
    if distinct:       # the two loops sum in different orders: identical bits would mean the new loop never ran
        assert not torch.equal(new, old)
    return e_new, e_old


def _run(dev, x, w, s, dcoef, bias, noise, cout, ksplit=0, clamp=None, **kw):
    from hfa_gp_amd import ops
    wts = {"fp32": ops.weight_prep(w)[0], "f16x3": ops.weight_prep_prec(w, "f16x3")}

    def fn(prec):
        return ops.modconv(x, wts[prec], cout, ops.CONV3X3, styles=s, dcoef=dcoef, noise=noise, noise_strength=0.3, bias=bias,
                           act="lrelu", gain=math.sqrt(2), clamp=clamp, ksplit=ksplit, **kw)
    return fn


# every forward 3x3 layer of the flagship render at B = 32 (H, Cin -> Cout); the 8^2 layer runs split-K by the plan
SHAPES = [(512, 128, 128), (256, 256, 256), (256, 128, 128), (128, 256, 256), (64, 512, 512), (32, 512, 512), (16, 512, 512),
          (8, 512, 512)]


@pytest.mark.gpu
@pytest.mark.parametrize("H,cin,cout", SHAPES)
def test_conv9_flagship_shapes_b32(dev, monkeypatch, H, cin, cout):
    x, w, s, dcoef, bias, noise = _layer(dev, 32, H, H, cin, cout, seed=H + cin)
    new, old, ref = _three(monkeypatch, _run(dev, x, w, s, dcoef, bias, noise, cout))
    _check(new, old, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,cin,cout,ksplit", [
    (1, 64, 64, 256, 256, 0),        # batch 1 (the plan splits K)
    (3, 40, 40, 128, 256, 0),        # odd batch, partial tiles on both axes
    (2, 24, 72, 256, 128, 0),        # non-square, W not a multiple of 16
    (2, 32, 32, 256, 128, 3),        # forced split-K: 8 chunks of 32 over 3 slices (odd pair tails)
    (2, 32, 32, 128, 128, 8),        # more slices than 32-channel chunks: empty slices store zeros
])
def test_conv9_edges(dev, monkeypatch, B, H, W, cin, cout, ksplit):
    x, w, s, dcoef, bias, noise = _layer(dev, B, H, W, cin, cout, seed=B * 7 + H)
    new, old, ref = _three(monkeypatch, _run(dev, x, w, s, dcoef, bias, noise, cout, ksplit=ksplit, clamp=4.0))
    _check(new, old, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("store_y", [True, False])
def test_conv9_fused_torgb(dev, monkeypatch, store_y):
    """SR conv1 with the fused toRGB (rgb_w / rgb_part) and y_absmax; store_y=False is the last SR layer of a forward-only call."""
    from hfa_gp_amd import ops
    B, H, cin, cout = 8, 64, 128, 128   # (256 blocks: no split-K, which the fused toRGB refuses)
    x, w, s, dcoef, bias, noise = _layer(dev, B, H, H, cin, cout, seed=5)
    rgb_w = torch.randn(B, 3, cout, device=dev, generator=torch.Generator(device=dev).manual_seed(6)) / math.sqrt(cout)
    wt = ops.weight_prep_prec(w, "f16x3")

    def fn():
        slots = ops.absmax_slots(1, dev)
        y, part = ops.modconv(x, wt, cout, ops.CONV3X3, styles=s, dcoef=dcoef, noise=noise, noise_strength=0.3, bias=bias,
                              act="lrelu", gain=math.sqrt(2), rgb_w=rgb_w, store_y=store_y,
                              y_absmax=slots[0] if store_y else None)
        return y, part, slots.max().item()
    monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY", raising=False)
    y_new, p_new, m_new = fn()
    monkeypatch.setenv("HFAGP_DEV_CONV9_LEGACY", "1")
    y_old, p_old, m_old = fn()
    monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY")
    y_ref = ops.modconv(x, ops.weight_prep(w)[0], cout, ops.CONV3X3, styles=s, dcoef=dcoef, noise=noise, noise_strength=0.3,
                        bias=bias, act="lrelu", gain=math.sqrt(2))
    rgb_ref = torch.einsum("bhwc,brc->bhwr", y_ref.double(), rgb_w.double())
    assert p_new.shape == p_old.shape
    rgb_new, rgb_old = p_new.sum(0)[..., :3].double(), p_old.sum(0)[..., :3].double()
    assert (p_new[..., 3] == 0).all()
    _check(rgb_new, rgb_old, rgb_ref)
    if store_y:
        _check(y_new, y_old, y_ref)
        want = y_ref.abs().max().item()
        assert abs(m_new - want) <= 1e-5 * want and abs(m_old - want) <= 1e-5 * want, (m_new, m_old, want)
    else:
        assert y_new is None and y_old is None


@pytest.mark.gpu
@pytest.mark.parametrize("xscale,sscale,tol", [(200.0, 40.0, 4e-6), (1e-3, 1.0, 1e-4), (1.0, 1e-4, 4e-6), (3e4, 1e3, 4e-6)])
def test_conv9_f16x3_range_guard(dev, monkeypatch, xscale, sscale, tol):
    """test_f16x3_range_guard's extremes on an image the staged kernel takes (the small-image kernel takes that test's 12^2),
    against a float64 reference, with x_absmax as a producer would publish it."""
    from hfa_gp_amd import ops
    g = torch.Generator().manual_seed(23)
    b, cin, cout, h = 2, 64, 128, 40
    x = torch.randn(b, cin, h, h, generator=g) * xscale
    if xscale > 1e4:
        x = x.clamp(-6e4, 6e4)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    s = (torch.randn(b, cin, generator=g) + 1.5) * sscale
    want = F.conv2d((x * s[:, :, None, None]).reshape(1, b * cin, h, h).double(), w.repeat(b, 1, 1, 1).double(),
                    padding=1, groups=b).reshape(b, cout, h, h)
    wb = ops.weight_prep_prec(w.to(dev), "f16x3")
    xd = ops.nchw_to_nhwc(x.to(dev))
    xam = xd.abs().amax().expand(64 * 32).contiguous()
    outs = {}
    for legacy in (False, True):
        if legacy:
            monkeypatch.setenv("HFAGP_DEV_CONV9_LEGACY", "1")
        else:
            monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY", raising=False)
        for name, am in (("guard", None), ("absmax", xam)):
            y = ops.nhwc_to_nchw(ops.modconv(xd, wb, cout, ops.CONV3X3, styles=s.to(dev), x_absmax=am)).cpu().double()
            assert torch.isfinite(y).all()
            err = (y - want).abs().max().item()
            assert err <= tol * want.abs().max().item(), (legacy, name, err, want.abs().max().item())
            outs[(legacy, name)] = err
    monkeypatch.delenv("HFAGP_DEV_CONV9_LEGACY")
    for name in ("guard", "absmax"):
        assert outs[(False, name)] <= BAR * outs[(True, name)] + 1e-30 or outs[(False, name)] <= 0.25 * tol * want.abs().max().item(), outs


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not available")
def test_conv9_loop_does_not_spill(tmp_path):
    """CPU check: the 32-channel loop compiles with build.sh's flags to 0 scratch at 2 waves per SIMD (two blocks per CU)."""
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-slp-vectorize", "-fno-vectorize",
                          "-S", "--cuda-device-only", os.path.join(ROOT, "hfa-gp_amd", "csrc", "modconv_bf16.hip"),
                          "-o", str(tmp_path / "x.s"), "-Rpass-analysis=kernel-resource-usage"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    name, seen = None, {}
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if name and "modconv_bf16_kernelILi4ELi2ELi9ELi0ELi1E" in name:
            for key in ("VGPRs Spill", "ScratchSize \\[bytes/lane\\]", "Occupancy \\[waves/SIMD\\]"):
                m = re.search(key + r": (\d+)", line)
                if m:
                    seen[key] = int(m.group(1))
    assert seen.get("VGPRs Spill") == 0 and seen.get("ScratchSize \\[bytes/lane\\]") == 0, seen
    assert seen.get("Occupancy \\[waves/SIMD\\]", 0) >= 2, seen
    isa = open(tmp_path / "x.s").read()
    body = isa[isa.index("_ZN5hfagp19modconv_bf16_kernelILi4ELi2ELi9ELi0ELi1EEEvNS_10ConvParamsEi:"):]
    body = body[:body.index("s_endpgm")]
    assert not re.search(r"v_pk_(fma|mul|add)_f32", body), "packed fp32 arithmetic (build.sh, lanes 48-63)"
    # the K loop (the pairs of chunks): the loop, from its header to the branch back to it, that holds the MFMAs
    loops = []
    for h in re.finditer(r"^(\.LBB\w+):[^\n]*Loop Header", body, re.M):
        back = re.search(r"s_cbranch\w* " + re.escape(h.group(1)) + r"\s", body[h.start():])
        if back:
            loops.append(body[h.start():h.start() + back.end()])
    loop = max(loops, key=lambda t: t.count("v_mfma"))
    assert loop.count("v_mfma_f32_16x16x32_f16") == 2 * 9 * 48
    assert "v_lshl_add_u64" not in loop, "64-bit address arithmetic in the 32-channel loop"
