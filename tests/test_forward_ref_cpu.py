"""tests/forward_ref.py is the contract, not a transcript of the kernels: every reference function against an independent float64
formulation (torch.nn.functional convolutions with the FIR kernel, and the oracle's own operators in float64) to 1e-12 of its
magnitude; the adjoint pair blur_down / blur_down_bwd by <A x, y> == <x, A^T y>; and the preconditions of the exact tier of
tests/test_gpu_forward_kernels.py (every integer case's reference is an fp32 number — an fp16 number for fp16 storage — and every
partial sum stays below 2^24 quanta), which need no GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import eg3d_oracle as O
from tests import forward_ref as R

F64 = torch.float64
TOL = 1e-12


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def agree(ref, mag, other, what):
    assert ref.shape == other.shape, f"{what}: {tuple(ref.shape)} vs {tuple(other.shape)}"
    err = (ref - other).abs()
    assert bool((err <= TOL * mag).all()), f"{what}: |reference - independent| = {err.max().item():.3e} (magnitude {mag.max().item():.3e})"
    assert bool((ref.abs() <= mag * (1 + TOL)).all()), f"{what}: |reference| above its magnitude"
    assert other.abs().max().item() > 0, f"{what}: the independent value is identically 0 (the check would be empty)"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


FIR = O.fir_kernel().double()             # outer([1,3,3,1]) / 64, dyadic


# ----------------------------------------------------------------------------- styles, demodulation, weight image, the FIR epilogue
@pytest.mark.parametrize("act_clamp", [None, 0.8])
def test_styles_wsq_and_fir_epilogue_make_the_oracles_up_sampling_layer(act_clamp):
    """styles_demod + weight_prep's wsq + upfir_epilogue over a float64 conv_transpose2d are the oracle's synthesis_layer(up=2), in
    both of its algebraic forms; styles alone are the oracle's fully_connected."""
    g = torch.Generator().manual_seed(3)
    b, cin, cout, h, w, wd = 2, 8, 5, 3, 4, 12
    P = {"L.affine.weight": rnd(g, cin, wd), "L.affine.bias": rnd(g, cin) + 1, "L.weight": rnd(g, cout, cin, 3, 3), "L.bias": rnd(g, cout),
         "L.noise_const": rnd(g, 2 * h, 2 * w), "L.noise_strength": torch.tensor(0.37, dtype=F64)}
    x, ws = rnd(g, b, cin, h, w), rnd(g, b, wd)
    (_, wsq), (_, mwsq) = R.weight_prep(P["L.weight"])
    agree(wsq, mwsq, P["L.weight"].square().sum(dim=(2, 3)), "wsq")
    (styles, dcoef), (ms, md) = R.styles_demod(ws, P["L.affine.weight"], P["L.affine.bias"], wsq, 1.0, 1e-8)
    agree(styles, ms, O.fully_connected(ws, P["L.affine.weight"], P["L.affine.bias"]), "styles")
    wmod = P["L.weight"][None] * styles[:, None, :, None, None]
    agree(dcoef, md, (wmod.square().sum(dim=(2, 3, 4)) + 1e-8).rsqrt(), "dcoef")
    yt = F.conv_transpose2d(x * styles[:, :, None, None], P["L.weight"].transpose(0, 1), stride=2)
    y, my = R.upfir_epilogue(nhwc(yt), dcoef, P["L.noise_const"], 0.37, P["L.bias"], "lrelu", 0.2, math.sqrt(2.0), act_clamp)
    for fused in (False, True):
        want = O.synthesis_layer(x, ws, P, "L", 2, FIR, "const", act_clamp, 0.2, fused, 1e-8)
        assert want.dtype == F64
        agree(nchw(y), nchw(my) + 1e-3, want, f"synthesis_layer fused={fused}")       # (the fused form rounds differently: 1e-15 absolute)


@pytest.mark.parametrize("h,w", R.UPFIR_HW)
@pytest.mark.parametrize("mask", range(8))
def test_upfir_epilogue_is_a_padded_fir_convolution_and_bias_act(h, w, mask):
    g = torch.Generator().manual_seed(10 * h + w + mask)
    b, c = 2, 4
    yt = rnd(g, b, 2 * h + 1, 2 * w + 1, c)
    d, nz, bs = (rnd(g, b, c) if mask & 1 else None), (rnd(g, 2 * h, 2 * w) if mask & 2 else None), (rnd(g, c) if mask & 4 else None)
    act, clamp = ("lrelu", "linear")[mask & 1], (None, 1.1)[(mask >> 1) & 1]
    ref, mag = R.upfir_epilogue(yt, d, nz, 0.3, bs, act, 0.2, 1.7, clamp)
    k = torch.outer(torch.tensor([1.0, 3, 3, 1], dtype=F64), torch.tensor([1.0, 3, 3, 1], dtype=F64)) / 16
    pre = F.conv2d(F.pad(nchw(yt), (1, 1, 1, 1)), k[None, None].repeat(c, 1, 1, 1), groups=c)
    assert torch.allclose(pre, O.upfirdn2d(nchw(yt), FIR, padding=(1, 1, 1, 1), gain=4.0), rtol=0, atol=1e-13)
    if d is not None:
        pre = pre * d[:, :, None, None]
    if nz is not None:
        pre = pre + nz * 0.3
    want = O.bias_act(pre, bs, act=act, alpha=0.2, gain=1.7, clamp=clamp)
    if act == "lrelu":
        assert torch.equal(want, (F.leaky_relu(pre + (0 if bs is None else bs[None, :, None, None]), 0.2) * 1.7).clamp(
            -(clamp or math.inf), clamp or math.inf))
    agree(nchw(ref), nchw(mag), want, "upfir_epilogue")
    assert ref.shape == (b, 2 * h, 2 * w, c)


# ----------------------------------------------------------------------------- skip, toRGB
@pytest.mark.parametrize("hw", [hw for hw in R.SKIP_IMG if hw])
def test_skip_upsample_add_is_the_oracles_upsample2d(hw):
    g = torch.Generator().manual_seed(hw[0])
    img, y = rnd(g, 2, hw[0], hw[1], 12), rnd(g, 2, 2 * hw[0], 2 * hw[1], 12)
    ref, mag = R.skip_upsample_add(img, y)
    want = O.upsample2d(nchw(img), FIR) + nchw(y)
    agree(nchw(ref), nchw(mag), want, "skip_upsample_add")
    pm, mpm = R.skip_upsample_add(img, y, plane_major=True)
    agree(pm, mpm, want.reshape(2, 3, 4, *want.shape[2:]).permute(0, 1, 3, 4, 2), "plane-major")
    alone, malone = R.skip_upsample_add(None, y)
    assert torch.equal(alone, y) and torch.equal(malone, y.abs())


@pytest.mark.parametrize("cout", R.TORGB_COUT)
@pytest.mark.parametrize("clamp", [None, 0.9])
def test_torgb_small_and_finish_are_the_oracles_torgb_layer_plus_skip(cout, clamp):
    g = torch.Generator().manual_seed(cout)
    b, cin, h, w, wd = 2, 8, 4, 6, 12
    P = {"T.affine.weight": rnd(g, cin, wd), "T.affine.bias": rnd(g, cin) + 1, "T.weight": rnd(g, cout, cin, 1, 1), "T.bias": rnd(g, cout)}
    x, ws, prev = rnd(g, b, cin, h, w), rnd(g, b, wd), rnd(g, b, cout, h // 2, w // 2)
    (styles, _), _ = R.styles_demod(ws, P["T.affine.weight"], P["T.affine.bias"], None, 1.0 / math.sqrt(cin))
    (out, pre), (mout, mpre) = R.torgb_small(nhwc(x), P["T.weight"].reshape(cout, cin), styles, P["T.bias"], prev, clamp)
    for fused in (False, True):
        agree(pre, mpre, O.torgb_layer(x, ws, P, "T", None, fused), f"y_pre fused={fused}")
        agree(out, mout, O.torgb_layer(x, ws, P, "T", clamp, fused) + O.upsample2d(prev, FIR), f"rgb_out fused={fused}")
    (o0, _), (m0, _) = R.torgb_small(nhwc(x), P["T.weight"].reshape(cout, cin), styles, P["T.bias"], None, clamp)
    agree(o0, m0, O.torgb_layer(x, ws, P, "T", clamp, False), "no previous image")
    if cout <= 3:                      # torgb_finish: the same image from partial sums split over the input channels
        xs = nhwc(x) * styles[:, None, None, :]
        wt = P["T.weight"].reshape(cout, cin)
        part = torch.zeros(3, b, h, w, 4, dtype=F64)
        for q, sl in enumerate((slice(0, 3), slice(3, 4), slice(4, 8))):
            part[q, ..., :cout] = xs[..., sl] @ wt[:, sl].T
        part[..., 3] = 7.0                                                   # the unused channel
        (fo, fp), (mfo, mfp) = R.torgb_finish(part, P["T.bias"], prev, clamp)
        agree(fo, mfo, out, "torgb_finish rgb_out")
        agree(fp, mfp, pre, "torgb_finish y_pre")


# ----------------------------------------------------------------------------- fully connected, weight image
@pytest.mark.parametrize("act", ["linear", "lrelu"])
@pytest.mark.parametrize("bias", [False, True])
def test_fully_connected_is_linear_plus_leaky_relu(act, bias):
    g = torch.Generator().manual_seed(5)
    x, wt, b = rnd(g, 3, 7), rnd(g, 5, 7), (rnd(g, 5) if bias else None)
    ref, mag = R.fully_connected(x, wt, b, 0.01, act, 0.2, 1.3)
    want = F.linear(x, wt * (0.01 / math.sqrt(7)), None if b is None else b * 0.01)
    agree(ref, mag, (F.leaky_relu(want, 0.2) if act == "lrelu" else want) * 1.3, "fully_connected")
    if act == "linear":
        agree(ref, mag, O.fully_connected(x, wt, b, 0.01) * 1.3, "the oracle's")


@pytest.mark.parametrize("co,ci,k", R.WPREP)
def test_weight_prep_image_is_the_documented_permutation(co, ci, k):
    wt = torch.arange(co * ci * k * k, dtype=F64).reshape(co, ci, k, k) + 1
    (img, wsq), (mimg, _) = R.weight_prep(wt)
    assert img.shape == (k * k, ci // 4, co, 4) and wsq.shape == (co, ci) and torch.equal(img, mimg)
    for t in range(k * k):
        for i in range(ci):
            assert torch.equal(img[t, i // 4, :, i % 4], wt.reshape(co, ci, -1)[:, i, t])
    assert torch.equal(img.flatten().sort().values, wt.flatten())                    # a permutation


# ----------------------------------------------------------------------------- blur, upfirdn2d, bias_act, layouts
@pytest.mark.parametrize("h,w", R.BLUR_HW)
def test_blur_down_is_a_strided_fir_convolution_and_blur_down_bwd_its_adjoint(h, w):
    g = torch.Generator().manual_seed(h + w)
    c = 4
    x, gy = rnd(g, 2, h, w, c).requires_grad_(True), rnd(g, 2, h // 2, w // 2, c)
    k = torch.outer(torch.tensor([1.0, 3, 3, 1], dtype=F64), torch.tensor([1.0, 3, 3, 1], dtype=F64)) / 64
    want = F.conv2d(nchw(x), k[None, None].repeat(c, 1, 1, 1), padding=1, stride=2, groups=c)
    y, my = R.blur_down(x)
    agree(nchw(y), nchw(my), want.detach(), "blur_down")
    agree(nchw(y), nchw(my), O.upfirdn2d(nchw(x.detach()), FIR, down=2, padding=(1, 1, 1, 1)), "the oracle's")
    gx, mgx = R.blur_down_bwd(gy)
    agree(gx, mgx, torch.autograd.grad(want, x, nchw(gy))[0], "blur_down_bwd")
    lhs, rhs = (y * gy).sum().item(), (x.detach() * gx).sum().item()                 # <A x, y> == <x, A^T y>
    assert abs(lhs - rhs) <= TOL * (my * gy.abs()).sum().item()


@pytest.mark.parametrize("up,down,pad", R.UPFIRDN)
def test_upfirdn2d_is_the_oracles(up, down, pad):
    x = rnd(torch.Generator().manual_seed(up + down), 2, 3, 9, 7)
    f = R.upfirdn_filter().double()
    ref, mag = R.upfirdn2d(x, f, up, down, pad, float(up * up))
    agree(ref, mag, O.upfirdn2d(x, f, up=up, down=down, padding=pad, gain=float(up * up)), "upfirdn2d")
    assert not torch.allclose(ref, R.upfirdn2d(x, f.flip(0), up, down, pad, float(up * up))[0])
    assert not torch.allclose(ref, R.upfirdn2d(x, f.flip(1), up, down, pad, float(up * up))[0])


@pytest.mark.parametrize("dim", [1, 3])
@pytest.mark.parametrize("act", ["linear", "lrelu"])
def test_bias_act_is_the_oracles(dim, act):
    g = torch.Generator().manual_seed(dim)
    x, b = rnd(g, 2, 3, 4, 5), rnd(g, (2, 3, 4, 5)[dim])
    for clamp in (None, 0.7):
        ref, mag = R.bias_act(x, b, dim, act, 0.2, 1.4, clamp)
        agree(ref, mag, O.bias_act(x, b, act=act, alpha=0.2, gain=1.4, clamp=clamp, dim=dim), "bias_act")


def test_layout_transposes():
    x = rnd(torch.Generator().manual_seed(1), 2, 3, 4, 5)
    assert torch.equal(R.nchw_to_nhwc(x)[0], x.permute(0, 2, 3, 1)) and torch.equal(R.nhwc_to_nchw(R.nchw_to_nhwc(x)[0])[0], x)


# ----------------------------------------------------------------------------- the premise of the exact tier
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("c", R.UPFIR_C)
def test_exact_tier_preconditions_upfir_epilogue(c, half):
    launches = set()
    for hw in R.UPFIR_HW:
        for case in R.upfir_cases(c, hw, half, "exact"):
            kw, q = R.upfir_inputs(case)
            ref, mag = R.upfir_epilogue(**kw)
            (R.f16_precondition if half else R.exact_precondition)(ref, mag, q, str(case))
            R.upfir_planted(case, ref)
            launches.add(R.upfir_threads(case["B"], case["H"], case["W"], c) % 64 == 0)
        for case in R.upfir_cases(c, hw, half, "realistic"):
            if half and case["B"] == 1:
                kw, _ = R.upfir_inputs(case)
                R.f16_in_normal_range(R.upfir_epilogue(**kw)[0], str(case))
    assert launches == ({False, True} if c == 64 else {False})       # C = 64: full waves and a partial one publish y_absmax


def test_fir_strip_shapes_sit_on_the_strip_height():
    (_, _), (h1, _), (h2, _), _ = R.UPFIR_HW
    assert 2 * h1 == R.K_STRIP and 2 * h2 == R.K_STRIP + 2 and R.K_STRIP % 2 == 0


def test_exact_tier_preconditions_skip_and_torgb():
    for c in R.SKIP_C:
        for hw in R.SKIP_IMG:
            for b in R.SKIP_B:
                img, y, q = R.skip_inputs(c, hw, b, "exact")
                R.exact_precondition(*R.skip_upsample_add(img, y), q, "skip")
    for cin in R.TORGB_CIN_LDS + R.TORGB_CIN_REG:
        for hw in R.TORGB_HW:
            t, q = R.torgb_inputs(cin, 4, hw, 2, "exact")
            (out, pre), (mout, mpre) = R.torgb_small(t["x"], t["weight"], t["styles"], t["bias"], t["rgb_in"], R.torgb_clamp(cin, "exact"))
            R.exact_precondition(out, mout, q, "rgb_out")
            R.exact_precondition(pre, mpre, q, "y_pre")
            assert (pre.abs() > R.torgb_clamp(cin, "exact")).any() and (pre.abs() < R.torgb_clamp(cin, "exact")).any()          # the clamp bites, not everywhere
    for nparts in R.FINISH_NPARTS:
        for hw in R.TORGB_HW:
            t, q = R.finish_inputs(nparts, 3, hw, 2, "exact")
            (out, pre), (mout, mpre) = R.torgb_finish(t["part"], t["bias"], t["rgb_in"], R.CLAMP["exact"])
            R.exact_precondition(out, mout, q, "finish rgb_out")
            R.exact_precondition(pre, mpre, q, "finish y_pre")


def test_exact_tier_preconditions_styles_and_fc():
    for wd in R.STYLE_WDIM["exact"]:
        assert math.log2(math.sqrt(wd)) == round(math.log2(math.sqrt(wd)))
        for cin in R.STYLE_CIN:
            for b in R.STYLE_B:
                t, q = R.style_inputs(wd, cin, 65, b, "exact")
                (s, d), (ms, _) = R.styles_demod(t["ws"][:, 1], t["affine_w"], t["affine_b"], t["wsq"], t["style_gain"], t["eps"])
                R.exact_precondition(s, ms, q, "styles")
                assert torch.isfinite(d).all()
    for n in (1, 3, 32):
        for wd, (t, q) in R.style_batch_items(n, "exact"):
            (s, _), (ms, _) = R.styles_demod(t["ws"][:, 1], t["affine_w"], t["affine_b"], None, t["style_gain"], t["eps"])
            R.exact_precondition(s, ms, q, "batch styles")
    items = R.style_batch_items(32, "realistic")
    assert {wd for wd, _ in items} == {64, 260, 512} and items[1][1][0]["wsq"] is None and items[0][1][0]["wsq"] is not None
    assert len({t["ws"].shape[0] * t["affine_w"].shape[0] for _, (t, _) in items}) > 3
    for fin in R.FC_IN["exact"]:
        for fout, b, bias, act in R.fc_cases():
            t, q = R.fc_inputs(fin, fout, b, "exact")
            R.exact_precondition(*R.fully_connected(t["x"], t["weight"], t["bias"] if bias else None, t["lr_mul"], act, t["alpha"], t["gain"]),
                                 q, "fully_connected")


def test_exact_tier_preconditions_of_the_smaller_families():
    for co, ci, k in R.WPREP:
        wt = R.Draw("exact", co).t(co, ci, k, k)
        (_, wsq), (_, mwsq) = R.weight_prep(wt)
        R.exact_precondition(wsq, mwsq, 1.0, "wsq")
    for (h, w) in R.BLUR_HW:
        for c in R.BLUR_C:
            x = R.Draw("exact", h * w + c).t(2, h, w, c)
            R.exact_precondition(*R.blur_down(x), 1 / 64, "blur_down")
            R.exact_precondition(*R.blur_down_bwd(x[:, :h // 2, :w // 2]), 1 / 64, "blur_down_bwd")
    for up, down, pad in R.UPFIRDN:
        x, q = R.upfirdn_inputs(up, down, "exact")
        R.exact_precondition(*R.upfirdn2d(x, R.upfirdn_filter(), up, down, pad, float(up * up)), q, "upfirdn2d")
    for shape, dim in (((2, 3, 5, 7), 1), ((2, 5, 7, 8), 3)):
        x, b, dr, q = R.bias_act_inputs(shape, dim, "exact")
        for act in ("linear", "lrelu"):
            ref, mag = R.bias_act(x, b, dim, act, dr.alpha, dr.gain, R.CLAMP["exact"])
            R.exact_precondition(ref, mag, q, "bias_act")
            assert ref.flatten()[0].item() == 0.0 and ref.flatten()[1].item() == R.CLAMP["exact"]
            assert ref.flatten()[2].item() == (-R.CLAMP["exact"] * (dr.alpha if act == "lrelu" else 1.0))
