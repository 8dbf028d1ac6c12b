"""tests/backward_ref.py is autograd, not a transcript of the kernels: every reference function against float64
`torch.autograd.grad` of the forward operation it is the adjoint of, to 1e-12 of its magnitude; and the preconditions of the
exact tier of tests/test_gpu_backward_kernels.py (the reference of every integer case is an fp32 number, every partial sum stays
below 2^24 quanta), which need no GPU.

Inputs are drawn so that no activation lies within 1e-6 of 0 or of a clamp: autograd and the contract agree everywhere off those
edges; the edges themselves are fixed by the contract (include/hfagp.h) and tested on the GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import eg3d_oracle as O
from tests import backward_ref as R

F64 = torch.float64
TOL = 1e-12


def rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def agree(ref, mag, auto, what):
    err = (ref - auto).abs()
    assert bool((err <= TOL * mag).all()), f"{what}: |reference - autograd| = {err.max().item():.3e} (magnitude {mag.max().item():.3e})"
    assert auto.abs().max().item() > 0, f"{what}: the autograd value is identically 0 (the check would be empty)"


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- pointwise_bwd
@pytest.mark.parametrize("torgb", ["rgb96", "small1", "small3", "small4"])
@pytest.mark.parametrize("act", ["lrelu", "linear"])
def test_pointwise_bwd_is_autograd_of_a_producer_layer_and_its_consumers(torgb, act):
    """X = clamp(act(d * conv(x * s, W) + noise * strength + bias) * gain) feeding a modulated 3x3 conv, a toRGB (96 channels, or
    1 .. 4 channels with its own clamp), a direct term and an NCHW 3-channel term on channels 0..2; L = a random linear functional."""
    g = torch.Generator().manual_seed({"rgb96": 1, "small1": 2, "small3": 3, "small4": 4}[torgb] + (10 if act == "linear" else 0))
    b, cin, c, h, w = 2, 5, 8, 5, 7
    gain, alpha, clamp, cs = math.sqrt(2.0), 0.2, 1.5, 1.0
    craw = F.conv2d(rnd(g, b, cin, h, w) * rnd(g, b, cin)[:, :, None, None], rnd(g, c, cin, 3, 3) / 4, padding=1).requires_grad_(True)
    d = (torch.rand(b, c, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    bias, strength, noise = rnd(g, c).requires_grad_(True), torch.tensor(0.1, dtype=F64, requires_grad=True), rnd(g, h, w)
    pre = craw * d[:, :, None, None] + noise * strength + bias[None, :, None, None]
    X = (O.bias_act(pre, None, act=act, alpha=alpha, gain=gain)).clamp(-clamp, clamp)
    assert ((X.abs() > 1e-6) & ((X.abs() - clamp).abs() > 1e-6) | (X.abs() == clamp)).all() and (pre.abs() > 1e-6).all()
    assert (X.abs() == clamp).any() and (X < 0).any()                     # both the mask and the alpha branch are exercised

    s_conv, s_rgb = rnd(g, b, c).requires_grad_(True), rnd(g, b, c).requires_grad_(True)
    xs_conv = X * s_conv[:, :, None, None]
    L = (F.conv2d(xs_conv, rnd(g, 6, c, 3, 3), padding=1) * rnd(g, b, 6, h, w)).sum()
    g_direct, g3 = rnd(g, b, c, h, w), rnd(g, b, 3, h, w)
    L = L + (X * g_direct).sum() + (X[:, :3] * g3).sum()
    kw = dict(g_direct=nhwc(g_direct), g_nchw3_a=g3, s_conv=s_conv)
    if torgb == "rgb96":
        xs_rgb = X * s_rgb[:, :, None, None]
        L = L + (F.conv2d(xs_rgb, rnd(g, 96, c, 1, 1)) * rnd(g, b, 96, h, w)).sum()
    else:
        co = int(torgb[-1])
        w_small = rnd(g, b, co, c).requires_grad_(True)                 # one copy per sample: sums[b][6+c] is per sample
        y_small = torch.einsum("bihw,boi->bohw", X * s_rgb[:, :, None, None], w_small)
        assert ((y_small.abs() - cs).abs() > 1e-6).all() and (y_small.abs() > cs).any()
        g_small = rnd(g, b, co, h, w)
        L = L + (y_small.clamp(-cs, cs) * g_small).sum()
    wanted = [craw, d, bias, strength, s_conv, s_rgb, xs_conv] + ([xs_rgb] if torgb == "rgb96" else [w_small])
    grads = torch.autograd.grad(L, wanted)
    a_craw, a_d, a_bias, a_strength, a_sconv, a_srgb, dxs_conv, last = grads
    kw.update(dxs_conv=nhwc(dxs_conv))
    if torgb == "rgb96":
        kw.update(dxs_rgb=nhwc(last), s_rgb=s_rgb)
    else:
        # (the kernel's w_rgb_small is shared by the batch: the reference is run per sample)
        pass
    prod = dict(dcoef=d, bias=bias, noise=noise, noise_strength=strength.item(), act=act, alpha=alpha, gain=gain, clamp=clamp)

    def run(sl):
        k = {n: (t[sl] if (torch.is_tensor(t) and t.dim() > 1 and t.shape[0] == b) else t) for n, t in kw.items()}
        p = dict(prod, dcoef=d[sl])
        if torgb != "rgb96":
            k.update(g_rgb_small=g_small[sl], y_rgb_small=y_small[sl], clamp_rgb_small=cs, w_rgb_small=w_small[sl][0], s_small=s_rgb[sl])
        return R.pointwise_bwd(nhwc(X)[sl], producer=p, **k)

    outs = [run(slice(i, i + 1)) for i in range(b)]
    g_out = torch.cat([o[0][0] for o in outs])
    sums = torch.cat([o[0][1] for o in outs])
    m_out = torch.cat([o[1][0] for o in outs])
    msums = torch.cat([o[1][1] for o in outs])
    agree(g_out, m_out, nhwc(a_craw), "g_out = dL/d(raw conv output)")
    agree(sums[:, 0], msums[:, 0], a_sconv, "sums[0] = dL/d s_conv")
    agree(sums[:, 3], msums[:, 3], a_d, "sums[3] = dL/d d")
    agree(sums[:, 4].sum(0), msums[:, 4].sum(0), a_bias, "sums[4] = dL/d bias")
    agree(sums[:, 5].sum(), msums[:, 5].sum(), a_strength, "sum_c sums[5] = dL/d strength")
    if torgb == "rgb96":
        agree(sums[:, 1], msums[:, 1], a_srgb, "sums[1] = dL/d s_rgb")
        assert not sums[:, 2].any() and not sums[:, 6:].any()
    else:
        agree(sums[:, 2], msums[:, 2], a_srgb, "sums[2] = dL/d s_small")
        for k in range(co):
            agree(sums[:, 6 + k] * s_rgb, msums[:, 6 + k] * s_rgb.abs(), last[:, k], f"sums[{6 + k}] * s = dL/d w_small[{k}]")
        assert not sums[:, 1].any() and not sums[:, 6 + co:].any()
    # the caller-masked form is the same operation
    if torgb != "rgb96":
        masked = g_small * (y_small.abs() < cs)
        k = dict(kw, g_rgb_small=masked[:1], w_rgb_small=w_small[0], s_small=s_rgb[:1])
        k = {n: (t[:1] if (torch.is_tensor(t) and t.dim() > 1 and t.shape[0] == b) else t) for n, t in k.items()}
        (g1, s1), _ = R.pointwise_bwd(nhwc(X)[:1], producer=dict(prod, dcoef=d[:1]), **k)
        assert torch.equal(g1, outs[0][0][0]) and torch.equal(s1, outs[0][0][1])
    # rows 4 .. 9 are the parameter gradients: absent without param_grads
    (_, s0), _ = R.pointwise_bwd(nhwc(X), producer=prod, param_grads=False, dxs_conv=kw["dxs_conv"], s_conv=s_conv)
    assert not s0[:, 4:].any() and s0[:, 3].any()


# ----------------------------------------------------------------------------- styles -> latent, affine layer
@pytest.mark.parametrize("demod", [True, False])
def test_style_bwd_and_affine_grad_are_autograd_through_the_demodulation_and_the_affine_layer(demod):
    g = torch.Generator().manual_seed(5 + demod)
    b, cin, cout, wd, sg, eps = 3, 7, 5, 9, 1 / math.sqrt(7), 1e-8
    lat = rnd(g, b, wd).requires_grad_(True)
    A, ab = rnd(g, cin, wd).requires_grad_(True), rnd(g, cin).requires_grad_(True)
    wsq = rnd(g, cout, cin, 3, 3).square().sum(dim=(2, 3))
    raw = O.fully_connected(lat, A, ab)
    styles = raw * sg
    dcoef = (styles.square() @ wsq.T + eps).rsqrt()
    ds, dd, dw0 = rnd(g, b, cin), rnd(g, b, cout), rnd(g, b, wd)
    L = (styles * ds).sum() + ((dcoef * dd).sum() if demod else 0.0)
    a_raw, a_lat, a_A, a_ab = torch.autograd.grad(L, [raw, lat, A, ab])
    args = (ds, dd, styles, dcoef, wsq) if demod else (ds, None, styles, None, None)
    (dstot, dw), (mstot, mdw) = R.style_bwd(*args, A, sg)
    agree(dstot, mstot, a_raw, "dstot = dL/d(affine output)")
    agree(dw, mdw, a_lat, "dw = dL/d ws")
    (_, dw1), (_, mdw1) = R.style_bwd(*args, A, sg, dw0=dw0)
    agree(dw1 - dw0, mdw1, a_lat, "dw accumulated")
    dA0, db0 = rnd(g, cin, wd), rnd(g, cin)
    (dA, db), (mA, mb) = R.affine_grad(dstot, lat, dA0, db0)
    agree(dA - dA0, mA, a_A, "dA")
    agree(db - db0, mb, a_ab, "db")


# ----------------------------------------------------------------------------- weight gradient with the demodulation term
@pytest.mark.parametrize("mode", ["3x3", "up", "1x1"])
def test_conv_wgrad_is_autograd_of_the_demodulated_convolution(mode):
    """y = d * conv(x * s, W), d = rsqrt(sum (W s)^2 + eps): dL/dW = conv-weight-gradient(x s, g) - W sum_b dd d^3 s^2 with
    g = dL/d(raw conv output) and dd = dL/d d; the up-sampling mode through the oracle's transposed conv + FIR."""
    g = torch.Generator().manual_seed({"3x3": 11, "up": 12, "1x1": 13}[mode])
    b, cin, cout, h, w, k = 2, 4, 6, 5, 3, (1 if mode == "1x1" else 3)
    x, s = rnd(g, b, cin, h, w), rnd(g, b, cin)
    W = rnd(g, cout, cin, k, k).requires_grad_(True)
    xs = x * s[:, :, None, None]
    raw = O._conv_up2(xs, W, O.fir_kernel().double()) if mode == "up" else F.conv2d(xs, W, padding=k // 2)
    dcoef = ((W[None] * s[:, None, :, None, None]).square().sum(dim=(2, 3, 4)) + 1e-8).rsqrt()
    cot = rnd(g, *raw.shape)
    L = (raw * dcoef[:, :, None, None] * cot).sum()
    a_W, a_raw, a_d = torch.autograd.grad(L, [W, raw, dcoef])
    gy = nhwc(a_raw)
    gin = R.upfir_bwd(gy)[0] if mode == "up" else gy
    dw, mdw = R.conv_wgrad(nhwc(x), s, gin, W, mode, dd=a_d, dcoef=dcoef)
    agree(dw, mdw + 1e-30, a_W, "dweight")
    plain, _ = R.conv_wgrad(nhwc(x), s, gin, W, mode)
    assert (plain - dw).abs().max().item() > 1e-3                         # the demodulation term is part of the value
    dw0 = rnd(g, *W.shape)
    acc, macc = R.conv_wgrad(nhwc(x), s, gin, W, mode, dd=a_d, dcoef=dcoef, dw0=dw0)
    agree(acc - dw0, macc, a_W, "dweight accumulated")


# ----------------------------------------------------------------------------- FIR adjoints, bias_act, layout
@pytest.mark.parametrize("h,w", R.FIR_HW)
def test_upfir_bwd_and_upsample2d_bwd_are_autograd_of_the_oracle_filters(h, w):
    g = torch.Generator().manual_seed(h * 31 + w)
    b, c, f = 2, 4, O.fir_kernel().double()
    yt = rnd(g, b, c, 2 * h + 1, 2 * w + 1).requires_grad_(True)
    y = O.upfirdn2d(yt, f, padding=(1, 1, 1, 1), gain=4.0)
    assert y.shape[2:] == (2 * h, 2 * w)
    cot = rnd(g, *y.shape)
    (a_yt,) = torch.autograd.grad((y * cot).sum(), [yt])
    gph, mph = R.upfir_bwd(nhwc(cot))
    assert gph.shape == (2, 2, b, h + 1, w + 1, c)
    full = gph.permute(2, 3, 0, 4, 1, 5).reshape(b, 2 * h + 2, 2 * w + 2, c)         # g_yt[2m+a][2n+b]
    mfull = mph.permute(2, 3, 0, 4, 1, 5).reshape(b, 2 * h + 2, 2 * w + 2, c)
    agree(full[:, :2 * h + 1, :2 * w + 1], mfull[:, :2 * h + 1, :2 * w + 1], nhwc(a_yt), "g_yt")
    assert not full[:, 2 * h + 1].any() and not full[:, :, 2 * w + 1].any()          # the padding row / column of the parity images

    img = rnd(g, b, c, h, w).requires_grad_(True)
    up = O.upsample2d(img, f)
    cot = rnd(g, *up.shape)
    (a_img,) = torch.autograd.grad((up * cot).sum(), [img])
    for channels_last in (False, True):
        got, mag = R.upsample2d_bwd(nhwc(cot) if channels_last else cot, channels_last)
        agree(got, mag, nhwc(a_img) if channels_last else a_img, f"upsample2d_bwd channels_last={channels_last}")


@pytest.mark.parametrize("act", sorted(["linear", "lrelu"]))
@pytest.mark.parametrize("clamp", [None, 1.5])
def test_bias_act_bwd_is_autograd_of_the_oracle_bias_act(act, clamp):
    from hfa_gp_amd import ops
    assert sorted(ops._ACT) == ["linear", "lrelu"]                        # every activation the library accepts
    g = torch.Generator().manual_seed(3)
    x = rnd(g, 2, 6, 5, 4).requires_grad_(True)
    alpha, gain = 0.2, math.sqrt(2.0)
    y = O.bias_act(x, rnd(g, 6), act=act, alpha=alpha, gain=gain, clamp=clamp)
    assert (y.abs() > 1e-6).all() and (clamp is None or ((y.abs() == clamp).any() and (((y.abs() - clamp).abs() > 1e-6) | (y.abs() == clamp)).all()))
    dy = rnd(g, *y.shape)
    (a_x,) = torch.autograd.grad((y * dy).sum(), [x])
    dx, mag = R.bias_act_bwd(dy, y, act, alpha, gain, clamp)
    agree(dx, mag, a_x, "dx")


def test_planes_to_nhwc_and_bias_noise_grads_are_what_their_contracts_say():
    g = torch.Generator().manual_seed(8)
    pm = rnd(g, 2, 3, 3, 5, 4)
    y, _ = R.planes_to_nhwc(pm)
    for p in range(3):
        assert torch.equal(y[..., 4 * p:4 * p + 4], pm[:, p])
    bias = rnd(g, 6).requires_grad_(True)
    strength = torch.tensor(0.3, dtype=F64, requires_grad=True)
    g_pre, noise = rnd(g, 2, 4, 5, 6), rnd(g, 4, 5)
    L = (g_pre * (bias + noise[None, :, :, None] * strength)).sum()
    a_b, a_s = torch.autograd.grad(L, [bias, strength])
    sums = torch.zeros(2, 10, 6, dtype=F64)
    sums[:, 4], sums[:, 5] = g_pre.sum(dim=(1, 2)), (g_pre * noise[None, :, :, None]).sum(dim=(1, 2))
    db0, dn0 = rnd(g, 6), rnd(g, 1)
    (db, dn), (mb, mn) = R.bias_noise_grads(sums, db0, dn0)
    agree(db - db0, mb, a_b, "dbias")
    agree(dn - dn0, mn, a_s.reshape(1), "dnoise")
    assert R.bias_noise_grads(sums, None, None)[0] == (None, None)


# ----------------------------------------------------------------------------- the exact tier's preconditions
def test_pointwise_cases_cover_every_variant_and_operand():
    R.pointwise_coverage(R.pointwise_cases())


@pytest.mark.parametrize("case", R.pointwise_cases(), ids=lambda c: f"{c['id']}-C{c['C']}")
def test_exact_tier_precondition_pointwise(case):
    kw, q = R.pointwise_inputs(case, "exact")
    (g_out, sums), (m_out, msums) = R.pointwise_bwd(**kw)
    R.exact_precondition(g_out, m_out, q, "g_out")
    R.exact_precondition(sums, msums, q, "sums")
    x = kw["x"]
    if x.numel() >= 3 and case["producer"]:
        assert (x == 0).any() and (x.abs() == R.PW_CLAMP["exact"]).any()              # the planted edges
    if case["small"] and case["mask_in_kernel"]:
        assert (kw["y_rgb_small"].abs() == kw["clamp_rgb_small"]).any()


@pytest.mark.parametrize("case", R.style_cases("exact"), ids=lambda c: f"{c['Cin']}-{c['Cout']}-{c['w_dim']}")
def test_exact_tier_precondition_style(case):
    t, (q_s, q_w) = R.style_inputs(case, "exact")
    assert math.sqrt(case["w_dim"]) == int(math.sqrt(case["w_dim"])) and case["w_dim"] in (16, 64, 256)
    (dstot, dw), (mstot, mdw) = R.style_bwd(t["ds"], t["dd"], t["styles"], t["dcoef"], t["wsq"], t["affine_w"], t["style_gain"],
                                            dw0=t["dw0"] if case["accumulate"] else None)
    R.exact_precondition(dstot, mstot, q_s, "dstot")
    R.exact_precondition(dw, mdw, q_w, "dw")


@pytest.mark.parametrize("shape,prec,mode", R.wgrad_cases())
def test_exact_tier_precondition_conv_wgrad(shape, prec, mode):
    t, q = R.wgrad_inputs(shape, mode, "exact")
    g, mg = R.upfir_bwd(t["gy"]) if mode == "up" else (t["gy"].double(), t["gy"].double().abs())
    R.exact_precondition(g, mg, q, "g")
    dw, mdw = R.conv_wgrad(t["x"], t["styles"], g, t["weight"], mode, dd=t["sums"][:, 3], dcoef=t["dcoef"], dw0=t["dw0"])
    R.exact_precondition(dw, mdw, q, "dweight")
    # bf16x3: every operand of the matrix pipe — x * styles, g — is ONE bf16 part (at most 8 significant bits)
    for v in (t["x"] * t["styles"][:, None, None, :], g.float()):
        assert torch.equal(v.bfloat16().float(), v.float())


@pytest.mark.parametrize("h,w", R.FIR_HW)
def test_exact_tier_precondition_fir_adjoints_and_affine(h, w):
    for c in R.FIR_C:
        gy = R.Draw("exact", 100 * c + h).t(2, 2 * h, 2 * w, c)
        R.exact_precondition(*R.upfir_bwd(gy), 1 / 16, "upfir_bwd")
        R.exact_precondition(*R.upsample2d_bwd(gy, True), 1 / 16, "upsample2d_bwd")
    ws = R.Draw("exact", 1).t(3, 14, 64)
    for i in range(8):
        dstot, wrow, dA0, db0 = R.affine_inputs(i, "exact", ws)
        (dA, db), (mA, mb) = R.affine_grad(dstot, wrow, dA0, db0)
        R.exact_precondition(dA, mA, 1 / 8, "dA")
        R.exact_precondition(db, mb, 1.0, "db")


@pytest.mark.parametrize("layout", ["one_launch", "two_launches", "straddle"])
def test_exact_tier_precondition_style_batch(layout):
    dw0, items, rows = R.style_batch(layout, "exact")
    for _, _, _, r_s, m_s, q_s in items:
        R.exact_precondition(r_s, m_s, q_s, "dstot")
    for v, m, _ in rows.values():
        R.exact_precondition(v, m, 0.125 * 0.25 / math.sqrt(dw0.shape[2]), "d_ws row")
    order = sorted(range(len(items)), key=lambda i: items[i][2])
    if layout != "one_launch":                       # the cut after 32 sorted items: between two rows / inside row 16
        assert (items[order[31]][2] == items[order[32]][2]) == (layout == "straddle")
    else:
        assert len(items) <= 32 and max(sum(1 for it in items if it[2] == r) for r in rows) >= 3


def test_exact_tier_precondition_bias_noise_grads_and_bias_act_bwd():
    for i in range(35):
        b, c = 1 + i % 3, (4, 32, 96, 512, 260)[i % 5]
        dr = R.Draw("exact", 500 + i)
        vals, mags = R.bias_noise_grads(dr.t(b, 10, c), dr.t(c), dr.t(1))
        for v, m in zip(vals, mags):
            R.exact_precondition(v, m, 1.0, "dbias / dnoise")
    dr = R.Draw("exact", 77)
    dy, y = dr.t(3, 5, 7, 6), dr.t(3, 5, 7, 6)
    for act in ("linear", "lrelu"):
        for clamp in (None, R.PW_CLAMP["exact"]):
            R.exact_precondition(*R.bias_act_bwd(dy, y, act, dr.alpha, dr.gain, clamp), 0.25, "dx")
