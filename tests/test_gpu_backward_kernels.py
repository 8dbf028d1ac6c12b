"""The backward streaming kernels (csrc/backward.hip) and the weight-gradient kernels (csrc/wgrad.hip, wgrad_bf16.hip) against
the float64 reference of tests/backward_ref.py, one entry point at a time, in two tiers:

  exact      integer inputs and power-of-two scalars: bit for bit (indexing, masks, variant dispatch, tails; no tolerance);
             every case asserts its precondition (backward_ref.exact_precondition), which tests/test_backward_ref_cpu.py also
             runs without a GPU.
  realistic  randn inputs: |got - ref| <= (N + 16) 2^-24 magnitude for every element, N = the number of terms summed into it.
             The bound is derived (backward_ref.bound), never measured; the worst error / bound per family is printed and
             recorded in profiles/backward_kernels_f64.md.  bf16x3 weight gradients: the class bar of
             test_gpu_backward.py::test_conv_weight_gradient_split_bf16 (atol 1e-4 max|ref|, rtol 1e-4).

N where one output is a sum of sums: dw = sum_i dstot_i A_ik with dstot_i itself a sum over Cout — an error of (Cout + 16) u in
every dstot_i and (Cin + 16) u in the outer sum add up to (Cin + Cout + 32) u of dw's magnitude, per layer on the row.

Needs an MI355X:  python -m pytest tests/test_gpu_backward_kernels.py -m gpu"""
import math

import pytest
import torch

from tests import backward_ref as R

pytestmark = pytest.mark.gpu

TIERS = ("exact", "realistic")
WORST = {}                     # family -> largest error / bound seen in the realistic tier


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    yield torch.device("cuda:0")
    for family in sorted(WORST):
        print(f"\nworst error / bound [{family}]: {WORST[family]:.4f}", end="")


def to_dev(v, dev):
    if torch.is_tensor(v):
        return v.to(dev)
    if isinstance(v, dict):
        return {k: to_dev(t, dev) for k, t in v.items()}
    return v


def hold(tier, family, got, ref, mag, n, what):
    """Exact tier: bit for bit.  Realistic tier: every element within (n + 16) u of its magnitude."""
    assert got.shape == ref.shape and got.dtype == torch.float32, what
    if tier == "exact":
        bad = (got.double().cpu() != ref).sum().item()
        assert bad == 0, f"{what}: {bad} of {ref.numel()} elements differ from the float64 reference"
        return
    ratio = R.worst_ratio(got, ref, mag, n)
    print(f"{family} {what}: error / bound = {ratio:.4f} (N = {n})")
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: error is {ratio:.3f} of the bound (N = {n})"


# ----------------------------------------------------------------------------- hfagp_pointwise_bwd
@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("case", R.pointwise_cases(), ids=lambda c: "{id}-C{C}-{H}x{W}-B{B}-{chunks}".format(**c))
def test_pointwise_bwd(dev, monkeypatch, case, tier):
    """g_out and all ten reduction rows of every kernel variant (SMALL x PG x PACKED) at every C that admits it, over the operand
    combinations of backward_ref.pointwise_cases: chunk counts forced through ops._DEV_PW_CHUNKS (one, one per pixel, trailing
    chunks without a pixel), the immediate and the deferred reduction, planted X == 0, |X| == clamp and |y| == clamp_rgb_small."""
    from hfa_gp_amd import ops
    kw, q = R.pointwise_inputs(case, tier)
    (r_out, r_sums), (m_out, m_sums) = R.pointwise_bwd(**kw)
    if tier == "exact":
        R.exact_precondition(r_out, m_out, q, "g_out")
        R.exact_precondition(r_sums, m_sums, q, "sums")
    monkeypatch.setattr(ops, "_DEV_PW_CHUNKS", R.pointwise_chunks(case))
    deferred = [] if case["deferred"] else None
    g_out, sums = ops.pointwise_bwd(deferred=deferred, **to_dev(kw, dev))
    if deferred is not None:
        partial = deferred[0][0]
        ops.reduce_partials_batch(deferred)
    if case["chunks"] == "empty" and deferred is not None:
        assert partial.shape[1] == 7 and not partial[:, 5:].any()                    # chunks 5 and 6 hold no pixel
    hold(tier, "pointwise_bwd g_out", g_out, r_out, m_out, 1, "g_out")
    hold(tier, "pointwise_bwd sums", sums, r_sums, m_sums, case["H"] * case["W"], "sums")


# ----------------------------------------------------------------------------- hfagp_style_bwd
def _style_ref(t, accumulate):
    return R.style_bwd(t["ds"], t["dd"], t["styles"], t["dcoef"], t["wsq"], t["affine_w"], t["style_gain"],
                       dw0=t["dw0"] if accumulate else None)


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("idx", range(20))
def test_style_bwd(dev, idx, tier):
    """dstot and the d ws row of one affine layer: Cin on both sides of the dw kernel's 32-row unroll, Cout around the 64-lane
    stride of the ds kernel, dd present and absent, overwrite and accumulate into a non-zero row of a wider d_ws."""
    from hfa_gp_amd import ops
    case = R.style_cases(tier)[idx]
    t, (q_s, q_w) = R.style_inputs(case, tier)
    (r_s, r_w), (m_s, m_w) = _style_ref(t, case["accumulate"])
    if tier == "exact":
        R.exact_precondition(r_s, m_s, q_s, "dstot")
        R.exact_precondition(r_w, m_w, q_w, "dw")
    d = to_dev(t, dev)
    d_ws = torch.full((case["B"], 3, case["w_dim"]), 7.0, device=dev)
    d_ws[:, 1] = d["dw0"]
    dstot = ops.style_bwd(d["ds"], d["dd"], d["styles"], d["dcoef"], d["wsq"], d["affine_w"], d_ws[:, 1], t["style_gain"],
                          accumulate=case["accumulate"])
    assert (d_ws[:, 0] == 7.0).all() and (d_ws[:, 2] == 7.0).all()                   # the neighbouring rows are not touched
    hold(tier, "style_bwd dstot", dstot, r_s, m_s, case["Cout"] + 1, "dstot")
    hold(tier, "style_bwd dw", d_ws[:, 1].contiguous(), r_w, m_w, case["Cin"] + case["Cout"] + 17, "dw")


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("layout", ["one_launch", "two_launches", "straddle"])
def test_style_bwd_batch(dev, layout, tier):
    """hfagp_style_batch_bwd through ops.style_bwd_batch: ds / dd as strided row views of [B, 10, C] reduction tensors, several
    layers on one ws row, 34 items (two launches, cut between two rows), and 34 items whose row 16 would straddle the cut (the
    per-layer fallback) — every dstot and every d_ws row against the reference."""
    from hfa_gp_amd import ops
    dw0, ref_items, rows = R.style_batch(layout, tier)
    b, wd = dw0.shape[0], dw0.shape[2]
    d_ws = dw0.to(dev)
    items = []
    for t, case, row, _, _, _ in ref_items:
        d = to_dev(t, dev)
        sums_in, sums_out = torch.full((b, 10, case["Cin"]), 3.0, device=dev), torch.full((b, 10, case["Cout"]), 5.0, device=dev)
        sums_in[:, 0] = d["ds"]
        dd = None
        if case["dd"]:
            sums_out[:, 3] = d["dd"]
            dd = sums_out[:, 3]
        assert not sums_in[:, 0].is_contiguous()
        items.append((sums_in[:, 0], dd, d["styles"], d["dcoef"], d["wsq"], d["affine_w"], row, t["style_gain"]))
    dstots = ops.style_bwd_batch(items, d_ws)
    for i, (dstot, (_, case, _, r_s, m_s, q_s)) in enumerate(zip(dstots, ref_items)):
        if tier == "exact":
            R.exact_precondition(r_s, m_s, q_s, f"dstot of item {i}")
        hold(tier, "style_bwd_batch dstot", dstot, r_s, m_s, case["Cout"] + 1, f"dstot of item {i}")
    for r, (v, m, terms) in rows.items():
        if tier == "exact":
            R.exact_precondition(v, m, 0.125 * 0.25 / math.sqrt(wd), f"d_ws row {r}")
        hold(tier, "style_bwd_batch dw", d_ws[:, r].contiguous(), v, m, terms, f"d_ws row {r}")


# ----------------------------------------------------------------------------- affine layer, bias and noise strength
@pytest.mark.parametrize("tier", TIERS)
def test_affine_grad_and_its_batch(dev, tier):
    """dA += dstot^T w / sqrt(w_dim), db += sum_b dstot for 35 layers in two launches, and the per-layer entry point, each
    against the reference (not against each other): w a strided row view of ws, non-zero targets."""
    from hfa_gp_amd import ops
    ws = R.Draw(tier, 1).t(3, 14, 64)
    ws_d = ws.to(dev)
    items, want = [], []
    for i in range(35):
        dstot, wrow, dA0, db0 = R.affine_inputs(i, tier, ws)
        want.append(R.affine_grad(dstot, wrow, dA0, db0))
        items.append((dstot.to(dev), ws_d[:, i % 14], dA0.to(dev), db0.to(dev)))
        assert not items[-1][1].is_contiguous()
    single = [(d.clone(), w, a.clone(), c.clone()) for d, w, a, c in items[:4]]
    ops.affine_grad_batch(items)
    for d, w, a, c in single:
        ops.affine_grad(d, w, a, c)
    for i, (it, ((dA, db), (mA, mb))) in enumerate(zip(items + single, want + want[:4])):
        if tier == "exact":
            R.exact_precondition(dA, mA, 1 / 8, "dA")
            R.exact_precondition(db, mb, 1.0, "db")
        hold(tier, "affine_grad dA", it[2], dA, mA, 3 + 1, f"dA of item {i}")
        hold(tier, "affine_grad db", it[3], db, mb, 3 + 1, f"db of item {i}")


@pytest.mark.parametrize("tier", TIERS)
def test_bias_noise_grads(dev, tier):
    """dbias[c] += sum_b sums[b][4][c], dnoise += sum_bc sums[b][5][c] for 35 layers (two launches); either target absent in
    some items; non-zero targets."""
    from hfa_gp_amd import ops
    items, want = [], []
    for i in range(35):
        b, c = 1 + i % 3, (4, 32, 96, 512, 260)[i % 5]
        dr = R.Draw(tier, 500 + i)
        sums, db0, dn0 = dr.t(b, 10, c), (None if i % 5 == 0 else dr.t(c)), (None if i % 4 == 0 else dr.t(1))
        want.append(R.bias_noise_grads(sums, db0, dn0) + (b, c))
        if tier == "exact":
            for r, m in zip(*want[-1][:2]):
                if r is not None:
                    R.exact_precondition(r, m, 1.0, "dbias / dnoise")
        items.append((sums.to(dev), to_dev(db0, dev), to_dev(dn0, dev)))
    assert any(db is None for _, db, _ in items) and any(dn is None for _, _, dn in items)
    ops.bias_noise_grads(items)
    for i, ((_, db, dn), ((r_b, r_n), (m_b, m_n), b, c)) in enumerate(zip(items, want)):
        if db is not None:
            hold(tier, "bias_noise_grads dbias", db, r_b, m_b, b + 1, f"dbias of item {i}")
        if dn is not None:
            hold(tier, "bias_noise_grads dnoise", dn, r_n, m_n, b * c + 1, f"dnoise of item {i}")


# ----------------------------------------------------------------------------- layout, bias_act, FIR adjoints
@pytest.mark.parametrize("cp", R.PLANES_CP)
@pytest.mark.parametrize("b", [1, 3])
def test_planes_to_nhwc_is_the_permutation(dev, b, cp):
    from hfa_gp_amd import ops
    pm = torch.randn(b, 3, 5, 7, cp, generator=torch.Generator().manual_seed(cp + b))
    got = ops.planes_to_nhwc(pm.to(dev))
    assert torch.equal(got.cpu(), pm.permute(0, 2, 3, 1, 4).reshape(b, 5, 7, 3 * cp))
    assert torch.equal(got.cpu().double(), R.planes_to_nhwc(pm)[0])


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("clamp", [None, "on"])
@pytest.mark.parametrize("act", ["linear", "lrelu"])
def test_bias_act_bwd(dev, act, clamp, tier):
    """ops.bias_act_bwd called directly, every activation the library accepts, clamp on and off, y planted at 0 (slope alpha)
    and at +-clamp (masked)."""
    from hfa_gp_amd import ops
    assert sorted(ops._ACT) == ["linear", "lrelu"]
    dr = R.Draw(tier, 77)
    cl = None if clamp is None else R.PW_CLAMP[tier]
    dy, y = dr.t(3, 5, 7, 6), dr.t(3, 5, 7, 6)
    y.view(-1)[0], y.view(-1)[1], y.view(-1)[2] = 0.0, R.PW_CLAMP[tier], -R.PW_CLAMP[tier]
    dy.view(-1)[:3] = 1.0
    ref, mag = R.bias_act_bwd(dy, y, act, dr.alpha, dr.gain, cl)
    assert ref.view(-1)[0].item() == dr.gain * (dr.alpha if act == "lrelu" else 1.0)
    assert cl is None or (ref.view(-1)[1].item() == 0.0 and ref.view(-1)[2].item() == 0.0)
    if tier == "exact":
        R.exact_precondition(ref, mag, 0.25, "dx")
    got = ops.bias_act_bwd(dy.to(dev), y.to(dev), act, dr.alpha, dr.gain, cl)
    hold(tier, "bias_act_bwd", got, ref, mag, 1, "dx")


@pytest.mark.parametrize("c", R.FIR_C)
@pytest.mark.parametrize("h,w", R.FIR_HW)
def test_upfir_bwd_and_upsample2d_bwd(dev, h, w, c):
    """The adjoints of the two FIR up-samplers (dyadic taps: the exact tier only): one pixel, ragged strips, both layouts of
    upsample2d_bwd."""
    from hfa_gp_amd import ops
    for b in (1, 2):
        gy = R.Draw("exact", 100 * c + h + b).t(b, 2 * h, 2 * w, c)
        ref, mag = R.upfir_bwd(gy)
        R.exact_precondition(ref, mag, 1 / 16, "upfir_bwd")
        hold("exact", "", ops.upfir_bwd(gy.to(dev)), ref, mag, 16, "upfir_bwd")
        for channels_last in (True, False):
            g = gy if channels_last else gy.permute(0, 3, 1, 2).contiguous()
            ref, mag = R.upsample2d_bwd(g, channels_last)
            R.exact_precondition(ref, mag, 1 / 16, "upsample2d_bwd")
            hold("exact", "", ops.upsample2d_bwd(g.to(dev), channels_last), ref, mag, 16, f"upsample2d_bwd channels_last={channels_last}")


# ----------------------------------------------------------------------------- hfagp_conv_wgrad
_MODE = {"3x3": "CONV3X3", "up": "CONVT3X3_UP2", "1x1": "CONV1X1"}


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("ksplit", ["one", "library", "tiles"])
@pytest.mark.parametrize("shape,prec,mode", R.wgrad_cases(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_conv_wgrad(dev, shape, prec, mode, ksplit, tier):
    """dweight with the demodulation term (dd a strided row view of a [B, 10, Cout] reduction tensor, dcoef), overwriting and
    accumulating into a non-zero `out`, at one split-K slab, the library's choice and one slab per position tile.  The fp32
    MFMA path and — in the exact tier, where a small integer is one bf16 part — the split-bf16 path equal the reference bit for
    bit; realistic tier: the derived bound (fp32) or the split-bf16 class bar, and the split kernel must have run."""
    from hfa_gp_amd import ops
    b, h, w, cin, cout = shape
    t, q = R.wgrad_inputs(shape, mode, tier)
    d = to_dev(t, dev)
    g = ops.upfir_bwd(d["gy"]) if mode == "up" else d["gy"]           # (the parity images are this kernel's INPUT: taken as given)
    dd = d["sums"][:, 3]
    assert dd.stride(0) == 10 * cout                                  # row 3 of [B, 10, Cout], read in place
    ks = {"one": 1, "library": None, "tiles": R.wgrad_position_tiles(shape, prec, mode)}[ksplit]
    op_mode = getattr(ops, _MODE[mode])
    n = b * h * w + b + 1
    for dw0 in (None, t["dw0"]):
        ref, mag = R.conv_wgrad(t["x"], t["styles"], g.cpu(), t["weight"], mode, dd=t["sums"][:, 3], dcoef=t["dcoef"], dw0=dw0)
        out = None if dw0 is None else dw0.to(dev)
        got = ops.conv_wgrad(d["x"], d["styles"], g, d["weight"], op_mode, dd=dd, dcoef=d["dcoef"], precision=prec, ksplit=ks, out=out)
        assert out is None or got.data_ptr() == out.data_ptr()
        what = f"dweight ({'overwritten' if dw0 is None else 'accumulated'})"
        if tier == "exact":
            R.exact_precondition(ref, mag, q, what)
            hold(tier, "", got, ref, mag, n, what)
        elif prec == "fp32":
            hold(tier, "conv_wgrad fp32", got, ref, mag, n, what)
        else:
            err = (got.double().cpu() - ref).abs()
            bar = 1e-4 * ref.abs().max() + 1e-4 * ref.abs()
            ratio = (err / bar).max().item()
            print(f"conv_wgrad bf16x3 {what}: error / class bar = {ratio:.4f}")
            WORST["conv_wgrad bf16x3 (class bar)"] = max(WORST.get("conv_wgrad bf16x3 (class bar)", 0.0), ratio)
            assert ratio <= 1.0, what
            if R.wgrad_split16(shape, prec, mode) and dw0 is None:
                fp32 = ops.conv_wgrad(d["x"], d["styles"], g, d["weight"], op_mode, dd=dd, dcoef=d["dcoef"], ksplit=1)
                assert not torch.equal(got, fp32), "the split kernel did not run"


# ----------------------------------------------------------------------------- documented refusals
def test_documented_refusals_raise_and_launch_nothing(dev):
    """C % 4 != 0, C > 1024, dxs_rgb together with g_rgb_small, five small-toRGB channels, dd without dcoef or wsq, a misaligned
    `out`: a Python exception each, the targets untouched, the device still healthy."""
    from hfa_gp_amd import ops
    z = lambda *s: torch.ones(*s, device=dev)        # noqa: E731
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.pointwise_bwd(z(1, 2, 2, 6), dxs_conv=z(1, 2, 2, 6), s_conv=z(1, 6))
    with pytest.raises(RuntimeError, match="1024"):
        ops.pointwise_bwd(z(1, 1, 1, 1028), dxs_conv=z(1, 1, 1, 1028), s_conv=z(1, 1028))
    small = dict(g_rgb_small=z(1, 3, 2, 2), w_rgb_small=z(3, 8), s_small=z(1, 8))
    with pytest.raises(RuntimeError, match="exclusive"):
        ops.pointwise_bwd(z(1, 2, 2, 8), dxs_rgb=z(1, 2, 2, 8), s_rgb=z(1, 8), **small)
    with pytest.raises(RuntimeError, match="1..4 channels"):
        ops.pointwise_bwd(z(1, 2, 2, 8), g_rgb_small=z(1, 5, 2, 2), w_rgb_small=z(5, 8), s_small=z(1, 8))
    d_ws = z(2, 2, 16)
    for dcoef, wsq in ((None, z(5, 4)), (z(2, 5), None)):
        with pytest.raises(RuntimeError, match="dd needs dcoef and wsq"):
            ops.style_bwd(z(2, 4), z(2, 5), z(2, 4), dcoef, wsq, z(4, 16), d_ws[:, 1])
        with pytest.raises(RuntimeError, match="dd needs dcoef and wsq"):
            ops.style_bwd_batch([(z(2, 4), z(2, 5), z(2, 4), dcoef, wsq, z(4, 16), 1, 1.0)], d_ws)
    x, g, wgt = z(1, 2, 2, 8), z(1, 2, 2, 32), z(32, 8, 3, 3)
    out = z(32, 8, 3, 3)
    with pytest.raises(RuntimeError, match="dd needs dcoef"):
        ops.conv_wgrad(x, z(1, 8), g, wgt, ops.CONV3X3, dd=z(1, 32), out=out)
    flat = z(32 * 8 * 9 + 4)
    odd = flat[1:1 + 32 * 8 * 9].view(32, 8, 3, 3)
    assert odd.data_ptr() % 16 != 0
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        ops.conv_wgrad(x, z(1, 8), g, wgt, ops.CONV3X3, out=odd)
    torch.cuda.synchronize()
    assert (d_ws == 1).all() and (out == 1).all() and (flat == 1).all()
