"""tests/conv_ref.py without a GPU: the float64 reference against torch.nn.functional (an independent formulation) and the adjoint
identities, the operand split against the weight-image rebuild of tests/test_gpu_weight_image.py, the route predictor against
what the library answers without a device, the preconditions of every exact and multipart case, and the coverage table:
every kernel instantiation the conv launchers can reach has a case in every tier and sub-tier that applies to its kind."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref as R

F64 = torch.float64


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    _lib.lib()
    return _lib


# ----------------------------------------------------------------------------- the reference
def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 5, 7, 3, 4), (1, 1, 1, 2, 3), (3, 2, 9, 5, 2)])
def test_reference_is_conv2d_and_conv_transpose2d(b, h, w, cin, cout):
    x, s = _rand(b, h, w, cin, seed=1), _rand(b, cin, seed=2)
    xs = nchw(x * s[:, None, None, :])
    w3, w1 = _rand(cout, cin, 3, 3, seed=3), _rand(cout, cin, 1, 1, seed=4)
    for got, want in ((R.modconv(x, w3, "3x3", s), F.conv2d(xs, w3, padding=1)),
                      (R.modconv(x, w1, "1x1", s), F.conv2d(xs, w1)),
                      (R.modconv(x, w3, "up", s), F.conv_transpose2d(xs, w3.transpose(0, 1), stride=2)),
                      # the data adjoint of a 3x3 conv with weight Wf [cin, cout] is conv_transpose2d; its image is made of Wf^T
                      (R.modconv(x, w3, "3x3_bwd", s), F.conv_transpose2d(xs, w3.transpose(0, 1), padding=1))):
        assert torch.allclose(got[0], nhwc(want), rtol=1e-12, atol=1e-12)
        assert bool((got[0].abs() <= got[1] * (1 + 1e-12)).all())
    # magnitude: the same sum over absolute values
    assert torch.allclose(R.modconv(x, w3, "3x3", s)[1], nhwc(F.conv2d(xs.abs(), w3.abs(), padding=1)), rtol=1e-12)


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 5, 7, 3, 4), (1, 1, 1, 2, 3)])
def test_adjoint_identities(b, h, w, cin, cout):
    """<conv(x), g> = <x, conv_bwd(g)> for both adjoint modes; the adjoint's weight image is that of the Cin / Cout transpose."""
    x, wf = _rand(b, h, w, cin, seed=5), _rand(cout, cin, 3, 3, seed=6)
    g = _rand(b, h, w, cout, seed=7)
    lhs = (R.modconv(x, wf, "3x3")[0] * g).sum()
    rhs = (x * R.modconv(g, wf.transpose(0, 1).contiguous(), "3x3_bwd")[0]).sum()
    assert torch.allclose(lhs, rhs, rtol=1e-12)
    gt = _rand(b, 2 * h + 1, 2 * w + 1, cout, seed=8)
    lhs = (R.modconv(x, wf, "up")[0] * gt).sum()
    rhs = (x * R.modconv(R.parity_images(gt), wf.transpose(0, 1).contiguous(), "s2_bwd")[0]).sum()
    assert torch.allclose(lhs, rhs, rtol=1e-12)
    # ... and against autograd of the independent formulation
    xr = nchw(x).clone().requires_grad_(True)
    (F.conv_transpose2d(xr, wf.transpose(0, 1), stride=2) * nchw(gt)).sum().backward()
    assert torch.allclose(R.modconv(R.parity_images(gt), wf.transpose(0, 1).contiguous(), "s2_bwd")[0], nhwc(xr.grad), rtol=1e-12, atol=1e-12)


def test_epilogue_composites():
    """The epilogue, the fused toRGB sums, and the two composed entry points against their parts."""
    x, wt, s = _rand(2, 3, 4, 4, seed=9), _rand(6, 4, 3, 3, seed=10), _rand(2, 4, seed=11)
    d, nz, bs = _rand(2, 6, seed=12).abs(), _rand(3, 4, seed=13), _rand(6, seed=14)
    y, m = R.modconv(x, wt, "3x3", s, d, nz, 0.5, bs, "lrelu", 0.2, 2.0, 1.0)
    pre = nhwc(F.conv2d(nchw(x * s[:, None, None, :]), wt, padding=1)) * d[:, None, None, :] + bs + nz[None, :, :, None] * 0.5
    assert torch.allclose(y, (F.leaky_relu(pre, 0.2) * 2.0).clamp(-1.0, 1.0), rtol=1e-12, atol=1e-12)
    rw = _rand(2, 3, 6, seed=15)
    assert torch.allclose(R.fused_torgb(y, m, rw)[0], torch.einsum("bhwo,bro->bhwr", y, rw))
    yt = R.modconv(x, wt, "up", s)[0]
    up = R.upconv_fir(x, wt, s, d, None, 0.0, bs, "lrelu", 0.2, 2.0, None)
    assert torch.equal(up[0], R.upfir_epilogue(yt, d, None, 0.0, bs, "lrelu", 0.2, 2.0, None)[0]) and bool((up[0].abs() <= up[1] + 1e-12).all())
    w1, img = _rand(6, 4, 1, 1, seed=16), _rand(2, 3, 4, 6, seed=17)
    x2 = _rand(2, 6, 8, 4, seed=18)
    sk = R.torgb_skip(x2, w1, s, bs, img, plane_major=True)
    assert torch.equal(sk[0], R.skip_upsample_add(img, R.modconv(x2, w1, "1x1", s, bias=bs)[0], True)[0])


# ----------------------------------------------------------------------------- the split
@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6", "f16", "f16x3"])
@pytest.mark.parametrize("cout,cin,k", [(128, 16, 3), (96, 32, 1), (40, 24, 3)])
def test_parts_are_the_weight_image(cout, cin, k, prec):
    """`parts` after `image_exponent` == `_rebuild` of tests/test_gpu_weight_image.py (which the device images equal bit for bit)
    on that file's edge weights: ties of both parities, subnormal residuals, +-0, planes at 2^-20 and 2^12."""
    from tests.test_gpu_weight_image import _edge_weight, _image_exponent, _rebuild
    w = _edge_weight(cout, cin, k, seed=cout + cin)
    img, _ = _rebuild(w, prec)
    assert R.image_exponent(w, prec) == (_image_exponent(w) if R.is_f16(prec) else 0)
    mine = R.parts(w * 2.0 ** -R.image_exponent(w, prec), prec, R.NPARTS_B[prec])
    assert len(mine) == img.shape[0]
    for p, part in enumerate(mine):
        want = img[p].float().permute(2, 1, 3, 0).reshape(cout, cin, k, k)            # [taps, Cin/8, Cout, 8] -> [Cout, Cin, k, k]
        assert torch.equal(part, want), (prec, p)


def test_guard_exponents():
    s = torch.tensor([0.3, -3.0, 1.0])
    assert R.guard(s, "f16x3") == 2 and R.guard(s, "bf16x3") == 0          # 3 = 0.75 * 2^2
    assert R.guard(torch.tensor([1.0, -0.5]), "f16") == 1 and R.guard(None, "f16") == 1
    assert R.guard(s, "f16x2", x_absmax=2.0) == 2 + 2 - 15
    ps = R.parts(torch.tensor([1.0 + 2.0 ** -11, 1.0 - 2.0 ** -11, 70000.0]), "f16x3", 2)
    assert ps[0].tolist() == [1.0, 1.0 - 2.0 ** -11, 65504.0] and ps[1].tolist() == [2.0 ** -11, 0.0, 70000.0 - 65504.0]
    ps = R.parts(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -16]), "bf16x6", 3)               # the first part rounds UP: two parts hold it
    assert ps[2].item() == 0.0


# ----------------------------------------------------------------------------- the route predictor
def _args(lib, c, ops):
    a = lib.ModconvArgs()
    a.x = a.wt = a.y = 1                        # non-null, never dereferenced by planning
    a.rgb_w = 1 if c["rgb"] else None
    a.B, a.H, a.W, a.Cin, a.Cout = (c[k] for k in ("B", "H", "W", "Cin", "Cout"))
    a.mode, a.precision = R.MODE_ID[c["mode"]], ops.PRECISIONS[c["kind"]]
    a.x_f16, a.y_f16, a.ksplit = int(c["x_f16"]), int(c["y_f16"]), c["ksplit"]
    a.x_batch_stride = 0 if c["bcast"] else c["H"] * c["W"] * c["Cin"]
    a.alpha, a.gain, a.clamp = 0.2, 1.0, 256.0
    return a


ALL_CASES = R.cases()


def test_modconv_enum_is_the_modes(lib):
    from hfa_gp_amd import ops
    assert [ops.CONV3X3, ops.CONVT3X3_UP2, ops.CONV1X1, ops.CONV3X3_BWD, ops.CONVS2_BWD] == [R.MODE_ID[m] for m in R.MODES]
    assert all(ops.NPARTS[k] == R.NPARTS_B[k] for k in R.KINDS) and lib.ABSMAX_FLOATS == R.ABSMAX_SLOTS * R.ABSMAX_STRIDE


def test_plan_is_the_librarys_workspace(lib):
    """hfagp_modconv_workspace_bytes of every case == the predictor's K slices x slabs (the small-image kernel's own slices
    included); several K slices of the small-image kernel do occur."""
    from hfa_gp_amd import ops
    for c in ALL_CASES:
        got = lib.lib().hfagp_modconv_workspace_bytes(C.byref(_args(lib, c, ops)))
        assert got == R.plan(c, c["env"])["ws_bytes"], c["id"]
    small = [R.plan(c)["ksplit"] for c in ALL_CASES if c["group"] == "small"]
    assert 1 in small and max(small) > 1
    # more slices asked for than there are chunks: clipped
    assert all(R.plan(c)["ksplit"] == c["Cin"] // 16 for c in ALL_CASES if c["group"] == "staged16" and c["ksplit"] == 7)


def test_plan_is_the_support_predicates(lib):
    from hfa_gp_amd import ops
    for b, side, cin, cout in ((1, 8, 32, 128), (32, 8, 64, 128), (2, 64, 128, 128), (8, 32, 256, 256), (1, 128, 64, 128), (5, 24, 32, 128)):
        c3 = R.case("q", "3x3", "f16", b, side, side, cin, cout, x_f16=True, y_f16=True)
        cu = R.case("q", "up", "f16", b, side, side, cin, cout, x_f16=True, y_f16=True)
        assert ops.f16_storage_supported(side, side, cin, cout, b) == (R.plan(c3)["ws_bytes"] == 0 and R.plan(cu)["ws_bytes"] == 0)
        for kind in ("f16x3", "bf16x6"):
            wt = torch.empty(ops.NPARTS[kind], 9, cin // 8, cout, 8, dtype=ops._IMAGE_DTYPE[kind])
            cr = R.case("q", "3x3", kind, b, side, side, cin, cout, rgb=True)
            assert ops.fused_torgb_supported(torch.empty(b, side, side, cin), wt, cout, b) == (R.plan(cr)["ws_bytes"] == 0)


def test_fir_cases_are_supported(lib, monkeypatch):
    """hfagp_upconv_fir_scratch_bytes: the streaming kernel answers with its token 256, the strip kernel with its scratch."""
    from hfa_gp_amd import ops
    for kernel in R.FIR_SHAPES:
        for k, v in R.FIR_ENV[kernel].items():
            monkeypatch.setenv(k, v)
        for c in R.fir_cases(kernel):
            n = lib.lib().hfagp_upconv_fir_scratch_bytes(C.byref(_args(lib, c, ops)))
            assert (n == 256) if kernel == "lean" else (n > 256), c["id"]
    b, h, w, cin = R.SKIP_SHAPE
    assert ops.torgb_skip_supported(torch.empty(b, h, w, cin), torch.empty(2, 1, 2, 32, 8, dtype=torch.float16), 32)
    assert not ops.torgb_skip_supported(torch.empty(b, h, w // 2, cin), torch.empty(2, 1, 2, 32, 8, dtype=torch.float16), 32)


def test_up_conv_cases_reach_their_branches():
    by = {c["id"]: R.plan(c) for c in ALL_CASES if c["group"] == "up"}
    assert {p["fringe"] for p in by.values()} == {False, True}
    assert any(p["up_ns"] >= 3 for p in by.values())                                    # a tile over three samples
    assert any(p["up_ns"] < c["B"] for c in ALL_CASES if c["group"] == "up" for p in [R.plan(c)])
    b9 = [R.plan(c) for c in ALL_CASES if c["group"] == "up" and c["B"] == 9]
    assert b9 and all(not p["fringe"] for p in b9)                                      # W % 16 == 0, but 9 samples > 8 staged
    assert R.plan(ALL_CASES[0], {"HFAGP_DEV_UP_WAVES": "8"})["up_waves"] == 0


# ----------------------------------------------------------------------------- coverage
def test_every_route_has_a_case_in_every_tier():
    seen = {}
    for c in ALL_CASES:
        seen.setdefault(R.route(c, c["env"]), []).append(c)
    assert set(seen) | set(R.CHILD_ONLY) == set(R.ROUTES), (sorted(set(R.ROUTES) - set(seen) - set(R.CHILD_ONLY)), sorted(set(seen) - set(R.ROUTES)))
    assert not set(seen) & set(R.CHILD_ONLY)
    for rt, cs in seen.items():
        kind = cs[0]["kind"]
        assert all(c["kind"] == kind for c in cs), rt
        for sub in R.SUBTIERS.get(kind, {}):
            assert any(R.multipart_fits(c, sub) for c in cs), (rt, sub)
    # the 8-wave block: the exact tier in a child process (tests/conv_child.py), every kind but bf16x6
    from tests import conv_child
    w8 = {R.route(c, conv_child.VARIANTS["waves8"]) for c in conv_child.variant_cases("waves8")}
    assert set(R.CHILD_ONLY) == w8
    # each read-once switch changes the plan of some case it runs (the XCD remap renumbers blocks only: nothing to predict)
    for variant in ("legacy_tiles", "no_fringe", "waves8"):
        env = conv_child.VARIANTS[variant]
        assert any(R.plan(dict(c, ksplit=0), env) != R.plan(dict(c, ksplit=0)) for c in conv_child.variant_cases(variant)), variant


# ----------------------------------------------------------------------------- preconditions
@pytest.mark.parametrize("group", sorted({c["group"] for c in ALL_CASES}))
def test_exact_preconditions(group):
    for c in (c for c in ALL_CASES if c["group"] == group):
        t, q = R.inputs(c, "exact")
        ref, mag = R.modconv(batch=c["B"], **R.ref_kwargs(t), mode=c["mode"])
        R.exact_precondition(ref, mag, q, c["id"])
        R.planted(c, ref)
        if c["mode"] in R.FUSED:                    # an output ON the clamp checks nothing of the sum: few are, and the planted one is
            share = R.saturated_share(ref, t["clamp"])
            assert share <= R.MAX_SATURATED and (share > 0) == (c["clamp"] and not c["bcast"]), (c["id"], share)
        if c["kind"] != "fp32":
            (_, ap), (_, bp) = R.operand_parts(t, c["kind"], c["mode"], x_absmax=float(t["x"].abs().max()) if c.get("x_absmax") else None)
            R.normal_parts(ap + bp, c["kind"], c["id"])
            assert not any(p.any() for p in ap[1:] + bp[1:]), c["id"]              # one part holds every exact-tier operand
        if c["y_f16"]:
            assert torch.equal(ref.half().double(), ref), c["id"]                     # the stored half is the reference itself
        if c["rgb"]:
            R.exact_precondition(*R.fused_torgb(ref, mag, t["rgb_w"]), q, c["id"])


@pytest.mark.parametrize("kind", [k for k in R.KINDS if R.SUBTIERS[k]])
def test_multipart_preconditions(kind):
    n = 0
    for c in (c for c in ALL_CASES if c["kind"] == kind):
        for sub in R.SUBTIERS[kind]:
            if not R.multipart_fits(c, sub):
                continue
            t, q = R.multipart_inputs(c, sub)
            ref, mag = R.modconv(t["x"], t["weight"], c["mode"], t["styles"])
            R.exact_precondition(ref, mag, q, f"{c['id']} {sub}")
            R.multipart_precondition(t, kind, sub, c["mode"], f"{c['id']} {sub}")
            n += 1
    assert n > 0


def test_fir_and_skip_preconditions():
    for kernel in R.FIR_SHAPES:
        for c in R.fir_cases(kernel):
            t, q = R.fir_inputs(c, "exact")
            ref, mag = R.upconv_fir(**t)
            R.exact_precondition(ref, mag, q, c["id"])
            R.fir_planted(c, t, ref)
            assert R.saturated_share(ref, t["clamp"]) <= R.MAX_SATURATED, c["id"]
        n = 0
        for c, sub, t, q in R.fir_multipart(kernel):
            R.exact_precondition(*R.upconv_fir(t["x"], t["weight"], t["styles"], act="linear", gain=1.0), q, f"{c['id']} {sub}")
            R.multipart_precondition(t, c["kind"], sub, "up", f"{c['id']} {sub}")
            n += 1
        assert n == 5                                  # f16x3 and bf16x3: two sub-tiers each, f16x2: one
    for c in R.skip_cases():
        t, q = R.skip_inputs(c, "exact")
        R.exact_precondition(*R.torgb_skip(plane_major=c["plane_major"], **t), q, c["id"])
    subs = set()
    for c, sub, t, q in R.skip_multipart():
        R.exact_precondition(*R.torgb_skip(t["x"], t["weight"], t["styles"], t["bias"]), q, f"{c['id']} {sub}")
        R.multipart_precondition(t, c["kind"], sub, "1x1", f"{c['id']} {sub}")
        subs.add((c["kind"], sub))
    assert subs == {(k, sub) for k in R.SKIP_KINDS for sub in R.SUBTIERS[k]}


def test_realistic_clamps_bite_on_few_outputs():
    bites = 0
    for c in (c for c in ALL_CASES if c["mode"] in R.FUSED and c["clamp"]):
        t, _ = R.inputs(c, "realistic")
        share = R.saturated_share(R.modconv(batch=c["B"], **R.ref_kwargs(t), mode=c["mode"])[0], t["clamp"])
        assert share <= R.MAX_SATURATED, (c["id"], share)
        bites += share > 0
    assert bites >= 10
    for kernel in R.FIR_SHAPES:
        for c in (c for c in R.fir_cases(kernel) if c["clamp"]):
            t, _ = R.fir_inputs(c, "realistic")
            assert R.saturated_share(R.upconv_fir(**t)[0], t["clamp"]) <= R.MAX_SATURATED, c["id"]


def test_the_epilogue_is_dealt_over_the_fused_cases():
    fused = [c for c in ALL_CASES if c["mode"] in R.FUSED]
    assert {c["epi"] for c in fused} == set(range(8)) and {c["act"] for c in fused} == {"lrelu", "linear"}
    on = [c for c in fused if c["clamp"]]
    assert 0 < len(on) <= len(fused) // 4 and {c["act"] for c in on} == {"lrelu", "linear"}
    for group in {c["group"] for c in fused} - {"up"}:          # ("up" holds one fused case, fp16 storage: no clamp, see cases())
        assert any(c["clamp"] for c in fused if c["group"] == group), group


def test_e_kind_is_the_derivation():
    assert R.e_kind("fp32") == 0.0
    k = 1.0 + 2.0 ** -7
    assert R.e_kind("f16") == 2.0 ** -10 * k and R.e_kind("f16x3") == 2.0 ** -21 * k and R.e_kind("bf16x3") == 2.0 ** -15 * k
    assert R.e_kind("f16x2") == (2.0 ** -11 + 2.0 ** -23) * k and R.e_kind("bf16x6") == (3 * 2.0 ** -25 + 2.0 ** -34) * k
    assert R.e_kind("f16", x_f16=True) == (3 * 2.0 ** -11) * k
    # the residual bounds R(n) behind it, on the worst values of each type: just above a tie
    for kind, t_bits in (("f16x3", 11), ("bf16x6", 8)):
        v = torch.tensor([1.0 + 2.0 ** -t_bits + 2.0 ** -23, 1.0 + 2.0 ** -t_bits - 2.0 ** -23, 1.9999999], dtype=torch.float32)
        ps = R.parts(v, kind, 3)
        for n in (1, 2, 3):
            assert bool(((v.double() - sum(p.double() for p in ps[:n])).abs() <= R._res(t_bits, n) * v.double().abs()).all()), (kind, n)
            assert n == 3 or bool((ps[n].double().abs() <= R._res(t_bits, n) * v.double().abs()).all()), (kind, n)
