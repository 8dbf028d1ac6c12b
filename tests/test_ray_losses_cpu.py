"""hfa_gp_amd.ray_losses (plain torch) against brute force in float64, and the CPU self-check of the references the GPU tests of
the per-sample outputs rest on (tests/ray_samples_ref.py).  No GPU."""
import pytest
import torch

from hfa_gp_amd import ray_losses as RLS

S = 24


def _rays(seed=0, n=37):
    """n rays of S sorted depths and S-1 weights in float64: random ones, two zero-opacity rays, two all-zero (empty) rows, one ray
    with all its weight in one interval and one with zero-width intervals."""
    g = torch.Generator().manual_seed(seed)
    t = torch.sort(2.25 + 1.05 * torch.rand(n, S, generator=g, dtype=torch.float64), -1).values
    alpha = torch.rand(n, S - 1, generator=g, dtype=torch.float64) ** 3
    w = alpha * torch.cumprod(torch.cat((torch.ones(n, 1, dtype=torch.float64), 1 - alpha[:, :-1]), -1), -1)
    w[3] = 0
    w[4] = 0
    t[5] = 0
    w[5] = 0
    t[6] = 0
    w[6] = 0
    w[7] = 0
    w[7, 11] = 0.8
    t[8, 5:9] = t[8, 5]
    return t, w


def _distortion_brute(t, w):
    mid, delta = 0.5 * (t[:, 1:] + t[:, :-1]), t[:, 1:] - t[:, :-1]
    pair = (w[:, :, None] * w[:, None, :] * (mid[:, :, None] - mid[:, None, :]).abs()).sum((1, 2))
    return pair + (w * w * delta).sum(-1) / 3


def test_distortion_loss_vs_pairwise_sum():
    t, w = _rays()
    got = RLS.distortion_loss(t, w)
    want = _distortion_brute(t, w)
    assert got.shape == (t.shape[0],)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-14)
    assert float(got[3]) == 0.0 and float(got[5]) == 0.0
    assert float(got.min()) >= -1e-15
    # batch dimensions pass through
    torch.testing.assert_close(RLS.distortion_loss(t[:36].reshape(4, 9, S), w[:36].reshape(4, 9, S - 1)).reshape(-1), want[:36],
                               rtol=1e-12, atol=1e-14)


def test_distortion_loss_t_range():
    t, w = _rays(1)
    near, far = 2.25, 3.3
    want = _distortion_brute((t - near) / (far - near), w)
    torch.testing.assert_close(RLS.distortion_loss(t, w, t_range=(near, far)), want, rtol=1e-12, atol=1e-14)
    # per-ray limits, an empty ray's limits not finite: mapped to 0, no NaN
    tn, tf = torch.full((t.shape[0],), near, dtype=torch.float64), torch.full((t.shape[0],), far, dtype=torch.float64)
    tn[5], tf[5] = float("inf"), float("-inf")
    tn[6], tf[6] = float("nan"), float("nan")
    got = RLS.distortion_loss(t, w, t_range=(tn, tf))
    assert torch.isfinite(got).all() and float(got[5]) == 0.0 and float(got[6]) == 0.0
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[5:7] = False
    torch.testing.assert_close(got[keep], want[keep], rtol=1e-12, atol=1e-14)


def test_distortion_loss_gradcheck():
    t, w = _rays(2, n=9)
    w = w.clone().requires_grad_(True)
    assert torch.autograd.gradcheck(lambda x: RLS.distortion_loss(t, x), (w,))
    assert torch.autograd.gradcheck(lambda x: RLS.distortion_loss(t, x, t_range=(2.0, 3.5)), (w,))
    RLS.distortion_loss(t, w).sum().backward()
    assert torch.isfinite(w.grad).all()


def _quantile_brute(t, w, q):
    out = []
    for ti, wi in zip(t.tolist(), w.tolist()):
        total = sum(wi)
        if total == 0:
            out.append(ti[-1])
            continue
        target, acc = q * total, 0.0
        for e, we in enumerate(wi):
            if acc + we >= target and (we > 0 or target == 0):
                frac = (target - acc) / we if we > 0 else 0.0
                out.append(ti[e] + min(max(frac, 0.0), 1.0) * (ti[e + 1] - ti[e]))
                break
            acc += we
        else:
            out.append(ti[-1])
    return torch.tensor(out, dtype=torch.float64)


@pytest.mark.parametrize("q", [0.5, 0.1, 0.9, 1.0])
def test_quantile_depth_vs_scan(q):
    t, w = _rays(3)
    got = RLS.quantile_depth(t, w, q)
    torch.testing.assert_close(got, _quantile_brute(t, w, q), rtol=1e-9, atol=1e-9)
    assert float(got[3]) == float(t[3, -1]) and float(got[5]) == 0.0          # zero opacity: the upper end; empty: its zeros
    if q == 0.5:                                                              # all weight in interval 11: its midpoint
        assert abs(float(got[7]) - 0.5 * float(t[7, 11] + t[7, 12])) <= 1e-12
    # the cumulative weight up to the returned depth is q * total (piecewise-linear CDF), checked by a second route
    cum = torch.cat((torch.zeros(t.shape[0], 1, dtype=torch.float64), torch.cumsum(w, -1)), -1)
    for i in range(t.shape[0]):
        if float(cum[i, -1]) > 0 and i != 8:
            cdf_at = torch.from_numpy(__import__("numpy").interp(got[i:i + 1].numpy(), t[i].numpy(), cum[i].numpy()))
            assert abs(float(cdf_at) - q * float(cum[i, -1])) <= 1e-9


def test_depth_variance_vs_definition():
    t, w = _rays(4)
    got = RLS.depth_variance(t, w)
    mid = 0.5 * (t[:, 1:] + t[:, :-1])
    for i in range(t.shape[0]):
        tot = float(w[i].sum())
        if tot == 0:
            assert float(got[i]) == 0.0
            continue
        d = float((w[i] * mid[i]).sum()) / tot
        assert abs(float(got[i]) - float((w[i] * (mid[i] - d) ** 2).sum()) / tot) <= 1e-14
    assert abs(float(got[7])) <= 1e-15
    w2 = w.clone().requires_grad_(True)
    RLS.depth_variance(t, w2).sum().backward()
    assert torch.isfinite(w2.grad).all()


def test_helpers_refuse_mismatched_shapes():
    t, w = _rays()
    for fn in (RLS.distortion_loss, RLS.quantile_depth, RLS.depth_variance):
        with pytest.raises(ValueError, match="sample_weights"):
            fn(t, w[:, :-1])
    with pytest.raises(ValueError, match="q must lie"):
        RLS.quantile_depth(t, w, 1.5)


@pytest.mark.parametrize("preset,limits", [("tiny64", None), ("small128", None), ("ffhq512_128", None), ("small128", "box")])
def test_reference_depths_self_check(preset, limits):
    """The condition the GPU depth test rests on, checked before anything runs on a GPU: the fp32 reference leaves at most 1 % of
    the valid rays unmatched against the float64 reference (else: other seeds), and TOL_T is 4 x their largest deviation over the
    matched rays."""
    from tests import ray_samples_ref as SR
    assert (preset, limits) in SR.CONFIGS
    valid, unmatched, dev_t, dev_w = SR.self_check(preset, limits)
    print(f"{preset}/{limits}: {valid} valid rays, {unmatched} unmatched fp32 vs float64, depth deviation {dev_t:.3e} over the matched "
          f"rays (TOL_T = {SR.tol_t(preset, limits):.3e}), weights_at fp32 vs float64 {dev_w:.3e}")
    assert unmatched <= SR.MAX_UNMATCHED_REF * valid
    assert 0 < dev_t <= SR.MAX_DEV_T and SR.tol_t(preset, limits) == 4 * dev_t
    assert SR.tol_w(preset, limits) == 2e-5            # fp32 against float64 weights are ~1e-7 apart: the forward bar governs
    ref = SR.reference(preset, limits)
    assert bool((ref["t"][..., 1:] >= ref["t"][..., :-1]).all())
    if limits is not None:
        empty = ~ref["valid"]
        assert int(empty.sum()) == 40 and not bool(ref["t"][empty].any()) and not bool(ref["w"][empty].any())
