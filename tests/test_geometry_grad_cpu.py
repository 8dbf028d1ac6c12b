"""Depth / opacity gradients of the ray marcher without a GPU: the C ABI of hfagp_raymarch_bwd_geom (binding, argument
validation) and the closed-form compositing adjoint G_e the kernel implements (include/hfagp.h) against autograd through the
oracle's MipRayMarcher2 in fp64."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.util import ROOT


@pytest.fixture(scope="module")
def lib():
    from hfa_gp_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib


def test_geom_grads_binding_matches_header(lib):
    text = open(os.path.join(ROOT, "include", "hfagp.h")).read()
    body = re.search(r"typedef struct \{([^{}]*)\} HfagpRaymarchGeomGrads;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"\w+", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in lib.RaymarchGeomGrads._fields_] == ["g_depth", "g_wsum", "depth_range"]
    assert "hfagp_raymarch_bwd_geom" in lib.SYMBOLS
    assert lib.ABI_VERSION == 15, "the export is additive: HfagpRaymarchBwdArgs keeps its layout"


def test_geom_entry_argument_validation(lib):
    h = lib.lib()
    assert h.hfagp_raymarch_bwd_geom(None, None, None) == -1
    assert b"null pointer" in h.hfagp_last_error()
    a = lib.RaymarchBwdArgs()
    a.d_planes, a.rec = 8, 8                # non-null, never dereferenced: the gradients are checked first
    assert h.hfagp_raymarch_bwd(C.byref(a), None) == -1
    assert b"no upstream gradient" in h.hfagp_last_error()
    g = lib.RaymarchGeomGrads()
    assert h.hfagp_raymarch_bwd_geom(C.byref(a), C.byref(g), None) == -1
    assert b"no upstream gradient" in h.hfagp_last_error()
    g.g_depth = 8
    assert h.hfagp_raymarch_bwd_geom(C.byref(a), C.byref(g), None) == -1
    assert b"g_depth needs depth_range" in h.hfagp_last_error()


def closed_form_G(colors, dens, depths, g, gW, gd, lo, hi, white_back):
    """dL/dw_e of L = <rgb, g> + <W, gW> + <clamp(nan_to_num(D / W)), gd> as the kernel forms it (hfagp.h): the forward's
    weights, then  G_e = 2 g . cbar_e - wb * 2 sum(g) + gamma_W + gamma_d (tbar_e - d) / W."""
    delta = depths[:, :, 1:] - depths[:, :, :-1]
    tbar = 0.5 * (depths[:, :, 1:] + depths[:, :, :-1])
    cbar = 0.5 * (colors[:, :, 1:] + colors[:, :, :-1])
    alpha = 1 - torch.exp(-torch.nn.functional.softplus(0.5 * (dens[:, :, 1:] + dens[:, :, :-1]) - 1) * delta)
    T = torch.cumprod(torch.cat([torch.ones_like(alpha[:, :, :1]), 1 - alpha + 1e-10], 2), 2)[:, :, :-1]
    w = alpha * T
    W = w.sum(2, keepdim=True)
    d = (w * tbar).sum(2, keepdim=True) / W
    live = (W > 0) & torch.isfinite(d) & (d >= lo) & (d <= hi)
    gamma_d = torch.where(live, gd[:, :, None], torch.zeros_like(d))
    G = 2 * (cbar * g[:, :, None]).sum(-1, keepdim=True) - (2 * g.sum(-1)[:, :, None, None] if white_back else 0) + gW[:, :, None]
    return G + torch.where(live, gamma_d * (tbar - d) / W, torch.zeros_like(d)), w


@pytest.mark.parametrize("white_back", [False, True])
def test_closed_form_adjoint_matches_oracle_autograd(white_back):
    """G_e is dL/dw_e: carried on through autograd of the weights alone, it must give the density gradients that autograd
    through the whole of O.ray_march gives (fp64, 1e-10).  Rays [0, :3] are transparent (W == 0): there the oracle's own
    autograd is NaN (0 * inf in the backward of D / W under nan_to_num), and the rule of hfagp.h — no depth gradient, nothing
    non-finite — is checked against the oracle WITHOUT the depth term.  A second pass narrows the clamp range (hi = a median
    depth) and checks the pass-through rule on `torch.clamp` itself."""
    from oracle import eg3d_oracle as O
    gen = torch.Generator().manual_seed(11)
    b, r, s = 2, 7, 12
    colors = torch.rand(b, r, s, 5, generator=gen, dtype=torch.float64)
    dens = (3 * torch.randn(b, r, s, 1, generator=gen, dtype=torch.float64)).requires_grad_(True)
    depths = torch.sort(2.25 + 1.05 * torch.rand(b, r, s, 1, generator=gen, dtype=torch.float64), dim=2).values
    with torch.no_grad():
        dens[0, :3] = -800.0            # softplus underflows to 0: alpha = 0 exactly, W = 0
    g = torch.randn(b, r, 5, generator=gen, dtype=torch.float64)
    gW = torch.randn(b, r, 1, generator=gen, dtype=torch.float64)
    gd = torch.randn(b, r, 1, generator=gen, dtype=torch.float64)

    def unclamped(w):
        tbar = 0.5 * (depths[:, :, 1:] + depths[:, :, :-1])
        return torch.nan_to_num((w * tbar).sum(2) / w.sum(2), float("inf"))

    for narrowed in (False, True):
        rgb, depth, w = O.ray_march(colors, dens, depths, white_back)
        assert bool((w.sum(2)[0, :3] == 0).all())
        lo, hi = depths.min(), depths.max()
        if narrowed:                    # the oracle's formula with another range, as `torch.clamp` differentiates it
            hi = unclamped(w.detach())[1].median()
            depth = torch.clamp(unclamped(w), lo, hi)
        image = (rgb * g).sum() + (w.sum(2) * gW).sum()
        ref, = torch.autograd.grad(image + (depth * gd).sum(), dens, retain_graph=True)
        ref0, = torch.autograd.grad(image, dens)
        assert not torch.isfinite(ref[0, :3]).any() and torch.isfinite(ref[0, 3:]).all() and torch.isfinite(ref[1]).all()
        ref[0, :3] = ref0[0, :3]
        G, w2 = closed_form_G(colors, dens, depths, g, gW, gd, lo, hi, white_back)
        assert torch.isfinite(G).all()
        got, = torch.autograd.grad(w2, dens, G.detach())
        assert float((got - ref).abs().max()) <= 1e-10, float((got - ref).abs().max())
        if narrowed:
            out = (unclamped(w.detach()) > hi)
            assert 0 < int(out.sum()) < out.numel()
