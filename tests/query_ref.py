"""Reference for the backward of the tri-plane point query: float64 autograd through the CPU oracle's
``osg_decoder(P, sample_from_planes(...))`` with respect to the planes, the points and the four decoder tensors, and the test
points (built on the CPU, away from the texel edges where the bilinear gather has no derivative).  Shared by
tests/test_query_grad_cpu.py (which checks this reference against central differences) and tests/test_gpu_query_grad.py."""
import functools

import torch

DEC_KEYS = ("decoder.net.0.weight", "decoder.net.0.bias", "decoder.net.2.weight", "decoder.net.2.bias")
AXES = ("eg3d_original", "eg3d_fixed")
# the base set-up of tests/test_gpu_shape.py::test_planes_query_vs_oracle
B, H, W, BOX_WARP, LR_MUL = 2, 20, 28, 0.8, 0.5
M = 16 * 9 + 5                   # 10 tiles per identity, the last one ragged: 20 tiles = 5 workgroups of 4 waves
SPECIAL = ((3.0, -3.0, 2.0), (-9.0, 9.0, 9.0), (0.6, 0.0, 0.0), (0.0, -0.41, 0.0), (0.4, 0.4, 0.4), (-0.4, -0.4, -0.4),
           (0.0, 0.0, 0.0))      # x box_warp; the first two lie outside every plane
EDGE = 1e-3                      # no pixel coordinate of a test point has a fractional part closer than this to 0 or 1


def decoder(g: torch.Generator, lr_mul: float):
    """Decoder parameters as tests/test_gpu_shape.py draws them."""
    return {"decoder.net.0.weight": torch.randn(64, 32, generator=g) / lr_mul,
            "decoder.net.0.bias": 0.3 * torch.randn(64, generator=g) / lr_mul,
            "decoder.net.2.weight": torch.randn(33, 64, generator=g) / lr_mul,
            "decoder.net.2.bias": 0.3 * torch.randn(33, generator=g) / lr_mul}


def pixel_coords(coords: torch.Tensor, box_warp: float, axes: str, h: int, w: int) -> torch.Tensor:
    """float64 pixel coordinates [..., 3 planes, 2 (ix, iy)] of the points in every plane (grid_sample, align_corners=False)."""
    from oracle import eg3d_oracle as O
    q = (2.0 / box_warp) * coords.double()
    inv = torch.linalg.inv(O.plane_axes(axes)).double()                  # [3, 3, 3]
    proj = torch.einsum("...k,pkc->...pc", q, inv)[..., :2]              # [..., 3, 2] = (gx, gy)
    size = torch.tensor([w, h], dtype=torch.float64)
    return (proj + 1.0) * (size / 2.0) - 0.5


def near_edge(coords: torch.Tensor, box_warp: float, h: int, w: int) -> torch.Tensor:
    """[...] bool: a pixel coordinate of the point, in any plane under either axes convention, lies within EDGE of an integer."""
    bad = torch.zeros(coords.shape[:-1], dtype=torch.bool)
    for axes in AXES:
        px = pixel_coords(coords, box_warp, axes, h, w)
        fr = px - px.floor()
        bad |= ((fr < EDGE) | (fr > 1.0 - EDGE)).flatten(-2).any(-1)
    return bad


def make_points(g: torch.Generator, b: int, m: int, box_warp: float = BOX_WARP, h: int = H, w: int = W, special: bool = True,
                spread: float = 1.3) -> torch.Tensor:
    """[b, m, 3] fp32 points, about a third of them outside the box, the SPECIAL ones first; a point near a texel edge is
    drawn again until none is left, so that every point can be compared."""
    coords = (torch.rand(b, m, 3, generator=g) - 0.5) * (spread * box_warp)
    if special:
        n = min(m, len(SPECIAL))
        coords[:, :n] = torch.tensor(SPECIAL[:n]) * box_warp
    for _ in range(100):
        bad = near_edge(coords, box_warp, h, w)
        if special:
            assert not bad[:, :min(m, len(SPECIAL))].any(), "a special point sits on a texel edge"
        if not bad.any():
            return coords
        coords[bad] = (torch.rand(int(bad.sum()), 3, generator=g) - 0.5) * (spread * box_warp)
    raise AssertionError("could not move the points off the texel edges")


def query_fp64(P, planes, coords, box_warp, axes, lr_mul):
    """(rgb [B,M,32], sigma [B,M,1]) in float64 of whatever (possibly grad-requiring) float64 inputs are given."""
    from oracle import eg3d_oracle as O
    b = planes.shape[0]
    return O.osg_decoder(P, O.sample_from_planes(O.plane_axes(axes), planes, coords.expand(b, -1, -1), box_warp), lr_mul)


def reference(P, planes_nchw, coords, g_sigma, g_rgb, box_warp, axes, lr_mul):
    """float64 autograd of  <sigma, g_sigma> + <rgb, g_rgb>  (either upstream may be None) →
    dict(planes [B,3,32,H,W], coords [Bc,M,3] (summed over B when Bc = 1), dec (four tensors))."""
    P64 = {k: P[k].detach().double().requires_grad_(True) for k in DEC_KEYS}
    pl = planes_nchw.detach().double().requires_grad_(True)
    co = coords.detach().double().requires_grad_(True)
    rgb, sigma = query_fp64(P64, pl, co, box_warp, axes, lr_mul)
    loss = 0.0
    if g_sigma is not None:
        loss = loss + (sigma * g_sigma.double().reshape(sigma.shape)).sum()
    if g_rgb is not None:
        loss = loss + (rgb * g_rgb.double()).sum()
    grads = torch.autograd.grad(loss, [pl, co] + [P64[k] for k in DEC_KEYS])
    return dict(planes=grads[0], coords=grads[1], dec=tuple(grads[2:]))


@functools.lru_cache(maxsize=None)
def base_case(seed: int = 5):
    """The shared inputs: decoder, planes in the oracle's layout [B,3,32,H,W], points and upstream gradients."""
    g = torch.Generator().manual_seed(seed)
    P = decoder(g, LR_MUL)
    pn = torch.randn(B, 3, 32, H, W, generator=g)
    coords = make_points(g, B, M)
    ups = dict(g_sigma=torch.randn(B, M, 1, generator=g), g_rgb=torch.randn(B, M, 32, generator=g))
    return dict(P=P, pn=pn, coords=coords, ups=ups)


UPSTREAM = {"sigma": (True, False), "rgb": (False, True), "both": (True, True)}


@functools.lru_cache(maxsize=None)
def base_reference(axes: str, which: str, broadcast: bool = False):
    """`reference` on `base_case` (computed once per configuration and left unchanged)."""
    cs = base_case()
    use_s, use_r = UPSTREAM[which]
    coords = cs["coords"][:1] if broadcast else cs["coords"]
    return reference(cs["P"], cs["pn"], coords, cs["ups"]["g_sigma"] if use_s else None, cs["ups"]["g_rgb"] if use_r else None,
                     BOX_WARP, axes, LR_MUL)
