"""Round-5 parity cases: the GENERATOR-TUNED optimisation step at BASELINE's own size.

The reference trains the generator from iteration `tune_iter` = 50 000 of its default 800 000 on
(/root/reference/code/train_rgb.py:132-134,162,193 -> trainer_rgb.py:69-71 `tune_generator`): 94 % of its iterations
back-propagate into all 30.7 M generator parameters.  `test_full_size_parameter_gradients_three_way` checks `synthesis`'
gradients for a white-noise cotangent; this file checks the TRAINER's composed step in that regime — driver net -> QR basis ->
HIP generator -> fused pool + MSE -> backward with the weight-gradient GEMMs, the decoder-gradient pass and the bucketed
gradient sink of the multi-GPU path active (1-rank RCCL group, small buckets) — against the identical step through the CPU
oracle under autograd.  Needs an MI355X:  python -m pytest tests -m gpu"""
import math
import os

import pytest
import torch

from tests.test_gpu_round4 import OwnSizeArgs, _free_port, _own_size_inputs, rel_l2
from tests.util import perturb_state

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the -m gpu tests need an MI355X")
    from hfa_gp_amd import _lib
    _lib.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("mode", ["3dmm", "rgb"])
def test_tuned_gen_update_at_own_size_matches_oracle_step(dev, mode):
    """`ffhq512_128`, B = 2, K = 50, L2 at 256^2, `tune_generator()` called on both sides.  The HIP side runs with the
    bucketed all-reduce sink ACTIVE (force_collective in a 1-rank "nccl" = RCCL group, 4 MB buckets: the generator's gradients
    are released block by block from inside SynthesisFn.backward into the flat buffer while collectives of finished buckets are
    in flight).  Compared: loss, pooled image, bases / delta / every driver gradient (bar 2e-4 as in the frozen test) and EVERY
    generator parameter's .grad after the step: tensor-valued ones by rel-L2 (bar 2e-3: split-bf16 weight-gradient GEMMs,
    2^-16 per product, K up to 524 288 positions; the three-way fp64 test prices the oracle's own fp32 distance from the truth
    at 1.0-1.2e-3 for a white-noise cotangent, the smooth loss gradient here is better conditioned), scalars (noise strengths:
    one number, near-total cancellation) against the cancellation scale the oracle's own fp32 run reaches."""
    import torch.distributed as dist
    from hfa_gp_amd import headnerf
    from hfa_gp_amd.trainer import FlatGrads, Trainer
    from tests.test_trainer_cpu import OracleGenerator
    cls = headnerf.HeadNeRF_final if mode == "rgb" else headnerf.HeadNeRF_3DMM

    def build(device, oracle):
        torch.manual_seed(0)
        gen = cls(OwnSizeArgs(), OwnSizeArgs.size, device, 512, OwnSizeArgs.latent_dim_shape)
        perturb_state(gen.generator)
        if oracle:
            OracleGenerator.adopt(gen.generator)
        tr = Trainer(OwnSizeArgs(), device, mode=mode, gen=gen, lpips="none")
        tr.optimizer = torch.optim.SGD(tr.gen.parameters(), lr=0.0)        # compare gradients, not Adam's first step
        tr.tune_generator()
        return tr

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(_free_port())
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        gpu = build(dev, False)
        gpu.force_collective = True
        gpu._flat = FlatGrads(gpu.shared_parameters(), bucket_bytes=4 << 20)
        gpu._bucketer = None
        cfg = gpu.gen.generator.cfg
        real, params, label, us, ui = _own_size_inputs(cfg, 2)
        out = gpu.gen_update(real.to(dev), label.clone().to(dev), None if mode == "rgb" else params.to(dev),
                             u_strat=us.to(dev), u_imp=ui.to(dev))
        torch.cuda.synchronize()
        order = gpu._bucketer.last_order
        assert len(order) == len(gpu._flat.buckets) > 8 and order == list(range(len(order))), order
        assert gpu._bucketer.launched_early == len(order), (gpu._bucketer.launched_early, len(order))
        l2_gpu, img_gpu = (out[0], out[2]) if mode == "rgb" else (out[1], out[3])
        got = {n: p.grad.detach().cpu() for n, p in gpu.gen.named_parameters() if p.grad is not None and p.requires_grad}
        l2_gpu, img_gpu = float(l2_gpu), img_gpu.cpu()
        del gpu
        torch.cuda.empty_cache()
    finally:
        dist.destroy_process_group()

    cpu = build("cpu", True)
    out = cpu.gen_update(real, label.clone(), None if mode == "rgb" else params, u_strat=us, u_imp=ui)
    l2_cpu, img_cpu = (out[0], out[2]) if mode == "rgb" else (out[1], out[3])
    want = {n: p.grad.detach() for n, p in cpu.gen.named_parameters() if p.grad is not None and p.requires_grad}
    l2_cpu = float(l2_cpu)
    assert abs(l2_gpu - l2_cpu) <= 1e-5 * max(1.0, abs(l2_cpu))
    assert (img_gpu - img_cpu).abs().max().item() <= 2e-5

    # ---- driver side: as in the frozen test
    drivers = sorted(n for n in want if not n.startswith(("generator.", "encoder.pose.")))
    assert "bases" in drivers and "delta" in drivers and set(drivers) <= set(got)
    d_errs = {n: rel_l2(got[n], want[n]) for n in drivers}
    assert all(e <= 2e-4 for e in d_errs.values()), {n: e for n, e in d_errs.items() if e > 2e-4}

    # ---- generator side: every parameter on the synthesis path (the mapping network is not: HFA-GP never calls it)
    gens = sorted(n for n in want if n.startswith("generator.") and float(want[n].abs().max()) > 0)
    assert len(gens) >= 100, len(gens)                       # 14 + 6 synthesis layers x (weight, bias, affine.*, noise) + toRGBs + decoder
    missing = [n for n in gens if n not in got]
    assert not missing, missing
    kinds = {"weight": 0, "affine": 0, "bias": 0, "noise_strength": 0, "const": 0, "decoder": 0}
    t_errs, s_errs = {}, {}
    for n in gens:
        for k in kinds:
            if k in n:
                kinds[k] += 1
        if want[n].numel() == 1:
            s_errs[n] = abs(float(got[n]) - float(want[n]))
        else:
            t_errs[n] = rel_l2(got[n], want[n])
    assert all(v > 0 for v in kinds.values()), kinds
    worst = max(t_errs, key=t_errs.get)
    conv_w = {n: e for n, e in t_errs.items() if n.endswith(("conv0.weight", "conv1.weight"))}
    worst_w = max(conv_w, key=conv_w.get)
    print(f"own-size TUNED {mode} step: l2 hip {l2_gpu:.8f} oracle {l2_cpu:.8f}; drivers worst {max(d_errs.values()):.2e}; "
          f"{len(t_errs)} generator tensors: worst {worst} {t_errs[worst]:.2e}, worst conv weight {worst_w} {conv_w[worst_w]:.2e}; "
          f"{len(s_errs)} scalars")
    bad = {n: e for n, e in t_errs.items() if not (e <= 2e-3)}
    assert not bad, bad
    # scalars (noise strengths): |error| against the size of the LARGEST tensor-valued noise-free quantity is meaningless; use the
    # scalar's own magnitude with a floor at the scale at which the oracle's fp32 sum itself is uncertain (sum over R^2 positions
    # x Cout channels of products g * noise of magnitude |g|_rms: eps_fp32 * sqrt(N) * rms — a few 1e-4 of the rms product sum)
    top = max(abs(float(want[n])) for n in s_errs)
    print("scalars (got, want):", {n.replace("generator.", ""): (round(float(got[n]), 7), round(float(want[n]), 7)) for n in s_errs})
    for n, e in s_errs.items():
        ref = abs(float(want[n]))
        assert e <= 5e-2 * ref + 5e-3 * top, (n, float(got[n]), float(want[n]))


@pytest.mark.parametrize("shape", [(2, 512, 512, 3), (2, 64, 64, 96), (3, 37, 5, 96), (1, 9, 7, 40), (2, 16, 16, 128), (1, 1, 1, 3)])
def test_channel_sum_flat_walk(dev, shape):
    """hfagp_channel_sum (round 5: flat walk with a grid stride that is a multiple of C; the toRGB bias gradients of the tuned step)
    against torch.sum in fp64, accumulate on and off, ragged sizes; bit-repeatable."""
    from hfa_gp_amd import ops
    g = torch.randn(*shape, generator=torch.Generator().manual_seed(5)).to(dev)
    want = g.double().sum(dim=(0, 1, 2))
    out = torch.full((shape[-1],), 3.0, device=dev)
    ops.channel_sum(g, out, accumulate=True)
    out2 = torch.full((shape[-1],), 3.0, device=dev)
    ops.channel_sum(g, out2, accumulate=False)
    again = torch.empty_like(out2)
    ops.channel_sum(g, again, accumulate=False)
    tol = 1e-5 * (g.abs().double().sum(dim=(0, 1, 2)) + 1.0)
    assert bool(((out.double() - 3.0 - want).abs() <= tol).all()), (out.double() - 3.0 - want).abs().max()
    assert bool(((out2.double() - want).abs() <= tol).all())
    assert torch.equal(out2, again)


def test_bench_with_a_forced_one_rank_rccl_group_reports_its_algorithm_field(tmp_path):
    """First-contact hardening: `HFAGP_BENCH_FORCE_DIST=1 python bench.py` drives every collective call of the
    N > 1 path through a ONE-rank RCCL group on this box — init with device_id, the probe all-reduce, the trainers' bucketed
    all-reduces, barriers, the MAX reduction of the timing — with RCCL's INFO log (INIT + TUNING) captured per rank; the line must
    carry `allreduce_us.algo`: the algorithm / protocol per payload on a multi-GPU node, here the note that one rank never runs
    RCCL's tuning model, plus the RCCL version read from the log (proof that the log was written and parsed)."""
    import json
    import subprocess
    import sys
    from tests.util import ROOT
    env = dict(os.environ, HFAGP_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("NCCL_DEBUG", "NCCL_DEBUG_SUBSYS", "NCCL_DEBUG_FILE", "RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    run = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "2", "--warmup", "1", "--batch", "2", "--no-cpu-baseline",
                          "--no-sweep", "--audio-frames", "0", "--fit-frames", "0", "--fit3dmm-frames-per-rank", "0", "--no-lpips",
                          "--no-fp32-leg", "--no-f16-leg", "--train-steps", "2", "--detail", str(tmp_path / "detail.json")],
                         capture_output=True, text=True, timeout=900, env=env)
    assert run.returncode == 0, run.stderr[-3000:]
    # ONE line on stdout, short enough for the driver's parser (round 5's 21.6 KB line came back unparsed); the tables live in the
    # detail file
    assert len(run.stdout.strip().splitlines()) == 1
    assert len(run.stdout.strip()) <= 6000, len(run.stdout.strip())
    line = json.loads(run.stdout.strip())
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "data", "config", "roofline"):
        assert key in line, key
    assert {"bound", "achieved", "peak", "frac", "traffic", "avg_launch_ms"} <= set(line["roofline"])
    detail = json.load(open(tmp_path / "detail.json"))
    algo = detail["allreduce_us"]["algo"]
    assert algo is not None and ("by_payload_bytes" in algo or "note" in algo), algo
    assert algo.get("rccl") and "version" in algo["rccl"].lower(), algo      # the per-rank RCCL log exists and was read
    assert line["n_gpus"] == 1 and line["train_step_ms_generator_tuned"] > 0


def test_tuned_generator_forward_uses_the_updated_weights(dev):
    """Round-5 find: `torch.optim.Adam(fused=True)` (what the trainers build) updates parameters WITHOUT advancing `_version`, the key
    of the generator's weight-image / wsq / scalar caches — rounds 2-4 ran the generator-tuned step on the weight images of step 0.
    After real Adam steps with the generator being tuned, `synthesis` must equal the synthesis of a FRESH (frozen) generator loaded
    with the updated state_dict — same kernels and weight images; the tuned path adds the noise as a pre-scaled image (noise x strength
    rounded once more than the frozen path's fused multiply-add, so 1e-6-level differences, not bits) — and the weights must indeed
    have moved.  With the stale images of rounds 2-4 the two differ at the 1e-3 level after three steps of lr 2e-3."""
    from hfa_gp_amd.generator import TriPlaneGenerator
    from hfa_gp_amd.trainer import Trainer
    from tests.test_gpu_round4 import RankArgs, _rank_frames
    torch.manual_seed(3)
    tr = Trainer(RankArgs(), dev, mode="3dmm", lpips="none")
    tr.tune_generator()
    gen = tr.gen.generator
    cfg = gen.cfg
    before = {n: p.detach().clone() for n, p in gen.named_parameters()}
    real, params, label, us, ui = (t.to(dev) for t in _rank_frames(2, cfg))
    sf = ui.shape[-1]
    for _ in range(3):
        tr.gen_update(real, label.clone(), params, u_strat=us, u_imp=ui.reshape(-1, sf).contiguous())
    moved = [n for n, p in gen.named_parameters() if not torch.equal(p.detach(), before[n])]
    assert any(n.endswith("conv1.weight") for n in moved) and any(n.endswith("noise_strength") for n in moved), moved[:5]
    ws = torch.randn(2, cfg.num_ws, 512, generator=torch.Generator().manual_seed(9)).to(dev)
    with torch.no_grad():
        got = gen.synthesis(ws, label.clone(), noise_mode="const", u_strat=us, u_imp=ui.reshape(-1, sf).contiguous())["image"]
        fresh = TriPlaneGenerator(cfg, seed=0).to(dev)
        fresh.load_state_dict(gen.state_dict())
        fresh.requires_grad_(False)
        want = fresh.synthesis(ws, label.clone(), noise_mode="const", u_strat=us, u_imp=ui.reshape(-1, sf).contiguous())["image"]
    err, scale = (got - want).abs().max().item(), want.abs().max().item()
    assert err <= 2e-5 * scale, (err, scale)
    # ... and the step-0 weights give a visibly different image (the test would be vacuous otherwise)
    stale = TriPlaneGenerator(cfg, seed=0).to(dev)
    stale.load_state_dict({n: (before[n[len(""):]] if n in before else v) for n, v in gen.state_dict().items()})
    stale.requires_grad_(False)
    with torch.no_grad():
        old = stale.synthesis(ws, label.clone(), noise_mode="const", u_strat=us, u_imp=ui.reshape(-1, sf).contiguous())["image"]
    assert (old - want).abs().max().item() > 50 * max(err, 1e-7), ((old - want).abs().max().item(), err)


@pytest.mark.parametrize("cout,cin,k", [(128, 64, 3), (96, 256, 1), (512, 512, 3), (32, 32, 3)])
def test_weight_prep_batch_equals_the_per_layer_calls(dev, cout, cin, k):
    """hfagp_weight_prep_batch (one launch: forward image, image of the Cin/Cout transpose, wsq, from one read of the weight through
    LDS) is BIT-IDENTICAL to hfagp_weight_prep_prec of the weight, of its transpose, and to hfagp_weight_prep's wsq, for every pair
    of operand kinds the generator uses; several items in one call."""
    from hfa_gp_amd import ops
    g = torch.Generator().manual_seed(cout + cin + k)
    w1 = (torch.randn(cout, cin, k, k, generator=g) * 3.0).to(dev)
    w2 = torch.randn(cin, cout, k, k, generator=g).to(dev)
    items = [(w1, "f16x3", "bf16x3", True), (w2, "bf16x3", None, False), (w1, "f16", "bf16x6", True), (w2, None, "bf16x3", True)]
    outs = ops.weight_prep_batch(items)
    for (w, prec, prec_t, want_wsq), (img, img_t, wsq) in zip(items, outs):
        if prec is not None:
            assert torch.equal(img, ops.weight_prep_prec(w, prec)), prec
        else:
            assert img is None
        if prec_t is not None:
            assert torch.equal(img_t, ops.weight_prep_prec(w.transpose(0, 1).contiguous(), prec_t)), prec_t
        else:
            assert img_t is None
        if want_wsq:
            ref = (w.double() ** 2).sum(dim=(2, 3)).float()
            assert torch.allclose(wsq, ref, rtol=1e-6, atol=0)
            if k == 3:
                assert torch.equal(wsq, ops.weight_prep(w)[1])
        else:
            assert wsq is None


def test_multi_tensor_adam_matches_torch_adam(dev):
    """trainer.MultiTensorAdam (hfagp_adam_step: one launch over device-resident pointer tables) against torch.optim.Adam's reference
    (non-fused) implementation: ragged sizes (1, 3, 4257, one chunk + 5, several chunks), a parameter without a gradient (skipped: no
    moment decay, no step advance), three steps with changing gradients, then a state_dict round trip into torch's own Adam."""
    from hfa_gp_amd.trainer import MultiTensorAdam
    g = torch.Generator().manual_seed(12)
    shapes = [(), (3,), (33, 129), (16384 + 5,), (512, 512, 3, 3), (7, 11)]
    mine = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in mine]
    o1 = MultiTensorAdam(mine, lr=3e-4)
    o2 = torch.optim.Adam(ref, lr=3e-4, foreach=False, fused=False)
    for step in range(3):
        for k, (a, b) in enumerate(zip(mine, ref)):
            if k == len(shapes) - 1 and step != 1:
                a.grad = b.grad = None                      # absent in steps 0 and 2
                continue
            gr = (torch.randn(tuple(a.shape), generator=g) * (10.0 ** (step - 1))).to(dev)
            a.grad, b.grad = gr.clone(), gr.clone()
        o1.step()
        o2.step()
    for a, b, s in zip(mine, ref, shapes):
        assert torch.allclose(a, b, rtol=2e-6, atol=2e-7), (s, (a - b).abs().max().item())
        assert torch.allclose(o1.state[a]["exp_avg"], o2.state[b]["exp_avg"], rtol=2e-6, atol=1e-9), s
        assert torch.allclose(o1.state[a]["exp_avg_sq"], o2.state[b]["exp_avg_sq"], rtol=2e-6, atol=1e-12), s
        assert float(o1.state[a]["step"]) == float(o2.state[b]["step"]), s
    assert float(o1.state[mine[-1]]["step"]) == 1.0
    o3 = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in mine], lr=3e-4)
    o3.load_state_dict(o1.state_dict())                     # same layout as torch's
    o1b = MultiTensorAdam([torch.nn.Parameter(p.detach().clone()) for p in mine], lr=3e-4)
    o1b.load_state_dict(o2.state_dict())                    # ... and torch's (host-side `step`) loads into ours
    for p in o1b.param_groups[0]["params"]:
        p.grad = torch.ones_like(p)
    o1b.step()
    assert float(o1b.state[o1b.param_groups[0]["params"][0]]["step"]) == 4.0


# ----------------------------------------------------------------------------- ray-march backward as sort + gather (ABI 12)
def _raybwd_case(dev, cfg, b, seed, h=None, w=None, **override):
    from hfa_gp_amd.generator import TriPlaneGenerator
    from tests.util import make_inputs
    gen = perturb_state(TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    ws, c, us, ui = (t.to(dev) for t in make_inputs(cfg, b, seed=seed))
    gdev = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        if h is None:
            planes = gen.backbone_planes(ws)
            pam = gen._planes_absmax
        else:
            planes = torch.randn(b, 3, h, w, 32, device=dev, generator=gdev)
            pam = None
        u_s, u_i = gen._uniforms(b, dev, us, ui)
        g = torch.randn(b, cfg.neural_rendering_resolution ** 2, 32, device=dev, generator=gdev)
    kw = dict(gen._render_args(c), u_strat=u_s, u_imp=u_i, planes_absmax=pam)
    kw.update(override)
    return g, planes, kw


@pytest.mark.parametrize("dec", [False, True])
def test_raymarch_backward_sort_gather_equals_the_scatter_kernels(dev, dec):
    """`HfagpRaymarchBwdArgs::rows_scratch` (csrc/raymarch_rows.hip) at BASELINE's size (2 frames x 128^2 rays x 96 samples, mirrored
    256^2 planes): the samples are counting-sorted by (plane, column strip, texel row), dL/dF goes to the sorted slots and every
    output row tile is W . dL/dF on the 16-bit matrix pipe (split bf16: 2^-16 per product) — against the column kernel's per-sample
    scatter with fp32 weights.  With `dec` the decoder-MLP gradients come out of the same pass that writes dL/dF."""
    from hfa_gp_amd import ops
    from hfa_gp_amd.config import ffhq512_128
    g, planes, kw = _raybwd_case(dev, ffhq512_128(), 2, 12)
    with torch.no_grad():
        ref = ops.raymarch_bwd(g, planes, rows=False, decoder_grads=dec, **kw)
        out = ops.raymarch_bwd(g, planes, rows=True, decoder_grads=dec, **kw)
        again = ops.raymarch_bwd(g, planes, rows=True, decoder_grads=dec, **kw)
    dref, dout, dagain = (ref[0], out[0], again[0]) if dec else (ref, out, again)
    scale = dref.abs().max().item()
    assert scale > 0 and torch.isfinite(dout).all()
    assert (dout - dref).abs().max().item() <= 2e-5 * scale
    assert rel_l2(dout, dref) <= 2e-5
    # a second call reuses nothing of the first (the scratch buffer's contents are undefined between calls)
    assert (dagain - dout).abs().max().item() <= 1e-5 * scale
    if dec:
        for x, y in zip(out[1], ref[1]):
            assert (x - y).abs().max().item() <= 2e-5 * y.abs().max().item()


@pytest.mark.parametrize("h,w,axes,box_warp", [(40, 72, "eg3d_original", 1.0), (33, 33, "eg3d_fixed", 1.0), (64, 64, "eg3d_original", 0.45),
                                               (20, 100, "eg3d_fixed", 0.6)])
def test_raymarch_backward_sort_gather_ragged_planes_and_rays_leaving_the_box(dev, h, w, axes, box_warp):
    """Planes that are not a multiple of the 32-texel strip, non-square planes and the fixed axes (three planes sorted instead of
    two + the mirror), and a box so small that most samples have taps outside the planes (zeros padding: they are in no bin or
    contribute to one row / column only): sort + gather against the per-sample scatter of `raymarch_bwd_tiles_kernel`."""
    import dataclasses
    from hfa_gp_amd import ops
    from hfa_gp_amd.config import PRESETS
    cfg = dataclasses.replace(PRESETS["small128"](), neural_rendering_resolution=24, img_resolution=96, plane_axes=axes)
    g, planes, kw = _raybwd_case(dev, cfg, 3, 5, h=h, w=w, box_warp=box_warp)
    with torch.no_grad():
        ref = ops.raymarch_bwd(g, planes, rows=False, **kw)
        out = ops.raymarch_bwd(g, planes, rows=True, **kw)
    scale = ref.abs().max().item()
    assert scale > 0 and torch.isfinite(out).all()
    assert (out - ref).abs().max().item() <= 2e-5 * scale
    assert rel_l2(out, ref) <= 2e-5


# ----------------------------------------------------------------------------- batched small gradients (ABI 12)
def test_bias_noise_and_affine_gradient_batches_equal_the_per_layer_forms(dev):
    """`hfagp_bias_noise_grads` / `hfagp_affine_grad_batch` (one launch per block / per pass, accumulating into the .grad slices)
    against the framework reductions and the per-layer `hfagp_affine_grad` they replace; more than 32 items (two launches),
    items without a noise strength, accumulation into non-zero targets."""
    from hfa_gp_amd import ops
    g = torch.Generator(device=dev).manual_seed(3)
    items, want = [], []
    for i in range(35):
        b, c = 2 + i % 3, (4, 32, 96, 512, 260)[i % 5]
        sums = torch.randn(b, 10, c, device=dev, generator=g)
        db = torch.randn(c, device=dev, generator=g)
        dn = torch.randn(1, device=dev, generator=g) if i % 4 else None
        want.append((db + sums[:, 4].sum(0), None if dn is None else dn + sums[:, 5].sum()))
        items.append((sums, db, dn))
    ops.bias_noise_grads(items)
    for (sums, db, dn), (wb, wn) in zip(items, want):
        assert (db - wb).abs().max().item() <= 1e-5 * max(1.0, wb.abs().max().item())
        if dn is not None:
            assert abs((dn - wn).item()) <= 1e-4 * max(1.0, abs(wn.item()))
    ws = torch.randn(3, 14, 512, device=dev, generator=g)
    aff, ref = [], []
    for i in range(34):
        cin = (512, 256, 64, 32, 3)[i % 5]
        dstot = torch.randn(3, cin, device=dev, generator=g)
        dA, dbb = torch.randn(cin, 512, device=dev, generator=g), torch.randn(cin, device=dev, generator=g)
        rA, rb = dA.clone(), dbb.clone()
        ops.affine_grad(dstot, ws[:, i % 14], rA, rb)
        aff.append((dstot, ws[:, i % 14], dA, dbb))
        ref.append((rA, rb))
    ops.affine_grad_batch(aff)
    for (_, _, dA, dbb), (rA, rb) in zip(aff, ref):
        assert torch.equal(dA, rA) and torch.equal(dbb, rb)


def test_weight_gradient_reads_dd_with_a_row_stride(dev):
    """`HfagpWgradArgs::dd_stride`: row 3 of pointwise_bwd's sums [B][10][C] goes in as a view — same bits as the contiguous copy."""
    from hfa_gp_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    b, h, cin, cout = 2, 32, 64, 128
    x = torch.randn(b, h, h, cin, device=dev, generator=g)
    gy = torch.randn(b, h, h, cout, device=dev, generator=g)
    w = torch.randn(cout, cin, 3, 3, device=dev, generator=g)
    st = torch.randn(b, cin, device=dev, generator=g)
    sums = torch.randn(b, 10, cout, device=dev, generator=g)
    dcoef = torch.rand(b, cout, device=dev, generator=g) + 0.5
    for prec in ("bf16x3", "fp32"):
        a = ops.conv_wgrad(x, st, gy, w, ops.CONV3X3, dd=sums[:, 3], dcoef=dcoef, precision=prec)
        c = ops.conv_wgrad(x, st, gy, w, ops.CONV3X3, dd=sums[:, 3].contiguous(), dcoef=dcoef, precision=prec)
        assert torch.equal(a, c)


@pytest.mark.parametrize("m,n", [(7168, 50), (7168, 64), (1000, 3), (64, 17), (65, 1)])
def test_tall_gram_matches_the_matrix_product(dev, m, n):
    """`hfagp_tall_gram` (X^T Y of tall-skinny operands in 64-row blocks + a fixed-order reduction; the three K = 7168 products of the
    latent basis' QR and its backward) against fp64, with row-major, column-major (the basis arrives as the transpose of [n, m]) and
    mixed operands, a scale, ragged m."""
    from hfa_gp_amd import ops
    g = torch.Generator(device=dev).manual_seed(m + n)
    x = torch.randn(m, n, device=dev, generator=g)
    yt = torch.randn(n, m, device=dev, generator=g)
    for a, b, sc in ((x, x, 1.0), (yt.T, yt.T, 1.0), (x, yt.T, -1.0), (yt.T, x, 0.5)):
        got = ops.tall_gram(a, b, sc)
        ref = (sc * (a.double().T @ b.double())).float()
        assert got.shape == (n, n)
        assert (got - ref).abs().max().item() <= 2e-6 * math.sqrt(m) * max(1.0, ref.abs().max().item() / math.sqrt(m))
    again = ops.tall_gram(x, x)
    assert torch.equal(again, ops.tall_gram(x, x))          # fixed summation order


def test_deferred_partial_sum_reduction_equals_the_immediate_one(dev):
    """`hfagp_pointwise_bwd` with sums = NULL + `hfagp_reduce_partials_batch` (all fused passes of a frozen-generator backward reduced
    in ONE launch at its end) gives the per-pass reducer's sums (to the summation order), deterministically, for passes of different batch / channel / chunk counts."""
    from hfa_gp_amd import ops
    g = torch.Generator(device=dev).manual_seed(21)
    cases, deferred, ref = [(2, 64, 128), (1, 16, 512), (3, 8, 40), (2, 128, 64)], [], []
    for b, h, c in cases:
        x = torch.randn(b, h, h, c, device=dev, generator=g)
        d = torch.randn(b, h, h, c, device=dev, generator=g)
        s = torch.randn(b, c, device=dev, generator=g)
        prod = dict(dcoef=torch.rand(b, c, device=dev, generator=g) + 0.5, bias=torch.randn(c, device=dev, generator=g),
                    noise=torch.randn(h, h, device=dev, generator=g), noise_strength=0.1, act="lrelu", alpha=0.2, gain=math.sqrt(2.0),
                    clamp=256.0)
        g0, s0 = ops.pointwise_bwd(x, dxs_conv=d, s_conv=s, producer=prod)
        g1, s1 = ops.pointwise_bwd(x, dxs_conv=d, s_conv=s, producer=prod, deferred=deferred)
        assert torch.equal(g0, g1)
        ref.append((s0, s1))
    assert len(deferred) == len(cases)
    ops.reduce_partials_batch(deferred)
    assert not deferred
    for s0, s1 in ref:
        assert (s0 - s1).abs().max().item() <= 2e-6 * s0.abs().max().item()        # (a different, equally fixed, summation order)
    again = []
    for (b, h, c), (s0, s1) in zip(cases[:1], ref[:1]):
        x = torch.randn(b, h, h, c, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
        _, t0 = ops.pointwise_bwd(x, dxs_conv=x, s_conv=torch.ones(b, c, device=dev), deferred=again)
        _, t1 = ops.pointwise_bwd(x, dxs_conv=x, s_conv=torch.ones(b, c, device=dev), deferred=again)
    ops.reduce_partials_batch(again)
    assert torch.equal(t0, t1)                                                     # deterministic


@pytest.mark.parametrize("b", [1, 4])
def test_raymarch_backward_sort_gather_other_batches(dev, b):
    """One frame (fewer bins than the scan tile) and four (16 448 bins: the scan kernel walks two LDS tiles with a carry) at
    BASELINE's plane / ray sizes: sort + gather against the scatter kernels."""
    from hfa_gp_amd import ops
    from hfa_gp_amd.config import ffhq512_128
    g, planes, kw = _raybwd_case(dev, ffhq512_128(), b, 30 + b)
    with torch.no_grad():
        ref = ops.raymarch_bwd(g, planes, rows=False, **kw)
        out = ops.raymarch_bwd(g, planes, rows=True, **kw)
    scale = ref.abs().max().item()
    assert scale > 0 and torch.isfinite(out).all()
    assert (out - ref).abs().max().item() <= 2e-5 * scale
    assert rel_l2(out, ref) <= 2e-5
