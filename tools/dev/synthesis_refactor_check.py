"""Developer: two checkouts of this repository against each other on `TriPlaneGenerator.synthesis` (the gate of a refactoring of the
call path; results: profiles/synthesis_refactor/README.md).  From the repository root, on the GPU box:

  synthesis_refactor_check.py dump OUT.pt [ROOT]        every forward output, ws.grad, c.grad, query.grad and every parameter gradient of
                                                        a fixed list of calls, of the package under ROOT (default: this checkout)
  synthesis_refactor_check.py compare P1.pt .. -- N1.pt ..
                                                        per tensor: reproduced bit for bit by the first group's runs -> must be bit-equal
                                                        in the second; else the largest deviation between the groups against the
                                                        largest within the first (allowed: 2 x); a markdown table, exit status 1 on a miss
  synthesis_refactor_check.py time [PARENT_ROOT] [rounds] [steps]
                                                        host (enqueue), device-event and wall time of a differentiated synthesis +
                                                        backward, medians per round; with PARENT_ROOT the two packages alternate step
                                                        by step in this one process

A ROOT without a built library of its own takes the one HFAGP_LIB_PATH names (the kernels are the same)."""
import dataclasses
import importlib.util
import itertools
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B, M = 2, 37
# (name, keywords of the call, c requires grad, query: None / "coords" / "coords_grad", rays per side, the loss's outputs or None = all
# that require grad)
CELLS = (
    ("plain", {}, False, None, 10, None),
    ("image_only_with_query", {}, False, "coords", 10, ("image",)),
    ("geometry_query_normal_camera", dict(geometry=True, normal_camera_grad=True, return_planes=True), True, "coords_grad", 10, None),
    ("query_normals_detached_normals", dict(query_normals=True, normals=True), True, "coords", 10, None),
    ("geometry_normal_grad_r7", dict(geometry=True, normal_grad=True), False, None, 7, None),
)


def load(root: str, alias: str):
    real = os.path.join(root, "hfa-gp_amd")
    spec = importlib.util.spec_from_file_location(alias, os.path.join(real, "__init__.py"), submodule_search_locations=[real])
    mod = sys.modules[alias] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return importlib.import_module(alias + ".generator"), importlib.import_module(alias + ".synthetic"), mod


def setup(root: str, alias: str, dev, tuned: bool = True):
    G, S, pkg = load(root, alias)
    cfg = dataclasses.replace(pkg.PRESETS["tiny64"](), neural_rendering_resolution=10, img_resolution=40, conv_precision="fp32")
    gen = S.perturb_state(G.TriPlaneGenerator(cfg, seed=0)).requires_grad_(False).to(dev)
    for n, p in gen.named_parameters():
        if tuned and not n.startswith("backbone.mapping."):
            p.requires_grad_(True)
    return gen, cfg, S


def call_inputs(S, cfg, dev, c_grad, query, res):
    ws, c, us, ui = (t.to(dev) for t in S.make_inputs(dataclasses.replace(cfg, neural_rendering_resolution=res), B))
    kw = dict(noise_mode="const", u_strat=us, u_imp=ui, neural_rendering_resolution=res)
    if query is not None:
        q = (torch.rand(1, M, 3, generator=torch.Generator().manual_seed(37)) - 0.5) * (0.8 * cfg.box_warp)
        kw["query"] = q.to(dev).requires_grad_(query == "coords_grad")
    return ws.requires_grad_(True), c.requires_grad_(c_grad), kw


def loss_of(out, keys, dev):
    g = torch.Generator().manual_seed(5)
    return sum((v * torch.randn(v.shape, generator=g).to(dev)).sum() for k, v in out.items()
               if v.requires_grad and (keys is None or k in keys))


def dump(path: str, root: str) -> None:
    dev = torch.device("cuda:0")
    gen, cfg, S = setup(root, "hfagp_dumped", dev)
    got = {}
    for name, kw, c_grad, query, res, keys in CELLS:
        ws, c, call = call_inputs(S, cfg, dev, c_grad, query, res)
        out = gen.synthesis(ws, c, **call, **kw)
        loss_of(out, keys, dev).backward()
        for k, v in out.items():
            got[f"{name}/out/{k}"] = v.detach().cpu()
        for k, t in (("ws", ws), ("c", c), ("query", call.get("query"))):
            if t is not None and t.grad is not None:
                got[f"{name}/grad/{k}"] = t.grad.cpu()
        for k, p in gen.named_parameters():
            if p.grad is not None:
                got[f"{name}/param/{k}"] = p.grad.cpu()
        gen.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.save(got, path)
    print(f"{path}: {len(got)} tensors")


def compare(first, second) -> int:
    first, second = [torch.load(p) for p in first], [torch.load(p) for p in second]
    assert all(set(r) == set(first[0]) for r in first + second), "the runs have different tensors"
    dev = lambda a, b: float((a.double() - b.double()).abs().max()) if a.numel() else 0.0      # noqa: E731
    bad, exact, rows = 0, {}, []
    for key in first[0]:
        cell, kind, _ = key.split("/", 2)
        if all(torch.equal(first[0][key], r[key]) for r in first[1:]):
            ok = all(torch.equal(first[0][key], r[key]) for r in second)
            n = exact.setdefault((cell, kind), [0, 0])
            n[0] += 1
            n[1] += ok
            bad += not ok
            continue
        within = max(dev(a[key], b[key]) for a, b in itertools.combinations(first, 2))
        across = max(dev(a[key], b[key]) for a in first for b in second)
        top = max(float(r[key].abs().max()) for r in first)
        bad += not across <= 2.0 * within
        rows.append(f"| `{key}` | {top:.3e} | {within:.3e} | {across:.3e} | {across / within:.2f} |")
    print("| call | tensors | reproduced bit for bit by the first group | of which bit-equal in the second |\n|---|---|---|---|")
    for (cell, kind), (n, ok) in exact.items():
        print(f"| {cell} | {kind} | {n} | {ok} |")
    print("\n| tensor (not bit-reproducible in the first group) | max abs | largest deviation within the first group | largest "
          "between the groups | ratio (allowed 2) |\n|---|---|---|---|---|")
    print("\n".join(rows))
    print(f"\n{bad} misses")
    return 1 if bad else 0


def timing(parent_root, rounds: int, iters: int) -> None:
    dev = torch.device("cuda:0")
    arms = {"new": setup(HERE, "hfagp_new", dev)}
    if parent_root:
        arms["parent"] = setup(parent_root, "hfagp_parent", dev)

    def step(gen, cfg, S):
        ws, c, call = step.inputs[id(gen)]
        ws.grad = None
        out = gen.synthesis(ws, c, **call, geometry=True)
        (out["image"].sum() + out["image_mask"].sum()).backward()

    step.inputs = {id(g): call_inputs(S, cfg, dev, False, "coords", 10) for g, cfg, S in arms.values()}
    for arm in arms.values():
        for _ in range(10):
            step(*arm)
    for _ in range(rounds):          # the arms alternate step by step; every step starts on an idle device
        times = {name: [] for name in arms}
        for _ in range(iters):
            for name, arm in arms.items():
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                step(*arm)
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                times[name].append((1e3 * (t1 - t0), e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t0)))
        for name, ts in times.items():
            host, events, wall = (sorted(t[k] for t in ts)[len(ts) // 2] for k in range(3))
            print(f"{name}: medians of {iters} steps: host {host:.4f} ms, device events {events:.4f} ms, wall {wall:.4f} ms", flush=True)


if __name__ == "__main__":
    cmd, args = sys.argv[1], sys.argv[2:]
    if cmd == "dump":
        dump(args[0], args[1] if len(args) > 1 else HERE)
    elif cmd == "compare":
        cut = args.index("--")
        sys.exit(compare(args[:cut], args[cut + 1:]))
    elif cmd == "time":
        root = args[0] if args and not args[0].isdigit() else None
        nums = [int(a) for a in args if a.isdigit()]
        timing(root, *(nums + [3, 150][len(nums):]))
    else:
        sys.exit(__doc__)
