"""Times the class / time conditioned ``AutoDiffusion`` on MNIST-32 shapes, and its FiLM kernels old against new, in one process on
one GPU:

    python tools/autodiffusion_bench.py [--batch 1024] [--steps 30] [--out profiles/autodiffusion_bench.txt]

  * ms / training step of ``AutoDiffusion(AutoEncoder(1, 128, 32, 1, capacity=8, num_classes=10, time_embed_dim=32, residual='add',
    down_up_sample=True), GaussianPrior(fixed_var=True))`` through ``HipTrainer``, eagerly issued and as a captured graph;
  * ms / ``sample()`` call (n_steps = 10: ten decodes and ten encodes), both algorithms;
  * the FiLM chain of one ConvLayer, forward + backward, at that network's own maps (N = batch, (HW, C) = (1024, 8), (256, 16), (64, 32),
    (16, 64), ReLU): the kept two-launch chain (otvae_film_fwd + otvae_bn_act_fwd; otvae_bn_act_bwd + otvae_film_bwd) against
    otvae_film_act_fwd + otvae_film_act_bwd.  Each chain is captured into a graph of ``--reps`` repetitions (device time, no host
    launch gaps), the two graphs are replayed alternately, HIP events around every replay, the median of ``--blocks`` replays.

The time of a step is a host clock around ``steps`` steps that end in a device synchronise, after a warm-up of the same length."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ot_vae_lightning_amd as A  # noqa: E402
from ot_vae_lightning_amd import _lib  # noqa: E402
from ot_vae_lightning_amd._lib import check, ptr, stream  # noqa: E402

FILM_SHAPES = [(1024, 8), (256, 16), (64, 32), (16, 64)]
RELU = 1


def build_model():
    torch.manual_seed(0)
    ae = A.AutoEncoder(1, 128, 32, 1, capacity=8, num_classes=10, time_embed_dim=32, residual="add", down_up_sample=True)
    return A.AutoDiffusion(autoencoder=ae, prior=A.GaussianPrior(loss_coeff=0.1, fixed_var=True), conditional=True).cuda()


def step_ms(batch, steps, use_graph):
    model = build_model().train()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(batch, 1, 32, 32, generator=g).cuda()
    eps = torch.randn(batch, *model.latent_size, generator=g).cuda()
    kw = {"time": torch.rand(batch, generator=g).cuda(), "labels": torch.randint(0, 10, (batch,), generator=g).cuda()}
    trainer = A.HipTrainer(model, batch_shape=(batch, 1, 32, 32), use_graph=use_graph, batch_kwargs=kw)
    for _ in range(steps):
        out = trainer.step(x, eps, **kw)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out = trainer.step(x, eps, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    loss = out.tolist()
    trainer.close()
    return ms, loss


def sample_ms(batch, iters, improved):
    model = build_model().eval()
    labels = torch.randint(0, 10, (batch,), generator=torch.Generator().manual_seed(2)).cuda()
    for _ in range(2):
        model.sample(batch, improved_algorithm=improved, labels=labels)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        model.sample(batch, improved_algorithm=improved, labels=labels)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def film_chains(n, hw, c):
    """(old, new): callables that issue one forward + backward of the FiLM chain on resident tensors"""
    lib = _lib.load()
    g = torch.Generator().manual_seed(3)
    dev = "cuda"
    x, gy = torch.randn(n, hw, c, generator=g).to(dev), torch.randn(n, hw, c, generator=g).to(dev)
    s, b = (1 + 0.5 * torch.randn(n, c, generator=g)).to(dev), (0.3 * torch.randn(n, c, generator=g)).to(dev)
    v, out, gv, gx = (torch.empty_like(x) for _ in range(4))
    gs, gb = torch.empty_like(s), torch.empty_like(s)
    nbytes = lib.otvae_film_act_bwd_ws(n, hw, c)
    ws = torch.empty(max(1, nbytes // 8), device=dev, dtype=torch.float64)

    def old():
        check(lib.otvae_film_fwd(ptr(x), ptr(s), ptr(b), n, hw, c, ptr(v), stream()), "otvae_film_fwd")
        check(lib.otvae_bn_act_fwd(ptr(v), None, None, RELU, n * hw, c, ptr(out), stream()), "otvae_bn_act_fwd")
        check(lib.otvae_bn_act_bwd(ptr(gy), ptr(v), None, None, None, None, RELU, n * hw, c, ptr(gv), None, stream()), "otvae_bn_act_bwd")
        check(lib.otvae_film_bwd(ptr(gv), ptr(x), ptr(s), n, hw, c, ptr(gx), ptr(gs), ptr(gb), stream()), "otvae_film_bwd")

    def new():
        check(lib.otvae_film_act_fwd(ptr(x), ptr(s), ptr(b), n, hw, c, RELU, ptr(out), stream()), "otvae_film_act_fwd")
        check(lib.otvae_film_act_bwd(ptr(gy), ptr(x), ptr(s), ptr(b), n, hw, c, RELU, ptr(gx), ptr(gs), ptr(gb),
                                     ptr(ws) if nbytes else None, stream()), "otvae_film_act_bwd")

    keep = (x, gy, s, b, v, out, gv, gx, gs, gb, ws)
    return old, new, keep


def captured(fn, reps):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph


def film_ab(n, hw, c, reps, blocks):
    old, new, keep = film_chains(n, hw, c)
    graphs = {"old": captured(old, reps), "new": captured(new, reps)}
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    times = {"old": [], "new": []}
    for _ in range(blocks):
        for tag in ("old", "new"):   # alternating
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            graphs[tag].replay()
            b.record()
            b.synchronize()
            times[tag].append(a.elapsed_time(b) * 1e3 / reps)
    del graphs
    return {tag: (statistics.median(t), min(t), max(t)) for tag, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("autodiffusion_bench needs the GPU: there is nothing to time on the host")
    n = args.batch
    lines = [f"device: {torch.cuda.get_device_name(0)}; AutoDiffusion MNIST-32, batch {n}, num_classes 10, time_embed_dim 32"]
    lines.append(f"FiLM chain, forward + backward, ReLU, us per chain (median [min, max] of {args.blocks} alternating graph replays of "
                 f"{args.reps} chains):")
    for hw, c in FILM_SHAPES:
        r = film_ab(n, hw, c, args.reps, args.blocks)
        o, w = r["old"], r["new"]
        lines.append(f"  N = {n} HW = {hw:4d} C = {c:2d}: old {o[0]:8.1f} [{o[1]:.1f}, {o[2]:.1f}]   new {w[0]:8.1f} [{w[1]:.1f}, {w[2]:.1f}]   "
                     f"old / new {o[0] / w[0]:5.2f}x")
    for use_graph in (False, True):
        ms, loss = step_ms(n, args.steps, use_graph)
        lines.append(f"training step, {'captured graph' if use_graph else 'eagerly issued'}: {ms:8.3f} ms / step   (loss vector after "
                     f"{2 * args.steps} steps: {[round(v, 5) for v in loss]})")
    for improved in (False, True):
        lines.append(f"sample(improved_algorithm={improved}): {sample_ms(n, 3, improved):8.3f} ms / call")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
