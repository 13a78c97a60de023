"""Times the filtered token draw against the torch composition it replaces and against the unfiltered draw, in one process on one GPU:

    python tools/token_filter_bench.py [--iters 100] [--rounds 7] [--out profiles/token_filter_bench.txt]

At (B, K) = (256, 512) and (64, 8192), temperature 0.8, top-k 50, top-p 0.9:
  (a) ``otvae_filtered_sample`` (``HF.categorical_sample_`` with the three arguments): one launch;
  (b) the same draw composed in torch: scale, ``topk``, ``sort``, ``softmax``, ``cumsum``, mask, ``scatter``, ``multinomial``;
  (c) ``otvae_categorical_sample``, the floor: it reads the row and sorts nothing;
  (d) ``DAD.sample(cached=True)`` with and without the filters on tools/dad_sample_bench.py's decoder at its shape (a), T = 16,
      B = 128, with K = 2048 instead of 8192: the decoder's head is a 1x1 convolution, which takes at most 2048 channels
      (``otvae_conv_multi``), so that script's K = 8192 model cannot run a step.
Eager calls; device events around ``iters`` back-to-back calls of one variant; the variants take turns inside every round, so each
sees the same state of the machine; per variant the median over the rounds and their spread (max - min) / median."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ot_vae_lightning_amd  # noqa: E402,F401
from ot_vae_lightning_amd import functional as HF  # noqa: E402

from dad_sample_bench import build  # noqa: E402

TAU, TOP_K, TOP_P = 0.8, 50, 0.9


def torch_filtered(logits, tau, k, p):
    """the usual composition: temperature, top-k, then top-p on the renormalised survivors, one multinomial draw"""
    scaled = logits / tau
    vals, idx = torch.topk(scaled, k, dim=-1)
    vals, order = torch.sort(vals, dim=-1, descending=True)
    probs = torch.softmax(vals, -1)
    before = probs.cumsum(-1) - probs
    probs = probs.masked_fill(before >= p, 0.0)
    full = torch.zeros_like(scaled).scatter_(1, idx.gather(1, order), probs)
    return torch.multinomial(full, 1)


def interleaved(variants, iters, rounds):
    """{name: (median, spread)} of the time of one call in microseconds; the variants alternate inside every round"""
    for fn in variants.values():
        for _ in range(iters):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / iters)
    return {name: (statistics.median(t), (max(t) - min(t)) / statistics.median(t)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--sample-iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f"device: {torch.cuda.get_device_name(0)}; eager calls, device events around {args.iters} calls per variant, variants interleaved "
        f"in each of {args.rounds} rounds; median us per call (spread = (max - min) / median); temperature {TAU}, top-k {TOP_K}, top-p {TOP_P}")
    for B, K in ((256, 512), (64, 8192)):
        g = torch.Generator().manual_seed(0)
        logits = (3.0 * torch.randn(B, 1, K, generator=g)).cuda()
        row = logits[:, 0]
        ids = torch.zeros(B, 2, dtype=torch.int64, device="cuda")
        u = torch.rand(B, generator=g).cuda()
        r = interleaved({
            "a": lambda: HF.categorical_sample_(ids, 1, logits, 0, u=u, temperature=TAU, top_k=TOP_K, top_p=TOP_P),
            "b": lambda: torch_filtered(row, TAU, TOP_K, TOP_P),
            "c": lambda: HF.categorical_sample_(ids, 1, logits, 0, u=u),
        }, args.iters, args.rounds)
        say(f"({B},{K}): (a) otvae_filtered_sample {r['a'][0]:8.1f} ({r['a'][1]:.2f})   (b) torch composition {r['b'][0]:8.1f} "
            f"({r['b'][1]:.2f})   (c) otvae_categorical_sample {r['c'][0]:8.1f} ({r['c'][1]:.2f})   (b)/(a) {r['b'][0] / r['a'][0]:5.2f}x   "
            f"(a)/(c) {r['a'][0] / r['c'][0]:5.2f}x")
    model, Bs = build(16, K=2048), 128
    with torch.no_grad():
        r = interleaved({
            "plain": lambda: model.sample(Bs, cached=True),
            "filtered": lambda: model.sample(Bs, cached=True, temperature=TAU, top_k=TOP_K, top_p=TOP_P),
        }, args.sample_iters, args.rounds)
    say(f"(d) DAD.sample(cached=True), T = {model.n_tokens}, B = {Bs}, K = {model.num_embeddings}: unfiltered {r['plain'][0] / 1e3:8.3f} ms "
        f"({r['plain'][1]:.2f})   filtered {r['filtered'][0] / 1e3:8.3f} ms ({r['filtered'][1]:.2f})   "
        f"{r['filtered'][0] / r['plain'][0]:5.2f}x")
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
