"""Times the Discrete Auto Diffuser's kernels against the stock-torch compositions they replace, in one process on one GPU:

    python tools/dad_bench.py [--iters 200] [--out profiles/dad_bench.txt]

At (B, T, K) = (50, 16, 128) and (32, 64, 8192): ``otvae::soft_cross_entropy`` forward and forward + backward against the reference's
composition (model/discrete_auto_diffuser.py:63-72) in fp32; ``otvae_categorical_sample`` against softmax + ``torch.multinomial``;
``otvae_codebook_gather`` against ``one_hot @ codebook`` (d = 64).  HIP events around ``iters`` back-to-back calls after a warm-up of
the same length, the median of 5 such blocks; GB/s of the forward against its algorithmic bytes 2 * B * (T - 1) * K * 4."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ot_vae_lightning_amd  # noqa: E402,F401
from ot_vae_lightning_amd import functional as HF  # noqa: E402


def timed(fn, iters):
    """median over 5 blocks of the mean time of one call, in microseconds"""
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    blocks = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        blocks.append(a.elapsed_time(b) * 1e3 / iters)
    return statistics.median(blocks)


def reference_ce(logits, probs):
    sl, sp = logits[:, :-1].contiguous(), probs[:, 1:].contiguous()
    return F.cross_entropy(sl.transpose(-1, -2), sp.transpose(-1, -2), reduction="none").sum(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; {args.iters} calls per block, median of 5 blocks; times in us"]
    for B, T, K in ((50, 16, 128), (32, 64, 8192)):
        g = torch.Generator().manual_seed(0)
        logits = torch.randn(B, T, K, generator=g).cuda()
        probs = torch.softmax(torch.randn(B, T, K, generator=g), -1).cuda()
        gl = torch.ones(B, device="cuda")
        lg, pg = logits.clone().requires_grad_(True), probs.clone().requires_grad_(True)

        def fb(ce):
            lg.grad = pg.grad = None
            ce(lg, pg).backward(gl)

        hip_f = timed(lambda: torch.ops.otvae.soft_cross_entropy(logits, probs), args.iters)
        ref_f = timed(lambda: reference_ce(logits, probs), args.iters)
        hip_fb = timed(lambda: fb(HF.soft_cross_entropy), args.iters)
        ref_fb = timed(lambda: fb(reference_ce), args.iters)
        nbytes = 2 * B * (T - 1) * K * 4
        lines.append(f"soft CE ({B},{T},{K}): forward hip {hip_f:8.1f}  torch {ref_f:8.1f}  ({ref_f / hip_f:4.1f}x)   "
                     f"{nbytes / hip_f / 1e3:7.1f} GB/s of {nbytes / 1e6:.2f} MB;  forward+backward hip {hip_fb:8.1f}  torch {ref_fb:8.1f}  "
                     f"({ref_fb / hip_fb:4.1f}x)")
        ids = torch.zeros(B, T, dtype=torch.int64, device="cuda")
        u = torch.rand(B, generator=g).cuda()
        hip_s = timed(lambda: HF.categorical_sample_(ids, 1, logits, 0, u=u), args.iters)
        ref_s = timed(lambda: torch.multinomial(logits[:, 0].softmax(-1), 1), args.iters)
        lines.append(f"sample  ({B},{K}): otvae_categorical_sample {hip_s:8.1f}  softmax + torch.multinomial {ref_s:8.1f}  ({ref_s / hip_s:4.1f}x)")
        d = 64
        cb = torch.randn(K, d, generator=g).cuda()
        tok = torch.randint(0, K, (B, T), generator=g).cuda()
        hip_g = timed(lambda: HF.codebook_gather(cb, tok), args.iters)
        ref_g = timed(lambda: F.one_hot(tok, K).type_as(cb) @ cb, args.iters)
        lines.append(f"gather  ({B},{T},{K},{d}): otvae_codebook_gather {hip_g:8.1f}  one_hot @ codebook {ref_g:8.1f}  ({ref_g / hip_g:4.1f}x)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
