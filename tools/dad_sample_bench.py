"""Times ``DAD.sample`` on its two routes -- the whole id matrix through the decoder T - 1 times (``cached=False``) and one token at a
time on key / value caches (``cached=True``) -- in one process on one GPU:

    python tools/dad_sample_bench.py [--iters 5] [--out profiles/dad_sample_bench.txt]

The autoregressive decoder is the reference's DAD configuration (configs/dad/defaults.yaml: dim 128, depth 2, 8 heads, mlp 512,
K = 8192) at (a) T = 16, B = 128 and (b) T = 256, B = 32; encoder and decoder are small ViTs (the decode tail is the same on both
routes).  HIP events around ``iters`` back-to-back ``sample`` calls after a warm-up of the same length, the median of 5 such blocks;
launches per token = device kernels of one decoder pass (or step) plus one draw, counted by the profiler."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ot_vae_lightning_amd as A  # noqa: E402
from ot_vae_lightning_amd import functional as HF  # noqa: E402


def timed(fn, iters):
    """median over 5 blocks of the mean time of one call, in milliseconds"""
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
        blocks.append(a.elapsed_time(b) / iters)
    return statistics.median(blocks)


def build(image_size, K=8192):
    v = dict(image_size=image_size, patch_size=4, dim=16, depth=1, heads=4, mlp_dim=32, channels=1, dropout=0.0, emb_dropout=0.)
    enc = A.ViT(n_embed_tokens=0, n_input_tokens=None, output_tokens="input", patch_to_embed=True, embed_to_patch=False, **v)
    dec = A.ViT(n_embed_tokens=None, n_input_tokens=enc.total_num_tokens, output_tokens="input", patch_to_embed=False,
                embed_to_patch=True, **v)
    ar = A.AutoRegressive(vocab_size=K, image_size=image_size, patch_size=4, dim=128, depth=2, heads=8, mlp_dim=512, channels=1,
                          dropout=0.0, emb_dropout=0., n_embed_tokens=0, n_input_tokens=enc.total_num_tokens, output_tokens="input",
                          patch_to_embed=False, embed_to_patch=False, causal_mask=True)
    prior = A.CodebookPrior(latent_size=enc.out_size, embed_dims=(2,), loss=None, loss_coeff=1.0, annealing_steps=0,
                            mixture_cfg=dict(n_components=K, metric="euclidean", temperature=1.0, training_mode="gumbel-softmax",
                                             inference_mode="gumbel-softmax"), update_with_autograd=True)
    return A.DAD(encoder=enc, decoder=dec, autoregressive_decoder=ar, prior=prior, ce_coeff=1.0).cuda().eval()


def launches_per_token(model, B, cached):
    from torch.profiler import ProfilerActivity, profile
    ar, T = model.autoregressive_decoder, model.n_tokens
    ids = torch.randint(0, model.num_embeddings, (B, T), device="cuda")
    u = torch.rand(B, device="cuda")
    state = ar.decode_state(B) if cached else None

    def one(i):
        with torch.no_grad():
            if cached:
                HF.categorical_sample_(ids, i + 1, ar.step(ids[:, i], state).unsqueeze(1), 0, u=u)
            else:
                HF.categorical_sample_(ids, i + 1, ar(ids), i, u=u)

    one(0)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        one(1)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; DAD.sample, decoder dim 128 / depth 2 / 8 heads / mlp 512 / K 8192; {args.iters} calls "
             f"per block, median of 5 blocks; ms per sample() call (T - 1 generated tokens per row, codebook gather and decode included)"]
    for tag, image_size, B in (("(a)", 16, 128), ("(b)", 64, 32)):
        model = build(image_size)
        T = model.n_tokens
        with torch.no_grad():
            ms = {c: timed(lambda: model.sample(B, cached=c), args.iters) for c in (False, True)}
        n = {c: launches_per_token(model, B, c) for c in (False, True)}
        lines.append(f"{tag} T = {T:3d}, B = {B:3d}: cached=False {ms[False]:9.3f} ms  {n[False]:3d} launches / token;   cached=True "
                     f"{ms[True]:9.3f} ms  {n[True]:3d} launches / token;   {ms[False] / ms[True]:6.2f}x")
        del model
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
