"""Times ``functional.gaussian_blur`` (kernel 5, sigma 1.5: the reference's degradation) against what a user can do without it, in one
process on one GPU:

    python tools/blur_bench.py [--reps 50] [--blocks 15] [--out profiles/blur_bench.txt]

per shape ([1024, 1, 32, 32], [256, 3, 32, 32], [64, 3, 64, 64], NCHW-contiguous float32):

    blur      otvae_gaussian_blur_fwd: one launch, reflection at the load, no padded copy
    stand-in  F.pad(x, (2, 2, 2, 2), mode="reflect") + F.conv2d with the 5 x 5 window, groups = C: the stand-in of
              tests/test_gpu_configs.py -- a pad pass plus a library convolution, at least twice the bytes
    copy      y.copy_(x) of the same tensor: one read and one write per element, the traffic floor

Each candidate is captured into a graph of ``--reps`` repetitions (device time, no host launch gaps); the three graphs are replayed in
turn, HIP events around every replay, the median of ``--blocks`` replays.  Every GPU step (a capture, a round of replays) runs under a
watchdog of ``--step-timeout`` seconds that ends the process: a step that hangs is not waited for."""
import argparse
import faulthandler
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ot_vae_lightning_amd import functional as HF  # noqa: E402

SHAPES = [(1024, 1, 32, 32), (256, 3, 32, 32), (64, 3, 64, 64)]
KERNEL, SIGMA = 5, 1.5


class step_limit:
    """ends the process when the enclosed GPU step takes longer than ``seconds``"""

    def __init__(self, seconds):
        self.seconds = seconds

    def __enter__(self):
        faulthandler.dump_traceback_later(self.seconds, exit=True)

    def __exit__(self, *exc):
        faulthandler.cancel_dump_traceback_later()
        return False


def candidates(shape):
    g = torch.Generator().manual_seed(0)
    x = torch.rand(shape, generator=g).cuda()
    y = torch.empty_like(x)
    half = (KERNEL - 1) * 0.5
    k1 = torch.exp(-0.5 * (torch.linspace(-half, half, KERNEL) / SIGMA).pow(2))
    k1 = k1 / k1.sum()
    c = shape[1]
    k2 = (k1[:, None] * k1[None, :]).expand(c, 1, KERNEL, KERNEL).contiguous().cuda()
    p = KERNEL // 2
    fns = {"blur": lambda: HF.gaussian_blur(x, KERNEL, SIGMA),
           "stand-in": lambda: F.conv2d(F.pad(x, (p, p, p, p), mode="reflect"), k2, groups=c),
           "copy": lambda: y.copy_(x)}
    err = (fns["blur"]() - fns["stand-in"]()).abs().max().item()
    return fns, err, (x, y, k2)


def captured(fn, reps):
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(reps):
            fn()
    return graph


def time_shape(shape, reps, blocks, limit):
    with step_limit(limit):
        fns, err, keep = candidates(shape)
        torch.cuda.synchronize()
    graphs = {}
    for tag, fn in fns.items():
        with step_limit(limit):
            graphs[tag] = captured(fn, reps)
            graphs[tag].replay()
            torch.cuda.synchronize()
    times = {tag: [] for tag in graphs}
    with step_limit(limit):
        for _ in range(blocks):
            for tag, gr in graphs.items():   # in turn
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                gr.replay()
                b.record()
                b.synchronize()
                times[tag].append(a.elapsed_time(b) * 1e3 / reps)
    del graphs, keep
    return {tag: (statistics.median(t), min(t), max(t)) for tag, t in times.items()}, err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--step-timeout", type=int, default=60)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blur_bench needs the GPU: there is nothing to time on the host")
    lines = [f"device: {torch.cuda.get_device_name(0)}; gaussian_blur kernel {KERNEL} sigma {SIGMA}, float32 NCHW",
             f"us per call (median [min, max] of {args.blocks} graph replays of {args.reps} calls, the three graphs in turn):"]
    for shape in SHAPES:
        r, err = time_shape(shape, args.reps, args.blocks, args.step_timeout)
        b, s, c = r["blur"], r["stand-in"], r["copy"]
        mb = 2 * 4 * torch.Size(shape).numel() / 1e6
        lines.append(f"  {str(list(shape)):20s} ({mb:5.2f} MB read + written): blur {b[0]:7.2f} [{b[1]:.2f}, {b[2]:.2f}]   "
                     f"stand-in {s[0]:7.2f} [{s[1]:.2f}, {s[2]:.2f}]   copy {c[0]:7.2f} [{c[1]:.2f}, {c[2]:.2f}]   "
                     f"stand-in / blur {s[0] / b[0]:5.2f}x   blur / copy {b[0] / c[0]:5.2f}x   (max |blur - stand-in| {err:.1e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
