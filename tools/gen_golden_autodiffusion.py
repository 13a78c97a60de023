"""Records ``tests/golden/autodiffusion.npz`` from the reference's own conditioned ``AutoEncoder`` (networks/cnn.py) and
``GaussianFourierProjection`` (networks/nets_utils.py) on the CPU.

    python tools/gen_golden_autodiffusion.py     # needs the reference checkout (OTVAE_REFERENCE_ROOT), build container only

Two modules, each run in float32 (the reference as it is) and again as the same module in ``.double()`` (the truth the GPU tests
measure both sides against) on the same weights and inputs:

    ae   AutoEncoder(1, 4, 8, 2, capacity=4, num_classes=10, time_embed_dim=8, residual="add", down_up_sample=True), train mode:
         h = encode(x, labels, time), y = decode(h, labels, time), the gradients of y.square().mean() for every parameter
    gfp  GaussianFourierProjection(8, 8): out = gfp(time), the gradients of out.square().mean()

B = 6; the times include exactly 0.0 and 1.0.  Layout of the file:

    <m>/names                  state-dict keys in order (both ``proj.2.*`` and ``proj.4.*``: one Linear object used twice)
    <m>/state/<key>            float32 values (int64 for num_batches_tracked), as constructed under the seed
    <m>/x, <m>/labels, <m>/time
    <m>/f32/..., <m>/f64/...   h, y (ae) or out (gfp) and grad/<parameter name> (``named_parameters``: a shared tensor once, under
                               its first name, holding the sum over its uses)

Data only: arrays and lists of names."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_import as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "autodiffusion.npz")
B = 6


def _record(out, tag, module, run):
    """names / state once, then the results of ``run(module)`` in float32 and of the same module in float64"""
    state = {k: v.detach().clone() for k, v in module.state_dict().items()}
    out[f"{tag}/names"] = np.array(list(state.keys()))
    for k, v in state.items():
        out[f"{tag}/state/{k}"] = v.numpy()
    for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        m = module if dtype is torch.float32 else module.double()
        m.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in state.items()})   # (running buffers as recorded)
        m.train()
        m.zero_grad(set_to_none=True)
        results, loss = run(m, dtype)
        loss.backward()
        for k, v in results.items():
            out[f"{tag}/{prec}/{k}"] = v.detach().numpy()
        for k, p in m.named_parameters():
            if p.grad is not None:
                out[f"{tag}/{prec}/grad/{k}"] = p.grad.detach().numpy()


def main():
    cnn, nets_utils = R.ref("networks.cnn"), R.ref("networks.nets_utils")
    g = torch.Generator().manual_seed(20240611)
    x = torch.randn(B, 1, 8, 8, generator=g)
    labels = torch.tensor([3, 0, 9, 9, 1, 7])
    time = torch.tensor([0.0, 1.0, 0.5, 0.03125, 0.73, 0.999])
    out = {}

    torch.manual_seed(1234)
    ae = cnn.AutoEncoder(1, 4, 8, 2, capacity=4, num_classes=10, time_embed_dim=8, residual="add", down_up_sample=True)
    with torch.no_grad():   # away from the symmetric initial state: BatchNorm affines and biases that are not 1 / 0
        for name, p in ae.named_parameters():
            if name.endswith("_normalization.weight"):
                p.add_(0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith("_normalization.bias"):
                p.add_(0.1 * torch.randn(p.shape, generator=g))

    def run_ae(m, dtype):
        h = m.encode(x.to(dtype), labels, time.to(dtype))
        y = m.decode(h, labels, time.to(dtype))
        return {"h": h, "y": y}, y.square().mean()

    _record(out, "ae", ae, run_ae)
    out["ae/x"], out["ae/labels"], out["ae/time"] = x.numpy(), labels.numpy(), time.numpy()

    torch.manual_seed(4321)
    gfp = nets_utils.GaussianFourierProjection(8, 8)

    def run_gfp(m, dtype):
        o = m(time.to(dtype))
        return {"out": o}, o.square().mean()

    _record(out, "gfp", gfp, run_gfp)
    out["gfp/time"] = time.numpy()

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {len(out)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
