"""GPU: the device-side image transforms -- ``functional.gaussian_blur`` / ``torch.ops.otvae.gaussian_blur`` and its adjoint,
``transforms.GaussianBlur``, ``functional.collage``, ``ProgressiveTransform`` on a small ``VAE`` and ``LatentTransport`` with the blur as
its degradation.

The blur is torchvision's ``gaussian_blur``.  torchvision is not installed where these goldens could be recorded, so none is: the
reference here is torchvision's own formula written out -- ``_get_gaussian_kernel1d`` per axis, the outer product as the window,
``F.pad(mode="reflect")`` and a grouped ``F.conv2d`` -- evaluated on the CPU in float32 (the reference) and in float64 (the truth).
Bounds follow the evidence rule of tests/test_gpu_autodiffusion.py::vs_truth: max(1e-4, 1.5 x the fp32 reference's own error against
the truth), relative to the truth's largest magnitude.  The collage only clamps and copies: it is compared with ``torch.equal``."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL32, FACTOR = 1e-4, 1.5


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as A_
    return A_


@pytest.fixture(scope="module")
def HF(A):
    from ot_vae_lightning_amd import functional
    return functional


def vs_truth(name, got, ref32, truth):
    t = truth.detach().double().cpu()
    scale = max(t.abs().max().item(), 1e-30)
    e_hip = (got.detach().double().cpu() - t).abs().max().item() / scale
    e_ref = (ref32.detach().double().cpu() - t).abs().max().item() / scale
    tol = max(TOL32, FACTOR * e_ref)
    print(f"[transforms] {name}: hip vs fp64 truth {e_hip:.3e}  reference fp32 vs truth {e_ref:.3e}  bound {tol:.3e}")
    assert math.isfinite(e_hip) and e_hip <= tol, (name, e_hip, e_ref, tol)


def pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def kernel1d(k, sigma, dtype):
    half = (k - 1) * 0.5
    x = torch.linspace(-half, half, steps=k, dtype=dtype)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return pdf / pdf.sum()


def blur_formula(x, kernel_size, sigma):
    """torchvision's gaussian_blur in the dtype of ``x`` ([N, C, H, W], CPU)"""
    (kx, ky), (sx, sy) = pair(kernel_size), pair(sigma)
    k2 = torch.mm(kernel1d(ky, sy, x.dtype)[:, None], kernel1d(kx, sx, x.dtype)[None, :])
    c = x.shape[1]
    xp = F.pad(x, (kx // 2, kx // 2, ky // 2, ky // 2), mode="reflect")
    return F.conv2d(xp, k2.expand(c, 1, ky, kx), groups=c)


def rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


FORWARD_CASES = [
    # shape, kernel, sigma, channels_last
    ((2, 3, 3, 4), 5, 1.3, False),               # p = H - 1: both reflections overlap
    ((1, 1, 32, 32), 5, 1.5, False),             # the reference's own use
    ((3, 2, 17, 70), (7, 3), (2.0, 0.6), False),  # tile seams, non-multiples, anisotropy
    ((2, 3, 9, 9), 5, 1.5, True),                # channels-last rows walked as they lie in memory
    ((3, 9, 9), 5, 1.5, False),                  # a single 3-D image
    ((1, 1, 16, 40), 31, 6.0, False),            # envelope edge: the largest kernel, p = 15 < H = 16
    ((1, 36, 16, 16), 31, 6.0, True),            # channels-last whose halo of 15 * 36 columns leaves LDS: the strided-plane route
    ((2, 2, 40, 33), (3, 9), (0.8, 2.5), True),  # channels-last, two tile rows
]


@pytest.mark.parametrize("shape,kernel,sigma,channels_last", FORWARD_CASES)
def test_forward_vs_truth(HF, shape, kernel, sigma, channels_last):
    x = rand(shape, 1)
    x4 = x if x.dim() == 4 else x[None]
    ref32, truth = blur_formula(x4, kernel, sigma), blur_formula(x4.double(), kernel, sigma)
    xd = x.cuda()
    if channels_last:
        xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert not xd.is_contiguous()
    y = HF.gaussian_blur(xd, kernel, sigma)
    assert y.shape == x.shape and y.dtype == torch.float32 and y.stride() == xd.stride(), "the output has the layout of the input"
    vs_truth(f"forward {shape} k {kernel}", y if y.dim() == 4 else y[None], ref32, truth)


def test_bit_properties(HF):
    x = rand((5, 3, 17, 23), 2).cuda()
    assert torch.equal(HF.gaussian_blur(x, 1, 1.0), x), "k = 1 is the identity, bit for bit"
    xl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert torch.equal(HF.gaussian_blur(xl, 1, 0.3), x)
    a, b = HF.gaussian_blur(x, (5, 7), (1.5, 0.9)), HF.gaussian_blur(x, (5, 7), (1.5, 0.9))
    assert torch.equal(a, b), "a repeated call gives equal bits"
    planes = x.reshape(15, 1, 17, 23)
    alone = HF.gaussian_blur(planes[3:4].clone(), (5, 7), (1.5, 0.9))
    assert torch.equal(a.reshape(15, 1, 17, 23)[3:4], alone), "a plane gives the same bits in a batch as alone"
    assert torch.equal(HF.gaussian_blur(xl, (5, 7), (1.5, 0.9)), a), "and in either layout"


@pytest.mark.parametrize("shape,kernel,sigma", [((2, 3, 3, 4), 5, 1.3), ((1, 2, 17, 70), (7, 3), (2.0, 0.6))])
def test_backward_vs_fp64_autograd(HF, shape, kernel, sigma):
    (kx, ky), (sx, sy) = pair(kernel), pair(sigma)
    x, g = torch.rand(shape, generator=torch.Generator().manual_seed(3)), torch.rand(shape, generator=torch.Generator().manual_seed(4))
    grads = {}
    for dtype in (torch.float32, torch.float64):
        leaf = x.to(dtype).clone().requires_grad_(True)
        (blur_formula(leaf, kernel, sigma) * g.to(dtype)).sum().backward()
        grads[dtype] = leaf.grad
    xd = x.cuda().requires_grad_(True)
    y = torch.ops.otvae.gaussian_blur(xd, kx, ky, sx, sy)
    (y * g.cuda()).sum().backward()
    vs_truth(f"backward {shape} k {kernel}", xd.grad, grads[torch.float32], grads[torch.float64])
    # the adjoint identity <blur(x), g> = <x, blur^T(g)>, the inner products in fp64 on the host from the device results.  x and g are
    # in [0, 1): both sides are sums of non-negative terms, so the relative bound of 1e-5 is not a bound on a cancelling difference
    # (fp32 rounding of each term is ~6e-8 relative).
    lhs = (y.detach().double().cpu() * g.double()).sum().item()
    rhs = (x.double() * xd.grad.double().cpu()).sum().item()
    print(f"[transforms] adjoint identity {shape}: {lhs:.12e} vs {rhs:.12e}")
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs)
    # channels-last gradients take the other addressing and must agree bit for bit
    xl = x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    gl = g.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    (torch.ops.otvae.gaussian_blur(xl, kx, ky, sx, sy) * gl).sum().backward()
    assert torch.equal(xl.grad, xd.grad)


def test_operator_checks(A):
    x = rand((2, 3, 9, 9), 5).cuda().requires_grad_(True)
    torch.library.opcheck(torch.ops.otvae.gaussian_blur.default, (x, 5, 3, 1.3, 0.7))
    xl = rand((2, 3, 9, 9), 6).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    torch.library.opcheck(torch.ops.otvae.gaussian_blur.default, (xl, 3, 3, 1.0, 1.0))


def test_refusals(HF):
    x = rand((1, 1, 8, 8), 7).cuda()
    for k in (4, (3, 2), 0):
        with pytest.raises(ValueError):
            HF.gaussian_blur(x, k, 1.0)
    for s in (0.0, -1.0, (1.0, 0.0)):
        with pytest.raises(ValueError):
            HF.gaussian_blur(x, 3, s)
    with pytest.raises(RuntimeError, match="Padding size should be less than"):     # F.pad(mode="reflect")'s refusal: k // 2 >= H
        HF.gaussian_blur(rand((1, 1, 2, 8), 8).cuda(), (3, 5), 1.0)
    with pytest.raises(NotImplementedError):     # beyond the envelope of 31 taps per axis
        HF.gaussian_blur(rand((1, 1, 40, 40), 9).cuda(), 33, 5.0)
    for dtype in (torch.float64, torch.float16):
        with pytest.raises(NotImplementedError):
            HF.gaussian_blur(x.to(dtype), 3, 1.0)
    with pytest.raises(RuntimeError):
        HF.gaussian_blur(x.cpu(), 3, 1.0)


def test_gaussian_blur_module(A, HF):
    x = rand((2, 3, 12, 12), 10).cuda()
    blur = A.GaussianBlur(5, sigma=(0.5, 2.0))
    for seed in (0, 123):
        torch.manual_seed(seed)
        want = torch.empty(1).uniform_(0.5, 2.0).item()
        torch.manual_seed(seed)
        y = blur(x)
        assert blur.last_sigma == want, "the draw torchvision makes after the same seed"
        assert torch.equal(y, HF.gaussian_blur(x, 5, want))
    assert torch.equal(A.GaussianBlur(5, sigma=(1.5, 1.5))(x), HF.gaussian_blur(x, 5, 1.5))
    assert torch.equal(A.GaussianBlur((5, 3), sigma=0.8)(x), HF.gaussian_blur(x, (5, 3), (0.8, 0.8)))
    assert torch.equal(A.GaussianBlur(5, sigma=1.5)(x[0]), HF.gaussian_blur(x, 5, 1.5)[0]), "a sample alone, as LatentTransport._collage feeds it"


# ------------------------------------------------------------------------------------------------ collage
def collage_formula(images, num_samples):
    """cat / clamp / make_grid(nrow=1, padding=2, pad_value=0) written out, on the CPU"""
    x = torch.cat([t.cpu() for t in images], -1).clamp(0, 1)
    x = x[:min(x.shape[0], num_samples)]
    n, c, h, w = x.shape
    if c == 1:
        x = torch.cat((x, x, x), 1)
    if n == 1:
        return x[0]
    grid = torch.zeros(x.shape[1], n * (h + 2) + 2, w + 4)
    for k in range(n):
        grid[:, k * (h + 2) + 2:k * (h + 2) + 2 + h, 2:2 + w] = x[k]
    return grid


def test_collage_single_channel(HF):
    maps = [(torch.rand(s, generator=torch.Generator().manual_seed(20 + i)) * 2 - 0.5).cuda()
            for i, s in enumerate([(5, 1, 4, 6), (5, 1, 4, 6), (5, 1, 4, 3)])]
    assert min(m.min().item() for m in maps) < 0 and max(m.max().item() for m in maps) > 1
    out = HF.collage(maps, 3)
    want = collage_formula(maps, 3)
    assert out.shape == (3, 20, 19) and out.dtype == torch.float32
    assert torch.equal(out.cpu(), want)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], out[2]), "one channel, three times"
    o = out.cpu()
    assert (o[:, :2] == 0).all() and (o[:, -2:] == 0).all() and (o[:, :, :2] == 0).all() and (o[:, :, -2:] == 0).all()
    assert (o[:, 6:8] == 0).all() and (o[:, 12:14] == 0).all(), "the padding between the samples"
    u8 = HF.collage(maps, 3, as_uint8=True)
    assert u8.shape == (20, 19, 3) and u8.dtype == torch.uint8
    assert torch.equal(u8.cpu(), want.mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8)), "save_image's quantisation"


def test_collage_colour_layouts_and_single_sample(A, HF):
    g = torch.Generator().manual_seed(30)
    a = (torch.rand((2, 3, 5, 7), generator=g) * 2 - 0.5).cuda()
    b = (torch.rand((2, 3, 5, 4), generator=g) * 2 - 0.5).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)   # channels-last
    out = HF.collage([a, b], 8)                  # n = B = 2
    assert out.shape == (3, 16, 15) and torch.equal(out.cpu(), collage_formula([a, b], 8))
    assert torch.equal(A.Collage.list_to_collage([a, b], 8), out)
    one = HF.collage([a, b], 1)                  # n = 1: the bare image, no border
    assert one.shape == (3, 5, 11) and torch.equal(one.cpu(), collage_formula([a, b], 1))
    grey = HF.collage([a[:1, :1], b[:1, :1]], 4)
    assert grey.shape == (3, 5, 11) and torch.equal(grey.cpu(), collage_formula([a[:1, :1], b[:1, :1]], 4))
    u8 = HF.collage([a, b], 1, as_uint8=True)
    assert torch.equal(u8.cpu(), collage_formula([a, b], 1).mul(255).add(0.5).clamp(0, 255).permute(1, 2, 0).to(torch.uint8))
    with pytest.raises(ValueError):
        HF.collage([a, b[:, :, :4]], 2)
    with pytest.raises(NotImplementedError):
        HF.collage([a[:, :, :, :1]] * 17, 2)
    with pytest.raises(RuntimeError):
        HF.collage([a.cpu()], 2)


# ------------------------------------------------------------------------------------------------ the callbacks
def tiny_vae(A):
    """the small model of tests/test_metrics_host.py"""
    return A.VAE(encoder=A.CNN(1, 16, 16, 1, capacity=2, down_sample=True), decoder=A.CNN(8, 1, 1, 16, capacity=2, up_sample=True),
                 prior=A.GaussianPrior(loss_coeff=0.1))


def test_progressive_transform_on_a_vae(A, HF):
    torch.manual_seed(0)
    model, other = tiny_vae(A).cuda(), tiny_vae(A).cuda()
    x, y = rand((4, 1, 16, 16), 40).cuda(), torch.zeros(4, dtype=torch.long).cuda()
    assert model.batch_preprocess((x, y))["samples"] is x, "no callback: the input object itself"
    cb = A.ProgressiveTransform(A.PgTransform(A.GaussianBlur, {"sigma": [(1, 1), (0.5, 0.5)]}, kernel_size=5), schedule=[0, 1])
    trainer = types.SimpleNamespace(current_epoch=0)
    for epoch, sigma in ((0, 1.0), (1, 0.5), (2, 0.5)):      # epoch 2 is not scheduled: the transform of epoch 1 stays
        trainer.current_epoch = epoch
        cb.on_train_epoch_start(trainer, model)
        pb = model.batch_preprocess((x, y))
        assert torch.equal(pb["samples"], HF.gaussian_blur(x, 5, sigma)), epoch
        assert pb["target"] is pb["samples"] and pb["kwargs"] == {}
        assert other.batch_preprocess((x, y))["samples"] is x, "a second instance is untouched"


def test_latent_transport_with_gaussian_blur(A, HF):
    torch.manual_seed(1)
    ae = A.AutoEncoder(1, 8, 16, 1, capacity=2, double_encoded_features=False, down_up_sample=True, residual="add")
    vae = A.VAE(autoencoder=ae, prior=None).cuda().eval()
    batches = [torch.rand((32, 1, 16, 16), generator=torch.Generator().manual_seed(50 + i)) for i in range(2)]
    k2 = torch.mm(kernel1d(5, 1.5, torch.float32)[:, None], kernel1d(5, 1.5, torch.float32)[None, :])[None, None].cuda()
    stand_in = lambda x: F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), k2)    # noqa: E731

    def run(transformations):
        w2_cfg = dict(diag=False, stochastic=False, pg_star=0., make_pd=True, verbose=False, dtype=torch.double)
        cb = A.LatentTransport(size=vae.latent_size, transport_operator=A.GaussianTransport, transport_dims=(1, 2, 3),
                               logging_prefix="gaussian", transport_cfg=w2_cfg, source_cfg=dict(dtype=torch.double),
                               target_cfg=dict(dtype=torch.double), transformations=transformations, unpaired=True,
                               common_operator=True, num_samples_to_log=3)
        cb.on_fit_start(None, vae)
        cb.on_validation_epoch_start(None, vae)
        with torch.no_grad():
            for i, xb in enumerate(batches):
                cb.on_validation_batch_end(None, vae, {"samples": xb.cuda()}, None, i)
            cb.on_validation_epoch_end(None, vae)
        src = cb.transport_operator.source_model
        return cb, (src._running_sum / src._n_obs.unsqueeze(-1)).flatten()

    cb, mean_hip = run(A.GaussianBlur(5, sigma=(1.5, 1.5)))
    _, mean_ref = run(stand_in)
    with torch.no_grad():   # the truth: the source batch blurred in fp64 on the host, then the same encoder
        z = vae.encode(blur_formula(batches[1].double(), 5, 1.5).float().cuda())
    vs_truth("LatentTransport source mean", mean_hip, mean_ref, z.double().flatten(1).mean(0))
    assert cb.dim == z[0].numel() and float(cb.transport_operator.source_model._n_obs.sum()) == 32

    trainer = types.SimpleNamespace(val_dataloaders=[[(batches[0].cuda(), torch.zeros(32, dtype=torch.long).cuda())]], logger=None,
                                    global_step=0)
    collage = cb._collage(trainer, vae)
    assert collage.shape == (3, 3 * (16 + 2) + 2, 6 * 16 + 4) and torch.isfinite(collage).all()
    assert float(collage.min()) >= 0 and float(collage.max()) <= 1
    logged = []
    trainer.logger = types.SimpleNamespace(log_image=lambda key, images, step: logged.append((key, images, step)))
    with torch.no_grad():
        cb.on_validation_epoch_end(trainer, vae)
    assert logged[0][0] == cb.logging_prefix and logged[0][1][0].shape == collage.shape
