"""GPU: the unfused normalisation / activation kernels a ``ConvLayer`` or ViT is built from outside the BatchNorm + ReLU route, each
on its own against a float64 truth computed on the host: GroupNorm / InstanceNorm + activation (csrc/groupnorm.hip), the BatchNorm
affine + activation and its backward sums (csrc/activation.hip), FiLM's backward (csrc/film_dropout2d.hip), the grouped / dilated
weight expansion (csrc/weight_expand.hip), the embedding and batch-broadcast backward sums, the scalar multiplier, and the plain and
residual instantiations of LayerNorm (csrc/layernorm.hip).  The shapes come from the kernels' own tiling (256-thread strides, 64-column
blocks, channel passes, values per lane); every one is named for the loop or branch it enters.

Bounds: ``vs_truth`` is the rule of tests/test_gpu_autodiffusion.py -- the HIP error against the truth is at most
max(1e-4, 1.5 x the error of the same torch operator in fp32), relative to max|truth|.  A result that is ONE rounding of an fp64
accumulation gets ``one_rounding``: |got - truth| <= 2^-23 |truth| + 1e-30 element-wise.  Copies and single multiplications are
``torch.equal``.  No constant here comes from a measured HIP number.

ReLU, LeakyReLU and SELU have a kink at 0: every random-input case asserts that the fp64 pre-activation stays 1e-5 away from it, so
that a sign that differs between fp32 and fp64 cannot pose as a kernel error; the seeds below were chosen so that this holds.  What
happens AT 0 is the deterministic ``test_bn_act_zero_convention``.  The host halves of all cases (truth, fp32 reference, the kink
condition, the fp64 check of the weight-expansion construction) are functions of their own: they run without a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL32, FACTOR = 1e-4, 1.5
EPS = 1e-5             # functional.BN_EPS (asserted below)
KINK = 1e-5
KINKED = (1, 2, 3)     # ReLU, LeakyReLU, SELU
TORCH_ACT = {0: lambda v: v, 1: F.relu, 2: lambda v: F.leaky_relu(v, 0.2), 3: F.selu, 4: F.gelu, 5: F.silu}


@pytest.fixture(scope="module")
def A():
    assert torch.cuda.is_available()
    import ot_vae_lightning_amd as A_
    assert A_.functional.BN_EPS == EPS
    return A_


def vs_truth(name, got, ref32, truth, floor=0.0):
    t = truth.detach().double().cpu()
    scale = max(t.abs().max().item(), floor, 1e-30)
    e_hip = (got.detach().double().cpu() - t).abs().max().item() / scale
    e_ref = (ref32.detach().double().cpu() - t).abs().max().item() / scale
    tol = max(TOL32, FACTOR * e_ref)
    print(f"[norm_act] {name}: hip vs fp64 truth {e_hip:.3e}  reference fp32 vs truth {e_ref:.3e}  bound {tol:.3e}")
    assert math.isfinite(e_hip) and e_hip <= tol, (name, e_hip, e_ref, tol)


def one_rounding(name, got, truth):
    """``got`` (fp32) is a single rounding of the fp64 number ``truth``: within one fp32 ulp (2^-23 relative), element-wise"""
    g, t = got.detach().double().cpu(), truth.detach().double().cpu()
    assert g.shape == t.shape, (name, g.shape, t.shape)
    err, bound = (g - t).abs(), 2.0 ** -23 * t.abs() + 1e-30
    worst = (err / bound).max().item()
    print(f"[norm_act] {name}: worst |hip - fp64 truth| / (2^-23 |truth| + 1e-30) = {worst:.3e}  bound 1")
    assert math.isfinite(worst) and bool((err <= bound).all()), (name, worst)


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def away_from_kink(name, u64, kind):
    """the condition on the inputs of a kinked activation (module docstring)"""
    if kind in KINKED:
        gap = u64.abs().min().item()
        assert gap >= KINK, f"{name}: fp64 pre-activation comes within {gap:.2e} of the kink: pick another seed"


# ---- otvae_group_norm_act_fwd / _bwd ----------------------------------------------------------------------------------------------------
# (N, C, G, HW, affine): InstanceNorm with 5-element groups (a fraction of one wave) / one element per group (variance exactly 0) /
# HW = 1 with cg = 4 / cnt = 444: one full 256-stride and a ragged second, cg = 12 does not divide 256 / G = 1, 34 full strides and a
# tail / cg = 260 > 256: the parameter-partial loop takes a second trip, N = 1: the column sum over one row
GN_SHAPES = [(2, 6, 6, 5, False), (2, 4, 4, 1, False), (3, 12, 3, 1, True), (2, 24, 2, 37, True), (2, 8, 1, 1089, True),
             (1, 520, 2, 3, True)]
GN_CASES = [(i, k) for i in range(len(GN_SHAPES)) for k in ((0, 1, 2, 3, 4, 5) if i in (3, 5) else (0, 2, 5))]
GN_SEED = {}   # (shape index, kind) -> seed, where the default 100 + 10 * index + kind comes too close to a kink


def gn_inputs(i, kind, offset=0.0):
    n, c, g, hw, affine = GN_SHAPES[i]
    seed = GN_SEED.get((i, kind), 100 + 10 * i + kind)
    x = offset + normal((n, c, hw, 1), seed)
    gamma = 1.0 + 0.5 * normal((c,), seed + 1000) if affine else None
    beta = 0.3 * normal((c,), seed + 2000) if affine else None
    return x, gamma, beta, normal((n, c, hw, 1), seed + 3000)


def gn_host(x, gamma, beta, g, groups, kind, dtype):
    """the definition with torch operators on the host: (pre-activation, out, dx, dgamma, dbeta)"""
    x = x.to(dtype).clone().requires_grad_(True)
    gamma, beta = (None, None) if gamma is None else (p.to(dtype).clone().requires_grad_(True) for p in (gamma, beta))
    u = F.group_norm(x, groups, gamma, beta, eps=EPS)
    out = TORCH_ACT[kind](u)
    out.backward(g.to(dtype))
    return u.detach(), out.detach(), x.grad, None if gamma is None else gamma.grad, None if beta is None else beta.grad


def gn_host_case(i, kind, offset=0.0):
    x, gamma, beta, g = gn_inputs(i, kind, offset)
    groups = GN_SHAPES[i][2]
    truth, ref32 = gn_host(x, gamma, beta, g, groups, kind, torch.float64), gn_host(x, gamma, beta, g, groups, kind, torch.float32)
    if i == 1:   # one element per group: the pre-activation IS the kink, exactly and in every precision -- nothing for rounding to flip;
        # dx = rstd (w - mean(w) - xhat mean(w xhat)) with one element is w - w: 0, which torch's own formula reaches to rounding only
        assert truth[0].abs().max().item() == 0.0 and truth[2].abs().max().item() <= 1e-9
    else:
        away_from_kink(f"group_norm {GN_SHAPES[i]} kind {kind}", truth[0], kind)
    return (x, gamma, beta, g), truth, ref32


def _gn_device(HF, x, gamma, beta, g, groups, kind):
    xd = HF.as_nhwc(x.cuda()).requires_grad_(True)
    gd = HF.as_nhwc(g.cuda())
    params = [] if gamma is None else [gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)]
    out = HF._GroupNormActFn.apply(xd, *(params or (None, None)), groups, kind, (None, None))
    grads = torch.autograd.grad(out, [xd] + params, gd)
    return xd, params, out.detach(), grads


def _gn_check(A, i, kind, offset=0.0):
    HF = A.functional
    (x, gamma, beta, g), truth, ref32 = gn_host_case(i, kind, offset)
    groups = GN_SHAPES[i][2]
    tag = f"group_norm {GN_SHAPES[i][:4]}{' x=30+randn' if offset else ''} kind {kind}"
    xd, params, out, grads = _gn_device(HF, x, gamma, beta, g, groups, kind)
    assert out.shape == x.shape and HF.is_nhwc(out) and HF.is_nhwc(grads[0])
    if i == 1:   # variance exactly 0, rstd = 1 / sqrt(eps): out = act(0), dx = 0, not a rounding error away from them
        assert torch.equal(out.cpu(), TORCH_ACT[kind](torch.zeros_like(x))) and torch.equal(out.cpu(), truth[1].float())
        assert torch.equal(grads[0].cpu(), torch.zeros_like(x))
    else:
        vs_truth(tag + " out", out, ref32[1], truth[1])
        vs_truth(tag + " dx", grads[0], ref32[2], truth[2])
    if gamma is None:   # InstanceNorm has no parameters: autograd refuses a backward that returns anything but None for a forward
        assert len(grads) == 1   # input that was no tensor, so dgamma = dbeta = None is what let the call above return
    else:
        vs_truth(tag + " dgamma", grads[1], ref32[3], truth[3])
        vs_truth(tag + " dbeta", grads[2], ref32[4], truth[4])
    # bits across kernels: the fused activation is the one of csrc/act.h that activation.hip applies to the un-activated output
    if kind != 0:
        with torch.no_grad():
            gam0, bet0 = [p.detach() for p in params] or (None, None)
            plain = HF._GroupNormActFn.apply(xd.detach(), gam0, bet0, groups, 0, (None, None))
            chained = HF._BnActFn.apply(plain, None, None, None, kind, (None, None))
        assert torch.equal(out, chained), f"{tag}: fused activation and activation.hip differ in bits"
    # the same call again: the same bits (fixed-order fp64 sums)
    _, _, out2, grads2 = _gn_device(HF, x, gamma, beta, g, groups, kind)
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize("i,kind", GN_CASES, ids=[f"{GN_SHAPES[i][:4]}-{'gn' if GN_SHAPES[i][4] else 'in'}-kind{k}" for i, k in GN_CASES])
def test_group_norm_act_against_fp64_truth(A, i, kind):
    _gn_check(A, i, kind)


def test_group_norm_act_with_a_mean_30_deviations_from_zero(A):
    """x = 30 + randn at the (2, 24, 2, 37) shape: the two-pass fp64 statistics and the cast of the mean to fp32; the bound is still
    the fp32 reference's own error"""
    _gn_check(A, 3, 4, offset=30.0)


def test_group_norm_act_refusals(A):
    """the C ABI refuses C % G != 0, G == 0, an unknown activation and gamma without beta (every buffer is large enough for the call it
    refuses)"""
    from ot_vae_lightning_amd import _lib as L
    lib = L.load()
    n, hw, c = 2, 3, 6
    x = torch.zeros(n, hw, c, device="cuda")
    out, ga, dx = torch.empty_like(x), torch.ones_like(x), torch.empty_like(x)
    mean, rstd = torch.zeros(n, c, device="cuda"), torch.ones(n, c, device="cuda")
    gamma, beta = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
    pg, pb = torch.empty(n, c, device="cuda"), torch.empty(n, c, device="cuda")

    def fwd(groups, kind, gam, bet):
        L.check(lib.otvae_group_norm_act_fwd(L.ptr(x), L.ptr(gam), L.ptr(bet), n, hw, c, groups, EPS, kind, L.ptr(out), L.ptr(mean),
                                             L.ptr(rstd), L.stream()), "otvae_group_norm_act_fwd")

    def bwd(groups, kind, gam, bet):
        L.check(lib.otvae_group_norm_act_bwd(L.ptr(ga), L.ptr(x), L.ptr(gam), L.ptr(bet), L.ptr(mean), L.ptr(rstd), n, hw, c, groups, kind,
                                             L.ptr(dx), L.ptr(pg), L.ptr(pb), L.stream()), "otvae_group_norm_act_bwd")

    for call in (fwd, bwd):
        call(3, 5, gamma, beta)   # the valid call goes through
        for groups, kind, gam, bet in ((4, 1, gamma, beta), (0, 1, gamma, beta), (3, 6, gamma, beta), (3, -1, gamma, beta),
                                      (3, 1, gamma, None), (3, 1, None, beta)):
            with pytest.raises(ValueError):
                call(groups, kind, gam, bet)
    torch.cuda.synchronize()


# ---- otvae_bn_act_fwd / _bwd behind otvae_bn_stats / _finalize and in front of otvae_bn_bwd_finalize / _apply ---------------------------
# (N, C, H, W): CW = 5 channel lanes x RW = 51 row lanes, one dead thread, one block / M = 1058: three blocks of 512 rows, the last
# with 34, RW = 21 / C = 1: 256 row lanes, two blocks / C = 300 > 256: two channel passes, the second with 44 live lanes, RW = 1
BN_SHAPES = [(2, 5, 3, 3), (2, 12, 23, 23), (600, 1, 1, 1), (3, 300, 2, 2)]
BN_CASES = [(i, k, True) for i in range(len(BN_SHAPES)) for k in ((0, 1, 2, 3, 4, 5) if i in (1, 3) else (2, 4))]
BN_CASES += [(i, k, False) for i in (0, 3) for k in ((0, 1, 2, 3, 4, 5) if i == 3 else (2, 4))]
BN_SEED = {(1, 2, True): 1313}   #(shape index, kind, training) -> seed, where the default 300 + 10 * index + kind comes too close to a kink
NBT0 = 7


def bn_inputs(i, kind, training):
    n, c, h, w = BN_SHAPES[i]
    seed = BN_SEED.get((i, kind, training), 300 + 10 * i + kind)
    x = 0.5 + 1.5 * normal((n, c, h, w), seed)
    gamma, beta = 1.0 + 0.5 * normal((c,), seed + 1000), 0.3 * normal((c,), seed + 2000)
    rm, rv = 0.4 * normal((c,), seed + 4000), 0.5 + normal((c,), seed + 5000).square()   # running buffers that are not (0, 1)
    return x, gamma, beta, rm, rv, normal((n, c, h, w), seed + 3000)


def bn_host(x, gamma, beta, rm, rv, g, kind, training, dtype):
    """(pre-activation, out, dx, dgamma, dbeta, running_mean, running_var) of F.batch_norm + activation on the host"""
    x, gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (x, gamma, beta))
    rm, rv = rm.to(dtype).clone(), rv.to(dtype).clone()
    u = F.batch_norm(x, rm, rv, gamma, beta, training=training, momentum=0.1, eps=EPS)
    out = TORCH_ACT[kind](u)
    out.backward(g.to(dtype))
    return u.detach(), out.detach(), x.grad, gamma.grad, beta.grad, rm, rv


def bn_host_case(i, kind, training):
    inputs = bn_inputs(i, kind, training)
    truth, ref32 = bn_host(*inputs, kind, training, torch.float64), bn_host(*inputs, kind, training, torch.float32)
    away_from_kink(f"bn_act {BN_SHAPES[i]} kind {kind} training {training}", truth[0], kind)
    return inputs, truth, ref32


@pytest.mark.parametrize("i,kind,training", BN_CASES,
                         ids=[f"{BN_SHAPES[i]}-kind{k}-{'train' if t else 'eval'}" for i, k, t in BN_CASES])
def test_bn_act_against_fp64_truth(A, i, kind, training):
    """driven as functional._conv_layer_general does, outside an engine step: per-block partials + finalize launches"""
    HF = A.functional
    (x, gamma, beta, rm, rv, g), truth, ref32 = bn_host_case(i, kind, training)
    tag = f"bn_act {BN_SHAPES[i]} kind {kind} {'train' if training else 'eval'}"
    xd = HF.as_nhwc(x.cuda()).requires_grad_(True)
    gd = HF.as_nhwc(g.cuda())
    gam, bet = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    rmd, rvd, nbt = rm.cuda(), rv.cuda(), torch.full((), NBT0, dtype=torch.int64, device="cuda")
    bn = HF.BNBranch(gam.detach(), bet.detach(), rmd, rvd, nbt)

    def run():
        if training:
            mean, invstd, sc, sh = HF.bn_batch_stats(xd.detach(), [bn])
        else:
            mean, invstd, s0, h0 = HF.bn_eval_affine(bn)
            sc, sh = [s0], [h0]
        out = HF._BnActFn.apply(xd, gam, bet, (mean, invstd, sc[0], sh[0], training), kind, (None, None))
        return out.detach(), torch.autograd.grad(out, (xd, gam, bet), gd)

    out, grads = run()
    assert out.shape == x.shape and HF.is_nhwc(out) and HF.is_nhwc(grads[0])
    vs_truth(tag + " out", out, ref32[1], truth[1])
    for name, got, r, t in zip(("dx", "dgamma", "dbeta"), grads, ref32[2:5], truth[2:5]):
        vs_truth(f"{tag} {name}", got, r, t)
    if training:
        vs_truth(tag + " running_mean", rmd, ref32[5], truth[5])
        vs_truth(tag + " running_var", rvd, ref32[6], truth[6])
        assert nbt.item() == NBT0 + 1
    else:   # a fixed affine: nothing is tracked
        assert torch.equal(rmd.cpu(), rm) and torch.equal(rvd.cpu(), rv) and nbt.item() == NBT0
        assert torch.equal(truth[5], rm.double()) and torch.equal(truth[6], rv.double())
    out2, grads2 = run()
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def act_host(x, g, kind, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    out = TORCH_ACT[kind](x)
    out.backward(g.to(dtype))
    return out.detach(), x.grad


def _act_device(HF, x, g, kind):
    xd = HF.as_nhwc(x.cuda()).requires_grad_(True)
    out = HF._BnActFn.apply(xd, None, None, None, kind, (None, None))
    (gv,) = torch.autograd.grad(out, xd, HF.as_nhwc(g.cuda()))
    return out.detach(), gv


ZERO_X = [0.0, -0.0, 1e-30, -1e-30, 1.0, -1.0, 3.0, -3.0]
ZERO_G = [1.5, -0.75, 2.0, 0.5, -1.25, 0.75, 1.0, -2.0]


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_bn_act_zero_convention(A, kind):
    """no normalisation (stats None); at u = 0 the gradient is 0 for ReLU, the slope 0.2 for LeakyReLU, the exponential branch for SELU:
    torch's conventions, which csrc/act.h states as its own"""
    HF = A.functional
    x, g = torch.tensor(ZERO_X).reshape(2, 4, 1, 1), torch.tensor(ZERO_G).reshape(2, 4, 1, 1)
    ref32, truth = act_host(x, g, kind, torch.float32), act_host(x, g, kind, torch.float64)
    at_zero = {1: 0.0, 2: 0.2, 3: 1.0507009873554805 * 1.6732632423543772}.get(kind)
    if at_zero is not None:   # the host reference itself follows the convention this case is about
        assert torch.allclose(truth[1].reshape(-1)[:2], at_zero * g.double().reshape(-1)[:2], rtol=1e-12, atol=0.0)
    out, gv = _act_device(HF, x, g, kind)
    for name, got, r, t in (("out", out, ref32[0], truth[0]), ("gv", gv, ref32[1], truth[1])):
        vs_truth(f"act at zero kind {kind} {name}", got, r, t)                   # against the fp64 truth, bounded by torch's fp32 error
        vs_truth(f"act at zero kind {kind} {name} (torch fp32 as the truth)", got, r, r)   # and against torch's fp32 result itself
    zeros = (slice(0, 1), slice(0, 2))   # the elements holding 0.0 and -0.0
    assert torch.equal(out.cpu()[zeros], ref32[0][zeros]) and torch.equal(gv.cpu()[zeros], ref32[1][zeros])


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 4, 5])
def test_bn_act_tails(A, kind):
    """SiLU's expf(-u) overflows from u = -89 on, GELU's erff saturates, SELU's expm1f reaches -1: finite results, within the bound"""
    HF = A.functional
    x = torch.tensor([20.0, -20.0, 89.0, -89.0, 104.0, -104.0, 1e4, -1e4]).reshape(2, 4, 1, 1)
    g = torch.tensor(ZERO_G).reshape(2, 4, 1, 1)
    ref32, truth = act_host(x, g, kind, torch.float32), act_host(x, g, kind, torch.float64)
    out, gv = _act_device(HF, x, g, kind)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gv).all())
    vs_truth(f"act tails kind {kind} out", out, ref32[0], truth[0])
    vs_truth(f"act tails kind {kind} gv", gv, ref32[1], truth[1])


# ---- otvae_film_bwd ---------------------------------------------------------------------------------------------------------------------
# (N, HW, C): the FILM_SHAPES of tests/test_gpu_autodiffusion.py and C = 300: a second trip of the kernel's `c += 256`
FILM_SHAPES = [(3, 5, 6), (2, 1, 8), (2, 1089, 12), (1, 70, 130), (1, 7, 300)]


def film_inputs(shape):
    n, hw, c = shape
    return normal((n, c, hw, 1), 501), 1.0 + 0.5 * normal((n, c), 502), 0.3 * normal((n, c), 503), normal((n, c, hw, 1), 504)


def film_host(shape):
    """fp64 sums of the fp32 operands (the products of two fp32 numbers are exact in fp64): what gscale / gbias round once"""
    x, s, b, g = film_inputs(shape)
    return (g.double() * x.double()).sum((2, 3)), g.double().sum((2, 3))


@pytest.mark.parametrize("shape", FILM_SHAPES, ids=str)
def test_film_backward(A, shape):
    HF = A.functional
    x, s, b, g = film_inputs(shape)
    gs64, gb64 = film_host(shape)
    xd = HF.as_nhwc(x.cuda()).requires_grad_(True)
    sd, bd = s.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    gd = HF.as_nhwc(g.cuda())
    gx, gs, gb = torch.autograd.grad(HF._FilmFn.apply(xd, sd, bd), (xd, sd, bd), gd)
    assert HF.is_nhwc(gx) and torch.equal(gx, gd * sd.detach()[:, :, None, None])   # one multiplication
    one_rounding(f"film_bwd {shape} gscale", gs, gs64)
    one_rounding(f"film_bwd {shape} gbias", gb, gb64)
    gx2, gs2, gb2 = torch.autograd.grad(HF._FilmFn.apply(xd, sd, bd), (xd, sd, bd), gd)
    assert torch.equal(gx, gx2) and torch.equal(gs, gs2) and torch.equal(gb, gb2)


# ---- otvae_weight_expand_fwd / _bwd -----------------------------------------------------------------------------------------------------
# (Cout, Cin, groups, KH, KW, dil): a plain grouped weight / depthwise 1x1 / Cig = 1, Cog = 2 / dilation only / a non-square footprint,
# dense 7 x 4 / dense 31 x 31, one under the 32-tap limit / 746 496 dense elements: more than the 2048 x 256 grid, the grid-stride loop
# repeats
EXPAND_CASES = [(6, 4, 2, 3, 3, 1), (8, 8, 8, 1, 1, 1), (12, 6, 6, 3, 3, 1), (4, 4, 1, 3, 3, 2), (6, 9, 3, 3, 2, 3),
                (2, 2, 1, 11, 11, 3), (96, 96, 2, 5, 5, 2)]


def expand_host(case):
    """(w, the dense weight built with plain slicing, a dense gradient and its strided gather back); the construction itself is
    checked in fp64: a dense convolution with it is the grouped / dilated convolution with w"""
    cout, cin, groups, kh, kw, dil = case
    cog, cig = cout // groups, cin // groups
    khd, kwd = (kh - 1) * dil + 1, (kw - 1) * dil + 1
    w = normal((cout, cig, kh, kw), 600 + cout + kh)
    gdense = normal((cout, cin, khd, kwd), 601 + cout + kh)
    dense, gw = torch.zeros(cout, cin, khd, kwd), torch.empty_like(w)
    for g in range(groups):
        dense[g * cog:(g + 1) * cog, g * cig:(g + 1) * cig, ::dil, ::dil] = w[g * cog:(g + 1) * cog]
        gw[g * cog:(g + 1) * cog] = gdense[g * cog:(g + 1) * cog, g * cig:(g + 1) * cig, ::dil, ::dil]
    x = normal((2, cin, khd + 1, kwd + 2), 602).double()
    a, b = F.conv2d(x, dense.double()), F.conv2d(x, w.double(), groups=groups, dilation=dil)
    assert a.shape == b.shape and (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), case
    return w, dense, gdense, gw


@pytest.mark.parametrize("case", EXPAND_CASES, ids=str)
def test_weight_expand_is_exact(A, case):
    HF = A.functional
    cout, cin, groups, kh, kw, dil = case
    w, dense, gdense, gw = expand_host(case)
    wd = w.cuda().requires_grad_(True)
    out = HF._WeightExpandFn.apply(wd, cin, groups, dil)
    assert out.shape == dense.shape and HF.is_hwio(out) and torch.equal(out.detach().cpu(), dense)
    (got,) = torch.autograd.grad(out, wd, gdense.cuda())   # an OIHW gradient: the Function brings it to HWIO itself
    assert got.shape == gw.shape and got.is_contiguous() and torch.equal(got.cpu(), gw)
    (got2,) = torch.autograd.grad(HF._WeightExpandFn.apply(wd, cin, groups, dil), wd, HF.hwio_weight(gdense.cuda()))
    assert torch.equal(got2, got)


def test_weight_expand_refusals(A):
    from ot_vae_lightning_amd import _lib as L
    HF, lib = A.functional, L.load()
    with pytest.raises(ValueError):   # Cin % groups != 0: from the Function
        HF._WeightExpandFn.apply(torch.zeros(4, 2, 3, 3, device="cuda"), 5, 2, 1)
    src, dst = torch.zeros(4096, device="cuda"), torch.zeros(4096, device="cuda")   # more than any of the refused calls would touch
    for name in ("otvae_weight_expand_fwd", "otvae_weight_expand_bwd"):
        fn = getattr(lib, name)
        L.check(fn(L.ptr(src), 6, 4, 2, 3, 3, 1, L.ptr(dst), L.stream()), name)         # the valid call goes through
        L.check(fn(L.ptr(src), 1, 1, 1, 11, 1, 3, L.ptr(dst), L.stream()), name)        # 31 taps: the last footprint that fits
        for cout, cin, groups, kh, kw, dil in ((5, 4, 2, 3, 3, 1), (4, 5, 2, 3, 3, 1), (4, 4, 0, 3, 3, 1), (1, 1, 1, 12, 1, 3),
                                               (1, 1, 1, 1, 12, 3), (1, 1, 1, 3, 3, 0)):
            with pytest.raises(ValueError):
                L.check(fn(L.ptr(src), cout, cin, groups, kh, kw, dil, L.ptr(dst), L.stream()), name)
    torch.cuda.synchronize()


# ---- otvae_embedding_bwd ----------------------------------------------------------------------------------------------------------------
# (K, d, B, indices): a single class / d exactly 64 and B exactly 4 / d = 64 + 6 columns, B % 4 = 1, the odd classes unused / B = 1 /
# every row into one class / the third again with a [3, 11] index tensor
def _idx(k, b, seed):
    return torch.randint(0, k, (b,), generator=torch.Generator().manual_seed(seed))


EMBED_CASES = {
    "one-class": (1, 5, torch.zeros(7, dtype=torch.int64)),
    "d64-b4": (3, 64, torch.tensor([2, 0, 1, 2])),
    "half-unused": (10, 70, 2 * _idx(5, 33, 701)),
    "b1": (5, 130, torch.tensor([3])),
    "all-equal": (4, 8, torch.full((257,), 2, dtype=torch.int64)),
    "index-3x11": (10, 70, (2 * _idx(5, 33, 702)).reshape(3, 11)),
}


def embed_host(name):
    k, d, idx = EMBED_CASES[name]
    g = normal(tuple(idx.shape) + (d,), 703 + d)
    flat = idx.reshape(-1)
    truth = torch.zeros(k, d, dtype=torch.float64).index_add_(0, flat, g.double().reshape(-1, d))
    ref32 = torch.zeros(k, d).index_add_(0, flat, g.reshape(-1, d))
    unused = torch.tensor([c not in set(flat.tolist()) for c in range(k)])
    return g, truth, ref32, unused


@pytest.mark.parametrize("name", list(EMBED_CASES))
def test_embedding_backward(A, name):
    HF = A.functional
    k, d, idx = EMBED_CASES[name]
    g, truth, ref32, unused = embed_host(name)
    weight = normal((k, d), 704).cuda().requires_grad_(True)
    out = HF.embedding(weight, idx.cuda())
    assert torch.equal(out.detach().cpu(), weight.detach().cpu()[idx])
    (gw,) = torch.autograd.grad(out, weight, g.cuda())
    vs_truth(f"embedding_bwd {name} (K, d, B) = {(k, d, idx.numel())}", gw, ref32, truth)
    # a class no sample selects gets exactly 0: the gradient slot is uninitialised memory, zeroing it is the kernel's job
    assert int(unused.sum()) == {"half-unused": 5, "index-3x11": 5, "b1": 4, "all-equal": 3}.get(name, int(unused.sum()))
    assert torch.equal(gw.cpu()[unused], torch.zeros(int(unused.sum()), d))
    (gw2,) = torch.autograd.grad(HF.embedding(weight, idx.cuda()), weight, g.cuda())
    assert torch.equal(gw, gw2)


# ---- otvae_colsum_f32 behind expand_batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 5), (7, 64), (33, 70), (1024, 3), (5, 1000)])
def test_expand_batch_backward(A, rows, cols):
    HF = A.functional
    t = normal((cols,), 801).cuda().requires_grad_(True)
    g = normal((rows, cols), 802 + rows)
    out = HF.expand_batch(t, rows)
    assert out.shape == (rows, cols) and torch.equal(out.detach(), t.detach().expand(rows, cols))
    (gt,) = torch.autograd.grad(out, t, g.cuda())
    assert gt.shape == t.shape
    one_rounding(f"colsum_f32 (R, C) = {(rows, cols)}", gt, g.double().sum(0))   # fp64 sums down the rows, rounded once
    (gt2,) = torch.autograd.grad(HF.expand_batch(t, rows), t, g.cuda())
    assert torch.equal(gt, gt2)


# ---- otvae_scale_f32 --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["contiguous", "channels-last", "slice", "beyond-the-grid"])
def test_scale_is_one_multiplication(A, case):
    HF = A.functional
    alpha = 0.37
    if case == "contiguous":
        t = normal((5, 7), 901).cuda()
    elif case == "channels-last":
        t = HF.as_nhwc(normal((2, 6, 3, 5), 902).cuda())
    elif case == "slice":                                  # not dense: the Function makes it contiguous first
        t = normal((4, 10), 903).cuda()[:, ::2]
        assert not t.is_contiguous()
    else:                                                  # 527 100 elements: more than 2048 blocks x 256 threads
        t = normal((3, 700, 251), 904).cuda()
        assert t.numel() > 2048 * 256
    g = torch.empty_like(t).copy_(normal(tuple(t.shape), 905).cuda())   # a gradient with t's own strides
    td = t.detach().requires_grad_(True)
    out = HF._ScaleFn.apply(td, alpha)
    assert out.shape == t.shape and torch.equal(out.detach(), alpha * t)
    if case != "slice":
        assert out.stride() == t.stride()                  # the output keeps the input's memory order
    (gt,) = torch.autograd.grad(out, td, g)
    assert gt.shape == t.shape and torch.equal(gt, alpha * g)


# ---- otvae_layernorm_fwd / _bwd without dropout -----------------------------------------------------------------------------------------
# (M, D): variance 0 / D < 64 / D exactly 64 / NV = 2 with one live column in the second slot / NV = 32 with its last 1023 columns dead /
# NV = 32 full, 32 KB of dynamic LDS in the backward pass, M % 16 = 3
LN_SHAPES = [(1, 1), (17, 3), (35, 64), (17, 65), (5, 1025), (19, 2048)]


def ln_inputs(m, d, with_res):
    x, res = normal((m, d), 950 + d), normal((m, d), 951 + d) if with_res else None
    return x, res, 1.0 + 0.1 * normal((d,), 952), 0.1 * normal((d,), 953), normal((m, d), 954 + d)


def ln_host(x, res, gamma, beta, g, dtype):
    """(y, d(x + res), dgamma, dbeta) of F.layer_norm on the host"""
    s = (x.to(dtype) if res is None else x.to(dtype) + res.to(dtype)).clone().requires_grad_(True)   # the sum is taken in `dtype`
    gamma, beta = (t.to(dtype).clone().requires_grad_(True) for t in (gamma, beta))
    y = F.layer_norm(s, (x.shape[-1],), gamma, beta, 1e-5)
    y.backward(g.to(dtype))
    return y.detach(), s.grad, gamma.grad, beta.grad


@pytest.mark.parametrize("with_res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("m,d", LN_SHAPES)
def test_layernorm_without_dropout(A, m, d, with_res):
    HF = A.functional
    x, res, gamma, beta, g = ln_inputs(m, d, with_res)
    truth, ref32 = ln_host(x, res, gamma, beta, g, torch.float64), ln_host(x, res, gamma, beta, g, torch.float32)
    leaves = [t.cuda().requires_grad_(True) for t in ((x, gamma, beta) if res is None else (x, gamma, beta, res))]
    gd = g.cuda()

    def run():
        y = HF.layer_norm_tokens(leaves[0], leaves[1], leaves[2], 1e-5, leaves[3] if with_res else None)
        return y.detach(), torch.autograd.grad(y, leaves, gd)

    y, grads = run()
    tag = f"layernorm (M, D) = {(m, d)} {'residual' if with_res else 'plain'}"
    assert y.shape == x.shape and all(a.shape == b.shape for a, b in zip(grads, leaves))
    if with_res:
        assert torch.equal(grads[3], grads[0])             # d res is d x: one tensor of the kernel
    if d == 1:   # variance exactly 0: y = beta and dx = 0 (and xhat = 0, so dgamma = 0), not a rounding error away from them
        assert torch.equal(y.cpu(), beta.expand(m, 1)) and torch.equal(grads[0].cpu(), torch.zeros(m, 1))
        assert torch.equal(grads[1].cpu(), torch.zeros(1)) and truth[1].abs().max().item() <= 1e-9 and truth[2].abs().max().item() <= 1e-9
    else:
        vs_truth(tag + " dx", grads[0], ref32[1], truth[1])
        vs_truth(tag + " dgamma", grads[1], ref32[2], truth[2])
    vs_truth(tag + " y", y, ref32[0], truth[0])
    vs_truth(tag + " dbeta", grads[2], ref32[3], truth[3])
    y2, grads2 = run()
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_layernorm_refuses_rows_longer_than_2048(A):
    HF = A.functional
    d = 2049
    x = torch.zeros(2, d, device="cuda")
    with pytest.raises(NotImplementedError):   # refused, not truncated to the 2048 columns a wave holds
        HF.layer_norm_tokens(x, torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"), 1e-5)
    with pytest.raises(NotImplementedError):
        HF.layer_norm_tokens(x, torch.ones(d, device="cuda"), torch.zeros(d, device="cuda"), 1e-5, torch.zeros_like(x))
    torch.cuda.synchronize()
