"""GPU: the AttentionBlock on a one-pixel map.  With one key the softmax weight is 1: the attention returns v, dq = dk = 0 and
dv = gout, so the block is ``proj_out(Wv . BN(x))`` and the query / key columns of ``qkv.weight`` have an exactly zero gradient.
``functional.attention_one_token`` runs the value projection alone: a forward job over the column window [2C, 3C) of the [C][3C]
weight (``otvae_conv_job.ldw``), the data gradient over the contiguous v rows of the transposed copy, and a C -> C weight-gradient
job whose reduction writes the window of the whole gradient and zeros around it (``ldgw`` / ``gw_col0``).

Shapes (N, C, heads): (3, 8, 2) vector path, one ragged 64-row tile; (5, 6, 3) channel counts that are no multiples of 4, window start
12 floats, scalar path; (70, 256, 16) the flagship step's layer: two row tiles, the second ragged, 8 K-chunks, window at column 512
of 768.  All have N < 128: the C -> C and the C -> 3C weight-gradient plans both have one split-K part and sum the same rows in the
same order, so every comparison between the windowed and the full-width computation is bit for bit.  At larger batches the windowed
weight-gradient job takes the wide layer's split-K parts (``otvae_conv_window_ws``), which keeps that true (n1024_c256, n300_c8)."""
import copy
import ctypes as C

import pytest
import torch

import test_gpu_conv_abi as T
from conftest import rel_err
from detfill import normal

pytestmark = pytest.mark.gpu

SHAPES = [(3, 8, 2), (5, 6, 3), (70, 256, 16)]
TOL = 1e-4    # the bound of tests/test_gpu_conv_geometry.py::test_attention_block_on_a_rectangle for the block's y and dx
NSLOTS = 8


def shape_id(s):
    return "n%d_c%d_h%d" % s


def _case(n, c, seed):
    """x [N, C, 1, 1], the [C][3C] HWIO weight, an affine of x and the gradient of the block's inner C-wide tensor"""
    x = T.nhwc(normal((n, c, 1, 1), seed).cuda())
    w = (normal((1, 1, c, 3 * c), seed + 1) * c ** -0.5).cuda().contiguous()
    scale = (normal((c,), seed + 2) * 0.2 + 1.0).cuda()
    shift = (normal((c,), seed + 3) * 0.3).cuda()
    gout = T.nhwc(normal((n, c, 1, 1), seed + 4).cuda())
    return x, w, scale, shift, gout


def _geom(n, cs, cn):
    return T._L().ConvGeom(n, 1, 1, cs, 1, 1, 1, cn, 1, 1, 1, 0)


def _nan(n, ch):
    return T.nhwc(torch.full((n, ch, 1, 1), float("nan"), device="cuda"))


def _run(jobs, n=1):
    """one otvae_conv_multi call; returns (launches, packed mask)"""
    L, lib = T._L(), T.load()
    L.check(lib.otvae_conv_multi(n, jobs, L.stream()), "otvae_conv_multi")
    nl, mask, ut = C.c_int(-1), C.c_uint(0), C.c_int(0)
    L.check(lib.otvae_conv_multi_launches(C.byref(nl)), "launches")
    L.check(lib.otvae_conv_multi_last(C.byref(mask), C.byref(ut)), "last")
    torch.cuda.synchronize()
    return nl.value, mask.value


# ---------------------------------------------------------------------------------------------------------------- 1. forward window
def _fwd(x, w, cn, col0, affine, scale, shift):
    """y of the forward job over the columns [col0, col0 + cn) of w (the whole weight: col0 = 0, cn = 3C), y pre-filled with NaN;
    ``affine``: None, "arrays" (scale / shift) or "fold" (the BatchNorm of x folded into the launch from statistic slots)"""
    L, lib = T._L(), T.load()
    n, c = x.shape[:2]
    ld = w.shape[-1]
    jobs = (L.ConvJob * 1)()
    jb = jobs[0]
    y = _nan(n, cn)
    jb.kind, jb.geom = L.JOB_FWD, _geom(n, c, cn)
    jb.x, jb.y = L.ptr(x), L.ptr(y)
    jb.w = w.data_ptr() + 4 * col0
    if cn != ld:
        jb.ldw = ld
    keep, pub = [], []
    if affine == "arrays":
        jb.scale, jb.shift = L.ptr(scale), L.ptr(shift)
    elif affine == "fold":
        xs = torch.zeros(lib.otvae_bn_slots_words(c, NSLOTS), device="cuda", dtype=torch.int64)
        L.check(lib.otvae_bn_stats_slots(L.ptr(x), n, c, L.ptr(xs), c, NSLOTS, L.stream()), "stats_slots")
        gamma, beta = scale.clone(), shift.clone()
        pub = [torch.full((c,), float("nan"), device="cuda") for _ in range(4)]   # mean, invstd, scale, shift
        pub += [torch.linspace(-1, 1, c, device="cuda"), torch.linspace(0.5, 2, c, device="cuda"), torch.tensor(7, device="cuda")]
        f = jb.fold
        f.slots, f.ld, f.nslots, f.count, f.eps, f.momentum = L.ptr(xs), c, NSLOTS, n, 1e-5, 0.1
        f.gamma, f.beta = L.ptr(gamma), L.ptr(beta)
        f.mean_out, f.invstd_out, f.scale_out, f.shift_out = (L.ptr(t) for t in pub[:4])
        f.running_mean, f.running_var, f.num_batches_tracked = (L.ptr(t) for t in pub[4:])
        keep = [xs, gamma, beta]
    launches, mask = _run(jobs)      # (synchronizes: `keep` outlives the launch)
    assert launches == 1 and mask == 0 and len(keep) in (0, 3)
    return y, pub


@pytest.mark.parametrize("affine", [None, "arrays", "fold"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_windowed_forward_equals_the_columns_of_the_full_job(shape, affine):
    n, c, _ = shape
    x, w, scale, shift, _ = _case(n, c, 10 * c)
    full, pub_full = _fwd(x, w, 3 * c, 0, affine, scale, shift)
    win, pub_win = _fwd(x, w, c, 2 * c, affine, scale, shift)
    assert not torch.isnan(full).any() and not torch.isnan(win).any()     # every element of the NaN-filled outputs written
    assert torch.equal(win, full[:, 2 * c:])
    assert float(win.abs().max()) > 0
    for a, b in zip(pub_win, pub_full):       # the fold published the same statistics and advanced the running buffers alike
        assert torch.equal(a, b) and not torch.isnan(a.float()).any()
    # the window is the weight's, not the output's: the q and k windows give the other two thirds
    for j in (0, 1):
        other, _ = _fwd(x, w, c, j * c, affine, scale, shift)
        assert torch.equal(other, full[:, j * c: (j + 1) * c])


def test_window_jobs_are_checked():
    L, lib = T._L(), T.load()
    x, w, scale, shift, gout = _case(3, 8, 5)
    jobs = (L.ConvJob * 1)()
    jb = jobs[0]
    y = _nan(3, 8)
    jb.kind, jb.geom, jb.x, jb.w, jb.y = L.JOB_FWD, _geom(3, 8, 8), L.ptr(x), L.ptr(w), L.ptr(y)
    jb.ldw = 4                                               # a pitch below the window's width
    assert lib.otvae_conv_multi(1, jobs, L.stream()) != 0
    jb.ldw, jb.ldgw = 24, 24                                 # gradient window on a forward job
    assert lib.otvae_conv_multi(1, jobs, L.stream()) != 0
    part, gw = torch.empty((1, 8, 8), device="cuda"), torch.zeros((8, 24), device="cuda")
    jb.kind, jb.ldw, jb.ldgw, jb.gw_col0 = L.JOB_BWD_WEIGHT, 0, 24, 20      # window past the end of the row
    jb.gy, jb.wpartial, jb.gw = L.ptr(gout), L.ptr(part), L.ptr(gw)
    assert lib.otvae_conv_multi(1, jobs, L.stream()) != 0
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and not gw.any()             # nothing was launched


# ---------------------------------------------------------------------------------------------------------------- 2. gradient window
def _wgrad(x, gout, scale, shift, window, deferred):
    """gw of the C -> C weight-gradient job: stand-alone [C][C] (window None), or into the window (col0, ld) of a NaN-filled [C][ld]"""
    L, lib = T._L(), T.load()
    n, c = x.shape[:2]
    g = _geom(n, c, c)
    p = C.c_int(0)
    L.check(lib.otvae_conv_bwd_weight_ws(C.byref(g), 0, C.byref(p)), "ws")
    assert p.value == 1
    part = torch.full((p.value, c, c), float("nan"), device="cuda")
    col0, ld = window if window is not None else (0, c)
    gw = torch.full((c, ld), float("nan"), device="cuda")
    jobs = (L.ConvJob * 1)()
    jb = jobs[0]
    jb.kind, jb.geom = L.JOB_BWD_WEIGHT, g
    jb.x, jb.scale, jb.shift, jb.gy = L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(gout)
    jb.wpartial, jb.gw = L.ptr(part), L.ptr(gw)
    jb.defer_reduce = L.DEFER_SPARSE if deferred else 0
    if window is not None:
        jb.ldgw, jb.gw_col0 = ld, col0
    launches, _ = _run(jobs)
    assert launches == (1 if deferred else 2)
    if deferred:
        assert torch.isnan(gw).all()
        dead = C.c_uint32(0)
        L.check(lib.otvae_conv_dead_taps(C.byref(g), C.byref(dead)), "dead_taps")
        ia = lambda v: (C.c_int * 1)(v)  # noqa: E731
        L.check(lib.otvae_wgrad_reduce_batched_win(1, L.ptr_array([part]), ia(p.value), ia(c), ia(c), ia(c), L.ptr_array([gw]),
                                                   L.ptr_array([None]), ia(c), (C.c_uint32 * 1)(dead.value),
                                                   ia(ld if window is not None else 0), ia(col0), L.stream()), "reduce")
        torch.cuda.synchronize()
    return gw


@pytest.mark.parametrize("deferred", [True, False], ids=["batched", "immediate"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_windowed_weight_gradient_reduction(shape, deferred):
    n, c, _ = shape
    x, _, scale, shift, gout = _case(n, c, 20 * c)
    want = _wgrad(x, gout, scale, shift, None, False)                  # stand-alone C -> C job, immediate reduction
    assert not torch.isnan(want).any() and float(want.abs().max()) > 0
    ref64 = ((x.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).flatten(1).t()
             @ gout.double().flatten(1))
    assert T.rel(want, ref64) < T.TOL
    got = _wgrad(x, gout, scale, shift, (2 * c, 3 * c), deferred)
    assert torch.equal(got[:, 2 * c:], want)
    assert not got[:, : 2 * c].any() and not torch.isnan(got).any()     # exact zeros over the NaN the buffer held
    assert torch.equal(got[:, : 2 * c], torch.zeros_like(got[:, : 2 * c]))
    mid = _wgrad(x, gout, scale, shift, (c, 3 * c), deferred)           # zeros on both sides of a window in the middle
    assert torch.equal(mid[:, c: 2 * c], want) and not mid[:, :c].any() and not mid[:, 2 * c:].any()


def _wgrad_parts(x, gy, scale, shift, window, deferred):
    """gw [C][ld] of a weight-gradient job at a batch with several split-K parts: the whole C -> ld layer (window None, gy ld wide), or
    the C -> C job of its window (col0, ld) with the parts of ``otvae_conv_window_ws``; returns (gw, parts)"""
    L, lib = T._L(), T.load()
    n, c = x.shape[:2]
    cn = gy.shape[1]
    g = _geom(n, c, cn)
    p = C.c_int(0)
    if window is None:
        col0, ld = 0, cn
        L.check(lib.otvae_conv_bwd_weight_ws(C.byref(g), 0, C.byref(p)), "ws")
    else:
        col0, ld = window
        L.check(lib.otvae_conv_window_ws(C.byref(g), ld, None, None, None, None, C.byref(p)), "window_ws")
    part = torch.full((p.value, c, cn), float("nan"), device="cuda")
    gw = torch.full((c, ld), float("nan"), device="cuda")
    jobs = (L.ConvJob * 1)()
    jb = jobs[0]
    jb.kind, jb.geom = L.JOB_BWD_WEIGHT, g
    jb.x, jb.scale, jb.shift, jb.gy = L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(gy)
    jb.wpartial, jb.gw = L.ptr(part), L.ptr(gw)
    jb.defer_reduce = L.DEFER_SPARSE if deferred else 0
    if window is not None:
        jb.ldgw, jb.gw_col0 = ld, col0
    _run(jobs)
    if deferred:
        ia = lambda v: (C.c_int * 1)(v)  # noqa: E731
        L.check(lib.otvae_wgrad_reduce_batched_win(1, L.ptr_array([part]), ia(p.value), ia(c), ia(c), ia(cn), L.ptr_array([gw]),
                                                   L.ptr_array([None]), ia(c), (C.c_uint32 * 1)(0),
                                                   ia(ld if window is not None else 0), ia(col0), L.stream()), "reduce")
        torch.cuda.synchronize()
    assert not torch.isnan(part).any()
    return gw, p.value


@pytest.mark.parametrize("deferred", [True, False], ids=["batched", "immediate"])
@pytest.mark.parametrize("n,c", [(1024, 256), (300, 8)], ids=["n1024_c256", "n300_c8"])
def test_windowed_weight_gradient_equals_the_columns_of_the_wide_job(n, c, deferred):
    """Several split-K parts (the flagship step's batch; a small ragged one): the C -> C and the C -> 3C plans of ``wgrad_plan`` split the
    rows differently, so the windowed job takes the wide layer's parts and its window is bit for bit the wide job's columns."""
    x = T.nhwc(normal((n, c, 1, 1), 31).cuda())
    scale, shift = (normal((c,), 32) * 0.2 + 1.0).cuda(), (normal((c,), 33) * 0.3).cuda()
    gqkv = T.nhwc(normal((n, 3 * c, 1, 1), 34).cuda())
    gqkv[:, : 2 * c] = 0                                               # dq = dk = 0, as the one-token attention backward leaves them
    gout = T.nhwc(gqkv[:, 2 * c:].clone())
    wide, p_wide = _wgrad_parts(x, gqkv, scale, shift, None, deferred)
    win, p_win = _wgrad_parts(x, gout, scale, shift, (2 * c, 3 * c), deferred)
    assert p_wide == p_win and p_wide > 1
    assert torch.equal(win, wide) and not win[:, : 2 * c].any() and float(win[:, 2 * c:].abs().max()) > 0
    ref64 = (x.double() * scale.double()[None, :, None, None] + shift.double()[None, :, None, None]).flatten(1).t() @ gout.double().flatten(1)
    assert T.rel(win[:, 2 * c:], ref64) < T.TOL


# ---------------------------------------------------------------------------------------------------------------- 3. the block
def _fill(mod, seed):
    with torch.no_grad():
        for i, p in enumerate(mod.parameters()):
            p.copy_(normal(tuple(p.shape), seed + i).mul_(0.4 if p.dim() > 1 else 0.2))
        for name, p in mod.named_parameters():
            if name.endswith("_normalization.weight"):
                p.add_(1.0)
    return mod


class flags:
    """module switches of ``functional`` for the duration of a block"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        from ot_vae_lightning_amd import functional as HF
        self.old = {k: getattr(HF, k) for k in self.kv}
        for k, v in self.kv.items():
            setattr(HF, k, v)

    def __exit__(self, *a):
        from ot_vae_lightning_amd import functional as HF
        for k, v in self.old.items():
            setattr(HF, k, v)


def _block_run(blk, x, gy, residual, one_token, train):
    """forward + backward of a copy of ``blk``; returns (dict of results, the jobs issued)"""
    from ot_vae_lightning_amd import functional as HF
    blk = copy.deepcopy(blk)
    blk.train(train)
    xg = x.clone().requires_grad_(True)
    trace = []
    with flags(ATTN_ONE_TOKEN=one_token, JOB_TRACE=trace):
        y = blk(xg, residual=xg if residual else None)
        y.backward(gy)
    torch.cuda.synchronize()
    out = {"y": y.detach(), "gx": xg.grad, "gwp": blk.proj_out.weight.grad, "gwq": blk.qkv.weight.grad}
    for k, p in blk.named_parameters():
        if "_normalization" in k:
            out["g:" + k] = p.grad
    for k, b in blk.named_buffers():
        out["b:" + k] = b.detach().clone()
    return out, trace


def _block_ref64(blk, x, gy, residual, train):
    """fp64 host evaluation of [x +] Wp . (Wv . BN(x)) and of its input gradient"""
    c = x.shape[1]
    x64 = x.detach().double().cpu().flatten(1).requires_grad_(True)             # [N, C]
    wq = blk.qkv.weight.detach().double().cpu().flatten(1)                      # [3C, C]
    wp = blk.proj_out.weight.detach().double().cpu().flatten(1)                 # [C, C]
    a = x64
    bn = blk.qkv._normalization
    if isinstance(bn, torch.nn.BatchNorm2d):
        if train:
            mean, var = x64.mean(0), x64.var(0, unbiased=False)
        else:
            mean, var = bn.running_mean.double().cpu(), bn.running_var.double().cpu()
        a = (x64 - mean) / torch.sqrt(var + bn.eps) * bn.weight.detach().double().cpu() + bn.bias.detach().double().cpu()
    y = (a @ wq[2 * c:].t()) @ wp.t()
    if residual:
        y = y + x64
    y.backward(gy.double().cpu().flatten(1))
    return y.detach(), x64.grad


@pytest.mark.parametrize("variant", ["batch-train", "batch-eval", "none-train", "batch-train-residual", "none-eval-residual"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_block_one_token_on_equals_off(shape, variant):
    from ot_vae_lightning_amd.networks.cnn import AttentionBlock
    n, c, heads = shape
    norm = "batch" if variant.startswith("batch") else None
    train, residual = "-train" in variant, variant.endswith("residual")
    blk = _fill(AttentionBlock(c, heads, normalization=norm).cuda(), 3 * c)
    if norm:
        with torch.no_grad():     # running statistics an eval-mode block really uses
            blk.qkv._normalization.running_mean.copy_(normal((c,), 7).cuda() * 0.1)
            blk.qkv._normalization.running_var.copy_(normal((c,), 8).cuda().abs() + 0.5)
    x = T.nhwc(normal((n, c, 1, 1), 11).cuda())
    gy = T.nhwc(normal((n, c, 1, 1), 12).cuda())
    on, trace_on = _block_run(blk, x, gy, residual, True, train)
    off, trace_off = _block_run(blk, x, gy, residual, False, train)
    # the route each side took: the first job is the value projection (C wide) resp. the qkv convolution (3C wide)
    assert trace_on[0]["jobs"][0]["geom"][7] == c and trace_off[0]["jobs"][0]["geom"][7] == 3 * c
    assert set(on) == set(off)
    for k in on:
        if k == "gwq":
            continue
        assert on[k] is not None and torch.equal(on[k], off[k]), (k, rel_err(on[k], off[k]))
    for side in (on, off):
        gq = side["gwq"].flatten(1)       # [3C, C]
        assert gq.shape == (3 * c, c) and not gq[: 2 * c].any() and not torch.isnan(gq).any()
        assert float(gq[2 * c:].abs().max()) > 0
    assert torch.equal(on["gwq"], off["gwq"])
    y64, gx64 = _block_ref64(blk, x, gy, residual, train)
    ey, ex = rel_err(on["y"].flatten(1), y64), rel_err(on["gx"].flatten(1), gx64)
    print(f"{shape} {variant}: y {ey:.3g} gx {ex:.3g} against fp64")
    assert ey < TOL and ex < TOL, (ey, ex)


# ---------------------------------------------------------------------------------------------------------------- 4. fallbacks
class _UserAttention(torch.nn.Module):
    """a user's attention module with the interface the block reads (``n_heads``)"""

    def __init__(self, n_heads):
        super().__init__()
        self.n_heads = n_heads


def _first_width(blk, x, embed=None):
    """width of the first convolution job the block issues (ATTN_STAGE off: the three-launch path is what a declined block runs)"""
    from ot_vae_lightning_amd import functional as HF
    trace = []
    taken = []
    old = HF.attention_one_token

    def spy(*a, **kw):
        y = old(*a, **kw)
        taken.append(y is not None)
        return y

    with flags(ATTN_STAGE=False, JOB_TRACE=trace, attention_one_token=spy):
        y = blk(x) if embed is None else blk(x, embed)
    torch.cuda.synchronize()
    assert tuple(y.shape) == tuple(x.shape) and bool(torch.isfinite(y).all())
    return trace[0]["jobs"][0]["geom"][7] if trace else None, taken


def test_fallbacks_run_the_three_launches(monkeypatch):
    from ot_vae_lightning_amd import functional as HF
    from ot_vae_lightning_amd.networks.cnn import AttentionBlock
    c, heads, n = 8, 2, 6
    x1 = T.nhwc(normal((n, c, 1, 1), 21).cuda())
    x4 = T.nhwc(normal((n, c, 2, 2), 22).cuda())
    attn_calls = []   # the attention launches (otvae_attn_fwd) of the three-launch path
    monkeypatch.setattr(HF, "_attention_op", lambda q, h, s, _o=HF._attention_op: (attn_calls.append(1), _o(q, h, s))[1])
    # plain block, one token: the value projection alone, no attention launch
    plain = _fill(AttentionBlock(c, heads, normalization="batch").cuda().train(), 1)
    w, taken = _first_width(plain, x1)
    assert w == c and taken == [True] and attn_calls == []
    # ... switched off: the parent's three launches
    with flags(ATTN_ONE_TOKEN=False):
        w, taken = _first_width(plain, x1)
    assert w == 3 * c and taken == [False] and len(attn_calls) == 1
    # T = 4
    del attn_calls[:]
    w, taken = _first_width(plain, x4)
    assert w == 3 * c and taken == [False] and len(attn_calls) == 1
    # FiLM, equalized learning rate, grouped projections: the general ConvLayer path issues no fused job for the qkv convolution, or a
    # 3C-wide one; never a C-wide first job, and the attention launch runs
    embed = normal((n, 4), 23).cuda()
    for what, blk, kw in (("film", AttentionBlock(c, heads, additional_embed=4, normalization="batch"), dict(embed=embed)),
                          ("equalized_lr", AttentionBlock(c, heads, normalization="batch", equalized_lr=1.0), {}),
                          ("groups", AttentionBlock(c, heads, normalization="batch", groups=2), {})):
        del attn_calls[:]
        blk = _fill(blk.cuda().train(), 2)
        w, taken = _first_width(blk, x1, **kw)
        assert taken == [False] and len(attn_calls) == 1, what
        assert w != c, (what, w)
    # a user-supplied attention module: attention_one_token is not even asked
    del attn_calls[:]
    user = _fill(AttentionBlock(c, heads, normalization="batch").cuda().train(), 1)
    user.attention = _UserAttention(heads)
    w, taken = _first_width(user, x1)
    assert w == 3 * c and taken == [] and len(attn_calls) == 1


# ---------------------------------------------------------------------------------------------------------------- 5. the trainer
def _train(one_token, graph, steps=2):
    import ot_vae_lightning_amd as A
    from ot_vae_lightning_amd.networks.cnn import AttentionBlock
    torch.manual_seed(5)
    enc = A.CNN(1, 16, 4, 1, capacity=2, down_sample=True, residual="add")
    dec = A.CNN(8, 1, 1, 4, capacity=2, up_sample=True, residual="add")
    last = [m for m in enc.modules() if isinstance(m, AttentionBlock)][-1]
    assert last.qkv.in_channels == 16
    model = A.VAE(encoder=enc, decoder=dec, prior=A.GaussianPrior(loss_coeff=0.1)).cuda().train()
    x, eps = normal((8, 1, 4, 4), 5).cuda(), normal((8, 8, 1, 1), 6).cuda()
    with flags(ATTN_ONE_TOKEN=one_token):
        tr = A.HipTrainer(model, batch_shape=(8, 1, 4, 4), use_graph=graph)
        losses = [tr.step(x, eps).clone() for _ in range(steps)]
        torch.cuda.synchronize()
        out = dict(loss=torch.stack(losses), latents=tr.latents.clone(), params=tr.pflat.clone(),
                   buffers={k: b.detach().clone() for k, b in model.named_buffers()})
        slot = last.qkv.weight._otvae_grad_view().detach().clone().flatten(1)     # [3C, C]: the flat gradient slot after the last step
        tr.close()
    return out, slot


def test_trainer_steps_with_the_one_token_block():
    on_graph, slot = _train(True, True)
    off_graph, slot_off = _train(False, True)
    on_eager, _ = _train(True, False)
    c = slot.shape[1]
    assert bool(torch.isfinite(on_graph["loss"]).all())
    # the q and k columns of the flat gradient slot (never cleared between steps) read exactly 0 after the step, on both sides
    for s in (slot, slot_off):
        assert s.shape == (3 * c, c) and not s[: 2 * c].any() and float(s[2 * c:].abs().max()) > 0
    for other, what in ((off_graph, "flag off"), (on_eager, "eager")):
        for k in ("loss", "latents", "params"):
            assert torch.equal(on_graph[k], other[k]), (what, k, rel_err(on_graph[k], other[k]))
        assert set(on_graph["buffers"]) == set(other["buffers"])
        for k, b in on_graph["buffers"].items():
            assert torch.equal(b, other["buffers"][k]), (what, k)
