"""GPU: the convolution kernels on geometries whose two axes differ -- rectangular maps, KH != KW, position counts that are no
multiple of 4, stride-2 parity classes with unequal (or no) taps, pad = 0 and pad > (k-1)/2 -- where an H/W or KH/KW transposition,
invisible on the square cases of the other conv tests, changes the result.

  * direct C ABI: every case under the default switches, the implicit GEMM alone and the tile kernels wherever they run, against the
    float64 restatement of tests/test_gpu_conv_abi.py at that file's tolerance (fp32 accumulation over K = KH*KW*Cs <= 1152 products
    of O(1) terms; the largest K here is 576), y / gv bit for bit between the variants, every output element written, BatchNorm sums;
  * which kernel family each case reaches, read off ``otvae_conv_gemm_chunks``;
  * the generic (any stride, no fusion) convolution against float64 ``F.conv2d`` autograd;
  * rectangular inputs through ConvLayer / AttentionBlock / ConvBlock against the CPU oracle, with the bounds of
    tests/test_gpu_attn_stage.py.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import otvae_oracle as O
import test_gpu_conv_abi as T
import test_gpu_conv_live_taps as LT
from conftest import rel_err
from detfill import normal

pytestmark = pytest.mark.gpu

# (n, cs, cn, hs, ws, kh, kw, stride, pad, up)
TILE_RANGE = [
    (5, 8, 12, 7, 11, 3, 3, 1, 1, 1),     # 77 positions, odd on both axes, Cn % 16 != 0; tile wgrad pads the positions to 80
    (6, 8, 16, 16, 24, 4, 4, 2, 1, 1),    # stride 2 -> 8x12: data-gradient parity classes on a rectangle
    (9, 16, 8, 4, 6, 3, 3, 1, 1, 2),      # up 2 -> 8x12: children decode with Ws / 2 != Hs / 2
    (3, 8, 8, 8, 10, 3, 5, 1, 1, 1),      # KH != KW -> 8x8: tap index kh * KW + kw, different offsets per axis
    (3, 8, 8, 10, 8, 5, 3, 1, 1, 1),      # ... and the other way round
    (4, 8, 8, 9, 13, 3, 3, 1, 0, 1),      # pad 0 -> 7x11; data gradient over 117 positions
    (3, 8, 8, 6, 10, 3, 3, 1, 2, 1),      # pad 2 -> 8x12 (larger than the input): the tile data gradient declines, the GEMM serves its
                                          # 60 positions (3 tiles, each with all 9 taps)
    (4, 8, 8, 16, 20, 3, 3, 2, 1, 1),     # 3x3 s2: parity classes with 1 / 2 / 2 / 4 taps
    (4, 8, 8, 16, 20, 5, 5, 2, 2, 1),     # 5x5 s2 p2, ConvLayer(kernel_size=5, down_sample=2): 25 taps are more than the tile forward
                                          # holds (16), so the GEMM serves the forward; the data gradient's classes have 9 / 6 / 6 / 4
    (4, 8, 8, 16, 20, 1, 1, 2, 0, 1),     # 1x1 s2: three parity classes without a tap, which must still write zeros
    (4, 8, 8, 18, 22, 3, 3, 2, 0, 1),     # 3x3 s2 p0 -> 8x10: the last input row and column are never read
]
DEEP = [
    (70, 64, 64, 2, 3, 3, 3, 1, 1, 1),    # ragged tiles, position classes differ per axis
    (37, 32, 32, 1, 4, 3, 3, 1, 1, 1),    # taps dead on the y axis only
    (37, 32, 32, 4, 1, 3, 3, 1, 1, 1),    # ... on the x axis only
    (21, 32, 64, 4, 6, 4, 4, 2, 1, 1),    # stride 2 -> 2x3
    (23, 64, 32, 1, 3, 3, 3, 1, 1, 2),    # up 2 -> 2x6, children grouping
    (19, 16, 32, 4, 6, 3, 5, 1, 1, 1),    # KH != KW with CK = 16 (a chunk spans taps)
    (6, 6, 12, 4, 6, 3, 3, 1, 1, 1),      # scalar path, Cs % 4 != 0
    (3, 6, 12, 9, 13, 3, 3, 1, 1, 1),     # scalar GEMM forward / data gradient at 117 positions; tile wgrad without float4, 117 -> 120
]
DIRECT = [
    (4, 1, 8, 10, 14, 4, 4, 2, 1, 1),     # 1-channel input, stride 2 -> 5x7
    (4, 8, 1, 5, 7, 3, 3, 1, 1, 2),       # 1-channel output, up 2
    (2, 3, 8, 6, 10, 3, 5, 1, 1, 1),      # KH != KW: the runtime-size instantiation (the compile-time ones need KH == KW)
    (3, 3, 16, 10, 14, 4, 4, 2, 1, 1),    # RGB special case 3 -> 16
    (3, 16, 3, 5, 7, 3, 3, 1, 1, 2),      # RGB special case 16 -> 3
]
CASES = TILE_RANGE + DEEP + DIRECT


def case_id(c):
    return "n%d_%dto%d_%dx%d_k%dx%ds%dp%du%d" % c


VARIANTS = [dict(OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None, OTVAE_NO_WTILE=None, OTVAE_WTILE_ALL=None),
            dict(OTVAE_NO_TILE="1", OTVAE_TILE_ALL=None, OTVAE_NO_WTILE="1", OTVAE_WTILE_ALL=None),  # implicit GEMM only
            dict(OTVAE_NO_TILE=None, OTVAE_TILE_ALL="1", OTVAE_NO_WTILE=None, OTVAE_WTILE_ALL="1")]  # tile kernels wherever they can run


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_rectangular_conv_entry_points_vs_float64(case):
    n, cs, cn, hs, ws, kh, kw, s, p, up = case
    c = T.make_case2(case, seed=sum(case))
    y64, gv64, gw64, gb64 = T.ref64(c)
    dv = T.Dev(c)
    outs = []
    for vi, v in enumerate(VARIANTS):
        with T.env(**v):
            y, ysum = LT.fwd(dv)                       # y and gv start as NaN
            gv, gsum, mean, invstd = LT.dgrad(dv)
            gw, gb = T.run_wgrad(dv)
        assert not torch.isnan(y).any() and not torch.isnan(gv).any()
        errs = (T.rel(T.raw(y), T.raw(y64)), T.rel(T.raw(gv), T.raw(gv64)), T.rel(gw, gw64.permute(2, 3, 1, 0)), T.rel(gb, gb64))
        print(f"{case} variant {vi}: rel err y {errs[0]:.3g} gv {errs[1]:.3g} gw {errs[2]:.3g} gb {errs[3]:.3g}")
        assert max(errs) < T.TOL, errs
        # BatchNorm statistics of the output / BatchNorm-backward sums: fp64 sums of the fp32 tensors the kernel wrote
        yd = T.raw(y).double().reshape(-1, cn)
        assert T.rel(ysum[0], yd.sum(0)) < 1e-10 and T.rel(ysum[1], (yd * yd).sum(0)) < 1e-10
        gd = T.raw(gv).double().reshape(-1, cs)
        xhat = ((T.raw(dv.x).reshape(-1, cs) - mean) * invstd).double()
        assert T.rel(gsum[0], gd.sum(0)) < 1e-10
        assert float((gsum[1] - (gd * xhat).sum(0)).abs().max()) < 1e-9 * float((gd.abs() * xhat.abs()).sum(0).max())
        # ---- what the geometry makes exactly zero
        g = T.raw(gv)                                  # [N][Hs][Ws][Cs]
        if (kh, kw, s, p) == (1, 1, 2, 0):             # only even (iy, ix) are ever read
            assert not g[:, 1::2, :, :].any() and not g[:, :, 1::2, :].any()
            assert g[:, 0::2, 0::2, :].any()
        if (hs, ws, kh, kw, s, p) == (18, 22, 3, 3, 2, 0):
            assert not g[:, 17, :, :].any() and not g[:, :, 21, :].any()
            assert g[:, :17, :21, :].any()
        if (kh, kw, s, p, up) == (3, 3, 1, 1, 1) and 1 in (hs, ws):   # a one-pixel axis: its outer taps never touch the image
            for a in range(kh):
                for b in range(kw):
                    dead = (hs == 1 and a != 1) or (ws == 1 and b != 1)
                    assert bool(gw[a, b].any()) == (not dead), (a, b)
        outs.append((y, gv))
    # different kernel families, same fp32 arithmetic in the same order: identical bits
    for y, gv in outs[1:]:
        assert torch.equal(y, outs[0][0])
        assert torch.equal(gv, outs[0][1])


# what otvae_conv_gemm_chunks says of each case under the default switches, (forward, data gradient):
#   "tile" / "direct": another family takes the layer; "drop": implicit GEMM whose tiles drop taps (per_tile < launch_rule);
#   "all": implicit GEMM where no tile can drop a tap
ROUTES = {
    TILE_RANGE[0]: ("tile", "tile"), TILE_RANGE[1]: ("tile", "tile"), TILE_RANGE[2]: ("tile", "tile"), TILE_RANGE[3]: ("tile", "tile"),
    TILE_RANGE[4]: ("tile", "tile"), TILE_RANGE[5]: ("tile", "tile"), TILE_RANGE[6]: ("tile", "all"), TILE_RANGE[7]: ("tile", "tile"),
    TILE_RANGE[8]: ("all", "tile"), TILE_RANGE[9]: ("tile", "tile"), TILE_RANGE[10]: ("tile", "tile"),
    DEEP[0]: ("drop", "drop"), DEEP[1]: ("drop", "drop"), DEEP[2]: ("drop", "drop"), DEEP[3]: ("drop", "drop"),
    DEEP[4]: ("drop", "all"), DEEP[5]: ("drop", "drop"), DEEP[6]: ("all", "all"), DEEP[7]: ("all", "all"),
    DIRECT[0]: ("direct", "direct"), DIRECT[1]: ("direct", "direct"), DIRECT[2]: ("direct", "direct"), DIRECT[3]: ("direct", "direct"),
    DIRECT[4]: ("direct", "direct"),
}


def route(case, mode):
    L, lib = T._L(), T.load()
    n, cs, cn, hs, ws, kh, kw, s, p, up = case
    ho, wo = (hs * up + 2 * p - kh) // s + 1, (ws * up + 2 * p - kw) // s + 1
    g = L.ConvGeom(n, hs, ws, cs, up, ho, wo, cn, kh, kw, s, p)
    a, b = C.c_int64(-1), C.c_int64(-1)
    rc = lib.otvae_conv_gemm_chunks(C.byref(g), mode, C.byref(a), C.byref(b))
    if rc == 0:
        assert 0 < b.value <= a.value
        return "drop" if b.value < a.value else "all"
    assert rc == -2, (case, mode, rc, L.last_error())
    err = L.last_error()
    assert ("the image-tile" in err) != ("the direct" in err), err
    return "tile" if "the image-tile" in err else "direct"


def test_cases_reach_the_families_they_are_named_for():
    with T.env(OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None):
        got = {case: (route(case, 0), route(case, 1)) for case in CASES}
    assert got == ROUTES, {k: (got[k], ROUTES[k]) for k in CASES if got[k] != ROUTES[k]}


# ---- the generic convolution: (n, cs, cn, hs, ws, kh, kw, stride, pad)
GENERIC = [(3, 4, 6, 9, 14, 8, 8, 4, 3),      # -> 2x4
           (2, 3, 5, 11, 7, 5, 9, 3, 2)]      # -> 4x1


@pytest.mark.parametrize("case", GENERIC, ids=lambda c: "n%d_%dto%d_%dx%d_k%dx%ds%dp%d" % c)
def test_generic_conv_vs_float64(case):
    L, lib = T._L(), T.load()
    n, cs, cn, hs, ws, kh, kw, s, p = case
    g = torch.Generator().manual_seed(sum(case))
    x = torch.randn(n, cs, hs, ws, generator=g)
    w = torch.randn(cn, cs, kh, kw, generator=g) * (1.0 / (kh * kw * cs) ** 0.5)
    b = torch.randn(cn, generator=g)
    ho, wo = (hs + 2 * p - kh) // s + 1, (ws + 2 * p - kw) // s + 1
    gy = torch.randn(n, cn, ho, wo, generator=g)
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = F.conv2d(x64, w64, b64, stride=s, padding=p)
    assert y64.shape == (n, cn, ho, wo)
    (y64 * gy.double()).sum().backward()
    geom = L.ConvGeom(n, hs, ws, cs, 1, ho, wo, cn, kh, kw, s, p)
    xd, gyd = T.nhwc(x.cuda()), T.nhwc(gy.cuda())
    wd = w.cuda().permute(2, 3, 1, 0).contiguous()     # [KH][KW][Cs][Cn]
    bd = b.cuda()
    y = T.nhwc(torch.full((n, cn, ho, wo), float("nan"), device="cuda"))
    gx = T.nhwc(torch.full((n, cs, hs, ws), float("nan"), device="cuda"))
    gw, gb = torch.full_like(wd, float("nan")), torch.full_like(bd, float("nan"))
    L.check(lib.otvae_conv_generic_fwd(C.byref(geom), L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(y), L.stream()), "generic fwd")
    L.check(lib.otvae_conv_generic_bwd_data(C.byref(geom), L.ptr(gyd), L.ptr(wd), L.ptr(gx), L.stream()), "generic dgrad")
    nws = lib.otvae_conv_generic_bwd_weight_ws(C.byref(geom), 1)
    assert nws > 0
    ws_ = torch.full((nws,), float("nan"), device="cuda")
    L.check(lib.otvae_conv_generic_bwd_weight(C.byref(geom), L.ptr(xd), L.ptr(gyd), 1, L.ptr(ws_), L.ptr(gw), L.ptr(gb), L.stream()),
            "generic wgrad")
    torch.cuda.synchronize()
    errs = (T.rel(T.raw(y), T.raw(y64.detach())), T.rel(T.raw(gx), T.raw(x64.grad)), T.rel(gw, w64.grad.permute(2, 3, 1, 0)),
            T.rel(gb, b64.grad))
    print(f"generic {case}: rel err y {errs[0]:.3g} gx {errs[1]:.3g} gw {errs[2]:.3g} gb {errs[3]:.3g}")
    assert max(errs) < T.TOL, errs          # (NaN left in an output fails this comparison too)


# ---- rectangular inputs through the public modules, against the CPU oracle ----------------------------------------------------------
TOL = 1e-4          # the bounds of tests/test_gpu_attn_stage.py
TOL_BN_GRAD = 2e-3
TOL_RUNNING = 1e-5


def _fill(mod, seed):
    with torch.no_grad():
        for i, p in enumerate(mod.parameters()):
            p.copy_(normal(tuple(p.shape), seed + i).mul_(0.4 if p.dim() > 1 else 0.2))
        for name, p in mod.named_parameters():
            if name.endswith("_normalization.weight"):
                p.add_(1.0)
    return mod


def _module_vs_oracle(mod, x, oracle_fn, what, zero_bias=()):
    """Forward + backward of ``mod`` on the device against ``oracle_fn(x, p)`` in fp32 on the CPU, from the same state dict.

    ``zero_bias``: layers whose convolution feeds a training-mode BatchNorm.  That BatchNorm subtracts the per-channel mean, so the
    exact gradient of the bias is zero and both sides hold rounding noise of a sum whose terms cancel; an error relative to that
    noise says nothing.  The bias gradient is sum_i g_i over the output positions and the layer's weight gradient is sum_i a_i g_i
    with activations a_i of order 1 -- the same terms -- so these biases are measured against the oracle's weight gradient of the same
    layer, at the same bound (as tests/test_gpu_parity.py floors such gradients by the network's gradient scale)."""
    from ot_vae_lightning_amd import functional as HF
    sd0 = {k: v.detach().clone() for k, v in mod.state_dict().items()}
    xg = HF.as_nhwc(x.cuda()).requires_grad_(True)
    y = mod(xg)
    gy = normal(tuple(y.shape), 97)
    y.backward(HF.as_nhwc(gy.cuda()))
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu() for k, p in mod.named_parameters()}
    sd1 = {k: v.detach().cpu() for k, v in mod.state_dict().items()}
    p = {k: v.detach().cpu().clone().contiguous() for k, v in sd0.items()}
    leaves = {k: v.requires_grad_(True) for k, v in p.items() if v.is_floating_point() and "running" not in k}
    xc = x.clone().requires_grad_(True)
    yo = oracle_fn(xc, p)
    assert tuple(yo.shape) == tuple(y.shape), (what, yo.shape, y.shape)
    yo.backward(gy)
    e = {"y": rel_err(y.detach().cpu(), yo.detach()), "dx": rel_err(xg.grad.cpu(), xc.grad)}
    assert e["y"] < TOL and e["dx"] < TOL, (what, e)
    assert set(grads) == set(leaves)
    for k, v in leaves.items():
        if k in [layer + "bias" for layer in zero_bias]:
            scale = leaves[k[:-4] + "weight"].grad.abs().max().item()
            assert v.grad.abs().max().item() < TOL * scale, (what, k, "the oracle's own gradient is not noise")
            e[k] = (grads[k].double() - v.grad.double()).abs().max().item() / scale
        else:
            e[k] = rel_err(grads[k], v.grad)
        assert e[k] < (TOL_BN_GRAD if "_normalization" in k else TOL), (what, k, e[k])
    for k in sd1:
        if "running_" in k:
            e[k] = rel_err(sd1[k], p[k])
            assert e[k] < TOL_RUNNING, (what, k, e[k])
    print(what + ": " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))


LAYERS = [  # (constructor arguments, input shape, oracle arguments)
    (dict(in_features=8, out_features=16), (5, 8, 6, 10), dict(down=False, up=False)),
    (dict(in_features=8, out_features=16, down_sample=2), (5, 8, 8, 12), dict(down=True, up=False)),
    (dict(in_features=16, out_features=8, up_sample=2), (5, 16, 3, 5), dict(down=False, up=True)),
]


@pytest.mark.parametrize("kw,shape,okw", LAYERS, ids=["6x10", "down2_8x12", "up2_3x5"])
def test_conv_layer_batchnorm_relu_on_a_rectangle(kw, shape, okw):
    from ot_vae_lightning_amd.networks.cnn import ConvLayer
    layer = _fill(ConvLayer(normalization="batchnorm", activation="relu", **kw).cuda().train(), 31)
    _module_vs_oracle(layer, normal(shape, 3), lambda x, p: O.conv_layer(x, p, "", relu=True, norm=True, training=True, **okw),
                      f"ConvLayer {kw} on {shape}")


def test_conv_layer_groupnorm_silu_on_a_rectangle():
    from ot_vae_lightning_amd.networks.cnn import ConvLayer
    layer = _fill(ConvLayer(8, 8, normalization="groupnorm", activation="silu").cuda().train(), 37)
    _module_vs_oracle(layer, normal((3, 8, 5, 9), 3),
                      lambda x, p: O.conv_layer(x, p, "", down=False, up=False, relu=False, norm=False, other_norm="group", act="silu"),
                      "ConvLayer(8, 8, groupnorm, silu) on (3, 8, 5, 9)")


@pytest.mark.parametrize("fused", [True, False], ids=["one_launch", "three_launches"])
def test_attention_block_on_a_rectangle(fused):
    from ot_vae_lightning_amd import functional as HF
    from ot_vae_lightning_amd.networks.cnn import AttentionBlock
    if fused:
        rows = C.c_int(0)
        assert T.load().otvae_attn_stage_plan(6, 4 * 6, 4, 4, 1, C.byref(rows)) == 0, "shape expected to fuse"
    blk = _fill(AttentionBlock(16, heads=4, normalization="batchnorm").cuda().train(), 11)
    old = HF.ATTN_STAGE, HF.ATTN_STAGE_BWD, HF.attention_stage
    took = []

    def spy(*a, **kw):   # which route the block really took
        y = old[2](*a, **kw)
        took.append(y is not None)
        return y

    HF.ATTN_STAGE, HF.ATTN_STAGE_BWD, HF.attention_stage = fused, fused, spy
    try:
        _module_vs_oracle(blk, normal((6, 16, 4, 6), 3), lambda x, p: O.attention_block(x, p, "", 4, training=True),
                          f"AttentionBlock(16, heads=4) on (6, 16, 4, 6), fused={fused}")
    finally:
        HF.ATTN_STAGE, HF.ATTN_STAGE_BWD, HF.attention_stage = old
    assert took == [fused]


def test_down_sampling_conv_block_with_attention_on_a_rectangle():
    from ot_vae_lightning_amd.networks.cnn import ConvBlock
    blk = _fill(ConvBlock(8, 16, n_attn_heads=4, n_layers=2, down_sample=2, residual="add").cuda().train(), 41)   # 4x4 s2 p1, -> 4x6
    arch = dict(down=2, up=False, n_layers=2, heads=4, residual="add")
    _module_vs_oracle(blk, normal((5, 8, 8, 12), 3), lambda x, p: O.conv_block(x, p, "", arch, training=True),
                      "ConvBlock(8, 16, heads 4, down 2, add) on (5, 8, 8, 12)", zero_bias=("block.0.", "block.1."))
