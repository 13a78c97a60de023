"""GPU: the implicit-GEMM convolution with position-major rows and a tap list per tile (the default of the vector paths) against

  (a) the same kernels in memory row order with the launch-wide tap list (``OTVAE_GEMM_LIVE_TAPS=0``): a dropped tap has all-zero A
      rows and the kept taps keep their (kh, kw) order, so ``y`` and ``gv`` must agree BIT FOR BIT;
  (b) the image-tile family (``OTVAE_TILE_ALL=1``), bit for bit as well;
  (c) the float64 restatement of tests/test_gpu_conv_abi.py, at that file's tolerance (fp32 accumulation over K <= 1152 products);
  (d) completeness: every output element written (the buffers start as NaN), and the per-channel BatchNorm sums equal to the fp64 sums
      of the tensors the kernel wrote (1e-10: fp64 accumulation of <= 2e4 terms);
  (e) two-branch ``otvae_conv_multi`` calls against single calls, bit for bit, partial sums included.

Shapes are the smallest that reach each path: one position class per tile, class boundaries inside a tile, ragged last tiles, the
stride-2 parity classes, the up-2 children grouping, the non-uniform-tap vector path, and the scalar path that must stay as it was.
"""
import ctypes as C

import pytest
import torch

import test_gpu_conv_abi as T

pytestmark = pytest.mark.gpu

# (n, cs, cn, hs, k, stride, pad, up)
CASES = [
    (64, 64, 64, 2, 3, 1, 1, 1),     # every tile one position class, uniform-tap pipeline
    (70, 64, 64, 2, 3, 1, 1, 1),     # class boundaries inside tiles, last tile ragged
    (37, 32, 32, 4, 3, 1, 1, 1),     # corner / edge / interior classes
    (21, 32, 64, 4, 4, 2, 1, 1),     # stride 2: parity classes x position classes in the data gradient
    (19, 16, 32, 8, 4, 2, 1, 1),     # forward CK = 16: the non-uniform-tap vector path, a chunk spans two taps
    (70, 128, 64, 1, 3, 1, 1, 2),    # up 2 forward; children grouping in the data gradient
    (23, 64, 32, 2, 3, 1, 1, 2),     # up 2 forward; children grouping in the data gradient
    (5, 12, 20, 4, 3, 1, 1, 1),      # CK % 4 == 0 but not % 32, Cn not a multiple of 16
    (1, 32, 32, 4, 3, 1, 1, 1),      # a single image
    (33, 64, 128, 2, 4, 2, 1, 1),    # forward already live-only: must not change
    (6, 3, 5, 4, 3, 1, 1, 1),        # channel counts not multiples of 4: must take the old path
]
IDS = ["n%d_%dto%d_%dx%d_k%ds%dp%du%d" % (c[0], c[1], c[2], c[3], c[3], c[4], c[5], c[6], c[7]) for c in CASES]

_cache = {}


def prepared(case, **flags):
    """One case: host tensors, float64 reference and device copies, built once and shared (never modified)."""
    key = (case, tuple(sorted(flags.items())))
    if key not in _cache:
        c = T.make_case(*case, seed=sum(case), **flags)
        _cache[key] = (c, T.ref64(c), T.Dev(c))
    return _cache[key]


def nan_nhwc(n, ch, h, w=None):
    return T.nhwc(torch.full((n, ch, h, h if w is None else w), float("nan"), device="cuda"))


def fwd(dv):
    L, lib = T._L(), T.load()
    y = nan_nhwc(dv.n, dv.cn, dv.c["ho"], dv.c["wo"])
    p, ld = C.c_int(0), C.c_int(0)
    L.check(lib.otvae_conv_fwd_stats_ws(C.byref(dv.geom), C.byref(p), C.byref(ld)), "ws")
    part = torch.full((2, ld.value, p.value), float("nan"), device="cuda", dtype=torch.float64)
    L.check(lib.otvae_conv_fwd(C.byref(dv.geom), L.ptr(dv.x), L.ptr(dv.scale), L.ptr(dv.shift), int(dv.c["relu"]),
                               L.ptr(dv.w_hwio), L.ptr(dv.bias), L.ptr(dv.res), L.ptr(y), L.ptr(part), L.stream()), "fwd")
    torch.cuda.synchronize()
    return y, part[:, :dv.cn, :].sum(-1)


def dgrad(dv):
    L, lib = T._L(), T.load()
    gv = nan_nhwc(dv.n, dv.cs, dv.hs, dv.ws)
    p, cp = C.c_int(0), C.c_int(0)
    L.check(lib.otvae_conv_bwd_data_ws(C.byref(dv.geom), C.byref(p), C.byref(cp)), "ws")
    mean = torch.linspace(-0.2, 0.2, dv.cs, device="cuda")
    invstd = torch.linspace(0.8, 1.2, dv.cs, device="cuda")
    part = torch.full((2, cp.value, p.value), float("nan"), device="cuda", dtype=torch.float64)
    L.check(lib.otvae_conv_bwd_data(C.byref(dv.geom), L.ptr(dv.gy), L.ptr(dv.wd), L.ptr(dv.x), L.ptr(dv.scale), L.ptr(dv.shift),
                                    int(dv.c["relu"]), L.ptr(mean), L.ptr(invstd), L.ptr(gv), L.ptr(part), L.stream()), "dgrad")
    torch.cuda.synchronize()
    return gv, part[:, :dv.cs, :].sum(-1), mean, invstd


def check_case(case, **flags):
    n, cs, cn, hs, k, s, p, up = case
    c, (y64, gv64, _, _), dv = prepared(case, **flags)
    gemm = dict(OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None)
    with T.env(OTVAE_GEMM_LIVE_TAPS=None, **gemm):
        y, ysum = fwd(dv)
        gv, gsum, mean, invstd = dgrad(dv)
    with T.env(OTVAE_GEMM_LIVE_TAPS="0", **gemm):
        y0, _ = fwd(dv)
        gv0, _, _, _ = dgrad(dv)
    with T.env(OTVAE_GEMM_LIVE_TAPS=None, OTVAE_NO_TILE=None, OTVAE_TILE_ALL="1"):
        yt, _ = fwd(dv)
        gvt, _, _, _ = dgrad(dv)
    # (d) every element written
    assert not torch.isnan(y).any() and not torch.isnan(gv).any()
    # (a), (b) same fp32 arithmetic in the same order
    assert torch.equal(y, y0) and torch.equal(gv, gv0)
    assert torch.equal(y, yt) and torch.equal(gv, gvt)
    # (c)
    ey, eg = T.rel(T.raw(y), T.raw(y64)), T.rel(T.raw(gv), T.raw(gv64))
    print(f"{case}: rel err y {ey:.3g} gv {eg:.3g}")
    assert ey < T.TOL and eg < T.TOL
    # (d) BatchNorm sums: fp64 sums of the fp32 tensors the kernel wrote
    yd = T.raw(y).double().reshape(-1, cn)
    gd = T.raw(gv).double().reshape(-1, cs)
    xhat = ((T.raw(dv.x).reshape(-1, cs) - mean) * invstd).double()      # the kernel's fp32 (x - mean) * invstd, then widened
    sums = [T.rel(ysum[0], yd.sum(0)), T.rel(ysum[1], (yd * yd).sum(0)),
            T.rel(gsum[0], gd.sum(0)), T.rel(gsum[1], (gd * xhat).sum(0))]
    print(f"{case}: rel err of the sums: y {sums[0]:.3g} y^2 {sums[1]:.3g} gv {sums[2]:.3g} gv*xhat {sums[3]:.3g}")
    assert max(sums) < 1e-10


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_live_taps_vs_row_major_tile_family_and_float64(case):
    check_case(case)


def test_without_norm_relu_bias_residual():
    check_case(CASES[0], norm=False, relu=False, bias=False, res=False)


def test_host_count_sees_what_the_test_cases_exercise():
    """The cases above do reach the paths they are named for: tiles that drop taps, and layers where nothing can be dropped."""
    L, lib = T._L(), T.load()

    def chunks(case, mode):
        n, cs, cn, hs, k, s, p, up = case
        ho = (hs * up + 2 * p - k) // s + 1
        g = L.ConvGeom(n, hs, hs, cs, up, ho, ho, cn, k, k, s, p)
        a, b = C.c_int64(), C.c_int64()
        L.check(lib.otvae_conv_gemm_chunks(C.byref(g), mode, C.byref(a), C.byref(b)), "chunks")
        return a.value, b.value

    with T.env(OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None):
        for case in CASES[:5] + [CASES[7]]:
            for mode in (0, 1):
                a, b = chunks(case, mode)
                assert 0 < b < a, (case, mode, a, b)
        a, b = chunks(CASES[8], 0)                   # one image: one tile holds every position, and with them every tap
        assert a == b > 0
        for case in CASES[5:7]:                      # up 2: forward drops, the data gradient (children together) cannot
            a, b = chunks(case, 0)
            assert 0 < b < a
            a, b = chunks(case, 1)
            assert a == b > 0
        a, b = chunks(CASES[9], 0)                   # 2x2 -> 1x1: the launch-wide list is already the live one
        assert a == b > 0


# (e) packed two-branch calls: (branch a, branch b) read the same input
# (8 entries: square, the tuple of CASES; 10 entries: (n, cs, cn, hs, ws, kh, kw, stride, pad, up))
MULTI = [((70, 64, 64, 2, 3, 1, 1, 1), (70, 64, 64, 2, 1, 1, 0, 1)),
         ((21, 32, 64, 4, 4, 2, 1, 1), (21, 32, 64, 4, 4, 2, 1, 1)),
         ((70, 64, 64, 2, 3, 3, 3, 1, 1, 1), (70, 64, 64, 2, 3, 1, 1, 1, 0, 1)),
         ((21, 32, 64, 4, 6, 4, 4, 2, 1, 1), (21, 32, 64, 4, 6, 4, 4, 2, 1, 1))]


@pytest.mark.parametrize("pair", MULTI, ids=["3x3_with_1x1_at_2x2", "two_4x4s2_at_4x4", "3x3_with_1x1_at_2x3", "two_4x4s2_at_4x6"])
def test_packed_two_branch_calls_equal_single_calls(pair):
    L, lib = T._L(), T.load()
    mk = lambda case, **kw: T.make_case(*case, **kw) if len(case) == 8 else T.make_case2(case, **kw)  # noqa: E731
    dvs = [T.Dev(mk(pair[0], seed=5)), T.Dev(mk(pair[1], bias=False, seed=6))]
    dvs[1].x = dvs[0].x
    singles = []
    for dv in dvs:
        y, ysum = fwd(dv)
        gv, gsum, _, _ = dgrad(dv)
        singles.append((y, ysum, gv, gsum))
    mask, ut = C.c_uint(0), C.c_int(0)
    # ---- forward
    jobs = (L.ConvJob * 2)()
    outs = []
    for jb, dv in zip(jobs, dvs):
        p, ld = C.c_int(0), C.c_int(0)
        L.check(lib.otvae_conv_fwd_stats_ws(C.byref(dv.geom), C.byref(p), C.byref(ld)), "ws")
        part = torch.full((2, ld.value, p.value), float("nan"), device="cuda", dtype=torch.float64)
        y = nan_nhwc(dv.n, dv.cn, dv.c["ho"], dv.c["wo"])
        jb.kind, jb.relu, jb.geom = L.JOB_FWD, int(dv.c["relu"]), dv.geom
        jb.x, jb.scale, jb.shift, jb.w = L.ptr(dv.x), L.ptr(dv.scale), L.ptr(dv.shift), L.ptr(dv.w_hwio)
        jb.bias, jb.residual, jb.y, jb.stat_partial = L.ptr(dv.bias), L.ptr(dv.res), L.ptr(y), L.ptr(part)
        outs.append((y, part))
    L.check(lib.otvae_conv_multi(2, jobs, L.stream()), "multi fwd")
    L.check(lib.otvae_conv_multi_last(C.byref(mask), C.byref(ut)), "last")
    torch.cuda.synchronize()
    assert mask.value == 0b11                        # both branches ran inside one packed launch
    for (y, part), dv, single in zip(outs, dvs, singles):
        assert torch.equal(y, single[0])
        assert torch.equal(part[:, :dv.cn].sum(-1), single[1])
    # ---- data gradient
    jobs = (L.ConvJob * 2)()
    outs, keep = [], []
    for jb, dv in zip(jobs, dvs):
        pd, cp = C.c_int(0), C.c_int(0)
        L.check(lib.otvae_conv_bwd_data_ws(C.byref(dv.geom), C.byref(pd), C.byref(cp)), "ws")
        gv = nan_nhwc(dv.n, dv.cs, dv.hs, dv.ws)
        mean = torch.linspace(-0.2, 0.2, dv.cs, device="cuda")
        invstd = torch.linspace(0.8, 1.2, dv.cs, device="cuda")
        part = torch.full((2, cp.value, pd.value), float("nan"), device="cuda", dtype=torch.float64)
        jb.kind, jb.relu, jb.geom = L.JOB_BWD_DATA, int(dv.c["relu"]), dv.geom
        jb.gy, jb.w, jb.x, jb.scale, jb.shift = L.ptr(dv.gy), L.ptr(dv.wd), L.ptr(dv.x), L.ptr(dv.scale), L.ptr(dv.shift)
        jb.mean, jb.invstd, jb.gv, jb.bn_partial = L.ptr(mean), L.ptr(invstd), L.ptr(gv), L.ptr(part)
        outs.append((gv, part))
        keep += [mean, invstd]
    L.check(lib.otvae_conv_multi(2, jobs, L.stream()), "multi dgrad")
    L.check(lib.otvae_conv_multi_last(C.byref(mask), C.byref(ut)), "last")
    torch.cuda.synchronize()
    assert mask.value == 0b11
    for (gv, part), dv, single in zip(outs, dvs, singles):
        assert torch.equal(gv, single[2])
        assert torch.equal(part[:, :dv.cs].sum(-1), single[3])
