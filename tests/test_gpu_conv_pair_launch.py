"""GPU: two image-tile jobs, or two direct-kernel jobs, of one ``otvae_conv_multi`` call in ONE launch (``conv_tile_kernel_pair``,
``conv_small_fwd_pair_kernel`` / ``conv_small_dgrad_pair_kernel``) against the same call with ``OTVAE_PAIR_LAUNCH=0`` (one launch per
job, the form before the two-job kernels).

The two-job kernels run the one-job bodies unchanged with a job-local block index, so everything a job writes must be BIT-EQUAL
(``torch.equal``) between the two: ``y`` / ``gv``, the fp64 partials ``[2][ld][P]`` (their block index is the job-local one), the
statistic slots (int64 limbs), and what a folded BatchNorm's first block publishes (scale / shift / mean / invstd / running buffers).
``otvae_conv_multi_launches`` must report 1 launch with the switch on and 2 with it off.

Cases: the ConvBlock heads of the capacity-8 network at 8x8 and larger maps -- two equal stride-2 branches; an up-sampling 3x3 with its
1x1 skip -- on the image-tile kernels and on the direct kernels (1 <-> 8 channels), forward and data gradient, at N = 3 and N = 5 (one
image per workgroup in the tile kernels, so 3 / 5 workgroups per job and a second job that starts at an odd block offset; a ragged
last 256-position block in the direct kernels).  One branch carries a BatchNorm affine, the other none.  Statistics go to fp64 partials
or to slots (forward: with the input's BatchNorm folded in).  The image-tile plan packs more than one image into a workgroup only
from about a thousand images on, so the tile pairs run again at N = 1025 / 1027 (two images per workgroup, a last group of one, the
two-job kernels the training step launches) and one pair at N = 2049 whose branches get DIFFERENT plans (two and four images per
workgroup: the two-arm form of the kernel, unequal grids and LDS); each of these asserts the block counts that show it.  Further:
three jobs in a call, a tile job beside an implicit-GEMM job
(no two-job kernel), and the packed data-gradient pair 16 -> 32 4x4 s2 8x8 -> 4x4 against separate calls.
"""
import ctypes as C

import pytest
import torch

import test_gpu_conv_abi as T

pytestmark = pytest.mark.gpu

# (cs, cn, hs, k, stride, pad, up) of branch 0 and branch 1
PAIRS = {
    "tile_s2_8to16_16x16": ((8, 16, 16, 4, 2, 1, 1), (8, 16, 16, 4, 2, 1, 1)),
    "tile_up_16to8_4x4": ((16, 8, 4, 3, 1, 1, 2), (16, 8, 4, 1, 1, 0, 2)),
    "tile_up_32to16_4x4": ((32, 16, 4, 3, 1, 1, 2), (32, 16, 4, 1, 1, 0, 2)),   # data gradient: two column blocks (grid y = 2)
    "tile_up_16to8_8x8": ((16, 8, 8, 3, 1, 1, 2), (16, 8, 8, 1, 1, 0, 2)),      # 256 positions per image: four row blocks per wave
    "small_s2_1to8_32x32": ((1, 8, 32, 4, 2, 1, 1), (1, 8, 32, 4, 2, 1, 1)),
    "small_up_8to1_16x16": ((8, 1, 16, 3, 1, 1, 2), (8, 1, 16, 1, 1, 0, 2)),
}
NSLOTS = 4

_cache = {}


def dev(n, spec, seed, **flags):
    """Device copy of one layer's tensors, built once and shared (never modified)."""
    key = (n, spec, seed, tuple(sorted(flags.items())))
    if key not in _cache:
        _cache[key] = T.Dev(T.make_case(n, *spec, seed=seed, **flags))
    return _cache[key]


def pair_devs(n, name):
    a, b = PAIRS[name]
    d0 = dev(n, a, 11)                                     # BatchNorm affine, bias, residual
    d1 = dev(n, b, 12, norm=False, bias=False, res=False)  # the skip branch: none of them
    return d0, d1


def nan_nhwc(n, ch, h, w):
    return T.nhwc(torch.full((n, ch, h, w), float("nan"), device="cuda"))


class Call:
    """One otvae_conv_multi call: the job array, and every tensor a job writes (fresh per call, NaN / zero filled)."""

    def __init__(self, n):
        self.L = T._L()
        self.lib = T.load()
        self.jobs = (self.L.ConvJob * n)()
        self.n = 0
        self.outs = []   # compared bit for bit between two calls
        self.keep = []

    def fwd(self, dv, x, stats):
        L, lib = self.L, self.lib
        jb = self.jobs[self.n]
        self.n += 1
        y = nan_nhwc(dv.n, dv.cn, dv.c["ho"], dv.c["wo"])
        p, ld = C.c_int(0), C.c_int(0)
        L.check(lib.otvae_conv_fwd_stats_ws(C.byref(dv.geom), C.byref(p), C.byref(ld)), "ws")
        jb.kind, jb.relu, jb.geom = L.JOB_FWD, int(dv.c["relu"]), dv.geom
        jb.x, jb.w, jb.bias, jb.residual, jb.y = L.ptr(x), L.ptr(dv.w_hwio), L.ptr(dv.bias), L.ptr(dv.res), L.ptr(y)
        self.outs.append(y)
        if stats == "partial":
            jb.scale, jb.shift = L.ptr(dv.scale), L.ptr(dv.shift)
            part = torch.full((2, ld.value, p.value), float("nan"), device="cuda", dtype=torch.float64)
            jb.stat_partial = L.ptr(part)
            self.outs.append(part[:, :dv.cn])    # the channels past Cn are padding the direct kernels leave unwritten
            return
        # the output's statistics into slots; the BatchNorm of x (where the branch has one) folded into the launch
        sl = torch.zeros(lib.otvae_bn_slots_words(ld.value, NSLOTS), device="cuda", dtype=torch.int64)
        jb.stat_slots, jb.stat_nslots = L.ptr(sl), NSLOTS
        self.outs.append(sl)
        if dv.scale is None:
            return
        cs, m = dv.cs, dv.n * dv.hs * dv.ws
        xs = torch.zeros(lib.otvae_bn_slots_words(cs, NSLOTS), device="cuda", dtype=torch.int64)
        L.check(lib.otvae_bn_stats_slots(L.ptr(x), m, cs, L.ptr(xs), cs, NSLOTS, L.stream()), "stats_slots")
        gamma, beta = dv.scale.clone(), dv.shift.clone()
        pub = [torch.full((cs,), float("nan"), device="cuda") for _ in range(4)]   # mean, invstd, scale, shift
        rmean, rvar = torch.linspace(-1, 1, cs, device="cuda"), torch.linspace(0.5, 2, cs, device="cuda")
        nbt = torch.tensor(7, device="cuda")
        f = jb.fold
        f.slots, f.ld, f.nslots, f.count, f.eps, f.momentum = L.ptr(xs), cs, NSLOTS, m, 1e-5, 0.1
        f.gamma, f.beta, f.running_mean, f.running_var, f.num_batches_tracked = L.ptr(gamma), L.ptr(beta), L.ptr(rmean), L.ptr(rvar), L.ptr(nbt)
        f.mean_out, f.invstd_out, f.scale_out, f.shift_out = (L.ptr(t) for t in pub)
        self.outs += pub + [rmean, rvar, nbt]
        self.keep += [xs, gamma, beta]

    def dgrad(self, dv, x, stats):
        L, lib = self.L, self.lib
        jb = self.jobs[self.n]
        self.n += 1
        gv = nan_nhwc(dv.n, dv.cs, dv.hs, dv.ws)
        p, cp = C.c_int(0), C.c_int(0)
        L.check(lib.otvae_conv_bwd_data_ws(C.byref(dv.geom), C.byref(p), C.byref(cp)), "ws")
        mean = torch.linspace(-0.2, 0.2, dv.cs, device="cuda")
        invstd = torch.linspace(0.8, 1.2, dv.cs, device="cuda")
        jb.kind, jb.relu, jb.geom = L.JOB_BWD_DATA, int(dv.c["relu"]), dv.geom
        jb.gy, jb.w, jb.x, jb.scale, jb.shift = L.ptr(dv.gy), L.ptr(dv.wd), L.ptr(x), L.ptr(dv.scale), L.ptr(dv.shift)
        jb.mean, jb.invstd, jb.gv = L.ptr(mean), L.ptr(invstd), L.ptr(gv)
        if stats == "partial":
            st = torch.full((2, cp.value, p.value), float("nan"), device="cuda", dtype=torch.float64)
            jb.bn_partial = L.ptr(st)
            st = st[:, :dv.cs]
        else:
            st = torch.zeros(lib.otvae_bn_slots_words(cp.value, NSLOTS), device="cuda", dtype=torch.int64)
            jb.bn_slots, jb.bn_nslots = L.ptr(st), NSLOTS
        self.outs += [gv, st]
        self.keep += [mean, invstd]

    def run(self):
        L, lib = self.L, self.lib
        assert self.n == len(self.jobs)
        L.check(lib.otvae_conv_multi(self.n, self.jobs, L.stream()), "multi")
        nl, mask, ut = C.c_int(-1), C.c_uint(0), C.c_int(0)
        L.check(lib.otvae_conv_multi_launches(C.byref(nl)), "launches")
        L.check(lib.otvae_conv_multi_last(C.byref(mask), C.byref(ut)), "last")
        torch.cuda.synchronize()
        return self.outs, nl.value, mask.value


def both_ways(build):
    """build() -> Call, run with the two-job launches on and off."""
    res = []
    for switch in (None, "0"):
        with T.env(OTVAE_PAIR_LAUNCH=switch, OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None, OTVAE_GEMM_LIVE_TAPS=None):
            res.append(build().run())
    return res


def assert_same_bits(on, off):
    assert len(on) == len(off)
    for i, (a, b) in enumerate(zip(on, off)):
        if a.is_floating_point():
            assert not torch.isnan(a).any(), f"output {i}: an element was not written"
        assert torch.equal(a, b), f"output {i} differs"


def build_pair(n, name, mode, stats, extra=None, pair=None):
    d0, d1 = pair_devs(n, name) if pair is None else pair
    call = Call(2 + (extra is not None))
    for dv in (d0, d1):
        (call.fwd if mode == "fwd" else call.dgrad)(dv, d0.x, stats)   # both branches read the same x
    if extra is not None:
        (call.fwd if mode == "fwd" else call.dgrad)(extra, extra.x, stats)
    return call


@pytest.mark.parametrize("stats", ["partial", "slots"])
@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_pair_in_one_launch_equals_two_launches(name, mode, n, stats):
    (on, n_on, m_on), (off, n_off, m_off) = both_ways(lambda: build_pair(n, name, mode, stats))
    assert (n_on, n_off) == (1, 2)
    assert m_on == m_off == 0            # otvae_conv_multi_last keeps its meaning: nothing ran inside conv_jobs_kernel
    assert_same_bits(on, off)


def blocks(dv, mode):
    """Workgroups over (grid x, grid z) of the one-job launch: what the workspace queries report as the number of partials."""
    L, lib = T._L(), T.load()
    p, ld = C.c_int(0), C.c_int(0)
    q = lib.otvae_conv_fwd_stats_ws if mode == "fwd" else lib.otvae_conv_bwd_data_ws
    L.check(q(C.byref(dv.geom), C.byref(p), C.byref(ld)), "ws")
    return p.value


# (pair, N, statistics, images per workgroup of branch 0 and of branch 1 in the forward plan / in the data-gradient plan)
MANY = [("tile_s2_8to16_16x16", 1025, "partial", (2, 2), (2, 2)),
        ("tile_up_16to8_4x4", 1027, "slots", (2, 2), (2, 2)),
        ("tile_up_32to16_4x4", 1025, "partial", (2, 2), (2, 2))]


@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("case", MANY, ids=[c[0] + "_n%d" % c[1] for c in MANY])
def test_tile_pair_with_two_images_per_workgroup_and_a_ragged_last_group(case, mode):
    name, n, stats, ipb_f, ipb_d = case
    d0, d1 = pair_devs(n, name)
    nz = 4 if (mode == "dgrad" and PAIRS[name][0][4] == 2) else 1    # stride-2 data gradient: one grid slice per input parity class
    for dv, ipb in zip((d0, d1), ipb_f if mode == "fwd" else ipb_d):
        assert blocks(dv, mode) == -(-n // ipb) * nz and n % ipb != 0, "the case no longer has the plan it was chosen for"
    (on, n_on, _), (off, n_off, _) = both_ways(lambda: build_pair(n, name, mode, stats))
    assert (n_on, n_off) == (1, 2)
    assert_same_bits(on, off)


def test_tile_pair_whose_branches_have_different_plans():
    """64 -> 32 up-sampling 3x3 with its 1x1 skip, 4x4 -> 8x8, forward, N = 2049: the 3x3 branch fits two images into a workgroup's LDS,
    the 1x1 branch four, so the two jobs have different bodies, grids (1025 and 513 workgroups) and LDS sizes; both last groups are ragged."""
    n, mode = 2049, "fwd"
    pair = (dev(n, (64, 32, 4, 3, 1, 1, 2), 21), dev(n, (64, 32, 4, 1, 1, 0, 2), 22, norm=False, bias=False, res=False))
    assert [blocks(dv, mode) for dv in pair] == [1025, 513], "the case no longer has the plans it was chosen for"
    (on, n_on, _), (off, n_off, _) = both_ways(lambda: build_pair(n, None, mode, "partial", pair=pair))
    assert (n_on, n_off) == (1, 2)
    assert_same_bits(on, off)


@pytest.mark.parametrize("order", ["skip_first"])
@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("name", ["small_up_8to1_16x16", "tile_up_16to8_4x4"])
def test_pair_is_found_in_either_order(name, mode, order):
    """The 1x1 skip handed in before the 3x3 branch: still one launch, same bits."""
    d0, d1 = pair_devs(3, name)
    (on, n_on, _), (off, n_off, _) = both_ways(lambda: build_pair(3, name, mode, "partial", pair=(d1, d0)))
    assert (n_on, n_off) == (1, 2)
    assert_same_bits(on, off)


@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_three_jobs_pair_and_a_single(name, mode):
    """The pair and a 3x3 layer on the same map: the pair shares a launch, the third job has no partner."""
    cs, _, hs = PAIRS[name][0][:3]
    single = dev(3, (cs, cs, hs, 3, 1, 1, 1), 13)
    (on, n_on, _), (off, n_off, _) = both_ways(lambda: build_pair(3, name, mode, "partial", extra=single))
    assert (n_on, n_off) == (2, 3)
    assert_same_bits(on, off)


@pytest.mark.parametrize("mode", ["fwd", "dgrad"])
def test_tile_job_beside_an_implicit_gemm_job_runs_as_before(mode):
    """No two-job kernel for an image-tile job and an implicit-GEMM job (32 -> 32 3x3 at 4x4): one launch each, either way."""
    tile, gemm = dev(5, PAIRS["tile_s2_8to16_16x16"][0], 11), dev(5, (32, 32, 4, 3, 1, 1, 1), 14)

    def build():
        call = Call(2)
        for dv in (tile, gemm):
            (call.fwd if mode == "fwd" else call.dgrad)(dv, dv.x, "partial")
        return call

    (on, n_on, _), (off, n_off, _) = both_ways(build)
    assert (n_on, n_off) == (2, 2)
    assert_same_bits(on, off)


def test_packed_dgrad_pair_16to32_s2_8x8_equals_separate_calls():
    """The data-gradient pair 16 -> 32 4x4 s2 8x8 -> 4x4 at N = 8 (implicit GEMM, packed by otvae_conv_multi) against the two jobs in
    calls of their own."""
    spec = (16, 32, 8, 4, 2, 1, 1)
    d0, d1 = dev(8, spec, 15), dev(8, spec, 16, norm=False, bias=False, res=False)
    with T.env(OTVAE_PAIR_LAUNCH=None, OTVAE_NO_TILE=None, OTVAE_TILE_ALL=None, OTVAE_GEMM_LIVE_TAPS=None):
        both = Call(2)
        for dv in (d0, d1):
            both.dgrad(dv, d0.x, "partial")
        together, _, mask = both.run()
        apart = []
        for dv in (d0, d1):
            one = Call(1)
            one.dgrad(dv, d0.x, "partial")
            apart += one.run()[0]
    assert mask == 0b11                  # both ran inside one conv_jobs_kernel launch
    assert_same_bits(together, apart)
