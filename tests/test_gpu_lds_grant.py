"""GPU: every launch that asks for more than 64 KiB of dynamic LDS goes through ``otvae_lds_grant`` (csrc/common.h), which remembers
the grant per kernel AND per device (run with ``-m gpu``).

One case per public entry whose kernel can cross 64 KiB, at the smallest supported shape that crosses, derived from the launcher's own
LDS formula (next to each case).  A case is the entry's EXISTING GPU test called with that shape -- the same reference, the same
tolerance, nothing new -- or, where that test is not a function of the shape, the existing helpers and the existing bounds.  Every case
runs on the calling thread's current device.

``test_second_device_gets_its_own_grant`` runs the cases on ``cuda:0`` and then on ``cuda:1`` in ONE fresh process (this file as a
script), so that the host-side records start cold and the second device meets them warm from the first: each device must meet the same
bounds, the entries documented as bit-reproducible (``mmd_prior``, loss / terms / gradient) must give the same bits on both, and a
Sinkhorn prior on ``cuda:1`` runs the per-device CU lookup (``otvae_cu_count``) for a second device."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 300   # seconds for the two-device child: a dozen cases of a few seconds each, twice, and the imports


def _pkg():
    import ot_vae_lightning_amd as pkg
    return pkg


# mmd.hip: ld = roundup32(D) + 4 words per staged row, LDS = (2 * 32 * ld + 32 * 36 + 4 * 32) * 4 bytes = (64 ld + 1280) words; above
# 16384 words from ld = 237, i.e. roundup32(D) = 256: D = 225 (ld = 260, 71 680 bytes; D = 224: ld = 228, 63 488 bytes).  One row tile.
def case_mmd(kernel):
    import test_gpu_mmd as M
    M._device_run.cache_clear()     # the cached run may be another device's
    _, _, loss, G, terms, _ = M._check(_pkg(), 32, 32, 225, kernel, M.DEFAULT, True)
    return dict(loss=loss.cpu(), G=G.cpu(), terms=terms.cpu())


# mvn.hip, full covariance: (D * D + D) * 8 bytes = 66 976 at D = 91 (D = 90: 65 520); forward and backward.  The case of
# ot_dense_cases.MVN_CASES that sits right after the switch, with the assertions of test_gpu_ot_dense.py.
def case_mvn():
    import ot_dense_cases as C
    import test_gpu_ot_dense as OD
    from ot_vae_lightning_amd import _lib
    case = (2, 257, 91)
    assert case in C.MVN_CASES and C.mvn_lds_bytes(91, False) > 65536 >= C.mvn_lds_bytes(90, False)
    lp, y, qg = OD._mvn(_lib.load(), case, False)
    t = C.mvn_truth(case, False)
    _, _, Lm, g = C.mvn_inputs(case, False)
    grads = C.mvn_caller_side(qg, y, Lm, g, False)
    errs = dict(lp=C.rel_to_max(lp, t["lp"]), y=C.rel_to_max(y, t["y"]), **{k: C.rel_to_max(grads[k], t[k]) for k in grads})
    print(f"[lds_grant] mvn {case} full: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["lp"] <= C.MVN_TOL and errs["y"] <= C.MVN_TOL, errs
    assert max(errs["dx"], errs["dmean"], errs["dL"]) <= C.MVN_GRAD_TOL, errs


# eigh_onesided.hip, one matrix per workgroup (D <= 128): roundup2(D) * (D + 1) * 8 bytes = 92 * 92 * 8 = 67 712 at D = 91
# (D = 90: 65 520).  otvae_eigh_fn cold and otvae_eigh_fn_warm from two bases.
def case_eigh_one_workgroup():
    import test_gpu_parity as P
    P.test_warm_started_eigensolver_gives_the_same_decomposition(91)


# eigh_onesided.hip, block solver (128 < D <= 1024): 16 columns of roundup16(D) + 1 doubles = 128 * (roundup16(D) + 1) bytes.  D = 160
# takes that path with 20 608 bytes (no grant); the first D above 64 KiB is 497 (512 + 1 rows: 65 664 bytes; D = 496: 63 616).
def case_eigh_block(D):
    import test_gpu_parity as P
    P.test_block_jacobi_eigh_large_D(_pkg(), D)


# ar_decode.hip: ARD_ROWS * (4 D + 2 * ARD_PAD) * 4 = 16 * (4 D + 8) * 4 bytes, above 65 536 from 4 D + 8 > 1024: D = 256 with
# D % 16 == 0 (66 048 bytes; D = 240: 61 952).  17 rows are two workgroups; three positions.
def case_ar_layer_step():
    import test_gpu_ar_decode as AR
    AR.test_layer_step_vs_fp64_truth(_pkg(), 17, 256, 4, 64, 3, False)


# attention.hip, the fused AttentionBlock stage: a workgroup holds s = min(256 / T, (24576 - weights) / per_slice) slices.  At a 2 x 2
# map (T = 4) with one head of width 32: forward per_slice = T * 4 C = 512 floats, weights 4 * 32 * 32 -> s = 40, 98 304 bytes;
# backward per_slice = T * (2 C + 68 + 2 C) = 784, weights 7 * 1024 + 512 -> s = 21, 96 576 bytes.  No smaller T * H * C crosses either
# way (searched over the formula of attn_stage_shape); the batch does not enter.  Five images: 20 samples per BatchNorm channel.
def case_attn_stage():
    import test_gpu_attn_stage as AT
    AT.test_stage_vs_oracle_and_three_launches(_pkg(), 5, 32, 2, 1, False)


# conv_tile.hip: (images per block * Hv * Wv * (CK + 4) + weight chunk) * 4 + reduction area.  A 3x3 stride-1 layer on a 16 x 16 map
# stages 18 * 18 positions of one image: with 36 channels either way the forward and the data-gradient plan take 69 248 bytes
# (32 channels: below 64 KiB).  conv_wtile.hip: the same layer with 20 -> 40 channels stages x and gy of one image in 73 104 bytes
# (and its data gradient, 40 channels staged, 74 432).  Both from conv_tile_plan / conv_wtile_plan evaluated on the host.
def case_conv_layer(cs, cn):
    import test_gpu_conv_abi as CA
    CA.test_conv_entry_points_vs_float64(CA.load(), (3, cs, cn, 16, 3, 1, 1, 1))


# conv_tile.hip, two jobs in one launch: two of the 36 -> 36 layers above (plans nt = 1, rbw = 4: the pair kernel (1, 4, 1, 4) exists
# forward and backward), LDS = the larger plan = 69 248 bytes <= the 96 KiB the pair launcher accepts.
def case_conv_pair(mode):
    import test_gpu_conv_pair_launch as PL
    PL._cache.clear()               # device tensors of another device
    spec = (36, 36, 16, 3, 1, 1, 1)
    pair = (PL.dev(3, spec, 11), PL.dev(3, spec, 12, norm=False, bias=False, res=False))
    (on, n_on, _), (off, n_off, _) = PL.both_ways(lambda: PL.build_pair(3, None, mode, "partial", pair=pair))
    assert (n_on, n_off) == (1, 2)
    PL.assert_same_bits(on, off)
    PL._cache.clear()


CASES = {
    "mmd_imq_d225": lambda: case_mmd("imq"),
    "mmd_rbf_d225": lambda: case_mmd("rbf"),
    "mvn_full_d91": case_mvn,
    "eigh_d91_cold_and_warm": case_eigh_one_workgroup,
    "eigh_block_d160": lambda: case_eigh_block(160),
    "eigh_block_d497": lambda: case_eigh_block(497),
    "ar_layer_step_d256": case_ar_layer_step,
    "attn_stage_w32_2x2": case_attn_stage,
    "conv_tile_36to36_16x16": lambda: case_conv_layer(36, 36),
    "conv_wtile_20to40_16x16": lambda: case_conv_layer(20, 40),
    "conv_pair_fwd_36to36_16x16": lambda: case_conv_pair("fwd"),
    "conv_pair_dgrad_36to36_16x16": lambda: case_conv_pair("dgrad"),
}
BIT_REPRODUCIBLE = ("mmd_imq_d225", "mmd_rbf_d225")
# on one device test_gpu_ot_dense.py::test_mvn_logprob_across_the_lds_switch already runs this very case: only the second device needs it
SECOND_DEVICE_ONLY = ("mvn_full_d91",)


@pytest.mark.parametrize("name", [n for n in CASES if n not in SECOND_DEVICE_ONLY])
def test_launch_above_64_kib(name):
    assert torch.cuda.is_available()
    CASES[name]()


def _sinkhorn_prior():
    from detfill import normal
    _pkg()
    z, y = normal((64, 8), 71).cuda(), normal((64, 8), 72).cuda()
    cost, pi, iters = torch.ops.otvae.sinkhorn_prior(z, y, 0.05, 50, 0.0, 1.0)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cost).all()) and bool(torch.isfinite(pi).all())
    return cost.cpu()


def _two_devices(first=0, second=1):
    """every case on ``first`` (results under key 0), then on ``second`` (key 1), in this process"""
    from conftest import rel_err
    out = {}
    for d, device in enumerate((first, second)):
        torch.cuda.set_device(device)
        for name, fn in CASES.items():
            print(f"[lds_grant] cuda:{device} {name}", flush=True)
            out[d, name] = fn()
        out[d, "sinkhorn"] = _sinkhorn_prior()   # (cuda:0 too: the value cuda:1 is held to)
    for name in BIT_REPRODUCIBLE:
        for k, v in out[0, name].items():
            assert torch.equal(v, out[1, name][k]), f"{name}: {k} differs between the devices"
    # the Sinkhorn loss of the second device, whose residency test reads ITS CU count: the fp32 contract for a loss (1e-4 relative)
    err = rel_err(out[1, "sinkhorn"], out[0, "sinkhorn"])
    print(f"[lds_grant] sinkhorn prior cuda:1 vs cuda:0: rel {err:.2e}")
    assert err <= 1e-4
    print("[lds_grant] two devices: ok")


def test_second_device_gets_its_own_grant():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--two-devices"], capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0, f"the two-device child ended with {r.returncode}"
    assert "[lds_grant] two devices: ok" in r.stdout


if __name__ == "__main__":
    assert sys.argv[1:] == ["--two-devices"], sys.argv
    import conftest  # noqa: F401  (puts the repository and the oracle on sys.path)
    assert torch.cuda.device_count() >= 2
    _two_devices()
