"""CPU: ``otvae_conv_gemm_chunks`` -- the host count of (tile, tap) visits of the implicit-GEMM convolution under the launch-wide tap
list and under the per-tile list of the position-major vector paths.  It walks the same row order with the same in-range predicate
as the kernel (one ``__host__ __device__`` function), so these counts are what the kernel's K loops run.

The expected ratios are counted here from first principles: with the batch a multiple of the 64-row tile every tile holds ONE output
position, so per-tile / launch-rule = (sum over positions of the taps that position can use) / (positions x taps some position can use).
"""
import ctypes as C
from fractions import Fraction

import pytest


@pytest.fixture(scope="module")
def lib():
    from ot_vae_lightning_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def geom(n, cs, cn, hs, k, stride, pad, up):
    from ot_vae_lightning_amd import _lib
    ho = (hs * up + 2 * pad - k) // stride + 1
    return _lib.ConvGeom(n, hs, hs, cs, up, ho, ho, cn, k, k, stride, pad)


def chunks(lib, case, mode):
    a, b = C.c_int64(-1), C.c_int64(-1)
    g = geom(*case)
    rc = lib.otvae_conv_gemm_chunks(C.byref(g), mode, C.byref(a), C.byref(b))
    return rc, a.value, b.value


def fwd_ratio(hs, k, stride, pad, up):
    """(position, tap) visits of the forward pass, per position / launch rule, by brute force on one image."""
    hu = hs * up
    ho = (hu + 2 * pad - k) // stride + 1
    live1 = [[0 <= o * stride + t - pad < hu for t in range(k)] for o in range(ho)]   # one axis: position o, tap t
    per_pos = sum(sum(r) for r in live1) ** 2                                           # square maps and kernels: the axes factor
    any_tap = sum(any(live1[o][t] for o in range(ho)) for t in range(k))
    return Fraction(per_pos, (ho * any_tap) ** 2)


# the deep layers of the benchmark's network at batch 1024: (n, cs, cn, hs, k, stride, pad, up), forward ratio of the issue's table
LAYERS = [
    ((1024, 16, 32, 8, 4, 2, 1, 1), Fraction(196, 256)),
    ((1024, 32, 32, 4, 3, 1, 1, 1), Fraction(100, 144)),
    ((1024, 32, 64, 4, 4, 2, 1, 1), Fraction(36, 64)),
    ((1024, 64, 64, 2, 3, 1, 1, 1), Fraction(16, 36)),
    ((1024, 128, 64, 1, 3, 1, 1, 2), Fraction(16, 36)),
    ((1024, 64, 32, 2, 3, 1, 1, 2), Fraction(100, 144)),
]


@pytest.mark.parametrize("case,want", LAYERS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_ratios_of_the_benchmark_layers(lib, case, want):
    n, cs, cn, hs, k, stride, pad, up = case
    assert fwd_ratio(hs, k, stride, pad, up) == want          # the table's figure is the brute-force count
    rc, launch, tile = chunks(lib, case, 0)
    assert rc == 0 and launch > 0
    assert Fraction(tile, launch) == want
    rc, launch, tile = chunks(lib, case, 1)
    assert rc == 0 and launch > 0
    # data gradient: the transposed problem has the same per-position counts; with up-sampling the 4 children of a source pixel
    # share a lane and together see every tap, so nothing is dropped
    assert Fraction(tile, launch) == (Fraction(1) if up == 2 else want)


def test_counts_are_tile_times_tap(lib):
    # 64 -> 64 3x3 on 2x2 maps, batch 1024: 4096 rows = 64 tiles; 9 taps under the launch rule, 4 per corner position
    rc, launch, tile = chunks(lib, (1024, 64, 64, 2, 3, 1, 1, 1), 0)
    assert (rc, launch, tile) == (0, 64 * 9, 64 * 4)
    # a ragged batch: 70 images x 4 positions = 280 rows = 5 tiles; tile 0 and the 24-row tail hold one corner (4 taps), tiles 1 and 3
    # two corners of one image row (2 x 3 taps), tile 2 the corners (0, 1) and (1, 0), which share only the centre tap (4 + 4 - 1)
    rc, launch, tile = chunks(lib, (70, 64, 64, 2, 3, 1, 1, 1), 0)
    assert (rc, launch, tile) == (0, 5 * 9, 4 + 6 + 7 + 6 + 4)


def test_1x1_kernel_and_1x1_output_have_nothing_to_drop(lib):
    for case in [(1024, 64, 64, 2, 1, 1, 0, 1), (1024, 64, 256, 2, 4, 2, 1, 1)]:
        rc, launch, tile = chunks(lib, case, 0)
        assert rc == 0 and launch == tile > 0
    rc, launch, tile = chunks(lib, (1024, 64, 64, 2, 1, 1, 0, 1), 1)
    assert rc == 0 and launch == tile > 0


def test_layers_of_other_kernel_families_are_not_served(lib):
    from ot_vae_lightning_amd import _lib
    for mode in (0, 1):
        rc, _, _ = chunks(lib, (1024, 8, 8, 16, 3, 1, 1, 1), mode)      # image-tile kernels
        assert rc == -2
        assert "not served by the implicit GEMM" in _lib.last_error()
    rc, _, _ = chunks(lib, (4, 1, 8, 32, 4, 2, 1, 1), 0)                # direct kernels
    assert rc == -2


def test_bad_arguments(lib):
    g = geom(64, 64, 64, 2, 3, 1, 1, 1)
    a, b = C.c_int64(), C.c_int64()
    assert lib.otvae_conv_gemm_chunks(C.byref(g), 2, C.byref(a), C.byref(b)) == -1
    assert lib.otvae_conv_gemm_chunks(C.byref(g), 0, None, C.byref(b)) == -1
    assert lib.otvae_conv_gemm_chunks(None, 0, C.byref(a), C.byref(b)) == -1
