"""CPU: ``otvae_conv_gemm_chunks`` -- the host count of (tile, tap) visits of the implicit-GEMM convolution under the launch-wide tap
list and under the per-tile list of the position-major vector paths.  It walks the same row order with the same in-range predicate
as the kernel (one ``__host__ __device__`` function), so these counts are what the kernel's K loops run.

The expected ratios are counted here from first principles: with the batch a multiple of the 64-row tile every tile holds ONE output
position, so per-tile / launch-rule = (sum over positions of the taps that position can use) / (positions x taps some position can use).

The second half takes the two axes apart: rectangular maps, KH != KW, pad > (k-1)/2 and stride 2 with unequal parity classes against a
row-by-row count (forward and data gradient), ``otvae_conv_dead_taps`` against a position-by-position mask, and the geometries every
``otvae_conv_*`` entry point must refuse (negative padding, an empty output, sizes of the other axis).
"""
import ctypes as C
from fractions import Fraction

import pytest


@pytest.fixture(scope="module")
def lib():
    from ot_vae_lightning_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def geom(n, cs, cn, hs, k, stride, pad, up, ws=None, kw=None):
    """``ws`` / ``kw``: width of the map / of the kernel when it differs from the height ``hs`` / ``k``."""
    from ot_vae_lightning_amd import _lib
    ws = hs if ws is None else ws
    kw = k if kw is None else kw
    ho = (hs * up + 2 * pad - k) // stride + 1
    wo = (ws * up + 2 * pad - kw) // stride + 1
    return _lib.ConvGeom(n, hs, ws, cs, up, ho, wo, cn, k, kw, stride, pad)


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


# ---- two axes: rectangular maps, non-square kernels, pad > (k-1)/2, stride 2 with unequal parity classes ---------------------------
# (hs, ws, kh, kw, stride, pad, up) at n = 70, 64 -> 64 channels (the vector paths: position-major rows, a tap list per tile)
RECT = [(1, 4, 3, 3, 1, 1, 1), (4, 1, 3, 3, 1, 1, 1), (2, 3, 3, 3, 1, 1, 1), (2, 6, 4, 4, 2, 1, 1), (1, 3, 3, 3, 1, 1, 2),
        (2, 3, 3, 5, 1, 1, 1), (2, 3, 5, 3, 1, 2, 1), (4, 6, 4, 4, 2, 1, 1), (2, 2, 3, 5, 1, 2, 1), (6, 4, 3, 3, 1, 2, 1),
        (2, 4, 1, 1, 2, 0, 1), (4, 6, 3, 3, 2, 1, 1)]
RECT_N, RECT_C, TILE = 70, 64, 64


def rect_geom(r, n=RECT_N, cs=RECT_C, cn=RECT_C):
    hs, ws, kh, kw, stride, pad, up = r
    return geom(n, cs, cn, hs, kh, stride, pad, up, ws=ws, kw=kw)


def out_size(r):
    hs, ws, kh, kw, stride, pad, up = r
    return (hs * up + 2 * pad - kh) // stride + 1, (ws * up + 2 * pad - kw) // stride + 1


def fwd_taps(r, oy, ox):
    """Taps (kh, kw) under which the output position (oy, ox) reads a pixel of the (up-sampled) input rather than padding."""
    hs, ws, kh, kw, stride, pad, up = r
    return {(a, b) for a in range(kh) for b in range(kw)
            if 0 <= oy * stride + a - pad < hs * up and 0 <= ox * stride + b - pad < ws * up}


def dgrad_taps(r, iy, ix):
    """Taps through which the (up-sampled) input position (iy, ix) was read by some output position: iy = oy * stride + kh - pad."""
    hs, ws, kh, kw, stride, pad, up = r
    ho, wo = out_size(r)
    return {(a, b) for a in range(kh) for b in range(kw)
            if (iy + pad - a) % stride == 0 and 0 <= (iy + pad - a) // stride < ho
            and (ix + pad - b) % stride == 0 and 0 <= (ix + pad - b) // stride < wo}


def brute_chunks(r, mode, n=RECT_N):
    """(launch rule, per tile, exact launch rule) counted row by row.  Every launch lists its rows position-major (the image index
    runs fastest), cut into tiles of 64; a tile visits the taps some row of it can use.  Forward: one launch, rows = output
    positions.  Data gradient: rows = input positions; stride 2 is one launch per parity class (iy % 2, ix % 2) of the input; with
    up 2 the 4 children of a source pixel are 4 consecutive rows.

    The launch rule makes every tile visit the launch-wide list.  ``exact``: the taps some row of the LAUNCH can use.  The kernel's
    list is cheaper to form: a tap of the class's parity whose offset moves SOME coordinate of [0, last] into the source range on
    each axis, whatever that coordinate's parity.  In a stride-2 class that can keep a tap no row of the class reaches (2x6, 4x4 s2,
    class py = 1: kh = 0 needs iy = 0); such a tap multiplies zeros, so the list may exceed the exact one and never fall short."""
    hs, ws, kh, kw, stride, pad, up = r
    ho, wo = out_size(r)
    launches = []   # (rows, parity class or None)
    if mode == 0:
        launches.append(([fwd_taps(r, oy, ox) for oy in range(ho) for ox in range(wo) for _ in range(n)], None))
    elif stride == 2:
        for py in (0, 1):
            for px in (0, 1):
                launches.append(([dgrad_taps(r, iy, ix) for iy in range(py, hs, 2) for ix in range(px, ws, 2) for _ in range(n)], (py, px)))
    elif up == 2:
        launches.append(([dgrad_taps(r, 2 * sy + cy, 2 * sx + cx) for sy in range(hs) for sx in range(ws) for _ in range(n)
                          for cy in (0, 1) for cx in (0, 1)], None))
    else:
        launches.append(([dgrad_taps(r, iy, ix) for iy in range(hs) for ix in range(ws) for _ in range(n)], None))
    launch_rule = per_tile = exact = 0
    for rows, cls in launches:
        tiles = [rows[i:i + TILE] for i in range(0, len(rows), TILE)]
        used = set().union(*rows)
        listed = used
        if cls is not None:   # the span rule of a stride-2 class
            span = lambda size, out, d: any(0 <= a + d < out * stride for a in range(size))   # noqa: E731
            listed = {(a, b) for a in range(kh) for b in range(kw)
                      if (cls[0] + pad - a) % 2 == 0 and (cls[1] + pad - b) % 2 == 0 and span(hs, ho, pad - a) and span(ws, wo, pad - b)}
            assert used <= listed
        exact += len(tiles) * len(used)
        launch_rule += len(tiles) * len(listed)
        per_tile += sum(len(set().union(*t)) for t in tiles)
    return launch_rule, per_tile, exact


def rect_chunks(lib, r, mode):
    a, b = C.c_int64(-1), C.c_int64(-1)
    g = rect_geom(r)
    rc = lib.otvae_conv_gemm_chunks(C.byref(g), mode, C.byref(a), C.byref(b))
    return rc, a.value, b.value


RECT_IDS = ["%dx%d_k%dx%ds%dp%du%d" % r for r in RECT]


@pytest.mark.parametrize("r", RECT, ids=RECT_IDS)
def test_rectangular_counts_equal_the_row_by_row_count(lib, r):
    for mode in (0, 1):
        rc, launch, tile = rect_chunks(lib, r, mode)
        assert rc == 0, (r, mode)
        want_launch, want_tile, exact = brute_chunks(r, mode)
        assert (launch, tile) == (want_launch, want_tile), (r, mode)
        assert tile <= exact <= launch
        if mode == 0 or r[4] == 1:
            assert launch == exact


def test_rectangular_counts_measured():
    """The brute force itself, pinned on five of the geometries (forward: launch rule, per tile) so that it cannot drift with the library."""
    got = [brute_chunks(r, 0)[:2] for r in (RECT[0], RECT[1], RECT[2], RECT[3], RECT[4])]
    assert got == [(15, 13), (15, 13), (63, 39), (32, 28), (126, 81)]


@pytest.mark.parametrize("r", RECT, ids=RECT_IDS)
def test_rectangular_dead_taps_equal_the_position_by_position_mask(lib, r):
    hs, ws, kh, kw, stride, pad, up = r
    ho, wo = out_size(r)
    used = set().union(*[fwd_taps(r, oy, ox) for oy in range(ho) for ox in range(wo)])
    want = sum(1 << (a * kw + b) for a in range(kh) for b in range(kw) if (a, b) not in used)
    g = rect_geom(r)
    mask = C.c_uint32(0xffffffff)
    assert lib.otvae_conv_dead_taps(C.byref(g), C.byref(mask)) == 0
    assert mask.value == want, (r, bin(mask.value), bin(want))


def test_dead_tap_masks_of_1x4_and_4x1_are_not_transposes_of_each_other(lib):
    m = {}
    for r in (RECT[0], RECT[1]):
        g = rect_geom(r)
        mask = C.c_uint32(0)
        assert lib.otvae_conv_dead_taps(C.byref(g), C.byref(mask)) == 0
        m[r[:2]] = mask.value
    assert m[(1, 4)] == 0b111000111 and m[(4, 1)] == 0b101101101      # bit kh * KW + kw: rows 0 and 2 dead / columns 0 and 2 dead


def ws_queries(lib, g):
    """(return code, error text) of the four host-only entry points that see a geometry first."""
    from ot_vae_lightning_amd._lib import last_error
    a, b, m = C.c_int(0), C.c_int(0), C.c_uint32(0)
    calls = {"fwd_stats_ws": lambda: lib.otvae_conv_fwd_stats_ws(C.byref(g), C.byref(a), C.byref(b)),
             "bwd_data_ws": lambda: lib.otvae_conv_bwd_data_ws(C.byref(g), C.byref(a), C.byref(b)),
             "bwd_weight_ws": lambda: lib.otvae_conv_bwd_weight_ws(C.byref(g), 1, C.byref(a)),
             "dead_taps": lambda: lib.otvae_conv_dead_taps(C.byref(g), C.byref(m))}
    out = {}
    for entry, call in calls.items():
        rc = call()
        out[entry] = (rc, last_error() if rc else "")
    return out


EINVAL = -1   # OTVAE_EINVAL (include/otvae.h)


def test_geometry_refusals(lib):
    from ot_vae_lightning_amd._lib import ConvGeom
    # fields: N, Hs, Ws, Cs, up, Ho, Wo, Cn, KH, KW, stride, pad
    refused = {
        "pad = -1 (6x10, 3x3 -> 2x6, consistent with the formula)": ConvGeom(4, 6, 10, 8, 1, 2, 6, 8, 3, 3, 1, -1),
        "Ho = -1 (1x5 map, 3x3, pad 0)": ConvGeom(4, 1, 5, 8, 1, -1, 3, 8, 3, 3, 1, 0),
        "Ho = 0 (2x5 map, 3x3, pad 0)": ConvGeom(4, 2, 5, 8, 1, 0, 3, 8, 3, 3, 1, 0),
        "Wo = 0 (5x2 map, 3x3, pad 0)": ConvGeom(4, 5, 2, 8, 1, 3, 0, 8, 3, 3, 1, 0),
        "Wo = -2 (6x2 map, 1x5, pad 0)": ConvGeom(4, 6, 2, 8, 1, 6, -2, 8, 1, 5, 1, 0),
        "stride 2 with odd Ws only": ConvGeom(4, 6, 9, 8, 1, 3, 4, 8, 4, 4, 2, 1),
        "stride 2 with odd Hs only": ConvGeom(4, 9, 6, 8, 1, 4, 3, 8, 4, 4, 2, 1),
        "Ho / Wo swapped on a 6x10 map": ConvGeom(4, 6, 10, 8, 1, 10, 6, 8, 3, 3, 1, 1),
        "KH / KW swapped sizes (3x5 kernel, output of 5x3)": ConvGeom(4, 6, 10, 8, 1, 4, 10, 8, 3, 5, 1, 1),
    }
    for what, g in refused.items():
        for entry, (rc, err) in ws_queries(lib, g).items():
            assert rc == EINVAL, (what, entry, rc)
            assert "otvae_conv_" + entry in err, (what, entry, err)
    accepted = {
        "pad = 3 with 3x3 on 6x10 -> 10x14": ConvGeom(4, 6, 10, 8, 1, 10, 14, 8, 3, 3, 1, 3),
        "pad = 0 with 3x3 on 3x5 -> 1x3": ConvGeom(4, 3, 5, 8, 1, 1, 3, 8, 3, 3, 1, 0),
        "3x5 kernel on 6x10 -> 6x8": ConvGeom(4, 6, 10, 8, 1, 6, 8, 8, 3, 5, 1, 1),
    }
    for what, g in accepted.items():
        for entry, (rc, err) in ws_queries(lib, g).items():
            assert rc == 0, (what, entry, rc, err)
