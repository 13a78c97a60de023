"""Inputs and CPU truth shared by ``test_prdc_host.py`` and ``test_gpu_prdc.py`` (no tests here).

Recipes.  ``x = 3 + z W`` with ``z [n, 6]`` standard normal and ``W [6, D] / sqrt(6)`` from a generator seeded by D: a six-dimensional
manifold in D dimensions, post-ReLU-like offsets.  Real: seed 11; fake: seed 12, ``z`` scaled by 0.8 and shifted by 0.4.
  * dyadic -- ``q = round(16 x)`` clamped to +-1023, int64 for the truth, ``q.float() / 16`` for the code.  Products and sums of the
    Gram form fit fp64 with 20 bits to spare at D = 2048, so the code under test must reproduce the int64 truth EXACTLY.
  * lattice -- small integer coordinates: hundreds of exact ``d2 == r2`` ties (they decide ``<=`` against ``<``), duplicates, zero radii.
  * float -- the recipe unquantised in fp32; truth in fp64 by the difference form ``sum (a - b)^2``, with the error bound of the
    Gram form ``e_ij = 2 (D + 4) u (|a|^2 + |b|^2)``, u = 2^-53 (norms and the inner product each err by at most D u times the sums
    of absolute products, which |a|^2 + |b|^2 bounds; forming the result adds a few u).  A radius errs by at most e at the row's
    largest partner norm.
Each case is computed once per process and shared; callers must not modify what they get."""
import functools
import math

import torch

U = 2.0 ** -53
SHAPES = [(4, 5, 1, 3), (33, 33, 70, 3), (65, 40, 96, 5), (130, 97, 2048, 3), (257, 257, 96, 5), (257, 130, 2048, 16), (1025, 300, 32, 5)]
# the smallest rows at which a workgroup of otvae_knn_sq_radii walks more than one column tile: 23 row strips, 12 groups
WALK_SHAPE = (2817, 200, 8, 5)


def _manifold(n, d, seed, scale=1.0, shift=0.0):
    w = torch.randn(6, d, generator=torch.Generator().manual_seed(d), dtype=torch.float64) / math.sqrt(6.0)
    z = torch.randn(n, 6, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return 3.0 + (scale * z + shift) @ w


def _pair(n, m, d):
    return _manifold(n, d, 11), _manifold(m, d, 12, scale=0.8, shift=0.4)


def _quantise(x):
    return torch.round(16.0 * x).clamp_(-1023, 1023).to(torch.int64)


def _int_sq_dists(a, b):
    return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * (a @ b.T)


def _diff_sq_dists(a, b):
    """fp64, the difference form, in row blocks"""
    rows = max(1, (1 << 23) // (b.shape[0] * a.shape[1]))
    return torch.cat([((a[lo:lo + rows, None, :] - b[None, :, :]) ** 2).sum(-1) for lo in range(0, a.shape[0], rows)])


def _radii(d, k):
    d = d.clone()
    big = torch.iinfo(torch.int64).max if d.dtype == torch.int64 else float("inf")
    d.fill_diagonal_(big)                                            # self, by index: duplicates stay
    return d.sort(dim=1).values[:, k - 1]


def truth(d_rr, d_ff, d_rf, k, strict=False):
    """every per-row output and the four values from the three distance blocks (int64 or float64)"""
    n, m = d_rf.shape
    r_real, r_fake = _radii(d_rr, k), _radii(d_ff, k)
    inside = (lambda a, b: a < b) if strict else (lambda a, b: a <= b)
    count_fake = inside(d_rf, r_real[:, None]).sum(0)
    hit_real = inside(d_rf, r_fake[None, :]).any(1)
    min_real = d_rf.min(1).values
    return dict(r_real=r_real, r_fake=r_fake, count_fake=count_fake, hit_real=hit_real, min_real=min_real,
                precision=int((count_fake > 0).sum()) / m, recall=int(hit_real.sum()) / n, density=int(count_fake.sum()) / (k * m),
                coverage=int(inside(min_real, r_real).sum()) / n)


def _integer_case(qr, qf, k, scale):
    t = truth(_int_sq_dists(qr, qr), _int_sq_dists(qf, qf), _int_sq_dists(qr, qf), k)
    strict = truth(_int_sq_dists(qr, qr), _int_sq_dists(qf, qf), _int_sq_dists(qr, qf), k, strict=True)
    for key in ("r_real", "r_fake", "min_real"):
        t[key] = t[key].double() / scale ** 2                        # exact
    ties = int((_int_sq_dists(qr, qf) == _radii(_int_sq_dists(qr, qr), k)[:, None]).sum())
    return dict(real=qr.float() / scale, fake=qf.float() / scale, k=k, truth=t, strict=strict, ties=ties)


@functools.lru_cache(maxsize=None)
def dyadic(n, m, d, k):
    xr, xf = _pair(n, m, d)
    return _integer_case(_quantise(xr), _quantise(xf), k, 16)


@functools.lru_cache(maxsize=None)
def lattice(which):
    """"ties": {-2 .. 2}^4, 130 and 97 rows, k = 3;  "duplicates": {-1, 0, 1}^3, 130 and 97 rows over 27 points, k = 3"""
    if which == "ties":
        g = torch.Generator().manual_seed(5)
        qr, qf = torch.randint(-2, 3, (130, 4), generator=g), torch.randint(-2, 3, (97, 4), generator=g)
    else:
        g = torch.Generator().manual_seed(6)
        qr, qf = torch.randint(-1, 2, (130, 3), generator=g), torch.randint(-1, 2, (97, 3), generator=g)
    return _integer_case(qr, qf, 3, 1)


@functools.lru_cache(maxsize=None)
def floating(n, m, d, k):
    """fp32 features, fp64 difference-form truth, the Gram form's error bounds and the smallest decision margin over the bound"""
    xr, xf = _pair(n, m, d)
    real, fake = xr.float(), xf.float()
    r64, f64 = real.double(), fake.double()
    d_rf = _diff_sq_dists(r64, f64)
    t = truth(_diff_sq_dists(r64, r64), _diff_sq_dists(f64, f64), d_rf, k)
    nr, nf = (r64 * r64).sum(1), (f64 * f64).sum(1)
    c = 2.0 * (d + 4) * U
    e_rf = c * (nr[:, None] + nf[None, :])
    e_r_real, e_r_fake = c * (nr + nr.max()), c * (nf + nf.max())
    margin = torch.minimum(((d_rf - t["r_real"][:, None]).abs() / (4 * (e_rf + e_r_real[:, None]))).min(),
                           ((d_rf - t["r_fake"][None, :]).abs() / (4 * (e_rf + e_r_fake[None, :]))).min())
    return dict(real=real, fake=fake, k=k, truth=t, e_r_real=e_r_real, e_r_fake=e_r_fake, e_min_real=c * (nr + nf.max()),
                margin=float(margin))
