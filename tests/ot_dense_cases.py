"""Case tables, input builders, fp64 truths and bound functions shared by ``test_ot_dense_host.py`` and ``test_gpu_ot_dense.py``
(no tests here): the dense helpers of the Gaussian OT path in ``csrc/gaussian_ot.hip`` and ``csrc/mvn.hip``, each kernel on its
own.  Pure torch / numpy on the CPU.  Every shape is named for the loop or branch of the kernel it enters; every bound is derived
from the arithmetic (u = 2^-53, or 2^-24 for fp32) or is a tolerance the suite already holds the same kernel to.  Nothing here
comes from a measured HIP number.  Builders are cached per process: callers must not modify what they get."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -53
U32 = 2.0 ** -24
F64 = torch.float64
INF, NAN = float("inf"), float("nan")


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(shape, seed, dtype=F64):
    """standard normal in fp64, rounded to ``dtype``: the fp32 operands are exactly representable in the fp64 truth"""
    return torch.randn(shape, generator=gen(seed), dtype=F64).to(dtype)


def worst_ratio(got, truth, bound):
    """max |got - truth| / bound, element-wise (inf if anything is not finite)"""
    g, t = got.detach().double().cpu(), truth.detach().double().cpu()
    assert g.shape == t.shape, (g.shape, t.shape)
    r = ((g - t).abs() / bound).max().item()
    return r if math.isfinite(r) else INF


def rel_to_max(got, truth):
    """max |got - truth| / max |truth|: the metric of the suite's softmax / log-density tolerances"""
    g, t = got.detach().double().cpu(), truth.detach().double().cpu()
    assert g.shape == t.shape, (g.shape, t.shape)
    r = (g - t).abs().max().item() / max(t.abs().max().item(), 1e-300)
    return r if math.isfinite(r) else INF


# ======================================================================================================== 1. otvae_cholesky
# D <= 128: the one-workgroup left-looking kernel -- one column / two / around one wave (63, 64, 65) / around the 128-thread half
# of its 256-stride (127) / its last size (128).  D > 128: panels of 64 columns and 64 x 64 SYRK tiles -- 129: a one-row trailing
# block; 130; 191: ragged third panel of 63; 192: a full last panel; 193: a last panel of ONE column; 200; 256: four full panels;
# 257, 320: two SYRK tile rows, the second ragged (1 and 64 rows) and five panels.
CHOL_SMALL = (1, 2, 63, 64, 65, 127, 128)
CHOL_BLOCKED = (129, 130, 191, 192, 193, 200, 256, 257, 320)
CHOL_BAD = {128: (0, 5, 63, 64, 127), 200: (0, 63, 64, 130, 199)}   # D -> pivots made negative


@functools.lru_cache(maxsize=None)
def chol_batch(D):
    """[3, D, D] symmetric positive definite: (a) X^T X / n + 0.1 I with X [3 D + 1, D]; (b) Q diag(logspace(0, -8, D)) Q^T,
    symmetrised (condition 1e8: smallest pivots 1e8 x the rounding level); (c) = 1e6 (a): scale must not matter"""
    n = 3 * D + 1
    x = randn((n, D), 1000 + D)
    a = x.T @ x / n + 0.1 * torch.eye(D, dtype=F64)
    a = 0.5 * (a + a.T)
    q = torch.linalg.qr(randn((D, D), 2000 + D))[0]
    b = q @ torch.diag(torch.logspace(0, -8, D, dtype=F64)) @ q.T
    b = 0.5 * (b + b.T)
    return torch.stack([a, b, 1e6 * a])


def chol_kernel_input(A):
    """what the kernel is handed: the lower triangle, NaN in the strict upper one (it must not be read, like torch.linalg.cholesky)"""
    upper = torch.ones(A.shape[-2:], dtype=torch.bool).triu(1)
    return A.masked_fill(upper, NAN).contiguous()


def chol_bound(A):
    """|L L^T - A|_ij <= 3 (D + 1) u sqrt(a_ii a_jj): one share for Higham's backward bound of a Cholesky factorisation whose sums
    run in ANY order (gamma_{D+1} (|L| |L^T|)_ij, and Cauchy-Schwarz on the rows of L gives (|L| |L^T|)_ij <= sqrt(a_ii a_jj) up to
    the same relative term), one for forming the product in fp64 here, one for the second-order terms"""
    D = A.shape[-1]
    d = A.diagonal(dim1=-2, dim2=-1)
    return 3.0 * (D + 1) * U * torch.sqrt(d.unsqueeze(-1) * d.unsqueeze(-2))


def chol_residual_ratio(L, A):
    """max |L L^T - A| / chol_bound(A) per matrix, product in fp64 on the CPU"""
    L = L.detach().double().cpu()
    r = ((L @ L.transpose(-1, -2) - A).abs() / chol_bound(A)).flatten(-2).max(-1).values
    return torch.where(torch.isfinite(r), r, torch.full_like(r, INF))


def chol_is_lower_positive(L):
    L = L.detach().cpu()
    return bool((L.triu(1) == 0).all()) and bool((L.diagonal(dim1=-2, dim2=-1) > 0).all())


@functools.lru_cache(maxsize=None)
def chol_bad_case(D, p):
    """batch [(b), (a) with pivot p made -1, (c)], torch's factor L0 of the UNMODIFIED (a), and the info the call must report:
    A[p][p] = sum_{k<p} L0[p][k]^2 - 1, so the p-th pivot is -1 to rounding, far from the decision at 0"""
    A = chol_batch(D).clone()
    a = A[0].clone()
    L0 = torch.linalg.cholesky(a)
    bad = a.clone()
    bad[p, p] = (L0[p, :p] ** 2).sum() - 1.0
    return dict(A=torch.stack([A[1], bad, A[2]]), L0=L0, a=a, info=[0, p + 1, 0])


def chol_right_looking(a):
    """an independent fp64 factor with the sums in another order (outer-product form): what a correct kernel may differ from torch by"""
    a = a.clone()
    D = a.shape[0]
    L = torch.zeros_like(a)
    for j in range(D):
        L[j, j] = math.sqrt(a[j, j].item())
        L[j + 1:, j] = a[j + 1:, j] / L[j, j]
        a[j + 1:, j + 1:] -= torch.outer(L[j + 1:, j], L[j + 1:, j])
    return L


# ======================================================================================================== 2. otvae_gemm_f64 / _f32
# (nb, m, n, k).  The fp64 entry takes the MFMA kernel (64 x 64 tiles, K chunks of 16, steps of 4) at max(m, n) >= 256 and k >= 64,
# the 16 x 16 tile kernel otherwise; the fp32 entry always the tile kernel.
GEMM_SHAPES = [(1, 1, 1, 1),          # one element
               (2, 17, 33, 15),       # tile kernel: ragged tiles in m and n, k short of one chunk
               (1, 255, 255, 64),     # tile kernel just under the MFMA line in m and n
               (1, 256, 1, 63),       # k under the line
               (1, 256, 1, 64),       # MFMA, one column
               (1, 1, 256, 64),       # MFMA, one row
               (3, 257, 65, 67),      # MFMA: ragged in m, n and k, k no multiple of 4
               (2, 300, 130, 70)]
GEMM_SCALARS = [(1.0, 0.0), (-0.75, 0.5)]
GEMM_BCAST = ("none", "A", "B")


def gemm_uses_mfma(m, n, k):
    return max(m, n) >= 256 and k >= 64


def gemm_combos(nb):
    return [(ta, tb, al, be, bc) for ta in (0, 1) for tb in (0, 1) for al, be in GEMM_SCALARS
            for bc in (GEMM_BCAST if nb > 1 else GEMM_BCAST[:1])]


@functools.lru_cache(maxsize=None)
def gemm_operands(shape, dtype):
    """A [nb, m, k], B [nb, k, n] in their logical (untransposed) orientation and the seeded prefill C0 [nb, m, n]"""
    nb, m, n, k = shape
    seed = 3000 + 7 * GEMM_SHAPES.index(shape)
    return randn((nb, m, k), seed, dtype), randn((nb, k, n), seed + 1, dtype), randn((nb, m, n), seed + 2, dtype)


def gemm_case(shape, dtype, ta, tb, alpha, beta, bcast):
    """(A as stored, B as stored, C0, truth, E): stored operands are [m, k] / [k, m] ([k, n] / [n, k]) row-major per the trans flag,
    with a leading batch of 1 for a shared operand; truth = alpha op(A) op(B) + beta C0 and E = |alpha| |op(A)| |op(B)| + |beta| |C0|
    in fp64"""
    A, B, C0 = gemm_operands(shape, dtype)
    if bcast == "A":
        A = A[:1]
    if bcast == "B":
        B = B[:1]
    a64, b64, c64 = A.double(), B.double(), C0.double()
    truth = alpha * (a64 @ b64) + beta * c64
    E = abs(alpha) * (a64.abs() @ b64.abs()) + abs(beta) * c64.abs()
    As = A.transpose(1, 2).contiguous() if ta else A.contiguous()
    Bs = B.transpose(1, 2).contiguous() if tb else B.contiguous()
    return As, Bs, C0, truth, E


def gemm_bound(E, k, dtype):
    """fp64: 2 (k + 4) u E -- one share for the kernel's k fused adds and its epilogue (alpha, beta, the sum), one for the
    reference's own evaluation.  fp32 against the fp64 truth: (k + 4) 2^-24 E, the kernel's share alone."""
    return (2.0 * (k + 4) * U if dtype == F64 else (k + 4) * U32) * E + 1e-300


def gemm_truth_longdouble(A, B, C0, alpha, beta):
    """the same value in numpy.longdouble (64-bit mantissa on x86): what torch's own fp64 product is measured against on the host"""
    a, b, c = (t.double().numpy().astype(np.longdouble) for t in (A, B, C0))
    return np.longdouble(alpha) * np.matmul(a, b) + np.longdouble(beta) * c


# ======================================================================================================== 3. row softmax / logsumexp
# (rows, K): a wave per row, lanes stride K by 64, four rows per workgroup -- one element / one short of, exactly and one over the
# 64-lane stride with rows short of, on and over one workgroup / 257 workgroups with a ragged last one, K = 2 strides + 2 / 16 strides
ROWS_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (1027, 130), (7, 1024)]
SOFTMAX_SCALES = [1.0, 1 / 0.3, 0.05]
ROWS_TOL = {torch.float32: 2e-6, F64: 1e-13}    # tests/test_gpu_parity.py::test_library_matmul_and_row_softmax_vs_float64
ROWS_GRAD_FACTOR = 5.0


@functools.lru_cache(maxsize=None)
def rows_input(shape, dtype, wide=False):
    """x = 3 randn, or (wide) rows that span [-1e4, 1e4] -- half of the entries within a few units of 1e4, so that the result is
    no one-hot row, the rest uniform over [-1e4, 0], both ends present where K >= 2: exp(x) overflows fp32 (and fp64) unless the
    row maximum is subtracted first.  The wide case is run at scale 1: there x - max is exact in either precision
    for every entry that matters (Sterbenz), so the suite's tolerance applies to it unchanged."""
    rows, K = shape
    seed = 4000 + 10 * ROWS_SHAPES.index(shape) + (5 if wide else 0)
    if not wide:
        x = 3.0 * randn((rows, K), seed)
    else:
        x = -1e4 * torch.rand((rows, K), generator=gen(seed), dtype=F64)
        x[:, ::2] = 1e4 - 3.0 * randn((rows, K), seed + 3).abs()[:, ::2]     # every other entry within a few units of the top
        if K >= 2:
            x[:, K // 3], x[:, K - 1] = 1e4, -1e4
    return x.to(dtype), randn((rows, K), seed + 1, dtype), randn((rows,), seed + 2, dtype)


def softmax_truth(x, scale, gy):
    xr = x.double().requires_grad_(True)
    y = torch.softmax(xr * scale, dim=-1)
    (gx,) = torch.autograd.grad(y, xr, gy.double())
    return y.detach(), gx


def lse_truth(x, g):
    xr = x.double().requires_grad_(True)
    out = torch.logsumexp(xr, dim=-1)
    (gx,) = torch.autograd.grad(out, xr, g.double())
    return out.detach(), gx


def lse_bwd_truth(x, lse, g):
    """the backward kernel's own definition, gx = g exp(x - lse), in fp64 from the operands AS HANDED to it.  For the wide fp32 rows:
    there |lse| ~ 1e4 carries an fp32 rounding of 2^-24 |lse| = 6e-4, which every exp(x - lse) inherits -- torch's own fp32
    gradient is 6e-5 of max |truth| away from the fp64 autograd gradient (asserted on the host), so that truth cannot judge an fp32
    kernel at 1e-5; this one can, and x - lse is exact for every entry that matters."""
    return g.double().unsqueeze(-1) * torch.exp(x.double() - lse.double().unsqueeze(-1))


# rows of specials, K in (3, 65, 130): the special entry sits in the first stride / alone in the second / in the third.
SPECIAL_K = (3, 65, 130)
LSE_SPECIAL_ROWS = ("all -inf", "some -inf", "+inf among finite", "nan among finite", "finite")
SOFTMAX_SPECIAL_ROWS = ("all -inf", "some -inf", "finite")


@functools.lru_cache(maxsize=None)
def special_rows(K, kinds, dtype):
    """one row per kind (five rows: over the four-rows-per-workgroup edge); the special entry of a row is at index 1 (K = 3) or K - 1"""
    x = randn((len(kinds), K), 4900 + K)
    at = 1 if K == 3 else K - 1
    for r, kind in enumerate(kinds):
        if kind == "all -inf":
            x[r] = -INF
        elif kind == "some -inf":
            x[r, 0] = x[r, at] = -INF
        elif kind == "+inf among finite":
            x[r, at] = INF
        elif kind == "nan among finite":
            x[r, at] = NAN
    return x.to(dtype), randn((len(kinds), K), 4950 + K, dtype), randn((len(kinds),), 4960 + K, dtype), at


def same_specials(got, truth):
    """(positions of NaN and positions AND signs of inf equal torch's, worst error of the finite entries / max |finite truth|)"""
    g, t = got.detach().double().cpu(), truth.detach().double().cpu()
    same = torch.equal(torch.isnan(g), torch.isnan(t)) and torch.equal(g == INF, t == INF) and torch.equal(g == -INF, t == -INF)
    fin = torch.isfinite(t) & torch.isfinite(g)
    if not bool(fin.any()):
        return same, 0.0
    scale = max(t[fin].abs().max().item(), 1e-300)
    return same, (g[fin] - t[fin]).abs().max().item() / scale


# ======================================================================================================== 4. otvae_mvn_logprob_fwd / _bwd
# (nb, B, D) IN THIS ORDER in one process: a full-covariance call needs (D^2 + D) 8 bytes of LDS, over 64 KiB from D = 91
# (91^2 + 91 = 8372 > 8192 >= 8190 = 90^2 + 90), and the entry raises the limit at the first such call -- here between the third case
# and the fourth.  One lane per sample in blocks of 256: B = 255, 256, 257 sit under, on and over the block edge.
MVN_CASES = [(1, 1, 1), (3, 255, 2), (1, 256, 90), (2, 257, 91), (1, 300, 128)]
MVN_TOL, MVN_GRAD_TOL = 1e-11, 1e-10     # tests/test_gpu_parity.py::test_gaussian_model_update_with_autograd
MVN_REFUSED_D = 129


def mvn_lds_bytes(D, diag):
    return ((D if diag else D * D) + D) * 8


@functools.lru_cache(maxsize=None)
def mvn_inputs(case, diag):
    """x, mean, L (or sigma for diag), g: L has its diagonal in [0.5, 2] and strict lower entries randn 0.3 / sqrt(D)"""
    nb, B, D = case
    seed = 5000 + 10 * MVN_CASES.index(case) + int(diag)
    dg = 0.5 + 1.5 * torch.rand((nb, D), generator=gen(seed), dtype=F64)
    mean = randn((nb, D), seed + 1)
    x = mean.unsqueeze(1) + 1.5 * randn((nb, B, D), seed + 2)
    g = randn((nb, B), seed + 3)
    if diag:
        return x, mean, dg, g
    L = (randn((nb, D, D), seed + 4) * (0.3 / math.sqrt(D))).tril(-1) + torch.diag_embed(dg)
    return x, mean, L, g


@functools.lru_cache(maxsize=None)
def mvn_truth(case, diag):
    """torch.distributions in fp64 under autograd: lp, the whitened y, and the gradients of sum(g lp) w.r.t. x, mean and L / sigma"""
    import torch.distributions as TD
    x, mean, L, g = mvn_inputs(case, diag)
    xr, mr, Lr = (t.clone().requires_grad_(True) for t in (x, mean, L))
    if diag:
        dist = TD.Independent(TD.Normal(mr.unsqueeze(-2), Lr.unsqueeze(-2)), 1)
        y = (x - mean.unsqueeze(1)) / L.unsqueeze(1)
    else:
        dist = TD.MultivariateNormal(mr.unsqueeze(-2), scale_tril=Lr.unsqueeze(-3))
        y = torch.linalg.solve_triangular(L, (x - mean.unsqueeze(1)).transpose(1, 2), upper=False).transpose(1, 2)
    lp = dist.log_prob(xr)
    dx, dmean, dL = torch.autograd.grad((lp * g).sum(), (xr, mr, Lr))
    return dict(lp=lp.detach(), y=y, dx=dx, dmean=dmean, dL=dL)


def mvn_caller_side(qg, y, L, g, diag):
    """the formulas of the header of csrc/mvn.hip, which turn the backward kernel's qg_b = g_b L^-T y_b into the gradients:
    d mean = sum_b qg_b, d x_b = -qg_b, d L = tril(sum_b qg_b y_b^T) - (sum_b g_b) diag(1 / L_ii)  (diag: sum_b qg_b y_b - sum_b g_b / sigma)"""
    qg, y = qg.double().cpu(), y.double().cpu()
    gs = g.sum(1)
    if diag:
        dL = (qg * y).sum(1) - gs.unsqueeze(-1) / L
    else:
        dL = (qg.transpose(1, 2) @ y).tril() - torch.diag_embed(gs.unsqueeze(-1) / L.diagonal(dim1=-2, dim2=-1))
    return dict(dx=-qg, dmean=qg.sum(1), dL=dL)


# ======================================================================================================== 5. otvae_apply_transport
# (nb, B, D): one workgroup of 256 threads per sample strides D -- one element / one short of, on and over one stride / four strides, ragged
TRANSPORT_CASES = [(1, 1, 1), (2, 3, 255), (2, 3, 256), (1, 2, 257), (1, 2, 1000)]


@functools.lru_cache(maxsize=None)
def transport_case(case, dtype):
    """x (in ``dtype``), ms, mt, T (fp64), truth = T (x - ms) + mt in fp64 and its bound:
    2 (D + 3) u (|T| |x - ms| + |mt|) -- the kernel's D fused adds, the centring and the shift, and the same again for the evaluation
    here -- plus, for an fp32 result, the one rounding 2^-23 |truth| of tests/test_gpu_norm_act.py::one_rounding"""
    nb, B, D = case
    seed = 6000 + 10 * TRANSPORT_CASES.index(case)
    x = (1.0 + randn((nb, B, D), seed)).to(dtype)
    ms, mt = 1.0 + 0.5 * randn((nb, D), seed + 1), randn((nb, D), seed + 2)
    T = randn((nb, D, D), seed + 3) / math.sqrt(D) + torch.eye(D, dtype=F64)
    xc = x.double() - ms.unsqueeze(1)
    truth = xc @ T.transpose(1, 2) + mt.unsqueeze(1)
    bound = 2.0 * (D + 3) * U * (xc.abs() @ T.abs().transpose(1, 2) + mt.abs().unsqueeze(1))
    if dtype == torch.float32:
        bound = bound + 2.0 ** -23 * truth.abs()
    return dict(x=x, ms=ms, mt=mt, T=T, truth=truth, bound=bound)


# ======================================================================================================== 6. otvae_gauss_stats
# B -> K split B / 64 clamped to [1, 16] and the rows per part: 130 -> 2 parts of 65 rows (four 16-row tiles and one row), 1100 -> 16
# parts of 69, the last of 65.  D + 1 (the augmented [x, 1]) under, on and over one 16-tile and on two: D = 1, 15, 16, 31.
STATS_B = (1, 63, 64, 130, 1024, 1100)
STATS_D = (1, 15, 16, 31)
STATS_KSPLIT = {1: 1, 63: 1, 64: 1, 130: 2, 1024: 16, 1100: 16}
STATS_NB = 2
STATS_MODES = (("overwrite", 0, 0.0), ("sum", 1, -1.0), ("ema", 1, 0.9))   # (name, accumulate, decay)


def stats_ksplit(B):
    return max(1, min(16, B // 64))


@functools.lru_cache(maxsize=None)
def stats_case(B, D, dtype, diag):
    """samples [nb, B, D], a prefilled state (n integer-valued: the counts stay exact) and the fp64 sums with the sums of the
    absolute values of their terms"""
    nb = STATS_NB
    seed = 7000 + 100 * STATS_B.index(B) + 10 * STATS_D.index(D) + int(diag)
    x = (0.5 + randn((nb, B, D), seed)).to(dtype)
    x64 = x.double()
    n = torch.full((nb,), float(B), dtype=F64)
    sx, ax = x64.sum(1), x64.abs().sum(1)
    if diag:
        sxx, axx = (x64 * x64).sum(1), (x64 * x64).sum(1)
    else:
        sxx, axx = x64.transpose(1, 2) @ x64, x64.abs().transpose(1, 2) @ x64.abs()
    old = dict(n=torch.tensor([7.0, 1000.0], dtype=F64), sx=3.0 * randn(sx.shape, seed + 1), sxx=5.0 * randn(sxx.shape, seed + 2))
    return dict(x=x, new=dict(n=n, sx=sx, sxx=sxx), abs=dict(n=n, sx=ax, sxx=axx), old=old)


def stats_truth_and_bound(case, B, accumulate, decay):
    """per output: (truth, bound).  bound = 2 (B + 4) u (sum of |terms| + |old state| in the accumulate modes): B adds (in any order:
    the K split regroups them), the combination with the old state, and the same again for the sums formed here"""
    out = {}
    for key in ("n", "sx", "sxx"):
        s, a, o = case["new"][key], case["abs"][key], case["old"][key]
        if not accumulate:
            truth, mag = s, a
        elif decay < 0:
            truth, mag = o + s, a + o.abs()
        else:
            truth, mag = o * decay + s * (1.0 - decay), a + o.abs()
        out[key] = (truth, 2.0 * (B + 4) * U * mag)
    return out


# ======================================================================================================== 7. otvae_codebook_assign
# (nb, B, K, d): a wave per sample, atoms strided over the 64 lanes, four samples per workgroup.  Samples and atoms are integers in
# [-3, 3]: squared distances are exact integers <= 36 d in fp32 and fp64, equal distances are exact ties, and two different ones
# differ by far more than an fp32 rounding (asserted on the host) -- so idx must equal the fp64 arg-min, first index, for EVERY sample.
CODEBOOK_SHAPES = [(1, 1, 1, 1), (2, 5, 63, 3), (1, 4, 64, 8), (2, 7, 65, 5), (1, 9, 130, 16)]
CODEBOOK_TEMPERATURE = 0.7
NAN_SHAPE = (2, 7, 65, 5)
NAN_SAMPLE = (1, 3, 2)      # problem, sample (not sample 0), component
NAN_ATOM = (0, 7)           # problem, atom


@functools.lru_cache(maxsize=None)
def codebook_case(shape):
    """x [nb, B, d], codebook [nb, K, d] (fp32, integer-valued) with planted exact ties at the minimum: atoms k and k + 64 equal
    (K > 64: both belong to ONE lane's stride) with sample 0 sitting on them, atoms j and j + 1 equal (neighbouring lanes) with the
    last sample on them.  truth: fp64 arg-min of the squared distance, first index."""
    nb, B, K, d = shape
    g = gen(8000 + CODEBOOK_SHAPES.index(shape))
    x = torch.randint(-3, 4, (nb, B, d), generator=g).float()
    cb = torch.randint(-3, 4, (nb, K, d), generator=g).float()
    planted = []
    if K > 64:
        k = K - 65            # 0 at K = 65, 65 at K = 130: the pair (65, 129) is the second and third trip of lane 1
        cb[:, k + 64] = cb[:, k]
        x[:, 0] = cb[:, k]
        planted.append((0, k, k + 64))
    if K >= 2 and B >= 2:
        j = min(K - 2, 2)
        cb[:, j + 1] = cb[:, j]
        x[:, B - 1] = cb[:, j]
        planted.append((B - 1, j, j + 1))
    return dict(x=x, cb=cb, planted=planted, **codebook_truth(x, cb))


def codebook_truth(x, cb):
    d2 = ((x.double().unsqueeze(2) - cb.double().unsqueeze(1)) ** 2).sum(-1)     # [nb, B, K], exact integers
    idx = d2.argmin(-1)                                                          # first index among equals
    enc = torch.gather(cb, 1, idx.unsqueeze(-1).expand(-1, -1, cb.shape[-1]))
    return dict(d2=d2, idx=idx, enc=enc)


def reference_assign(x, cb, temperature):
    """the reference's arithmetic in fp32 torch: argmax(softmax(1 / (cdist + 1e-8) / T)).  Used for the NaN rule only."""
    energy = 1.0 / (torch.cdist(x, cb) + 1e-8)
    return torch.softmax(energy / temperature, dim=-1).argmax(-1)


@functools.lru_cache(maxsize=None)
def codebook_nan_cases():
    """the clean case of NAN_SHAPE and its two poisoned copies, each with the indices the fixed kernel must return: a NaN weight makes
    the reference's softmax row all NaN, whose argmax is 0; everything else keeps its arg-min"""
    base = codebook_case(NAN_SHAPE)
    b, r, c = NAN_SAMPLE
    xs = base["x"].clone()
    xs[b, r, c] = NAN
    idx_s = base["idx"].clone()
    idx_s[b, r] = 0
    pb, k = NAN_ATOM
    cba = base["cb"].clone()
    cba[pb, k, 1] = NAN
    idx_a = base["idx"].clone()
    idx_a[pb] = 0
    return dict(clean=base, sample=dict(x=xs, cb=base["cb"], idx=idx_s), atom=dict(x=base["x"], cb=cba, idx=idx_a))


def kmeans_truth(x, idx, K):
    """counts [nb, K] and sums [nb, K, d] of the one-hot k-means accumulation, members added in increasing sample order (fp32; exact
    on the integer-valued samples)"""
    nb, B, d = x.shape
    counts = torch.zeros(nb, K)
    sums = torch.zeros(nb, K, d)
    for b in range(nb):
        for r in range(B):
            counts[b, idx[b, r]] += 1
            sums[b, idx[b, r]] += x[b, r]
    return counts, sums


def equal_with_nan(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())
