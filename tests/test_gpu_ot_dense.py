"""GPU: the dense helpers of the Gaussian OT path, each kernel on its own through its raw entry point against an fp64 truth computed on
the host -- ``otvae_cholesky`` (both implementations, ``info`` included), ``otvae_gemm_f64 / _f32`` (both kernels, all layouts,
alpha / beta / broadcast), the row softmax and logsumexp pairs with their +-inf / NaN rows, ``otvae_mvn_logprob_fwd / _bwd`` across
the 64 KiB LDS switch, ``otvae_apply_transport``, ``otvae_gauss_stats`` and ``otvae_codebook_assign`` (csrc/gaussian_ot.hip,
csrc/mvn.hip).  Cases, truths and bounds live in ``ot_dense_cases.py``; ``test_ot_dense_host.py`` asserts, without a GPU, the
conditions they rest on and that the reference arithmetic alone meets every bound.  Each figure is printed before it is asserted."""
import pytest
import torch

import ot_dense_cases as C

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
DTYPES = [F32, F64]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ot_vae_lightning_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def MU():
    from ot_vae_lightning_amd.ot import matrix_utils
    return matrix_utils


def _L():
    from ot_vae_lightning_amd import _lib
    return _lib


def dev(t):
    return t.contiguous().cuda()


def code(dtype):
    return int(dtype == F64)


# ---------------------------------------------------------------------------------------------------------------- 1. otvae_cholesky
def _cholesky(lib, A):
    """raw entry on the lower triangle of A [nb, D, D] (NaN above it); L and info start from values the kernel never produces"""
    L_ = _L()
    a = dev(C.chol_kernel_input(A))
    nb, D = a.shape[0], a.shape[-1]
    out = torch.full_like(a, 7.0)
    info = torch.full((nb,), -1, dtype=torch.int32, device="cuda")
    L_.check(lib.otvae_cholesky(L_.ptr(a), nb, D, L_.ptr(out), L_.ptr(info), L_.stream()), "otvae_cholesky")
    return out.cpu(), info.cpu().tolist(), a


@pytest.mark.parametrize("D", C.CHOL_SMALL + C.CHOL_BLOCKED)
def test_cholesky_factor(lib, D):
    A = C.chol_batch(D)
    L, info, _ = _cholesky(lib, A)
    ratio = C.chol_residual_ratio(L, A)
    print(f"[ot_dense] cholesky D={D}: info {info}, |L L^T - A| / bound per matrix {ratio.tolist()}")
    assert info == [0, 0, 0]
    assert C.chol_is_lower_positive(L)          # strict upper triangle exactly 0, diagonal > 0
    assert float(ratio.max()) <= 1.0


@pytest.mark.parametrize("D,p", [(D, p) for D, ps in C.CHOL_BAD.items() for p in ps])
def test_cholesky_reports_the_first_bad_pivot(lib, MU, D, p):
    case = C.chol_bad_case(D, p)
    A = case["A"]
    L, info, a_dev = _cholesky(lib, A)
    good = C.chol_residual_ratio(L[[0, 2]], A[[0, 2]])
    cols = C.worst_ratio(L[1][:, :p], case["L0"][:, :p], C.chol_bound(case["a"])[:, :p]) if p else 0.0
    print(f"[ot_dense] cholesky D={D} bad pivot {p}: info {info}, neighbours {good.tolist()} of the bound, columns < p vs torch "
          f"{cols:.3f} of the bound, L[p][p] = {float(L[1, p, p])}")
    assert info == case["info"]
    assert C.chol_is_lower_positive(L[[0, 2]]) and float(good.max()) <= 1.0
    assert cols <= 1.0 and bool(torch.isfinite(L[1][:, :p]).all())
    assert bool(torch.isnan(L[1, p, p]))
    # the public route (info = NULL): NaN in the bad matrix only, the neighbours are the same bits
    Lw = MU.cholesky(a_dev).cpu()
    assert bool(torch.isnan(Lw[1]).any()) and bool(torch.isnan(Lw[1, p, p]))
    assert torch.equal(Lw[0], L[0]) and torch.equal(Lw[2], L[2])


# ---------------------------------------------------------------------------------------------------------------- 2. otvae_gemm_f64 / _f32
def _gemm(lib, dtype, ta, tb, shape, alpha, As, Bs, beta, Cd):
    L_ = _L()
    nb, m, n, k = shape
    fn, name = (lib.otvae_gemm_f64, "otvae_gemm_f64") if dtype == F64 else (lib.otvae_gemm_f32, "otvae_gemm_f32")
    a_b = int(As is not None and As.shape[0] == 1 and nb > 1)
    b_b = int(Bs is not None and Bs.shape[0] == 1 and nb > 1)
    L_.check(fn(ta, tb, nb, m, n, k, alpha, L_.ptr(As), a_b, L_.ptr(Bs), b_b, beta, L_.ptr(Cd), L_.stream()), name)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", C.GEMM_SHAPES, ids=str)
def test_gemm(lib, shape, dtype):
    nb, m, n, k = shape
    worst, where = 0.0, None
    for ta, tb, alpha, beta, bcast in C.gemm_combos(nb):
        As, Bs, C0, truth, E = C.gemm_case(shape, dtype, ta, tb, alpha, beta, bcast)
        Ad, Bd, Cd = dev(As), dev(Bs), dev(C0).clone()
        _gemm(lib, dtype, ta, tb, shape, alpha, Ad, Bd, beta, Cd)
        got = Cd.cpu()
        r = C.worst_ratio(got, truth, C.gemm_bound(E, k, dtype))
        if r > worst:
            worst, where = r, (ta, tb, alpha, beta, bcast)
        if beta == 0.0:   # beta == 0 overwrites C without reading it
            Cn = torch.full_like(Cd, C.NAN)
            _gemm(lib, dtype, ta, tb, shape, alpha, Ad, Bd, beta, Cn)
            assert bool(torch.isfinite(Cn).all()), (shape, ta, tb, bcast, "NaN-prefilled C leaks into the result at beta = 0")
            assert torch.equal(Cn.cpu(), got)
    mfma = dtype == F64 and C.gemm_uses_mfma(m, n, k)
    print(f"[ot_dense] gemm {dtype} {shape} ({'mfma' if mfma else 'tile'} kernel): worst |got - truth| / bound {worst:.3f} at "
          f"(transA, transB, alpha, beta, shared) = {where}")
    assert worst <= 1.0, (shape, dtype, worst, where)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_mm_wrapper(MU, dtype):
    """``matrix_utils.mm`` on the MFMA-sized case, batched and with a shared 2-D operand"""
    shape = (3, 257, 65, 67)
    for bcast in ("none", "B"):
        As, Bs, _, truth, E = C.gemm_case(shape, dtype, 0, 0, 1.0, 0.0, bcast)
        out = MU.mm(dev(As), dev(Bs[0] if bcast == "B" else Bs))
        assert out.dtype == dtype and out.shape == truth.shape
        r = C.worst_ratio(out, truth, C.gemm_bound(E, shape[3], dtype))
        print(f"[ot_dense] mm {dtype} {shape} shared={bcast}: {r:.3f} of the bound")
        assert r <= 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_gemm_refusals(lib, dtype):
    shape = (2, 17, 33, 15)
    As, Bs, C0, _, _ = C.gemm_case(shape, dtype, 0, 0, 1.0, 0.0, "none")
    Ad, Bd, Cd = dev(As), dev(Bs), dev(C0).clone()
    for zero in range(4):
        bad = tuple(0 if i == zero else v for i, v in enumerate(shape))
        with pytest.raises(ValueError):
            _gemm(lib, dtype, 0, 0, bad, 1.0, Ad, Bd, 0.0, Cd)
    for a, b in ((None, Bd), (Ad, None)):
        with pytest.raises(ValueError):
            _gemm(lib, dtype, 0, 0, shape, 1.0, a, b, 0.0, Cd)
    with pytest.raises(ValueError):
        _gemm(lib, dtype, 0, 0, shape, 1.0, Ad, Bd, 0.0, None)
    assert torch.equal(Cd.cpu(), C0)


# ---------------------------------------------------------------------------------------------------------------- 3. rows
def _softmax(lib, x, scale, gy):
    """raw forward, then the raw backward on the forward's own output"""
    L_ = _L()
    rows, K = x.shape
    xd, gyd = dev(x), dev(gy)
    y, gx = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    L_.check(lib.otvae_softmax_rows(code(x.dtype), L_.ptr(xd), rows, K, scale, L_.ptr(y), L_.stream()), "otvae_softmax_rows")
    L_.check(lib.otvae_softmax_rows_bwd(code(x.dtype), L_.ptr(y), L_.ptr(gyd), rows, K, scale, L_.ptr(gx), L_.stream()),
             "otvae_softmax_rows_bwd")
    return y.cpu(), gx.cpu()


def _lse(lib, x, g):
    L_ = _L()
    rows, K = x.shape
    xd, gd = dev(x), dev(g)
    out, gx = torch.full((rows,), 7.0, dtype=x.dtype, device="cuda"), torch.full_like(xd, 7.0)
    L_.check(lib.otvae_lse_rows(code(x.dtype), L_.ptr(xd), rows, K, L_.ptr(out), L_.stream()), "otvae_lse_rows")
    L_.check(lib.otvae_lse_rows_bwd(code(x.dtype), L_.ptr(xd), L_.ptr(out), L_.ptr(gd), rows, K, L_.ptr(gx), L_.stream()),
             "otvae_lse_rows_bwd")
    return out.cpu(), gx.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", C.ROWS_SHAPES, ids=str)
def test_softmax_rows(lib, shape, dtype):
    tol = C.ROWS_TOL[dtype]
    for wide, scale in [(False, s) for s in C.SOFTMAX_SCALES] + [(True, 1.0)]:
        x, gy, _ = C.rows_input(shape, dtype, wide)
        y, gx = _softmax(lib, x, scale, gy)
        ty, tgx = C.softmax_truth(x, scale, gy)
        ey, eg = C.rel_to_max(y, ty), C.rel_to_max(gx, tgx)
        print(f"[ot_dense] softmax {dtype} {shape} scale {scale:.3g}{' wide' if wide else ''}: y {ey:.2e} (tol {tol:.0e}), "
              f"dx {eg:.2e} (tol {C.ROWS_GRAD_FACTOR * tol:.0e})")
        assert y.dtype == dtype and ey <= tol and eg <= C.ROWS_GRAD_FACTOR * tol, (shape, dtype, scale, wide, ey, eg)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("shape", C.ROWS_SHAPES, ids=str)
def test_lse_rows(lib, shape, dtype):
    tol = C.ROWS_TOL[dtype]
    for wide in (False, True):
        x, _, g = C.rows_input(shape, dtype, wide)
        out, gx = _lse(lib, x, g)
        tout, tgx = C.lse_truth(x, g)
        if wide:   # the backward's own definition from the operands it was handed (ot_dense_cases.lse_bwd_truth says why)
            tgx = C.lse_bwd_truth(x, out, g)
        eo, eg = C.rel_to_max(out, tout), C.rel_to_max(gx, tgx)
        print(f"[ot_dense] lse {dtype} {shape}{' wide' if wide else ''}: out {eo:.2e} (tol {tol:.0e}), dx {eg:.2e} "
              f"(tol {C.ROWS_GRAD_FACTOR * tol:.0e})")
        assert out.dtype == dtype and eo <= tol and eg <= C.ROWS_GRAD_FACTOR * tol, (shape, dtype, wide, eo, eg)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("K", C.SPECIAL_K)
def test_rows_with_inf_and_nan(lib, K, dtype):
    """positions and signs of inf / NaN equal torch's, forward and backward; the finite entries stay within tolerance"""
    tol = C.ROWS_TOL[dtype]
    x, _, g, _ = C.special_rows(K, C.LSE_SPECIAL_ROWS, dtype)
    out, gx = _lse(lib, x, g)
    tout, tgx = C.lse_truth(x, g)
    for name, got, want, t in (("lse", out, tout, tol), ("lse dx", gx, tgx, C.ROWS_GRAD_FACTOR * tol)):
        same, err = C.same_specials(got, want)
        print(f"[ot_dense] special rows K={K} {dtype} {name}: masks equal {same}, finite entries {err:.2e} (tol {t:.0e})")
        assert same, (name, K, dtype, got, want)
        assert err <= t
    x, gy, _, _ = C.special_rows(K, C.SOFTMAX_SPECIAL_ROWS, dtype)
    scale = 1 / 0.3
    y, gx = _softmax(lib, x, scale, gy)
    ty, tgx = C.softmax_truth(x, scale, gy)
    for name, got, want, t in (("softmax", y, ty, tol), ("softmax dx", gx, tgx, C.ROWS_GRAD_FACTOR * tol)):
        same, err = C.same_specials(got, want)
        print(f"[ot_dense] special rows K={K} {dtype} {name}: masks equal {same}, finite entries {err:.2e} (tol {t:.0e})")
        assert same, (name, K, dtype, got, want)
        assert err <= t


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_rows_wrappers(MU, dtype):
    """``matrix_utils.softmax_rows`` / ``lse_rows`` under autograd, at the stride edge"""
    tol = C.ROWS_TOL[dtype]
    x, gy, g = C.rows_input((5, 65), dtype)
    xd = dev(x).requires_grad_(True)
    y = MU.softmax_rows(xd, 1 / 0.3)
    (gx,) = torch.autograd.grad(y, xd, dev(gy))
    ty, tgx = C.softmax_truth(x, 1 / 0.3, gy)
    assert C.rel_to_max(y, ty) <= tol and C.rel_to_max(gx, tgx) <= C.ROWS_GRAD_FACTOR * tol
    out = MU.lse_rows(xd)
    (gx,) = torch.autograd.grad(out, xd, dev(g))
    tout, tgx = C.lse_truth(x, g)
    assert C.rel_to_max(out, tout) <= tol and C.rel_to_max(gx, tgx) <= C.ROWS_GRAD_FACTOR * tol


# ---------------------------------------------------------------------------------------------------------------- 4. mvn log-density
def _mvn(lib, case, diag):
    L_ = _L()
    nb, B, D = case
    x, mean, Lm, g = (dev(t) for t in C.mvn_inputs(case, diag))
    y, qg = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    lp = torch.full((nb, B), 7.0, dtype=F64, device="cuda")
    L_.check(lib.otvae_mvn_logprob_fwd(L_.ptr(x), L_.ptr(mean), L_.ptr(Lm), nb, B, D, int(diag), L_.ptr(y), L_.ptr(lp), L_.stream()),
             "otvae_mvn_logprob_fwd")
    L_.check(lib.otvae_mvn_logprob_bwd(L_.ptr(g), L_.ptr(y), L_.ptr(Lm), nb, B, D, int(diag), L_.ptr(qg), L_.stream()),
             "otvae_mvn_logprob_bwd")
    return lp.cpu(), y.cpu(), qg.cpu()


def test_mvn_logprob_across_the_lds_switch(lib):
    """every case diag and full, in the table's order in this one test: the full-covariance calls cross 64 KiB of LDS between the
    third case and the fourth, so the limit is raised between two calls"""
    for case in C.MVN_CASES:
        for diag in (True, False):
            lp, y, qg = _mvn(lib, case, diag)
            t = C.mvn_truth(case, diag)
            _, _, Lm, g = C.mvn_inputs(case, diag)
            grads = C.mvn_caller_side(qg, y, Lm, g, diag)
            errs = dict(lp=C.rel_to_max(lp, t["lp"]), y=C.rel_to_max(y, t["y"]), **{k: C.rel_to_max(grads[k], t[k]) for k in grads})
            print(f"[ot_dense] mvn {case} {'diag' if diag else 'full'} (LDS {C.mvn_lds_bytes(case[2], diag)} B): "
                  + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
            assert errs["lp"] <= C.MVN_TOL and errs["y"] <= C.MVN_TOL, (case, diag, errs)
            assert max(errs["dx"], errs["dmean"], errs["dL"]) <= C.MVN_GRAD_TOL, (case, diag, errs)


@pytest.mark.parametrize("diag", [False, True])
def test_mvn_refuses_wide_covariances(lib, diag):
    L_ = _L()
    D = C.MVN_REFUSED_D
    x = torch.zeros(1, 2, D, dtype=F64, device="cuda")
    mean = torch.zeros(1, D, dtype=F64, device="cuda")
    Lm = torch.ones(1, D, dtype=F64, device="cuda") if diag else torch.eye(D, dtype=F64, device="cuda").unsqueeze(0).contiguous()
    g = torch.ones(1, 2, dtype=F64, device="cuda")
    y, lp = torch.full_like(x, 7.0), torch.full((1, 2), 7.0, dtype=F64, device="cuda")
    with pytest.raises(NotImplementedError):
        L_.check(lib.otvae_mvn_logprob_fwd(L_.ptr(x), L_.ptr(mean), L_.ptr(Lm), 1, 2, D, int(diag), L_.ptr(y), L_.ptr(lp), L_.stream()), "fwd")
    with pytest.raises(NotImplementedError):
        L_.check(lib.otvae_mvn_logprob_bwd(L_.ptr(g), L_.ptr(x), L_.ptr(Lm), 1, 2, D, int(diag), L_.ptr(y), L_.stream()), "bwd")
    assert bool((y == 7.0).all()) and bool((lp == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- 5. otvae_apply_transport
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("case", C.TRANSPORT_CASES, ids=str)
def test_apply_transport(lib, case, dtype):
    L_ = _L()
    nb, B, D = case
    c = C.transport_case(case, dtype)
    x, ms, mt, T = (dev(c[k]) for k in ("x", "ms", "mt", "T"))
    y = torch.full_like(x, 7.0)
    L_.check(lib.otvae_apply_transport(code(dtype), L_.ptr(x), L_.ptr(ms), L_.ptr(mt), L_.ptr(T), nb, B, D, L_.ptr(y), L_.stream()),
             "otvae_apply_transport")
    r = C.worst_ratio(y, c["truth"], c["bound"])
    print(f"[ot_dense] apply_transport {dtype} {case}: worst |got - truth| / bound {r:.3f}")
    assert y.dtype == dtype and r <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 6. otvae_gauss_stats
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("B", C.STATS_B)
def test_gauss_stats(lib, B, dtype):
    L_ = _L()
    nb = C.STATS_NB
    worst, where = 0.0, None
    for D in C.STATS_D:
        for diag in (False, True):
            case = C.stats_case(B, D, dtype, diag)
            x = dev(case["x"])
            nbytes = lib.otvae_gauss_stats_ws(nb, B, D, int(diag))
            assert nbytes == (8 if diag else nb * C.stats_ksplit(B) * (D + 1) * (D + 1) * 8)
            ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            for name, acc, decay in C.STATS_MODES:
                n, sx, sxx = (dev(case["old"][k]).clone() for k in ("n", "sx", "sxx"))
                L_.check(lib.otvae_gauss_stats(code(dtype), L_.ptr(x), nb, B, D, int(diag), acc, decay, L_.ptr(ws), L_.ptr(n), L_.ptr(sx),
                                               L_.ptr(sxx), L_.stream()), "otvae_gauss_stats")
                tb = C.stats_truth_and_bound(case, B, acc, decay)
                for key, got in (("n", n), ("sx", sx), ("sxx", sxx)):
                    truth, bound = tb[key]
                    r = C.worst_ratio(got, truth, bound + 1e-300)
                    if r > worst:
                        worst, where = r, (D, diag, name, key)
                    assert r <= 1.0, (B, D, dtype, diag, name, key, r)
                if name != "ema":
                    assert torch.equal(n.cpu(), tb["n"][0]), (B, D, dtype, diag, name)      # counts are exact
    print(f"[ot_dense] gauss_stats {dtype} B={B} (K split {C.stats_ksplit(B)}): worst |got - truth| / bound {worst:.3f} at "
          f"(D, diag, mode, output) = {where}")


# ---------------------------------------------------------------------------------------------------------------- 7. otvae_codebook_assign
def _assign(lib, x, cb):
    L_ = _L()
    nb, B, d = x.shape
    K = cb.shape[1]
    xd, cd = dev(x), dev(cb)
    idx = torch.full((nb, B), -5, dtype=torch.int64, device="cuda")
    enc = torch.full_like(xd, 7.0)
    L_.check(lib.otvae_codebook_assign(L_.ptr(xd), L_.ptr(cd), nb, B, K, d, C.CODEBOOK_TEMPERATURE, L_.ptr(idx), L_.ptr(enc), L_.stream()),
             "otvae_codebook_assign")
    return idx, enc, xd


def _kmeans_with_guard(lib, xd, idx, K):
    """counts / sums with one guard row of sentinels behind the nb * K real rows"""
    L_ = _L()
    nb, B, d = xd.shape
    counts = torch.full((nb * K + 1,), -3.0, device="cuda")
    sums = torch.full((nb * K + 1, d), -3.0, device="cuda")
    L_.check(lib.otvae_codebook_kmeans(L_.ptr(xd), L_.ptr(idx), nb, B, K, d, L_.ptr(counts), L_.ptr(sums), L_.stream()),
             "otvae_codebook_kmeans")
    counts, sums = counts.cpu(), sums.cpu()
    assert float(counts[-1]) == -3.0 and bool((sums[-1] == -3.0).all()), "otvae_codebook_kmeans wrote behind its K rows"
    return counts[:-1].reshape(nb, K), sums[:-1].reshape(nb, K, d)


@pytest.mark.parametrize("shape", C.CODEBOOK_SHAPES, ids=str)
def test_codebook_assign_is_the_argmin_with_first_index_ties(lib, shape):
    case = C.codebook_case(shape)
    idx, enc, xd = _assign(lib, case["x"], case["cb"])
    wrong = int((idx.cpu() != case["idx"]).sum())
    print(f"[ot_dense] codebook_assign {shape}: {wrong} of {idx.numel()} indices differ from the fp64 arg-min; planted ties "
          f"{[(r, lo, hi, idx[:, r].tolist()) for r, lo, hi in case['planted']]}")
    assert torch.equal(idx.cpu(), case["idx"])
    assert torch.equal(enc.cpu(), case["enc"])
    counts, sums = _kmeans_with_guard(lib, xd, idx, shape[2])
    want_counts, want_sums = C.kmeans_truth(case["x"], case["idx"], shape[2])
    assert torch.equal(counts, want_counts) and torch.equal(sums, want_sums)


@pytest.mark.parametrize("which", ["sample", "atom"])
def test_codebook_assign_with_nan_stays_inside_the_codebook(lib, which):
    """a NaN component of one sample / one NaN atom: index 0 like the reference's argmax(softmax(.)), every index inside [0, K),
    enc = that atom, the other samples untouched, and the k-means accumulation on these indices stays in its rows"""
    c = C.codebook_nan_cases()[which]
    nb, B, K, d = C.NAN_SHAPE
    idx, enc, xd = _assign(lib, c["x"], c["cb"])
    print(f"[ot_dense] codebook_assign NaN {which}: idx {idx.tolist()}")
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    assert torch.equal(idx.cpu(), c["idx"])
    want_enc = torch.gather(c["cb"], 1, c["idx"].unsqueeze(-1).expand(-1, -1, d))
    assert C.equal_with_nan(enc, want_enc) and bool(torch.isfinite(enc).all())
    counts, sums = _kmeans_with_guard(lib, xd, idx, K)
    want_counts, want_sums = C.kmeans_truth(c["x"], c["idx"], K)
    assert torch.equal(counts, want_counts) and counts.sum(-1).tolist() == [B] * nb
    assert C.equal_with_nan(sums, want_sums)
