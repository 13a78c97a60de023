"""CPU: the host half of ``test_gpu_ot_dense.py`` -- for every case of ``ot_dense_cases`` the conditions its expectation rests on, and
that the REFERENCE arithmetic alone (torch on the CPU, or an independent evaluation in another order or precision) meets the bound
the kernel will be held to.  So the bounds are pinned to the reference and to the number formats, not to the kernels.  No kernel runs."""
import math

import numpy as np
import pytest
import torch

import ot_dense_cases as C

F32, F64 = torch.float32, torch.float64


# ---------------------------------------------------------------------------------------------------------------- 1. Cholesky
@pytest.mark.parametrize("D", C.CHOL_SMALL + C.CHOL_BLOCKED)
def test_cholesky_reference_meets_the_residual_bound(D):
    A = C.chol_batch(D)
    assert A.shape == (3, D, D) and torch.equal(A, A.transpose(1, 2))
    assert torch.equal(A[2], 1e6 * A[0])
    if D > 1:
        lam = torch.linalg.eigvalsh(A[1])
        assert 1e7 < float(lam[-1] / lam[0]) < 1e9        # the graded spectrum: condition 1e8, pivots far above u
    L, info = torch.linalg.cholesky_ex(A)
    assert info.tolist() == [0, 0, 0] and C.chol_is_lower_positive(L)
    ratio = C.chol_residual_ratio(L, A)
    print(f"[ot_dense] cholesky D={D}: torch uses {ratio.tolist()} of the bound")
    assert float(ratio.max()) <= 0.5
    # the kernel's input holds NaN above the diagonal, and torch's factor of it is the same: the lower triangle is all that is read
    assert torch.equal(torch.linalg.cholesky(C.chol_kernel_input(A)), L)


@pytest.mark.parametrize("D,p", [(D, p) for D, ps in C.CHOL_BAD.items() for p in ps])
def test_cholesky_bad_pivot_cases(D, p):
    case = C.chol_bad_case(D, p)
    L, info = torch.linalg.cholesky_ex(case["A"])
    assert info.tolist() == case["info"]                  # torch reports 1 + the index of the failed pivot, too
    L0, a = case["L0"], case["a"]
    assert abs(float(case["A"][1, p, p] - (L0[p, :p] ** 2).sum()) + 1.0) < 1e-12
    ok = C.chol_residual_ratio(L[[0, 2]], case["A"][[0, 2]])
    assert float(ok.max()) <= 0.5
    # columns < p do not depend on A[p][p]; a correct factor with its sums in another order stays within the bound of torch's
    other = C.chol_right_looking(a)
    r = C.worst_ratio(other[:, :p], L0[:, :p], C.chol_bound(a)[:, :p]) if p else 0.0
    print(f"[ot_dense] cholesky D={D} p={p}: right-looking vs torch, columns < p: {r:.3f} of the bound")
    assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 2. GEMM
def test_gemm_table_straddles_the_dispatch_line():
    kinds = [C.gemm_uses_mfma(m, n, k) for _, m, n, k in C.GEMM_SHAPES]
    assert kinds == [False, False, False, False, True, True, True, True]
    assert not C.gemm_uses_mfma(255, 255, 64) and not C.gemm_uses_mfma(256, 1, 63) and C.gemm_uses_mfma(256, 1, 64)
    assert len(C.gemm_combos(1)) == 8 and len(C.gemm_combos(2)) == 24


@pytest.mark.parametrize("shape", C.GEMM_SHAPES, ids=str)
def test_gemm_reference_meets_both_bounds(shape):
    nb, m, n, k = shape
    worst32 = worst64 = 0.0
    for ta, tb, alpha, beta, bcast in C.gemm_combos(nb):
        # fp32: torch's own fp32 evaluation against the fp64 truth
        As, Bs, C0, truth, E = C.gemm_case(shape, F32, ta, tb, alpha, beta, bcast)
        assert As.dtype == F32 and As.shape[1:] == ((k, m) if ta else (m, k)) and Bs.shape[1:] == ((n, k) if tb else (k, n))
        assert As.shape[0] == (1 if bcast == "A" else nb) and Bs.shape[0] == (1 if bcast == "B" else nb)
        opa, opb = (As.transpose(1, 2) if ta else As), (Bs.transpose(1, 2) if tb else Bs)
        ref32 = alpha * (opa @ opb) + beta * C0
        worst32 = max(worst32, C.worst_ratio(ref32, truth, C.gemm_bound(E, k, F32)))
        # fp64: torch's fp64 evaluation against numpy.longdouble
        As, Bs, C0, truth, E = C.gemm_case(shape, F64, ta, tb, alpha, beta, bcast)
        opa, opb = (As.transpose(1, 2) if ta else As), (Bs.transpose(1, 2) if tb else Bs)
        if ta == 0 and tb == 0:   # the value does not depend on the storage order: one long-double product per (scalars, broadcast)
            ld = C.gemm_truth_longdouble(opa, opb, C0, alpha, beta)
            err = np.abs(truth.numpy().astype(np.longdouble) - ld).astype(np.float64)
            worst64 = max(worst64, float((torch.from_numpy(err) / C.gemm_bound(E, k, F64)).max()))
        # the stored (transposed, shared) operands describe the same product
        assert C.worst_ratio(alpha * (opa @ opb) + beta * C0, truth, C.gemm_bound(E, k, F64)) <= 1.0
    print(f"[ot_dense] gemm {shape}: torch fp32 uses {worst32:.3f} of the fp32 bound, torch fp64 {worst64:.3f} of the fp64 bound")
    assert worst32 <= 1.0 and worst64 <= 1.0


# ---------------------------------------------------------------------------------------------------------------- 3. rows
@pytest.mark.parametrize("shape", C.ROWS_SHAPES, ids=str)
def test_rows_reference_fp32_meets_the_tolerances(shape):
    """torch's own fp32 softmax / logsumexp of the same fp32 inputs against the fp64 truth, at the suite's tolerance"""
    tol = C.ROWS_TOL[F32]
    for wide in (False, True):
        x, gy, g = C.rows_input(shape, F32, wide)
        if wide and shape[1] >= 2:
            assert float(x.max()) == 1e4 and float(x.min()) == -1e4
            assert not torch.isfinite(torch.exp(x)).all()          # the naive form overflows fp32
        for scale in ([1.0] if wide else C.SOFTMAX_SCALES):
            y, gx = C.softmax_truth(x, scale, gy)
            xr = x.clone().requires_grad_(True)
            y32 = torch.softmax(xr * scale, dim=-1)
            (gx32,) = torch.autograd.grad(y32, xr, gy)
            assert C.rel_to_max(y32, y) <= tol and C.rel_to_max(gx32, gx) <= C.ROWS_GRAD_FACTOR * tol, (shape, wide, scale)
        out, gx = C.lse_truth(x, g)
        xr = x.clone().requires_grad_(True)
        o32 = torch.logsumexp(xr, dim=-1)
        (gx32,) = torch.autograd.grad(o32, xr, g)
        assert C.rel_to_max(o32, out) <= tol, (shape, wide)
        if not wide:
            assert C.rel_to_max(gx32, gx) <= C.ROWS_GRAD_FACTOR * tol, shape
        else:
            # |lse| ~ 1e4 in fp32 is rounded by up to 6e-4, and exp(x - lse) inherits it: torch's own fp32 gradient misses the fp64
            # autograd gradient here by up to 5e-4 of its maximum (printed), so the wide fp32 backward is judged against its own
            # definition evaluated in fp64 from the operands it is handed (C.lse_bwd_truth) -- which torch's fp32 arithmetic meets
            print(f"[ot_dense] wide lse {shape}: torch fp32 gradient vs fp64 autograd {C.rel_to_max(gx32, gx):.2e}")
            ref32 = g.unsqueeze(-1) * torch.exp(x - o32.detach().unsqueeze(-1))
            assert C.rel_to_max(ref32, C.lse_bwd_truth(x, o32.detach(), g)) <= C.ROWS_GRAD_FACTOR * tol, shape
            # (fp64: the same rounding is 2^-53 |lse| = 1e-12 against a tolerance of 5e-13 -- the wide backward uses that truth in
            # both precisions)


@pytest.mark.parametrize("K", C.SPECIAL_K)
def test_special_rows_are_what_torch_gives(K):
    """the table of the special rows, recorded from torch on the CPU: the kernels are held to these, not the other way round"""
    for dtype in (F32, F64):
        x, gy, g, at = C.special_rows(K, C.LSE_SPECIAL_ROWS, dtype)
        out, gx = C.lse_truth(x, g)
        row = {kind: r for r, kind in enumerate(C.LSE_SPECIAL_ROWS)}
        r = row["all -inf"]
        assert out[r] == -C.INF and torch.isnan(gx[r]).all()
        r = row["some -inf"]
        assert torch.isfinite(out[r]) and gx[r, 0] == 0 and gx[r, at] == 0 and torch.isfinite(gx[r]).all()
        r = row["+inf among finite"]
        want_nan = torch.zeros(K, dtype=torch.bool)
        want_nan[at] = True
        assert out[r] == C.INF and torch.equal(torch.isnan(gx[r]), want_nan) and bool((gx[r][~want_nan] == 0).all())
        r = row["nan among finite"]
        assert torch.isnan(out[r]) and torch.isnan(gx[r]).all()
        assert torch.isfinite(out[row["finite"]]) and torch.isfinite(gx[row["finite"]]).all()
        # fp32 torch agrees with the fp64 truth on every special
        if dtype == F32:
            xr = x.clone().requires_grad_(True)
            o32 = torch.logsumexp(xr, dim=-1)
            (g32,) = torch.autograd.grad(o32, xr, g)
            assert C.same_specials(o32, out)[0] and C.same_specials(g32, gx)[0]

        x, gy, g, at = C.special_rows(K, C.SOFTMAX_SPECIAL_ROWS, dtype)
        y, gx = C.softmax_truth(x, 1 / 0.3, gy)
        assert torch.isnan(y[0]).all() and torch.isnan(gx[0]).all()                       # all -inf: NaN like torch
        assert y[1, 0] == 0 and y[1, at] == 0 and gx[1, 0] == 0 and gx[1, at] == 0 and torch.isfinite(y[1:]).all()
        assert torch.isfinite(gx[1:]).all() and abs(float(y[1].sum()) - 1.0) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- 4. mvn
def test_mvn_cases_cross_the_lds_limit_in_order():
    full = [C.mvn_lds_bytes(D, False) > 65536 for _, _, D in C.MVN_CASES]
    assert full == [False, False, False, True, True]               # raised between the third call and the fourth
    assert C.mvn_lds_bytes(90, False) <= 65536 < C.mvn_lds_bytes(91, False)
    assert [B % 256 for _, B, _ in C.MVN_CASES[1:4]] == [255, 0, 1]
    assert C.MVN_REFUSED_D == C.MVN_CASES[-1][2] + 1


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("case", C.MVN_CASES, ids=str)
def test_mvn_truth_and_the_caller_side_formulas(case, diag):
    """cond(L) < 1e3, and the header's formulas applied to an fp64 qg = g L^-T y computed here reproduce autograd's gradients to the
    tolerance the kernel gets: the expectation is the reference's, the formulas are the right ones"""
    x, mean, L, g = C.mvn_inputs(case, diag)
    t = C.mvn_truth(case, diag)
    if diag:
        assert float(L.max() / L.min()) < 1e3 and float(L.min()) >= 0.5
        qg = g.unsqueeze(-1) * t["y"] / L.unsqueeze(1)
    else:
        assert float(torch.linalg.cond(L).max()) < 1e3
        d = L.diagonal(dim1=-2, dim2=-1)
        assert float(d.min()) >= 0.5 and float(d.max()) <= 2.0 and bool((L.triu(1) == 0).all())
        qg = g.unsqueeze(-1) * torch.linalg.solve_triangular(L.transpose(1, 2), t["y"].transpose(1, 2), upper=True).transpose(1, 2)
    got = C.mvn_caller_side(qg, t["y"], L, g, diag)
    for key in ("dx", "dmean", "dL"):
        assert C.rel_to_max(got[key], t[key]) <= C.MVN_GRAD_TOL, (case, diag, key)
    D = case[2]
    lp = -0.5 * (t["y"] ** 2).sum(-1) - (L if diag else L.diagonal(dim1=-2, dim2=-1)).log().sum(-1, keepdim=True) - 0.5 * D * math.log(2 * math.pi)
    assert C.rel_to_max(lp, t["lp"]) <= C.MVN_TOL


# ---------------------------------------------------------------------------------------------------------------- 5. transport
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("case", C.TRANSPORT_CASES, ids=str)
def test_transport_reference_meets_the_bound(case, dtype):
    """the same map evaluated in another order ((T x) - (T ms) + mt, fp64) stays within the bound; an fp32 rounding of it, too"""
    c = C.transport_case(case, dtype)
    other = c["x"].double() @ c["T"].transpose(1, 2) - (c["T"] @ c["ms"].unsqueeze(-1)).squeeze(-1).unsqueeze(1) + c["mt"].unsqueeze(1)
    if dtype == F32:
        other = other.float()
    # the split form cancels |T| |x| + |T| |ms| instead of |T| |x - ms|: grant it that, it is the reference's own error here
    extra = 2.0 * (case[2] + 3) * C.U * (c["x"].double().abs() @ c["T"].abs().transpose(1, 2) + (c["T"].abs() @ c["ms"].abs().unsqueeze(-1)).squeeze(-1).unsqueeze(1))
    assert C.worst_ratio(other, c["truth"], c["bound"] + extra) <= 1.0
    assert bool((c["bound"] > 0).all())


# ---------------------------------------------------------------------------------------------------------------- 6. statistics
def test_stats_table_enters_every_split():
    assert {B: C.stats_ksplit(B) for B in C.STATS_B} == C.STATS_KSPLIT
    rows_per = {B: -(-B // C.stats_ksplit(B)) for B in C.STATS_B}
    assert rows_per[130] == 65 and rows_per[1100] == 69 and 1100 - 15 * 69 == 65     # ragged parts, ragged 16-row tiles inside them
    assert [(D + 1) % 16 for D in C.STATS_D] == [2, 0, 1, 0] and [-(-(D + 1) // 16) for D in C.STATS_D] == [1, 1, 2, 2]


@pytest.mark.parametrize("B", C.STATS_B)
def test_stats_reference_meets_the_bound(B):
    """the sums in another order (reversed rows, fp64) and, for fp32 samples, exactly the same numbers: within the bound"""
    for D in C.STATS_D:
        for dtype in (F32, F64):
            for diag in (False, True):
                case = C.stats_case(B, D, dtype, diag)
                xr = case["x"].double().flip(1)
                other = dict(n=torch.full((C.STATS_NB,), float(B), dtype=F64), sx=xr.sum(1),
                             sxx=(xr * xr).sum(1) if diag else torch.einsum("nbi,nbj->nij", xr, xr))
                for name, acc, decay in C.STATS_MODES:
                    tb = C.stats_truth_and_bound(case, B, acc, decay)
                    for key, (truth, bound) in tb.items():
                        o = case["old"][key]
                        got = other[key] if not acc else (o + other[key] if decay < 0 else o * decay + other[key] * (1.0 - decay))
                        assert C.worst_ratio(got, truth, bound + 1e-300) <= 1.0, (B, D, dtype, diag, name, key)
                    if name != "ema":
                        n_truth = tb["n"][0]
                        assert torch.equal(n_truth, n_truth.round()) and float(n_truth.max()) < 2 ** 53


# ---------------------------------------------------------------------------------------------------------------- 7. codebook
@pytest.mark.parametrize("shape", C.CODEBOOK_SHAPES, ids=str)
def test_codebook_cases_are_exact_and_decided(shape):
    nb, B, K, d = shape
    case = C.codebook_case(shape)
    x, cb, d2 = case["x"], case["cb"], case["d2"]
    for t in (x, cb):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
    # squared distances: the same exact integers in fp32 (fused or not) and fp64
    d2_32 = ((x.unsqueeze(2) - cb.unsqueeze(1)) ** 2).sum(-1)
    assert torch.equal(d2_32.double(), d2) and float(d2.max()) <= 36 * d < 2 ** 24
    # the winner and the first DIFFERENT distance are more than 1e-3 apart relatively: no fp32 rounding of 1 / (dist + 1e-8) / T
    # can reorder them (equal distances give equal bits, and then the first index must win)
    dist = d2.sqrt()
    best = dist.min(-1, keepdim=True).values
    rest = torch.where(dist > best, dist, torch.full_like(dist, C.INF)).min(-1, keepdim=True).values
    gap = ((rest - best) / rest).min().item() if K > 1 else 1.0
    assert gap > 1e-3, gap
    e32 = (1.0 / (d2_32.sqrt() + 1e-8)) * (1.0 / C.CODEBOOK_TEMPERATURE)
    assert torch.equal(e32.argmax(-1), case["idx"])       # torch.argmax: first index among equal bits
    for r, lo, hi in case["planted"]:
        assert torch.equal(cb[:, lo], cb[:, hi]) and torch.equal(x[:, r], cb[:, lo])
        assert bool((case["idx"][:, r] == lo).all()), "an earlier random atom equals the planted one: pick another seed"
    assert [hi - lo for _, lo, hi in case["planted"]] == ([64, 1] if K > 64 else ([1] if K >= 2 else []))
    assert torch.equal(case["enc"], torch.stack([cb[b][case["idx"][b]] for b in range(nb)]))


def test_codebook_nan_rule_is_the_references():
    """argmax(softmax(energy / T)) of a row holding a NaN is 0 -- for a NaN component of the sample and for a NaN atom -- and every
    other sample keeps its index"""
    cases = C.codebook_nan_cases()
    nb, B, K, d = C.NAN_SHAPE
    (b, r, _), (pb, k) = C.NAN_SAMPLE, C.NAN_ATOM
    assert r != 0 and k == 7 and K == 65 and b != pb
    for name in ("sample", "atom"):
        c = cases[name]
        ref = C.reference_assign(c["x"], c["cb"], C.CODEBOOK_TEMPERATURE)
        poisoned = torch.zeros(nb, B, dtype=torch.bool)
        if name == "sample":
            poisoned[b, r] = True
        else:
            poisoned[pb] = True
        assert bool((ref[poisoned] == 0).all()) and bool((c["idx"][poisoned] == 0).all())
        assert torch.equal(c["idx"][~poisoned], cases["clean"]["idx"][~poisoned])
        assert bool((c["idx"] >= 0).all()) and bool((c["idx"] < K).all())
        # the clean indices of the poisoned samples were not 0 to begin with, or the case would show nothing
        assert bool((cases["clean"]["idx"][poisoned] != 0).any())
    counts, sums = C.kmeans_truth(cases["atom"]["x"], cases["atom"]["idx"], K)
    assert counts.sum(-1).tolist() == [B] * nb
