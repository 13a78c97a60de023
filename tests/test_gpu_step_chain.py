"""GPU: the kernels that end every training step (csrc/loss_optim.hip), each on its own through its raw entry point on tensors built
here -- no model, no trainer -- against the fp64 truths of ``step_chain_cases.py``: ``otvae_adam_step`` (float4 body, tail, capped
grid, bias correction at t > 1, host and device scale, the step guard with its restore loop, the folded EMA), ``otvae_ema_update``,
``otvae_grad_clip_coef``, ``otvae_nelbo_fwd / _bwd``, ``otvae_copy_batched``, ``otvae_step_begin``, ``otvae_zero_words``, and one
five-step chain against ``torch.optim.Adam`` and ``clip_grad_norm_`` in float64.  Every buffer a kernel writes sits between guard bands
that are asserted untouched; pure outputs start from a sentinel.  ``test_step_chain_host.py`` asserts, without a GPU, that the
reference arithmetic meets every bound used here and that each bound rejects a defective kernel.  Every refusal exercised is made by
the entry point on the host before anything is launched; NaN and inf travel as data only.  Each figure is printed before it is
asserted."""
import ctypes

import pytest
import torch

import step_chain_cases as C

pytestmark = pytest.mark.gpu

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    from ot_vae_lightning_amd import _lib
    return _lib.load()


def _L():
    from ot_vae_lightning_amd import _lib
    return _lib


def band(inner):
    return C.banded(inner, device="cuda")


def ints(*values):
    return band(torch.tensor(values, dtype=I32))


def floats(*values):
    return band(torch.tensor(values, dtype=F32))


def adam(lib, p, g, m, v, step, s=1.0, scale_dev=None, watch=None, guard=None, state=None, backup=None, n_state=0, ema=None,
         decay=0.0, n=None, hyper="default"):
    L_ = _L()
    hyper = C.HYPER.cuda() if isinstance(hyper, str) else hyper
    rc = lib.otvae_adam_step(L_.ptr(p), L_.ptr(g), L_.ptr(m), L_.ptr(v), p.numel() if n is None else n, L_.ptr(hyper), L_.ptr(step), s,
                             L_.ptr(scale_dev), L_.ptr(watch), L_.ptr(guard), L_.ptr(state), L_.ptr(backup), n_state, L_.ptr(ema),
                             decay, L_.stream())
    L_.check(rc, "otvae_adam_step")


# ---------------------------------------------------------------------------------------------------------------- 1. otvae_adam_step
@pytest.mark.parametrize("t", C.ADAM_T)
@pytest.mark.parametrize("n", C.ADAM_N)
def test_adam_plain(lib, n, t):
    """m', v' and the update at p = 0 against fp64, with the host scalar; the device scalar must give the same bits"""
    g, m, v = C.adam_inputs(n)
    p0 = torch.zeros(n)
    Wg, gd = band(g)
    worst, relu, common = dict(m=0.0, v=0.0, upd=0.0), 0.0, 0.0
    for s in C.ADAM_SCALES:
        got = {}
        for route in ("host", "device"):
            (Wp, pd), (Wm, md), (Wv, vd), (Wt, td) = band(p0), band(m), band(v), ints(t)
            if route == "host":
                adam(lib, pd, gd, md, vd, td, s=s)
            else:           # the host scalar must be ignored: it would change every value
                Ws, sd = floats(s, 1.0)
                adam(lib, pd, gd, md, vd, td, s=3.0, scale_dev=sd)
                assert C.bits_equal(Ws.cpu(), C.banded(torch.tensor([s, 1.0]))[0])
            assert all(C.bands_intact(W) for W in (Wp, Wm, Wv, Wt, Wg)), (n, t, s, route)
            assert int(td[0]) == t                                     # an accepted step leaves the counter alone
            got[route] = (pd.cpu(), md.cpu(), vd.cpu())
        assert C.bits_equal(gd.cpu(), g)
        assert all(C.bits_equal(a, b) for a, b in zip(got["host"], got["device"])), (n, t, s, "host and device scale differ")
        pg, mg, vg = got["host"]
        tr = C.adam_truth(g, m, v, p0, s, t)
        b = C.adam_bounds(g, m, v, s, t, tr)
        r = dict(m=C.worst_ratio(mg, tr["m"], b["m"]), v=C.worst_ratio(vg, tr["v"], b["v"]), upd=C.worst_ratio(-pg.double(), tr["upd"], b["upd"]))
        worst = {k: max(worst[k], r[k]) for k in r}
        relu = max(relu, C.rel_err(-pg.double(), tr["upd"]))
        common = max(common, C.median_rel_err(-pg.double(), tr["upd"]))
        if n >= 5:      # the fresh parameter with a zero gradient: a zero update, not 0 / 0
            assert float(pg[-1]) == 0.0 and float(mg[-1]) == 0.0 and float(vg[-1]) == 0.0
    print(f"[step_chain] adam n={n} t={t}: worst |got - truth| / bound m {worst['m']:.3f}, v {worst['v']:.3f}, update {worst['upd']:.3f}; "
          f"relative update error: largest {relu:.3e} (where m and g cancel), median {common:.3e} (the bias corrections' common mode)")
    assert max(worst.values()) <= 1.0, (n, t, worst)


def test_adam_generic_p(lib):
    """the new parameter at a p of order 1: within half an ulp of p plus the update's bound"""
    n, t, s = 4099, 10, 0.5
    g, m, v = C.adam_inputs(n)
    p0 = C.generic_p(n)
    (Wp, pd), (Wg, gd), (Wm, md), (Wv, vd), (Wt, td) = band(p0), band(g), band(m), band(v), ints(t)
    adam(lib, pd, gd, md, vd, td, s=s)
    tr = C.adam_truth(g, m, v, p0, s, t)
    b = C.adam_bounds(g, m, v, s, t, tr)
    r = C.worst_ratio(pd, tr["p"], C.p_bound(tr, b["upd"]))
    print(f"[step_chain] adam generic p n={n} t={t} s={s}: worst |p' - truth| / (update bound + half ulp) {r:.3f}")
    assert r <= 1.0 and all(C.bands_intact(W) for W in (Wp, Wm, Wv, Wt))


# ---------------------------------------------------------------------------------------------------------------- 2. the guard matrix
@pytest.mark.parametrize("n_state", C.GUARD_N_STATE)
def test_guard_matrix(lib, n_state):
    n, t = C.GUARD_N, 7
    g, m, v = C.adam_inputs(n)
    p0, e0 = C.generic_p(n), C.randn32(n, 77)
    state0, backup0 = C.randn32(max(n_state, 1), 78)[:n_state], C.randn32(max(n_state, 1), 79)[:n_state]
    seen = []
    for source in C.GUARD_SOURCES:
        for value in C.GUARD_VALUES:
            (Wp, pd), (Wg, gd), (Wm, md), (Wv, vd), (We, ed) = band(p0), band(g), band(m), band(v), band(e0)
            (Wt, td), (Wq, qd) = ints(t), ints(3, 2)
            Wst, std = band(state0)
            Wb, bd = band(backup0)
            watch = floats(value if source == "watch_loss" else 0.25)[1] if source in ("watch_loss", "norm") else None
            sdev = None
            if source == "norm":
                sdev = floats(0.5, value)[1]
            elif source == "device grad_scale":
                sdev = floats(value, 1.0)[1]
            s = value if source == "host grad_scale" else 1.0
            adam(lib, pd, gd, md, vd, td, s=s, scale_dev=sdev, watch=watch, guard=qd, state=std if n_state else None,
                 backup=bd if n_state else None, n_state=n_state, ema=ed, decay=0.9)
            assert all(C.bands_intact(W) for W in (Wp, Wm, Wv, We, Wt, Wq, Wst, Wb)), (source, value)
            assert C.bits_equal(bd.cpu(), backup0)
            refused = C.guard_refuses(value)
            seen.append((source, value, refused))
            if refused:
                assert C.bits_equal(pd.cpu(), p0) and C.bits_equal(md.cpu(), m) and C.bits_equal(vd.cpu(), v), (source, value)
                assert C.bits_equal(ed.cpu(), e0), (source, value)
                assert C.bits_equal(std.cpu(), backup0), (source, value, "state was not restored")
                assert td.tolist() == [t - 1] and qd.tolist() == [4, t], (source, value, td.tolist(), qd.tolist())
            else:
                assert C.bits_equal(std.cpu(), state0), (source, value, "an accepted step touched the state")
                assert td.tolist() == [t] and qd.tolist() == [3, 2], (source, value, td.tolist(), qd.tolist())
                s_eff = value if source in ("host grad_scale", "device grad_scale") else (0.5 if source == "norm" else 1.0)
                tr = C.adam_truth(g, m, v, p0, s_eff, t)
                b = C.adam_bounds(g, m, v, s_eff, t, tr)
                r = max(C.worst_ratio(md, tr["m"], b["m"]), C.worst_ratio(vd, tr["v"], b["v"]), C.worst_ratio(pd, tr["p"], C.p_bound(tr, b["upd"])))
                assert r <= 1.0, (source, value, r)
                assert C.bits_equal(ed.cpu(), C.ema_rule(e0, pd.cpu(), 0.9, t))
    print(f"[step_chain] guard n_state={n_state}: (source, value, refused) {seen}")
    if n_state:
        assert not C.bits_equal(state0, backup0)


def test_adam_entry_refusals(lib):
    """refusals of the entry itself: made on the host, nothing is launched, nothing changes"""
    n, t = C.GUARD_N, 7
    g, m, v = C.adam_inputs(n)
    p0 = C.generic_p(n)
    (Wp, pd), (Wg, gd), (Wm, md), (Wv, vd), (We, ed) = band(p0), band(g), band(m), band(v), band(p0)
    (Wt, td), (Wq, qd) = ints(t), ints(3, 2)
    (Wst, std), (Wb, bd) = band(C.randn32(7, 1)), band(C.randn32(7, 2))
    watch = floats(0.25)[1]
    off = {k: band(x)[0][C.BAND + 1:C.BAND + 1 + n] for k, x in (("p", p0), ("g", g), ("m", m), ("v", v), ("ema", p0))}   # 4 bytes off
    calls = {
        "n_state without state": dict(guard=qd, backup=bd, n_state=7),
        "n_state without backup": dict(guard=qd, state=std, n_state=7),
        "n_state without guard": dict(state=std, backup=bd, n_state=7),
        "negative n_state": dict(guard=qd, state=std, backup=bd, n_state=-1),
        "watched loss without guard": dict(watch=watch),
        "ema_decay above 1": dict(ema=ed, decay=1.0 + 2.0 ** -52),
        "ema_decay below 0": dict(ema=ed, decay=-2.0 ** -60),
        "ema_decay NaN": dict(ema=ed, decay=C.NAN),
        "n = 0": dict(n=0),
        "negative n": dict(n=-4),
    }
    for what, kw in calls.items():
        with pytest.raises(ValueError):
            adam(lib, pd, gd, md, vd, td, **kw)
    for k in off:
        args = dict(p=pd, g=gd, m=md, v=vd)
        kw = {}
        if k == "ema":
            kw = dict(ema=off[k], decay=0.9)
        else:
            args[k] = off[k]
        assert off[k].data_ptr() % 16 == 4
        with pytest.raises(ValueError):
            adam(lib, args["p"], args["g"], args["m"], args["v"], td, **kw)
    for nul in range(6):
        a = [pd, gd, md, vd, C.HYPER.cuda(), td]
        a[nul] = None
        with pytest.raises(ValueError):
            adam(lib, a[0], a[1], a[2], a[3], a[5], hyper=a[4], n=n)
    torch.cuda.synchronize()
    assert C.bits_equal(pd.cpu(), p0) and C.bits_equal(md.cpu(), m) and C.bits_equal(vd.cpu(), v) and C.bits_equal(ed.cpu(), p0)
    assert td.tolist() == [t] and qd.tolist() == [3, 2]
    assert all(C.bands_intact(W) for W in (Wp, Wm, Wv, We, Wt, Wq, Wst, Wb))


# ---------------------------------------------------------------------------------------------------------------- 3. the parameter EMA
@pytest.mark.parametrize("decay", C.EMA_DECAYS)
def test_ema_inside_adam(lib, decay):
    """the shadow is, bit for bit, oracle.ParamEMARef's rule applied to the p the kernel wrote.  (A decay of 1 is the warm-up
    (1 + t) / (10 + t) for ever here: min(1, .) never reaches 1.)"""
    n = C.EMA_IN_ADAM_N
    g, m, v = C.adam_inputs(n)
    p0, e0 = C.generic_p(n), C.randn32(n, 70)
    for t in C.EMA_T:
        (Wp, pd), (Wg, gd), (Wm, md), (Wv, vd), (We, ed), (Wt, td) = band(p0), band(g), band(m), band(v), band(e0), ints(t)
        adam(lib, pd, gd, md, vd, td, s=0.5, ema=ed, decay=decay)
        want = C.ema_rule(e0, pd.cpu(), decay, t)
        diff = int((ed.cpu().view(I32) != want.view(I32)).sum())
        print(f"[step_chain] ema inside adam decay={decay} t={t}: {diff} of {n} shadow entries differ from ParamEMARef's rule")
        assert diff == 0 and all(C.bands_intact(W) for W in (Wp, Wm, Wv, We, Wt))
        # the same step without a shadow: the same p, m, v
        (Wp2, pd2), (Wm2, md2), (Wv2, vd2), (Wt2, td2) = band(p0), band(m), band(v), ints(t)
        adam(lib, pd2, gd, md2, vd2, td2, s=0.5)
        assert C.bits_equal(pd2.cpu(), pd.cpu()) and C.bits_equal(md2.cpu(), md.cpu()) and C.bits_equal(vd2.cpu(), vd.cpu())


@pytest.mark.parametrize("n", C.EMA_N)
def test_ema_update(lib, n):
    L_ = _L()
    s0, p = C.randn32(n, 60), C.randn32(n, 61)
    Wp, pd = band(p)
    for decay in C.EMA_DECAYS:
        Ws, sd = band(s0)
        L_.check(lib.otvae_ema_update(L_.ptr(sd), L_.ptr(pd), n, decay, L_.stream()), "otvae_ema_update")
        want = s0 if decay == 1.0 else C.ema_fixed_rule(s0, p, decay)      # decay 1: bit-unchanged
        diff = int((sd.cpu().view(I32) != want.view(I32)).sum())
        print(f"[step_chain] ema_update n={n} decay={decay}: {diff} entries differ from the three-rounding rule")
        assert diff == 0 and C.bands_intact(Ws) and C.bits_equal(pd.cpu(), p)
    Ws, sd = band(s0)
    for bad in (dict(decay=1.5), dict(decay=-0.1), dict(n=0), dict(shadow=None), dict(p=None)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_ema_update(L_.ptr(bad.get("shadow", sd)), L_.ptr(bad.get("p", pd)), bad.get("n", n), bad.get("decay", 0.9),
                                          L_.stream()), "otvae_ema_update")
    assert C.bits_equal(sd.cpu(), s0)


# ---------------------------------------------------------------------------------------------------------------- 4. otvae_grad_clip_coef
def clip(lib, gd, n, s, max_norm):
    """raw entry with a NaN-filled workspace and a sentinel output, both banded: (out as fp64 pair on the host, out on the device)"""
    L_ = _L()
    Ww, wd = band(torch.full((lib.otvae_grad_clip_ws(),), C.NAN, dtype=F64))
    Wo, od = band(2)
    L_.check(lib.otvae_grad_clip_coef(L_.ptr(gd), n, s, max_norm, L_.ptr(wd), L_.ptr(od), L_.stream()), "otvae_grad_clip_coef")
    assert C.bands_intact(Ww) and C.bands_intact(Wo)
    return od.cpu().double().tolist(), od


@pytest.mark.parametrize("n", C.CLIP_N)
def test_grad_clip_coef(lib, n):
    g = C.clip_gradient(n)
    Wg, gd = band(g)
    worst0 = worst1 = 0.0
    for s in C.CLIP_SCALES:
        norm = C.clip_truth(g, s, 0.0)[1]
        for fac in C.CLIP_MAX_NORM_FACTORS:
            mx = float(torch.tensor(fac * norm, dtype=F32))
            tr = C.clip_truth(g, s, mx)
            d0, d1 = C.clip_bounds(n, s, mx, tr)
            out, _ = clip(lib, gd, n, s, mx)
            r0, r1 = C.worst_ratio(out[0], tr[0], d0), C.worst_ratio(out[1], tr[1], d1)
            worst0, worst1 = max(worst0, r0), max(worst1, r1)
            if d0 == 0.0:
                assert out[0] == s, (n, s, fac, out)           # not clipping, or reporting only: the scale is s itself
            assert r0 <= 1.0 and r1 <= 1.0, (n, s, fac, out, tr)
    print(f"[step_chain] grad_clip_coef n={n} ({C.clip_parts(n)} parts): worst |got - truth| / bound scale {worst0:.3f}, norm {worst1:.3f}")
    assert C.bits_equal(gd.cpu(), g) and C.bands_intact(Wg)


@pytest.mark.parametrize("poison", [1e20, C.NAN], ids=["square overflows", "nan"])
def test_grad_clip_of_a_diverged_gradient_makes_adam_refuse(lib, poison):
    """outside the range the truth states (clip_in_range) nothing is asserted about the norm but this: an fp32 square that overflows
    reports +inf, a NaN entry NaN, and the guarded Adam fed this pair refuses the step"""
    n, t = 4097, 5
    g = C.clip_gradient(n).clone()
    g[n // 2] = poison
    assert not C.clip_in_range(g) or poison != poison
    Wg, gd = band(g)
    out, od = clip(lib, gd, n, 1.0, 1.0)
    print(f"[step_chain] grad_clip_coef with an entry of {poison}: out = {out}")
    assert out[1] == C.INF if poison == 1e20 else out[1] != out[1]
    _, m, v = C.adam_inputs(n)
    p0 = C.generic_p(n)
    (Wp, pd), (Wm, md), (Wv, vd), (Wt, td), (Wq, qd) = band(p0), band(m), band(v), ints(t), ints(0, 0)
    adam(lib, pd, gd, md, vd, td, scale_dev=od, guard=qd)
    assert C.bits_equal(pd.cpu(), p0) and C.bits_equal(md.cpu(), m) and C.bits_equal(vd.cpu(), v)
    assert td.tolist() == [t - 1] and qd.tolist() == [1, t]
    assert all(C.bands_intact(W) for W in (Wp, Wm, Wv, Wt, Wq))


def test_grad_clip_refusals(lib):
    L_ = _L()
    g = C.clip_gradient(4097)
    Wg, gd = band(g)
    Ww, wd = band(torch.full((lib.otvae_grad_clip_ws(),), C.NAN, dtype=F64))
    Wo, od = band(2)
    for a in ((None, 5, wd, od), (gd, 0, wd, od), (gd, -1, wd, od), (gd, 5, None, od), (gd, 5, wd, None), (gd[1:], 5, wd, od)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_grad_clip_coef(L_.ptr(a[0]), a[1], 1.0, 1.0, L_.ptr(a[2]), L_.ptr(a[3]), L_.stream()), "otvae_grad_clip_coef")
    assert bool((od.cpu() == C.SENT).all()) and bool(torch.isnan(wd.cpu()).all())


# ---------------------------------------------------------------------------------------------------------------- 5. nelbo
def nelbo_fwd(lib, pd, td, numel, prd, B, chw):
    L_ = _L()
    Ww, wd = band(torch.full((lib.otvae_nelbo_ws(),), C.NAN, dtype=F64))
    Wo, od = band(3)
    L_.check(lib.otvae_nelbo_fwd(L_.ptr(pd), L_.ptr(td), numel, L_.ptr(prd), B, chw, L_.ptr(wd), L_.ptr(od), L_.stream()), "otvae_nelbo_fwd")
    assert C.bands_intact(Ww) and C.bands_intact(Wo)
    return od.cpu().double().tolist()


@pytest.mark.parametrize("numel", C.NELBO_FWD_NUMEL)
def test_nelbo_fwd(lib, numel):
    worst = [0.0, 0.0, 0.0]
    for B in C.NELBO_B:
        pred, target, prior = C.nelbo_inputs(numel, B)
        pd, td, prd = pred.cuda(), target.cuda(), prior.cuda()
        for chw in C.NELBO_CHW:
            for pl, pld in ((None, None), (prior, prd)):
                tr, bd = C.nelbo_fwd_truth(pred, target, pl, chw)
                out = nelbo_fwd(lib, pd, td, numel, pld, B, chw)
                r = [C.worst_ratio(o, t, b) for o, t, b in zip(out, tr, bd)]
                worst = [max(a, b) for a, b in zip(worst, r)]
                if pl is None:
                    assert out[2] == 0.0 and out[0] == out[1]
                assert max(r) <= 1.0, (numel, B, chw, pl is not None, out, tr, r)
    print(f"[step_chain] nelbo_fwd numel={numel} ({C.nelbo_parts(numel)} parts): worst |got - truth| / bound (total, recon, prior) "
          f"{[round(w, 3) for w in worst]}")
    # a NaN in pred reaches the loss: the step guard watches out[0]
    pred = pred.clone()
    pred[numel // 2] = C.NAN
    out = nelbo_fwd(lib, pred.cuda(), td, numel, prd, B, 3072.0)
    assert out[0] != out[0] and out[1] != out[1] and out[2] == out[2]


def test_nelbo_fwd_refusals(lib):
    L_ = _L()
    pred, target, prior = C.nelbo_inputs(1025, 257)
    pd, td, prd = pred.cuda(), target.cuda(), prior.cuda()
    Ww, wd = band(torch.full((lib.otvae_nelbo_ws(),), C.NAN, dtype=F64))
    Wo, od = band(3)
    for a in ((None, td, 5, 1, 1.0, wd, od), (pd, None, 5, 1, 1.0, wd, od), (pd, td, 0, 1, 1.0, wd, od), (pd, td, 5, 0, 1.0, wd, od),
              (pd, td, 5, 1, 0.0, wd, od), (pd, td, 5, 1, 1.0, None, od), (pd, td, 5, 1, 1.0, wd, None)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_nelbo_fwd(L_.ptr(a[0]), L_.ptr(a[1]), a[2], L_.ptr(prd), a[3], a[4], L_.ptr(a[5]), L_.ptr(a[6]), L_.stream()),
                     "otvae_nelbo_fwd")
    assert bool((od.cpu() == C.SENT).all())


@pytest.mark.parametrize("numel", C.NELBO_BWD_NUMEL)
def test_nelbo_bwd(lib, numel):
    L_ = _L()
    worst = [0.0, 0.0]
    for B in C.NELBO_B:
        pred, target, _ = C.nelbo_inputs(numel, B)
        pd, td = pred.cuda(), target.cuda()
        for chw in C.NELBO_CHW:
            for gout in (None, C.NELBO_GOUT):
                for with_prior in (False, True):
                    god = None if gout is None else torch.tensor(gout, dtype=F32).cuda()
                    Wg, gpd = band(numel)
                    Wq, gqd = band(B)
                    L_.check(lib.otvae_nelbo_bwd(L_.ptr(pd), L_.ptr(td), numel, B, chw, L_.ptr(god), L_.ptr(gpd),
                                                 L_.ptr(gqd) if with_prior else None, L_.stream()), "otvae_nelbo_bwd")
                    (tp, tq), (bp, bq) = C.nelbo_bwd_truth(pred, target, B, chw, gout)
                    r = [C.worst_ratio(gpd, tp, bp), C.worst_ratio(gqd, tq, bq) if with_prior else 0.0]
                    worst = [max(a, b) for a, b in zip(worst, r)]
                    assert C.bands_intact(Wg) and C.bands_intact(Wq)
                    if not with_prior:
                        assert bool((gqd.cpu() == C.SENT).all())
                    assert max(r) <= 1.0, (numel, B, chw, gout, with_prior, r)
    print(f"[step_chain] nelbo_bwd numel={numel}: worst |got - truth| / bound (gpred, gprior) {[round(w, 3) for w in worst]}")
    Wg, gpd = band(numel)
    for a in ((None, td, numel, 1, gpd), (pd, None, numel, 1, gpd), (pd, td, 0, 1, gpd), (pd, td, numel, 0, gpd), (pd, td, numel, 1, None)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_nelbo_bwd(L_.ptr(a[0]), L_.ptr(a[1]), a[2], a[3], 1.0, None, L_.ptr(a[4]), None, L_.stream()), "otvae_nelbo_bwd")
    assert bool((gpd.cpu() == C.SENT).all())


# ---------------------------------------------------------------------------------------------------------------- 6. otvae_copy_batched
def copy_args(count, sd, dd, skip_src=None, zero_len=None):
    lengths, soff, doff, _, _ = C.copy_layout(count)
    P, N = ctypes.c_void_p * count, ctypes.c_int64 * count
    esz = sd.element_size()
    src = P(*[None if i == skip_src else sd.data_ptr() + esz * o for i, o in enumerate(soff)])
    dst = P(*[dd.data_ptr() + esz * o for o in doff])
    cnt = N(*[0 if i == zero_len else n for i, n in enumerate(lengths)])
    return src, dst, cnt


@pytest.mark.parametrize("count", C.COPY_COUNTS)
def test_copy_batched(lib, count):
    L_ = _L()
    lengths, soff, doff, stotal, dtotal = C.copy_layout(count)
    src = C.randn32(stotal, 6000 + count)
    sd = src.cuda()
    dd = torch.full((dtotal,), C.SENT, dtype=F32, device="cuda")
    s, d, c = copy_args(count, sd, dd)
    L_.check(lib.otvae_copy_batched(count, s, d, c, L_.stream()), "otvae_copy_batched")
    got, want = dd.cpu(), C.copy_expected(count, src)
    diff = int((got.view(I32) != want.view(I32)).sum())
    print(f"[step_chain] copy_batched count={count} (lengths {min(lengths)} .. {max(lengths)}, {sum(lengths)} elements): {diff} words of "
          f"the destination buffer, gaps and bands included, differ from the expected image")
    assert diff == 0 and C.bits_equal(sd.cpu(), src)


def test_copy_batched_refuses_an_entry_by_its_index(lib):
    """an entry of length 0 or a NULL entry: refused on the host with the entry's index; launches of earlier chunks of 32 have
    been issued by then, so only a bad entry of the FIRST chunk leaves the destination untouched"""
    L_ = _L()
    count = 33
    _, _, _, stotal, dtotal = C.copy_layout(count)
    sd = C.randn32(stotal, 6100).cuda()
    dd = torch.full((dtotal,), C.SENT, dtype=F32, device="cuda")
    for kw, idx in ((dict(zero_len=7), 7), (dict(skip_src=31), 31), (dict(zero_len=0), 0)):
        s, d, c = copy_args(count, sd, dd, **kw)
        with pytest.raises(ValueError, match=rf"entry {idx}\b"):
            L_.check(lib.otvae_copy_batched(count, s, d, c, L_.stream()), "otvae_copy_batched")
    assert bool((dd.cpu() == C.SENT).all())
    s, d, c = copy_args(count, sd, dd)
    for a in ((0, s, d, c), (-1, s, d, c), (count, None, d, c), (count, s, None, c), (count, s, d, None)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_copy_batched(*a, L_.stream()), "otvae_copy_batched")
    assert bool((dd.cpu() == C.SENT).all())
    s, d, c = copy_args(count, sd, dd, zero_len=32)           # the second chunk's only entry
    with pytest.raises(ValueError, match=r"entry 32\b"):
        L_.check(lib.otvae_copy_batched(count, s, d, c, L_.stream()), "otvae_copy_batched")


# ---------------------------------------------------------------------------------------------------------------- 7. step_begin / zero_words
def words(n):
    """n int64 words of a non-zero pattern between bands, 16-byte aligned"""
    W, w = band(torch.arange(1, n + 1, dtype=I64) * 0x0101010101 + 5)
    assert n == 0 or w.data_ptr() % 16 == 0
    return W, w


@pytest.mark.parametrize("n,zero_words", C.STEP_BEGIN_CASES)
def test_step_begin(lib, n, zero_words):
    L_ = _L()
    state = C.randn32(max(n, 1), 7000)[:n]
    (Ws, sd), (Wb, bd), (Wt, td), (Wz, zd) = band(state), band(n), ints(41), words(zero_words)
    L_.check(lib.otvae_step_begin(L_.ptr(td), L_.ptr(sd) if n else None, L_.ptr(bd) if n else None, n, L_.ptr(zd) if zero_words else None,
                                  zero_words, L_.stream()), "otvae_step_begin")
    wrong_b = int((bd.cpu().view(I32) != state.view(I32)).sum())
    nonzero = int((zd.cpu() != 0).sum())
    print(f"[step_chain] step_begin n={n} zero_words={zero_words} (grid {C.step_begin_grid(n, zero_words)}): counter {td.tolist()}, "
          f"{wrong_b} backup words differ, {nonzero} words not zero")
    assert td.tolist() == [42] and wrong_b == 0 and nonzero == 0
    assert C.bits_equal(sd.cpu(), state)
    assert all(C.bands_intact(W) for W in (Ws, Wb, Wt, Wz))


@pytest.mark.parametrize("zero_words", sorted({z for _, z in C.STEP_BEGIN_CASES if z}))
def test_zero_words(lib, zero_words):
    L_ = _L()
    Wz, zd = words(zero_words)
    L_.check(lib.otvae_zero_words(L_.ptr(zd), zero_words, L_.stream()), "otvae_zero_words")
    nonzero = int((zd.cpu() != 0).sum())
    print(f"[step_chain] zero_words {zero_words}: {nonzero} words not zero")
    assert nonzero == 0 and C.bands_intact(Wz)


def test_step_begin_and_zero_words_refusals(lib):
    L_ = _L()
    state = C.randn32(5, 7001)
    (Ws, sd), (Wb, bd), (Wt, td), (Wz, zd) = band(state), band(5), ints(41), words(8)
    z0 = zd.cpu().clone()
    off8 = zd[1:]                 # 8 bytes off a 16-byte boundary
    assert off8.data_ptr() % 16 == 8
    bad = {"odd word count": (td, sd, bd, 5, zd, 3), "zero pointer 8 bytes off": (td, sd, bd, 5, off8, 2), "negative n": (td, sd, bd, -1, zd, 2),
           "negative word count": (td, sd, bd, 5, zd, -2), "words without a pointer": (td, sd, bd, 5, None, 2),
           "no counter": (None, sd, bd, 5, zd, 2), "n without state": (td, None, bd, 5, zd, 2), "n without backup": (td, sd, None, 5, zd, 2)}
    for what, a in bad.items():
        with pytest.raises(ValueError):
            L_.check(lib.otvae_step_begin(L_.ptr(a[0]), L_.ptr(a[1]), L_.ptr(a[2]), a[3], L_.ptr(a[4]), a[5], L_.stream()), "otvae_step_begin")
    for a in ((zd, 3), (off8, 2), (zd, 0), (zd, -2), (None, 2)):
        with pytest.raises(ValueError):
            L_.check(lib.otvae_zero_words(L_.ptr(a[0]), a[1], L_.stream()), "otvae_zero_words")
    assert td.tolist() == [41] and bool((bd.cpu() == C.SENT).all()) and torch.equal(zd.cpu(), z0)
    assert all(C.bands_intact(W) for W in (Ws, Wb, Wt, Wz))


# ---------------------------------------------------------------------------------------------------------------- 8. the chain
def test_chain_against_torch_adam_and_clip_grad_norm(lib):
    """five steps of step_begin -> grad_clip_coef -> adam_step with the step guard; the third gradient holds a NaN and is refused.
    Truth: torch.optim.Adam and clip_grad_norm_ in float64 on the host, skipping the same step."""
    L_ = _L()
    n, ns = C.CHAIN_N, C.CHAIN_N_STATE
    p0, grads = C.chain_inputs()
    steps = C.chain_truth()
    zeros = torch.zeros(n)
    (Wp, pd), (Wm, md), (Wv, vd), (Wt, td), (Wq, qd) = band(p0), band(zeros), band(zeros), ints(0), ints(0, 0)
    (Wst, std), (Wb, bd) = band(C.randn32(ns, 8200)), band(ns)
    Ww, wd = band(torch.full((lib.otvae_grad_clip_ws(),), C.NAN, dtype=F64))
    Wo, od = band(2)
    skips = 0
    for k, (g, tr) in enumerate(zip(grads, steps)):
        Wg, gd = band(g)
        running = C.randn32(ns, 8300 + k)              # what the step's forward pass would leave in the running buffers
        L_.check(lib.otvae_step_begin(L_.ptr(td), L_.ptr(std), L_.ptr(bd), ns, None, 0, L_.stream()), "otvae_step_begin")
        before = std.cpu().clone()
        std.copy_(running.cuda())
        L_.check(lib.otvae_grad_clip_coef(L_.ptr(gd), n, 1.0, C.CHAIN_MAX_NORM, L_.ptr(wd), L_.ptr(od), L_.stream()), "otvae_grad_clip_coef")
        adam(lib, pd, gd, md, vd, td, scale_dev=od, guard=qd, state=std, backup=bd, n_state=ns)
        out = od.cpu().double().tolist()
        r = dict(p=C.worst_ratio(pd, tr["p"], tr["Ep"]), m=C.worst_ratio(md, tr["m"], tr["Em"]), v=C.worst_ratio(vd, tr["v"], tr["Ev"]))
        print(f"[step_chain] chain step {k + 1}: scale, norm = {out}, counter {td.tolist()}, guard {qd.tolist()}, "
              f"|got - torch fp64| / accumulated bound {r}")
        assert td.tolist() == [tr["t"]]
        if tr["skipped"]:
            skips += 1
            assert out[1] != out[1] and qd.tolist() == [skips, tr["t"] + 1]
            assert C.bits_equal(std.cpu(), before), "the refused step did not put the running state back"
        else:
            assert C.bits_equal(std.cpu(), running)
            assert C.worst_ratio(out[0], tr["scale"], tr["dscale"]) <= 1.0 and C.worst_ratio(out[1], tr["norm"], tr["dnorm"]) <= 1.0
            if tr["scale"] == 1.0:
                assert out[0] == 1.0
        assert max(r.values()) <= 1.0, (k, r)
        assert all(C.bands_intact(W) for W in (Wp, Wm, Wv, Wt, Wq, Wst, Wb, Ww, Wo, Wg))
    assert td.tolist() == [4] and qd.tolist() == [1, 3]
