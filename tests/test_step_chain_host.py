"""CPU: the host half of ``test_gpu_step_chain.py`` -- for every case of ``step_chain_cases`` the conditions its expectation rests on,
that the REFERENCE arithmetic alone (the kernels' operation order emulated in fp32 on the host) meets the bound the kernel will be
held to, and that each bound rejects a kernel with one plausible defect.  So the bounds are pinned to the number formats and are
neither loose enough to pass a wrong kernel nor tight enough to fail a right one.  No kernel runs."""
import math

import numpy as np
import pytest
import torch

import step_chain_cases as C

F32, F64 = C.F32, C.F64
HOST_N = 4099       # body and tail; the bounds are per element, so the size adds nothing on the host


def test_the_hyper_parameters_make_one_minus_beta_exact():
    lr, b1, b2, eps = C.hyper64()
    for b in (b1, b2):
        assert 0.5 <= b < 1.0                                           # Sterbenz: 1 - b is exact in fp32
        assert float(np.float32(1) - np.float32(b)) == 1.0 - b
        assert float(np.power(np.float32(b), np.float32(1))) == b       # t = 1: the bias corrections carry no pow error
    assert C.MARGIN <= 2.0
    assert float(np.float32(C.SENT)) == float(torch.tensor(C.SENT, dtype=F32))


# ---------------------------------------------------------------------------------------------------------------- 1. Adam
def test_adam_inputs_span_the_range_and_plant_the_zeros():
    for n in C.ADAM_N:
        g, m, v = C.adam_inputs(n)
        assert g.dtype == F32 and g.shape == m.shape == v.shape == (n,)
        assert bool((v >= 0).all())
    g, m, v = C.adam_inputs(HOST_N)
    for x in (g, m, v):
        nz = x[x != 0].abs()
        assert float(nz.min()) < 1e-5 and float(nz.max()) > 1e2 and float(nz.min()) >= 0.99e-6 and float(nz.max()) <= 1.01e3
    assert bool(((g == 0) & (m != 0)).any()) and bool(((m == 0) & (v != 0) & (g != 0)).any()) and bool(((m == 0) & (v == 0) & (g != 0)).any())
    assert float(g[-1]) == float(m[-1]) == float(v[-1]) == 0.0
    # the fresh parameter with a zero gradient: a zero update in the truth, with a zero bound
    tr = C.adam_truth(g, m, v, torch.zeros(HOST_N), 1.0, 1)
    b = C.adam_bounds(g, m, v, 1.0, 1, tr)
    assert float(tr["upd"][-1]) == 0.0 and float(b["upd"][-1]) == 0.0
    assert bool(torch.isfinite(tr["upd"]).all())


def test_adam_grid_cases():
    grids = [C.adam_grid(n) for n in C.ADAM_N]
    assert grids == [1, 1, 1, 1, 1, 1, 2, 5, 2048]
    n = C.ADAM_N[-1]
    assert n // 4 > C.ADAM_GRID_CAP * 256 and n % 4 == 3          # a second pass of the float4 loop, and a tail
    assert [n % 4 for n in C.ADAM_N[:4]] == [1, 3, 0, 1]


@pytest.mark.parametrize("s", C.ADAM_SCALES)
@pytest.mark.parametrize("t", C.ADAM_T + (3, 100, 10000))
def test_adam_emulation_meets_the_bounds(t, s):
    g, m, v = C.adam_inputs(HOST_N)
    worst = {}
    for name, p in (("p=0", torch.zeros(HOST_N)), ("generic p", C.generic_p(HOST_N))):
        tr = C.adam_truth(g, m, v, p, s, t)
        b = C.adam_bounds(g, m, v, s, t, tr)
        em = C.adam_emulate(g, m, v, p, s, t)
        worst[name] = dict(m=C.worst_ratio(em["m"], tr["m"], b["m"]), v=C.worst_ratio(em["v"], tr["v"], b["v"]),
                           p=C.worst_ratio(em["p"], tr["p"], C.p_bound(tr, b["upd"])))
        if name == "p=0":
            worst[name]["upd"] = C.worst_ratio(em["upd"], tr["upd"], b["upd"])
            assert torch.equal(em["p"], -em["upd"])
            relu, common = C.rel_err(em["upd"], tr["upd"]), C.median_rel_err(em["upd"], tr["upd"])
            assert common <= relu
    print(f"[step_chain] host adam t={t} s={s}: fp32 emulation / bound {worst}, relative update error: largest {relu:.3e}, "
          f"median {common:.3e}")
    assert max(max(w.values()) for w in worst.values()) <= 1.0


@pytest.mark.parametrize("defect", C.ADAM_DEFECTS)
def test_adam_bounds_reject_single_defects(defect):
    g, m, v = C.adam_inputs(HOST_N)
    p = torch.zeros(HOST_N)
    # where fp64 itself can tell: t - 1 = t and bc2 = 1 to every digit at t = 100000; the scale shows at s != 1
    ts = {"t-1": (1, 2, 10, 1000), "no bc2": (1, 2, 10, 1000)}.get(defect, C.ADAM_T)
    ss = (0.5,) if defect == "scale twice" else C.ADAM_SCALES
    for t in ts:
        for s in ss:
            tr = C.adam_truth(g, m, v, p, s, t)
            b = C.adam_bounds(g, m, v, s, t, tr)
            bad = C.adam_truth(g, m, v, p, s, t, defect=defect)
            r = {k: C.worst_ratio(bad[k], tr[k], b[k]) for k in ("m", "v", "upd")}
            print(f"[step_chain] host adam defect '{defect}' t={t} s={s}: {r} of the bounds")
            assert max(r.values()) > 1.0, (defect, t, s, r)
            if defect == "tail unchanged":       # seen in the tail alone
                k = HOST_N - HOST_N % 4
                assert max(C.worst_ratio(bad[q][:k], tr[q][:k], b[q][:k]) for q in ("m", "v", "upd")) == 0.0


# ---------------------------------------------------------------------------------------------------------------- 2. guard
def test_guard_matrix():
    assert [C.guard_refuses(x) for x in C.GUARD_VALUES] == [False, True, True, True]
    assert C.adam_grid(C.GUARD_N) == 1 and max(C.GUARD_N_STATE) > 256 and 0 in C.GUARD_N_STATE


# ---------------------------------------------------------------------------------------------------------------- 3. EMA
def test_ema_rule_and_its_defect():
    s0, p = C.randn32(HOST_N, 31), C.randn32(HOST_N, 32)
    for decay in C.EMA_DECAYS:
        for t in C.EMA_T:
            d = min(decay, (1 + t) / (10 + t))
            want = s0 - (s0 - p) * (1.0 - d)          # torch's own fp32 operators: three roundings
            got = C.ema_rule(s0, p, decay, t)
            assert C.bits_equal(got, want), (decay, t)
            for off in (-1, 1):
                same = C.bits_equal(C.ema_rule(s0, p, decay, t, off_by=off), got)
                d_off = min(decay, (1 + t + off) / (10 + t + off))
                # one step off is seen exactly where it changes the fp32 factor: wherever the warm-up decides
                assert same == (np.float32(1.0 - d_off) == np.float32(1.0 - d)), (decay, t, off)
                if (1 + t) / (10 + t) < decay:
                    assert not same, (decay, t, off)
    assert (1 + 80) / (10 + 80) == 0.9 and (1 + 79) / (10 + 79) < 0.9 < (1 + 81) / (10 + 81)
    # decay 1 inside Adam is the warm-up for ever (min(1, (1 + t) / (10 + t)) < 1); the stand-alone kernel's decay 1 is a no-op
    assert not C.bits_equal(C.ema_rule(s0, p, 1.0, 1000), s0)
    assert C.bits_equal(C.ema_fixed_rule(s0, p, 1.0), s0)
    assert C.bits_equal(C.ema_fixed_rule(s0, p, 0.0), s0 - (s0 - p))
    assert C.bits_equal(C.ema_fixed_rule(s0, p, 0.9), C.ema_rule(s0, p, 0.9, 1000))


# ---------------------------------------------------------------------------------------------------------------- 4. clip
def test_clip_parts():
    assert [C.clip_parts(n) for n in C.CLIP_N] == [1, 1, 1, 1, 1, 2, 512]
    assert C.CLIP_N[-1] > 512 * 4096 and C.CLIP_N[-1] % 4 == 3


@pytest.mark.parametrize("n", C.CLIP_N)
def test_clip_emulation_meets_the_bounds_and_defects_miss_them(n):
    g = C.clip_gradient(n)
    assert C.clip_in_range(g)
    for s in C.CLIP_SCALES:
        norm = C.clip_truth(g, s, 0.0)[1]
        assert 0.01 < norm < 0.2
        for fac in C.CLIP_MAX_NORM_FACTORS:
            mx = float(np.float32(fac * norm))
            tr = C.clip_truth(g, s, mx)
            d0, d1 = C.clip_bounds(n, s, mx, tr)
            em = C.clip_emulate(g, s, mx)
            r0, r1 = C.worst_ratio(em[0], tr[0], d0), C.worst_ratio(em[1], tr[1], d1)
            print(f"[step_chain] host clip n={n} s={s} max_norm={fac} |g|: fp32 emulation / bound: scale {r0:.3f}, norm {r1:.3f}")
            assert r0 <= 1.0 and r1 <= 1.0
            if fac < 1.0 and fac > 0:
                assert tr[0] < s and d0 > 0
            else:
                assert tr[0] == s and d0 == 0.0 and em[0] == s          # not clipping: the scale is s itself
            bad = C.clip_truth(g, s, mx, defect="scale twice")
            assert (C.worst_ratio(bad[0], tr[0], d0) > 1.0) == (s != 1.0)
            bad = C.clip_truth(g, s, mx, defect="no 1e-6")
            assert (C.worst_ratio(bad[0], tr[0], d0) > 1.0) == (0 < fac < 1.0)


def test_clip_range_statement():
    g = C.clip_gradient(4097).clone()
    g[17] = 1e20
    assert not C.clip_in_range(g)
    assert math.isinf(C.clip_emulate(g, 1.0, 1.0)[1]) and C.clip_emulate(g, 1.0, 1.0)[0] == 0.0
    g[17] = C.NAN
    assert math.isnan(C.clip_emulate(g, 1.0, 1.0)[1])
    g[17] = 1e-30
    assert not C.clip_in_range(g)
    g[17] = 0.0
    assert C.clip_in_range(g)


# ---------------------------------------------------------------------------------------------------------------- 5. nelbo
def test_nelbo_parts():
    assert [C.nelbo_parts(n) for n in C.NELBO_FWD_NUMEL] == [1, 1, 1, 2, 256]
    assert C.NELBO_FWD_NUMEL[-1] > 256 * 1024
    assert C.NELBO_BWD_NUMEL[-1] > 2048 * 256 and max(C.NELBO_B) > 256
    assert all(float(np.float32(n)) == n for n in C.NELBO_BWD_NUMEL)          # (float) numel is exact


@pytest.mark.parametrize("numel", C.NELBO_FWD_NUMEL)
def test_nelbo_fwd_emulation_meets_the_bounds(numel):
    for B in C.NELBO_B:
        pred, target, prior = C.nelbo_inputs(numel, B)
        for chw in C.NELBO_CHW:
            for pl in (None, prior):
                tr, bd = C.nelbo_fwd_truth(pred, target, pl, chw)
                em = C.nelbo_fwd_emulate(pred, target, pl, chw)
                r = [C.worst_ratio(e, t, b) for e, t, b in zip(em, tr, bd)]
                print(f"[step_chain] host nelbo_fwd numel={numel} B={B} chw={chw} prior={'given' if pl is not None else 'NULL'}: "
                      f"fp32 emulation / bound (total, recon, prior) {r}")
                assert max(r) <= 1.0
                if pl is None:
                    assert tr[2] == 0.0 and bd[2] == 0.0 and em[2] == 0.0
                elif chw != 1.0:
                    bad, _ = C.nelbo_fwd_truth(pred, target, pl, chw, defect="prior not divided by chw")
                    assert C.worst_ratio(bad[0], tr[0], bd[0]) > 1.0 and C.worst_ratio(bad[2], tr[2], bd[2]) > 1.0


@pytest.mark.parametrize("numel", C.NELBO_BWD_NUMEL)
def test_nelbo_bwd_emulation_meets_the_bounds(numel):
    B, chw = 257, 3072.0
    pred, target, _ = C.nelbo_inputs(numel, B)
    for gout in (None, C.NELBO_GOUT):
        (gp, gq), (bp, bq) = C.nelbo_bwd_truth(pred, target, B, chw, gout)
        ep, eq = C.nelbo_bwd_emulate(pred, target, B, chw, gout)
        r = (C.worst_ratio(ep, gp, bp), C.worst_ratio(eq, gq, bq))
        print(f"[step_chain] host nelbo_bwd numel={numel} gout={gout}: fp32 emulation / bound (gpred, gprior) {r}")
        assert max(r) <= 1.0
        (bad, _), _ = C.nelbo_bwd_truth(pred, target, B, chw, gout, defect="1/numel")
        assert C.worst_ratio(bad, gp, bp) > 1.0
    g0, g1, g2 = C.NELBO_GOUT
    assert g0 + g1 != 0 and g0 + g2 != 0 and g0 + g1 != g0 + g2 != 1.0


# ---------------------------------------------------------------------------------------------------------------- 6. copy
@pytest.mark.parametrize("count", C.COPY_COUNTS)
def test_copy_layout(count):
    lengths, soff, doff, stotal, dtotal = C.copy_layout(count)
    assert len(lengths) == count and min(lengths) >= 1 and max(lengths) == C.COPY_LONGEST
    assert -(-C.COPY_LONGEST // 1024) > 256           # the grid cap is reached
    if count > 1:
        chunk0 = lengths[:C.COPY_CHUNK]
        assert C.COPY_LONGEST in chunk0 and 1 in chunk0
    for i in range(count - 1):                        # disjoint, with a gap
        assert soff[i] + lengths[i] < soff[i + 1] and doff[i] + lengths[i] < doff[i + 1]
    assert doff[0] >= C.BAND and doff[-1] + lengths[-1] + C.BAND <= dtotal and soff[-1] + lengths[-1] <= stotal
    src = torch.arange(stotal, dtype=F32)
    exp = C.copy_expected(count, src)
    assert int((exp != C.SENT).sum()) == sum(lengths)


# ---------------------------------------------------------------------------------------------------------------- 7. step_begin
def test_step_begin_grids():
    assert [C.step_begin_grid(n, z) for n, z in C.STEP_BEGIN_CASES] == [1, 1, 1, 257, 1024]
    n, z = C.STEP_BEGIN_CASES[3]
    assert z % 2 == 0 and z // 2 > 257 * 256 - 1 and z // 2 > 256 * 1024        # more int4 than the grid has threads
    n, z = C.STEP_BEGIN_CASES[4]
    assert n > 1024 * 256


# ---------------------------------------------------------------------------------------------------------------- 8. chain
def test_chain_emulation_meets_the_accumulated_bounds():
    steps, em = C.chain_truth(), C.chain_emulate()
    assert [s["skipped"] for s in steps] == [False, False, True, False, False]
    assert [s["scale"] < 1.0 for s in steps if not s["skipped"]] == [True, False, True, False]      # clipping on some steps
    assert steps[-1]["t"] == 4 and em[-1]["t"] == 4
    for k, (s, e) in enumerate(zip(steps, em)):
        r = dict(p=C.worst_ratio(e["p"], s["p"], s["Ep"]), m=C.worst_ratio(e["m"], s["m"], s["Em"]), v=C.worst_ratio(e["v"], s["v"], s["Ev"]))
        print(f"[step_chain] host chain step {k + 1} (t={s['t']}, {'skipped' if s['skipped'] else 'scale %.4f' % s['scale']}): "
              f"fp32 emulation / accumulated bound {r}")
        assert max(r.values()) <= 1.0
    # the skipped step changes nothing, and the truth moves on every other one
    assert torch.equal(steps[2]["p"], steps[1]["p"]) and not torch.equal(steps[3]["p"], steps[2]["p"])
    # a chain that forgets to take the counter back (t = 4 in place of 3 on the fourth step) leaves the bound
    p0, grads = C.chain_inputs()
    s3 = steps[3]
    bad = C.adam_truth(grads[3], steps[2]["m"].float(), steps[2]["v"].float(), steps[2]["p"].float(), s3["scale"], 4)
    assert C.worst_ratio(bad["p"], s3["p"], s3["Ep"]) > 1.0
