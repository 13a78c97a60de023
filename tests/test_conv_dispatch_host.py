"""CPU: the argument checks of a convolution job are one function, whichever entry point the job comes through.

Every row below is a malformed job that the library refuses before any HIP call, so the table runs without a GPU.  Where the one-job
entry point (``otvae_conv_fwd`` / ``otvae_conv_bwd_data`` / ``otvae_conv_bwd_weight``) can express the row, it and ``otvae_conv_multi``
with that single job must return the same code; rows that need a field only ``otvae_conv_job`` has (statistic slots, a BatchNorm fold,
the kind itself) go through ``otvae_conv_multi`` alone.  The error text names the entry point that was called.
"""
import ctypes as C

import pytest

EINVAL = -1     # OTVAE_EINVAL (include/otvae.h)
BN_TAB = 1024   # channels a folded BatchNorm may have (csrc/common.h)
P = 0x10000     # a non-NULL, 16-byte aligned address; never dereferenced: every row is refused on the host


@pytest.fixture(scope="module")
def L():
    from ot_vae_lightning_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    return _lib


def good_job(L, kind, cs=8):
    """A complete job of the kind on an 8x8 map, 3x3 s1 p1, cs -> 8 channels."""
    jb = L.ConvJob()
    jb.kind = kind
    jb.geom = L.ConvGeom(2, 8, 8, cs, 1, 8, 8, 8, 3, 3, 1, 1)
    if kind == L.JOB_FWD:
        jb.x, jb.w, jb.y = P, P, P
    elif kind == L.JOB_BWD_DATA:
        jb.gy, jb.w, jb.gv = P, P, P
    else:
        jb.x, jb.gy, jb.wpartial, jb.gw = P, P, P, P
    return jb


def fold(jb):
    f = jb.fold
    f.slots, f.ld, f.nslots, f.count, f.eps, f.momentum = P, jb.geom.Cs, 4, 128, 1e-5, 0.1
    f.gamma = f.beta = f.scale_out = f.shift_out = P


def one_job(L, jb):
    """The job through its one-job entry point -> (return code, entry point's name)."""
    lib, g = L.load(), C.byref(jb.geom)
    if jb.kind == L.JOB_FWD:
        return lib.otvae_conv_fwd(g, jb.x, jb.scale, jb.shift, jb.relu, jb.w, jb.bias, jb.residual, jb.y, jb.stat_partial, None), "otvae_conv_fwd"
    if jb.kind == L.JOB_BWD_DATA:
        return lib.otvae_conv_bwd_data(g, jb.gy, jb.w, jb.x, jb.scale, jb.shift, jb.relu, jb.mean, jb.invstd, jb.gv, jb.bn_partial,
                                       None), "otvae_conv_bwd_data"
    return lib.otvae_conv_bwd_weight(g, jb.x, jb.scale, jb.shift, jb.relu, jb.gy, jb.has_bias, jb.wpartial, jb.gw, jb.gb, jb.defer_reduce,
                                     None), "otvae_conv_bwd_weight"


def named(err):
    """The entry point an error text names: its first word."""
    return err.split(":")[0].split(" ")[0]


def setf(**kw):
    return lambda jb: [setattr(jb, k, v) for k, v in kw.items()]


FWD, DGRAD, WGRAD = 0, 1, 2
# (what, kind, edit of a good job, expressible through the one-job entry point)
ROWS = [
    ("forward: NULL x", FWD, setf(x=None), True),
    ("forward: NULL w", FWD, setf(w=None), True),
    ("forward: NULL y", FWD, setf(y=None), True),
    ("data gradient: NULL gy", DGRAD, setf(gy=None), True),
    ("data gradient: NULL w", DGRAD, setf(w=None), True),
    ("data gradient: NULL gv", DGRAD, setf(gv=None), True),
    ("weight gradient: NULL x", WGRAD, setf(x=None), True),
    ("weight gradient: NULL gy", WGRAD, setf(gy=None), True),
    ("weight gradient: NULL partial workspace", WGRAD, setf(wpartial=None), True),
    ("weight gradient: NULL gw", WGRAD, setf(gw=None), True),
    ("forward: scale without shift", FWD, setf(scale=P), True),
    ("data gradient: shift without scale", DGRAD, setf(shift=P), True),
    ("weight gradient: scale without shift", WGRAD, setf(scale=P), True),
    ("data gradient: mean without invstd", DGRAD, setf(x=P, mean=P, bn_partial=P), True),
    ("data gradient: invstd without mean", DGRAD, setf(x=P, invstd=P, bn_partial=P), True),
    ("data gradient: ReLU without x", DGRAD, setf(relu=1), True),
    ("data gradient: BatchNorm sums without x", DGRAD, setf(mean=P, invstd=P, bn_partial=P), True),
    ("data gradient: mean without partials or slots", DGRAD, setf(x=P, mean=P, invstd=P), True),
    ("data gradient: partials and slots both given", DGRAD, setf(x=P, mean=P, invstd=P, bn_partial=P, bn_slots=P, bn_nslots=4), False),
    ("data gradient: 3 slots in use", DGRAD, setf(x=P, mean=P, invstd=P, bn_slots=P, bn_nslots=3), False),
    ("forward: partials and slots both given", FWD, setf(stat_partial=P, stat_slots=P, stat_nslots=4), False),
    ("forward: 65 slots in use", FWD, setf(stat_slots=P, stat_nslots=65), False),
    ("forward: misaligned slots", FWD, setf(stat_slots=P + 8, stat_nslots=4), False),
    ("weight gradient: has_bias without gb", WGRAD, setf(has_bias=1), True),
    ("forward: fold with Cs > BN_TAB", FWD, fold, False),
    ("data gradient: fold", DGRAD, fold, False),
    ("weight gradient: fold", WGRAD, fold, False),
    ("data gradient: stat_slots", DGRAD, setf(stat_slots=P, stat_nslots=4), False),
    ("weight gradient: stat_slots", WGRAD, setf(stat_slots=P, stat_nslots=4), False),
    ("kind 3", FWD, setf(kind=3), False),
]


@pytest.mark.parametrize("what,kind,edit,single", ROWS, ids=[r[0] for r in ROWS])
def test_malformed_jobs_are_refused_alike(L, what, kind, edit, single):
    lib = L.load()
    jobs = (L.ConvJob * 1)()
    jobs[0] = good_job(L, kind, cs=2 * BN_TAB if "BN_TAB" in what else 8)
    edit(jobs[0])
    rc_multi = lib.otvae_conv_multi(1, jobs, None)
    err = L.last_error()
    assert rc_multi == EINVAL, (what, rc_multi, err)
    assert named(err) == "otvae_conv_multi", err
    if single:
        rc_one, entry = one_job(L, jobs[0])
        err = L.last_error()
        assert rc_one == rc_multi, (what, rc_one, err)
        assert named(err) == entry, err


def test_a_fold_within_the_table_passes_the_channel_check(L):
    """The BN_TAB row above is refused for its channel count, not for its descriptor: the same fold on BN_TAB channels with an
    incomplete descriptor is refused by the descriptor check, and a bad kind by the kind check."""
    lib = L.load()
    jobs = (L.ConvJob * 1)()
    jobs[0] = good_job(L, L.JOB_FWD, cs=2 * BN_TAB)
    fold(jobs[0])
    assert lib.otvae_conv_multi(1, jobs, None) == EINVAL and "at most %d channels" % BN_TAB in L.last_error()
    jobs[0] = good_job(L, L.JOB_FWD, cs=BN_TAB)
    fold(jobs[0])
    jobs[0].fold.gamma = None
    assert lib.otvae_conv_multi(1, jobs, None) == EINVAL and "fold descriptor" in L.last_error()
    jobs[0].kind = 3
    assert lib.otvae_conv_multi(1, jobs, None) == EINVAL and "kind" in L.last_error()
