"""CPU: the argument checks of ``otvae_layernorm_fwd`` / ``otvae_layernorm_bwd`` / ``otvae_dropout_keep_mask``.  Every call here is
one the entry point refuses BEFORE it launches anything (there is no GPU here): a non-zero return and a message naming the entry.
Pointers a case leaves valid are small non-null dummy addresses; nothing dereferences them."""
import pytest

P = 64       # a non-null dummy address
M, D = 8, 32


@pytest.fixture(scope="module")
def lib():
    from ot_vae_lightning_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def refused(lib, name, *args):
    rc = getattr(lib, name)(*args)
    msg = lib.otvae_last_error().decode()
    assert rc == -1, f"{name} returned {rc}: not refused by its argument check (OTVAE_EINVAL)"
    assert name in msg, msg


def ln_fwd(res=P, p=0.1, key=P, stream_id=0, sum_out=P, used=P):
    """a valid dropout call of otvae_layernorm_fwd, one argument at a time replaced by the case"""
    return (P, res, P, P, M, D, 1e-5, p, key, stream_id, sum_out, P, P, P, used, None)


@pytest.mark.parametrize("case", [dict(res=None), dict(used=None), dict(key=None, used=None), dict(key=None, used=None, p=0.0, sum_out=None),
                                  dict(p=1.0), dict(stream_id=4095)],
                         ids=["key-no-res", "key-no-used", "p-no-key", "res-no-sum_out", "p=1", "stream_id=4095"])
def test_layernorm_fwd_refusals(lib, case):
    refused(lib, "otvae_layernorm_fwd", *ln_fwd(**case))


@pytest.mark.parametrize("used,gx_dropped", [(P, None), (None, P)], ids=["used-no-gx_dropped", "gx_dropped-no-used"])
def test_layernorm_bwd_refusals(lib, used, gx_dropped):
    p = 0.1 if used else 0.0
    refused(lib, "otvae_layernorm_bwd", P, P, P, P, P, M, D, p, used, P, gx_dropped, P, P, P, None)


@pytest.mark.parametrize("rows,cols,p,used", [(2 ** 32, 4, 0.1, P), (4, 0, 0.1, P), (4, 4, 1.0, P), (4, 4, 0.1, None)],
                         ids=["rows=2^32", "cols=0", "p=1", "used-NULL"])
def test_keep_mask_refusals(lib, rows, cols, p, used):
    refused(lib, "otvae_dropout_keep_mask", rows, cols, p, used, P, None)
