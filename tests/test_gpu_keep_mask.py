"""GPU: ``otvae_dropout_keep_mask`` (through ``functional._keep_mask``) against a host copy of the hash of ``csrc/dropout_hash.h``.
Integer arithmetic on both sides: exact equality, no tolerance.  ``used`` is set by the test; no forward pass is needed."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PS = (0.0, 0.1, 0.9)
USED = (0, 1, 0x0123456789ABCDEF, -1, -2 ** 63)   # the negative values: the kernel reads int64 and hashes it as uint64


def mix32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def dropout_threshold(p):
    return min(int(float(np.float32(p)) * 4294967296.0), 2 ** 32 - 1)


def host_keep(used, rows, cols, p):
    """bool [rows, cols]: keep_pair(row_hash(uint64(used), row), col, dropout_threshold(p))"""
    ck = np.uint64(used & (2 ** 64 - 1))
    lo, hi = np.uint32(ck & np.uint64(0xFFFFFFFF)), np.uint32(ck >> np.uint64(32))
    rh = mix32(np.arange(rows, dtype=np.uint32) ^ lo) ^ hi
    h = mix32(rh[:, None] + np.arange(cols, dtype=np.uint32)[None, :] * np.uint32(0x9E3779B9))
    return h.astype(np.uint64) >= np.uint64(dropout_threshold(p))


def device_used(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("rows,cols", [(1, 1), (3, 257), (777, 5), (70000, 1)])
def test_keep_mask_equals_the_host_hash(rows, cols):
    """one element; a column count that is no multiple of the block; a row count that is none; a row index above 16 bits"""
    import ot_vae_lightning_amd.functional as HF
    for used in USED:
        u = device_used(used)
        for p in PS:
            got = HF._keep_mask(u, rows, cols, p)
            assert got.dtype == torch.bool and tuple(got.shape) == (rows, cols)
            want = host_keep(used, rows, cols, p)
            assert np.array_equal(got.cpu().numpy(), want), (rows, cols, p, used)
            if p == 0.0:
                assert bool(got.all())


def test_public_helpers_reshape_the_same_call():
    import ot_vae_lightning_amd.functional as HF
    u, p = device_used(0x0123456789ABCDEF), 0.1
    n, h, t = 2, 3, 20
    assert torch.equal(HF.attention_dropout_mask(u, n, t, h, p), HF._keep_mask(u, n * h * t, t, p).reshape(n, h, t, t))
    n, h, tq, tk = 2, 2, 7, 13
    assert torch.equal(HF.attention_cross_mask(u, n, tq, tk, h, p), HF._keep_mask(u, n * h * tq, tk, p).reshape(n, h, tq, tk))
    m, d = 37, 100
    got = HF.layer_norm_dropout_mask(u, m, d, p)
    assert tuple(got.shape) == (m, d) and torch.equal(got, HF._keep_mask(u, m, d, p))
    n, c = 5, 16
    got = HF.dropout2d_mask(u, n, c, p)
    assert tuple(got.shape) == (n, c) and torch.equal(got, HF._keep_mask(u, n, c, p))


def test_attention_mask_beyond_the_attention_kernels_token_limit():
    """T = 300: past what the attention kernels' LDS plan takes, which the mask (no LDS) never needed"""
    import ot_vae_lightning_amd.functional as HF
    used, n, h, t, p = -1, 1, 2, 300, 0.1
    got = HF.attention_dropout_mask(device_used(used), n, t, h, p)
    assert tuple(got.shape) == (n, h, t, t)
    assert np.array_equal(got.cpu().numpy(), host_keep(used, n * h * t, t, p).reshape(n, h, t, t))
