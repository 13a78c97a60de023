"""CPU only: a digest of what the conv host dispatch plans, for comparing two builds of the library.

    python tools/conv_plan_digest.py                          # this tree's build
    OTVAE_LIB=libotvae_other.so python tools/conv_plan_digest.py   # another build, a file next to ot_vae_lightning_amd/_lib.py

Calls only the host queries (nothing here launches or touches a device): for every geometry of a grid the return code and every
output of ``otvae_conv_fwd_stats_ws``, ``otvae_conv_bwd_data_ws``, ``otvae_conv_bwd_weight_ws`` (has_bias 0 and 1),
``otvae_conv_dead_taps`` and ``otvae_conv_gemm_chunks`` (modes 0 and 1), once with no selection switch set and once under each of
``SWITCHES``.  Two builds whose digests agree size every workspace alike and send every geometry down the same route.

The grid: N x Cs x Cn x map x kernel x (stride, up) x pad, pad running over 0 .. max(KH, KW) - 1 wherever the output is not empty.
Combinations the library refuses (stride 2 with up 2, stride 2 on an odd map) are kept: their return codes are part of the digest.

Route counts.  Forward and data gradient: read from ``otvae_conv_gemm_chunks`` (served = implicit GEMM; its refusal names the direct
or the image-tile kernels).  The weight gradient has no such query, so its route is inferred, for the counts only: image-tile when
``OTVAE_NO_WTILE`` changes the number of split-K partials (a lower bound: the two numbers may coincide), otherwise direct when the
direct kernels take the layer and (taps, Cs, Cn) is one of ``SMALL_WGRAD`` (the shapes conv_small_wgrad_ok lists), else implicit GEMM.
The digest does not depend on that inference.  The run fails when one of the nine (kind, route) counts of the no-switch sweep is
zero: then the grid no longer reaches every branch of the planner.
"""
import ctypes as C
import hashlib
import multiprocessing as mp
import os
import struct
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SWITCHES = [None, "OTVAE_NO_TILE", "OTVAE_TILE_ALL", "OTVAE_NO_WTILE", "OTVAE_WTILE_ALL"]
BATCH = [1, 3, 5, 64, 1024]
CHANNELS = [1, 3, 4, 8, 16, 20, 32, 36, 40, 64, 128, 256]
MAPS = [(s, s) for s in (1, 2, 3, 4, 5, 6, 7, 8, 12, 16, 24, 32)] + [(6, 10), (2, 3), (8, 12), (1, 4), (4, 1), (16, 32)]
KERNELS = [(1, 1), (3, 3), (4, 4), (5, 5), (7, 7), (1, 4), (4, 1)]
STRIDE_UP = [(1, 1), (2, 1), (1, 2), (2, 2)]
SMALL_WGRAD = {(16, 1, 8), (9, 8, 1), (9, 1, 1), (1, 1, 3), (1, 1, 1), (1, 8, 1), (9, 3, 3), (1, 3, 3), (1, 3, 9), (1, 16, 3)}
KINDS, ROUTES = ("fwd", "dgrad", "wgrad"), ("direct", "tile", "gemm")


def spatial(hs, ws):
    """(kh, kw, stride, up, pad, ho, wo) of one map."""
    for kh, kw in KERNELS:
        for stride, up in STRIDE_UP:
            for pad in range(max(kh, kw)):
                ho = (hs * up + 2 * pad - kh) // stride + 1
                wo = (ws * up + 2 * pad - kw) // stride + 1
                if ho > 0 and wo > 0:
                    yield kh, kw, stride, up, pad, ho, wo


def sweep(item):
    """One (switch, N, map) cell of the grid -> (sha256 of its records, geometries, route counts)."""
    switch, n, (hs, ws) = item
    for s in SWITCHES[1:]:
        os.environ.pop(s, None)
    if switch:
        os.environ[switch] = "1"
    from ot_vae_lightning_amd import _lib
    lib = _lib.load()
    g = _lib.ConvGeom()
    gp = C.byref(g)
    a, b, m, la, lb = C.c_int(), C.c_int(), C.c_uint32(), C.c_int64(), C.c_int64()
    pa, pb, pm, pla, plb = C.byref(a), C.byref(b), C.byref(m), C.byref(la), C.byref(lb)
    rec, pack = bytearray(), struct.Struct("<18q").pack   # 18 numbers per geometry: return codes and outputs, in call order
    counts = {(k, r): 0 for k in KINDS for r in ROUTES}
    geoms = 0
    for kh, kw, stride, up, pad, ho, wo in spatial(hs, ws):
        for cs in CHANNELS:
            for cn in CHANNELS:
                g.N, g.Hs, g.Ws, g.Cs, g.up, g.Ho, g.Wo, g.Cn = n, hs, ws, cs, up, ho, wo, cn
                g.KH, g.KW, g.stride, g.pad = kh, kw, stride, pad
                geoms += 1
                out = []
                a.value = b.value = -1
                out += [lib.otvae_conv_fwd_stats_ws(gp, pa, pb), a.value, b.value]
                a.value = b.value = -1
                out += [lib.otvae_conv_bwd_data_ws(gp, pa, pb), a.value, b.value]
                wp = []
                for has_bias in (0, 1):
                    a.value = -1
                    out += [lib.otvae_conv_bwd_weight_ws(gp, has_bias, pa), a.value]
                    wp.append(a.value)
                m.value = 0xffffffff
                out += [lib.otvae_conv_dead_taps(gp, pm), m.value]
                route = {}
                for mode in (0, 1):
                    la.value = lb.value = -1
                    rc = lib.otvae_conv_gemm_chunks(gp, mode, pla, plb)
                    out += [rc, la.value, lb.value]
                    if rc == 0:
                        route[mode] = "gemm"
                    elif rc == -2:
                        err = _lib.last_error()
                        route[mode] = "direct" if "the direct" in err else "tile"
                rec += pack(*out)
                if out[0] != 0:
                    continue
                counts["fwd", route[0]] += 1
                counts["dgrad", route[1]] += 1
                if switch is None:   # the weight gradient's route, inferred (module docstring)
                    os.environ["OTVAE_NO_WTILE"] = "1"
                    lib.otvae_conv_bwd_weight_ws(gp, 1, pa)
                    del os.environ["OTVAE_NO_WTILE"]
                    if a.value != wp[1]:
                        counts["wgrad", "tile"] += 1
                    elif route[0] == "direct" and (kh * kw, cs, cn) in SMALL_WGRAD:
                        counts["wgrad", "direct"] += 1
                    else:
                        counts["wgrad", "gemm"] += 1
    return hashlib.sha256(bytes(rec)).digest(), geoms, counts


def main():
    from ot_vae_lightning_amd import _lib
    print("library:", _lib.LIB_PATH)
    items = [(s, n, hw) for s in SWITCHES for n in BATCH for hw in MAPS]
    with mp.Pool(min(16, os.cpu_count() or 1)) as pool:
        results = pool.map(sweep, items, chunksize=1)
    total = hashlib.sha256()
    per_switch = {s: {(k, r): 0 for k in KINDS for r in ROUTES} for s in SWITCHES}
    geoms = 0
    for (s, _, _), (digest, ng, counts) in zip(items, results):
        total.update(digest)
        geoms += ng
        for key, v in counts.items():
            per_switch[s][key] += v
    print(f"{geoms} geometry records ({geoms // len(SWITCHES)} geometries x {len(SWITCHES)} sweeps)")
    for s in SWITCHES:
        kinds = KINDS if s is None else KINDS[:2]
        print(f"  {s or 'no switch':16s} " + "  ".join(
            f"{k}: " + " ".join(f"{r} {per_switch[s][k, r]}" for r in ROUTES) for k in kinds))
    print("sha256", total.hexdigest())
    empty = [key for key, v in per_switch[None].items() if v == 0]
    if empty:
        sys.exit(f"the no-switch sweep reaches no geometry on: {empty}")


if __name__ == "__main__":
    main()
