"""Times vra_moe_route and vra_moe_experts at the Qwen3-30B-A3B layer shape (H 2048, I 768, E 128, top-k 8, bf16) under uniform random routing,
HIP events, the decode and the tiled path alternating inside one process where both can run (T <= 32).  Routing rotates through a pool of
id sets, so consecutive calls stream different experts: with 1.2 GB of expert weights against a 256 MB last-level cache the small-T rows
are HBM numbers.  Two bounds per row, and the achieved fraction of each:
  HBM   bytes of the DISTINCT ACTIVE experts' weights + x + h (written, read) + y (written, read) + out, over 8 TB/s;
  MFMA  2 * pairs * 3 * H * I FLOP over the dense 16-bit peak, 2.5 PFLOP/s.
    python tools/moe_bench.py > profiles/moe_shapes.txt
With `mxfp4` as its argument it times vra_moe_mxfp4_experts instead: both of its paths and, in the same alternating rounds of the same
process, the 16-bit block on its default switch (the yardstick), on the same rotating id pool; the HBM bound is recomputed at 0.53 B per
weight (a 4-bit code + one scale byte per 32).
    python tools/moe_bench.py mxfp4 > profiles/moe_mxfp4_shapes.txt"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllm_rs_amd import ops  # noqa: E402

L = ops.lib()
H, I, E, TOPK, DT = 2048, 768, 128, 8, ops.BF16
TOKENS = [1, 4, 16, 32, 33, 64, 128, 512, 2048, 8192]
ROUNDS = 5
HBM, MFMA = 8e12, 2.5e15
MX4 = sys.argv[1:] == ["mxfp4"]
assert MX4 or not sys.argv[1:], "usage: moe_bench.py [mxfp4]"


def timed(fn, n):
    e0, e1 = L.vra_event_create(), L.vra_event_create()
    L.vra_event_record(e0, 0)
    for i in range(n):
        fn(i)
    L.vra_event_record(e1, 0)
    L.vra_device_sync()
    us = L.vra_event_elapsed_ms(e0, e1) * 1e3 / n
    L.vra_event_destroy(e0), L.vra_event_destroy(e1)
    return us


def normal(n, std, seed):
    b = ops.DevBuf(n * 2)
    L.vra_fill_normal(b.ptr, n, seed, 0.0, std, DT, 0)
    return b


gate_up, down = normal(2 * E * I * H, H ** -0.5, 1), normal(E * H * I, I ** -0.5, 2)  # random weights are random in any layout: filled as tiles
ws = ops.DevBuf(L.vra_moe_workspace_bytes(max(TOKENS), E, TOPK, H, I))
if MX4:  # uniform codes as tiles; every scale byte 2^-7 (gate/up) | 2^-6 (down): weights of std ~ 1 / sqrt(K)
    q_gu, s_gu, q_dn, s_dn = (ops.DevBuf(E * I * H // d) for d in (1, 16, 2, 32))
    L.vra_fill_hash_u32(q_gu.ptr, q_gu.nbytes // 4, 11, 0), L.vra_fill_const_u32(s_gu.ptr, s_gu.nbytes // 4, 0x78787878, 0)
    L.vra_fill_hash_u32(q_dn.ptr, q_dn.nbytes // 4, 12, 0), L.vra_fill_const_u32(s_dn.ptr, s_dn.nbytes // 4, 0x79797979, 0)
    print("# us per call, median of %d alternating rounds; H %d I %d E %d top-k %d bf16, uniform random routing; MXFP4 experts %.0f MiB, 16-bit %.0f MiB" %
          (ROUNDS, H, I, E, TOPK, (q_gu.nbytes + s_gu.nbytes + q_dn.nbytes + s_dn.nbytes) / 2 ** 20, (gate_up.nbytes + down.nbytes) / 2 ** 20))
    print("# 16-bit = vra_moe_experts on its default switch in the same rounds; HBM us = the bound at 0.53 B per weight; frac = that bound / the time")
    print("# of the MXFP4 path the default switch takes; x = 16-bit time / that time")
    print("%6s %7s | %9s %9s | %9s | %9s %5s | %5s" % ("T", "active", "decode", "tiled", "16-bit", "HBM us", "frac", "x"))
else:
    print("# us per call, median of %d alternating rounds; H %d I %d E %d top-k %d bf16, uniform random routing; workspace %.0f MiB" %
          (ROUNDS, H, I, E, TOPK, ws.nbytes / 2 ** 20))
    print("# bound = max(HBM bound, MFMA bound) in us; frac = bound / time of the path the default switch takes")
    print("%6s %7s | %8s | %9s %9s | %9s %9s | %s" % ("T", "active", "route", "decode", "tiled", "HBM us", "MFMA us", "frac of the larger bound (which)"))
r = np.random.default_rng(0)
for T in TOKENS:
    sets = max(2, min(16, 4096 // T))
    idsets = [np.argsort(r.random((T, E)), 1)[:, :TOPK].astype(np.uint32) for _ in range(sets)]
    active = float(np.mean([np.unique(s).size for s in idsets]))
    ids = [ops.dev(s) for s in idsets]
    tw = ops.dev(np.full((T, TOPK), 1.0 / TOPK, np.float32))
    x, out = normal(T * H, 1.0, 3), ops.DevBuf(T * H * 2)
    logits, rw, ri = ops.dev(r.standard_normal((T, E)).astype(np.float32)), ops.DevBuf(T * TOPK * 4), ops.DevBuf(T * TOPK * 4)

    def route(i):
        L.vra_moe_route(logits.ptr, rw.ptr, ri.ptr, T, E, TOPK, 1, 1.0, 0)

    def experts(rows):
        def fn(i):
            L.vra_debug_set_moe_decode_max_rows(rows)
            L.vra_moe_experts(x.ptr, gate_up.ptr, down.ptr, tw.ptr, ids[i % sets].ptr, None, out.ptr, ws.ptr, T, E, TOPK, H, I, DT, 0)
        return fn

    def experts_mx4(rows):
        def fn(i):
            L.vra_debug_set_moe_mxfp4_decode_max_rows(rows)
            L.vra_moe_mxfp4_experts(x.ptr, q_gu.ptr, s_gu.ptr, q_dn.ptr, s_dn.ptr, tw.ptr, ids[i % sets].ptr, None, out.ptr, ws.ptr, T, E, TOPK, H, I, DT, 0)
        return fn

    if MX4:
        variants = [("16-bit", experts(32)), ("tiled", experts_mx4(0))] + ([("decode", experts_mx4(32))] if T <= 32 else [])
    else:
        variants = [("route", route), ("tiled", experts(0))] + ([("decode", experts(32))] if T <= 32 else [])
    pairs = T * TOPK
    n = max(4, min(200, int(4e11 / (6.0 * pairs * H * I))))
    t = {v: [] for v, _ in variants}
    for rnd in range(ROUNDS + 1):  # round 0 warms every variant up
        for v, fn in variants:
            us = timed(fn, n)
            if rnd:
                t[v].append(us)
    L.vra_debug_set_moe_decode_max_rows(32), L.vra_debug_set_moe_mxfp4_decode_max_rows(32)
    ops.check_error()
    med = {v: sorted(ts)[len(ts) // 2] for v, ts in t.items()}
    wbytes = (0.5 + 1 / 32) if MX4 else 2  # per weight
    hbm = (active * 3 * H * I * wbytes + 2 * T * H * 2 + 2 * pairs * I * 2 + 2 * pairs * H * 4) / HBM * 1e6
    mfma = 2.0 * pairs * 3 * H * I / MFMA * 1e6
    took = med.get("decode", med["tiled"])
    if MX4:
        print("%6d %7.1f | %9s %9.1f | %9.1f | %9.1f %5.2f | %5.2f" %
              (T, active, "%.1f" % med["decode"] if "decode" in med else "-", med["tiled"], med["16-bit"], hbm, hbm / took, med["16-bit"] / took))
    else:
        print("%6d %7.1f | %8.1f | %9s %9.1f | %9.1f %9.1f | %.2f (%s)" %
              (T, active, med["route"], "%.1f" % med["decode"] if "decode" in med else "-", med["tiled"], hbm, mfma, max(hbm, mfma) / took,
               "HBM" if hbm >= mfma else "MFMA"))
    sys.stdout.flush()
