"""Times vra_fp8_gemm / vra_fp8_gate_up_silu on the Llama-3-8B widths against vra_dense_gemm on a 16-bit weight of the same shape
(dequantise + dense GEMM is the only other way to serve an FP8 checkpoint), HIP events, the variants of a shape alternating inside
one process.  Up to 32 rows both FP8 kernels are timed (streaming kernel | tile GEMM): their crossover is the dispatch threshold.
Weights rotate through a pool larger than the 256 MB last-level cache, so the small-row numbers are HBM numbers.
    python tools/fp8_gemm_bench.py > profiles/fp8_linear_gemm_shapes.txt"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vllm_rs_amd import ops  # noqa: E402

L = ops.lib()
SHAPES = [("q|k|v", 4096, 6144, False), ("o_proj", 4096, 4096, False), ("gate/up+SiLU", 4096, 14336, True), ("down", 14336, 4096, False)]
ROWS = [1, 4, 16, 32, 128, 512, 2048, 4096]
POOL_BYTES = 640 << 20
ROUNDS = 5


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


def fill(nbytes, seed):
    b = ops.DevBuf(nbytes)
    L.vra_fill_hash_u32(b.ptr, nbytes // 4, seed, 0)
    return b


print("# us per call, median of %d alternating rounds; TB/s of algorithmic bytes against 8 (rows <= 32), PFLOP/s against 2.5 (rows >= 128)" % ROUNDS)
print("%-13s %5s | %9s %9s %9s | %s" % ("shape", "rows", "fp8 gemv", "fp8 gemm", "dense16", "best fp8: rate (fraction of peak); dense: rate"))
for name, K, N, dual in SHAPES:
    nt = 2 if dual else 1
    copies = max(2, -(-POOL_BYTES // (K * N * nt)))
    w8 = [[fill(K * N, 11 * c + t) for t in range(nt)] for c in range(copies)]
    sc = [[ops.DevBuf((N // 128) * (K // 128) * 4) for t in range(nt)] for c in range(copies)]
    for c in range(copies):
        for t in range(nt):
            L.vra_fill_uniform(sc[c][t].ptr, (N // 128) * (K // 128), 5 + c + t, 1e-4, 4e-4, 2, 0)
    dcopies = max(2, -(-POOL_BYTES // (K * N * nt * 2)))
    w16 = [ops.DevBuf(K * N * nt * 2) for c in range(dcopies)]
    for c in range(dcopies):
        L.vra_fill_normal(w16[c].ptr, K * N * nt, 77 + c, 0.0, 0.02, 0, 0)
    for M in ROWS:
        x = ops.DevBuf(M * K * 2)
        L.vra_fill_normal(x.ptr, M * K, 3, 0.0, 1.0, 0, 0)
        out = ops.DevBuf(M * N * nt * 2)

        def fp8(i):
            c = i % copies
            if dual:
                L.vra_fp8_gate_up_silu(x.ptr, w8[c][0].ptr, sc[c][0].ptr, w8[c][1].ptr, sc[c][1].ptr, out.ptr, M, K, N, 128, 128, 0, 0)
            else:
                L.vra_fp8_gemm(x.ptr, w8[c][0].ptr, sc[c][0].ptr, None, None, out.ptr, M, K, N, 128, 128, 0, 0)

        def dense(i):
            L.vra_dense_gemm(x.ptr, w16[i % dcopies].ptr, None, out.ptr, M, K, N * nt, 0, 0, 0)

        flops = 2.0 * M * K * N * nt
        n = max(4, min(200, int(2e10 / flops)))
        variants = ([("gemv", 32), ("gemm", 0)] if M <= 32 else [("gemm", 0)]) + [("dense", None)]
        t = {v: [] for v, _ in variants}
        for r in range(ROUNDS + 1):  # round 0 warms every variant up
            for v, rows in variants:
                if rows is not None:
                    L.vra_debug_set_fp8_decode_max_rows(rows)
                us = timed(dense if v == "dense" else fp8, n)
                if r:
                    t[v].append(us)
        ops.check_error()
        med = {v: sorted(ts)[len(ts) // 2] for v, ts in t.items()}
        best = min(med[v] for v in med if v != "dense")
        b8 = K * N * nt + (N // 128) * (K // 128) * 4 * nt + M * K * 2 + M * N * 2
        b16 = K * N * nt * 2 + M * K * 2 + M * N * nt * 2
        if M <= 32:
            rate = "%.2f TB/s (%.2f); dense %.2f TB/s" % (b8 / best / 1e6, b8 / best / 1e6 / 8, b16 / med["dense"] / 1e6)
        else:
            rate = "%.3f PFLOP/s (%.2f); dense %.3f PFLOP/s" % (flops / best / 1e9, flops / best / 1e9 / 2.5, flops / med["dense"] / 1e9)
        print("%-13s %5d | %9s %9.1f %9.1f | %s" % (name, M, "%.1f" % med["gemv"] if "gemv" in med else "-", med["gemm"], med["dense"], rate))
        sys.stdout.flush()
    L.vra_debug_set_fp8_decode_max_rows(32)
    del w8, sc, w16
