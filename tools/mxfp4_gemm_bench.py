"""Times vra_mxfp4_gemm / vra_mxfp4_gate_up_silu on the Llama-3-8B widths beside the NVFP4 (vra_nvfp4_gemm), FP8 (vra_fp8_gemm) and int4 g128
(vra_wna16_gemm) linears of the same shape, HIP events, the four formats alternating inside one process — a gap beyond the run-to-run noise of this log is a
property of the kernels, not of the box.  Up to 32 rows MXFP4 and NVFP4 run their decode kernels, above the widening pass + kernel X.  Weights
rotate through a pool larger than the 256 MB last-level cache, so the small-row numbers are HBM numbers.
    python tools/mxfp4_gemm_bench.py > profiles/nvfp4_linear_gemm_shapes.txt        (profiles/mxfp4_linear_gemm_shapes.txt: the run before the NVFP4 column)"""
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


def scales16(K, N, seed):
    b = ops.DevBuf(K // 128 * N * 2)
    L.vra_fill_uniform(b.ptr, K // 128 * N, seed, 0.002, 0.02, 0, 0)
    return b


def scales32(K, N, seed):
    b = ops.DevBuf((N // 128) * (K // 128) * 4)
    L.vra_fill_uniform(b.ptr, (N // 128) * (K // 128), seed, 1e-4, 4e-4, 2, 0)
    return b


print("# us per call, median of %d alternating rounds; mxfp4 rate: TB/s of algorithmic bytes against 8 (rows <= 32), PFLOP/s against 2.5 (rows >= 128)" % ROUNDS)
print("%-13s %5s | %9s %9s %9s %9s | %9s %11s | %s" % ("shape", "rows", "mxfp4", "nvfp4", "fp8", "int4", "mxfp4/fp8", "nvfp4/mxfp4", "mxfp4 rate (fraction of peak)"))
for name, K, N, dual in SHAPES:
    nt = 2 if dual else 1
    copies = max(2, -(-POOL_BYTES // (K * N * nt // 2)))  # (of the 4-bit formats; FP8 rotates through half as many of twice the size)
    w4 = [[fill(K * N // 2, 11 * c + t) for t in range(nt)] for c in range(copies)]  # hash nibbles: codes of either 4-bit format
    s4 = [[ops.DevBuf(K * N // 32).fill_bytes(0x78) for t in range(nt)] for c in range(copies)]  # every block 2^-7
    sn = [[ops.DevBuf(K * N // 16).fill_bytes(0x3A) for t in range(nt)] for c in range(copies)]  # NVFP4: every group 1.25, g below
    sq = [[scales16(K, N, 5 + c + t) for t in range(nt)] for c in range(copies)]
    w8 = [[fill(K * N, 7 * c + t) for t in range(nt)] for c in range(copies // 2)]
    s8 = [[scales32(K, N, 5 + c + t) for t in range(nt)] for c in range(copies // 2)]
    for M in ROWS:
        x = ops.DevBuf(M * K * 2)
        L.vra_fill_normal(x.ptr, M * K, 3, 0.0, 1.0, 0, 0)
        out = ops.DevBuf(M * N * 2)

        def mx4(i):
            w, s = w4[i % copies], s4[i % copies]
            if dual:
                L.vra_mxfp4_gate_up_silu(x.ptr, w[0].ptr, s[0].ptr, w[1].ptr, s[1].ptr, out.ptr, M, K, N, 0, 0)
            else:
                L.vra_mxfp4_gemm(x.ptr, w[0].ptr, s[0].ptr, None, None, out.ptr, M, K, N, 0, 0)

        def nv4(i):
            w, s = w4[i % copies], sn[i % copies]
            if dual:
                L.vra_nvfp4_gate_up_silu(x.ptr, w[0].ptr, s[0].ptr, 0.005, w[1].ptr, s[1].ptr, 0.006, out.ptr, M, K, N, 0, 0)
            else:
                L.vra_nvfp4_gemm(x.ptr, w[0].ptr, s[0].ptr, 0.005, None, None, out.ptr, M, K, N, 0, 0)

        def fp8(i):
            w, s = w8[i % len(w8)], s8[i % len(w8)]
            if dual:
                L.vra_fp8_gate_up_silu(x.ptr, w[0].ptr, s[0].ptr, w[1].ptr, s[1].ptr, out.ptr, M, K, N, 128, 128, 0, 0)
            else:
                L.vra_fp8_gemm(x.ptr, w[0].ptr, s[0].ptr, None, None, out.ptr, M, K, N, 128, 128, 0, 0)

        def int4(i):
            w, s = w4[i % copies], sq[i % copies]
            if dual:
                L.vra_wna16_gate_up_silu(x.ptr, w[0].ptr, s[0].ptr, None, w[1].ptr, s[1].ptr, None, out.ptr, M, K, N, 128, 0, 0, 0, 0)
            else:
                L.vra_wna16_gemm(x.ptr, w[0].ptr, s[0].ptr, None, None, None, out.ptr, M, K, N, 128, 0, 0, 0, 0)

        flops = 2.0 * M * K * N * nt
        n = max(4, min(200, int(2e10 / flops)))
        variants = [("mxfp4", mx4), ("nvfp4", nv4), ("fp8", fp8), ("int4", int4)]
        t = {v: [] for v, _ in variants}
        for r in range(ROUNDS + 1):  # round 0 warms every variant up
            for v, fn in variants:
                us = timed(fn, n)
                if r:
                    t[v].append(us)
        ops.check_error()
        med = {v: sorted(ts)[len(ts) // 2] for v, ts in t.items()}
        b4 = (K * N // 2 + K * N // 32) * nt + M * K * 2 + M * N * 2
        if M <= 32:
            rate = "%.2f TB/s (%.2f)" % (b4 / med["mxfp4"] / 1e6, b4 / med["mxfp4"] / 1e6 / 8)
        else:
            rate = "%.3f PFLOP/s (%.2f)" % (flops / med["mxfp4"] / 1e9, flops / med["mxfp4"] / 1e9 / 2.5)
        print("%-13s %5d | %9.1f %9.1f %9.1f %9.1f | %9.2f %11.2f | %s" %
              (name, M, med["mxfp4"], med["nvfp4"], med["fp8"], med["int4"], med["mxfp4"] / med["fp8"], med["nvfp4"] / med["mxfp4"], rate))
        sys.stdout.flush()
    del w4, s4, sn, sq, w8, s8
