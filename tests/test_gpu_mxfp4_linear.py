"""MXFP4 linears (vllm_rs_amd/csrc/gemv_mx4.cuh up to 32 rows; the widening pass + kernel X above) against the contract of DESIGN.md
§5.2 in float64, rounded once: w = E2M1(code) * 2^(byte - 127), out = round(x . w (+ bias)), then round(out + residual).  Codes are
uniform over the 16; block exponents are round(log2(1 / sqrt(8.5625 K))) + U{-2..2} (8.5625 = the codes' mean square), so neighbouring
blocks differ by up to 16x and a wrong block index shows.

Margin of the 1-ulp / 2 % bound at these shapes: an f32-accumulating emulation of the contract on the CPU differs from the float64
reference in <= 0.006 % of elements in bf16 and <= 0.054 % in f16."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_fp8_linear import ENGINE_CFGS, check_logits
from tests.util import BF16, F16, assert_close_dt, rand_dt, rng
from vllm_rs_amd import ops

pytestmark = pytest.mark.gpu

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
SCALE_RANGE = {BF16: (2, 252), F16: (114, 140)}  # bytes between which w is exact in the dtype
MMAX = 257
SHAPES = [(256, 144), (384, 128)]  # a ragged column count / an odd number of tiles
ROWS = [1, 4, 5, 16, 17, 32, 33, 64, 257]  # both sides of the row tiles (16, 32), of the kernel switch (32 | 33) and of kernel X's 256-row tile


def pack(codes, sbytes):
    """codes [N, K], scale bytes [N, K/32] -> device (tiles, scale words), through the checkpoint layout (k = 2i in the low nibble of byte i)"""
    N, K = codes.shape
    packed = (codes[:, 0::2] | codes[:, 1::2] << 4).astype(np.uint8)
    return ops.mxfp4_weight_repack(ops.dev(packed), ops.dev(sbytes.astype(np.uint8)), N, K)


def dequant(codes, sbytes):
    return E2M1[codes] * 2.0 ** (np.repeat(sbytes.astype(np.float64), 32, 1) - 127)


def draw(r, N, K, spread=2):
    e = int(np.round(np.log2(1 / np.sqrt(8.5625 * K))))
    return r.integers(0, 16, (N, K)).astype(np.uint8), (127 + e + r.integers(-spread, spread + 1, (N, K // 32))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def problem(dt, K, N, seed=0):
    """-> x bits [MMAX, K], float64 product [MMAX, N], device (tiles, scale words)"""
    codes, sb = draw(rng(1000 * seed + K + N + dt), N, K)
    x = rand_dt(rng(7 + K + dt), (MMAX, K), dt)  # (the same activations for every weight tensor of a K)
    return x, orc.from_dt(x, dt).astype(np.float64) @ dequant(codes, sb).T, pack(codes, sb)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [32, 33])
def test_mxfp4_codes_and_scales_are_exact(dt, M):
    """one-hot rows read single weights back: pins the nibble order, the byte select, the scale shift and the convert's exactness"""
    K, N = 128, 16
    lo, hi = SCALE_RANGE[dt]
    codes = ((np.arange(N)[:, None] + np.arange(K)[None, :]) % 16).astype(np.uint8)
    sb = np.tile(np.array([lo, hi, 120, 130], np.uint8), (N, 1))
    ks = [(i // 8) * 32 + ((i // 2) % 4) * 8 + i % 8 for i in range(32)] + [127]  # every block x every in-word position, the octets mixed
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), ks[:M]] = 1.0
    out = ops.mxfp4_gemm(ops.dev(orc.to_dt(x, dt)), *pack(codes, sb), M, K, N, dtype=dt, out=ops.DevBuf(M * N * 2).fill_bytes(0xEE))
    want = orc.to_dt((dequant(codes, sb)[:, ks[:M]].T + 0.0).astype(np.float32), dt)  # (+ 0.0: a sum that holds -0 * 1 is +0)
    assert np.array_equal(out.numpy(np.uint16, (M, N)), want)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M,K,N", [(M, K, N) for K, N in SHAPES for M in ROWS] + [(M, 2048, 272) for M in (1, 32, 129)])
def test_mxfp4_gemm(dt, M, K, N):
    x, ref, (w, s) = problem(dt, K, N)
    out = ops.mxfp4_gemm(ops.dev(x[:M]), w, s, M, K, N, dtype=dt, out=ops.DevBuf(M * N * 2).fill_bytes(0xEE))
    assert_close_dt(out.numpy(np.uint16, (M, N)), orc.to_dt(ref[:M], dt), dt, max_ulp=1.0, abs_floor=2e-3, name="mxfp4_gemm")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [3, 40])
def test_mxfp4_gemm_bias_residual(dt, M):
    K, N = SHAPES[0]
    x, ref, (w, s) = problem(dt, K, N)
    r = rng(M)
    bias, res = rand_dt(r, (N,), dt), rand_dt(r, (M, N), dt)
    out = ops.mxfp4_gemm(ops.dev(x[:M]), w, s, M, K, N, bias=ops.dev(bias), residual=ops.dev(res), dtype=dt)
    pre = ref[:M] + orc.from_dt(bias, dt).astype(np.float64)[None, :]
    want = orc.to_dt(orc.from_dt(orc.to_dt(pre, dt), dt).astype(np.float64) + orc.from_dt(res, dt), dt)
    mag = np.maximum(np.abs(ref[:M]), np.abs(pre)).astype(np.float32)
    assert_close_dt(out.numpy(np.uint16, (M, N)), want, dt, max_ulp=3.0, name="mxfp4_gemm bias+residual", mag=mag)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [2, 48])
def test_mxfp4_gate_up_silu(dt, M):
    K, N = SHAPES[0]
    x, g, (wg, sg) = problem(dt, K, N)
    _, u, (wu, su) = problem(dt, K, N, seed=1)  # the up tensor: other weights and scales, same x
    out = ops.mxfp4_gate_up_silu(ops.dev(x[:M]), wg, sg, wu, su, M, K, N, dtype=dt)
    want = orc.silu_mul(orc.to_dt(g[:M], dt), orc.to_dt(u[:M], dt), dt)
    assert_close_dt(out.numpy(np.uint16, (M, N)), want, dt, max_ulp=3.0, max_mismatch_frac=0.04, abs_floor=4e-3, name="mxfp4_gate_up_silu")


@pytest.mark.parametrize("K,N,scales", [(192, 144, True), (256, 24, True), (256, 144, False)])
def test_mxfp4_rejects(K, N, scales):
    M = 4
    L = ops.lib()
    x, w, sc = ops.DevBuf(M * K * 2).zero(), ops.DevBuf(N * K).zero(), ops.DevBuf(N * K).zero()
    s = sc.ptr if scales else None
    out = ops.DevBuf(M * N * 2).fill_bytes(0xEE)
    for call in (lambda: L.vra_mxfp4_repack(w.ptr, s, out.ptr, out.ptr, N, K, 0),
                 lambda: L.vra_mxfp4_gemm(x.ptr, w.ptr, s, None, None, out.ptr, M, K, N, BF16, 0),
                 lambda: L.vra_mxfp4_gate_up_silu(x.ptr, w.ptr, s, w.ptr, s, out.ptr, M, K, N, BF16, 0)):
        call()
        assert L.vra_last_error().decode(), "no error reported"
        L.vra_clear_error()
        assert (out.numpy(np.uint8, (M * N * 2,)) == 0xEE).all(), "output written despite the rejection"


def mx4_model(variant, seed):
    """-> cfg, engine tensors (packed nibbles + E8M0 bytes; qwen2 under the `blocks` / `scales` names), oracle tensors (w * 2^e, exact in 16 bits)"""
    from oracle import model as om
    cfg = dict(hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, vocab_size=512,
               max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0, quant_method=None, group_size=32, **ENGINE_CFGS[variant])
    dense = om.make_random_checkpoint(cfg, seed)
    r, eng_w = rng(seed), dict(dense)
    wn, sn = ("weight_packed", "weight_scale") if variant == "llama" else ("blocks", "scales")
    for name in [n for n in dense if n.endswith("_proj.weight")]:
        codes, sb = draw(r, *dense[name].shape, spread=1)
        dense[name] = orc.to_dt(dequant(codes, sb).astype(np.float32), cfg["dtype"])
        del eng_w[name]
        eng_w[name[:-6] + wn], eng_w[name[:-6] + sn] = (codes[:, 0::2] | codes[:, 1::2] << 4).astype(np.uint8), sb
    return cfg, eng_w, dense


@pytest.mark.parametrize("variant", ["llama", "qwen2"])
def test_mxfp4_engine_matches_dense_oracle(variant):
    """the engine on MXFP4 tensors and the dense oracle on w * 2^e (exact in 16 bits) compute the same real function"""
    from oracle import model as om
    from vllm_rs_amd.engine import Engine
    cfg, eng_w, dense = mx4_model(variant, 3)
    eng = Engine(dict(cfg, quant_method="mxfp4"), num_gpu_blocks=64, max_num_seqs=32, max_model_len=512, use_graph=False).load_weights(eng_w)
    oracle = om.OracleModel(cfg, dense, num_blocks=64)
    seqs = [rng(1 + n).integers(0, cfg["vocab_size"], size=n).tolist() for n in (5, 70, 1, 33)]  # ragged prefill: 109 rows (pass + kernel X)
    bt = np.arange(8, dtype=np.uint32).reshape(4, 2)  # two 64-token blocks per sequence
    slot = lambda b, j: int(bt[b, j // 64]) * 64 + j % 64
    ids, pos = np.array([t for s in seqs for t in s], np.uint32), np.array([j for s in seqs for j in range(len(s))], np.int64)
    slots = np.array([slot(b, j) for b, s in enumerate(seqs) for j in range(len(s))], np.int64)
    ctx, cu = np.array([len(s) for s in seqs], np.uint32), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint32)
    ref = oracle.forward(ids, pos, slots, bt, ctx, cu)
    check_logits(eng.forward_raw(ids, pos, slots, bt, ctx, cu), ref, f"mxfp4 {variant} prefill", cfg["dtype"])
    for step in range(3):  # decode (4 rows: the decode kernel), both sides fed the oracle's greedy token
        for s, t in zip(seqs, orc.argmax_f32(ref)):
            s.append(int(t))
        ids, pos = np.array([s[-1] for s in seqs], np.uint32), np.array([len(s) - 1 for s in seqs], np.int64)
        slots, ctx = np.array([slot(b, len(s) - 1) for b, s in enumerate(seqs)], np.int64), np.array([len(s) for s in seqs], np.uint32)
        ref = oracle.forward(ids, pos, slots, bt, ctx, None)
        check_logits(eng.forward_raw(ids, pos, slots, bt, ctx, None), ref, f"mxfp4 {variant} decode {step}", cfg["dtype"])
    eng.close()


def test_mxfp4_engine_graph_decode_is_bit_equal_to_eager():
    from vllm_rs_amd.engine import Engine
    cfg, eng_w, _ = mx4_model("llama", 5)
    prompt, runs = rng(2).integers(0, cfg["vocab_size"], size=33).tolist(), []
    for graph in (False, True):
        eng = Engine(dict(cfg, quant_method="mxfp4"), num_gpu_blocks=64, max_model_len=512, use_graph=graph).load_weights(eng_w)
        rid, logits = eng.add_request(prompt, 4, True), []
        while eng.has_unfinished():
            eng.step()
            logits.append(eng.last_logits(1).copy())
        runs.append((np.stack(logits), np.asarray(eng.output(rid))))
        eng.close()
    assert len(runs[0][0]) == len(runs[1][0]) >= 4 and np.array_equal(runs[0][1], runs[1][1])  # one prefill step, then decode steps
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32)), "graph replay and eager decode logits differ"


def test_mxfp4_engine_synthetic_weights_and_load_time_refusals():
    from vllm_rs_amd.engine import Engine
    cfg = dict(mx4_model("llama", 5)[0], quant_method="mxfp4")
    eng = Engine(cfg, num_gpu_blocks=16, max_model_len=512, use_graph=True).init_synthetic()
    out = eng.generate([list(range(3, 40))], max_tokens=3, ignore_eos=True)[0]
    assert len(out) == 3 and np.isfinite(eng.last_logits(1)).all()
    eng.close()
    with pytest.raises(RuntimeError, match="mxfp4 linears .* one rank only"):
        Engine(cfg, num_gpu_blocks=16, max_model_len=512, use_graph=False, tp_rank=0, tp_world_size=2).init_synthetic()
    cfg16, eng_w, _ = mx4_model("qwen2", 5)  # f16: a scale byte of 141 would overflow 6 * 2^14
    eng_w["model.layers.1.mlp.down_proj.scales"][7, 3] = 141
    with pytest.raises(RuntimeError, match=r"layers\.1\.mlp\.down_proj\.scales.*scale byte 141"):
        Engine(dict(cfg16, quant_method="mxfp4"), num_gpu_blocks=16, max_model_len=512, use_graph=False).load_weights(eng_w)
