"""NVFP4 linears (vllm_rs_amd/csrc/gemv_nv4.cuh up to 32 rows; the widening pass + kernel X above) against the contract of DESIGN.md
§5.3 in float64, rounded once: w = E2M1(code) * E4M3(scale byte), out = round(g * (x . w) (+ bias)), then round(out + residual).  Codes
are uniform over the 16; scale bytes have exponent field 5..9 (2^-2 .. 2^2) and all eight mantissas, so neighbouring groups differ by up
to 30x and a wrong group index or a dropped mantissa shows; g = 0.73 / sqrt(K mean(w^2)) is no power of two.

Margin of the 1-ulp / 2 % bound at these shapes: an f32-accumulating emulation of the contract on the CPU differs from the float64
reference in <= 0.008 % of elements in bf16 and <= 0.10 % in f16, and every w is exact in 16 bits."""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.test_gpu_fp8_linear import E4M3, ENGINE_CFGS, check_logits
from tests.util import BF16, F16, assert_close_dt, rand_dt, rng
from vllm_rs_amd import ops

pytestmark = pytest.mark.gpu

E2M1 = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6])
MMAX = 257
SHAPES = [(256, 144), (384, 128)]  # a ragged column count / an odd number of tiles
ROWS = [1, 4, 16, 17, 32, 33, 64, 257]  # both sides of the row tiles (16, 32), of the kernel switch (32 | 33) and of kernel X's 256-row tile


def nibbles(codes):
    return (codes[:, 0::2] | codes[:, 1::2] << 4).astype(np.uint8)  # checkpoint layout: k = 2i in the low nibble of byte i


def pack(codes, sbytes):
    """codes [N, K], scale bytes [N, K/16] -> device (tiles, scale words), through the checkpoint layout"""
    return ops.nvfp4_weight_repack(ops.dev(nibbles(codes)), ops.dev(sbytes.astype(np.uint8)), *codes.shape)


def dequant(codes, sbytes):
    return E2M1[codes] * np.repeat(E4M3[sbytes], 16, 1)


def draw(r, N, K, exps=(5, 10)):
    return r.integers(0, 16, (N, K)).astype(np.uint8), (r.integers(*exps, (N, K // 16)) << 3 | r.integers(0, 8, (N, K // 16))).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def problem(dt, K, N, seed=0):
    """-> x bits [MMAX, K], float64 g * (x . w) [MMAX, N], device (tiles, scale words), g"""
    codes, sb = draw(rng(1000 * seed + K + N + dt), N, K)
    w = dequant(codes, sb)
    g = float(np.float32(0.73 / np.sqrt(K * np.mean(w * w))))  # (the f32 the kernel is handed)
    x = rand_dt(rng(7 + K + dt), (MMAX, K), dt)  # (the same activations for every weight tensor of a K)
    return x, g * (orc.from_dt(x, dt).astype(np.float64) @ w.T), pack(codes, sb), g


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [32, 33])
def test_nvfp4_codes_groups_and_scale_bytes_are_exact(dt, M):
    """one-hot rows read single weights back bit-exactly: pins the nibble order, the byte select, the group of a lane (wrong group index),
    the scale word's byte (wrong scale byte) and the mantissa of the scale (a convert that keeps only the exponent)"""
    K, N = 128, 16
    codes = ((np.arange(N)[:, None] + np.arange(K)[None, :]) % 16).astype(np.uint8)
    base = np.array([0x01, 0x7E, 0xB5, 0x3B, 0x45, 0x29, 0x4F, 0x36], np.uint8)  # smallest subnormal, 448, a negative one, five more mantissas
    sb = np.stack([np.roll(base, n) for n in range(N)])
    # row i: K-step i // 8, octet i % 4 (both groups of every step), in-word position i % 8 (all eight in every step); row 32: the last k
    ks = [(i // 8) * 32 + (i % 4) * 8 + i % 8 for i in range(32)] + [127]
    x = np.zeros((M, K), np.float32)
    x[np.arange(M), ks[:M]] = 1.0
    out = ops.nvfp4_gemm(ops.dev(orc.to_dt(x, dt)), *pack(codes, sb), 1.0, M, K, N, dtype=dt, out=ops.DevBuf(M * N * 2).fill_bytes(0xEE))
    want = orc.to_dt((dequant(codes, sb)[:, ks[:M]].T + 0.0).astype(np.float32), dt)  # (+ 0.0: a sum that holds -0 * 1 is +0)
    assert np.array_equal(out.numpy(np.uint16, (M, N)), want)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M,K,N", [(M, K, N) for K, N in SHAPES for M in ROWS] + [(M, 2048, 272) for M in (1, 32, 129)])
def test_nvfp4_gemm(dt, M, K, N):
    x, ref, (w, s), g = problem(dt, K, N)
    out = ops.nvfp4_gemm(ops.dev(x[:M]), w, s, g, M, K, N, dtype=dt, out=ops.DevBuf(M * N * 2).fill_bytes(0xEE))
    assert_close_dt(out.numpy(np.uint16, (M, N)), orc.to_dt(ref[:M], dt), dt, max_ulp=1.0, abs_floor=2e-3, name="nvfp4_gemm")


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [3, 40])
def test_nvfp4_gemm_bias_residual(dt, M):
    K, N = SHAPES[0]
    x, ref, (w, s), g = problem(dt, K, N)
    r = rng(M)
    bias, res = rand_dt(r, (N,), dt), rand_dt(r, (M, N), dt)
    out = ops.nvfp4_gemm(ops.dev(x[:M]), w, s, g, M, K, N, bias=ops.dev(bias), residual=ops.dev(res), dtype=dt)
    pre = ref[:M] + orc.from_dt(bias, dt).astype(np.float64)[None, :]
    want = orc.to_dt(orc.from_dt(orc.to_dt(pre, dt), dt).astype(np.float64) + orc.from_dt(res, dt), dt)
    mag = np.maximum(np.abs(ref[:M]), np.abs(pre)).astype(np.float32)
    assert_close_dt(out.numpy(np.uint16, (M, N)), want, dt, max_ulp=3.0, name="nvfp4_gemm bias+residual", mag=mag)


@pytest.mark.parametrize("dt", [BF16, F16])
@pytest.mark.parametrize("M", [2, 48])
def test_nvfp4_gate_up_silu(dt, M):
    K, N = SHAPES[0]
    x, gt, (wg, sg), gg = problem(dt, K, N)
    _, up, (wu, su), gu = problem(dt, K, N, seed=1)  # the up tensor: other weights, scales and global scale, same x
    assert gg != gu
    out = ops.nvfp4_gate_up_silu(ops.dev(x[:M]), wg, sg, gg, wu, su, gu, M, K, N, dtype=dt)
    want = orc.silu_mul(orc.to_dt(gt[:M], dt), orc.to_dt(up[:M], dt), dt)
    assert_close_dt(out.numpy(np.uint16, (M, N)), want, dt, max_ulp=3.0, max_mismatch_frac=0.04, abs_floor=4e-3, name="nvfp4_gate_up_silu")


@pytest.mark.parametrize("K,N,scales", [(192, 144, True), (256, 24, True), (256, 144, False)])
def test_nvfp4_rejects(K, N, scales):
    M = 4
    L = ops.lib()
    x, w, sc = ops.DevBuf(M * K * 2).zero(), ops.DevBuf(N * K).zero(), ops.DevBuf(N * K).zero()
    s = sc.ptr if scales else None
    out = ops.DevBuf(M * N * 2).fill_bytes(0xEE)
    for call in (lambda: L.vra_nvfp4_repack(w.ptr, s, out.ptr, out.ptr, N, K, 0),
                 lambda: L.vra_nvfp4_gemm(x.ptr, w.ptr, s, 1.0, None, None, out.ptr, M, K, N, BF16, 0),
                 lambda: L.vra_nvfp4_gate_up_silu(x.ptr, w.ptr, s, 1.0, w.ptr, s, 1.0, out.ptr, M, K, N, BF16, 0)):
        call()
        assert L.vra_last_error().decode(), "no error reported"
        L.vra_clear_error()
        assert (out.numpy(np.uint8, (M * N * 2,)) == 0xEE).all(), "output written despite the rejection"


def nv4_model(variant, seed):
    """-> cfg, engine tensors, oracle tensors (w * g, exact in 16 bits: every g is a power of two).  llama takes the compressed-tensors
    names (weight_global_scale = 1 / g, a divisor), qwen2 the ModelOpt ones (the codes are `.weight`, weight_scale_2 = g, a 0-d tensor);
    both carry an activation scale the W4A16 path must ignore.  g = 2^-6 .. 2^-10 changes from each projection to the next (q, k, v and
    gate, up all differ), so a scale that reaches the wrong projection shows."""
    from oracle import model as om
    cfg = dict(hidden_size=256, intermediate_size=512, num_layers=2, num_heads=4, num_kv_heads=2, head_dim=64, vocab_size=512,
               max_position_embeddings=512, rms_norm_eps=1e-5, rope_theta=10000.0, quant_method=None, group_size=16, **ENGINE_CFGS[variant])
    dense = om.make_random_checkpoint(cfg, seed)
    r, eng_w = rng(seed), dict(dense)
    for i, name in enumerate(n for n in list(dense) if n.endswith("_proj.weight")):
        codes, sb = draw(r, *dense[name].shape, exps=(6, 9))
        g = 2.0 ** -(6 + i % 5)
        dense[name] = orc.to_dt((dequant(codes, sb) * g).astype(np.float32), cfg["dtype"])
        del eng_w[name]
        p = name[:-6]
        if variant == "llama":
            eng_w.update({p + "weight_packed": nibbles(codes), p + "weight_scale": sb, p + "weight_global_scale": np.array([1 / g], np.float32),
                          p + "input_global_scale": np.array([123.0], np.float32)})
        else:
            eng_w.update({p + "weight": nibbles(codes), p + "weight_scale": sb, p + "weight_scale_2": np.array(g, np.float32),
                          p + "input_scale": np.array(0.37, np.float32)})
    return cfg, eng_w, dense


@pytest.mark.parametrize("variant", ["llama", "qwen2"])
def test_nvfp4_engine_matches_dense_oracle(variant):
    """the engine on NVFP4 tensors and the dense oracle on w * g (exact in 16 bits) compute the same real function"""
    from oracle import model as om
    from vllm_rs_amd.engine import Engine
    cfg, eng_w, dense = nv4_model(variant, 3)
    eng = Engine(dict(cfg, quant_method="nvfp4"), num_gpu_blocks=64, max_num_seqs=32, max_model_len=512, use_graph=False).load_weights(eng_w)
    oracle = om.OracleModel(cfg, dense, num_blocks=64)
    seqs = [rng(1 + n).integers(0, cfg["vocab_size"], size=n).tolist() for n in (5, 70, 1, 33)]  # ragged prefill: 109 rows (pass + kernel X)
    bt = np.arange(8, dtype=np.uint32).reshape(4, 2)  # two 64-token blocks per sequence
    slot = lambda b, j: int(bt[b, j // 64]) * 64 + j % 64
    ids, pos = np.array([t for s in seqs for t in s], np.uint32), np.array([j for s in seqs for j in range(len(s))], np.int64)
    slots = np.array([slot(b, j) for b, s in enumerate(seqs) for j in range(len(s))], np.int64)
    ctx, cu = np.array([len(s) for s in seqs], np.uint32), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint32)
    ref = oracle.forward(ids, pos, slots, bt, ctx, cu)
    check_logits(eng.forward_raw(ids, pos, slots, bt, ctx, cu), ref, f"nvfp4 {variant} prefill", cfg["dtype"])
    for step in range(3):  # decode (4 rows: the decode kernel), both sides fed the oracle's greedy token
        for s, t in zip(seqs, orc.argmax_f32(ref)):
            s.append(int(t))
        ids, pos = np.array([s[-1] for s in seqs], np.uint32), np.array([len(s) - 1 for s in seqs], np.int64)
        slots, ctx = np.array([slot(b, len(s) - 1) for b, s in enumerate(seqs)], np.int64), np.array([len(s) for s in seqs], np.uint32)
        ref = oracle.forward(ids, pos, slots, bt, ctx, None)
        check_logits(eng.forward_raw(ids, pos, slots, bt, ctx, None), ref, f"nvfp4 {variant} decode {step}", cfg["dtype"])
    eng.close()


def test_nvfp4_engine_synthetic_weights_and_load_time_refusals():
    from vllm_rs_amd.engine import Engine
    cfg16, eng_w, _ = nv4_model("qwen2", 5)
    cfg = dict(nv4_model("llama", 5)[0], quant_method="nvfp4")
    eng = Engine(cfg, num_gpu_blocks=16, max_model_len=512, use_graph=True).init_synthetic()
    out = eng.generate([list(range(3, 40))], max_tokens=3, ignore_eos=True)[0]
    assert len(out) == 3 and np.isfinite(eng.last_logits(1)).all()
    eng.close()
    with pytest.raises(RuntimeError, match="nvfp4 linears .* one rank only"):
        Engine(cfg, num_gpu_blocks=16, max_model_len=512, use_graph=False, tp_rank=0, tp_world_size=2).init_synthetic()
    eng_w["model.layers.1.mlp.down_proj.weight_scale"][7, 3] = 0x7F
    with pytest.raises(RuntimeError, match=r"layers\.1\.mlp\.down_proj\.weight_scale.*scale byte 127 at \[7, 3\]"):
        Engine(dict(cfg16, quant_method="nvfp4"), num_gpu_blocks=16, max_model_len=512, use_graph=False).load_weights(eng_w)
