"""Mixture-of-experts block on MXFP4 experts (vllm_rs_amd/csrc/moe_mx4.cuh): vra_moe_mxfp4_experts against the contract of DESIGN.md §5.4
in float64 with w = E2M1(code) * 2^(byte - 127) (§5.2) on the decode path (T <= 32) and on the tiled path (every T), a one-hot layout pin,
and the refusals.  Codes are uniform over the 16; block exponents are round(log2(1 / sqrt(8.5625 K))) + U{-2..2} as in
test_gpu_mxfp4_linear.py, so a wrong block index shows.  I 384 gives three K tiles in down (and in gate/up at H 384): waves without a tile
and a tile count that the wave count does not divide.

Margin of the 1-ulp / 2 % bound at these shapes (abs_floor = one dt ulp at the rms of the reference): an f32-accumulating emulation of
the contract on the CPU differs from the float64 reference in <= 0.13 % of elements in bf16 and <= 1.13 % in f16 over every case below
(worst: 40 random tokens | 16 tokens on two experts), each within the 1-ulp bound.  The residual step is checked exactly, as in test_gpu_moe.py."""
import functools

import numpy as np
import pytest

from tests.test_gpu_moe import ROUTINGS, experts_ref, f64, round_dt
from tests.test_gpu_mxfp4_linear import E2M1, SCALE_RANGE, dequant, draw
from tests.util import BF16, F16, assert_close_dt, rand_dt, rng, ulp_of
from vllm_rs_amd import ops

pytestmark = pytest.mark.gpu

E, TOPK, I = 8, 2, 384


def repack(H, *tensors):
    """(codes [E, N, K], scale bytes [E, N, K/32]) of gate, up, down -> the device tiles and scale words, through the checkpoint layout"""
    args = [ops.dev(a) for c, s in tensors for a in ((c[..., 0::2] | c[..., 1::2] << 4).astype(np.uint8), s.astype(np.uint8))]
    return ops.moe_mxfp4_weight_repack(*args, E, H, I)


@functools.lru_cache(maxsize=None)
def weights(dt, H):
    """-> [(codes, scale bytes)] and the float64 weights of gate, up, down"""
    r = rng(200 + H + dt)
    q = [tuple(a.reshape(E, n, -1) for a in draw(r, E * n, k)) for n, k in ((I, H), (I, H), (H, I))]
    return q, [dequant(c.reshape(-1, c.shape[2]), s.reshape(-1, s.shape[2])).reshape(c.shape) for c, s in q]


@functools.lru_cache(maxsize=None)
def tiles(dt, H):
    return repack(H, *weights(dt, H)[0])


@functools.lru_cache(maxsize=None)
def case(dt, H, kind, T):
    r = rng(T + H + dt)
    x, res = rand_dt(r, (T, H), dt), rand_dt(r, (T, H), dt)
    ids = np.stack([r.permutation(E)[:TOPK] for _ in range(T)]).astype(np.uint32)
    if kind == "two":
        ids[:] = (0, 1)  # six experts idle, the two busy ones straddle the 16- and 32-row tiles and the 64-row work item
    if kind == "drop":
        ids[2, 1] = E
    tw = r.random((T, TOPK), np.float32) + np.float32(0.1)
    tw /= tw.sum(1, keepdims=True)
    return x, res, ids, tw, experts_ref(dt, f64(x, dt), *weights(dt, H)[1], ids, tw)


def run_paths(T, fn):
    """fn(name) on every path that can take T tokens"""
    try:
        for rows, name in ((32, "decode"), (0, "tiled")):
            if rows == 0 or T <= rows:
                ops.lib().vra_debug_set_moe_mxfp4_decode_max_rows(rows)
                fn(name)
    finally:
        ops.lib().vra_debug_set_moe_mxfp4_decode_max_rows(32)


@pytest.mark.parametrize("H,kind,T", [(256, k, T) for k, T in ROUTINGS] + [(384, "rand", 40)])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_moe_mxfp4_experts(dt, H, kind, T):
    x, res, ids, tw, pre = case(dt, H, kind, T)
    floor = float(ulp_of(np.sqrt(np.mean(pre * pre)), dt))

    def run(residual):
        out = ops.moe_mxfp4_experts(ops.dev(x), *tiles(dt, H), ops.dev(tw), ops.dev(ids), T, E, TOPK, H, I, residual=residual, dtype=dt,
                                    out=ops.DevBuf(T * H * 2).fill_bytes(0xEE))
        return out.numpy(np.uint16, (T, H))

    def check(name):
        got = run(None)
        assert_close_dt(got, round_dt(pre, dt), dt, max_ulp=1.0, abs_floor=floor, name=f"moe_mxfp4_experts {name}")
        assert np.array_equal(run(None), got), f"{name}: two runs differ"
        # the residual step is round(out + residual) on the ROUNDED out: exact given the output above
        assert np.array_equal(run(ops.dev(res)), round_dt(f64(got, dt) + f64(res, dt), dt)), f"{name}: residual"

    run_paths(T, check)


@pytest.mark.parametrize("path", [0, 32])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_moe_mxfp4_layout_pin(dt, path):
    """one-hot x rows read single gate / up weights back through silu(g) * u, down is a permutation (code 2 = 1.0 at byte 127): a swapped
    gate / up interleave, a wrong nibble, byte select, scale shift or expert stride is a gross error.  The scale bytes take both ends of
    the dtype's range in both tensors, gate's low end against up's high end, so that |g * u| <= 36 stays finite in f16."""
    H, T = 256, 33 if path == 0 else 32
    lo, hi = SCALE_RANGE[dt]
    e_, i_, k_ = np.ogrid[:E, :I, :H]
    gu = [((e_ * 7 + i_ * 3 + k_ * 5) % 17 % 16, np.array([lo, hi, 120, 130, 125])[(e_ + i_ + k_[:, :, ::32] // 32) % 5]),  # no period a tile size divides
          ((e_ * 5 + i_ * 11 + k_ * 3) % 19 % 16, np.array([hi, lo, 130, 120, 125])[(e_ + i_ + k_[:, :, ::32] // 32) % 5])]
    cd = np.zeros((E, H, I), np.int64)
    for e in range(E):
        cd[e, np.arange(H), (np.arange(H) * 5 + 7 * e) % I] = 2  # out[c] = h[(5 c + 7 e) % I]
    wg, wu = (E2M1[c] * 2.0 ** (np.repeat(s, 32, 2) - 127.0) for c, s in gu)
    ks = (np.arange(T) * 37 + 5) % H
    x = np.zeros((T, H))
    x[np.arange(T), ks] = 1.0
    ids, tw = (np.arange(T, dtype=np.uint32) % E)[:, None], np.ones((T, 1), np.float32)
    with np.errstate(over="ignore"):  # silu of a gate weight at the high end: exp overflows to inf, silu is -0 as in f32
        want = round_dt(experts_ref(dt, x, wg, wu, E2M1[cd], ids, tw), dt)
    try:
        ops.lib().vra_debug_set_moe_mxfp4_decode_max_rows(path)
        out = ops.moe_mxfp4_experts(ops.dev(round_dt(x, dt)), *repack(H, *gu, (cd, np.full((E, H, I // 32), 127))), ops.dev(tw), ops.dev(ids),
                                    T, E, 1, H, I, dtype=dt)
    finally:
        ops.lib().vra_debug_set_moe_mxfp4_decode_max_rows(32)
    assert_close_dt(out.numpy(np.uint16, (T, H)), want, dt, max_ulp=1.0, name="moe mxfp4 layout pin")


@pytest.mark.parametrize("experts,topk,H,inter,dt,scales,ws", [(8, 2, 256, 192, BF16, True, True), (8, 2, 192, 384, BF16, True, True),
                                                               (257, 2, 256, 384, BF16, True, True), (16, 9, 256, 384, BF16, True, True),
                                                               (8, 2, 256, 384, 2, True, True), (8, 2, 256, 384, BF16, False, True),
                                                               (8, 2, 256, 384, F16, True, False)])
def test_moe_mxfp4_experts_rejects(experts, topk, H, inter, dt, scales, ws):
    T = 4
    big = ops.DevBuf(1 << 20).zero()  # stands for x, weights, routing and workspace: nothing may be launched
    out = ops.DevBuf(T * H * 2).fill_bytes(0xEE)
    ops.lib().vra_moe_mxfp4_experts(big.ptr, big.ptr, big.ptr, big.ptr, big.ptr if scales else None, big.ptr, big.ptr, None, out.ptr,
                                    big.ptr if ws else None, T, experts, topk, H, inter, dt, 0)
    with pytest.raises(RuntimeError):
        ops.check_error()
    assert (out.numpy(np.uint8, (T * H * 2,)) == 0xEE).all(), "output written despite the rejection"
