"""Mixture-of-experts block (vllm_rs_amd/csrc/moe.cuh): vra_moe_route against a float64 softmax + stable argsort, vra_moe_experts against
the contract of DESIGN.md §5.4 in float64 (exact products, h rounded once to dt, y and the slot sum unrounded, one final rounding, then
the residual) on the decode path (T <= 32) and on the tiled path (every T), a one-hot layout pin, and the refusals.

Margin of the 1-ulp / 2 % bound at these shapes (H 256 | 384, I 192, E 8, topk 2; abs_floor = one dt ulp at the rms of the reference):
an f32-accumulating emulation of the contract on the CPU differs from the float64 reference in <= 0.24 % of elements in bf16 and
<= 1.08 % in f16 over every case below (worst: 130 random tokens | 32 tokens on two experts), each within the 1-ulp bound.  The residual step is checked exactly instead: round(out + residual)
of the rounded out is one deterministic f32 add, so the run with a residual must equal it bit for bit on the run without.  (Against the
float64 reference it would need ulp(out) + ulp(result): a flipped out lands the sum on the other side of a tie of the second rounding.)"""
import functools

import numpy as np
import pytest

from tests.util import BF16, F16, assert_close_dt, orc, rand_dt, rng, ulp_of
from vllm_rs_amd import ops

pytestmark = pytest.mark.gpu

E, TOPK, I = 8, 2, 192
ROUTINGS = [("two", T) for T in (1, 16, 17, 32, 33, 65)] + [("rand", T) for T in (4, 40, 130)] + [("drop", 5)]


def f64(bits, dt):
    return orc.from_dt(bits, dt).astype(np.float64)


def round_dt(v, dt):
    return orc.to_dt(np.asarray(v, np.float32), dt)


# ---------------------------------------------------------------- routing
def route_ref(logits, topk, norm, scale):
    p = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    ids = np.argsort(-p, axis=1, kind="stable")[:, :topk]
    w = np.take_along_axis(p, ids, 1)
    return (w / w.sum(1, keepdims=True) if norm else w) * scale, ids


@pytest.mark.parametrize("scale", [1.0, 2.5])
@pytest.mark.parametrize("norm", [0, 1])
@pytest.mark.parametrize("experts,topk", [(e, k) for e in (8, 128, 256) for k in (1, 2, 8) if k <= e])
def test_moe_route(experts, topk, norm, scale):
    T, r = 5, rng(experts + topk)
    logits = np.stack([r.permutation(experts) for _ in range(T)]).astype(np.float32) * np.float32(0.03) - 1  # no two probabilities of a row tie
    w, ids = ops.moe_route(ops.dev(logits), T, experts, topk, norm, scale)
    want_w, want_ids = route_ref(logits, topk, norm, scale)
    assert np.array_equal(ids.numpy(np.uint32, (T, topk)), want_ids)
    np.testing.assert_allclose(w.numpy(np.float32, (T, topk)), want_w, rtol=1e-5)


def test_moe_route_ties_take_the_lower_index():
    w, ids = ops.moe_route(ops.dev(np.full((3, 128), 0.25, np.float32)), 3, 128, 8, 1, 1.0)
    assert np.array_equal(ids.numpy(np.uint32, (3, 8)), np.tile(np.arange(8), (3, 1)))
    np.testing.assert_allclose(w.numpy(np.float32, (3, 8)), 0.125, rtol=1e-5)


# ---------------------------------------------------------------- experts
@functools.lru_cache(maxsize=None)
def experts_problem(dt, H):
    """-> float64 (gate, up, down) and the device tiles"""
    r = rng(100 + H + dt)
    g, u, d = rand_dt(r, (E, I, H), dt, H ** -0.5), rand_dt(r, (E, I, H), dt, H ** -0.5), rand_dt(r, (E, H, I), dt, I ** -0.5)
    return f64(g, dt), f64(u, dt), f64(d, dt), ops.moe_weight_repack(ops.dev(g), ops.dev(u), ops.dev(d), E, H, I, dt)


def experts_ref(dt, x, wg, wu, wd, ids, tw):
    """the contract in float64: out before the final rounding"""
    out = np.zeros((x.shape[0], wd.shape[1]))
    for t, j in np.ndindex(*ids.shape):
        e = int(ids[t, j])
        if e < wg.shape[0]:  # an id past the experts is dropped
            g, u = wg[e] @ x[t], wu[e] @ x[t]
            out[t] += np.float64(tw[t, j]) * (wd[e] @ f64(round_dt(g / (1 + np.exp(-g)) * u, dt), dt))
    return out


@functools.lru_cache(maxsize=None)
def case(dt, H, kind, T):
    r = rng(T + H + dt)
    x, res = rand_dt(r, (T, H), dt), rand_dt(r, (T, H), dt)
    ids = np.stack([r.permutation(E)[:TOPK] for _ in range(T)]).astype(np.uint32)
    if kind == "two":
        ids[:] = (0, 1)  # six experts idle, the two busy ones straddle the 16- and 32-row tiles
    if kind == "drop":
        ids[2, 1] = E
    tw = r.random((T, TOPK), np.float32) + np.float32(0.1)
    tw /= tw.sum(1, keepdims=True)
    wg, wu, wd, _ = experts_problem(dt, H)
    return x, res, ids, tw, experts_ref(dt, f64(x, dt), wg, wu, wd, ids, tw)


def run_paths(T, fn):
    """fn(name) on every path that can take T tokens"""
    try:
        for rows, name in ((32, "decode"), (0, "tiled")):
            if rows == 0 or T <= rows:
                ops.lib().vra_debug_set_moe_decode_max_rows(rows)
                fn(name)
    finally:
        ops.lib().vra_debug_set_moe_decode_max_rows(32)


@pytest.mark.parametrize("H,kind,T", [(256, k, T) for k, T in ROUTINGS] + [(384, "rand", 40)])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_moe_experts(dt, H, kind, T):
    x, res, ids, tw, pre = case(dt, H, kind, T)
    tiles = experts_problem(dt, H)[3]
    floor = float(ulp_of(np.sqrt(np.mean(pre * pre)), dt))

    def run(residual):
        out = ops.moe_experts(ops.dev(x), *tiles, ops.dev(tw), ops.dev(ids), T, E, TOPK, H, I, residual=residual, dtype=dt,
                              out=ops.DevBuf(T * H * 2).fill_bytes(0xEE))
        return out.numpy(np.uint16, (T, H))

    def check(name):
        got = run(None)
        assert_close_dt(got, round_dt(pre, dt), dt, max_ulp=1.0, abs_floor=floor, name=f"moe_experts {name}")
        assert np.array_equal(run(None), got), f"{name}: two runs differ"
        # the residual step is round(out + residual) on the ROUNDED out: exact given the output above
        assert np.array_equal(run(ops.dev(res)), round_dt(f64(got, dt) + f64(res, dt), dt)), f"{name}: residual"

    run_paths(T, check)


@pytest.mark.parametrize("path", [0, 32])
@pytest.mark.parametrize("dt", [BF16, F16])
def test_moe_layout_pin(dt, path):
    """one-hot x rows read single gate / up weights back through silu(g) * u: a wrong fragment, a swapped gate / up interleave or a wrong
    expert stride is a gross error, not noise (T = 33 forced onto the decode kernel is refused by the clamp, so it runs T = 32 there)"""
    H, T = 256, 33 if path == 0 else 32
    e_, i_, k_ = np.ogrid[:E, :I, :H]
    wg = ((e_ * 7 + i_ * 3 + k_ * 5) % 13 - 6).astype(np.float64)  # small integers, exact in dt, no period that a tile size divides
    wu = ((e_ * 5 + i_ * 11 + k_ * 3) % 17 - 8).astype(np.float64)
    wd = np.zeros((E, H, I))
    for e in range(E):
        wd[e, np.arange(H), (np.arange(H) * 5 + 7 * e) % I] = 1.0  # out[c] = h[(5 c + 7 e) % I]
    ks = (np.arange(T) * 37 + 5) % H
    x = np.zeros((T, H))
    x[np.arange(T), ks] = 1.0
    ids, tw = (np.arange(T, dtype=np.uint32) % E)[:, None], np.ones((T, 1), np.float32)
    tiles = ops.moe_weight_repack(*(ops.dev(round_dt(w, dt)) for w in (wg, wu, wd)), E, H, I, dt)
    want = round_dt(experts_ref(dt, x, wg, wu, wd, ids, tw), dt)
    try:
        ops.lib().vra_debug_set_moe_decode_max_rows(path)
        out = ops.moe_experts(ops.dev(round_dt(x, dt)), *tiles, ops.dev(tw), ops.dev(ids), T, E, 1, H, I, dtype=dt)
    finally:
        ops.lib().vra_debug_set_moe_decode_max_rows(32)
    assert_close_dt(out.numpy(np.uint16, (T, H)), want, dt, max_ulp=1.0, name="moe layout pin")


@pytest.mark.parametrize("experts,topk,H,inter,dt,ws", [(257, 2, 256, 192, BF16, True), (16, 9, 256, 192, BF16, True), (4, 5, 256, 192, BF16, True),
                                                        (8, 2, 192, 192, BF16, True), (8, 2, 256, 96, BF16, True), (8, 2, 256, 192, 2, True),
                                                        (8, 2, 256, 192, F16, False)])
def test_moe_experts_rejects(experts, topk, H, inter, dt, ws):
    T = 4
    big = ops.DevBuf(1 << 20).zero()  # stands for x, weights, routing and workspace: nothing may be launched
    out = ops.DevBuf(T * H * 2).fill_bytes(0xEE)
    ops.lib().vra_moe_experts(big.ptr, big.ptr, big.ptr, big.ptr, big.ptr, None, out.ptr, big.ptr if ws else None, T, experts, topk, H, inter, dt, 0)
    with pytest.raises(RuntimeError):
        ops.check_error()
    assert (out.numpy(np.uint8, (T * H * 2,)) == 0xEE).all(), "output written despite the rejection"
