"""bench.py's command line without a GPU: a plain run is the headline figure only (`--full` is off by default), and `--dump-outputs`
writes float32 / float64 .npy files under its size cap, the same sample on every run."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_full_is_off_by_default_and_steps_are_taken_as_given(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "somewhere"


class _FakeEngine:
    """the engine calls run_decode makes, on the host: one request, a token per decode step (its running count), requests end at
    max_tokens or at max_model_len — as the real engine's do"""

    class ec:
        max_model_len = 64

    cfg = {}

    def __init__(self):
        self.reqs, self.count, self.timed = [], 0, []

    def add_request(self, prompt, max_tokens, ignore_eos):
        self.reqs.append(dict(n=len(prompt), left=max_tokens, out=[], prefilled=False))
        return len(self.reqs) - 1

    def _live(self):
        return [r for r in self.reqs if r["left"] > 0 and r["n"] < self.ec.max_model_len]

    def step(self):
        live = self._live()
        prefill = [r for r in live if not r["prefilled"]]
        for r in prefill or live:
            r["prefilled"] = True
            self.count += 1
            r["out"].append(self.count)
            r["n"] += 1
            r["left"] -= 1
        return len(prefill or live), bool(prefill)

    def timed_decode(self, steps):
        done = 0
        while done < steps and self.step()[0] > 0:
            done += 1
        self.timed.append(done)
        return float(done)

    def output(self, rid):
        return np.array(self.reqs[rid]["out"], np.uint32)

    def has_unfinished(self):
        return bool(self._live())


def test_steps_beyond_one_request_are_timed_in_rounds_and_all_of_them_run():
    eng = _FakeEngine()
    prompts = [np.arange(8, dtype=np.uint32)]
    dt, ms, outs = bench.run_decode_rounds(eng, prompts, 4, 100, lambda: None)
    assert sum(eng.timed) == 100 and ms == 100.0 and max(eng.timed) <= 64 - 8 - 4
    assert len(outs) == 1 and len(outs[0]) == 100 and len(set(outs[0].tolist())) == 100
    # one round when the steps fit, and `after` runs once, behind the last timed step
    eng, seen = _FakeEngine(), []
    dt, ms, outs = bench.run_decode_rounds(eng, prompts, 4, 20, lambda: None, after=lambda: seen.append(eng.count))
    assert eng.timed == [20] and seen == [int(outs[0][-1])]


def test_a_timed_region_that_falls_short_is_an_error():
    import pytest
    eng = _FakeEngine()
    with pytest.raises(RuntimeError, match="not the 200 asked for"):
        bench.run_decode(eng, [np.arange(8, dtype=np.uint32)], 4, 200, lambda: None)


def test_dump_outputs_writes_float_arrays(tmp_path):
    tokens = np.arange(10, dtype=np.uint32).reshape(2, 5) + 128000
    logits = np.random.default_rng(1).standard_normal((2, 7)).astype(np.float32)
    bench.dump_outputs(str(tmp_path / "d"), {"tokens": tokens, "logits": logits})
    t, l = np.load(tmp_path / "d" / "tokens.npy"), np.load(tmp_path / "d" / "logits.npy")
    assert t.dtype == np.float64 and (t == tokens).all()
    assert l.dtype == np.float32 and (l == logits).all()


def test_dump_outputs_samples_the_same_rows_under_the_cap(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_CAP_BYTES", 2 * 40 * 4 * 3)  # two arrays: three rows of 40 floats each
    big = np.random.default_rng(2).standard_normal((11, 40)).astype(np.float32)
    small = np.ones((2, 3), np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (3, 40) and (a == b).all()
    assert all(any((row == r).all() for r in big) for row in a)
    assert (np.load(tmp_path / "a" / "small.npy") == small).all()
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= bench.DUMP_CAP_BYTES
