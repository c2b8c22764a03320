"""tests/repeat_judge.py judged itself, on the CPU: the numpy statement of the rule in include/thewhisper.h equals HF's two processors bit
for bit; the oracle's run of every picks case, judged through HF's classes, has no wrong step, stays within the undecided cap and
shows every event; a row that is off is its row of the plain run."""
import numpy as np
import pytest

from tests import repeat_judge as rj
from tests import sampler_judge as sj


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.uint32)


def test_the_numpy_rule_is_hfs_two_processors_bit_for_bit():
    rng = np.random.default_rng(3)
    V = 301
    for trial in range(60):
        x = (rng.standard_normal(V) * 10 ** rng.uniform(-3, 3)).astype(np.float32)
        x[rng.integers(0, V, 6)] = [0.0, -0.0, -np.inf, 1e-42, -65504.0, 65504.0]
        n = int(rng.integers(0, 40))
        hist = rng.integers(0, 12 if trial % 2 else V, n).tolist()
        row = rj.Row(float(rng.choice([1.0, 1.1, 1.3, 0.7, 2.0, 1.0000001])), int(rng.choice([0, 1, 2, 3, 5])))
        ignore = int(rng.choice([0, 2, n]))
        if n == 0:      # (HF's n-gram processor indexes the last token: the engine never has an empty history)
            row = rj.Row(row.penalty, 0)
        want = rj.HFRepeat(row, ignore)(x, hist)
        got = rj.apply_rule(x, hist, row, ignore)
        assert np.array_equal(_bits(got), _bits(want)), (trial, row, ignore, hist)


def test_an_id_that_occurs_twice_is_penalised_once_and_the_division_is_not_a_reciprocal_multiply():
    x = np.array([3.0, -3.0, 7.0, 0.1], np.float32)
    got = rj.apply_rule(x, [0, 0, 1, 1, 0], rj.Row(1.3, 0))
    assert got[0] == np.float32(3.0) / np.float32(1.3) and got[1] == np.float32(-3.0) * np.float32(1.3) and got[2] == 7.0
    # values for which x / r and x * (1 / r) differ in float32 are plentiful for the ordinary penalties of the GPU bit test
    rng = np.random.default_rng(0)
    v = rng.uniform(0.0, 30.0, 20000).astype(np.float32)
    for r in (1.1, 1.3, 0.7):
        r32 = np.float32(r)
        assert (v / r32 != v * (np.float32(1.0) / r32)).any(), r


def test_ngram_rule_edges():
    x = np.zeros(10, np.float32)
    inf = np.isneginf
    assert not inf(rj.apply_rule(x, [1, 2], rj.Row(1.0, 3))).any()                         # n < N: nothing
    assert inf(rj.apply_rule(x, [1, 2, 3, 1, 2], rj.Row(1.0, 3))).nonzero()[0].tolist() == [3]
    assert inf(rj.apply_rule(x, [4, 5, 4], rj.Row(1.0, 1))).nonzero()[0].tolist() == [4, 5]
    assert inf(rj.apply_rule(x, [4, 5, 4], rj.Row(1.0, 2))).nonzero()[0].tolist() == [5]
    assert not inf(rj.apply_rule(x, [4, 5, 6], rj.Row(1.0, 3))).any()                      # n == N: the one window is the suffix's own start
    for hist, N in (([1, 2, 3, 1, 2], 3), ([4, 5, 4], 1), ([4, 5, 4], 2), ([7, 7, 7, 7], 2), ([7, 7, 7, 7], 5)):
        assert np.array_equal(_bits(rj.apply_rule(x, hist, rj.Row(1.0, N))), _bits(rj.HFRepeat(rj.Row(1.0, N))(x, hist)))


@pytest.mark.parametrize("case_id", [c.id for c in rj.REPEAT_CASES if not c.graph or c.B == 17 or c.dtype != "f32"])
def test_the_oracles_run_of_every_picks_case_shows_every_event_within_the_cap(case_id):
    rc = next(c for c in rj.REPEAT_CASES if c.id == case_id)
    built = rj.build(rc)
    rows, bias = rj.rows_of(rc.B), rj.bias_rows_of(built, rc.B)
    assert len({r for r in rows if r.on}) >= min(4, rc.B - 1) and sum(not r.on for r in rows) == 1
    assert rc.B < 17 or (rows[16].on and not rows[15].on)
    seqs, lg = rj.oracle_repeat_run(built.dims, built.weights, built.prompt, built.opt, rows, rj.IGNORE, bias)
    v = rj.judge_repeat(lg, seqs, rj.N_PROMPT, built.opt, rows, rj.IGNORE, bias)
    assert v.count("wrong") == 0, v.wrong[:3]
    assert v.count("undecided") * 100 <= v.judged
    seen = rj.events_seen(rows, rj.IGNORE, seqs, lg, rj.N_PROMPT, built.opt, bias)
    assert set(rj.EVENTS) <= seen, sorted(set(rj.EVENTS) - seen)
    plain, _ = sj.oracle_run(built.dims, built.weights, built.prompt, built.opt)
    off = rows.index(rj.OFF)
    n = min(plain.shape[1], seqs.shape[1])
    assert np.array_equal(plain[off, :n], seqs[off, :n])
    # judged WITHOUT the processors the same run has wrong steps: the judge sees the rule
    assert sj.judge(lg, seqs, rj.N_PROMPT, built.opt).count("wrong") > 0
