"""What tests/test_gpu_deep.py relies on, checked on the numpy oracle (no GPU): tests/pointer_model.py really points, every key and every
fragment edge is pointed at from every depth, and a kernel that dropped or displaced one pointed-at key could not pass.

Figures of P = 448 (``pytest tests/test_pointer_model.py -s`` prints them): smallest probability on a target 0.99999964, largest
|logit| 22.6, smallest move of a pointing query's logits under a mutant 0.240 relative L2 (needed: 0.09 = 3 x the bf16 tolerance; bf16
rounding itself costs about 6e-3); at P = 200 the float32 oracle is 4.0e-7 relative L2 from its own float64 run, 7.8e-6 in the
log-probability of the next id.
"""
import functools

import numpy as np
import pytest

from oracle import whisper_oracle as wo
from tests import pointer_model as pm
from tests.util import rel_l2

SIZES = [448, 200]          # every bucket of the self-attention kernel; a bound that is no multiple of 64
BF16_TOL = 3e-2             # tests/test_gpu_parity.py
POWER = 3 * BF16_TOL        # a condition on the construction, not a tolerance: below it, change the patterns


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    restated.cache_clear()          # 0.8 GB of oracle logits at P = 448: not kept for the rest of the session
    pm.build.cache_clear()


@pytest.fixture(scope="module", params=SIZES)
def P(request):
    """Module scope: pytest runs every test of one size before the next size, so `restated` is computed once per size."""
    return request.param


@functools.lru_cache(maxsize=1)
def restated(P):
    """(built, oracle, encoder output, hidden, probabilities) of the unhooked restated loop."""
    b = pm.build(P)
    om = wo.OracleWhisper(b.dims, b.weights, T=pm.T)
    enc = om.encode(b.mel)
    hidden, probs = pm.decode_hooked(om, b.ids, enc)
    return b, om, enc, hidden, probs


def test_the_restated_loop_is_the_oracles_decode(P):
    b, om, _, hidden, _ = restated(P)
    assert b.ids.shape == (len(pm.PATTERNS), P) and b.logits.shape == (len(pm.PATTERNS), P, b.dims.vocab) and b.logits.dtype == np.float32
    worst = 0.0
    for s in range(b.ids.shape[0]):          # stream by stream: [P, 51866] at a time
        got = pm.logits_of(om, hidden[s])
        worst = max(worst, float(np.abs(got - b.logits[s]).max()))
        assert np.allclose(got, b.logits[s], rtol=1e-5, atol=1e-5), s
    print(f"P={P}: restated loop against OracleWhisper.decode, max |difference| {worst:.2e}")


def test_every_query_is_saturated_on_its_target_and_the_logits_are_moderate(P):
    b, _, _, _, probs = restated(P)
    tg = pm.targets(b.ids)                                                    # [B, P, 2]
    on_target = np.take_along_axis(probs.transpose(0, 2, 1, 3), tg[..., None], axis=-1)[..., 0]   # [B, P, H]
    print(f"P={P}: smallest probability on a target {on_target.min():.8f} (head 0 {on_target[..., 0].min():.8f}, head 1 {on_target[..., 1].min():.8f}); "
          f"max |logit| {np.abs(b.logits).max():.1f}")
    assert on_target.min() >= 0.999
    assert np.abs(b.logits).max() < 30.0          # test_gpu_score's Z_MAX, behind its 1e-4, is 60


def test_every_key_and_every_boundary_is_pointed_at(P):
    ids = pm.pattern_ids(P)
    assert (ids <= np.arange(P)).all()
    later = [set(ids[:, k + 1:][ids[:, k + 1:] == k].tolist()) for k in range(P - 1)]
    assert all(later[k] == {k} for k in range(P - 1)), "every key 0 .. P-2 is head 0's target of some later query"
    assert (pm.targets(ids)[..., 1] == np.arange(P)).all(), "head 1: the query's own position"
    bnd = pm.boundaries(P)
    assert P - 2 in bnd and 0 in bnd and all(k in bnd for k in (63, 64, 65) if k < P)
    for m in bnd:
        for g in range(P // pm.GROUP):          # the whole groups of 64 query positions that begin behind key m
            if g * pm.GROUP > m:
                assert (ids[:, g * pm.GROUP:(g + 1) * pm.GROUP] == m).any(), (m, g)


def test_a_hidden_or_displaced_key_moves_every_query_that_points_at_it(P):
    b, om, enc, hidden, _ = restated(P)
    worst = np.inf
    for k in pm.boundaries(P):
        at = np.argwhere(b.ids[:, k + 1:] == k)           # (stream, position - k - 1) of the later queries pointing at k
        assert len(at), k
        rows = (at[:, 0], at[:, 1] + k + 1)
        base = pm.logits_of(om, hidden[rows])
        for name, hook in (("hidden", pm.hide_key(k)), ("swapped", pm.swap_with_next(k))):
            mut = pm.logits_of(om, pm.decode_hooked(om, b.ids, enc, hook)[0][rows])
            moved = [rel_l2(m, r) for m, r in zip(mut, base)]
            worst = min(worst, min(moved))
            assert min(moved) >= POWER, (k, name, min(moved), at[int(np.argmin(moved))].tolist())
    print(f"P={P}: smallest move of a pointing query's logits under a mutant {worst:.3f} relative L2 (needed {POWER:g})")


def test_the_float32_oracle_is_within_a_tenth_of_the_f32_bounds_of_its_float64_run():
    """tests/test_gpu_deep.py holds the f32 engine to 2e-5 relative L2 per step and to 1e-4 in the log-probability of the next id against the
    float32 oracle: both bounds must be at least 10 times the oracle's own distance from a float64 run of itself."""
    b = pm.build(SIZES[1])
    z64 = pm.oracle_logits(b.dims, b.weights, b.ids, b.mel, dtype=np.float64)
    per_step = [rel_l2(b.logits[:, p], z64[:, p]) for p in range(b.ids.shape[1])]

    def next_id_logprob(z):
        m = z.max(-1, keepdims=True)
        return np.take_along_axis(z - m - np.log(np.exp(z - m).sum(-1, keepdims=True)), b.ids[:, 1:, None].astype(np.int64), -1)

    d_lp = float(np.abs(next_id_logprob(b.logits[:, :-1].astype(np.float64)) - next_id_logprob(z64[:, :-1])).max())
    print(f"float32 oracle against float64: logits {max(per_step):.2e} relative L2 per step at most, log-probability of the next id {d_lp:.2e}")
    assert max(per_step) <= 2e-5 / 10 and d_lp <= 1e-4 / 10
