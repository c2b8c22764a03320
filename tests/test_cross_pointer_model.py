"""What tests/test_gpu_cross.py relies on, checked on the numpy oracle (no GPU): tests/cross_pointer_model.py really points, every frame and
every fragment / chunk edge is pointed at, and a kernel that dropped a pointed-at key, paired it with its neighbour's value or read the
neighbouring stream's arena could not pass - while on unchanged random weights the same faults are invisible in 16 bits.

Figures (``pytest tests/test_cross_pointer_model.py -s`` prints them), T = 500 / T = 1500:
  * smallest score margin m_min 26.49 / 26.25 (needed 12), so the probability on a target is >= 1 - T exp(-m_min) = 1 - 2e-9 / 1 - 6e-9
    (1.0 in float32) and the GPU test's floor 1 - T exp(-(m_min - 1)) is 1 - 4e-9 / 1 - 2e-8; largest |logit| 22.0 / 24.2;
  * hiding a frame of BND(T) or swapping its value with the next one's moves every query pointing at it by 0.323 / 0.311 relative L2 or
    more (needed 0.12 = 4 x the bf16 tolerance) and no other query at all (0.0; allowed 1e-5);
  * the neighbouring stream's K/V: median 0.236 / 0.228 (needed 0.12), minimum 0.061 / 0.051 (stated, not a gate);
  * OracleWhisperMXFP8 at T = 500, W8A16 and W8A8 alike: m_min 25.50, hiding a frame moves a pointing query by 0.324 or more (needed
    0.3 = 3 x the 0.1 bound of the fp8 GPU cases, so A and BETA stay); the restatements are 6.0e-2 / 7.1e-2 from the float32 oracle at the
    worst (stream, step): one frame's e4m3 value row is the whole attended value here, where on random weights hundreds average;
  * random weights (test_decoder_teacher_forced's micro model), one cross key hidden from every query: relative L2 of the logits median
    1.4e-3, maximum 5.3e-3 at T = 500; median 4.3e-4, maximum 1.9e-3 at T = 1500 - a sixth of the bf16 tolerance at the worst;
  * the float32 oracle at T = 500 is 5.5e-7 relative L2 per (stream, step) from its own float64 run, 9.7e-12 in an alignment-row entry.
"""
import functools

import numpy as np
import pytest

from oracle import whisper_oracle as wo
from tests import cross_pointer_model as xm
from tests.util import PROMPT, clips, dims_variant, rel_l2

SIZES = [1500, 500]         # the three-chunk kernel and the single-pass one (last: the tests behind the sized ones share its build)
SMALL = SIZES[-1]
BF16_TOL = 3e-2             # tests/test_gpu_parity.py
POWER = 4 * BF16_TOL        # conditions on the construction, not tolerances: below them, change the construction
FP8_POWER = 3 * 0.1         # 0.1: the fp8 cases' bound against exact arithmetic in tests/test_gpu_cross.py
M_MIN = 12.0
OTHERS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    oracle_run.cache_clear()          # 0.34 GB of oracle logits at T = 1500: not kept for the rest of the session
    xm.build.cache_clear()


@pytest.fixture(scope="module", params=SIZES)
def T(request):
    """Module scope: pytest runs every test of one size before the next size, so `oracle_run` is computed once per size."""
    return request.param


@functools.lru_cache(maxsize=1)
def oracle_run(T):
    """(built, oracle, encoder output, hidden, targets, logit norms) of the unchanged model."""
    b = xm.build(T)
    om = wo.OracleWhisper(b.dims, b.weights, T=T)
    hidden, cross = xm.hidden_of(om, b.ids, b.enc)
    assert np.array_equal(cross, b.cross)
    return b, om, b.enc, hidden, xm.targets(b.ids, b.g), xm.LogitNorms(om)


def test_the_construction_is_exact_where_it_claims_to_be(T):
    b, om, enc, hidden, _, norms = oracle_run(T)
    table = b.weights["model.encoder.embed_positions.weight"]
    assert np.array_equal(om.enc_pos, table), "A0 is the identity at max_source_positions = T"
    c = xm.codes(T)
    assert (c.sum(1) == 0).all() and set(np.unique(c)) == {-1.0, 1.0}
    dots = c @ c.T - 64 * np.eye(T, dtype=np.float32)
    assert dots.max() <= xm.MAX_DOT
    some = [0, 1, 2, xm.B - 1]                        # (the conv stem is most of an oracle pass: four streams' layers are formed again)
    out, layers = om.encode(b.mel[some], return_layers=True)
    stem = layers[0]
    assert np.array_equal(out, enc[some])
    assert np.array_equal(stem[..., :xm.HALF], np.broadcast_to(xm.A * c, stem[..., :xm.HALF].shape)), "the code half: exact, the same for every stream"
    assert np.array_equal(layers[1], layers[0]), "encoder layer 0 is the identity"
    other = stem[..., xm.HALF:]
    apart = min(float(np.abs(other[s] - other[s + 1]).mean()) for s in range(len(some) - 1))
    assert apart > 1e-3, "the other half carries the stream's audio"
    assert np.array_equal(om._dec_logits(hidden[:2]), b.logits[:2]), "hidden_of is OracleWhisper.decode in front of the tied projection"
    for p in range(4):                                # the Gram-matrix norm against the logits formed outright
        direct = rel_l2(b.logits[1, p], b.logits[0, p])
        assert abs(norms.rel_l2(hidden[1, p], hidden[0, p]) - direct) < 1e-5 * direct
    print(f"T={T}: largest code dot product {dots.max():.0f}, mean |difference| of the audio half between neighbouring streams {apart:.3f} at the least")


def test_every_query_is_saturated_on_its_target(T):
    b, _, _, _, tg, _ = oracle_run(T)
    m = xm.margins(b.cross, tg)
    floor = xm.floor_probability(T, m.min())
    print(f"T={T}: smallest score margin {m.min():.2f} (head 0 {m[:, 0].min():.2f}, head 1 {m[:, 1].min():.2f}; needed {M_MIN:g}); probability on a target "
          f">= 1 - {T * np.exp(-m.min()):.1e}; the GPU test's floor {floor:.8f}; max |logit| {np.abs(b.logits).max():.1f}")
    assert np.array_equal(b.cross.argmax(-1), tg)
    assert m.min() >= M_MIN and floor >= 0.999
    assert np.take_along_axis(b.cross, tg[..., None], -1).min() >= 1.0 - T * np.exp(-m.min()) - 1e-6
    assert np.abs(b.logits).max() < 30.0          # test_gpu_score's Z_MAX, behind its 1e-4, is 60


def test_every_frame_and_every_boundary_is_pointed_at(T):
    P = xm.positions(T)
    ids, g, bnd = xm.pointer_ids(T, P), xm.frame_map(T, P), xm.boundaries(T)
    assert P % 32 == 0 and 16 * P >= T and 16 * (P - 32) < T and P == {500: 32, 1500: 96}[T]
    assert ids.shape == (17, P) and ids.dtype == np.int32 and (ids < T).all() and (ids >= 0).all()
    assert set(ids.ravel().tolist()) == set(range(T)), "every frame is head 0's target of some (stream, position)"
    assert {0, 1, 63, 64, 65, T - 2, T - 1} <= set(bnd) and (T < 1500 or {511, 512, 513, 1023, 1024, 1025} <= set(bnd))
    assert set(bnd) <= set(ids[:16].ravel().tolist()) and set(bnd) == set(ids[16].tolist()) and set(bnd) == set(g.tolist())
    assert (ids[16] != g).all(), "stream 16: the two heads point at different frames"
    assert np.array_equal(xm.targets(ids, g)[:, 0], ids) and (xm.targets(ids, g)[:, 1] == g).all()


def test_a_hidden_key_a_displaced_value_or_the_neighbours_arena_moves_the_logits(T):
    b, om, enc, hidden, tg, norms = oracle_run(T)
    worst, leak = np.inf, 0.0
    for k in xm.boundaries(T):
        for name, hook, partner in (("hidden", xm.hide_key(k), k), ("value swapped", xm.swap_values(k), xm.swap_partner(k, T))):
            moved = norms.rel_l2(xm.hidden_of(om, b.ids, enc, hook)[0], hidden)                # [B, P]
            at = (tg == k).any(1)
            others = ~at & ~(tg == partner).any(1)
            assert at[:16].any() and at[16].any(), k
            worst, leak = min(worst, float(moved[at].min())), max(leak, float(moved[others].max()))
            assert moved[at].min() >= POWER, (k, name, float(moved[at].min()), np.argwhere(at & (moved < POWER))[:3].tolist())
            assert moved[others].max() <= OTHERS, (k, name, float(moved[others].max()))
    nb = norms.rel_l2(xm.hidden_of(om, b.ids, enc, xm.neighbour_stream)[0], hidden)
    print(f"T={T}: smallest move of a pointing query's logits under a hidden key or a swapped value {worst:.3f} relative L2 (needed {POWER:g}); largest "
          f"move of any other query {leak:.1e} (allowed {OTHERS:g}); the neighbouring stream's K/V: median {np.median(nb):.3f} (needed {POWER:g}), "
          f"minimum {nb.min():.3f}, maximum {nb.max():.3f}")
    assert np.median(nb) >= POWER


@pytest.mark.parametrize("act_quant", [False, True])
def test_the_fp8_restatements_point_as_sharply(act_quant):
    """OracleWhisperMXFP8 (W8A16: act_quant=False, W8A8: True) at T = 500: cross K/V through the e4m3 round trip, quantised weights."""
    T = SMALL
    b = xm.build(T)
    oq = wo.OracleWhisperMXFP8(b.dims, b.weights, T=T, act_quant=act_quant)
    enc = b.enc
    hidden, cross = xm.hidden_of(oq, b.ids, enc)
    tg = xm.targets(b.ids, b.g)
    m = xm.margins(cross, tg)
    away = max(rel_l2(zq, z) for s in range(xm.B) for zq, z in zip(oq._dec_logits(hidden[s]), b.logits[s]))
    # one pass over len(BND) copies of the streams, copy j without frame BND[j] (a restatement pass costs as much as its quantiser calls)
    bnd, n = xm.boundaries(T), xm.B
    mutants = xm.hidden_of(oq, np.tile(b.ids, (len(bnd), 1)), np.tile(enc, (len(bnd), 1, 1)), xm.hide_key_per_block(bnd, n))[0]
    at = [np.nonzero((tg == k).any(1)) for k in bnd]          # (stream, position) of the queries pointing at each frame
    assert all(len(a[0]) for a in at)
    base = oq._dec_logits(np.concatenate([hidden[a] for a in at]))
    mut = oq._dec_logits(np.concatenate([mutants[j * n:(j + 1) * n][a] for j, a in enumerate(at)]))
    moved = np.array([rel_l2(x, y) for x, y in zip(mut, base)])
    worst = float(moved.min())
    assert worst >= FP8_POWER, (np.repeat(bnd, [len(a[0]) for a in at])[moved < FP8_POWER].tolist(), worst)
    print(f"T={T} act_quant={act_quant}: smallest score margin {m.min():.2f} (needed {M_MIN:g}), floor {xm.floor_probability(T, m.min()):.8f}; smallest move "
          f"of a pointing query's logits under a hidden key {worst:.3f} (needed {FP8_POWER:g}); at most {away:.1e} from the float32 oracle per (stream, step)")
    assert np.array_equal(cross.argmax(-1), tg) and m.min() >= M_MIN and xm.floor_probability(T, m.min()) >= 0.999


@pytest.mark.parametrize("T", SIZES)
def test_on_random_weights_a_hidden_cross_key_is_below_the_bf16_tolerance(T):
    """The figure that motivates the file: test_decoder_teacher_forced's micro model and ids, one cross key hidden from every query of every
    layer - the existing reduced-precision cases cannot see it."""
    dims = dims_variant("micro", enc_layers=1, dec_layers=2)
    w = wo.make_weights(dims, 2)
    Bn = 3
    om = wo.OracleWhisper(dims, w, T=T)
    enc = om.encode(wo.log_mel(clips(T * 320, Bn), dims.n_mels))
    ids = np.concatenate([np.tile(np.array(PROMPT), (Bn, 1)), np.random.default_rng(3).integers(0, 50000, size=(Bn, 6))], axis=1)
    base = om.decode(ids, om.new_cache(enc))[0]
    moved = []
    for k in xm.boundaries(T):
        cache = om.new_cache(enc)
        xm.hide_key(k)(cache)
        z = om.decode(ids, cache)[0]
        moved += [rel_l2(z[s, p], base[s, p]) for s in range(Bn) for p in range(ids.shape[1])]
    print(f"random weights, T={T}: one cross key hidden from every query moves the logits by {np.median(moved):.1e} relative L2 (median), "
          f"{max(moved):.1e} (maximum); bf16 tolerance {BF16_TOL:g}")
    assert max(moved) < BF16_TOL


def test_the_float32_oracle_is_within_a_tenth_of_the_f32_bounds_of_its_float64_run():
    """tests/test_gpu_cross.py holds the f32 engine to 2e-5 relative L2 per (stream, step) and to 1e-4 per alignment-row entry against the
    float32 oracle: both bounds must be at least 10 times the oracle's own distance from a float64 run of itself."""
    b = xm.build(SMALL)
    o64 = wo.OracleWhisper(b.dims, b.weights, T=SMALL, dtype=np.float64)
    z64, c64 = o64.decode(b.ids, o64.new_cache(o64.encode(b.mel)), want_cross=xm.HEADS)
    d_z = max(rel_l2(b.logits[s, p], z64[s, p]) for s in range(xm.B) for p in range(b.ids.shape[1]))
    d_c = float(np.abs(b.cross - c64).max())
    print(f"float32 oracle against float64 at T={SMALL}: logits {d_z:.2e} relative L2 per (stream, step) at most, alignment rows {d_c:.2e}")
    assert d_z <= 2e-5 / 10 and d_c <= 1e-4 / 10
