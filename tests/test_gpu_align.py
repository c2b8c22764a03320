"""Word timestamps (k_dtw.hip through tw_token_timestamps) on alignment surfaces put in with tw_set_alignment: no decoder runs here.
The surfaces, the oracle's results and the judge come from tests/align_surfaces.py, whose claims tests/test_align_surfaces.py proves
on the CPU.  Exact, zero-variance and N = 1 surfaces: the engine's timestamps EQUAL the oracle's (np.array_equal; the judge does
nothing else for them).  Generic surfaces: the margin rule under the eps derived from the reference's own float32 rounding, at most
2 % of a case's tokens.  Run on the MI355X: ``pytest -m gpu``."""
import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import align_surfaces as al
from tests.util import dims_variant, make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _model(Ha):
    """The smallest model with Ha alignment heads: micro (2 x 2 heads), micro80 (2 x 3), micro with five decoder layers (5 x 2)."""
    dims = wo.PRESETS["micro"] if Ha <= 2 else wo.PRESETS["micro80"] if Ha == 6 else dims_variant("micro", dec_layers=5)
    heads = [(l, h) for l in range(dims.dec_layers) for h in range(dims.heads)]
    heads = heads[-Ha:] if Ha <= 2 else heads
    assert len(heads) == Ha, (Ha, heads)
    return dims, heads


@pytest.fixture(scope="module")
def contexts():
    """Contexts that never decode, made on first use and shared: key (Ha, T, max_batch, tag)."""
    made, weights = {}, {}

    def get(Ha, T=300, max_batch=3, tag=""):
        key = (Ha, T, max_batch, tag)
        if key not in made:
            dims, heads = _model(Ha)
            if dims not in weights:
                weights[dims] = wo.make_weights(dims, 0)
            made[key] = make_engine(dims, weights[dims], T=T, max_batch=max_batch, dtype="f32", heads=heads)
        return made[key]

    yield get
    for eng in made.values():
        eng.close()


def run(eng, cases, poison=False):
    """One tw_token_timestamps call over `cases` (one per slot; same Ha, T, n_prompt, N) -> float32 [B, seq_len]."""
    c0 = cases[0]
    assert all((c.Ha, c.T, c.n_prompt, c.N) == (c0.Ha, c0.T, c0.n_prompt, c0.N) for c in cases)
    eng.set_alignment(np.stack([al.poisoned(c) if poison else al.surface(c) for c in cases]))
    return eng.token_timestamps(len(cases), c0.n_prompt, c0.seq_len, [c.frames for c in cases])


def check(case, ts):
    v = al.judge(case, ts)
    assert v, v.detail
    return v


def test_set_alignment_round_trip_and_argument_checks(contexts):
    eng = contexts(2)
    rng = np.random.default_rng(0)
    a = rng.random((3, 2, 10, 300), dtype=np.float32)
    a[0, 0, 0, 0], a[2, 1, 9, 299], a[1, 0, 3, 7] = np.nan, -np.inf, 1e30          # bits, not values
    eng.set_alignment(a)
    assert np.array_equal(eng.get_alignment(3, 10).view(np.uint32), a.view(np.uint32))
    b = rng.random((2, 2, 5, 300), dtype=np.float32)
    eng.set_alignment(b)                                                         # rows 5.. and slot 2 keep what they held
    want = a.copy()
    want[:2, :, :5] = b
    assert np.array_equal(eng.get_alignment(3, 10).view(np.uint32), want.view(np.uint32))
    full = rng.random((1, 2, 448, 300), dtype=np.float32)                         # every row of a slot
    eng.set_alignment(full)
    assert np.array_equal(eng.get_alignment(1, 448), full)
    with pytest.raises(RuntimeError, match="bad B/n_rows"):
        eng.set_alignment(np.zeros((4, 2, 5, 300), np.float32))                   # more slots than the context has
    with pytest.raises(RuntimeError, match="bad B/n_rows"):
        eng.set_alignment(np.zeros((1, 2, 449, 300), np.float32))
    with pytest.raises(ValueError):
        eng.set_alignment(np.zeros((1, 2, 5, 299), np.float32))
    with pytest.raises(ValueError):
        eng.set_alignment(np.zeros((1, 1, 5, 300), np.float32))
    assert np.array_equal(eng.get_alignment(1, 448), full)                        # the refused calls wrote nothing


@pytest.mark.parametrize("case", al.M_SWEEP, ids=lambda c: c.name)
def test_m_sweep(contexts, case):
    """Kept columns 1 .. 9 (M <= 3 passes the median filter by; 4 .. 9 reflect across both edges of a window at once), the 256-thread
    block edges of the two column kernels, and all T columns; each bound given as 2M and as 2M + 1."""
    check(case, run(contexts(2), [case])[0])


@pytest.mark.parametrize("case", al.N_SWEEP, ids=lambda c: c.name)
def test_n_sweep(contexts, case):
    check(case, run(contexts(2), [case])[0])


@pytest.mark.parametrize("case", al.HEADS, ids=lambda c: c.name)
def test_heads(contexts, case):
    """1, 2, 6 (turbo) and 10 (large-v3) alignment heads; the head mean divides an exact sum once on both sides."""
    check(case, run(contexts(case.Ha), [case])[0])


def test_largest_problem(contexts):
    """444 tokens x 1500 frames in both streams of one call, the second under a negative bound."""
    ts = run(contexts(2, T=1500, max_batch=2), al.LARGEST)
    for c, row in zip(al.LARGEST, ts):
        check(c, row)


def test_stale_work_buffers(contexts):
    """zbuf / mat / trace after the largest call hold its values at other strides: a small call behind it must not see them."""
    eng = contexts(2, T=1500, max_batch=2)
    run(eng, al.LARGEST)
    small = al.SMALL_AFTER_LARGEST
    after = run(eng, [small])[0]
    fresh = run(contexts(2, T=1500, max_batch=1, tag="fresh"), [small])[0]
    assert np.array_equal(after, fresh)
    check(small, after)


@pytest.mark.parametrize("case", al.PROMPTS, ids=lambda c: c.name)
def test_prompt_lengths_on_poisoned_buffers(contexts, case):
    """Prompt rows, rows behind n_rows and columns >= M hold NaN / 1e30: the reference crops them, nothing of them may arrive."""
    ts = run(contexts(2), [case], poison=True)[0]
    assert (ts[:case.n_prompt] == 0).all()
    check(case, ts)
    assert np.array_equal(ts, run(contexts(2), [case])[0])


def test_batch_of_different_surfaces_and_bounds(contexts):
    eng = contexts(2)
    ts = run(eng, al.BATCH)
    for c, row in zip(al.BATCH, ts):
        check(c, row)
        assert np.array_equal(row, run(eng, [c])[0]), c.name                     # = the stream's own single call
    order = [2, 0, 1]
    assert np.array_equal(run(eng, [al.BATCH[i] for i in order]), ts[order])      # whichever slot it sits in
    none = al.BATCH[0]
    assert (ts[0, none.n_prompt:] == np.float32(-0.02)).all() and (ts[0, :none.n_prompt] == 0).all()


@pytest.mark.parametrize("case", al.ZERO_VARIANCE, ids=lambda c: c.name)
def test_zero_variance_columns_and_single_row(contexts, case):
    """Columns that hold one value in all N rows z-score to NaN.  The reference sorts NaN last: one NaN drops out of its neighbours'
    median windows, five in a row make NaN medians that reach the DTW; with N = 1 every cell is NaN.  Regression test of the
    compare-exchange rule of align_median_mean_kernel (fminf / fmaxf dropped the NaN: every zv_* case differed)."""
    check(case, run(contexts(case.Ha), [case])[0])


@pytest.mark.parametrize("case", al.GENERIC, ids=lambda c: c.name)
def test_generic_surfaces(contexts, case):
    delta, eps = al.delta_eps(case)
    v = check(case, run(contexts(case.Ha), [case])[0])
    print(f"{case.name}: delta {delta:.3e} eps {eps:.3e}; {v.differing} of {case.N} tokens differ, {v.excused} excused")
    assert v.excused <= al.MAX_EXCUSED * case.N
