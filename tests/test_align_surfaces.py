"""CPU proof of the tools tests/test_gpu_align.py judges the word-timestamp kernels with (tests/align_surfaces.py): the exact surfaces
are exact, the oracle they are compared with is the installed HF code on exactly these inputs (NaN columns and ties included), the
restatement of the kernels' order of operations agrees with the oracle bit for bit, and the judge rejects eight wrong pipelines on
the very cases the GPU suite runs.  Seconds, no GPU."""
import warnings

import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests import align_surfaces as al

torch.set_grad_enabled(False)

ALL_CASES = [*al.EXACT_CASES, *al.GENERIC]


def test_case_names_are_unique_and_bounds_keep_the_stated_columns():
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
    for c in ALL_CASES:
        assert al.engine_columns(c.frames, c.T) == c.M, c.name
        assert c.seq_len <= 448 and c.N >= 1 and 0 <= c.M <= c.T, c.name


@pytest.mark.parametrize("case", al.EXACT_CASES, ids=lambda c: c.name)
def test_exact_cases_are_exact_and_the_kernel_order_agrees_with_the_oracle(case):
    """No rounding anywhere before the head mean: the reference's float32 matrix IS the float64 evaluation rounded once (NaN cells in
    the same places), and the kernels' order of operations (serial sums, fma, compare-exchange network, anti-diagonal DTW) gives the
    oracle's timestamps bit for bit.  What the GPU then shows is the kernels against this, not one summation order against another."""
    if case.M > 0:
        m32 = al.oracle_matrix(case)
        assert np.array_equal(m32, al.matrix64(case).astype(np.float32), equal_nan=True)
        w = al.surface(case)[:, case.n_prompt:, :case.M]
        assert np.array_equal(al.mirror_matrix(w), m32, equal_nan=True)
        if case.const and case.N > 1:
            assert np.isnan(m32).any() == ("run5" in case.name)          # a single NaN per window drops out; five reach the DTW
        if case.N == 1:
            assert np.isnan(m32).all()
    got = al.mirror(case)
    assert np.array_equal(got, al.oracle_timestamps(case))
    assert al.judge(case, got)


def test_exact_surfaces_hold_the_stated_values():
    """a + d * s with s a placement of one of the three patterns: column sums N * a, z-scores from {0, +-0.5, +-1, +-2, +-2.5}."""
    seen = set()
    for case in (al.HEADS[2], al.HEADS[3], al.N_SWEEP[1]):
        w = al.surface(case)[:, case.n_prompt:].astype(np.float64)
        mean = w.mean(1, keepdims=True)
        assert np.array_equal(mean * 64, np.rint(mean * 64))
        z = (w - mean) / w.std(1, keepdims=True)
        seen |= set(np.unique(z).tolist())
        assert (al.surface(case)[:, :case.n_prompt] == np.float32(1.0 / case.T)).all()
    assert seen == {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 2.5, -2.5}
    # banded: the rows above a column's mean gather around row j * N / M; random: they do not
    for c, lo, hi in ((al.HEADS[3], 0.8, 1.0), (al.HEADS[2], -0.3, 0.3)):
        w = al.surface(c)[0, c.n_prompt:, :c.M].astype(np.float64)
        above = w > w.mean(0, keepdims=True)
        centroid = (above * np.arange(c.N)[:, None]).sum(0) / above.sum(0)
        assert lo < np.corrcoef(centroid, np.arange(c.M))[0, 1] < hi, c.name


def test_poisoned_keeps_the_cells_the_reference_reads_and_nothing_else():
    c = al.PROMPTS[2]
    p = al.poisoned(c, extra_rows=2)
    assert p.shape == (c.Ha, c.n_rows + 2, c.T)
    kept = p[:, c.n_prompt:c.n_rows, :c.M]
    assert np.array_equal(kept, al.surface(c)[:, c.n_prompt:, :c.M]) and np.isfinite(kept).all()
    rest = p.copy()
    rest[:, c.n_prompt:c.n_rows, :c.M] = np.nan
    assert (np.isnan(rest) | (rest == np.float32(1e30))).all() and (rest == np.float32(1e30)).any()


# ---------------------------------------------------------------------------------------------------------------- HF pin
@pytest.fixture(scope="module")
def micro_hf():
    dims = wo.PRESETS["micro"]
    return dims, hr.build_hf_model(dims, wo.make_weights(dims, 0))


HF_CASES = [c for c in [*al.M_SWEEP, *al.PROMPTS, *al.BATCH, *al.ZERO_VARIANCE, al.N_SWEEP[0]] if c.Ha <= 4 and c.N * c.M <= 4000]


@pytest.mark.parametrize("case", HF_CASES, ids=lambda c: c.name)
def test_oracle_matches_hf_extract_token_timestamps_on_small_surfaces(micro_hf, case):
    """Same construction as tests/test_oracle_vs_hf.py::test_token_timestamp_cropping_matches_hf_for_every_num_frames_flavour: the
    installed `_extract_token_timestamps` on the case's surface and bound - ties, NaN columns, N = 1 and the short axes included."""
    from transformers.generation.utils import GenerateEncoderDecoderOutput

    dims, hf = micro_hf
    heads = [(l, h) for l in range(dims.dec_layers) for h in range(dims.heads)][:case.Ha]
    probs = al.surface(case)[None].copy()
    steps = []
    for i in range(case.n_rows):
        layers = [torch.zeros(1, dims.heads, 1, case.T) for _ in range(dims.dec_layers)]
        for a, (l, h) in enumerate(heads):
            layers[l][:, h, 0, :] = torch.from_numpy(probs[:, a, i, :])
        steps.append(tuple(layers))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        go = GenerateEncoderDecoderOutput(sequences=torch.zeros((1, case.seq_len), dtype=torch.long), cross_attentions=tuple(steps))
        ref = hf._extract_token_timestamps(go, heads, num_frames=case.frames, num_input_ids=case.n_prompt).numpy()
    assert np.array_equal(al.oracle_timestamps(case)[None], ref)


def test_median_filter_orders_nan_last_as_hf_does():
    from transformers.models.whisper.generation_whisper import _median_filter

    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, 23)).astype(np.float32)
    for r in range(200):                                   # one to five NaN per row, at the edges too
        x[r, rng.choice(23, 1 + r % 5, replace=False)] = np.nan
    x[0, 0] = x[1, 22] = np.nan
    for m in (4, 5, 7, 8, 23):
        want = _median_filter(torch.from_numpy(x[None, None, :, :m].copy()), 7).numpy()[0, 0]
        assert np.array_equal(wo.median_filter(x[:, :m], 7), want, equal_nan=True)
        # the compare-exchange network under the NaN-last rule is that sort; with fmin/fmax it is not
        win = np.lib.stride_tricks.sliding_window_view(np.pad(x[:, :m], [(0, 0), (3, 3)], mode="reflect"), 7, axis=-1)
        cols = [win[..., k] for k in range(7)]
        assert np.array_equal(al._median7(cols, "nanlast"), want, equal_nan=True)
        assert not np.array_equal(al._median7(cols, "fminmax"), want, equal_nan=True)


def test_dtw_matches_hf_on_ties_and_on_nan_cells():
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping

    rng = np.random.default_rng(4)
    ties = rng.integers(-2, 3, (12, 31)).astype(np.float64) * 0.5
    flat = np.zeros((7, 9))
    holes = rng.standard_normal((11, 40))
    holes[:, 17:22] = np.nan
    holes[4, 3] = np.nan
    allnan = np.full((1, 6), np.nan)
    for m in (ties, flat, holes, allnan):
        a, b = wo.dtw(m)
        ra, rb = _dynamic_time_warping(m)
        assert np.array_equal(a, ra) and np.array_equal(b, rb)
        jumps = np.pad(np.diff(a), (1, 0), constant_values=1).astype(bool)
        assert np.array_equal(al.mirror_dtw((-m).astype(np.float32)), b[jumps])          # the anti-diagonal order, same path


# ---------------------------------------------------------------------------------------------------------------- the judge
@pytest.mark.parametrize("name", list(al.WRONG_MIRRORS))
def test_the_judge_rejects_every_wrong_mirror(name):
    """Each wrong pipeline, run through the same judge on the cases of the GPU suite, is rejected by at least one of them: a case list
    that loses its power against one of these mistakes fails here."""
    wrong = al.WRONG_MIRRORS[name]
    cases = sorted((c for c in ALL_CASES if c.M > 0), key=lambda c: c.N * c.M)
    rejected = next((c.name for c in cases if c.N * c.M <= 20000 and not al.judge(c, al.mirror(c, **wrong))), None)
    assert rejected is not None, name
    print(f"{name}: first rejected by {rejected}")


def test_the_median_network_of_old_fails_every_constant_column_case():
    for c in al.ZERO_VARIANCE:
        if c.const:
            v = al.judge(c, al.mirror(c, median="fminmax"))
            assert not v and v.differing > 0, c.name


def test_tie_break_mistakes_move_tokens_on_the_exact_surfaces_at_no_cost():
    """Why array_equal and not the margin rule: the wrong tie-breaks move many tokens on a path that costs exactly the optimum."""
    from tests.util import dtw_jump_margins

    c = al.HEADS[3]
    want = al.oracle_timestamps(c)
    for tie in ("nonstrict", "up_first"):
        got = al.mirror(c, tie=tie)
        moved = got[c.n_prompt:c.n_rows] != want[c.n_prompt:c.n_rows]
        frames = np.rint(got[c.n_prompt:c.n_rows] / 0.02).astype(int)
        margins, _ = dtw_jump_margins(al.oracle_matrix(c), frames)
        assert moved.sum() >= c.N // 4 and np.abs(margins[moved]).max() < 1e-4
        assert not al.judge(c, got)


# ---------------------------------------------------------------------------------------------------------------- generic cases
@pytest.mark.parametrize("case", al.GENERIC, ids=lambda c: c.name)
def test_generic_cases_need_no_excuse_in_the_kernel_order(case):
    """delta is the float32 rounding the reference itself carries (its matrix against a float64 evaluation of the same steps), eps =
    4 (N + M) delta.  The seeds are chosen so that the kernels' order of operations lands on the reference's path outright: the 2 %
    allowance of the judge is for the GPU's own rounding, not needed by the arithmetic as written."""
    s = al.surface(case)[:, case.n_prompt:]
    assert np.abs(s.sum(-1) - 1).max() < 1e-5 and s.min() > 0
    delta, eps = al.delta_eps(case)
    print(f"{case.name}: delta {delta:.3e} eps {eps:.3e}")
    # z-scores of magnitude <= ~10 summed over N <= 100 rows in float32: delta is of the order N * 2^-24 * |z|
    assert 0 < delta < 1e-4 and eps == 4 * (case.N + case.M) * delta
    v = al.judge(case, al.mirror(case))
    assert v and v.differing == 0 and v.excused == 0, v.detail
    assert not al.judge(case, al.mirror(case, dup_last=False))      # what is not a generated token's own time is never excused
