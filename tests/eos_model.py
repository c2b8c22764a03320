"""A micro model WITH decoder layers whose streams reach <eos> at different steps, and some never.  No GPU in here.

`wo.make_weights(PRESETS["micro"], 0)` does not emit <eos> within 90 tokens on the suite's clips, nor with its <eos> row scaled by 3 to 6
(numpy oracle), so no test on it ever had a finished row beside a running one.  The recipe here takes the
sampler tables of the crafted zero-layer model `sampler_judge.crafted_model(V=1000, eos=700, no_ts=720, eos_scale=ES, ts_dir=1.0)` (the
ids of case `v1000-b33`: token embedding, positions, final LayerNorm) and puts them on two decoder layers of `make_weights`, so that the
next token depends on the audio and on the whole history (self-attention cache, cross attention, alignment rows) AND <eos> wins at
some steps.  TABLE holds, per setting, the number of generated tokens before each clip's <eos> by the numpy oracle; tests/test_eos_model.py
recomputes it, so that a change of `make_weights` or `synth_audio` fails there instead of leaving the GPU tests vacuous.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests import sampler_judge as sj
from tests.util import clips

V, EOS, NO_TS = 1000, 700, 720
T = 100
MAX_NEW = 40
N_CLIPS = 20
N_PROMPT = 3
HEADS = [(1, 0), (1, 1)]
_TABLES = ("embed_tokens.weight", "embed_positions.weight", "layer_norm.weight", "layer_norm.bias")

# (ES, timestamps) -> generated tokens before the <eos> of clips 0 .. 19 (None: no <eos> within MAX_NEW tokens)
_N = None
TABLE: Dict[Tuple[float, bool], Tuple[Optional[int], ...]] = {
    (2.0, True): (23, 25, _N, _N, 20, 12, _N, 12, _N, 15, _N, _N, 15, 15, _N, _N, 10, 18, _N, 23),
    (2.5, True): (10, 14, _N, 17, 13, 6, _N, 10, 16, 9, _N, 10, 10, 3, _N, _N, 10, 14, _N, 10),
    (2.0, False): (14, 12, _N, 10, 14, 18, _N, 10, _N, 25, _N, 10, 10, 18, _N, _N, 10, _N, _N, 15),
}
SETTINGS = list(TABLE)


@functools.lru_cache(maxsize=None)
def model(es: float):
    """(dims, weights): two decoder layers of make_weights(seed 0) under the crafted sampler tables, <eos> row x `es`.  Shared: read only."""
    dims, w0 = sj.crafted_model(V=V, eos=EOS, no_ts=NO_TS, seed=0, eos_scale=es, ts_dir=1.0)
    dims = dataclasses.replace(dims, dec_layers=2)
    w = dict(wo.make_weights(dims, 0))
    for name in _TABLES:
        w["model.decoder." + name] = w0["model.decoder." + name]
    return dims, w


def audio(sel: Sequence[int]) -> np.ndarray:
    """float32 [len(sel), T * 320]: the suite's clips with these indices."""
    return clips(T * 320, N_CLIPS)[list(sel)]


def prompt(sel: Sequence[int]) -> np.ndarray:
    """int32 [len(sel), 3]: `sampler_judge.case_prompt`'s rows of these clips ([3, 5, 9 + 7 b])."""
    return np.array([[3, 5, 9 + 7 * int(b)] for b in sel], dtype=np.int32)


def options(timestamps: bool, max_new: int = MAX_NEW, heads=None) -> wo.GreedyOptions:
    return wo.GreedyOptions(eos=EOS, pad=EOS, max_new_tokens=max_new, min_new_tokens=0, begin_suppress=(), suppress=(),
                            timestamps=timestamps, no_timestamps_id=NO_TS, alignment_heads=heads)


def engine_kw(timestamps: bool, max_new: int = MAX_NEW) -> dict:
    """The same options as keyword arguments of WhisperEngine.generate_greedy."""
    return dict(max_new_tokens=max_new, min_new_tokens=0, eos_id=EOS, pad_id=EOS, timestamps=timestamps, no_timestamps_id=NO_TS,
                begin_suppress=(), suppress=(), want_alignment=True)


# the biased two-row case, per setting: (text id X, tokens row 0 then generates before its <eos>, the token the row would get BEHIND its
# <eos> if it were decoded on).  X is chosen so that this last one is not <eos> (= pad): a call that decodes a finished row on then
# returns other ids than the plain call (with most X the model answers <eos> with <eos> and such a call would go unnoticed)
BIAS_CASE: Dict[Tuple[float, bool], Tuple[int, int, int]] = {(2.0, True): (200, 32, 257), (2.5, True): (400, 9, 946), (2.0, False): (11, 23, 257)}


def bias_rows(gen: np.ndarray, es: float, timestamps: bool) -> list:
    """`sequence_bias_rows` of the biased two-row case, from the UNBIASED run's generated tokens: ONE two-token sequence on row 0 (the row
    that ends) - the row's second generated token followed by BIAS_CASE's text id, bias 8 - and none on row 1.  By the oracle
    (tests/test_eos_model.py) the bias changes row 0 from its third token on and the row still ends."""
    return [{(int(gen[0][1]), BIAS_CASE[(es, timestamps)][0]): 8.0}, None]


def eos_steps(gen: np.ndarray, eos: int = EOS) -> List[Optional[int]]:
    """Per row of `gen` (generated tokens, prompt cut off): the number of tokens before the row's <eos>, None without one."""
    return [int(np.nonzero(r == eos)[0][0]) if (r == eos).any() else None for r in np.asarray(gen)]


@functools.lru_cache(maxsize=None)
def _oracle_run(es: float, timestamps: bool, sel: Tuple[int, ...], max_new: int) -> np.ndarray:
    dims, w = model(es)
    om = wo.OracleWhisper(dims, w, T=T)
    seq = wo.greedy_generate(om, om.encode(wo.log_mel(audio(sel), dims.n_mels)), prompt(sel), options(timestamps, max_new))["sequences"]
    seq.setflags(write=False)
    return seq


def oracle_run(es: float, timestamps: bool, sel: Sequence[int], max_new: int = MAX_NEW) -> np.ndarray:
    """The numpy oracle's sequences [len(sel), L] for these clips (computed once per process, read-only)."""
    return _oracle_run(float(es), bool(timestamps), tuple(int(i) for i in sel), int(max_new))


@dataclasses.dataclass(frozen=True)
class Batch:
    """A batch selection a GPU test uses, with what the test relies on (tests/test_eos_model.py asserts it on the oracle's table)."""
    name: str
    es: float
    timestamps: bool
    sel: Tuple[int, ...]
    all_finish: Optional[bool]      # True: every row ends; False: some row never ends; None: the case does not care

    def steps(self) -> List[Optional[int]]:
        return [TABLE[(self.es, self.timestamps)][i] for i in self.sel]


B20 = tuple(range(20))
BATCHES: List[Batch] = (
    [Batch(f"b2-es{es}-ts{int(ts)}", es, ts, (5, 2), False) for es, ts in SETTINGS]
    + [Batch("b5-all-end", 2.5, True, (0, 1, 3, 4, 5), True)]
    + [Batch(f"b16-es{es}-ts{int(ts)}", es, ts, tuple(range(16)), False) for es, ts in SETTINGS]
    + [Batch(f"b20-es{es}-ts{int(ts)}", es, ts, B20, False) for es, ts in SETTINGS]
    + [Batch(f"b1-es{es}-ts{int(ts)}", es, ts, (5,), True) for es, ts in SETTINGS]
    + [Batch(f"b4-parity-es{es}-ts{int(ts)}", es, ts, (0, 1, 2, 3), False) for es, ts in ((2.5, True), (2.0, False))]
)


def batch(name: str) -> Batch:
    return next(b for b in BATCHES if b.name == name)


def check_batch(b: Batch, steps: Sequence[Optional[int]]):
    """What the GPU tests rely on, for the <eos> steps `steps` of the rows of `b` (the table's, or an engine's own plain call's)."""
    ended = [s for s in steps if s is not None]
    assert ended, (b.name, "no row ends")
    assert min(ended) >= 3, (b.name, "a row ends before three tokens", steps)
    if len(steps) > 1:
        assert len(set(steps)) > 1, (b.name, "every row ends at the same step", steps)
    if b.all_finish is True:
        assert len(ended) == len(steps), (b.name, "a row never ends", steps)
    if b.all_finish is False:
        assert len(ended) < len(steps), (b.name, "every row ends", steps)


# --------------------------------------------------------------------------------------------------------------------
# drafts that run past a row's <eos>
# --------------------------------------------------------------------------------------------------------------------
def draft_span(gen: np.ndarray, max_new: int, eos: int = EOS) -> int:
    """Tokens a draft may cover: up to the LONGEST row's <eos> step, or max_new - 2 where a row never ends."""
    steps = eos_steps(gen, eos)
    return min(max_new - 2, max(max_new if s is None else s for s in steps))


def filled_draft(gen: np.ndarray, n: int, rng: np.random.Generator, repeat_last: bool = False, eos: int = EOS) -> np.ndarray:
    """int32 [B, n]: each row's true continuation up to its own <eos>, and behind it filler that is not <eos> - random text ids, or
    (`repeat_last`) the row's own last tokens again: a previous tick that was longer than this tick's output.  Text ids are [0, eos)."""
    gen = np.asarray(gen)
    out = np.zeros((gen.shape[0], n), dtype=np.int32)
    for b, s in enumerate(eos_steps(gen, eos)):
        k = n if s is None else min(s, n)
        out[b, :k] = gen[b, :k]
        if k < n:
            if repeat_last and k > 0:
                tail = gen[b, max(0, k - 3):k]
                out[b, k:] = np.resize(tail, n - k)
            else:
                out[b, k:] = rng.integers(0, eos, size=n - k)
    assert not (out == eos).any()
    return out


def corrupt(draft: np.ndarray, row: int, at: int, eos: int = EOS) -> np.ndarray:
    """`draft` with the token of `row` at index `at` replaced by another text id (text ids are [0, eos))."""
    d = draft.copy()
    d[row, at] = (int(d[row, at]) + 1) % eos if int(d[row, at]) < eos else 1
    assert d[row, at] != draft[row, at] and d[row, at] != eos
    return d


# --------------------------------------------------------------------------------------------------------------------
# the situations of tests/test_gpu_draft.py's fuzz on this model
# --------------------------------------------------------------------------------------------------------------------
FUZZ_EOS_SEED = {"f32": 102, "bf16": 105, "f16": 106, "fp8a16": 109, "fp8a8": 113}     # each: 20 or more of 40 by the oracle's table


def fuzz_eos_situations(dtype, n=40):
    """The situations of the second half of the fuzz, drawn WITHOUT looking at any result (so that tests/test_eos_model.py can count, on
    the oracle's table, how many of them have a row ending inside the drafted span): dicts of es, timestamps, sel, max_new, u (the
    draft's length as a fraction of the span), rate, one_row, repeat."""
    rng = np.random.default_rng(FUZZ_EOS_SEED[dtype])
    out = []
    for case in range(n):
        es, ts_on = SETTINGS[int(rng.integers(0, len(SETTINGS)))]
        B = int(rng.choice([1, 2, 3, 5, 8, 16]))
        out.append(dict(es=es, timestamps=ts_on, sel=tuple(int(i) for i in rng.permutation(16)[:B]), max_new=int(rng.integers(16, 41)),
                        u=float(rng.random()), rate=float(rng.choice([0.0, 0.0, 0.03, 0.15, 0.5, 1.0])), one_row=bool(rng.integers(0, 2)),
                        repeat=bool(rng.integers(0, 2)), graph=bool(case % 2)))
    return out


def fuzz_eos_draft_length(steps, max_new, u):
    """(draft length, a row ends inside it) for rows that end after `steps` tokens (None: not within max_new)."""
    span = min(max_new - 2, max(max_new if s is None else s for s in steps))
    nd = 1 + min(span - 1, int(u * span)) if span >= 1 else 0
    return nd, any(s is not None and s < nd for s in steps)
