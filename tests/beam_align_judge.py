"""Token timestamps of beam hypotheses by the rule of include/thewhisper.h (tw_generate_beam_aligned), restated in numpy.  No GPU.

The rule: a hypothesis `h` of `len` tokens is timed on ITS OWN alignment rows n0 .. len - 2 - the rows of the beams it descends from -
and on nothing else, which is what HF's `_extract_token_timestamps` returns when the hypothesis's clip is decoded alone.  The rows along
the ancestry are the rows of a teacher-forced pass over h[:-1] (a beam's row at position p depends on h[0 .. p] only), so the judge
teacher-forces every hypothesis of `beam_judge.run(case, clip)["nbest"]` through the oracle and runs `wo.token_timestamps` on the result.
tests/test_beam_align_judge.py pins this to HF's own generate + `_extract_token_timestamps` on every fixture clip, decoded alone.
"""
from __future__ import annotations

import functools
from typing import List, Optional, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests import beam_judge as bj
from tests import eos_model as em

HEADS = [tuple(h) for h in em.HEADS]


def rows_of(case: bj.Case, clip: int, hyp, want=HEADS) -> np.ndarray:
    """float32 [Ha, len - 1, T]: the alignment rows 0 .. len - 2 of hypothesis `hyp` (ids, prompt included) of this clip."""
    om, enc = bj._encoded(case.es)
    h = np.asarray(list(hyp), dtype=np.int64)
    cache = om.new_cache(enc[clip : clip + 1])
    _, cross = om.decode(h[None, :-1], cache, want_cross=want)
    return np.asarray(cross, dtype=np.float32)[0]


def hyp_timestamps(case: bj.Case, clip: int, hyp, n_prompt: int = em.N_PROMPT, columns: Optional[int] = None) -> np.ndarray:
    """float32 [len]: zeros for the prompt, the jump times of the generated tokens, the last one twice (HF's layout); all zeros when
    the hypothesis has at most one generated token (N = len - 1 - n0 <= 0)."""
    n = len(hyp)
    if n - 1 - n_prompt <= 0:
        return np.zeros(n, dtype=np.float32)
    cross = rows_of(case, clip, hyp)[None]
    return wo.token_timestamps(cross, n_prompt, None, columns=None if columns is None else [columns])[0]


@functools.lru_cache(maxsize=None)
def run(case: bj.Case, clip: int, prompt: Optional[Tuple[int, ...]] = None) -> dict:
    """The judge's result for every hypothesis of `clip` under `case`: nbest / scores as beam_judge.run, lengths (prompt included; the
    prompt's for a placeholder) and timestamps (one float32 array per hypothesis).  Computed once per process; read-only."""
    ref = bj.run(case, clip, prompt)
    n0 = len(prompt) if prompt is not None else em.N_PROMPT
    ts: List[np.ndarray] = []
    for h, s in zip(ref["nbest"], ref["scores"]):
        t = hyp_timestamps(case, clip, h, n0) if s > -1e8 else np.zeros(len(h), dtype=np.float32)
        t.setflags(write=False)
        ts.append(t)
    return {"nbest": ref["nbest"], "scores": ref["scores"], "lengths": [len(h) for h in ref["nbest"]], "timestamps": ts}


def padded(ts: np.ndarray, L: int) -> np.ndarray:
    """A hypothesis's timestamps in a row of L entries, as tw_token_timestamps_each lays it out: the last jump time repeats."""
    out = np.zeros(L, dtype=np.float32)
    out[: len(ts)] = ts
    out[len(ts):] = ts[-1] if len(ts) else 0.0
    return out
