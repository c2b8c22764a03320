"""Whisper's temperature fallback on the engine: decode at temperature 0, measure the result, decode the rows that fail again at
0.2, 0.4 ... 1.0 (``WhisperGenerationMixin.generate_with_fallback``, HF:models/whisper/generation_whisper.py:970-1116; the checks
``_need_fallback``, :1898-1947, and ``_retrieve_compression_ratio``, :1949-1955).

The measurements: the compression ratio of the token bytes (``zlib``, host), and ``avg_logprob`` / ``no_speech_prob`` of
``shortform.score_entries`` (scores of the PROCESSED logits at T = 1: what HF averages after rescaling by the temperature, :1958-1967).
The draws are ``WhisperEngine.generate_sample``'s: a row's result at a given (seed, offset) does not depend on the rows decoded beside it,
so rows that passed are FROZEN in later attempts (temperature < 0) instead of being cut out of the batch.  ``FallbackPolicy.top_k`` /
``top_p`` narrow the candidate set of every sampled attempt (tw_generate_sample_filtered); they are off by default, as in openai/whisper's
draw, and ``top_k=50`` reproduces HF's candidate set.  Deviation from HF: the random numbers are Philox's, not torch's.
"""
from __future__ import annotations

import dataclasses
import math
import zlib
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .shortform import score_entries


@dataclasses.dataclass(frozen=True)
class FallbackPolicy:
    """HF's ``temperature`` tuple and thresholds (the defaults of the reference's long-form recipe), the base seed of the draws, and the
    candidate set of the sampled attempts (``top_k`` / ``top_p``, None = off; ``top_k=50`` is what HF's ``generate`` resolves to)."""
    temperatures: Tuple[float, ...] = (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)
    compression_ratio_threshold: Optional[float] = 1.35
    logprob_threshold: Optional[float] = -1.0
    no_speech_threshold: Optional[float] = None
    seed: int = 0
    top_k: Optional[int] = None
    top_p: Optional[float] = None

    def __post_init__(self):
        if self.top_k is not None and (isinstance(self.top_k, bool) or int(self.top_k) != self.top_k or self.top_k < 0):
            raise ValueError(f"top_k must be an integer >= 0 (0 or None = off), got {self.top_k!r}")
        if self.top_p is not None and not (0 < float(self.top_p) <= 1):
            raise ValueError(f"top_p must lie in (0, 1] (1 or None = off), got {self.top_p!r}")
        t = tuple(float(x) for x in self.temperatures)
        if not t or any(not math.isfinite(x) or x < 0 for x in t):
            raise ValueError(f"temperatures must be finite and >= 0, got {self.temperatures}")
        object.__setattr__(self, "temperatures", t)


def as_policy(x) -> Optional[FallbackPolicy]:
    """None | FallbackPolicy | a tuple of temperatures."""
    return x if x is None or isinstance(x, FallbackPolicy) else FallbackPolicy(temperatures=tuple(x))


def compression_ratio(tokens, vocab: int) -> float:
    """``_retrieve_compression_ratio``: byte length of the token bytes over the byte length of their zlib compression."""
    length = int(math.log2(vocab) / 8) + 1
    token_bytes = b"".join(int(t).to_bytes(length, "little") for t in np.asarray(tokens).reshape(-1).tolist())
    return len(token_bytes) / len(zlib.compress(token_bytes))


def need_fallback(tokens, vocab: int, avg_logprob: Optional[float], no_speech_prob: Optional[float], policy: FallbackPolicy
                  ) -> Tuple[bool, bool]:
    """``_need_fallback``: (needs_fallback, should_skip).  ``tokens``: the generated ids of the row without padding, the <eos> kept when
    the row ended with one (what HF hands to both checks)."""
    needs, skip = False, False
    if policy.compression_ratio_threshold is not None and compression_ratio(tokens, vocab) > policy.compression_ratio_threshold:
        needs = True
    low = False
    if policy.logprob_threshold is not None:
        if avg_logprob is None:
            raise ValueError("logprob_threshold needs the row's average log-probability")
        low = avg_logprob < policy.logprob_threshold
        needs = needs or low
    if policy.no_speech_threshold is not None and policy.logprob_threshold is not None:
        if no_speech_prob is None:
            raise ValueError("no_speech_threshold needs the row's no-speech probability (no_speech_id)")
        if low and no_speech_prob > policy.no_speech_threshold:      # silence, not a failed decode: skip the segment
            needs, skip = False, True
    return needs, skip


def _row_tokens(entry: Dict[str, Any], eos: int) -> np.ndarray:
    toks = np.asarray(entry["tokens"], dtype=np.int64)
    ended = len(entry["logprob"]) == len(toks) + 1
    return np.append(toks, eos) if ended else toks


def generate_with_fallback(engine, prompt: np.ndarray, greedy: Dict[str, Any], policy: FallbackPolicy, no_speech_id: Optional[int],
                           seeds: Sequence[int], offsets: Sequence[int],
                           first_call: Optional[Callable[[], Dict[str, Any]]] = None,
                           on_attempt: Optional[Callable[[int, float, Dict[str, Any], List[int]], None]] = None) -> List[Dict[str, Any]]:
    """The ladder for the rows of ``prompt`` [B, n_prompt].  Attempt k runs at ``policy.temperatures[k]`` with per-row
    ``(seeds[b], offsets[b] + k)``; attempt 0 is ``first_call()`` when given (the caller's greedy call: it may carry a draft) and
    ``generate_greedy`` / ``generate_sample`` otherwise; ``prompt`` and ``greedy`` are the draft-free prompt and keywords (``n_draft`` /
    ``n_forced`` are dropped from ``greedy``: the library refuses them under sampling).  Every attempt is scored with ``score_entries``; rows that pass (or are
    skipped as silence) are frozen in later attempts and keep the rows of the attempt that accepted them; at the last temperature
    every remaining row is kept as it is.  ``on_attempt(k, temperature, out, rows)``: called after attempt k with the engine's result
    and the rows accepted in it - the moment to take ``token_timestamps``, whose alignment rows belong to the LAST engine call.
    Returns one dict per row: ``sequence`` (the row of the accepting attempt, that attempt's length), ``temperature``, ``attempts``,
    ``should_skip``, ``score`` (the ``score_entries`` entry), ``top_k`` / ``top_p`` (the policy's)."""
    prompt = np.ascontiguousarray(prompt, dtype=np.int32)
    B, n_prompt = prompt.shape
    vocab = int(engine.vocab)
    eos = int(greedy.get("eos_id", 50257))
    greedy = {k: v for k, v in greedy.items() if k not in ("n_draft", "n_forced")}
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(B)
    offsets = np.asarray(offsets, dtype=np.uint64).reshape(B)
    need_ns = policy.no_speech_threshold is not None
    if need_ns and no_speech_id is None:
        raise ValueError("no_speech_threshold needs no_speech_id")
    results: List[Optional[Dict[str, Any]]] = [None] * B
    pending = list(range(B))
    temps = policy.temperatures
    # (handed on only when set: an engine stand-in without the two keywords keeps working with the default policy)
    filters = {n: v for n, v in (("top_k", policy.top_k), ("top_p", policy.top_p)) if v is not None}
    for k, T in enumerate(temps):
        if k == 0 and first_call is not None:
            out = first_call()
        elif T == 0.0 and len(pending) == B:
            out = engine.generate_greedy(prompt, **greedy)
        else:
            t = np.full((B,), -1.0, dtype=np.float32)
            t[pending] = T
            out = engine.generate_sample(prompt, t, seeds, offsets + np.uint64(k), **greedy, **filters)
        seq = np.asarray(out["sequences"])
        # (all B rows, frozen ones included: a row's cross K/V live in the slot of its index, so the call cannot be cut down to the live rows)
        entries = score_entries(engine, seq, n_prompt, greedy, no_speech_id)
        accepted, still = [], []
        for b in pending:
            e = entries[b]
            needs, skip = need_fallback(_row_tokens(e, eos), vocab, e["avg_logprob"], e["no_speech_prob"], policy)
            if needs and k < len(temps) - 1:
                still.append(b)
                continue
            results[b] = {"sequence": seq[b].copy(), "temperature": float(T), "attempts": k + 1, "should_skip": bool(skip), "score": e,
                          "needs_fallback": bool(needs), "top_k": policy.top_k, "top_p": policy.top_p}
            accepted.append(b)
        if on_attempt is not None:
            on_attempt(k, float(T), out, accepted)
        pending = still
        if not pending:
            break
    return results  # type: ignore[return-value]
