"""CPU stand-ins with ``WhisperEngine.detect_language`` (TESTS ONLY): subclasses of the stand-ins of tests/oracle_engine.py and
tests/stub_engine.py whose ``detect_language`` is THE RULE of include/thewhisper.h in numpy (``lang_rule``) over the stand-in's own
``decode_step`` logits.  ``lang_rule`` is also what the GPU tests hold the kernel's results against."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np
import torch

from tests.oracle_engine import OracleEngine
from tests.stub_engine import StubEngine


def lang_rule(logits: np.ndarray, lang_ids: Sequence[int]) -> Dict[str, np.ndarray]:
    """THE RULE on float32 logits [rows, V]: ids int32 [rows], probs float32 [rows, n_lang] (the float32 sum here is numpy's
    order, not the kernel's: compare probabilities with a tolerance, or bit for bit only between two results of the kernel)."""
    ids = np.asarray(list(lang_ids), dtype=np.int64)
    x = np.asarray(logits, dtype=np.float32)[:, ids].copy()
    x[np.isnan(x)] = -np.inf
    m = x.max(axis=1)
    out_id = np.zeros(x.shape[0], dtype=np.int32)
    probs = np.zeros(x.shape, dtype=np.float32)
    for r in range(x.shape[0]):
        out_id[r] = int(ids[x[r] == m[r]].min())
        if m[r] != -np.inf:
            e = np.exp((x[r] - m[r]).astype(np.float32)).astype(np.float32)
            probs[r] = e / e.sum(dtype=np.float32)
    return {"ids": out_id, "probs": probs}


class LangMixin:
    """``detect_language`` for a stand-in that has ``decoder_reset`` / ``decode_step`` (the launches tw_detect_language issues)."""

    def detect_language(self, B: int, sot_id: int, lang_ids: Sequence[int]):
        self.calls["detect"] = self.calls.get("detect", 0) + 1
        self.decoder_reset(int(B))
        lg = self.decode_step([int(sot_id)] * int(B))
        return lang_rule(lg.detach().cpu().numpy(), lang_ids)


class LangOracleEngine(LangMixin, OracleEngine):
    def sibling(self, max_batch=None):
        new = super().sibling(max_batch)
        new.__class__ = type(self)
        return new


def lang_engine_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return LangOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


class LangStubEngine(StubEngine):
    """Computes nothing: every row's language is the first listed id, with probability 1."""

    def detect_language(self, B: int, sot_id: int, lang_ids: Sequence[int]):
        ids = list(lang_ids)
        probs = np.zeros((B, len(ids)), dtype=np.float32)
        probs[:, 0] = 1.0
        return {"ids": np.full(B, ids[0], dtype=np.int32), "probs": probs}
