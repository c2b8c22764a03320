"""Beam search by the rule of include/thewhisper.h (tw_generate_beam), restated in numpy over `oracle.whisper_oracle.OracleWhisper`.  No GPU.

The rule is HF 5.15's `GenerationMixin._beam_search`; tests/test_beam_judge.py pins this restatement to HF's own `generate` on the model of
tests/eos_model.py.  One clip at a time (a clip's result does not depend on its batch-mates); the self-attention cache is reordered by
indexing `DecoderCache.self_k` / `self_v`.  Besides the n-best list a run reports what the GPU tests rely on: the steps whose beam
permutation is not the identity (with the position they consumed) and the smallest gap between neighbours in each of the step's three
selections - a device whose scores differ from these by a summation order picks the same ids only where the gaps are larger than that.

CASES is the fixture table: per case the clips of eos_model's 20 whose smallest gap is >= the case's gap_min, as the judge found them;
tests/test_beam_judge.py recomputes it.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests import eos_model as em

F32 = np.float32
NEG = F32(-1e9)
GAP_MIN = 1e-4        # cases whose scores are length-normalised (a few units: float32 steps of 5e-7)
GAP_MIN_SUM = 4e-4    # length_penalty 0: the score is the plain sum, near -100 where float32 has steps of 7.6e-6 (see Case.gap_min)
MAX_NEW = 24


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    es: float
    timestamps: bool
    K: int
    early: bool
    length_penalty: float
    min_new: int = 0
    suppress: Tuple[int, ...] = ()
    begin_suppress: Tuple[int, ...] = ()
    max_new: int = MAX_NEW

    @property
    def gap_min(self) -> float:
        """The gap a clip needs to be selected: four times the device's score tolerance for this kind of case (tests/test_gpu_beam.py)."""
        return GAP_MIN_SUM if self.length_penalty == 0.0 else GAP_MIN

    def options(self) -> wo.GreedyOptions:
        return wo.GreedyOptions(eos=em.EOS, pad=em.EOS, max_new_tokens=self.max_new, min_new_tokens=self.min_new,
                                begin_suppress=tuple(self.begin_suppress), suppress=tuple(self.suppress), timestamps=self.timestamps,
                                no_timestamps_id=em.NO_TS)

    def engine_kw(self) -> dict:
        """The same options as keyword arguments of WhisperEngine.generate_beam."""
        return dict(num_beams=self.K, length_penalty=self.length_penalty, early_stopping=self.early, max_new_tokens=self.max_new,
                    min_new_tokens=self.min_new, eos_id=em.EOS, pad_id=em.EOS, timestamps=self.timestamps, no_timestamps_id=em.NO_TS,
                    begin_suppress=tuple(self.begin_suppress), suppress=tuple(self.suppress))


def pen(g: int, length_penalty: float) -> np.float32:
    return F32(float(g) ** float(length_penalty))


def _top(values: np.ndarray, n: int) -> Tuple[np.ndarray, float]:
    """Indices of the n largest of `values` (descending, lower index first on ties) and the smallest gap between neighbours among the
    n + 1 largest - counted only between values above -5e8: behind a -1e9 penalty float32 has steps of 64 and equal values are the
    rule's own ties, which both sides resolve by index."""
    order = np.lexsort((np.arange(values.size), -values.astype(np.float64)))
    head = values[order[: n + 1]].astype(np.float64)
    live = head[head > -5e8]
    gap = float(np.min(-np.diff(live))) if live.size > 1 else float("inf")
    return order[:n], gap


def run_clip(om: wo.OracleWhisper, enc1: np.ndarray, prompt: Sequence[int], opt: wo.GreedyOptions, K: int, length_penalty: float,
             early: bool) -> dict:
    """Beam search for ONE clip (enc1: [1, T, d]).  Returns nbest (list of K id lists, prompt included), scores float32 [K], steps (list of
    dicts pos / nonid), gaps (the smallest per selection: cand, run, fin) and finite (the 2K candidates were finite at every step)."""
    prompt = [int(t) for t in prompt]
    n0, V = len(prompt), om.dims.vocab
    max_len = min(opt.max_length, n0 + opt.max_new_tokens, om.dims.max_target_positions)
    cache = om.new_cache(np.repeat(enc1, K, axis=0))
    run_seq = [list(prompt) for _ in range(K)]
    run_score = np.full(K, NEG, dtype=F32)
    run_score[0] = 0
    fin_seq = [list(prompt) for _ in range(K)]
    fin_score = np.full(K, NEG, dtype=F32)
    fin_flag = np.zeros(K, dtype=bool)
    open_, cur = True, n0
    feed = np.asarray(run_seq, dtype=np.int64)
    steps: List[dict] = []
    gaps = {"cand": float("inf"), "run": float("inf"), "fin": float("inf")}
    finite = True
    while True:
        logits, _ = om.decode(feed, cache)
        x = logits[:, -1].astype(F32)
        m = x.max(axis=1, keepdims=True)
        lp = (x - m) - np.log(np.exp(x - m).sum(axis=1, keepdims=True, dtype=F32))
        a = np.stack([wo.apply_logits_processors(lp[k], run_seq[k], n0, opt) + run_score[k] for k in range(K)]).astype(F32)
        top, g = _top(a.reshape(-1), 2 * K)
        gaps["cand"] = min(gaps["cand"], g)
        s = a.reshape(-1)[top]
        finite = finite and bool(np.isfinite(s).all())
        b, t = top // V, top % V
        hit = (t == opt.eos) | (cur + 1 >= max_len)
        r = np.where(hit, s + NEG, s).astype(F32)
        keep, g = _top(r, K)
        gaps["run"] = min(gaps["run"], g)
        f = (s / pen(cur + 1 - n0, length_penalty)).astype(F32)
        if early and fin_flag.all():
            f = f + NEG
        if not open_:
            f = f + NEG
        f = np.where((np.arange(2 * K) < K) & hit, f, f + NEG).astype(F32)
        pool = np.concatenate([fin_score, f]).astype(F32)
        fkeep, g = _top(pool, K)
        gaps["fin"] = min(gaps["fin"], g)
        new_fin_seq, new_flag = [], []
        for i in fkeep:
            if i < K:
                new_fin_seq.append(fin_seq[i]); new_flag.append(bool(fin_flag[i]))
            else:
                j = int(i) - K
                new_fin_seq.append(run_seq[b[j]] + [int(t[j])]); new_flag.append(bool(j < K and hit[j]))
        fin_seq, fin_score, fin_flag = new_fin_seq, pool[fkeep], np.asarray(new_flag)
        beam_idx = b[keep]
        run_seq = [run_seq[b[j]] + [int(t[j])] for j in keep]
        run_score = r[keep]
        for i in range(om.dims.dec_layers):
            cache.self_k[i] = cache.self_k[i][beam_idx]
            cache.self_v[i] = cache.self_v[i][beam_idx]
        steps.append({"pos": cur - 1, "nonid": bool((beam_idx != np.arange(K)).any())})
        cur += 1
        lhs = F32(run_score[0] / pen(cur - n0, length_penalty))
        open_ = open_ and any(lhs > (fin_score.min() if fin_flag[k] else NEG) for k in range(K))
        if (not open_) or (early and fin_flag.all()) or bool(hit.all()):
            break
        feed = np.asarray([[q[-1]] for q in run_seq], dtype=np.int64)
    return {"nbest": fin_seq, "scores": fin_score.astype(F32), "steps": steps, "gaps": gaps, "finite": finite, "max_len": max_len}


def pad_nbest(nbest: Sequence[Sequence[int]], pad: int) -> np.ndarray:
    """int64 [K, L]: the hypotheses padded to the longest."""
    L = max(len(h) for h in nbest)
    return np.asarray([list(h) + [pad] * (L - len(h)) for h in nbest], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _encoded(es: float):
    dims, w = em.model(es)
    om = wo.OracleWhisper(dims, w, T=em.T)
    enc = om.encode(wo.log_mel(em.audio(range(em.N_CLIPS)), dims.n_mels))
    enc.setflags(write=False)
    return om, enc


@functools.lru_cache(maxsize=None)
def run(case: Case, clip: int, prompt: Optional[Tuple[int, ...]] = None) -> dict:
    """The judge's result for clip `clip` of eos_model under `case` (computed once per process; treat as read-only)."""
    om, enc = _encoded(case.es)
    p = prompt if prompt is not None else tuple(int(x) for x in em.prompt([clip])[0])
    return run_clip(om, enc[clip : clip + 1], p, case.options(), case.K, case.length_penalty, case.early)


def min_gap(res: dict) -> float:
    return min(res["gaps"].values())


def nonid_steps(res: dict) -> int:
    return sum(1 for s in res["steps"] if s["nonid"])


def ends_by_eos(res: dict) -> bool:
    """The best hypothesis ends with <eos> before max_len."""
    h = res["nbest"][0]
    return res["scores"][0] > -1e8 and h[-1] == em.EOS and len(h) < res["max_len"]


def never_eos(res: dict) -> bool:
    return all(em.EOS not in h[em.N_PROMPT:] for h, s in zip(res["nbest"], res["scores"]) if s > -1e8)


def select(case: Case, clips=range(em.N_CLIPS)) -> Tuple[int, ...]:
    """The clips whose smallest gap under `case` is >= case.gap_min and whose candidates were always finite."""
    return tuple(c for c in clips if min_gap(run(case, c)) >= case.gap_min and run(case, c)["finite"])


# the settings the issue names (K in {2, 3, 5}, early_stopping, length_penalty in {1, 0, 2}, timestamps on and off) and one case each with
# min_new_tokens, a suppress list and begin-suppress ids
CASE_LIST: List[Case] = [
    Case("k2-ts", 2.5, True, 2, False, 1.0),
    Case("k3-ts-early", 2.5, True, 3, True, 1.0),
    Case("k5-ts", 2.5, True, 5, False, 1.0),
    Case("k3-text-lp0", 2.0, False, 3, False, 0.0),
    Case("k5-text-early-lp0", 2.0, False, 5, True, 0.0),
    Case("k2-ts-es2-lp2", 2.0, True, 2, True, 2.0),
    Case("k3-ts-minnew", 2.5, True, 3, False, 1.0, min_new=8),
    Case("k3-text-suppress", 2.0, False, 3, False, 1.0, suppress=(11, 257, 400, 701, 946)),
    Case("k2-text-bsup", 2.0, False, 2, True, 1.0, begin_suppress=(5, 9, 200)),
]


def case(name: str) -> Case:
    return next(c for c in CASE_LIST if c.name == name)


# case name -> the clips select() keeps (tests/test_beam_judge.py recomputes this)
CASES: Dict[str, Tuple[int, ...]] = {
    'k2-ts': (0, 1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 16, 17, 18, 19),
    'k3-ts-early': (0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19),
    'k5-ts': (0, 1, 2, 5, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18),
    'k3-text-lp0': (0, 1, 2, 3, 5, 6, 7, 8, 10, 11, 12, 15, 16, 17, 18, 19),
    'k5-text-early-lp0': (0, 3, 6, 17, 19),
    'k2-ts-es2-lp2': (0, 1, 2, 7, 12, 14, 15, 16, 17, 18, 19),
    'k3-ts-minnew': (0, 1, 2, 4, 5, 6, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19),
    'k3-text-suppress': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 19),
    'k2-text-bsup': (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19),
}
