"""Host-side reference for the repetition penalty and the no-repeat n-gram rule (tw_generate_greedy_repeat; k_decode.hip: repeat_kernel).
No GPU in here.

The crafted zero-layer models and the judge of tests/sampler_judge.py are reused unchanged, as tests/bias_judge.py reuses them: the
replayed `decode_step` logits of a finished sequence are the RAW logits x the loop saw.  `repeat_logits` turns them into x', per step
and row, from that row's history and that row's setting, by calling HF's own `RepetitionPenaltyLogitsProcessor` and
`NoRepeatNGramLogitsProcessor` - behind `bias_judge`'s HF sequence bias where the row has a list - and `sampler_judge.judge` is handed
x'.  The reference for the rule is therefore HF's classes.  `apply_rule` is an independent numpy statement of the rule in
include/thewhisper.h; `repeat_greedy` runs it on the numpy oracle, and tests/test_repeat_judge.py has that run judged through HF.

`events_seen` recomputes, from a final run alone, which kinds of events were decisive in it.
"""
from __future__ import annotations

import dataclasses
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor

from oracle import whisper_oracle as wo
from tests import bias_judge as bj
from tests import sampler_judge as sj

MAX_NEW = 40              # generated tokens of a run
EVENTS = ("pen_pos", "pen_neg", "pen_prompt", "pen_ignore", "ban1", "ban2", "ban3", "ts_flip", "ban_suppressed")


@dataclasses.dataclass(frozen=True)
class Row:
    """One row's setting: the penalty (1.0 = off) and the n-gram size (0 = off)."""
    penalty: float = 1.0
    ngram: int = 0

    @property
    def on(self) -> bool:
        return np.float32(self.penalty) != np.float32(1.0) or self.ngram != 0


OFF = Row()


# --------------------------------------------------------------------------------------------------------------------
# the rule: HF's processors (the reference), and a numpy statement of include/thewhisper.h
# --------------------------------------------------------------------------------------------------------------------
class HFRepeat:
    """x -> x' for one row's setting by HF's two processors, in HF's order (penalty, then n-gram)."""

    def __init__(self, row: Row, ignore: int = 0, penalty: bool = True, ngram: bool = True):
        self.procs = []
        if penalty and np.float32(row.penalty) != np.float32(1.0):
            self.procs.append(RepetitionPenaltyLogitsProcessor(float(row.penalty), prompt_ignore_length=int(ignore) or None))
        if ngram and row.ngram:
            self.procs.append(NoRepeatNGramLogitsProcessor(int(row.ngram)))

    def __call__(self, x: np.ndarray, hist: Sequence[int]) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32)
        if not self.procs:
            return x.copy()
        ids = torch.tensor([[int(t) for t in hist]], dtype=torch.long)
        s = torch.from_numpy(x.copy())[None]
        for p in self.procs:
            s = p(ids, s)
        return s[0].numpy()


def apply_rule(x: np.ndarray, hist: Sequence[int], row: Row, ignore: int = 0) -> np.ndarray:
    """The rule of include/thewhisper.h in numpy: every distinct id of hist[ignore:] penalised once from its original value by one float32
    multiply or division; every id that would complete a repeated N-gram set to -inf."""
    out = np.asarray(x, dtype=np.float32).copy()
    h = [int(t) for t in hist]
    n = len(h)
    r = np.float32(row.penalty)
    if r != np.float32(1.0):
        for v in sorted(set(h[ignore:])):
            with np.errstate(all="ignore"):
                out[v] = np.float32(x[v] * r) if x[v] < 0 else np.float32(np.float32(x[v]) / r)
    N = int(row.ngram)
    if N > 0 and n >= N:
        suffix = h[n - N + 1:]
        for i in range(n - N + 1):
            if h[i:i + N - 1] == suffix:
                out[h[i + N - 1]] = -np.inf
    return out


def repeat_logits(logits: np.ndarray, sequences: np.ndarray, n_begin: int, rows: Sequence[Row], ignore: int = 0, bias_rows=None) -> np.ndarray:
    """x' [L-1, B, V] of the raw logits [L-1, B, V] of `sequences` [B, L], by HF's processors; steps inside the prompt are left alone."""
    out = np.array(logits, dtype=np.float32, copy=True)
    B, L = sequences.shape
    for b in range(B):
        hb = bj.HFBias(bias_rows[b] if bias_rows is not None else None)
        hr_ = HFRepeat(rows[b], ignore)
        if hb.proc is None and not hr_.procs:
            continue
        for s in range(n_begin - 1, L - 1):
            out[s, b] = hr_(hb(logits[s, b], sequences[b, :s + 1]), sequences[b, :s + 1])
    return out


def judge_repeat(lg: np.ndarray, seqs: np.ndarray, n_begin: int, opt: wo.GreedyOptions, rows: Sequence[Row], ignore: int = 0, bias_rows=None
                 ) -> sj.Verdict:
    """sampler_judge.judge on x' = HF's processors applied to the raw logits, per step and row."""
    return sj.judge(repeat_logits(lg, seqs, n_begin, rows, ignore, bias_rows), seqs, n_begin, opt)


def repeat_greedy(model: wo.OracleWhisper, enc: np.ndarray, prompt: np.ndarray, opt: wo.GreedyOptions, rows: Sequence[Row], ignore: int = 0,
                  bias_rows=None, begin_index: Optional[int] = None):
    """wo.greedy_generate with `bias_judge.add_bias` and `apply_rule` in front of the logits processors of every row."""
    prompt = np.asarray(prompt, dtype=np.int64)
    b, n0 = prompt.shape
    cache = model.new_cache(enc)
    seqs = [list(map(int, prompt[i])) for i in range(b)]
    unfinished = np.ones(b, dtype=bool)
    nb = n0 if begin_index is None else int(begin_index)
    max_len = min(opt.max_length, nb + opt.max_new_tokens)
    cross_rows: List[np.ndarray] = []
    feed = prompt
    while True:
        logits, cross = model.decode(feed, cache, want_cross=opt.alignment_heads)
        if cross is not None:
            cross_rows.append(cross)
        last = logits[:, -1].astype(np.float32)
        nxt = np.zeros(b, dtype=np.int64)
        for i in range(b):
            x = bj.add_bias(last[i], seqs[i], bias_rows[i] if bias_rows is not None else None)
            sc = wo.apply_logits_processors(apply_rule(x, seqs[i], rows[i], ignore), seqs[i], nb, opt)
            tok = int(np.argmax(sc)) if unfinished[i] else opt.pad
            nxt[i] = tok
            seqs[i].append(tok)
        unfinished &= nxt != opt.eos
        if len(seqs[0]) >= max_len or not unfinished.any():
            break
        feed = nxt[:, None]
    return {"sequences": np.asarray(seqs, dtype=np.int64), "cross": np.concatenate(cross_rows, axis=2) if cross_rows else None}


def oracle_repeat_run(dims, weights, prompt: np.ndarray, opt: wo.GreedyOptions, rows, ignore: int = 0, bias_rows=None):
    """sampler_judge.oracle_run with a setting per row: (sequences [B, L], RAW logits [L-1, B, V])."""
    om = sj._OracleExactTies(dims, weights, T=sj.T_FRAMES)
    prompt = np.asarray(prompt)
    enc = np.zeros((prompt.shape[0], sj.T_FRAMES, dims.d_model), np.float32)
    seqs = repeat_greedy(om, enc, prompt, opt, rows, ignore, bias_rows)["sequences"]
    cache = om.new_cache(enc)
    lg = [om.decode(seqs[:, s:s + 1], cache)[0][:, 0].astype(np.float32) for s in range(seqs.shape[1] - 1)]
    return seqs, np.stack(lg)


def settings_of(repetition_penalty, no_repeat_ngram_size, B: int) -> List[Row]:
    """WhisperEngine.generate_greedy's two keywords (None, a scalar or one value per row) as a Row per row."""
    pen = np.broadcast_to(np.asarray(1.0 if repetition_penalty is None else repetition_penalty, dtype=np.float64).reshape(-1), (B,))
    ngr = np.broadcast_to(np.asarray(0 if no_repeat_ngram_size is None else no_repeat_ngram_size).reshape(-1), (B,))
    return [Row(float(p), int(n)) for p, n in zip(pen, ngr)]


class RepeatOracleEngine(bj.BiasedOracleEngine):
    """tests/bias_judge.BiasedOracleEngine whose generate_greedy also takes WhisperEngine's three repeat keywords."""

    def generate_greedy(self, prompt, repetition_penalty=None, no_repeat_ngram_size=None, penalty_ignore=0, **kw):
        prompt = np.asarray(prompt)
        B = prompt.shape[0]
        rows = settings_of(repetition_penalty, no_repeat_ngram_size, B)
        if not any(r.on for r in rows):
            return super().generate_greedy(prompt, **kw)
        from thewhisper_amd.engine import sequence_bias_dict

        self.calls["generate"] += 1
        sb, sbr = kw.get("sequence_bias"), kw.get("sequence_bias_rows")
        if sb is not None:
            sbr = [sb] * B
        bias_rows = [sequence_bias_dict(r) for r in sbr] if sbr is not None else None
        n_forced, n_draft = int(kw.get("n_forced", 0)), int(kw.get("n_draft", 0))
        opt = wo.GreedyOptions(eos=kw.get("eos_id", 50257), pad=kw.get("pad_id", 50257), max_new_tokens=kw.get("max_new_tokens", 128),
                               min_new_tokens=kw.get("min_new_tokens", 0), max_length=kw.get("max_length", 448),
                               begin_suppress=tuple(kw.get("begin_suppress", (220, 50257))), suppress=tuple(kw.get("suppress", ())),
                               timestamps=kw.get("timestamps", False), no_timestamps_id=kw.get("no_timestamps_id", 50364),
                               max_initial_timestamp_index=kw.get("max_initial_timestamp_index", 50),
                               alignment_heads=self.alignment_heads if kw.get("want_alignment", False) else None)
        draft = None
        if n_draft:
            draft, prompt = prompt[:, prompt.shape[1] - n_draft:], prompt[:, : prompt.shape[1] - n_draft]
        res = repeat_greedy(self.model, self._enc[:B], prompt, opt, rows, int(penalty_ignore), bias_rows,
                            begin_index=(prompt.shape[1] - n_forced) if n_forced else None)
        self._cross = res["cross"]
        out = {"sequences": res["sequences"], "length": int(res["sequences"].shape[1])}
        if draft is not None:
            gen = res["sequences"][:, prompt.shape[1]:]
            n = min(gen.shape[1], draft.shape[1])
            first = [int(np.argmax(np.append(gen[b, :n] != draft[b, :n], True))) for b in range(B)]
            out["draft"] = {"offered": n_draft * B, "accepted": min(first) * B, "launches": 0, "rounds": 0}
        return out


def repeat_oracle_engine_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return RepeatOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


# --------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class RepeatCase:
    name: str                      # a case of sampler_judge.CASES
    B: int
    dtype: str
    graph: bool
    seed: int = 0

    @property
    def id(self) -> str:
        return f"{self.name}-{self.dtype}-B{self.B}" + ("-graph" if self.graph else "")


IGNORE = 2                # penalty_ignore of the picks cases: the first two prompt tokens are not penalised
TS_BIAS = -64.0           # row 0 of a picks case carries this length-1 bias on every timestamp id: its first token is picked among negative logits
# per-row settings of the picks cases, cycled over the rows, one of which is off: N = 1, 2, 3 and penalties, alone and combined
ROW_CYCLE = (Row(2.0, 0), Row(1.0, 2), Row(1.1, 3), Row(1.0, 1), Row(1.3, 0), Row(1.3, 2), Row(0.7, 3), Row(1.1, 1))
REPEAT_CASES = [
    RepeatCase("v66", 5, "f32", False),
    RepeatCase("v66", 5, "f32", True),
    RepeatCase("v66", 5, "bf16", True),
    RepeatCase("v66", 5, "f16", False),
    RepeatCase("v127-b6", 17, "f32", True),
]
N_PROMPT = 6
_OFF_PROMPT = (3, 5, 9, 10, 12, 30)
# Prompts of the set rows, in row order (the off row takes _OFF_PROMPT), found by a search over crafted prompts on the numpy oracle: a
# zero-layer model's logits depend on the last token and the position only, so a prompt that holds the first step's winner - alone,
# in front of penalty_ignore, behind the last token, behind the last two - makes that step an event, and the repeats the models fall
# into supply the rest.  tests/test_repeat_judge.py checks that the oracle's run of every case shows every event within the cap.
_SET_PROMPTS = {
    ("v66", 5): [(3, 19, 21, 22, 53, 22), (3, 1, 14, 60, 1, 14), (3, 16, 59, 17, 34, 8), (3, 2, 5, 60, 21, 28)],
    ("v127-b6", 17): [(3, 68, 101, 25, 22, 26), (3, 1, 14, 124, 1, 14), (3, 4, 75, 102, 4, 75), (3, 6, 34, 37, 102, 37), (3, 6, 124, 9, 35, 27),
                      (3, 18, 4, 102, 73, 4), (3, 8, 12, 124, 8, 12), (3, 5, 78, 83, 124, 83), (3, 8, 22, 102, 8, 22), (3, 8, 38, 45, 124, 45),
                      (3, 9, 10, 101, 9, 10), (3, 9, 51, 74, 124, 74), (3, 9, 51, 102, 9, 51), (3, 9, 61, 102, 9, 61), (3, 12, 1, 79, 102, 79),
                      (3, 12, 8, 80, 102, 80)],
}


def rows_of(B: int) -> List[Row]:
    """The settings of a picks case: rows differ, the last row is off; at B = 17 row 16 - the second group of 16 - is set and row 15 off."""
    if B == 1:
        return [ROW_CYCLE[0]]
    rows = [ROW_CYCLE[b % len(ROW_CYCLE)] for b in range(B)]
    rows[B - 1 if B <= 16 else 15] = OFF
    return rows


def bias_rows_of(built: sj.Built, B: int):
    """The sequence-bias lists of a picks case: row 0 has TS_BIAS on every timestamp id (every logit it may pick first is negative)."""
    c = built.case
    return [{(v,): TS_BIAS for v in range(c.no_ts + 1, c.V)}] + [None] * (B - 1)


def build(rc: RepeatCase) -> sj.Built:
    """The sampler case with the repeat run's budget (kw and opt alike) and with the first prompt token - common to every row - ALSO on the
    suppress list: under N = 1 that id is banned and suppressed at once."""
    built = sj.build_case(dataclasses.replace(sj.case_by_name(rc.name), B=rc.B, dtype=rc.dtype, graph=rc.graph, seed=rc.seed))
    sup = tuple(built.kw["suppress"]) + (int(built.prompt[0, 0]),)
    if (rc.name, rc.B) in _SET_PROMPTS:
        it = iter(_SET_PROMPTS[(rc.name, rc.B)])
        built.prompt = np.array([next(it) if r.on else _OFF_PROMPT for r in rows_of(rc.B)], dtype=np.int32)
    built.kw["max_new_tokens"] = MAX_NEW
    built.kw["suppress"] = sup
    built.opt = dataclasses.replace(built.opt, max_new_tokens=MAX_NEW, suppress=sup)
    return built


def events_seen(rows: Sequence[Row], ignore: int, seqs: np.ndarray, lg: np.ndarray, n_begin: int, opt: wo.GreedyOptions, bias_rows=None) -> set:
    """Kinds of EVENTS that were decisive in the run (seqs, raw logits lg), recomputed from the run alone through HF's processors.
    At a step of a row, with x the logits behind the row's bias, full = both processors, no_pen = the n-gram one alone, no_ban = the
    penalty alone, w = the pick without the processor in question, tok = the run's token = the pick from full:
      pen_pos / pen_neg   w = pick(no_pen) != tok, w is penalised and x[w] > 0 / x[w] < 0;
      pen_prompt          as above, and w occurs in the history in the prompt only;
      pen_ignore          the pick with penalty_ignore = 0 differs from tok (ignore > 0 spares an id that would have been dethroned);
      ban1 / ban2 / ban3  w = pick(no_ban) != tok, the row's N is 1 / 2 / 3 and w is banned;
      ts_flip             one of the above where the sign of the timestamp-mass margin differs between full and without, and so does
                          the class of the pick;
      ban_suppressed      a banned id is on the suppress list, and tok is the pick without the ban as well."""
    seen = set()
    V = lg.shape[2]
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    B, L = seqs.shape
    for b in range(B):
        row = rows[b]
        if not row.on:
            continue
        hb = bj.HFBias(bias_rows[b] if bias_rows is not None else None)
        full_p, no_pen_p, no_ban_p = HFRepeat(row, ignore), HFRepeat(row, ignore, penalty=False), HFRepeat(row, ignore, ngram=False)
        all_p = HFRepeat(row, 0)
        for s in range(n_begin - 1, L - 1):
            hist = [int(t) for t in seqs[b, :s + 1]]
            if opt.eos in hist[n_begin:]:
                break
            tok = int(seqs[b, s + 1])
            x = hb(lg[s, b], hist)
            full = full_p(x, hist)
            if bj.pick(full, hist, n_begin, opt) != tok:
                continue
            pre = bj.mask_of(V, hist, n_begin, opt)

            def flips(minus):
                if not opt.timestamps:
                    return False
                a, c = sj._mass_margin(minus, pre, tb), sj._mass_margin(full, pre, tb)
                return np.isfinite(a) and np.isfinite(c) and (a > 0) != (c > 0) and (bj.pick(minus, hist, n_begin, opt) >= tb) != (tok >= tb)

            if full_p.procs and np.float32(row.penalty) != np.float32(1.0):
                minus = no_pen_p(x, hist)
                w = bj.pick(minus, hist, n_begin, opt)
                if w != tok and w in hist[ignore:] and row.penalty > 1.0:
                    if x[w] > 0:
                        seen.add("pen_pos")
                    if x[w] < 0:
                        seen.add("pen_neg")
                    if w in hist[ignore:n_begin] and w not in hist[n_begin:]:
                        seen.add("pen_prompt")
                if w != tok and flips(minus):
                    seen.add("ts_flip")
                if ignore > 0 and bj.pick(all_p(x, hist), hist, n_begin, opt) != tok:
                    seen.add("pen_ignore")
            if row.ngram:
                minus = no_ban_p(x, hist)
                banned = np.isneginf(full) & ~np.isneginf(minus)
                w = bj.pick(minus, hist, n_begin, opt)
                if w != tok and banned[w] and row.ngram in (1, 2, 3):
                    seen.add(f"ban{row.ngram}")
                if w != tok and flips(minus):
                    seen.add("ts_flip")
                if w == tok and any(banned[int(t)] for t in opt.suppress if 0 <= int(t) < V):
                    seen.add("ban_suppressed")
    return seen
