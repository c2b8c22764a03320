"""Host-side reference for the per-stream sequence bias (tw_generate_greedy_biased; k_decode.hip: seq_bias_kernel).  No GPU in here.

The crafted zero-layer models and the judge of tests/sampler_judge.py are reused unchanged: with no decoder layer the replayed
`decode_step` logits of a finished sequence are the RAW logits x the loop saw.  `biased_logits` turns them into x', per step and row,
from that row's history, by calling HF's own `SequenceBiasLogitsProcessor` with that row's list; `sampler_judge.judge` is then handed
x'.  The reference for the rule is therefore HF's class.  `add_bias` below is an independent numpy statement of the rule in
include/thewhisper.h; `biased_greedy` runs it on the numpy oracle, and tests/test_bias_judge.py has that run judged through HF.

`build_lists` grows a bias list per row from runs of the case itself (`run(rows) -> (sequences, raw logits)`: the oracle on the CPU, the
engine and its replay on the GPU), one event at a time, every margin at least MARGIN over the gap it has to close; `events_seen`
recomputes, from the final run alone, which events were decisive.
"""
from __future__ import annotations

import dataclasses
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from transformers.generation.logits_process import SequenceBiasLogitsProcessor

from oracle import whisper_oracle as wo
from tests import sampler_judge as sj
from tests.oracle_engine import OracleEngine

BiasDict = Dict[Tuple[int, ...], float]
MARGIN = 1.5              # a bias closes its gap by at least this much (>= 1.0: GEMM rounding cannot undo it)
MAX_NEW = 24              # generated tokens of a bias run: every event happens within the first few
EVENTS = ("pos1", "neg1", "len3", "two_onto_one", "ts_flip", "suppressed", "prompt_len")


# --------------------------------------------------------------------------------------------------------------------
# the rule: HF's processor (the reference), and a numpy statement of include/thewhisper.h
# --------------------------------------------------------------------------------------------------------------------
class HFBias:
    """x -> x' for one row's list by HF's SequenceBiasLogitsProcessor (one processor per list: it caches its length-1 table)."""

    def __init__(self, bias: Optional[BiasDict]):
        self.proc = SequenceBiasLogitsProcessor({tuple(int(t) for t in k): float(v) for k, v in bias.items()}) if bias else None

    def __call__(self, x: np.ndarray, hist: Sequence[int]) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32)
        if self.proc is None:
            return x.copy()
        ids = torch.tensor([list(int(t) for t in hist)], dtype=torch.long)
        return self.proc(ids, torch.from_numpy(x.copy())[None])[0].numpy()


def add_bias(x: np.ndarray, hist: Sequence[int], bias: Optional[BiasDict]) -> np.ndarray:
    """The rule of include/thewhisper.h in numpy: per last token a float32 total from 0.0f, the length-1 sequence first, then the active
    longer ones in list order; one float32 add; every other logit keeps its bits."""
    out = np.asarray(x, dtype=np.float32).copy()
    if not bias:
        return out
    n = len(hist)
    total: Dict[int, np.float32] = {}
    for k, b in bias.items():
        if len(k) == 1:
            total[k[0]] = np.float32(0.0) + np.float32(b)
    for k, b in bias.items():
        L = len(k)
        if L == 1 or L > n or tuple(hist[n - (L - 1):]) != tuple(k[:-1]):
            continue
        total[k[-1]] = np.float32(total.get(k[-1], np.float32(0.0)) + np.float32(b))
    for v, t in total.items():
        out[v] = np.float32(out[v] + t)
    return out


def biased_logits(logits: np.ndarray, sequences: np.ndarray, n_begin: int, rows: Sequence[Optional[BiasDict]]) -> np.ndarray:
    """x' [L-1, B, V] of the raw logits [L-1, B, V] of `sequences` [B, L], by HF's processor; steps inside the prompt are left alone."""
    out = np.array(logits, dtype=np.float32, copy=True)
    B, L = sequences.shape
    for b in range(B):
        hf = HFBias(rows[b])
        if hf.proc is None:
            continue
        for s in range(n_begin - 1, L - 1):
            out[s, b] = hf(logits[s, b], sequences[b, :s + 1])
    return out


def biased_greedy(model: wo.OracleWhisper, enc: np.ndarray, prompt: np.ndarray, opt: wo.GreedyOptions, rows: Sequence[Optional[BiasDict]],
                  begin_index: Optional[int] = None):
    """wo.greedy_generate with `add_bias` in front of the logits processors of every row: dict(sequences, cross)."""
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
            sc = wo.apply_logits_processors(add_bias(last[i], seqs[i], rows[i]), seqs[i], nb, opt)
            tok = int(np.argmax(sc)) if unfinished[i] else opt.pad
            nxt[i] = tok
            seqs[i].append(tok)
        unfinished &= nxt != opt.eos
        if len(seqs[0]) >= max_len or not unfinished.any():
            break
        feed = nxt[:, None]
    return {"sequences": np.asarray(seqs, dtype=np.int64), "cross": np.concatenate(cross_rows, axis=2) if cross_rows else None}


def oracle_biased_run(dims, weights, prompt: np.ndarray, opt: wo.GreedyOptions, rows, begin_index: Optional[int] = None):
    """sampler_judge.oracle_run with a bias list per row: (sequences [B, L], RAW logits [L-1, B, V])."""
    om = sj._OracleExactTies(dims, weights, T=sj.T_FRAMES)
    prompt = np.asarray(prompt)
    enc = np.zeros((prompt.shape[0], sj.T_FRAMES, dims.d_model), np.float32)
    seqs = biased_greedy(om, enc, prompt, opt, rows, begin_index=begin_index)["sequences"]
    cache = om.new_cache(enc)
    lg = [om.decode(seqs[:, s:s + 1], cache)[0][:, 0].astype(np.float32) for s in range(seqs.shape[1] - 1)]
    return seqs, np.stack(lg)


class BiasedOracleEngine(OracleEngine):
    """tests/oracle_engine.OracleEngine whose generate_greedy takes WhisperEngine's two sequence-bias keywords."""

    def generate_greedy(self, prompt, max_new_tokens=128, min_new_tokens=0, max_length=448, eos_id=50257, pad_id=50257,
                        timestamps=False, no_timestamps_id=50364, max_initial_timestamp_index=50, begin_suppress=(220, 50257),
                        suppress=(), want_alignment=False, n_forced=0, n_draft=0, sequence_bias=None, sequence_bias_rows=None):
        from thewhisper_amd.engine import sequence_bias_dict

        kw = dict(max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, max_length=max_length, eos_id=eos_id, pad_id=pad_id,
                  timestamps=timestamps, no_timestamps_id=no_timestamps_id, max_initial_timestamp_index=max_initial_timestamp_index,
                  begin_suppress=begin_suppress, suppress=suppress, want_alignment=want_alignment, n_forced=n_forced, n_draft=n_draft)
        if sequence_bias is not None and sequence_bias_rows is not None:
            raise ValueError("sequence_bias and sequence_bias_rows: give one of the two")
        prompt = np.asarray(prompt)
        B = prompt.shape[0]
        if sequence_bias is not None:
            sequence_bias_rows = [sequence_bias] * B
        rows = [sequence_bias_dict(r) for r in sequence_bias_rows] if sequence_bias_rows is not None else None
        if not rows or not any(rows):
            return super().generate_greedy(prompt, **kw)
        self.calls["generate"] += 1
        opt = wo.GreedyOptions(eos=eos_id, pad=pad_id, max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens,
                               max_length=max_length, begin_suppress=tuple(begin_suppress), suppress=tuple(suppress),
                               timestamps=timestamps, no_timestamps_id=no_timestamps_id,
                               max_initial_timestamp_index=max_initial_timestamp_index,
                               alignment_heads=self.alignment_heads if want_alignment else None)
        draft = None
        if n_draft:
            draft, prompt = prompt[:, prompt.shape[1] - int(n_draft):], prompt[:, : prompt.shape[1] - int(n_draft)]
        res = biased_greedy(self.model, self._enc[:B], prompt, opt, rows, begin_index=(prompt.shape[1] - int(n_forced)) if n_forced else None)
        self._cross = res["cross"]
        out = {"sequences": res["sequences"], "length": int(res["sequences"].shape[1])}
        if draft is not None:
            gen = res["sequences"][:, prompt.shape[1]:]
            n = min(gen.shape[1], draft.shape[1])
            first = [int(np.argmax(np.append(gen[b, :n] != draft[b, :n], True))) for b in range(B)]
            out["draft"] = {"offered": int(n_draft) * B, "accepted": min(first) * B, "launches": 0, "rounds": 0}
        return out


def biased_oracle_engine_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return BiasedOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


# --------------------------------------------------------------------------------------------------------------------
# cases and their lists
# --------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class BiasCase:
    name: str                      # a case of sampler_judge.CASES
    B: int
    dtype: str
    graph: bool
    expect: Tuple[str, ...]        # events that must be decisive in some row of the run

    @property
    def id(self) -> str:
        return f"{self.name}-{self.dtype}-B{self.B}" + ("-graph" if self.graph else "")


_NO_TS = tuple(e for e in EVENTS if e != "ts_flip")
BIAS_CASES = [
    BiasCase("v1000-ts-odd", 6, "f32", False, EVENTS),
    BiasCase("v1000-ts-odd", 6, "f32", True, EVENTS),
    BiasCase("real-f16", 3, "f16", False, EVENTS),
    BiasCase("v127-no-timestamps", 1, "f32", False, _NO_TS),
]


def build(bc: BiasCase) -> sj.Built:
    """The sampler case with the bias run's shorter budget (kw and opt alike); model, prompt and processors unchanged."""
    built = sj.build_case(dataclasses.replace(sj.case_by_name(bc.name), B=bc.B, dtype=bc.dtype, graph=bc.graph))
    built.kw["max_new_tokens"] = MAX_NEW
    built.opt = dataclasses.replace(built.opt, max_new_tokens=MAX_NEW)
    return built


def listed_rows(B: int) -> List[int]:
    """Rows that carry a list: all but the last, which has none (B = 1: the one row there is)."""
    return list(range(B - 1)) if B > 1 else [0]


def mask_of(V: int, hist: Sequence[int], n_begin: int, opt: wo.GreedyOptions) -> np.ndarray:
    """What the processors mask ahead of the mass rule, read off apply_logits_processors (as sampler_judge.judge does)."""
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    probe = np.zeros(V, np.float32)
    probe[tb:] = -1e30
    pre = np.isneginf(wo.apply_logits_processors(probe, list(hist), n_begin, opt))
    probe = np.zeros(V, np.float32)
    probe[:tb] = -1e30
    pre[tb:] = np.isneginf(wo.apply_logits_processors(probe, list(hist), n_begin, opt))[tb:]
    return pre


def pick(x: np.ndarray, hist: Sequence[int], n_begin: int, opt: wo.GreedyOptions) -> int:
    return int(np.argmax(wo.apply_logits_processors(np.asarray(x, np.float32), list(hist), n_begin, opt)))


def _f32(v: float) -> float:
    return float(np.float32(np.ceil(v * 4.0) / 4.0))      # a multiple of 0.25: exact in float32


def _need(x: np.ndarray, pre: np.ndarray, target: int) -> float:
    """How far x[target] lies below the largest unmasked other logit (so that target + gap ties it; negative: it leads)."""
    other = np.where(pre, -np.inf, x.astype(np.float64))
    other[target] = -np.inf
    return float(other.max() - float(x[target]))


@dataclasses.dataclass
class Event:
    kind: str
    row: int
    step: int                              # the judged step s: position s consumed, token s + 1 produced
    keys: Tuple[Tuple[int, ...], ...]      # the sequences the event added
    target: int


def _propose(kind: str, x: np.ndarray, hist: List[int], pre: np.ndarray, n_begin: int, opt: wo.GreedyOptions, have: BiasDict
             ) -> Optional[Tuple[BiasDict, int]]:
    """Sequences for `kind` at a step whose current biased logits are `x` (the list so far applied), or None if the step does not
    lend itself to it.  Every new bias closes its gap by MARGIN."""
    V = x.shape[0]
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    w = pick(x, hist, n_begin, opt)
    free = np.flatnonzero(~pre)
    n = len(hist)
    ctx = tuple(hist[-2:])

    def unused(keys):       # (token ids of at least 1: HF's list form of `sequence_bias` refuses 0)
        return all(k not in have and min(k) >= 1 for k in keys)

    if kind == "suppressed":
        masked = np.flatnonzero(pre & (np.arange(V) != w))
        if masked.size == 0 or not np.isfinite(x[masked[0]]):
            return None
        listed = [int(t) for t in opt.suppress if 0 <= int(t) < V and pre[int(t)] and int(t) != w and np.isfinite(x[int(t)])]
        u = listed[0] if listed else int(masked[0])      # an id of the suppress list where the case has one
        key = ctx + (u,)
        return ({key: _f32(float(x.max()) - float(x[u]) + MARGIN)}, u) if unused([key]) else None
    if pre[w] or free.size < 3:
        return None
    if kind == "ts_flip":
        ts_free = free[free >= tb]
        if not opt.timestamps or w >= tb or ts_free.size == 0:
            return None
        t = int(ts_free[np.argmax(x[ts_free])])
        key = ctx + (t,)
        return ({key: _f32(_need(x, pre, t) + MARGIN)}, t) if unused([key]) else None
    # a text-class target where the winner is text (the boosted logit must also beat the timestamp mass), else one of the winner's class
    cls = free[free < tb] if w < tb else free[free >= tb]
    cls = cls[cls != w]
    if cls.size < 2:
        return None
    order = cls[np.argsort(-x[cls], kind="stable")]
    lse_ts = -np.inf
    if opt.timestamps and w < tb and (free >= tb).any():
        z = x[free[free >= tb]].astype(np.float64)
        lse_ts = float(z.max() + np.log(np.exp(z - z.max()).sum()))

    def gap(t):      # what t needs to tie the strongest opponent: another id, or - for a text id - the timestamp mass
        return max(_need(x, pre, t), lse_ts - float(x[t]))

    if kind == "pos1":
        t = int(order[0])
        return ({(t,): _f32(gap(t) + MARGIN)}, t) if unused([(t,)]) else None
    if kind == "neg1":
        second = float(np.where(pre, -np.inf, x)[np.arange(V) != w].max())
        return ({(w,): -_f32(float(x[w]) - second + MARGIN)}, w) if unused([(w,)]) and np.isfinite(second) else None
    if kind == "len3":
        t = int(order[1])
        key = ctx + (t,)
        return ({key: _f32(gap(t) + MARGIN)}, t) if unused([key]) and n >= 2 else None
    if kind == "two_onto_one":
        far = [int(t) for t in order if gap(int(t)) >= 2 * MARGIN + 1.0]
        if not far or n < 3:
            return None
        t = far[0]
        g = gap(t)
        half = _f32((g + MARGIN) / 2.0)            # each alone falls short by g - half >= MARGIN / 2 + ... (checked by events_seen)
        ka, kb = (hist[-1], t), tuple(hist[-3:]) + (t,)
        return ({ka: half, kb: half}, t) if unused([ka, kb]) and g - half >= 1.0 else None
    raise AssertionError(kind)


Runner = Callable[[List[Optional[BiasDict]]], Tuple[np.ndarray, np.ndarray]]


def build_lists(run: Runner, built: sj.Built, n_begin: int, kinds: Sequence[str], max_rounds: int = 48):
    """Grows one list per listed row, event by event, from runs of the case itself.  An event proposed at step s of the current run is
    kept iff the next run is unchanged up to position s and differs at s + 1 as the event demands; otherwise the next step is tried.
    Returns (rows [B], events, final sequences, final raw logits)."""
    opt = built.opt
    B = built.prompt.shape[0]
    rows: List[Optional[BiasDict]] = [None] * B
    todo = {b: [k for k in kinds if k != "prompt_len"] for b in listed_rows(B)}
    for i, b in enumerate(todo):         # lists differ per row: the conditional events in a rotated order, then the two length-1 ones
        cond = [k for k in todo[b] if k not in ("pos1", "neg1")]      # (a length-1 bias acts at every step: last, so that the steps
        r = i % max(1, len(cond))                                     #  the other events were built on are already behind it)
        todo[b] = cond[r:] + cond[:r] + [k for k in ("neg1", "pos1") if k in todo[b]]
    at = {b: n_begin - 1 for b in todo}
    events: List[Event] = []
    seqs, lg = run(rows)
    for _ in range(max_rounds):
        trial = [dict(r) if r else None for r in rows]
        pending: Dict[int, Tuple[str, BiasDict, int, int]] = {}
        for b, left in todo.items():
            while left and at[b] < seqs.shape[1] - 2 and b not in pending:
                s = at[b]
                hist = [int(t) for t in seqs[b, :s + 1]]
                if opt.eos in hist[n_begin:]:
                    left.clear()
                    break
                x = HFBias(rows[b])(lg[s, b], hist)
                got = _propose(left[0], x, hist, mask_of(x.shape[0], hist, n_begin, opt), n_begin, opt, rows[b] or {})
                if got is None:
                    at[b] += 1
                    continue
                trial[b] = {**(rows[b] or {}), **got[0]}
                pending[b] = (left[0], got[0], got[1], s)
        if not pending:
            break
        seqs2, lg2 = run(trial)
        keep = False
        for b, (kind, add, target, s) in pending.items():
            same = seqs2.shape[1] > s + 1 and np.array_equal(seqs2[b, :s + 1], seqs[b, :s + 1])
            tok = int(seqs2[b, s + 1]) if same else -1
            ok = same and ((tok == int(seqs[b, s + 1]) and tok != target) if kind == "suppressed" else
                           (tok != int(seqs[b, s + 1]) and (tok == target) != (kind == "neg1")))
            if ok:
                rows[b] = trial[b]
                events.append(Event(kind, b, s, tuple(add), target))
                todo[b].pop(0)
                keep = True
            at[b] = s + 1
        if keep:      # the accepted lists together (rows are independent: the run of each is the trial's)
            seqs, lg = run(rows)
    if "prompt_len" in kinds:
        # a sequence of length n_prompt + 1 whose prefix is the whole prompt and whose bias would win the first step: never active there
        s = n_begin - 1
        for b in todo:
            hist = [int(t) for t in seqs[b, :s + 1]]
            x = HFBias(rows[b])(lg[s, b], hist)
            pre = mask_of(x.shape[0], hist, n_begin, opt)
            w = pick(x, hist, n_begin, opt)
            free = [int(t) for t in np.flatnonzero(~pre) if int(t) != w and int(t) >= 1]
            if not free:
                continue
            t = max(free, key=lambda v: float(x[v]))
            key = tuple(hist) + (t,)
            if min(key) < 1:
                continue
            rows[b] = {**(rows[b] or {}), key: _f32(_need(x, pre, t) + MARGIN)}
            events.append(Event("prompt_len", b, s, (key,), t))
        seqs, lg = run(rows)
    return rows, events, seqs, lg


def events_seen(events: Sequence[Event], rows, seqs: np.ndarray, lg: np.ndarray, n_begin: int, opt: wo.GreedyOptions) -> set:
    """Kinds that were decisive in the run (seqs, raw logits lg) - recomputed from the run alone, through HF's processor.  Decisive: the
    pick from x' (the whole list) is the run's token and differs from the pick from x (no list) AND from the pick without the event's
    sequences; "two_onto_one": either sequence alone leaves the pick of neither; "suppressed": the biased id is masked, its x' is the
    row's largest logit, and the token is what it is without the event; "prompt_len": HF does not apply the sequence at the first step,
    where applying it would change the pick."""
    seen = set()
    for e in events:
        b, s = e.row, e.step
        if seqs.shape[1] <= s + 1 or opt.eos in [int(t) for t in seqs[b, n_begin:s + 1]]:
            continue
        hist = [int(t) for t in seqs[b, :s + 1]]
        tok = int(seqs[b, s + 1])
        x = lg[s, b]
        full = HFBias(rows[b])(x, hist)
        minus = HFBias({k: v for k, v in rows[b].items() if k not in e.keys})(x, hist)
        p_full, p_minus, p_raw = (pick(z, hist, n_begin, opt) for z in (full, minus, x))
        if tok != p_full:
            continue
        if e.kind == "suppressed":
            pre = mask_of(x.shape[0], hist, n_begin, opt)
            if pre[e.target] and full[e.target] > minus[e.target] and int(np.argmax(full)) == e.target and p_full == p_minus and tok != e.target:
                seen.add(e.kind)
        elif e.kind == "prompt_len":
            key = e.keys[0]
            forced = minus.copy()
            forced[e.target] = np.float32(forced[e.target] + np.float32(rows[b][key]))
            if len(key) == n_begin + 1 and list(key[:-1]) == hist and s == n_begin - 1 and full[e.target] == minus[e.target] \
                    and pick(forced, hist, n_begin, opt) == e.target != p_full:
                seen.add(e.kind)
        elif p_full != p_minus and p_full != p_raw:
            if e.kind == "two_onto_one":
                alone = [pick(HFBias({k: v for k, v in rows[b].items() if k != drop})(x, hist), hist, n_begin, opt) for drop in e.keys]
                if all(a == p_minus for a in alone) and max(len(k) for k in e.keys) >= 3:
                    seen.add(e.kind)
            elif e.kind == "ts_flip":
                tb = opt.no_timestamps_id + 1
                pre = mask_of(x.shape[0], hist, n_begin, opt)
                if sj._mass_margin(minus, pre, tb) < 0 < sj._mass_margin(full, pre, tb) and p_full >= tb > p_minus:
                    seen.add(e.kind)
            elif e.kind == "len3":
                if all(len(k) >= 3 for k in e.keys):
                    seen.add(e.kind)
            elif e.kind == "pos1":
                if all(len(k) == 1 and rows[b][k] > 0 for k in e.keys):
                    seen.add(e.kind)
            elif e.kind == "neg1":
                if all(len(k) == 1 and rows[b][k] < 0 for k in e.keys) and p_minus == e.target:
                    seen.add(e.kind)
    return seen


def judge_biased(lg: np.ndarray, seqs: np.ndarray, n_begin: int, opt: wo.GreedyOptions, rows) -> sj.Verdict:
    """sampler_judge.judge on x' = HF's SequenceBiasLogitsProcessor applied to the raw logits, per step and row."""
    return sj.judge(biased_logits(lg, seqs, n_begin, rows), seqs, n_begin, opt)


# --------------------------------------------------------------------------------------------------------------------
# bit-level sum order
# --------------------------------------------------------------------------------------------------------------------
def sum_order_betas() -> Tuple[float, float, float]:
    """Three float32 biases, large against any logit, whose sum in list order, (b1 + b2) + b3, is LARGER than b1 + (b2 + b3)."""
    rng = np.random.default_rng(7)
    f = np.float32
    for _ in range(10000):
        b1, b2, b3 = (f(300.0 + rng.random()), f(200.0 + rng.random()), f(100.0 + rng.random()))
        if f(f(b1 + b2) + b3) > f(b1 + f(b2 + b3)):
            return float(b1), float(b2), float(b3)
    raise AssertionError("no such triple")


def sum_order_lists(built: sj.Built, plain: np.ndarray, n_begin: int) -> Tuple[int, int, BiasDict]:
    """(lo, hi, list) for row 0 at the first judged step: a planted duplicate pair (bit-equal logits) unmasked there; lo gets three
    active sequences - length 1, 2 and 3 - and hi the single float32 value (b1 + b2) + b3.  In list order the two totals are the same
    float32, the tie survives and lo, the lower id, wins; summed in the other association lo falls one ulp short and hi wins."""
    hist = [int(t) for t in plain[0, :n_begin]]
    pre = mask_of(built.dims.vocab, hist, n_begin, built.opt)
    pairs = [p for kind, lst in built.planted.items() if kind != "masked_lower" for p in lst if not pre[p[0]] and not pre[p[1]]]
    assert pairs, "no planted duplicate pair is unmasked at the first step"
    lo, hi = min(pairs[0]), max(pairs[0])
    b1, b2, b3 = sum_order_betas()
    single = float(np.float32(np.float32(np.float32(b1) + np.float32(b2)) + np.float32(b3)))
    lst: BiasDict = {(hist[-1], lo): b2, (hist[-2], hist[-1], lo): b3, (lo,): b1, (hist[-1], hi): single}
    return lo, hi, lst
