"""A host-side mirror and judge of the top-k / top-p filtered draw (k_decode.hip: sample_filter_kernel; the rule is stated at
tw_generate_sample_filtered in include/thewhisper.h and at FilterArgs in tw_common.h).  No GPU in here.  Built on tests/sample_judge.py
and tests/sampler_judge.py: the same crafted zero-layer models, replay idea, bands and Philox mirror.

`kept(x, inv_t, k, p)` restates the rule in numpy, float64 behind the float32 x and y.  Top-k is exact: the k-th largest float32
value, ties kept.  `judge_filtered` accepts a token iff it is the perturbed arg-max over an ADMISSIBLE kept set: the top-k membership
as the mirror has it, and a top-p membership taken either way when |G(v) / Z - top_p| <= TOPP_BAND.

TOPP_BAND = 1e-4 (the value of MASS_BAND).  Derivation for the reduction built: the kernel evaluates e = exp(y - m) in float32 with
the fast exponential, 2^((y - m) * log2 e): the product rounds to half an ulp of a value below 128 (every case keeps |y| < 256 and the
terms that matter lie within 88 of the maximum), 2^-18 = 3.8e-6 in the exponent, so about 2.7e-6 relative in e, plus one ulp or so of
the hardware's 2^x, 1.2e-7; a thread's 64 terms are added in float32, at most 64 * 2^-24 = 3.8e-6 relative; the 1024 threads' sums in
double, nothing to speak of.  G and Z are sums of non-negative terms with relative error below 7e-6 each, so G / Z is within 1.4e-5
of the exact quotient, and top_p * Z (double) adds nothing: the band of 1e-4 holds with a factor of 7 to spare and stays at the
issue's value.  A step is `undecided` when the admissible picks differ or when one of sample_judge's own bands is open.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests import sample_judge as sm
from tests import sampler_judge as sj

TOPP_BAND = 1e-4
SAMPLE_BAND = sm.SAMPLE_BAND
MASS_BAND = sm.MASS_BAND


# --------------------------------------------------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------------------------------------------------
def kept_margins(x: np.ndarray, inv_t, k: int, p: float) -> Tuple[np.ndarray, np.ndarray]:
    """(kept [V] bool, margin [V] float64) for processed logits x (float32, -inf = masked; the mass rule already applied).  margin =
    |G(v) / Z - top_p| for the ids of K when top-p is on, +inf elsewhere: how far a top-p membership is from being decided otherwise."""
    x = np.asarray(x, dtype=np.float32)
    S = x > -np.inf
    K = S.copy()
    k = int(k)
    if k > 0 and int(S.sum()) > k:
        tau = np.partition(x[S], -k)[-k]                       # the k-th largest, with multiplicity
        K = S & (x >= tau)
    margin = np.full(x.shape, np.inf)
    p32 = np.float32(p)
    if not (p32 < 1) or not K.any():
        return K, margin
    y = (x[K] * np.float32(inv_t)).astype(np.float32).astype(np.float64)       # the float32 product the draw perturbs
    e = np.exp(y - y.max())
    Z = e.sum()
    uniq, inv = np.unique(y, return_inverse=True)             # ascending
    mass = np.bincount(inv, weights=e, minlength=len(uniq))
    above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])           # mass strictly above each distinct value
    G = above[inv]
    keep = np.zeros(x.shape, bool)
    keep[K] = G < float(p32) * Z
    margin[K] = np.abs(G / Z - float(p32))
    return keep, margin


def kept(x: np.ndarray, inv_t, k: int, p: float) -> np.ndarray:
    """The ids the filtered draw is taken over."""
    return kept_margins(x, inv_t, k, p)[0]


def admissible_sets(x: np.ndarray, inv_t, k: int, p: float) -> List[np.ndarray]:
    """The kept set, and every kept set that differs from it by memberships inside TOPP_BAND (a kept set is the ids at or above a
    threshold in y, so the open ids enter from the largest down)."""
    keep, margin = kept_margins(x, inv_t, k, p)
    open_ = margin <= TOPP_BAND
    if not open_.any():
        return [keep]
    y = (np.asarray(x, dtype=np.float32) * np.float32(inv_t)).astype(np.float32)
    sure = keep & ~open_
    sets = [sure.copy()]
    for cut in np.unique(y[open_])[::-1]:
        sets.append(sure | (open_ & (y >= cut)))
    return sets


def draw(lg: np.ndarray, seq, n_begin: int, opt: wo.GreedyOptions, T: float, seed: int, offset: int, k: int, p: float) -> int:
    """sample_judge.draw over the kept set."""
    natural = wo.apply_logits_processors(np.asarray(lg, dtype=np.float32), list(seq), n_begin, opt)
    if T == 0:
        return int(np.argmax(natural))
    sc = sm.scores(natural, T, len(seq) - 1, seed, offset)
    return int(np.argmax(np.where(kept(natural, sm.inv_t32(T), k, p), sc, -np.inf)))       # all -inf: 0


def _rows(x, B: int, dtype) -> np.ndarray:
    return np.broadcast_to(np.asarray(x, dtype=dtype), (B,))


def mirror_generate(model: wo.OracleWhisper, enc: np.ndarray, prompt: np.ndarray, opt: wo.GreedyOptions, temperature, seed, offset=None,
                    top_k=0, top_p=1.0):
    """tw_generate_sample_filtered on the numpy oracle (sample_judge.mirror_generate with the filtered draw): (sequences, logits)."""
    prompt = np.asarray(prompt, dtype=np.int64)
    B, n0 = prompt.shape
    temperature, seed = _rows(temperature, B, np.float32), _rows(seed, B, np.uint64)
    offset = _rows(0 if offset is None else offset, B, np.uint64)
    top_k, top_p = _rows(top_k, B, np.int64), _rows(top_p, B, np.float32)
    cache = model.new_cache(enc)
    seqs = [list(map(int, r)) for r in prompt]
    unfinished = temperature >= 0
    max_len = min(opt.max_length, n0 + opt.max_new_tokens)
    rows: List[np.ndarray] = []
    feed = prompt
    while True:
        logits, _ = model.decode(feed, cache)
        for s in range(logits.shape[1]):
            rows.append(logits[:, s].astype(np.float32))
        nxt = np.zeros(B, dtype=np.int64)
        for i in range(B):
            nxt[i] = draw(rows[-1][i], seqs[i], n0, opt, float(temperature[i]), int(seed[i]), int(offset[i]), int(top_k[i]),
                          float(top_p[i])) if unfinished[i] else opt.pad
            seqs[i].append(int(nxt[i]))
        unfinished = unfinished & (nxt != opt.eos)
        if len(seqs[0]) >= max_len or not unfinished.any():
            break
        feed = nxt[:, None]
    return np.asarray(seqs, dtype=np.int64), np.stack(rows)


# --------------------------------------------------------------------------------------------------------------------
# the judge
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class FilteredVerdict(sm.SampledVerdict):
    filtered: int = 0          # drawn steps of rows with a filter on
    shows: int = 0             # ... at which the unfiltered draw of the same (seed, offset) lies outside the kept set
    tau_inf_mass: int = 0      # ... at which the mass rule fired and fewer than k ids were left: tau = -inf
    k_above_open: int = 0      # ... at which k exceeded the number of unmasked ids (mass rule or not)
    tie_at_tau: int = 0        # ... at which the kept set is larger than k: ties at the threshold
    sizes: List[int] = field(default_factory=list)

    def summary(self) -> str:
        return (super().summary() + f" | filtered {self.filtered}, unfiltered draw outside the kept set at {self.shows}, kept sizes "
                f"{min(self.sizes, default=0)}..{max(self.sizes, default=0)}, tau = -inf under the mass rule at {self.tau_inf_mass}, "
                f"k above the open ids at {self.k_above_open}, ties at tau at {self.tie_at_tau}")


def judge_filtered(logits: np.ndarray, sequences: np.ndarray, n_begin: int, opt: wo.GreedyOptions, temperature, seed, offset=None,
                   top_k=0, top_p=1.0) -> FilteredVerdict:
    """sample_judge.judge_sampled with per-row `top_k`, `top_p`: logits [L-1, B, V] float32 (row s: what the sampler read when it
    produced position s + 1), sequences [B, L] as returned by the filtered call."""
    logits, sequences = np.asarray(logits), np.asarray(sequences)
    B, L = sequences.shape
    assert logits.shape[:2] == (L - 1, B), (logits.shape, sequences.shape)
    V = logits.shape[2]
    temperature, seed = _rows(temperature, B, np.float32), _rows(seed, B, np.uint64)
    offset = _rows(0 if offset is None else offset, B, np.uint64)
    top_k, top_p = _rows(top_k, B, np.int64), _rows(top_p, B, np.float32)
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    ids = np.arange(V)
    status = np.full((L - 1, B), "prompt", dtype=object)
    v = FilteredVerdict(status)
    for b in range(B):
        T, k, p = float(temperature[b]), int(top_k[b]), float(top_p[b])
        on = T > 0 and (k > 0 or p < 1)
        inv_t = sm.inv_t32(T) if T > 0 else np.float32(1)
        if T > 0:      # the bands' premise
            assert float(np.abs(logits[:, b][np.isfinite(logits[:, b])]).max()) * float(inv_t) < 256.0, "|x| / T must stay below 256"
        for s in range(n_begin - 1, L - 1):
            seq = [int(t) for t in sequences[b, :s + 1]]
            tok = int(sequences[b, s + 1])
            if T < 0 or opt.eos in seq[n_begin:]:       # sits the call out / finished: pad
                status[s, b] = "ok" if tok == opt.pad else "wrong"
                if tok != opt.pad:
                    v.wrong.append(dict(step=s, stream=b, rule="pad", expected=opt.pad, got=tok))
                continue
            lg = logits[s, b].astype(np.float32)
            pre = sm._pre_mask(V, tb, seq, n_begin, opt)
            d = sj._mass_margin(lg, pre, tb) if opt.timestamps else float("-inf")
            mass_open = bool(opt.timestamps and np.isfinite(d) and abs(d) <= MASS_BAND and int((~pre[tb:]).sum()) != 1)
            x = np.where(pre, -np.inf, lg).astype(np.float32)
            sc = sm.scores(x, T, s, int(seed[b]), int(offset[b])) if T > 0 else x.astype(np.float64)
            band = SAMPLE_BAND if T > 0 else 0.0
            alts = []                                         # the processed logits under each admissible mass decision
            if mass_open or not (d > 0):
                alts.append(x)
            if mass_open or d > 0:
                alts.append(np.where(ids < tb, -np.inf, x).astype(np.float32))
            accept, close, picks = set(), mass_open, set()
            for xa in alts:
                for keep in (admissible_sets(xa, inv_t, k, p) if on else [xa > -np.inf]):
                    z = np.where(keep & (xa > -np.inf), sc, -np.inf)
                    top = z.max()
                    if not np.isfinite(top):
                        accept.add(0)
                        picks.add(0)
                        continue
                    near = np.flatnonzero(z >= top - band)
                    if T > 0 and len(near) > 1:
                        close = True
                        accept.update(int(i) for i in near)
                    else:
                        accept.add(int(near[0]))                                 # lowest id at the maximum
                    picks.add(int(near[0]))
            natural = wo.apply_logits_processors(lg, seq, n_begin, opt)
            if T > 0:
                v.drawn += 1
                v.differ += int(tok != int(np.argmax(natural)))
            if on:       # the figures of the case, on the mirror's own decision
                keep = kept(natural, inv_t, k, p)
                n_open = int((natural > -np.inf).sum())
                v.filtered += 1
                v.sizes.append(int(keep.sum()))
                v.shows += int(not keep[int(np.argmax(sm.scores(natural, T, s, int(seed[b]), int(offset[b]))))])
                v.tau_inf_mass += int(k > 0 and d > 0 and not mass_open and n_open < k)
                v.k_above_open += int(k > n_open)
                v.tie_at_tau += int(0 < k < int(kept(natural, inv_t, k, 1.0).sum()))
            if tok not in accept:
                status[s, b] = "wrong"
                v.wrong.append(dict(step=s, stream=b, T=T, k=k, p=p, accepted=sorted(accept)[:4], got=tok, got_masked=bool(pre[tok]),
                                    mass_margin=d, score_got=float(sc[tok]), tail=seq[-3:]))
                continue
            status[s, b] = "undecided" if close or len(picks) > 1 else "ok"
    return v


def check_conditions(v: FilteredVerdict, what: str) -> None:
    """sample_judge.check_conditions, and "the filter shows": at 25 % or more of the drawn steps of filtered rows the unfiltered draw
    of the same (seed, offset) lies outside the kept set - an engine that ignores the filter is `wrong` there."""
    sm.check_conditions(v, what)
    assert v.shows * 4 >= v.filtered > 0, (what, "the filter does not show:", v.shows, v.filtered)


# --------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------
MIXED_FILTERS = ((0, 1.0), (8, 1.0), (0, 0.6), (50, 0.9), (2000, 1.0))


@dataclass(frozen=True)
class FilterCase:
    name: str
    base: str                          # sampler_judge case: layout, model, options
    temperature: object                # one float for every row, or a tuple cycled over the rows
    filters: object                    # (k, p) for every row, or a tuple of pairs cycled over the rows: row b takes pair stride * b
    stride: int = 1
    B: Optional[int] = None
    graph: bool = False
    tau_inf: bool = False              # the mirror's run reaches a step where the mass rule fired with fewer than k ids left
    ties: bool = False                 # ... and a step with ties at the top-k threshold


FILTER_CASES: List[FilterCase] = [
    FilterCase("v66-k3", "v66", 1.0, (3, 1.0), B=6),                                      # V below the workgroup size
    FilterCase("v127-no-timestamps-k5-p0.8", "v127-no-timestamps", 1.0, (5, 0.8), B=6),
    FilterCase("v1000-ts-odd-k8", "v1000-ts-odd", 1.0, (8, 1.0), tau_inf=True, ties=True),
    FilterCase("v1000-ts-odd-k8-graph", "v1000-ts-odd", 1.0, (8, 1.0), graph=True, tau_inf=True, ties=True),
    FilterCase("v1000-ts-odd-p0.6", "v1000-ts-odd", 1.0, (0, 0.6)),
    FilterCase("v1000-ts-odd-t0.6-k50-p0.9", "v1000-ts-odd", 0.6, (50, 0.9), tau_inf=True),
    FilterCase("v2049-k50", "v2049", 1.0, (50, 1.0), tau_inf=True),
    FilterCase("real-f32-k50", "real-f32", 1.0, (50, 1.0), B=3),                          # V = 51865, odd: 51 values per thread
    FilterCase("v1000-bf16-k8", "v1000-bf16", 1.0, (8, 1.0)),
    FilterCase("v1000-f16-k8", "v1000-f16", 1.0, (8, 1.0)),
    # rows cycle over the temperatures with b and over the filters with 2 b, so that every live temperature meets a filter: 0.2 takes
    # k = 2000 (above V), 0.6 takes k = 8, 1.0 takes (50, 0.9); cycled in step, two of the five filters would sit on the greedy and the
    # idle rows and the filter would show at 146 of 787 drawn steps of the mirror's run, below what check_conditions asks (380 of 772 so)
    FilterCase("v1000-b33-mixed", "v1000-b33", sm.MIXED, MIXED_FILTERS, stride=2, tau_inf=True),
]


def filter_case_by_name(name: str) -> FilterCase:
    return next(c for c in FILTER_CASES if c.name == name)


@dataclass
class BuiltFilter:
    case: FilterCase
    sample: sm.BuiltSample
    top_k: np.ndarray
    top_p: np.ndarray

    @property
    def built(self) -> sj.Built:
        return self.sample.built


def build_filter_case(fc: FilterCase) -> BuiltFilter:
    bs = sm.build_sample_case(sm.SampleCase(fc.name, fc.base, fc.temperature, B=fc.B, graph=fc.graph))
    B = bs.built.case.B
    pairs = [fc.filters[(fc.stride * b) % len(fc.filters)] for b in range(B)] if isinstance(fc.filters[0], tuple) else [fc.filters] * B
    return BuiltFilter(fc, bs, np.asarray([k for k, _ in pairs], dtype=np.int32), np.asarray([p for _, p in pairs], dtype=np.float32))


def mirror_run(bf: BuiltFilter) -> Tuple[np.ndarray, np.ndarray]:
    """The mirror's own run of a case on the crafted zero-layer model: (sequences, logits)."""
    b, s = bf.built, bf.sample
    om = sj._OracleExactTies(b.dims, b.weights, T=sj.T_FRAMES)
    enc = np.zeros((b.prompt.shape[0], sj.T_FRAMES, b.dims.d_model), np.float32)        # no decoder layer reads it
    return mirror_generate(om, enc, b.prompt, b.opt, s.temperature, s.seed, s.offset, bf.top_k, bf.top_p)


def judge_case(bf: BuiltFilter, logits: np.ndarray, sequences: np.ndarray, n_prompt: int) -> FilteredVerdict:
    s = bf.sample
    return judge_filtered(logits, sequences, n_prompt, bf.built.opt, s.temperature, s.seed, s.offset, bf.top_k, bf.top_p)
