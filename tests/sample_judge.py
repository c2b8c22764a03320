"""A host-side mirror and judge of the temperature sampler (k_decode.hip: sample_part_kernel, sample_finish_kernel; the draw is defined
at SampleArgs in tw_common.h and in include/thewhisper.h).  No GPU in here.  Built on tests/sampler_judge.py: the same crafted
zero-layer models, replay idea and `MASS_BAND`.  The mirror restates the draw in numpy, float64 behind the float32 inputs.

`judge_sampled` calls a step `undecided`, and accepts either candidate, when the mass rule is inside MASS_BAND or the two largest
perturbed scores are within SAMPLE_BAND = 1e-4.  Derivation: x * inv_t rounds to half an ulp of a value below 256, about 1.5e-5; g
stays within (-2.9, 16.7) with a few ulp of logf error, about 4e-6; both on each of the two scores compared: about 4e-5 (the sum's own
rounding, half an ulp below 512, still fits).  Every case must keep |x| / T < 256, which `judge_sampled` asserts.  Rows with temperature
0 are judged as greedy rows (exact); rows with a negative temperature must hold `pad` from the begin index on.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests import sampler_judge as sj

SAMPLE_BAND = 1e-4
MASS_BAND = sj.MASS_BAND
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)


# --------------------------------------------------------------------------------------------------------------------
# the draw
# --------------------------------------------------------------------------------------------------------------------
def philox4x32_10(counter: Sequence, key: Sequence) -> np.ndarray:
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11).  `counter`: four words, `key`: two words,
    each a scalar or an array (broadcast together); returns uint32 [..., 4]."""
    c = [np.asarray(x, dtype=np.uint64) & _LO for x in np.broadcast_arrays(*[np.asarray(x, dtype=np.uint64) for x in counter])]
    k0, k1 = (int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & _LO, p1 >> np.uint64(32), p1 & _LO
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=-1).astype(np.uint32)


def u_of(w) -> np.ndarray:
    """The uniform of a Philox word: ((w >> 9) * 2 + 1) * 2^-24 - an odd multiple of 2^-24 below 1: exact in float32, never 0 or 1."""
    w = np.asarray(w, dtype=np.uint64)
    return ((w >> np.uint64(9)) * np.uint64(2) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def gumbel(V: int, p: int, seed: int, offset: int) -> np.ndarray:
    """g(v) for v in [0, V) at position p, float64."""
    seed, offset = int(seed), int(offset)
    blocks = philox4x32_10((np.arange((V + 3) // 4, dtype=np.uint64), p, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                           (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = blocks.reshape(-1)[:V]                      # id v is word v & 3 of block v >> 2
    return -np.log(-np.log(u_of(w)))


def inv_t32(T: float) -> np.float32:
    return np.float32(1.0) / np.float32(T)          # the host's 1.0f / T


def scores(x: np.ndarray, T: float, p: int, seed: int, offset: int) -> np.ndarray:
    """score(v) in float64 for processed logits x (float32, -inf = masked)."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(np.isneginf(x), -np.inf, x * np.float64(inv_t32(T)) + gumbel(len(x), p, seed, offset))


def draw(lg: np.ndarray, seq: Sequence[int], n_begin: int, opt: wo.GreedyOptions, T: float, seed: int, offset: int) -> int:
    """The token row `seq` (prompt included; it consumes position len(seq) - 1) gets from float32 logits `lg`."""
    natural = wo.apply_logits_processors(np.asarray(lg, dtype=np.float32), list(seq), n_begin, opt)    # mass rule included, on lg itself
    if T == 0:
        return int(np.argmax(natural))
    return int(np.argmax(scores(natural, T, len(seq) - 1, seed, offset)))       # all -inf: 0


def mirror_generate(model: wo.OracleWhisper, enc: np.ndarray, prompt: np.ndarray, opt: wo.GreedyOptions, temperature, seed, offset=None,
                    cross_out: Optional[list] = None):
    """tw_generate_sample on the numpy oracle: (sequences [B, L], logits [L-1, B, V] float32 at positions 0 .. L-2).  Rows with
    temperature < 0 sit the call out; the call ends when the live rows have ended or at the token budget.  `cross_out` (a list):
    receives the alignment heads' cross-attention rows [B, Ha, L-1, T] when `opt.alignment_heads` is set."""
    prompt = np.asarray(prompt, dtype=np.int64)
    B, n0 = prompt.shape
    temperature = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (B,))
    seed = np.broadcast_to(np.asarray(seed, dtype=np.uint64), (B,))
    offset = np.broadcast_to(np.asarray(0 if offset is None else offset, dtype=np.uint64), (B,))
    assert np.isfinite(temperature).all() and (temperature >= 0).any()
    cache = model.new_cache(enc)
    seqs = [list(map(int, r)) for r in prompt]
    unfinished = temperature >= 0
    max_len = min(opt.max_length, n0 + opt.max_new_tokens)
    rows: List[np.ndarray] = []
    crosses: List[np.ndarray] = []
    feed = prompt
    while True:
        logits, cross = model.decode(feed, cache, want_cross=opt.alignment_heads)
        if cross is not None:
            crosses.append(cross)
        for s in range(logits.shape[1]):
            rows.append(logits[:, s].astype(np.float32))
        last = rows[-1]
        nxt = np.zeros(B, dtype=np.int64)
        for i in range(B):
            tok = draw(last[i], seqs[i], n0, opt, float(temperature[i]), int(seed[i]), int(offset[i])) if unfinished[i] else opt.pad
            nxt[i] = tok
            seqs[i].append(tok)
        unfinished = unfinished & (nxt != opt.eos)
        if len(seqs[0]) >= max_len or not unfinished.any():
            break
        feed = nxt[:, None]
    if cross_out is not None and crosses:
        cross_out.append(np.concatenate(crosses, axis=2))
    return np.asarray(seqs, dtype=np.int64), np.stack(rows)


# --------------------------------------------------------------------------------------------------------------------
# the judge
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class SampledVerdict:
    status: np.ndarray                     # [L-1, B] of "prompt" | "ok" | "undecided" | "wrong"
    drawn: int = 0                         # judged steps of live rows with temperature > 0 that were not yet finished
    differ: int = 0                        # ... at which the token is not the processors' argmax
    wrong: List[dict] = field(default_factory=list)

    def count(self, what: str) -> int:
        return int((self.status == what).sum())

    @property
    def judged(self) -> int:
        return int((self.status != "prompt").sum())

    def summary(self) -> str:
        return (f"judged {self.judged} ok {self.count('ok')} undecided {self.count('undecided')} wrong {self.count('wrong')} | "
                f"drawn {self.drawn}, not the argmax at {self.differ} ({100.0 * self.differ / max(1, self.drawn):.0f} %)")


def _pre_mask(V: int, tb: int, seq: List[int], n_begin: int, opt: wo.GreedyOptions) -> np.ndarray:
    """Everything the processors mask AHEAD of the mass rule, read off apply_logits_processors itself (see sampler_judge.judge)."""
    probe = np.zeros(V, np.float32)
    probe[tb:] = -1e30
    pre = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))
    probe = np.zeros(V, np.float32)
    probe[:tb] = -1e30
    pre[tb:] = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))[tb:]
    return pre


def judge_sampled(logits: np.ndarray, sequences: np.ndarray, n_begin: int, opt: wo.GreedyOptions, temperature, seed, offset=None
                  ) -> SampledVerdict:
    """logits [L-1, B, V] float32 (row s: what the sampler read when it produced position s + 1), sequences [B, L] as returned by
    the sampling call with per-row `temperature`, `seed`, `offset`."""
    logits, sequences = np.asarray(logits), np.asarray(sequences)
    B, L = sequences.shape
    assert logits.shape[:2] == (L - 1, B), (logits.shape, sequences.shape)
    V = logits.shape[2]
    temperature = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (B,))
    seed = np.broadcast_to(np.asarray(seed, dtype=np.uint64), (B,))
    offset = np.broadcast_to(np.asarray(0 if offset is None else offset, dtype=np.uint64), (B,))
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    ids = np.arange(V)
    status = np.full((L - 1, B), "prompt", dtype=object)
    v = SampledVerdict(status)
    for b in range(B):
        T = float(temperature[b])
        if T > 0:      # the band's premise
            assert float(np.abs(logits[:, b][np.isfinite(logits[:, b])]).max()) * float(inv_t32(T)) < 256.0, "|x| / T must stay below 256"
        for s in range(n_begin - 1, L - 1):
            seq = [int(t) for t in sequences[b, :s + 1]]
            tok = int(sequences[b, s + 1])
            if T < 0 or opt.eos in seq[n_begin:]:       # sits the call out / finished: pad
                status[s, b] = "ok" if tok == opt.pad else "wrong"
                if tok != opt.pad:
                    v.wrong.append(dict(step=s, stream=b, rule="pad", expected=opt.pad, got=tok))
                continue
            lg = logits[s, b].astype(np.float32)
            pre = _pre_mask(V, tb, seq, n_begin, opt)
            d = sj._mass_margin(lg, pre, tb) if opt.timestamps else float("-inf")
            mass_open = bool(opt.timestamps and np.isfinite(d) and abs(d) <= MASS_BAND and int((~pre[tb:]).sum()) != 1)
            x = np.where(pre, -np.inf, lg).astype(np.float32)
            sc = scores(x, T, s, int(seed[b]), int(offset[b])) if T > 0 else x.astype(np.float64)
            band = SAMPLE_BAND if T > 0 else 0.0
            sets = []
            if mass_open or not (d > 0):
                sets.append(sc)                                              # the rule does not fire: every unmasked id
            if mass_open or d > 0:
                sets.append(np.where(ids < tb, -np.inf, sc))                 # it fires: timestamps only
            accept, close = set(), mass_open
            for z in sets:
                top = z.max()
                if not np.isfinite(top):
                    accept.add(0)
                    continue
                near = np.flatnonzero(z >= top - band)
                if T > 0 and len(near) > 1:
                    close = True
                    accept.update(int(i) for i in near)
                else:
                    accept.add(int(near[0]))                                 # lowest id at the maximum
            natural = wo.apply_logits_processors(lg, seq, n_begin, opt)
            if T > 0:
                v.drawn += 1
                v.differ += int(tok != int(np.argmax(natural)))
            if tok not in accept:
                status[s, b] = "wrong"
                v.wrong.append(dict(step=s, stream=b, T=T, accepted=sorted(accept)[:4], got=tok, got_masked=bool(pre[tok]), mass_margin=d,
                                    score_got=float(sc[tok]), score_top=float(max(z.max() for z in sets)), tail=seq[-3:]))
                continue
            status[s, b] = "undecided" if close else "ok"
    return v


# --------------------------------------------------------------------------------------------------------------------
# cases: sampler_judge layouts x temperatures, for the CPU proof (the mirror's own run meets every condition) and for the GPU replay
# --------------------------------------------------------------------------------------------------------------------
MIXED = (0.0, -1.0, 0.2, 0.6, 1.0)


@dataclass(frozen=True)
class SampleCase:
    name: str
    base: str                          # sampler_judge case: layout, model, options
    temperature: object                # one float for every row, or a tuple cycled over the rows
    B: Optional[int] = None
    graph: bool = False


SAMPLE_CASES: List[SampleCase] = [
    SampleCase("v66-t0.6", "v66", 0.6, B=6),
    SampleCase("v127-no-timestamps-t1.0", "v127-no-timestamps", 1.0),
    SampleCase("v1000-ts-odd-t0.2", "v1000-ts-odd", 0.2),
    SampleCase("v1000-ts-odd-t0.2-graph", "v1000-ts-odd", 0.2, graph=True),
    SampleCase("v1000-ts-odd-t1.0", "v1000-ts-odd", 1.0),
    SampleCase("v1000-ts-odd-t1.0-graph", "v1000-ts-odd", 1.0, graph=True),
    SampleCase("v2049-t0.4", "v2049", 0.4),
    SampleCase("real-f32-t0.6", "real-f32", 0.6, B=3),            # V = 51865: the scalar path
    SampleCase("v1000-bf16-t0.6", "v1000-bf16", 0.6),
    SampleCase("v1000-f16-t0.6", "v1000-f16", 0.6),
    SampleCase("v1000-b33-mixed", "v1000-b33", MIXED),
]


def sample_case_by_name(name: str) -> SampleCase:
    return next(c for c in SAMPLE_CASES if c.name == name)


@dataclass
class BuiltSample:
    case: SampleCase
    built: sj.Built
    temperature: np.ndarray
    seed: np.ndarray
    offset: np.ndarray


def build_sample_case(sc: SampleCase) -> BuiltSample:
    base = sj.case_by_name(sc.base)
    base = dataclasses.replace(base, B=sc.B or base.B, graph=sc.graph)
    built = sj.build_case(base)
    B = base.B
    t = np.asarray([sc.temperature[b % len(sc.temperature)] for b in range(B)] if isinstance(sc.temperature, tuple) else [sc.temperature] * B,
                   dtype=np.float32)
    seed = np.asarray([0x123456789ABCDEF0 + 977 * b for b in range(B)], dtype=np.uint64)           # both key words in use
    offset = np.asarray([(b + 1) * 0x100000001 + 7 for b in range(B)], dtype=np.uint64)            # both counter words in use
    return BuiltSample(sc, built, t, seed, offset)


def mirror_run(bs: BuiltSample) -> Tuple[np.ndarray, np.ndarray]:
    """The mirror's own run of a case on the crafted zero-layer model: (sequences, logits)."""
    b = bs.built
    om = sj._OracleExactTies(b.dims, b.weights, T=sj.T_FRAMES)
    enc = np.zeros((b.prompt.shape[0], sj.T_FRAMES, b.dims.d_model), np.float32)        # no decoder layer reads it
    return mirror_generate(om, enc, b.prompt, b.opt, bs.temperature, bs.seed, bs.offset)


def check_conditions(v: SampledVerdict, what: str) -> None:
    """What every run of a case - the mirror's here, the engine's on the GPU - must show."""
    assert v.count("wrong") == 0, (what, v.wrong[:3])
    assert v.count("undecided") * 100 <= v.judged, (what, v.count("undecided"), v.judged)
    assert v.judged >= 40, (what, v.judged)
    assert v.differ * 4 >= v.drawn > 0, (what, "the noise does not show:", v.differ, v.drawn)


# --------------------------------------------------------------------------------------------------------------------
# a crafted model whose greedy output repeats for some rows and not for others (the temperature fallback's ladder)
# --------------------------------------------------------------------------------------------------------------------
STICKY = (100, 200, 300)              # text ids that, once produced, reproduce themselves under greedy decoding
STICKY_STRENGTH = (0.16, 0.2, 0.26)   # ... with growing persistence: the weakest lets go at a low temperature, the strongest at a high one
REPEAT_LAYOUT = sj.V1000A
REPEAT_MAX_NEW = 60


def repeating_model(dtype: str = "f32"):
    """(dims, weights, prompt [6, 3], options, generate_greedy keywords) of a zero-layer model without the timestamp grammar: the rows
    of the STICKY ids live on 32 coordinates where the final LayerNorm's weight is positive, so the logit of such an id given itself
    is a sum of squares and beats every other; rows 0-2 of the prompt end in a sticky id (greedy: one token repeated, compression ratio
    about 9), rows 3-5 in ordinary ids (a random walk, ratio below 1).  Sampling leaves a sticky id the sooner the weaker its row."""
    V, eos, no_ts = REPEAT_LAYOUT
    dims, w = sj.crafted_model(V, eos, no_ts, seed=0, pos_scale=2.0, dtype=dtype)
    d = "model.decoder"
    E, g = w[d + ".embed_tokens.weight"].copy(), w[d + ".layer_norm.weight"]
    rng = np.random.default_rng(5)
    for t, a in zip(STICKY, STICKY_STRENGTH):
        sup = np.zeros(dims.d_model, bool)
        sup[rng.permutation(np.flatnonzero(g > 0))[:32]] = True
        E[t] = np.float32(a) * sup * rng.standard_normal(dims.d_model).astype(np.float32)
    w[d + ".embed_tokens.weight"] = sj.round_to(E, dtype)
    prompt = np.array([[3, 5, t] for t in STICKY + (9, 16, 23)], dtype=np.int32)
    begin = (11, eos)
    opt = wo.GreedyOptions(eos=eos, pad=eos, max_new_tokens=REPEAT_MAX_NEW, min_new_tokens=0, max_length=448, begin_suppress=begin,
                           suppress=(), timestamps=False, no_timestamps_id=no_ts, max_initial_timestamp_index=None)
    kw = dict(max_new_tokens=REPEAT_MAX_NEW, min_new_tokens=0, eos_id=eos, pad_id=eos, timestamps=False, no_timestamps_id=no_ts,
              max_initial_timestamp_index=None, begin_suppress=begin, suppress=())
    return dims, w, prompt, opt, kw


def options_of(kw: dict) -> wo.GreedyOptions:
    """generate_greedy keywords -> the oracle's options."""
    return wo.GreedyOptions(eos=kw.get("eos_id", 50257), pad=kw.get("pad_id", 50257), max_new_tokens=kw.get("max_new_tokens", 128),
                            min_new_tokens=kw.get("min_new_tokens", 0), max_length=kw.get("max_length", 448),
                            begin_suppress=tuple(kw.get("begin_suppress", (220, 50257))), suppress=tuple(kw.get("suppress", ())),
                            timestamps=kw.get("timestamps", False), no_timestamps_id=kw.get("no_timestamps_id", 50364),
                            max_initial_timestamp_index=kw.get("max_initial_timestamp_index", 50))


def oracle_scores(model: wo.OracleWhisper, enc: np.ndarray, sequences: np.ndarray, n_prompt: int, kw: dict, no_speech_id=None):
    """WhisperEngine.score_tokens on the numpy oracle: log-softmax (float64) of the processed logits at every generated token, 0 for
    the prompt and behind a row's first eos; the raw ones; softmax(raw)[no_speech_id] at position 0."""
    seq = np.asarray(sequences, dtype=np.int64)
    B, L = seq.shape
    opt = options_of(kw)
    logits, _ = model.decode(seq[:, :-1], model.new_cache(enc))
    lp, raw = np.zeros((B, L), np.float32), np.zeros((B, L), np.float32)
    ns = None
    if no_speech_id is not None:
        z = logits[:, 0].astype(np.float64)
        ns = (np.exp(z[:, no_speech_id] - z.max(-1)) / np.exp(z - z.max(-1, keepdims=True)).sum(-1)).astype(np.float32)
    for b in range(B):
        for p in range(n_prompt - 1, L - 1):
            t = int(seq[b, p + 1])
            z = logits[b, p].astype(np.float64)
            raw[b, p + 1] = z[t] - (z.max() + np.log(np.exp(z - z.max()).sum()))
            m = wo.apply_logits_processors(logits[b, p].astype(np.float32), [int(x) for x in seq[b, :p + 1]], n_prompt, opt).astype(np.float64)
            lp[b, p + 1] = m[t] - (m.max() + np.log(np.exp(m - m.max()).sum())) if np.isfinite(m[t]) else -np.inf
            if t == opt.eos:
                break
    return {"logprob": lp, "logprob_raw": raw, "no_speech_prob": ns}
