"""A host-side judge for the greedy sampler (k_decode.hip: sampler_part_kernel, sampler_merge, sampler_finish_kernel,
sampler_rows_finish_kernel, suppress_bitmap_kernel), and the crafted zero-layer models it is used on.  No GPU in here.

With `dec_layers=0` the logits of a step are LN(E[token] + P[position]) E^T: a function of the input token and its position alone, so
feeding a finished sequence back through `decode_step` reproduces, launch for launch, the logits the loop inside `generate_greedy`
sampled from.  `judge` then decides per step and stream whether the appended token is the one HF's processors + argmax pick from
THOSE logits (`oracle.whisper_oracle.apply_logits_processors`, `np.argmax`): equality of ids, ties included, with GEMM rounding out of
the comparison.  Which rule decided a step is reported too, so that a test can demand that every rule did decide something.

The one decision that depends on float32 summation order is the timestamp-mass rule.  The kernel merges 32 slice sums in float32; the
judge compares d = logsumexp(timestamps) - max(text) in float64.  Logits here are below ~50 in magnitude and a float32 log-sum-exp over
at most 1501 terms merged in 32 parts is off by a few 1e-5 at worst, so |d| <= MASS_BAND = 1e-4 is `undecided`: either outcome is
accepted there and the judge continues along the sequence it was given.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests.util import dims_variant

MASS_BAND = 1e-4
T_FRAMES = 50          # encoder frames of every crafted engine (1 s chunks); the zero-layer decoder never looks at them

# every rule a step can be decided by (ISSUE: "Nothing shows that each grammar rule changes a result")
RULES = ("pair_ts_ts", "pair_ts_text", "mono_next", "mono_same", "initial", "max_initial", "mass", "no_ts", "min_new",
         "begin_suppress", "suppress", "pad_after_eos", "all_masked")


# --------------------------------------------------------------------------------------------------------------------
# crafted models
# --------------------------------------------------------------------------------------------------------------------
def round_to(x: np.ndarray, dtype: str) -> np.ndarray:
    """float32 values representable in the engine's element type (so that the engine's conversion of the weights is exact)."""
    if dtype == "f32":
        return np.asarray(x, dtype=np.float32)
    if dtype == "f16":
        return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)
    assert dtype == "bf16", dtype
    return wo.bf16_round(np.asarray(x, dtype=np.float32)).astype(np.float32)


def crafted_model(V: int, eos: int, no_ts: int, seed: int = 0, pos_scale: float = 1.0, ts_dir: float = 0.75, eos_scale: float = 1.0,
                  no_ts_scale: float = 1.0, gain: float = 1.0, dups: Sequence[Tuple[int, int]] = (), dtype: str = "f32"):
    """(dims, weights) of a one-encoder-layer, zero-decoder-layer model with vocabulary V whose tables are shaped for the sampler:
      * random signs on the final LayerNorm's weight: with a tied embedding the input token otherwise boosts its own logit and every
        stream repeats one token; with the signs the next token depends on the last one like a random bigram table, and on the
        position (embed_positions x pos_scale), so streams that start from different prompt tokens take different paths;
      * a common unit direction x ts_dir added to every timestamp row (> no_ts): the timestamp MASS then beats the best text token
        at steps where the best single timestamp does not;
      * the eos row x eos_scale: some streams finish early, others do not; the no_ts row x no_ts_scale: the id that is always
        masked under timestamps would be picked at some steps;
      * the final LayerNorm's weight and bias x gain: peakedness of the logits;
      * dups = [(src, dst), ...]: row dst of embed_tokens := row src, which makes logits[dst] == logits[src] bit for bit at every step.
    Decoder tables are rounded to `dtype`, so a 16-bit engine holds exactly these values."""
    dims = dims_variant("micro", vocab=V, enc_layers=1, dec_layers=0)
    w = dict(wo.make_weights(dims, seed))
    d = "model.decoder"
    emb = w[d + ".embed_tokens.weight"].copy()
    rng = np.random.default_rng(1000 + seed)
    u = rng.standard_normal(dims.d_model).astype(np.float32)
    u /= np.linalg.norm(u)
    emb[no_ts + 1:] += np.float32(ts_dir) * u
    emb[eos] *= np.float32(eos_scale)
    emb[no_ts] *= np.float32(no_ts_scale)
    for src, dst in dups:
        emb[dst] = emb[src]
    w[d + ".embed_tokens.weight"] = round_to(emb, dtype)
    w[d + ".embed_positions.weight"] = round_to(w[d + ".embed_positions.weight"] * np.float32(pos_scale), dtype)
    signs = np.where(rng.random(dims.d_model) < 0.5, -1.0, 1.0).astype(np.float32)
    w[d + ".layer_norm.weight"] = round_to(w[d + ".layer_norm.weight"] * signs * np.float32(gain), dtype)
    w[d + ".layer_norm.bias"] = round_to(w[d + ".layer_norm.bias"] * np.float32(gain), dtype)
    return dims, w


def logits_f64(weights: Dict[str, np.ndarray], ids: np.ndarray, pos: int) -> np.ndarray:
    """float64 restatement of a zero-layer step: LN(E[ids] + P[pos]) E^T, [B, V]."""
    d = "model.decoder"
    E = weights[d + ".embed_tokens.weight"].astype(np.float64)
    x = E[np.asarray(ids)] + weights[d + ".embed_positions.weight"][pos].astype(np.float64)
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    h = (x - mu) / np.sqrt(var + 1e-5) * weights[d + ".layer_norm.weight"].astype(np.float64) + weights[d + ".layer_norm.bias"].astype(np.float64)
    return h @ E.T


class _OracleExactTies(wo.OracleWhisper):
    """The numpy oracle with the logits of identical embedding rows computed ONCE: BLAS sums a row's products in an order that depends on
    where the row sits in the matrix, so two identical rows need not come out bit-equal from one matmul.  (A GPU replay has to
    show its duplicated columns bit-equal before it may count them as ties.)"""

    def _dec_logits(self, x):
        if not hasattr(self, "_uniq"):
            self._uniq = np.unique(self.w["model.decoder.embed_tokens.weight"], axis=0, return_inverse=True)
        rows, inverse = self._uniq
        return (self._ln(x, "model.decoder.layer_norm") @ rows.T)[..., np.asarray(inverse).reshape(-1)]


def oracle_run(dims, weights, prompt: np.ndarray, opt: wo.GreedyOptions, begin_index: Optional[int] = None):
    """wo.greedy_generate on a zero-layer model: (sequences [B, L], logits [L-1, B, V] at positions 0 .. L-2)."""
    assert dims.dec_layers == 0
    om = _OracleExactTies(dims, weights, T=T_FRAMES)
    prompt = np.asarray(prompt)
    enc = np.zeros((prompt.shape[0], T_FRAMES, dims.d_model), np.float32)   # no decoder layer reads it
    out = wo.greedy_generate(om, enc, prompt, opt, begin_index=begin_index)
    seqs = out["sequences"]
    cache = om.new_cache(enc)
    lg = [om.decode(seqs[:, s:s + 1], cache)[0][:, 0].astype(np.float32) for s in range(seqs.shape[1] - 1)]
    return seqs, np.stack(lg)


# --------------------------------------------------------------------------------------------------------------------
# the judge
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class Verdict:
    status: np.ndarray                                   # [L-1, B] of "prompt" | "ok" | "undecided" | "wrong"
    decisive: Dict[str, List[Tuple[int, int]]]           # rule -> [(step, stream)] where removing that rule alone changes the token
    ties: List[Tuple[int, int, Tuple[int, ...]]]         # (step, stream, ids): the maximum after the processors is attained at all of `ids`
    masked_ties: List[Tuple[int, int, int, int]]         # (step, stream, lower, chosen): raw logits equal, the lower id masked
    wrong: List[dict] = field(default_factory=list)      # one report per wrong step

    def count(self, what: str) -> int:
        return int((self.status == what).sum())

    @property
    def judged(self) -> int:
        return int((self.status != "prompt").sum())

    def tie_pairs(self) -> set:
        out = set()
        for _, _, ids in self.ties:
            out.update((a, b) for i, a in enumerate(ids) for b in ids[i + 1:])
        return out

    def summary(self) -> str:
        dec = ", ".join(f"{r}:{len(v)}" for r, v in self.decisive.items() if v)
        return (f"judged {self.judged} ok {self.count('ok')} undecided {self.count('undecided')} wrong {self.count('wrong')} | "
                f"ties {len(self.ties)} masked-lower ties {len(self.masked_ties)} | decisive {dec}")


def _rule_masks(V: int, seq: Sequence[int], n_begin: int, opt: wo.GreedyOptions) -> Dict[str, np.ndarray]:
    """The processors' masks one rule at a time.  Used for ATTRIBUTION only: `judge` checks at every step that their union is
    exactly what apply_logits_processors masks, and takes the token to compare with from apply_logits_processors itself."""
    m: Dict[str, np.ndarray] = {}

    def rng(lo, hi):
        x = np.zeros(V, bool)
        x[max(lo, 0):max(hi, 0)] = True
        return x

    def ids(lst):
        x = np.zeros(V, bool)
        x[[i for i in lst if 0 <= i < V]] = True
        return x

    n_new = len(seq) - n_begin
    if opt.min_new_tokens > 0 and n_new < opt.min_new_tokens:
        m["min_new"] = ids([opt.eos])
    if opt.begin_suppress and n_new == 0:
        m["begin_suppress"] = ids(opt.begin_suppress)
    if opt.suppress:
        m["suppress"] = ids(opt.suppress)
    if opt.timestamps:
        tb = opt.no_timestamps_id + 1
        m["no_ts"] = ids([opt.no_timestamps_id])
        sampled = list(seq[n_begin:])
        last_ts = len(sampled) >= 1 and sampled[-1] >= tb
        penult_ts = len(sampled) < 2 or sampled[-2] >= tb
        if last_ts and penult_ts:
            m["pair_ts_ts"] = rng(tb, V)
        if last_ts and not penult_ts:
            m["pair_ts_text"] = rng(0, opt.eos)
        stamps = [t for t in sampled if t >= tb]
        if stamps:
            if last_ts and not penult_ts:
                m["mono_same"] = rng(tb, stamps[-1])
            else:
                m["mono_next"] = rng(tb, stamps[-1] + 1)
        if n_new == 0:
            m["initial"] = rng(0, tb)
            if opt.max_initial_timestamp_index is not None:
                m["max_initial"] = rng(tb + opt.max_initial_timestamp_index + 1, V)
    return m


def _mass_margin(lg: np.ndarray, masked: np.ndarray, tb: int) -> float:
    """d = logsumexp(unmasked timestamp logits) - max(unmasked text logits) in float64 (+-inf where one side is empty, nan where both)."""
    x = np.where(masked, -np.inf, lg.astype(np.float64))
    ts, tx = x[tb:], x[:tb]
    mt = ts.max() if ts.size else -np.inf
    mx = tx.max() if tx.size else -np.inf
    if not np.isfinite(mt):
        return float("nan") if not np.isfinite(mx) else float("-inf")
    lse = mt + np.log(np.exp(ts - mt).sum())
    return float(lse - mx) if np.isfinite(mx) else float("inf")


def _pick(lg: np.ndarray, masked: np.ndarray, opt: wo.GreedyOptions, mass: bool = True) -> int:
    s = np.where(masked, -np.inf, lg)
    if opt.timestamps and mass:
        tb = opt.no_timestamps_id + 1
        d = _mass_margin(lg, masked, tb)
        if d > 0:
            s[:tb] = -np.inf
    return int(np.argmax(s))


def judge(logits: np.ndarray, sequences: np.ndarray, n_begin: int, opt: wo.GreedyOptions) -> Verdict:
    """logits [L-1, B, V] float32 (row s: what the sampler read when it produced position s + 1), sequences [B, L] as returned by the
    call, n_begin: the begin index of the generation (= n_prompt of a plain call, n_prompt - n_forced / - n_draft otherwise; tokens
    from n_begin on are judged, forced ones included: they came out of a generation, `wo.greedy_generate(begin_index=...)`)."""
    logits = np.asarray(logits)
    sequences = np.asarray(sequences)
    B, L = sequences.shape
    assert logits.shape[:2] == (L - 1, B), (logits.shape, sequences.shape)
    V = logits.shape[2]
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    status = np.full((L - 1, B), "prompt", dtype=object)
    v = Verdict(status, {r: [] for r in RULES}, [], [])
    for b in range(B):
        for s in range(n_begin - 1, L - 1):
            seq = [int(t) for t in sequences[b, :s + 1]]
            tok = int(sequences[b, s + 1])
            lg = logits[s, b].astype(np.float32)
            natural = wo.apply_logits_processors(lg, seq, n_begin, opt)
            if opt.eos in seq[n_begin:]:                        # a finished row keeps receiving pad (HF:generation/utils.py:2929-2936)
                status[s, b] = "ok" if tok == opt.pad else "wrong"
                if int(np.argmax(natural)) != opt.pad:
                    v.decisive["pad_after_eos"].append((s, b))
                if tok != opt.pad:
                    v.wrong.append(dict(step=s, stream=b, rule="pad_after_eos", expected=opt.pad, got=tok))
                continue
            expected = int(np.argmax(natural))
            # everything the processors mask ahead of the mass rule, read off apply_logits_processors itself: with the timestamps
            # pushed far down the mass rule cannot fire and the text side shows its mask; with the text pushed down, the timestamp side
            probe = np.zeros(V, np.float32)
            probe[tb:] = -1e30
            pre = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))
            probe = np.zeros(V, np.float32)
            probe[:tb] = -1e30
            pre[tb:] = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))[tb:]
            masks = _rule_masks(V, seq, n_begin, opt)
            union = np.zeros(V, bool)
            for x in masks.values():
                union |= x
            assert np.array_equal(union, pre), f"judge: rule masks disagree with apply_logits_processors at step {s} stream {b}"
            d = _mass_margin(lg, pre, tb) if opt.timestamps else float("-inf")
            # (one unmasked timestamp: its log-sum-exp is that logit itself in any summation order - decided, d == 0 included)
            undecided = opt.timestamps and np.isfinite(d) and abs(d) <= MASS_BAND and int((~pre[tb:]).sum()) != 1
            if undecided:
                accept = {_pick(lg, pre, opt, mass=False), int(np.argmax(np.where(pre | (np.arange(V) < tb), -np.inf, lg)))}
            else:
                assert _pick(lg, pre, opt) == expected, f"judge: float64 mass decision differs from the oracle's at step {s} stream {b} (d={d})"
                accept = {expected}
            if tok not in accept:
                status[s, b] = "wrong"
                v.wrong.append(dict(step=s, stream=b, expected=expected, got=tok, logit_expected=float(lg[expected]), logit_got=float(lg[tok]),
                                    got_masked=bool(pre[tok]), mass_margin=d, active=sorted(masks), tail=seq[-3:]))
                continue
            status[s, b] = "undecided" if undecided else "ok"
            if undecided:
                continue
            # ---- attribution: which rule, removed alone, changes the token ----
            if pre.all():
                v.decisive["all_masked"].append((s, b))
            for r, x in masks.items():
                rest = np.zeros(V, bool)
                for r2, x2 in masks.items():
                    if r2 != r:
                        rest |= x2
                if _pick(lg, rest, opt) != expected:
                    v.decisive[r].append((s, b))
            if opt.timestamps and _pick(lg, pre, opt, mass=False) != expected:
                v.decisive["mass"].append((s, b))
            # ---- ties: the maximum attained more than once; or attained by a masked lower id as well ----
            top = natural[expected]
            if np.isfinite(top):
                at = np.flatnonzero(natural == top)
                if len(at) > 1:
                    v.ties.append((s, b, tuple(int(i) for i in at)))
                lower = np.flatnonzero((lg[:expected] == lg[expected]) & pre[:expected])
                for j in lower:
                    v.masked_ties.append((s, b, int(j), expected))
    return v


# --------------------------------------------------------------------------------------------------------------------
# cases: one table for the CPU proof (the oracle's own run meets every condition) and for the replay of an engine's run on the GPU
# --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    V: int
    eos: int
    no_ts: int
    B: int = 6
    max_new: int = 70
    dtype: str = "f32"
    graph: bool = False
    timestamps: bool = True
    max_initial: Optional[int] = 50
    min_new: int = 0
    seed: int = 0
    pos_scale: float = 1.0
    eos_scale: float = 1.0
    no_ts_scale: float = 1.0
    ts_dir: float = 0.75
    gain: float = 1.0
    begin_suppress: str = "default"       # "default": (a text id, eos) as HF's (220, eos); "pick": what an unsuppressed call picks first
    suppress: str = "none"                # "none" | "picks": half of what the free run picks + bitmap word-edge ids | "all": every id | "one_ts"
    ties: bool = True                     # plant duplicate rows along the free run's path
    check_logits: bool = False            # also compare the replayed logits with the float64 restatement (strict f32: rel_l2 < 2e-5)
    expect: Tuple[str, ...] = ()          # rules that must be decisive in this case's run
    expect_ties: Tuple[str, ...] = ()     # kinds of planted ties that must occur at the maximum


@dataclass
class Built:
    case: Case
    dims: wo.WhisperDims
    weights: Dict[str, np.ndarray]
    prompt: np.ndarray
    opt: wo.GreedyOptions
    planted: Dict[str, List[Tuple[int, int]]]     # kind -> [(lower id, higher id)] duplicate rows
    kw: dict                                      # the same options as keyword arguments of WhisperEngine.generate_greedy


def sampler_chunk(V: int) -> int:
    return ((V + 63) // 64) * 2          # k_decode.hip: logits per vocabulary slice (32 slices per stream)


def case_prompt(c: Case) -> np.ndarray:
    """[B, 3]: two common tokens and a last one that differs per stream (text ids below eos, whatever the vocabulary)."""
    last = [(9 + 7 * b) % c.eos for b in range(c.B)]
    assert len(set(last)) == c.B
    return np.array([[3 % c.eos, 5 % c.eos, t] for t in last], dtype=np.int32)


def _options(c: Case, begin_suppress, suppress) -> wo.GreedyOptions:
    return wo.GreedyOptions(eos=c.eos, pad=c.eos, max_new_tokens=c.max_new, min_new_tokens=c.min_new, max_length=448,
                            begin_suppress=tuple(begin_suppress), suppress=tuple(suppress), timestamps=c.timestamps,
                            no_timestamps_id=c.no_ts, max_initial_timestamp_index=c.max_initial)


def _suppress_picks(c: Case, picked: Sequence[int]) -> List[int]:
    """Half of the text ids the free run picks, plus ids at the edges of the suppress bitmap's 32-bit words."""
    txt = [t for t in picked if t < c.eos]
    edges = (0, 31, 32, 63, 64, c.V - 1, (c.V - 1) & ~31, ((c.V - 1) & ~31) - 1)
    sup = txt[: max(1, len(txt) // 2)] + [i for i in edges if 0 <= i < c.V and i != c.eos]
    return list(dict.fromkeys(sup))


def _one_timestamp(c: Case, model: dict, prompt: np.ndarray, begin: List[int], free: np.ndarray):
    """(suppress list, duplicates, planted) of the "one_ts" case.  Every timestamp but the last two suppressed, V-2 := the row of the
    free run's first timestamp: the run opens with V-2, after which V-1 is the ONE unmasked timestamp: the mass rule compares a single
    logit, exactly.  V-1 := the row of a text token picked later makes text and timestamp maxima equal there: the merge of the two
    classes must return the text id (lower)."""
    sup = list(range(c.no_ts + 1, c.V - 2))
    dups = [(int(free[0, 3]), c.V - 2)]
    dims, w = crafted_model(c.V, c.eos, c.no_ts, dups=dups, **model)
    mid, _ = oracle_run(dims, w, prompt, _options(c, begin, sup))
    later = [int(t) for t in mid[0, 6:] if t < c.eos]
    dups.append((later[len(later) // 2], c.V - 1))
    return sup, dups, {"text_ts": [dups[-1]]}


def _plant_ties(c: Case, base: np.ndarray, prompt: np.ndarray, begin: List[int], sup: List[int]):
    """(duplicates, planted) along the path `base` of the un-duplicated model: each id on the path gets a copy at one of the distances
    below, kinds taken in turn, text ids and timestamp ids separately; the first text id also gets a copy whose LOWER id goes onto the
    suppress list `sup` (appended in place): that tie must go to the higher id."""
    tb = c.no_ts + 1 if c.timestamps else c.V
    text_hi = c.eos                                    # ordinary text ids: [0, eos)
    planted: Dict[str, List[Tuple[int, int]]] = {}
    dups: List[Tuple[int, int]] = []
    path = [int(t) for t in dict.fromkeys(base[:, 3:].T.ravel().tolist())]
    taken = set(base.ravel().tolist()) | set(prompt.ravel().tolist()) | {c.eos, c.no_ts} | set(sup) | set(begin)
    chunk = sampler_chunk(c.V)
    # distances between the two copies: the next id (the other element of a thread's pair where the lower id is even), the next lane,
    # another wavefront (scalar / vector path), another pass of the same thread, the next slice, a far slice
    offs = {"pair": 1, "lane": 2, "wave": 64, "wave2": 128, "pass": 512, "slice": chunk, "far": 5 * chunk + 3}

    def plant(kind, src, dst):
        if dst in taken or not (0 <= dst < c.V) or any(src in p or dst in p for p in dups):
            return False
        dups.append((src, dst))
        taken.add(dst)
        planted.setdefault(kind, []).append((src, dst))
        return True

    kinds = list(offs)
    texts = [t for t in path if t < text_hi]
    stamps = [t for t in path if t > c.no_ts] if c.timestamps else []
    if texts and c.suppress != "picks":
        for off in (chunk + 1, 3, 1):
            if texts[0] + off < text_hi and plant("masked_lower", texts[0], texts[0] + off):
                sup.append(texts[0])
                break
        texts = texts[1:]
    for grp, lo, hi in (("text", 0, text_hi), ("ts", tb, c.V)):
        toks = texts if grp == "text" else stamps
        k = 0
        for t in toks:
            for j in range(len(kinds)):
                kind = kinds[(k + j) % len(kinds)]
                if lo <= t + offs[kind] < hi and plant(f"{grp}_{kind}", t, t + offs[kind]):
                    k += j + 1
                    break
    return dups, planted


def build_case(c: Case) -> Built:
    """Model, prompt and options of a case.  Everything that depends on "what an unconstrained run picks" (suppress lists, duplicate
    rows) is derived from the numpy oracle's run of the un-duplicated model: deterministic, milliseconds."""
    model = dict(seed=c.seed, pos_scale=c.pos_scale, eos_scale=c.eos_scale, no_ts_scale=c.no_ts_scale, ts_dir=c.ts_dir, gain=c.gain, dtype=c.dtype)
    dims, w = crafted_model(c.V, c.eos, c.no_ts, **model)
    prompt = case_prompt(c)
    begin = [11 % c.eos, c.eos]
    sup: List[int] = []
    free, _ = oracle_run(dims, w, prompt, _options(c, begin, sup))
    if c.begin_suppress == "pick":
        begin = [c.eos] + [int(t) for t in dict.fromkeys(free[:, 3].tolist())][:2]
    if c.suppress == "all":
        sup = list(range(c.V))
    elif c.suppress == "picks":
        sup = _suppress_picks(c, [int(t) for t in dict.fromkeys(free[:, 3:].T.ravel().tolist())])      # in order of appearance, step-major
    planted: Dict[str, List[Tuple[int, int]]] = {}
    dups: List[Tuple[int, int]] = []
    if c.suppress == "one_ts":
        sup, dups, planted = _one_timestamp(c, model, prompt, begin, free)
    elif c.ties and c.suppress != "all":
        base, _ = oracle_run(dims, w, prompt, _options(c, begin, sup))
        dups, planted = _plant_ties(c, base, prompt, begin, sup)
    if dups:
        dims, w = crafted_model(c.V, c.eos, c.no_ts, dups=dups, **model)
    opt = _options(c, begin, sup)
    kw = dict(max_new_tokens=c.max_new, min_new_tokens=c.min_new, eos_id=c.eos, pad_id=c.eos, timestamps=c.timestamps,
              no_timestamps_id=c.no_ts, max_initial_timestamp_index=c.max_initial, begin_suppress=tuple(begin), suppress=tuple(sup))
    return Built(c, dims, w, prompt, opt, planted, kw)


def tie_kinds_seen(built: Built, v: Verdict) -> set:
    """Kinds of planted duplicates that occurred AT THE MAXIMUM of a judged step (for "masked_lower": with the lower id masked)."""
    pairs = v.tie_pairs()
    masked = {(lo, hi) for _, _, lo, hi in v.masked_ties}
    seen = set()
    for kind, lst in built.planted.items():
        if any((p in masked) if kind == "masked_lower" else (p in pairs) for p in lst):
            seen.add(kind)
    return seen


# vocabulary layouts: (V, eos, no_ts).  Real multilingual layout at 51865; small ones keep eos a little below no_ts as the real one does
REAL = (51865, 50257, 50363)
V66, V127, V1000A, V1000B = (66, 40, 47), (127, 90, 99), (1000, 700, 720), (1000, 700, 735)
V2047, V2048, V2049, V4097 = (2047, 1500, 1530), (2048, 1500, 1530), (2049, 1500, 1530), (4097, 3000, 3050)


def _c(name, layout, **kw) -> Case:
    return Case(name, *layout, **kw)


_TS7 = ("pair_ts_ts", "pair_ts_text", "mono_next", "mono_same", "mass", "no_ts", "suppress")
_HALF = ("pair_ts_ts", "mono_next", "mass", "no_ts")          # 16-bit engines: their logits, hence their path, differ from the float32 oracle's
_TIES_BIG = ("masked_lower", "text_pair", "text_lane", "text_wave", "text_wave2", "text_slice", "text_far", "ts_pair", "ts_lane")
_TIES_SMALL = ("masked_lower", "text_pair", "text_lane", "text_slice", "ts_pair", "ts_lane")
_M = dict(pos_scale=2.0, ts_dir=0.5, no_ts_scale=3.0)            # the setting in which the mass rule and both pairing forms decide steps
CASES: List[Case] = [
    # the real multilingual layout: V odd (scalar path of sampler_part_kernel), rows of odd streams not 8-byte aligned, N % 16 = 9
    _c("real-f32", REAL, B=3, check_logits=True, **_M, expect=_TS7 + ("max_initial",), expect_ties=_TIES_BIG),
    _c("real-f32-graph", REAL, B=3, graph=True, **_M, expect=_TS7 + ("max_initial",), expect_ties=_TIES_BIG),
    # small vocabularies with eos / no_ts inside them
    _c("v66", V66, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_SMALL),
    _c("v127", V127, B=1, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_SMALL),
    _c("v1000-ts-odd", V1000A, check_logits=True, **_M, expect=_TS7 + ("max_initial",), expect_ties=_TIES_BIG),
    _c("v1000-ts-slice-edge", V1000B, check_logits=True, **_M, expect=_TS7 + ("max_initial",), expect_ties=_TIES_BIG),
    _c("v2047", V2047, B=1, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    _c("v2048", V2048, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    _c("v2049", V2049, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    _c("v4097", V4097, B=1, check_logits=True, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    # the odd small vocabularies with six streams: rows of odd streams start at addresses that are not 8-byte aligned
    _c("v127-b6", V127, **_M, expect=_TS7, expect_ties=_TIES_SMALL),
    _c("v2047-b6", V2047, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    _c("v4097-b6", V4097, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    # timestamps off: ts_begin = V, every token is a text token
    _c("v127-no-timestamps", V127, timestamps=False, begin_suppress="pick", eos_scale=2.0, expect=("begin_suppress", "suppress", "pad_after_eos"), expect_ties=("masked_lower", "text_pair", "text_lane", "text_slice")),
    _c("v1000-no-timestamps", V1000A, timestamps=False, begin_suppress="pick", eos_scale=2.0, expect=("begin_suppress",), expect_ties=("text_pair", "text_lane", "text_slice")),
    # max_initial_timestamp_index: None, 0 (50 is every other case)
    _c("v1000-max-initial-none", V1000A, max_initial=None, gain=2.0, **_M, expect=_TS7, expect_ties=_TIES_BIG),
    _c("v1000-max-initial-0", V1000A, max_initial=0, gain=2.0, begin_suppress="pick", **_M, expect=("initial", "max_initial", "begin_suppress", "all_masked", "pair_ts_ts", "mass"), expect_ties=("text_pair", "text_lane", "ts_pair")),
    # min_new_tokens = max_new with a boosted eos
    _c("v1000-min-new", V1000A, max_new=60, min_new=60, eos_scale=4.0, **_M, expect=_TS7 + ("min_new",), expect_ties=_TIES_BIG),
    # suppress lists: the unconstrained picks + bitmap word edges; every id
    _c("v1000-suppress-picks", V1000A, suppress="picks", **_M, expect=("suppress", "pair_ts_ts", "mono_next", "mass", "no_ts"), expect_ties=("text_pair", "text_lane", "text_slice", "ts_pair")),
    _c("v66-suppress-all", V66, suppress="all", max_new=60, **_M, expect=("suppress", "all_masked"), expect_ties=()),
    # one unmasked timestamp: text / timestamp tie at the maximum
    _c("v1000-one-timestamp", V1000A, suppress="one_ts", max_initial=None, B=1, **_M, expect=("no_ts",), expect_ties=("text_ts",)),
    # 16-bit engines: judge only
    _c("v1000-bf16", V1000A, dtype="bf16", **_M, expect=_HALF, expect_ties=("text_pair", "text_lane", "ts_pair")),
    _c("v1000-f16", V1000A, dtype="f16", **_M, expect=_HALF, expect_ties=("text_pair", "text_lane", "ts_pair")),
    _c("real-bf16", REAL, B=3, dtype="bf16", **_M, expect=_HALF, expect_ties=("text_pair", "text_lane", "ts_pair")),
    _c("real-f16", REAL, B=3, dtype="f16", **_M, expect=_HALF, expect_ties=("text_pair", "text_lane", "ts_pair")),
    # more streams than wavefronts of sampler_finish_kernel: streams w, w + 16, w + 32 share a wavefront and finish at different steps
    _c("v1000-b33", V1000A, B=33, eos_scale=2.5, ts_dir=1.0, expect=("pair_ts_ts", "mono_next", "mono_same", "max_initial", "mass", "pad_after_eos"), expect_ties=("masked_lower", "text_pair", "text_wave", "text_slice", "ts_pair", "ts_slice")),
    _c("v1000-b64", V1000A, B=64, eos_scale=2.5, ts_dir=1.0, expect=("pair_ts_ts", "mono_next", "mono_same", "max_initial", "mass", "pad_after_eos"), expect_ties=("masked_lower", "text_pair", "text_wave", "text_slice", "ts_pair", "ts_slice")),
]


def case_by_name(name: str) -> Case:
    return next(c for c in CASES if c.name == name)


def forced_after_open_timestamp(seqs: np.ndarray, n_begin: int, no_ts: int) -> int:
    """n_forced such that stream 0's forced prefix ends in a timestamp that opens a pair (a text token before it), the generation
    continues with the closing timestamp and then a text token: the call has to seed the last timestamp from the forced tokens."""
    r = seqs[0]
    for i in range(n_begin + 2, len(r) - 2):
        if r[i - 1] <= no_ts and r[i] > no_ts and r[i + 1] > no_ts and r[i + 2] <= no_ts:
            return i + 1 - n_begin
    raise AssertionError("no text, timestamp, timestamp, text run in stream 0")
