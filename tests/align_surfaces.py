"""Chosen alignment surfaces for the word-timestamp kernels (k_dtw.hip: align_zscore_kernel, align_median_mean_kernel, dtw_kernel),
restatements of what those kernels compute, and the judge the GPU tests use.  No GPU and no torch in here.

The alignment rows normally come out of a decoder, so tests/test_gpu_parity.py only ever sees the diffuse, tie-free surfaces of a
randomly initialised model.  `WhisperEngine.set_alignment` puts a surface of our choosing into the recorded-alignment buffer; this
module makes such surfaces:

  * EXACT surfaces.  For every head and column the N generated rows hold a + d*s_i: `a` a multiple of 1/64, `d` a power of two, `s` a
    placement of an integer pattern with sum(s) = 0 and sum(s^2)/N a perfect square (PATTERNS).  Sum, mean, centred values, variance,
    sd and z-score are then exact in float32 whatever the summation order (every partial sum is an integer multiple of 2^-9 below
    2^9, resp. of 2^-18 below 2^-1), the z-scores are multiples of 1/2 of magnitude <= 2.5, the median is a selection and the head
    mean is one rounding of an exact sum: the engine and the oracle must produce the SAME matrix, bit for bit, and - the matrix being
    full of equal values - a DTW full of ties.  Timestamps are compared with np.array_equal.
  * ZERO-VARIANCE variants: columns whose N rows all hold one dyadic constant.  Mean exact, sd = 0, z = 0/0 = NaN in every row.  The
    reference sorts NaN last (torch.sort / np.sort), so one NaN drops out of its neighbours' windows and four or more make the
    median NaN, which then reaches the DTW (every comparison false: "left").  N = 1 makes every column such a column.
  * GENERIC surfaces: softmax rows of a noisy diagonal band.  Not exact; judged with the margin rule of tests/util.py under an eps
    derived from the reference's own float32 rounding (`delta_eps`).

`mirror_timestamps` restates the kernels' own order of operations (serial float32 sums over rows, fma in the variance, the 16
compare-exchange network, serial sum over heads, anti-diagonal DTW, back-trace by one walker) with switches that turn it into the
WRONG pipelines of WRONG_MIRRORS; tests/test_align_surfaces.py proves that the judge rejects each of them on the listed cases.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests.util import alignment_matrix, dtw_jump_margins

TIME_PRECISION = 0.02
F32 = np.float32

# name -> the integer pattern (tiled N / len times).  sum = 0; sum of squares / length = 1, 4, 4: sd = 1, 2, 2
PATTERNS: Dict[str, Tuple[int, ...]] = {
    "pm1": (1, -1),                                   # z = +-1
    "z2": (4, -4, 0, 0, 0, 0, 0, 0),                  # z in {0, +-2}
    "half": (5, -5) + (1, -1) * 7,                    # z in {+-0.5, +-2.5}
}


def patterns_for(N: int) -> Tuple[str, ...]:
    return tuple(p for p, v in PATTERNS.items() if N % len(v) == 0)


# --------------------------------------------------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One stream's problem: N generated rows behind n_prompt prompt rows, M kept columns of T, Ha heads."""
    name: str
    Ha: int
    N: int
    M: int
    T: int = 300
    n_prompt: int = 3
    num_frames: Optional[int] = None        # the bound handed to the engine; None: 2 * M
    kind: str = "exact"                     # exact | diffuse | peaky
    placement: str = "random"               # random | banded
    seed: int = 0
    const: Tuple[Tuple[Optional[int], Tuple[int, ...], float], ...] = ()   # (head or None = all, columns, value)

    @property
    def n_rows(self) -> int:
        return self.n_prompt + self.N

    @property
    def seq_len(self) -> int:
        return self.n_rows + 1

    @property
    def frames(self) -> int:
        return 2 * self.M if self.num_frames is None else self.num_frames

    @property
    def exact(self) -> bool:
        return self.kind == "exact"


def engine_columns(num_frames: int, T: int) -> int:
    """The columns tw_token_timestamps keeps for one bound: the Python slice [: num_frames // 2] on T columns."""
    k = num_frames // 2
    return min(T, k) if k >= 0 else max(0, T + k)


def _exact(Ha: int, N: int, T: int, M: int, seed: int, placement: str) -> np.ndarray:
    names = patterns_for(N)
    assert names or N == 1, f"no exact pattern divides N = {N}"
    rng = np.random.default_rng(seed)
    out = np.empty((Ha, N, T), dtype=np.float64)
    rows = np.arange(N)
    for h in range(Ha):
        for j in range(T):
            # N = 1: the one row IS the column mean, whatever it holds; z = 0/0
            s = np.array(PATTERNS[names[rng.integers(len(names))]] if names else (0,), dtype=np.int64)
            s = np.tile(s, N // len(s))
            a = rng.integers(8, 41) / 64.0
            d = 2.0 ** -int(rng.integers(7, 10))
            if placement == "random":
                s = rng.permutation(s)
            else:
                # banded: the largest values go to the rows nearest j * N / M (as speech aligns), with some jitter
                centre = (j % max(M, 1)) * N / max(M, 1)
                order = np.argsort(np.abs(rows - centre) + rng.normal(0.0, 1.0 + N / 16.0, N), kind="stable")
                placed = np.empty(N, dtype=np.int64)
                placed[order] = np.sort(s)[::-1]
                s = placed
            out[h, :, j] = a + d * s
    got = out.astype(F32)
    assert np.array_equal(got.astype(np.float64), out)       # every value is a float32
    return got


def _generic(Ha: int, N: int, T: int, seed: int, peaky: bool) -> np.ndarray:
    rng = np.random.default_rng(seed)
    j = np.arange(T)[None, None, :]
    centre = ((np.arange(N)[None, :, None] + 0.5) / N) * T * 0.9 + rng.normal(0.0, 3.0, (Ha, 1, 1))
    width = 4.0 if peaky else T / 6.0
    logits = -0.5 * ((j - centre) / width) ** 2
    logits = np.maximum(logits, -30.0) + rng.normal(0.0, 1.0 if peaky else 0.5, (Ha, N, T))   # floor: no column underflows to 0
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(F32)


@functools.lru_cache(maxsize=None)
def _surface(case: Case) -> np.ndarray:
    if case.exact:
        s = _exact(case.Ha, case.N, case.T, case.M, case.seed, case.placement)
    else:
        s = _generic(case.Ha, case.N, case.T, case.seed, case.kind == "peaky")
    for head, cols, value in case.const:
        assert float(F32(value)) == value and value * 1024 == int(value * 1024)      # dyadic: the column mean is exact
        for c in cols:
            s[slice(None) if head is None else head, :, c % max(case.M, 1)] = value
    buf = np.full((case.Ha, case.n_rows, case.T), F32(1.0 / case.T), dtype=F32)      # prompt rows: a flat softmax row
    buf[:, case.n_prompt:] = s
    buf.setflags(write=False)
    return buf


def surface(case: Case) -> np.ndarray:
    """float32 [Ha, n_rows, T], read-only and cached: what the decoder would have recorded for this stream."""
    return _surface(case)


def poisoned(case: Case, extra_rows: int = 2) -> np.ndarray:
    """surface(case) with everything the reference crops away made hostile: prompt rows NaN, columns >= M 1e30 / NaN alternating,
    `extra_rows` rows behind n_rows NaN.  The oracle never looks at those cells, so the engine's result must not move."""
    src = surface(case)
    buf = np.full((case.Ha, case.n_rows + extra_rows, case.T), np.nan, dtype=F32)
    buf[:, case.n_prompt:case.n_rows, :case.M] = src[:, case.n_prompt:, :case.M]
    tail = buf[:, case.n_prompt:case.n_rows, case.M:]
    tail[..., ::2] = F32(1e30)
    return buf


# --------------------------------------------------------------------------------------------------------------------
# the reference, and what it costs in float32
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_timestamps(case: Case) -> np.ndarray:
    """float32 [n_rows + 1]: oracle.whisper_oracle.token_timestamps on the case's surface with its M columns.  Cached, read-only."""
    ts = wo.token_timestamps(surface(case)[None], case.n_prompt, None, columns=[case.M])[0]
    ts.setflags(write=False)
    return ts


def oracle_matrix(case: Case) -> np.ndarray:
    """The reference's float32 [N, M] matrix (its DTW runs on the negation)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return alignment_matrix(surface(case), case.n_prompt, case.M)


def matrix64(case: Case) -> np.ndarray:
    """The same steps evaluated in float64 on the float32 surface."""
    w = surface(case)[:, case.n_prompt:, :case.M].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = (w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)
    return wo.median_filter(w, 7).mean(axis=0)


def delta_eps(case: Case) -> Tuple[float, float]:
    """(delta, eps) of a generic case.  delta = max |float32 reference matrix - float64 evaluation|: the float32 rounding the
    reference itself carries, which any other summation order may carry differently.  A monotone path visits at most N + M cells, two
    paths are compared, and either side may be off by delta per cell in either direction: eps = 4 * (N + M) * delta."""
    delta = float(np.abs(oracle_matrix(case).astype(np.float64) - matrix64(case)).max())
    return delta, 4.0 * (case.N + case.M) * delta


# --------------------------------------------------------------------------------------------------------------------
# the kernels' order of operations, with switches for the wrong pipelines
# --------------------------------------------------------------------------------------------------------------------
_NETWORK = ((0, 6), (2, 3), (4, 5), (0, 2), (1, 4), (3, 6), (0, 1), (2, 5), (3, 4), (1, 2), (4, 6), (2, 3), (4, 5), (1, 2), (3, 4),
            (5, 6))


def _median7(win: List[np.ndarray], rule: str) -> np.ndarray:
    """align_median_mean_kernel's 16 compare-exchanges on seven arrays.  rule 'nanlast': exchange when x is NaN or y < x (NaN sorts
    last, as torch.sort and np.sort order it); 'fminmax': lo = fminf(x, y), hi = fmaxf(x, y), which DROP a NaN operand."""
    w = list(win)
    for p, q in _NETWORK:
        x, y = w[p], w[q]
        if rule == "nanlast":
            swap = (x != x) | (y < x)
            w[p], w[q] = np.where(swap, y, x), np.where(swap, x, y)
        else:
            assert rule == "fminmax", rule
            w[p], w[q] = np.fmin(x, y), np.fmax(x, y)
    return w[3]


def mirror_matrix(w: np.ndarray, ddof: int = 0, median: str = "nanlast", pad: str = "reflect", filter_short: bool = False) -> np.ndarray:
    """w: float32 [Ha, N, M] (cropped, prompt rows dropped) -> float32 [N, M] in the kernels' order."""
    Ha, N, M = w.shape
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.zeros((Ha, M), dtype=F32)
        for i in range(N):
            s = s + w[:, i]
        mean = s / F32(N)
        q = np.zeros((Ha, M), dtype=F32)
        for i in range(N):
            c = (w[:, i] - mean).astype(np.float64)
            q = (q.astype(np.float64) + c * c).astype(F32)              # fma: one rounding per step
        sd = np.sqrt(q / F32(N - ddof))
        z = (w - mean[:, None, :]) / sd[:, None, :]
        if M <= 3 and not filter_short:
            f = z
        else:
            win = []
            for k in range(7):
                jj = np.arange(M) + k - 3
                if pad == "zero":
                    inside = (jj >= 0) & (jj < M)
                    win.append(np.where(inside, z[..., np.clip(jj, 0, M - 1)], F32(0)))
                    continue
                assert pad == "reflect", pad
                if M == 1:
                    jj = np.zeros_like(jj)
                else:
                    jj = np.mod(jj, 2 * (M - 1))
                    jj = np.where(jj >= M, 2 * (M - 1) - jj, jj)
                win.append(z[..., jj])
            f = _median7(win, median)
        acc = np.zeros((N, M), dtype=F32)
        for h in range(Ha):
            acc = acc + f[h]
        return acc / F32(Ha)


def mirror_dtw(mat: np.ndarray, tie: str = "strict") -> np.ndarray:
    """dtw_kernel: anti-diagonal sweep of the float32 cost table on -mat, then the back-trace.  Returns the frame at which each of the
    N tokens starts.  tie 'strict' is HF's rule (diagonal if c0 < c1 and c0 < c2, else up if c1 < c0 and c1 < c2, else LEFT - so every
    tie that involves the minimum goes left); 'nonstrict' is the arg-min with diagonal, up, left priority; 'up_first' the arg-min with
    up, diagonal, left priority."""
    N, M = mat.shape
    neg = -mat.astype(np.float64)
    cost = np.full((N + 1, M + 1), np.inf, dtype=F32)
    cost[0, 0] = 0
    trace = np.full((N + 1, M + 1), 2, dtype=np.int8)
    with np.errstate(invalid="ignore"):
        for k in range(2, N + M + 1):
            i = np.arange(max(1, k - M), min(N, k - 1) + 1)
            j = k - i
            c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
            if tie == "strict":
                dg = (c0 < c1) & (c0 < c2)
                up = ~dg & (c1 < c0) & (c1 < c2)
            elif tie == "nonstrict":
                dg = (c0 <= c1) & (c0 <= c2)
                up = ~dg & (c1 <= c0) & (c1 <= c2)
            else:
                assert tie == "up_first", tie
                up = (c1 <= c0) & (c1 <= c2)
                dg = ~up & (c0 <= c1) & (c0 <= c2)
            cm = np.where(dg, c0, np.where(up, c1, c2))
            cost[i, j] = (neg[i - 1, j - 1] + cm.astype(np.float64)).astype(F32)
            trace[i, j] = np.where(dg, 0, np.where(up, 1, 2))
    jump = np.zeros(N, dtype=np.int64)
    i, j = N, M
    while i > 0 or j > 0:
        if i > 0:
            jump[i - 1] = j - 1
        t = 2 if i == 0 else 1 if j == 0 else trace[i, j]
        if t == 0:
            i -= 1
            j -= 1
        elif t == 1:
            i -= 1
        else:
            j -= 1
    return jump


def mirror_timestamps(buf: np.ndarray, n_prompt: int, cols: int, tie: str = "strict", ddof: int = 0, median: str = "nanlast",
                      pad: str = "reflect", filter_short: bool = False, crop_shift: int = 0, dup_last: bool = True) -> np.ndarray:
    """float32 [n_rows + 1] from one stream's buffer [Ha, n_rows, T]: tw_token_timestamps restated (all defaults), or one of the wrong
    pipelines."""
    buf = np.asarray(buf, dtype=F32)
    n_rows, T = buf.shape[1], buf.shape[2]
    N = n_rows - n_prompt
    M = min(max(cols + crop_shift, 0), T)
    ts = np.zeros(n_rows + 1, dtype=F32)
    if M == 0:
        jump = np.full(N, -1, dtype=np.int64)
    else:
        mat = mirror_matrix(buf[:, n_prompt:, :M], ddof=ddof, median=median, pad=pad, filter_short=filter_short)
        jump = mirror_dtw(mat, tie)
    ts[n_prompt:n_rows] = (jump * TIME_PRECISION).astype(F32)
    ts[n_rows] = ts[n_rows - 1] if dup_last else 0
    return ts


def mirror(case: Case, **wrong) -> np.ndarray:
    return mirror_timestamps(surface(case), case.n_prompt, engine_columns(case.frames, case.T), **wrong)


# the pipelines the judge has to reject (tests/test_align_surfaces.py::test_the_judge_rejects_every_wrong_mirror)
WRONG_MIRRORS: Dict[str, dict] = {
    "non-strict tie-break": dict(tie="nonstrict"),
    "up before diagonal": dict(tie="up_first"),
    "fmin/fmax median network": dict(median="fminmax"),
    "sample std (N - 1)": dict(ddof=1),
    "zero padding instead of reflect": dict(pad="zero"),
    "median applied when M <= 3": dict(filter_short=True),
    "crop off by one column": dict(crop_shift=1),
    "last token not duplicated": dict(dup_last=False),
}


# --------------------------------------------------------------------------------------------------------------------
# the judge
# --------------------------------------------------------------------------------------------------------------------
@dataclass
class Verdict:
    ok: bool
    differing: int = 0       # generated tokens whose timestamp is not the reference's
    excused: int = 0         # of those, the ones within eps of the reference's optimum (generic cases only)
    detail: str = ""

    def __bool__(self) -> bool:
        return self.ok


MAX_EXCUSED = 0.02           # of a generic case's tokens


def judge(case: Case, ts: np.ndarray) -> Verdict:
    """Is `ts` (float32 [n_rows + 1]) what the reference computes for `case`?  Exact, zero-variance and N = 1 cases: np.array_equal
    with the oracle's timestamps, nothing else.  Generic cases: equal, or every generated token that differs lies on a path that
    costs at most eps more than the reference's optimum on the REFERENCE's matrix (tests.util.dtw_jump_margins, eps from delta_eps),
    at most MAX_EXCUSED of the tokens do, and everything that is not a generated token's own time is exactly right."""
    want = oracle_timestamps(case)
    ts = np.asarray(ts)
    if ts.shape != want.shape or ts.dtype != want.dtype:
        return Verdict(False, detail=f"{case.name}: shape/dtype {ts.shape} {ts.dtype}, want {want.shape} {want.dtype}")
    if np.array_equal(ts, want):
        return Verdict(True)
    diff = np.flatnonzero(ts != want)
    where = f"{case.name}: {diff.size} entries differ, first at {diff[0]}: got {ts[diff[0]]!r}, want {want[diff[0]]!r}"
    if case.exact or case.M == 0:
        return Verdict(False, differing=int(diff.size), detail=where)
    p, n = case.n_prompt, case.n_rows
    if (ts[:p] != 0).any() or ts[n] != ts[n - 1]:
        return Verdict(False, differing=int(diff.size), detail=where + " (prompt entries / duplicate of the last token)")
    frames = np.rint(ts[p:n].astype(np.float64) / TIME_PRECISION).astype(np.int64)
    if not np.array_equal((frames * TIME_PRECISION).astype(F32), ts[p:n]) or frames.min() < 0 or frames.max() >= case.M \
            or (np.diff(frames) < 0).any() or frames[0] != 0:
        return Verdict(False, differing=int(diff.size), detail=where + " (not the start frames of a monotone path)")
    _, eps = delta_eps(case)
    margins, _ = dtw_jump_margins(oracle_matrix(case), frames)
    moved = ts[p:n] != want[p:n]
    beyond = moved & ~(margins <= eps)
    if beyond.any():
        k = int(np.flatnonzero(beyond)[0])
        return Verdict(False, differing=int(moved.sum()), detail=where + f"; token {k}: margin {margins[k]:.3e} > eps {eps:.3e}")
    excused = int(moved.sum())
    if excused > MAX_EXCUSED * case.N:
        return Verdict(False, differing=excused, excused=excused, detail=where + f"; {excused} of {case.N} tokens within eps: more than 2 %")
    return Verdict(True, differing=excused, excused=excused, detail=where + f"; all within eps {eps:.3e}")


# --------------------------------------------------------------------------------------------------------------------
# the case lists of tests/test_gpu_align.py (tests/test_align_surfaces.py proves their exactness and their power on the CPU)
# --------------------------------------------------------------------------------------------------------------------
M_SWEEP = [Case(f"m{M}{'+' if odd else ''}", Ha=2, N=16, M=M, num_frames=2 * M + odd, seed=100 + M, placement=("random", "banded")[M % 2])
           for M in (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 300) for odd in (0, 1)]
N_SWEEP = [Case(f"n{N}", Ha=2, N=N, M=64, seed=200 + N, placement=("random", "banded")[(N // 2) % 2])
           for N in (2, 62, 64, 66, 126, 128, 444)]
HEADS = [Case(f"h{Ha}_{pl}", Ha=Ha, N=48, M=257, seed=300 + Ha, placement=pl) for Ha in (1, 2, 6, 10) for pl in ("random", "banded")]
# the largest problem of the path: 444 tokens x 1500 frames; the second stream under a negative (odd) bound that keeps 1100 columns
LARGEST = [Case("big_all", Ha=2, N=444, M=1500, T=1500, seed=400, placement="banded"),
           Case("big_negative", Ha=2, N=444, M=1100, T=1500, num_frames=-799, seed=401)]
PROMPTS = [Case(f"prompt{p}", Ha=2, N=32, M=100, n_prompt=p, seed=500 + p, placement="banded") for p in (1, 3, 8)]
# one call, three streams: no column kept / 5 / all of them
BATCH = [Case("batch_none", Ha=2, N=32, M=0, num_frames=-700, seed=600), Case("batch_5", Ha=2, N=32, M=5, seed=601, placement="banded"),
         Case("batch_all", Ha=2, N=32, M=300, num_frames=640, seed=602, placement="banded")]
SMALL_AFTER_LARGEST = Case("stale", Ha=2, N=16, M=40, T=1500, seed=700, placement="banded")
ZERO_VARIANCE = [
    Case("zv_one_head", Ha=2, N=32, M=40, seed=800, placement="banded", const=((0, (17,), 0.0),)),
    Case("zv_all_heads", Ha=2, N=32, M=40, seed=801, placement="banded", const=((None, (17,), 0.25),)),
    Case("zv_edges", Ha=2, N=32, M=40, seed=802, placement="banded", const=((None, (0, 39), 0.0), (1, (2, 36), 0.5))),
    Case("zv_run5", Ha=2, N=32, M=40, seed=803, placement="banded", const=((None, (20, 21, 22, 23, 24), 0.0),)),
    Case("zv_run5_random", Ha=2, N=16, M=9, seed=804, const=((None, (2, 3, 4, 5, 6), 0.125),)),
    Case("zv_six_heads", Ha=6, N=48, M=65, seed=805, placement="banded", const=((3, (30,), 0.0), (None, (7, 64), 0.0))),
    Case("n1", Ha=2, N=1, M=40, seed=806), Case("n1_m3", Ha=2, N=1, M=3, seed=807), Case("n1_prompt8", Ha=1, N=1, M=257, n_prompt=8, seed=808),
]
GENERIC = [
    Case("diffuse_h2", Ha=2, N=48, M=300, kind="diffuse", seed=900), Case("peaky_h2", Ha=2, N=64, M=257, kind="peaky", seed=901),
    Case("diffuse_h6", Ha=6, N=30, M=200, kind="diffuse", seed=902), Case("peaky_h6", Ha=6, N=100, M=300, kind="peaky", seed=903),
    Case("peaky_h2_short", Ha=2, N=17, M=65, kind="peaky", seed=904),
]
EXACT_CASES: Sequence[Case] = [*M_SWEEP, *N_SWEEP, *HEADS, *LARGEST, *PROMPTS, *BATCH, SMALL_AFTER_LARGEST, *ZERO_VARIANCE]
