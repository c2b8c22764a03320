"""A one-layer micro decoder whose self-attention POINTS: every query puts (to 1e-6) all its probability on one key the test chooses.
No GPU in here.

Why: with `make_weights` the decoder's self-attention is near-uniform, so a key that the kernel drops, or reads from the neighbouring
slot, moves a deep position's logits by 2.5e-3 relative L2 (median) - inside the bf16 tolerance of 3e-2 and below bf16 rounding itself.
Sharpening the random weights (q_proj x 8, x 32) does not help: near-ties between two keys amplify the rounding of the scores.  A saturated
pointer has neither problem: rounding cannot move probability 1, and one wrong key replaces the whole attended value.

Construction on `dims_variant("micro", enc_layers=1, dec_layers=1, max_target_positions=P)` and `make_weights(dims, 2)`; d_model = 128 is
two heads of 64, written [first half | second half] below, and c(i) is row i of a seeded table of P codes of 64 entries +-1:

    embed_positions[p] = [A c(p) | 0]          embed_tokens[id]  = [0 | A c(id)]   for id < P (the other rows keep their values)
    self_attn_layer_norm: gain 1, bias 0       k_proj.weight     = [[I, 0], [I, 0]]
    q_proj.bias = 0                            q_proj.weight     = BETA [[0, I], [I, 0]]

so the key at position k is (LayerNorm of) c(k) in both heads, head 0's query at position p is BETA c(ids[p]) and head 1's is BETA c(p):
head 0 attends to the key whose POSITION is the token id fed at p (any id <= p), head 1 to the query's own position - the newest key,
written in the same step, at the edge of the kernel's `t < n_keys` mask.  The matched score is BETA * 64 / 8 = 32 against about +-4 for
any other key.  Identity and power-of-two weights are exact in every element type; v_proj, out_proj and everything behind them keep
their seeded values, so the attended value is an ordinary random vector.  tests/test_pointer_model.py checks, on the oracle, everything
the GPU cases (tests/test_gpu_deep.py) rely on: saturation, which keys are pointed at from where, and that hiding or displacing one
pointed-at key moves the logits by far more than the reduced-precision tolerances.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests.util import clips, dims_variant

A = 0.5
BETA = 4.0
T = 100
HALF = 64
GROUP = 64          # keys per wavefront pass of attn_mfma_block
PATTERNS = ("previous", "key 0", "first of own group", "last of group before", "p-63", "p-64", "uniform a", "uniform b", "boundary cycle")
_LAYER = "model.decoder.layers.0"


def boundaries(P: int) -> List[int]:
    """BND: the keys on either side of every 16-, 32- and 64-key edge of the fragment arithmetic, and the last key a later query can see."""
    return sorted({k for k in (0, 1, 15, 16, 31, 32, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 319, 320, 383, 384, P - 2) if 0 <= k < P})


def pattern_ids(P: int, seed: int = 0) -> np.ndarray:
    """int32 [len(PATTERNS), P], ids[b, p] <= p: the key (= token id) head 0 of stream b's query at position p points at."""
    p = np.arange(P)
    rng = np.random.default_rng([seed, P])
    bnd = np.array(boundaries(P))
    cycle, j = np.zeros(P, np.int64), 0
    for q in range(P):                       # the next member of BND, wrapping behind the last one that is <= q
        j = (j + 1) % int((bnd <= q).sum())
        cycle[q] = bnd[j]
    rows = [np.maximum(p - 1, 0), np.zeros(P, np.int64), p // GROUP * GROUP, np.maximum(p // GROUP * GROUP - 1, 0), np.maximum(p - 63, 0),
            np.maximum(p - 64, 0), rng.integers(0, p + 1), rng.integers(0, p + 1), cycle]
    ids = np.stack(rows).astype(np.int32)
    assert ids.shape == (len(PATTERNS), P) and (ids <= p).all() and (ids >= 0).all()
    return ids


def pointer_weights(P: int, seed: int = 0) -> Tuple[wo.WhisperDims, Dict[str, np.ndarray]]:
    dims = dims_variant("micro", enc_layers=1, dec_layers=1, max_target_positions=P)
    assert dims.d_model == 2 * HALF and dims.heads == 2 and P <= dims.vocab
    w = dict(wo.make_weights(dims, 2))
    code = np.random.default_rng([seed, P, 1]).integers(0, 2, size=(P, HALF)).astype(np.float32) * 2 - 1
    zero, eye = np.zeros((P, HALF), np.float32), np.eye(HALF, dtype=np.float32)
    o = np.zeros((HALF, HALF), np.float32)
    w["model.decoder.embed_positions.weight"] = np.concatenate([A * code, zero], axis=1)
    tok = w["model.decoder.embed_tokens.weight"].copy()
    tok[:P] = np.concatenate([zero, A * code], axis=1)
    w["model.decoder.embed_tokens.weight"] = tok
    w[_LAYER + ".self_attn_layer_norm.weight"] = np.ones(2 * HALF, np.float32)
    w[_LAYER + ".self_attn_layer_norm.bias"] = np.zeros(2 * HALF, np.float32)
    w[_LAYER + ".self_attn.k_proj.weight"] = np.block([[eye, o], [eye, o]])
    w[_LAYER + ".self_attn.q_proj.weight"] = np.float32(BETA) * np.block([[o, eye], [eye, o]])
    w[_LAYER + ".self_attn.q_proj.bias"] = np.zeros(2 * HALF, np.float32)
    return dims, w


@dataclasses.dataclass(frozen=True)
class Built:
    """Shared between tests: read only."""
    dims: wo.WhisperDims
    weights: Dict[str, np.ndarray]
    ids: np.ndarray        # int32 [B, P]
    mel: np.ndarray        # float32 [B, n_mels, 2 T]
    logits: np.ndarray     # float32 [B, P, V]: OracleWhisper.decode over all positions at once


def oracle_logits(dims, weights, ids, mel, dtype=np.float32) -> np.ndarray:
    om = wo.OracleWhisper(dims, weights, T=T, dtype=dtype)
    return om.decode(ids, om.new_cache(om.encode(mel)))[0]


@functools.lru_cache(maxsize=1)
def build(P: int, B: int = len(PATTERNS)) -> Built:
    """The pointer model at P positions with B streams: the patterns, repeated from the first where B > len(PATTERNS), each stream on a clip
    of its own.  (One entry is kept: [B, P, 51866] float32 is 0.8 GB at P = 448.)"""
    dims, w = pointer_weights(P)
    ids = np.ascontiguousarray(np.resize(pattern_ids(P), (B, P)))
    mel = wo.log_mel(clips(T * 320, B), dims.n_mels)
    return Built(dims, w, ids, mel, oracle_logits(dims, w, ids, mel))


def targets(ids: np.ndarray) -> np.ndarray:
    """int [B, P, 2]: the key each head of each query points at."""
    B, P = ids.shape
    return np.stack([ids.astype(np.int64), np.broadcast_to(np.arange(P), (B, P))], axis=-1)


# ---- the score hook: OracleWhisper.decode restated for all positions at once, with a function applied to the self-attention scores ------
Hook = Callable[[np.ndarray], np.ndarray]      # [B, H, P, P] scores with -inf above the diagonal -> the same


def hide_key(k: int) -> Hook:
    """Key k is invisible to every LATER query (its own query still sees it): what a kernel that skips the slot would compute."""
    def f(s):
        s = s.copy()
        s[:, :, k + 1:, k] = -np.inf
        return s
    return f


def swap_with_next(k: int) -> Hook:
    """Every query behind k sees key k's score at k + 1 and the reverse: what a kernel that pairs scores with the neighbouring value slot would compute."""
    def f(s):
        s = s.copy()
        s[:, :, k + 1:, [k, k + 1]] = s[:, :, k + 1:, [k + 1, k]]
        return s
    return f


def decode_hooked(om: wo.OracleWhisper, ids: np.ndarray, enc: np.ndarray, hook: Optional[Hook] = None):
    """(hidden [B, P, d] in front of the final LayerNorm, self-attention probabilities [B, H, P, P] of the last layer): the arithmetic of
    `OracleWhisper.decode` on an empty cache, operation for operation, with `hook` applied to the masked scores of every layer."""
    w, dims = om.w, om.dims
    B, n = ids.shape
    d = "model.decoder"
    scale = om.dtype(dims.head_dim ** -0.5)
    x = w[d + ".embed_tokens.weight"][ids] + w[d + ".embed_positions.weight"][:n][None]
    causal = np.triu(np.full((n, n), -np.inf, dtype=om.dtype), k=1)
    probs = None
    for i in range(dims.dec_layers):
        p = f"{d}.layers.{i}"
        h = om._ln(x, p + ".self_attn_layer_norm")
        q = om._heads(om._lin(h, p + ".self_attn.q_proj") * scale)
        k = om._heads(om._lin(h, p + ".self_attn.k_proj", bias=False))
        v = om._heads(om._lin(h, p + ".self_attn.v_proj"))
        s = q @ k.transpose(0, 1, 3, 2) + causal[None, None]
        if hook is not None:
            s = hook(s)
        probs = wo.softmax(s)
        x = x + om._lin(om._merge(probs @ v), p + ".self_attn.out_proj")
        h = om._ln(x, p + ".encoder_attn_layer_norm")
        q = om._heads(om._lin(h, p + ".encoder_attn.q_proj") * scale)
        ck = om._heads(om._lin(enc, p + ".encoder_attn.k_proj", bias=False))
        cv = om._heads(om._lin(enc, p + ".encoder_attn.v_proj"))
        x = x + om._lin(om._merge(wo.softmax(q @ ck.transpose(0, 1, 3, 2)) @ cv), p + ".encoder_attn.out_proj")
        h = wo.gelu(om._lin(om._ln(x, p + ".final_layer_norm"), p + ".fc1"))
        x = (x + om._lin(h, p + ".fc2")).astype(om.dtype)
    return x, probs


def logits_of(om: wo.OracleWhisper, hidden: np.ndarray) -> np.ndarray:
    """The final LayerNorm and the tied projection on any selection of rows of `decode_hooked`'s hidden state."""
    return om._dec_logits(hidden)
