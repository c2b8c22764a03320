"""A micro model (1 + 1 layers) whose decoder CROSS-attention points: every query puts all its probability (to float32) on one encoder
frame the test chooses.  No GPU in here; sibling of tests/pointer_model.py, which does the same for the self-attention.

Why: with `make_weights` cross-attention is near-uniform over 500 to 1500 frames, so a key that the kernel drops, reads from the
neighbouring slot, or pairs with the wrong value or scale byte moves a query's logits by about 1 / T - far inside the reduced-precision
tolerances (tests/test_cross_pointer_model.py measures it).  Under a saturated pointer one wrong key replaces the whole attended value.

Construction on `dims_variant("micro", enc_layers=1, dec_layers=1, max_source_positions=T, max_target_positions=P)` and
`make_weights(dims, 2)`; d_model = 128 is two heads of 64, written [first half | second half], and c(t) is row t of a seeded table of T
BALANCED codes of 64 entries +-1 (32 of each sign: a constant shift of a key cancels in the score) with pairwise dot products <= 24:

    encoder   embed_positions[t] = [A c(t) | 0]; conv2 output channels 0..63 zeroed (the code half is exact, the other half carries the
              stream's audio); layer 0's self_attn.out_proj and fc2 zero (the layer is the identity); final layer_norm gain 1, bias 0
    cross     encoder_attn.k_proj = [[I, 0], [I, 0]], q_proj = BETA [[0, I], [I, 0]] with zero bias, encoder_attn_layer_norm gain 1, bias 0
    decoder   self_attn.out_proj zero (x in front of the cross-attention is the embedding, exactly);
              embed_tokens[id] = [0 | A c(id)] for id < T, embed_positions[p] = [A c(g(p)) | 0]

so the key of frame t is (the frame's LayerNorm of) c(t) in both heads, head 0's query at position p is BETA c(ids[p]) and head 1's is
BETA c(g(p)): head 0 attends to the frame whose INDEX is the token id fed at p, head 1 to frame g(p), a fixed map that cycles through
the boundary frames `boundaries(T)`.  Identity and power-of-two weights are exact in bf16, f16 and e4m3; v_proj, both out_proj of the
cross-attention and everything behind them keep their seeded values, and V differs per stream through the audio half.
tests/test_cross_pointer_model.py checks on the oracle everything the GPU cases (tests/test_gpu_cross.py) rely on.
"""
from __future__ import annotations

import dataclasses
import functools
from typing import Callable, Dict, List, Tuple

import numpy as np

from oracle import whisper_oracle as wo
from tests.util import clips, dims_variant

A = 0.5
BETA = 4.0
HALF = 64
MAX_DOT = 24
B = 17               # sixteen streams and the first of a second group of sixteen
HEADS = [(0, 0), (0, 1)]
_ENC = "model.encoder"
_LAYER = "model.decoder.layers.0"


def boundaries(T: int) -> List[int]:
    """BND(T): the frames on either side of every 16-, 32-, 64- and 512-key edge of the kernels' fragment and chunk arithmetic, and the last two."""
    return sorted({k for k in (0, 1, 15, 16, 31, 32, 63, 64, 65, 127, 128, 255, 256, 511, 512, 513, 767, 768, 1023, 1024, 1025, T - 2, T - 1)
                   if 0 <= k < T})


def positions(T: int) -> int:
    """P: the smallest multiple of 32 with 16 P >= T (sixteen streams x P positions point at every frame once)."""
    return -(-T // (16 * 32)) * 32


def codes(T: int, seed: int = 0) -> np.ndarray:
    """float32 [T, 64]: balanced +-1 codes, drawn by rejection until every pairwise dot product is <= MAX_DOT."""
    rng = np.random.default_rng([seed, T])
    base = np.array([1.0] * (HALF // 2) + [-1.0] * (HALF // 2), np.float32)
    out = np.zeros((T, HALF), np.float32)
    n = 0
    while n < T:
        c = rng.permutation(base)
        if n == 0 or (out[:n] @ c).max() <= MAX_DOT:
            out[n] = c
            n += 1
    return out


def frame_map(T: int, P: int) -> np.ndarray:
    """g, int [P]: the frame head 1 of the query at position p points at - BND(T) in a cycle, half a cycle ahead of stream 16's ids."""
    bnd = np.array(boundaries(T))
    return bnd[(np.arange(P) + len(bnd) // 2) % len(bnd)]


def pointer_ids(T: int, P: int) -> np.ndarray:
    """int32 [B, P], ids < T: the frame (= token id) head 0 points at.  Streams 0..15 sweep every frame, stream 16 cycles through BND(T)."""
    bnd = np.array(boundaries(T))
    sweep = (np.arange(P)[None, :] * 16 + np.arange(16)[:, None]) % T
    ids = np.concatenate([sweep, bnd[np.arange(P) % len(bnd)][None]]).astype(np.int32)
    assert ids.shape == (B, P) and (ids >= 0).all() and (ids < T).all()
    return ids


def pointer_weights(T: int, P: int, seed: int = 0) -> Tuple[wo.WhisperDims, Dict[str, np.ndarray], np.ndarray]:
    """(dims, weights, g)."""
    dims = dims_variant("micro", enc_layers=1, dec_layers=1, max_source_positions=T, max_target_positions=P)
    assert dims.d_model == 2 * HALF and dims.heads == 2 and T <= dims.vocab
    w = dict(wo.make_weights(dims, 2))
    c, g = codes(T, seed), frame_map(T, P)
    eye, o = np.eye(HALF, dtype=np.float32), np.zeros((HALF, HALF), np.float32)
    for name in (".conv2.weight", ".conv2.bias"):
        w[_ENC + name] = w[_ENC + name].copy()
        w[_ENC + name][:HALF] = 0
    w[_ENC + ".embed_positions.weight"] = np.concatenate([A * c, np.zeros((T, HALF), np.float32)], axis=1)
    for name in (_ENC + ".layers.0.self_attn.out_proj", _ENC + ".layers.0.fc2", _LAYER + ".self_attn.out_proj"):
        for s in (".weight", ".bias"):
            w[name + s] = np.zeros_like(w[name + s])
    for name in (_ENC + ".layer_norm", _LAYER + ".encoder_attn_layer_norm"):
        w[name + ".weight"] = np.ones(2 * HALF, np.float32)
        w[name + ".bias"] = np.zeros(2 * HALF, np.float32)
    w[_LAYER + ".encoder_attn.k_proj.weight"] = np.block([[eye, o], [eye, o]])
    w[_LAYER + ".encoder_attn.q_proj.weight"] = np.float32(BETA) * np.block([[o, eye], [eye, o]])
    w[_LAYER + ".encoder_attn.q_proj.bias"] = np.zeros(2 * HALF, np.float32)
    w["model.decoder.embed_positions.weight"] = np.concatenate([A * c[g], np.zeros((P, HALF), np.float32)], axis=1)
    tok = w["model.decoder.embed_tokens.weight"].copy()
    tok[:T] = np.concatenate([np.zeros((T, HALF), np.float32), A * c], axis=1)
    w["model.decoder.embed_tokens.weight"] = tok
    return dims, w, g


@dataclasses.dataclass(frozen=True)
class Built:
    """Shared between tests: read only."""
    dims: wo.WhisperDims
    weights: Dict[str, np.ndarray]
    ids: np.ndarray        # int32 [B, P]
    mel: np.ndarray        # float32 [B, n_mels, 2 T]
    logits: np.ndarray     # float32 [B, P, V]: OracleWhisper.decode over all positions at once
    cross: np.ndarray      # float32 [B, 2, P, T]: the oracle's want_cross=HEADS rows
    g: np.ndarray          # int [P]
    enc: np.ndarray        # float32 [B, T, d]: the oracle's encoder output


@functools.lru_cache(maxsize=1)
def build(T: int, B: int = B) -> Built:
    """The pointer model at T frames: `B` streams (the first B rows of `pointer_ids`), each on a clip of its own.  (One entry is kept:
    [17, 96, 51866] float32 is 0.34 GB at T = 1500.)"""
    P = positions(T)
    dims, w, g = pointer_weights(T, P)
    ids = np.ascontiguousarray(pointer_ids(T, P)[:B])
    mel = wo.log_mel(clips(T * 320, B), dims.n_mels)
    om = wo.OracleWhisper(dims, w, T=T)
    enc = om.encode(mel)
    logits, cross = om.decode(ids, om.new_cache(enc), want_cross=HEADS)
    return Built(dims, w, ids, mel, logits, cross, g, enc)


def targets(ids: np.ndarray, g: np.ndarray) -> np.ndarray:
    """int [B, 2, P]: the frame each head of each query points at, in the layout of the alignment rows [B, 2, P, T]."""
    return np.stack([ids.astype(np.int64), np.broadcast_to(np.asarray(g, np.int64), ids.shape)], axis=1)


def margins(cross: np.ndarray, tgt: np.ndarray) -> np.ndarray:
    """float64 [B, 2, P]: score on the target minus the best other frame's score, read off softmax rows [B, 2, P, T] in float64 as
    log p_target - log max p_other (-inf where the target carries no probability; probabilities down to 1e-38 are kept by float32 rows)."""
    p = np.asarray(cross, np.float64)
    on = np.take_along_axis(p, tgt[..., None], axis=-1)[..., 0]
    rest = p.copy()
    np.put_along_axis(rest, tgt[..., None], -1.0, axis=-1)
    with np.errstate(divide="ignore"):
        return np.log(on) - np.log(rest.max(-1))


def floor_probability(T: int, m_min: float) -> float:
    """The least probability on the target of a softmax over T keys whose matched score leads every other by m_min - 1 (one unit of
    slack for score rounding: a bf16 key or query entry is off by 2^-9 relative, 0.2 in all on a matched score of about 42; the fp8
    contexts' margin is read off their own restatement's rows, whose keys went through e4m3)."""
    return 1.0 - T * float(np.exp(-(m_min - 1.0)))


# ---- mutants: what a wrong kernel would compute, as a change of the oracle's cross K/V cache -----------------------------------------
Hook = Callable[[wo.DecoderCache], None]


def hide_key(k: int) -> Hook:
    """Frame k does not exist for any query: the softmax runs over the other T - 1 frames - what a kernel that skips or masks the slot
    computes.  (Every decoder layer's cache, as the other hooks.)"""
    def f(cache):
        for i in range(len(cache.cross_k)):
            cache.cross_k[i] = np.delete(cache.cross_k[i], k, axis=2)
            cache.cross_v[i] = np.delete(cache.cross_v[i], k, axis=2)
    return f


def hide_key_per_block(ks: List[int], n: int) -> Hook:
    """`hide_key(ks[j])` for streams j n .. (j + 1) n - 1 of a cache that holds len(ks) copies of n streams: one oracle pass for all of them."""
    def f(cache):
        for i in range(len(cache.cross_k)):
            for name in ("cross_k", "cross_v"):
                x = getattr(cache, name)[i]
                assert x.shape[0] == len(ks) * n
                getattr(cache, name)[i] = np.concatenate([np.delete(x[j * n:(j + 1) * n], k, axis=2) for j, k in enumerate(ks)])
    return f


def swap_partner(k: int, T: int) -> int:
    return k + 1 if k + 1 < T else k - 1


def swap_values(k: int) -> Hook:
    """V[k] and V[k + 1] change places (k - 1 for the last frame): a kernel that pairs a probability with the neighbouring value slot."""
    def f(cache):
        for i in range(len(cache.cross_v)):
            v = cache.cross_v[i].copy()
            j = swap_partner(k, v.shape[2])
            v[:, :, [k, j]] = v[:, :, [j, k]]
            cache.cross_v[i] = v
    return f


def neighbour_stream(cache: wo.DecoderCache) -> None:
    """Stream b attends to the K/V of stream b + 1 (the last to the first's): a wrong arena offset."""
    for i in range(len(cache.cross_k)):
        cache.cross_k[i] = np.roll(cache.cross_k[i], -1, axis=0)
        cache.cross_v[i] = np.roll(cache.cross_v[i], -1, axis=0)


def hidden_of(om: wo.OracleWhisper, ids: np.ndarray, enc: np.ndarray, hook: Hook = None):
    """(hidden [B, P, d] in front of the final LayerNorm, alignment rows [B, 2, P, T']) of `om.decode` - the oracle's own method, of
    either oracle class, with the tied projection (the expensive part) left out - on the cache of `enc` after `hook`."""
    cache = om.new_cache(enc)
    if hook is not None:
        hook(cache)
    kept = []
    om._dec_logits = lambda x: kept.append(x) or np.zeros(x.shape[:-1] + (0,), np.float32)   # shadows the method for this call
    try:
        _, cross = om.decode(ids, cache, want_cross=HEADS)
    finally:
        del om._dec_logits
    return kept[0], cross


class LogitNorms:
    """Relative L2 of the f32 oracle's logits between two hidden states without forming [rows, 51866] logits: the logits are
    E LayerNorm(x), so |E y|^2 = y^T (E^T E) y, with the 128 x 128 Gram matrix computed once in float64."""

    def __init__(self, om: wo.OracleWhisper):
        self.om = om
        e = om.w["model.decoder.embed_tokens.weight"].astype(np.float64)
        self.gram = e.T @ e

    def _norm(self, y):
        return np.sqrt(np.einsum("...i,ij,...j->...", y, self.gram, y))

    def rel_l2(self, hidden: np.ndarray, base: np.ndarray) -> np.ndarray:
        a = self.om._ln(hidden, "model.decoder.layer_norm").astype(np.float64)
        b = self.om._ln(base, "model.decoder.layer_norm").astype(np.float64)
        return self._norm(a - b) / self._norm(b)
