"""``WhisperEngine`` - thin Python handle on a ``tw_ctx`` (include/thewhisper.h).

PyTorch is used only as plumbing here: it owns the caller-side device tensors (PCM, mel, logits)
and hands raw device pointers + the current HIP stream to the C ABI.  Every operation of the hot
path runs in libthewhisper_gfx950.so.
"""
from __future__ import annotations

import os

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _cabi

_TORCH2TW = {torch.float32: _cabi.TW_F32, torch.bfloat16: _cabi.TW_BF16, torch.float16: _cabi.TW_F16}


def _stream_ptr(device: torch.device) -> C.c_void_p:
    s = torch.cuda.current_stream(device).cuda_stream
    return C.c_void_p(int(s) if s else None)


# Which flavour `dtype="fp8"` means (BASELINE config 5): "fp8a16" = MXFP8 weights widened to bf16 in registers, activations not
# quantised (TW_BF16_W8A16: no activation-quantisation error, up to 64 streams); "fp8a8" = weights AND activations on the scaled fp8
# MFMA (TW_BF16_MXFP8, <= 16 streams).  THEWHISPER_FP8=a8|a16 overrides.
FP8_DEFAULT = {"a8": "fp8a8", "a16": "fp8a16"}.get(os.environ.get("THEWHISPER_FP8", "").lower(), "fp8a16")


def filter_rows(top_k, top_p, B: int):
    """``generate_sample``'s ``top_k`` / ``top_p`` (None, a scalar or one value per row) as the library's per-row arrays, checked with
    the library's rules: (int32 [B], float32 [B]), or None when every row is off - the call is then the unfiltered one."""
    k = np.zeros(B, dtype=np.int64) if top_k is None else np.asarray(top_k)
    p = np.ones(B, dtype=np.float32) if top_p is None else np.asarray(top_p, dtype=np.float32)
    if k.dtype.kind not in "iu" or k.size not in (1, B):
        raise ValueError(f"top_k must be an integer or one integer per row ({B}), got {top_k!r}")
    if p.size not in (1, B):
        raise ValueError(f"top_p must be a number or one number per row ({B}), got {top_p!r}")
    k = np.broadcast_to(k.reshape(-1).astype(np.int64), (B,))
    p = np.broadcast_to(p.reshape(-1), (B,))
    if (k < 0).any():
        raise ValueError(f"top_k must be >= 0 (0 = off), got {top_k!r}")
    if not ((p > 0) & (p <= 1)).all():
        raise ValueError(f"top_p must lie in (0, 1] (1 = off), got {top_p!r}")
    if not (k > 0).any() and not (p < 1).any():
        return None
    return np.ascontiguousarray(np.minimum(k, 2 ** 31 - 1), dtype=np.int32), np.ascontiguousarray(p, dtype=np.float32)


_F32_MAX = float(np.finfo(np.float32).max)


def sequence_bias_dict(sequence_bias) -> Dict[Tuple[int, ...], float]:
    """HF's ``sequence_bias`` - a list of ``[[token ids], bias]`` or a dict ``{tuple of token ids: bias}`` - as the dict
    ``SequenceBiasLogitsProcessor._convert_list_arguments_into_dict`` makes of it: a later duplicate of a list overwrites the bias and
    keeps the first one's place.  None or empty: the empty dict."""
    if not sequence_bias:
        return {}
    items = sequence_bias.items() if isinstance(sequence_bias, dict) else [(x[0], x[1]) for x in sequence_bias]
    out: Dict[Tuple[int, ...], float] = {}
    for ids, bias in items:
        key = tuple(int(t) for t in ids)
        if not key or any(t < 0 for t in key):
            raise ValueError(f"sequence_bias: every sequence is a non-empty list of token ids >= 0, got {ids!r}")
        bias = float(bias)
        if not abs(bias) <= _F32_MAX:      # (NaN fails the comparison too)
            raise ValueError(f"sequence_bias: the bias of {ids!r} must be a finite float32, got {bias!r}")
        out[key] = bias
    return out


def pack_sequence_bias(rows, B: int) -> Optional[Dict[str, np.ndarray]]:
    """The per-row lists of a call (``rows[b]``: HF's list or dict form, or None / empty for a row without one) as the arrays of
    ``tw_bias_opts``: ``row_off`` int32 [B + 1], ``seq_off`` int32 [n_seq + 1], ``tokens`` int32, ``bias`` float32 [n_seq]; row b owns
    sequences ``row_off[b] .. row_off[b + 1] - 1`` in the order of its dict (the order the library sums the biases of one last token
    in, a length-1 sequence first).  None when no row lists anything: the call is then the unbiased one."""
    if len(rows) != B:
        raise ValueError(f"sequence_bias_rows: {len(rows)} lists for {B} rows")
    row_off, seq_off, tokens, bias = [0], [0], [], []
    for r in rows:
        for key, val in sequence_bias_dict(r).items():
            tokens.extend(key)
            seq_off.append(len(tokens))
            bias.append(val)
        row_off.append(len(bias))
    if not bias:
        return None
    return {"row_off": np.asarray(row_off, dtype=np.int32), "seq_off": np.asarray(seq_off, dtype=np.int32),
            "tokens": np.asarray(tokens, dtype=np.int32), "bias": np.asarray(bias, dtype=np.float32)}


def merge_sequence_bias(first, second) -> Dict[Tuple[int, ...], float]:
    """Two lists for one row as one dict: ``first``'s entries keep their places, a sequence listed in both takes ``second``'s bias."""
    out = sequence_bias_dict(first)
    out.update(sequence_bias_dict(second))
    return out


def pack_ragged_prompts(prompts, pad_id: int) -> Tuple[np.ndarray, np.ndarray]:
    """Prompts of different lengths (a list of 1-D id sequences, none empty) as one LEFT-padded batch, the way HF batches Whisper's
    previous-text prompts: ``(prompt int32 [B, n], n_pad int32 [B])`` with n = the longest length and ``prompt[b, n_pad[b]:]`` = row b."""
    rows = [np.asarray(p, dtype=np.int64).reshape(-1) for p in prompts]
    if not rows or any(r.size == 0 for r in rows):
        raise ValueError("pack_ragged_prompts: at least one prompt, and every prompt needs one token")
    n = max(r.size for r in rows)
    out = np.full((len(rows), n), int(pad_id), dtype=np.int32)
    n_pad = np.zeros(len(rows), dtype=np.int32)
    for b, r in enumerate(rows):
        n_pad[b] = n - r.size
        out[b, n - r.size:] = r
    return out, n_pad


def ragged_n_pad(n_pad, B: int, n_forced: int = 0, n_draft: int = 0, biased: bool = False) -> Optional[np.ndarray]:
    """``generate_greedy``'s ``n_pad`` as the library's int32 [B] (None when nothing was given).  Padding does not go with forced
    tokens, drafts or a sequence bias; the values themselves are the library's to check (tw_generate_greedy_ragged: 0 <= n_pad < n_prompt)."""
    if n_pad is None:
        return None
    arr = np.asarray(n_pad)
    if arr.ndim != 1 or arr.size != B or arr.dtype.kind not in "iu":
        raise ValueError(f"n_pad must be one integer per row ({B}), got {n_pad!r}")
    if int(n_forced) or int(n_draft) or biased:
        raise ValueError("n_pad does not go together with n_forced, n_draft or sequence_bias / sequence_bias_rows")
    if (np.abs(arr.astype(np.int64)) > 2 ** 31 - 1).any():
        raise ValueError(f"n_pad does not fit int32: {n_pad!r}")
    return np.ascontiguousarray(arr, dtype=np.int32)


def repeat_rows(repetition_penalty, no_repeat_ngram_size, B: int):
    """``repetition_penalty`` / ``no_repeat_ngram_size`` (None, a scalar for every row, or one value per row) as the arrays of
    ``tw_repeat_opts``: float32 [B] (1.0 = off) and int32 [B] (0 = off).  None when every row has both off: the call is then the plain
    one.  Values the library would refuse raise ``ValueError`` here."""
    pen = np.ones(B, dtype=np.float32) if repetition_penalty is None else np.asarray(repetition_penalty, dtype=np.float32).reshape(-1)
    ngr = np.zeros(B, dtype=np.int64) if no_repeat_ngram_size is None else np.asarray(no_repeat_ngram_size).reshape(-1)
    if ngr.dtype.kind not in "iu":
        raise ValueError(f"no_repeat_ngram_size must be integers, got {no_repeat_ngram_size!r}")
    if pen.size not in (1, B) or ngr.size not in (1, B):
        raise ValueError(f"repetition_penalty / no_repeat_ngram_size: one value or one per row ({B}), got {pen.size} / {ngr.size}")
    pen = np.ascontiguousarray(np.broadcast_to(pen, (B,)), dtype=np.float32)
    ngr = np.broadcast_to(ngr, (B,))
    if not (np.isfinite(pen).all() and (pen > 0).all()):
        raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty!r}")
    if (ngr < 0).any() or (ngr > 2 ** 31 - 1).any():
        raise ValueError(f"no_repeat_ngram_size must be >= 0, got {no_repeat_ngram_size!r}")
    if (pen == 1.0).all() and (ngr == 0).all():
        return None
    return pen, np.ascontiguousarray(ngr, dtype=np.int32)


def _repeat_opts(rows, penalty_ignore: int):
    """``tw_repeat_opts`` over the arrays of ``repeat_rows`` (which the caller keeps alive)."""
    ro = _cabi.tw_repeat_opts()
    ro.penalty = rows[0].ctypes.data_as(C.POINTER(C.c_float))
    ro.no_repeat_ngram = rows[1].ctypes.data_as(C.POINTER(C.c_int32))
    ro.penalty_ignore = int(penalty_ignore)
    return ro


def _bias_opts(packed):
    """``tw_bias_opts`` over the arrays of ``pack_sequence_bias`` (which the caller keeps alive); None for None."""
    if packed is None:
        return None
    bo = _cabi.tw_bias_opts()
    bo.n_seq = int(packed["bias"].size)
    bo.row_off, bo.seq_off, bo.tokens = (packed[k].ctypes.data_as(C.POINTER(C.c_int32)) for k in ("row_off", "seq_off", "tokens"))
    bo.bias = packed["bias"].ctypes.data_as(C.POINTER(C.c_float))
    return bo


class WhisperEngine:
    """One MI355X context: weights + workspace + KV arenas for up to ``max_batch`` concurrent streams
    of ``T`` encoder frames (= 50 x chunk seconds)."""

    #: optional raw ``hipStream_t`` (int) to enqueue on instead of torch's current stream, e.g. a stream created with
    #: ``hipExtStreamCreateWithCUMask`` to confine this context to a subset of the CUs
    raw_stream: Optional[int] = None

    def _sp(self) -> C.c_void_p:
        if self.raw_stream is not None:
            return C.c_void_p(self.raw_stream)
        return _stream_ptr(self.device)

    def _decode_stream(self) -> Optional[int]:
        """The stream the greedy loop runs on when the caller does not manage streams (``raw_stream`` is None): confined to 160 of
        the 256 compute units.  Alone on the chip the loop is FASTER there than on all of them - 16 streams 1.3415 vs 1.3937 ms per
        step (192 CUs: 1.3564; 128: 1.664), one stream 1.0615 vs 1.0724 (tools/dbg/decode_cu_mask.py,
        profiles/r04_decode_cu_mask.txt): its launches have 160 or 320 workgroups.  THEWHISPER_DECODE_CUS=0 turns it off."""
        d = self.__dict__
        if "_dec_stream" not in d:
            ds = None
            try:
                n = int(os.environ.get("THEWHISPER_DECODE_CUS", "160"))
                total = torch.cuda.get_device_properties(self.device).multi_processor_count
                if 0 < n < total:
                    from .overlap import masked_stream

                    ds = masked_stream(0, n, total, self.device.index or 0)
            except Exception:  # noqa: BLE001  (no CU masks on this runtime: the loop runs on the caller's stream)
                ds = None
            d["_dec_stream"] = ds
        return d["_dec_stream"]

    def _adopt(self, *tensors) -> None:
        """With ``raw_stream`` set the work runs on a stream torch's caching allocator knows nothing about: order that
        stream after torch's current stream (which produced the inputs: H2D copies, slicing, casts) and keep every tensor
        handed to the library alive until the stream has been synchronised (``_release_held``), so that a temporary dropped
        on return is not recycled while the launches still read or write it.  (``Tensor.record_stream`` is not used: the
        allocator would touch the foreign stream when the tensor is freed - possibly after the stream was destroyed.)"""
        if self.raw_stream is None:
            return
        ext = torch.cuda.ExternalStream(self.raw_stream, device=self.device)
        ext.wait_stream(torch.cuda.current_stream(self.device))
        held = self.__dict__.setdefault("_held", [])
        if len(held) > 256:      # only asynchronous calls for a long time: drain rather than grow without bound
            ext.synchronize()
            held.clear()
        held.extend(t for t in tensors if t is not None and t.is_cuda)

    def _release_held(self) -> None:
        """Called after an entry point that synchronised the stream in use (greedy decode, timestamps, weight upload)."""
        held = self.__dict__.get("_held")
        if held:
            held.clear()

    def _publish(self) -> None:
        """Counterpart of ``_adopt`` for tensors RETURNED to the caller: torch's current stream waits for the foreign stream,
        so that the caller may consume the result with ordinary torch ops."""
        if self.raw_stream is not None:
            torch.cuda.current_stream(self.device).wait_stream(torch.cuda.ExternalStream(self.raw_stream, device=self.device))

    def _sync_used_stream(self) -> None:
        if self.raw_stream is not None:
            torch.cuda.ExternalStream(self.raw_stream, device=self.device).synchronize()
        else:
            torch.cuda.current_stream(self.device).synchronize()
        self._release_held()


    def __init__(
        self,
        dims: Dict[str, int],
        T: int,
        max_batch: int = 1,
        dtype: str = "bf16",
        alignment_heads: Optional[Sequence[Tuple[int, int]]] = None,
        device: int = 0,
        use_graph: bool = True,
    ):
        if not torch.cuda.is_available():
            raise RuntimeError("thewhisper_amd needs an MI355X (torch.cuda is not available); there is no CPU fallback")
        self.lib = _cabi.load_library()
        self.dims = dict(dims)
        self.T = int(T)
        self.max_batch = int(max_batch)
        self.device = torch.device("cuda", device)
        # "fp8" = bf16 activations and encoder, decoder projection weights quantised to MXFP8 at load (BASELINE config 5)
        # "fp8a16" = the same fp8 weights widened to bf16 in registers, activations NOT quantised (up to 64 streams); "fp8a8" =
        # weights and activations on the scaled fp8 MFMA (<= 16 streams); "fp8" = the flavour config 5 ships with (FP8_DEFAULT)
        if dtype == "fp8":
            dtype = FP8_DEFAULT
        self.dtype_name = dtype
        # "f16" = float16 context (round 4): the reference's streaming default dtype; same kernels instantiated for _Float16
        self.tw_dtype = {"bf16": _cabi.TW_BF16, "f16": _cabi.TW_F16, "f32": _cabi.TW_F32, "fp8a8": _cabi.TW_BF16_MXFP8,
                         "fp8a16": _cabi.TW_BF16_W8A16}[dtype]
        self.torch_dtype = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "fp8a8": torch.bfloat16,
                            "fp8a16": torch.bfloat16}[dtype]
        self.alignment_heads = [tuple(map(int, x)) for x in (alignment_heads or [])]
        cfg = _cabi.tw_config()
        cfg.d_model = dims["d_model"]
        cfg.enc_layers = dims["enc_layers"]
        cfg.dec_layers = dims["dec_layers"]
        cfg.heads = dims["heads"]
        cfg.ffn = dims["ffn"]
        cfg.vocab = dims["vocab"]
        cfg.n_mels = dims["n_mels"]
        cfg.source_positions = self.T
        cfg.target_positions = dims.get("max_target_positions", 448)
        cfg.max_batch = self.max_batch
        cfg.dtype = self.tw_dtype
        cfg.n_align_heads = len(self.alignment_heads)
        for i, (l, h) in enumerate(self.alignment_heads):
            cfg.align_heads[2 * i] = l
            cfg.align_heads[2 * i + 1] = h
        cfg.device = device
        cfg.use_graph = 1 if use_graph else 0
        self.P = cfg.target_positions
        self.vocab = cfg.vocab
        self.n_mels = cfg.n_mels
        self.d_model = cfg.d_model
        ctx = C.c_void_p()
        rc = self.lib.tw_create(C.byref(cfg), C.byref(ctx))
        if rc != 0:
            raise RuntimeError(f"tw_create failed ({rc}): {self.lib.tw_last_error(None).decode()}")
        self.ctx = ctx
        self._finalized = False

    def sibling(self, max_batch: Optional[int] = None) -> "WhisperEngine":
        """A second context of the same model on the same device that SHARES this engine's (finalized) weights and has its own
        workspace and K/V arenas (tw_create_sibling): two stages of a serving pipeline can then run at the same time - a context
        is not thread-safe, two contexts are independent.  This engine must outlive the sibling."""
        if not self._finalized:
            raise RuntimeError("sibling() needs loaded weights")
        new = object.__new__(type(self))
        new.__dict__.update({k: v for k, v in self.__dict__.items() if k not in ("ctx", "_held", "raw_stream", "_owner", "_dec_stream")})
        new.max_batch = int(max_batch or self.max_batch)
        ctx = C.c_void_p()
        rc = self.lib.tw_create_sibling(self.ctx, new.max_batch, C.byref(ctx))
        if rc != 0:
            raise RuntimeError(f"tw_create_sibling failed ({rc}): {self.lib.tw_last_error(None).decode()}")
        new.ctx = ctx
        new._owner = self           # keeps the weights' owner alive
        new._siblings = []
        self.__dict__.setdefault("_siblings", []).append(new)
        return new

    # ---- lifetime ----------------------------------------------------------------------------
    def close(self):
        for sib in self.__dict__.get("_siblings", []):   # they read this context's weights: they go first
            sib.close()
        self.__dict__["_siblings"] = []
        ds = self.__dict__.pop("_dec_stream", None)
        if ds is not None:
            try:
                from .overlap import _hiplib

                _hiplib().stream_destroy(ds)     # synchronises first
            except Exception:  # noqa: BLE001
                pass
        if getattr(self, "ctx", None):
            self.lib.tw_destroy(self.ctx)
            self.ctx = None

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int, what: str):
        _cabi.check(self.lib, self.ctx, rc, what)

    # ---- weights -----------------------------------------------------------------------------
    def load_weight(self, name: str, tensor: torch.Tensor):
        t = tensor.detach()
        if t.device.type != "cuda":
            t = t.to(self.device, non_blocking=False)
        t = t.contiguous()
        if t.dtype not in _TORCH2TW:
            t = t.float()
        shape = (C.c_int64 * t.dim())(*t.shape)
        self._adopt(t)
        rc = self.lib.tw_load_weight(self.ctx, name.encode(), C.c_void_p(t.data_ptr()), _TORCH2TW[t.dtype], t.dim(), shape,
                                     self._sp())
        self._chk(rc, f"tw_load_weight({name})")
        self._sync_used_stream()  # `t` may be a temporary

    def finalize(self):
        self._chk(self.lib.tw_finalize_weights(self.ctx, self._sp()), "tw_finalize_weights")
        self._finalized = True

    def load_state_dict(self, sd: Dict[str, torch.Tensor]):
        for k, v in sd.items():
            if k == "proj_out.weight":
                continue
            self.load_weight(k, v)
        self.finalize()

    @classmethod
    def from_numpy_weights(cls, dims, weights: Dict[str, np.ndarray], T: int, **kw) -> "WhisperEngine":
        eng = cls(dims, T, **kw)
        eng.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in weights.items()})
        return eng

    # ---- A1 ----------------------------------------------------------------------------------
    def logmel(self, pcm: torch.Tensor, n_valid: Optional[Sequence[int]] = None, n_samples: Optional[int] = None,
               out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
        """pcm: float32 CUDA tensor [B, n] -> [B, n_mels, n_samples//160] (zero padded to ``n_samples``)."""
        if pcm.dim() == 1:
            pcm = pcm[None]
        pcm = pcm.to(self.device, torch.float32).contiguous()
        B, n = pcm.shape
        n_samples = int(n_samples or n)
        if n_valid is None and n < n_samples:
            n_valid = [n] * B
        nv = None
        if n_valid is not None:
            nv = (C.c_int32 * B)(*[int(min(v, n)) for v in n_valid])
        out_dtype = out_dtype or self.torch_dtype
        out = torch.empty((B, self.n_mels, n_samples // 160), dtype=out_dtype, device=self.device)
        self._adopt(pcm, out)
        rc = self.lib.tw_logmel(self.ctx, C.c_void_p(pcm.data_ptr()), pcm.stride(0), nv, B, n_samples,
                                C.c_void_p(out.data_ptr()), _TORCH2TW[out_dtype], self._sp())
        self._chk(rc, "tw_logmel")
        self._publish()
        return out

    # ---- A2-A5 -------------------------------------------------------------------------------
    def encode(self, mel: torch.Tensor, return_hidden: bool = False, hidden_dtype: torch.dtype = torch.float32, slot0: int = 0):
        """Encoder for the B clips of ``mel`` into slots ``slot0 .. slot0+B-1`` of the context (``slot0 > 0``: the slots
        before it keep what earlier calls of this pass put there - ``tw_encode_at``)."""
        mel = mel.to(self.device).contiguous()
        if mel.dtype not in _TORCH2TW:
            mel = mel.float()
        B = mel.shape[0]
        if tuple(mel.shape[1:]) != (self.n_mels, 2 * self.T):
            # same failure mode as HF:models/whisper/modeling_whisper.py:612-617
            raise ValueError(
                f"Whisper expects the mel input features to be of length {2 * self.T}, but found {mel.shape[-1]} "
                f"(shape {tuple(mel.shape)})")
        out = None
        if return_hidden:
            out = torch.empty((B, self.T, self.d_model), dtype=hidden_dtype, device=self.device)
        self._adopt(mel, out)
        if slot0:
            if return_hidden:
                raise ValueError("return_hidden is only available for slot0 = 0")
            rc = self.lib.tw_encode_at(self.ctx, C.c_void_p(mel.data_ptr()), _TORCH2TW[mel.dtype], B, int(slot0), self._sp())
            self._chk(rc, "tw_encode_at")
            return None
        rc = self.lib.tw_encode(self.ctx, C.c_void_p(mel.data_ptr()), _TORCH2TW[mel.dtype], B,
                                C.c_void_p(out.data_ptr()) if out is not None else None,
                                _TORCH2TW[hidden_dtype], self._sp())
        self._chk(rc, "tw_encode")
        if out is not None:
            self._publish()
        return out

    def encode_tapped(self, mel: torch.Tensor, layer: int = 0, hidden_dtype: torch.dtype = torch.float32):
        """Test instrument (tw_encode_tapped): ``encode(mel, return_hidden=True)`` that also returns the intermediate buffers of encoder
        layer ``layer``, each copied on the device right after the launch that wrote it.  Returns ``(hidden [B, T, d], taps)``; every
        tap is the WHOLE workspace buffer, sized for ``max_batch`` (Bm) clips whatever B is, in the context dtype (the statistics in
        float32).  With T frames, d = d_model, H heads, F = ffn, Tp = T rounded up to 64:

        ``h1`` [Bm, 2T+2, d] (conv1 + GELU; rows 0 and 2T+1 of a clip are conv2's zero padding) - ``xa_in`` [Bm*T, d] (the layer's
        input; layer 0: conv2 + GELU + positions) - ``ln_stats_a`` [Bm*T, d/32, 2] ((sum, sum of squares) per 32-column block of
        ``xa_in``) - ``q``, ``k`` [Bm, H, T, 64] (q scaled by 1/8) - ``vt`` [Bm, H, 64, Tp] - ``attn`` [Bm*T, d] - ``xb`` [Bm*T, d]
        (after the out-projection and residual) - ``ln_stats_b`` [Bm*T, d/32, 2] - ``ffnh`` [Bm*T, F] - ``xa_out`` [Bm*T, d] (the
        layer's output) - ``enc_out`` [Bm*T, d] (after the final LayerNorm).  Contexts that do not fold the encoder's LayerNorms
        (d_model > 1280 or no multiple of 64) have no statistics taps."""
        mel = mel.to(self.device).contiguous()
        if mel.dtype not in _TORCH2TW:
            mel = mel.float()
        B = mel.shape[0]
        if tuple(mel.shape[1:]) != (self.n_mels, 2 * self.T):
            raise ValueError(f"Whisper expects the mel input features to be of length {2 * self.T}, but found {mel.shape[-1]}")
        Bm, T, d, H, F = self.max_batch, self.T, self.d_model, self.dims["heads"], self.dims["ffn"]
        Tp = (T + 63) // 64 * 64
        shapes = {"h1": (Bm, 2 * T + 2, d), "xa_in": (Bm * T, d), "q": (Bm, H, T, 64), "k": (Bm, H, T, 64), "vt": (Bm, H, 64, Tp),
                  "attn": (Bm * T, d), "xb": (Bm * T, d), "ffnh": (Bm * T, F), "xa_out": (Bm * T, d), "enc_out": (Bm * T, d)}
        if d % 64 == 0 and d <= 1280:
            shapes.update(ln_stats_a=(Bm * T, d // 32, 2), ln_stats_b=(Bm * T, d // 32, 2))
        taps = {k: torch.empty(v, dtype=torch.float32 if k.startswith("ln_stats") else self.torch_dtype, device=self.device)
                for k, v in shapes.items()}
        st = _cabi.tw_encode_taps()
        st.layer = int(layer)
        for k, t in taps.items():
            setattr(st, k, t.data_ptr())
        out = torch.empty((B, T, d), dtype=hidden_dtype, device=self.device)
        self._adopt(mel, out, *taps.values())
        rc = self.lib.tw_encode_tapped(self.ctx, C.c_void_p(mel.data_ptr()), _TORCH2TW[mel.dtype], B, C.c_void_p(out.data_ptr()),
                                       _TORCH2TW[hidden_dtype], C.byref(st), self._sp())
        self._chk(rc, "tw_encode_tapped")
        self._publish()
        return out, taps

    def cross_kv(self, B: int, slot0: int = 0):
        if slot0:
            self._chk(self.lib.tw_cross_kv_at(self.ctx, B, int(slot0), self._sp()), "tw_cross_kv_at")
        else:
            self._chk(self.lib.tw_cross_kv(self.ctx, B, self._sp()), "tw_cross_kv")

    def adopt_cross_kv(self, src: "WhisperEngine", src_slot0: int, B: int, dst_slot0: int):
        """Slots ``src_slot0 .. +B`` of ``src`` (another context of the same weights, e.g. one that encoded new arrivals on a
        CU-masked side stream while this one was decoding) become slots ``dst_slot0 .. +B`` of this context (tw_adopt_cross_kv)."""
        self._chk(self.lib.tw_adopt_cross_kv(self.ctx, int(dst_slot0), src.ctx, int(src_slot0), int(B), self._sp(), src._sp()),
                  "tw_adopt_cross_kv")

    # ---- A6-A8 (teacher-forced stepping, used by the parity tests) ---------------------------
    def decoder_reset(self, B: int):
        self._chk(self.lib.tw_decoder_reset(self.ctx, B, self._sp()), "tw_decoder_reset")

    def decode_step(self, ids: Sequence[int], want_logits: bool = True) -> Optional[torch.Tensor]:
        B = len(ids)
        arr = (C.c_int32 * B)(*[int(i) for i in ids])
        out = torch.empty((B, self.vocab), dtype=torch.float32, device=self.device) if want_logits else None
        self._adopt(out)
        rc = self.lib.tw_decode_step(self.ctx, B, arr, C.c_void_p(out.data_ptr()) if out is not None else None,
                                     self._sp())
        self._chk(rc, "tw_decode_step")
        if out is not None:
            self._publish()
        return out

    # ---- language detection (include/thewhisper.h: THE RULE) ------------------------------------
    def detect_language(self, B: int, sot_id: int, lang_ids: Sequence[int]) -> Dict[str, np.ndarray]:
        """Rows 0 .. B-1 of the cross K/V (``encode`` + ``cross_kv`` first): one decoder step on ``sot_id`` and the language rule on that
        step's logits (tw_detect_language) - ``ids`` int32 [B], the winning token id per row, and ``probs`` float32 [B, n_lang], the
        softmax over the listed ids in the order of ``lang_ids``.  Only those come back, not the logits.  It belongs in front of the
        generate call of a pass: it rewinds the decoder and overwrites the alignment rows of a previous decode."""
        ids = np.ascontiguousarray(np.asarray(list(lang_ids), dtype=np.int32).reshape(-1))
        n = int(ids.size)
        out_id = np.zeros(max(int(B), 1), dtype=np.int32)
        out_p = np.zeros((max(int(B), 1), max(n, 1)), dtype=np.float32)
        rc = self.lib.tw_detect_language(self.ctx, int(B), int(sot_id), ids.ctypes.data_as(C.POINTER(C.c_int32)), n,
                                         out_id.ctypes.data_as(C.POINTER(C.c_int32)), out_p.ctypes.data_as(C.POINTER(C.c_float)), self._sp())
        self._chk(rc, "tw_detect_language")
        return {"ids": out_id, "probs": out_p}

    def language_logits(self, logits: torch.Tensor, lang_ids: Sequence[int]) -> Dict[str, np.ndarray]:
        """The language rule on caller-provided logits (tw_language_logits): ``logits`` - a contiguous float32 ``[rows, V]`` tensor on this
        engine's device, only read.  Returns ``ids`` int32 [rows] and ``probs`` float32 [rows, n_lang]."""
        if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous() or logits.device != torch.device(self.device):
            raise ValueError("language_logits: a contiguous float32 [rows, V] tensor on the engine's device")
        rows, V = int(logits.shape[0]), int(logits.shape[1])
        ids = np.ascontiguousarray(np.asarray(list(lang_ids), dtype=np.int32).reshape(-1))
        n = int(ids.size)
        out_id = np.zeros(max(rows, 1), dtype=np.int32)
        out_p = np.zeros((max(rows, 1), max(n, 1)), dtype=np.float32)
        self._adopt(logits)
        rc = self.lib.tw_language_logits(int(torch.device(self.device).index or 0), C.c_void_p(logits.data_ptr()), V, rows,
                                         ids.ctypes.data_as(C.POINTER(C.c_int32)), n, out_id.ctypes.data_as(C.POINTER(C.c_int32)),
                                         out_p.ctypes.data_as(C.POINTER(C.c_float)), self._sp())
        _cabi.check(self.lib, None, rc, "tw_language_logits")     # (context-free: the message is the library's, not the context's)
        return {"ids": out_id, "probs": out_p}

    # ---- A9/A10 ------------------------------------------------------------------------------
    @staticmethod
    def _greedy_opts(eos_id, pad_id, timestamps, no_timestamps_id, max_initial_timestamp_index, begin_suppress, suppress, min_new_tokens=0,
                     max_new_tokens=0, max_length=0, want_alignment=False, n_forced=0, n_draft=0):
        """``tw_greedy_opts`` of a call's keywords (generate_greedy, generate_sample, score_tokens build it here, so they cannot drift);
        the struct points into the two arrays returned beside it: keep them alive for the call."""
        o = _cabi.tw_greedy_opts()
        o.eos_id, o.pad_id = int(eos_id), int(pad_id)
        o.max_new_tokens, o.min_new_tokens, o.max_length = int(max_new_tokens), int(min_new_tokens), int(max_length)
        o.timestamps = 1 if timestamps else 0
        o.no_timestamps_id = int(no_timestamps_id)
        o.max_initial_timestamp_index = -1 if max_initial_timestamp_index is None else int(max_initial_timestamp_index)
        bs = [int(x) for x in begin_suppress]
        sp = [int(x) for x in suppress]
        bs_arr = (C.c_int32 * max(1, len(bs)))(*bs)
        sp_arr = (C.c_int32 * max(1, len(sp)))(*sp)
        o.n_begin_suppress, o.begin_suppress = len(bs), bs_arr
        o.n_suppress, o.suppress = len(sp), sp_arr
        o.want_alignment = 1 if want_alignment else 0
        o.n_forced = int(n_forced)
        o.n_draft = int(n_draft)
        return o, (bs_arr, sp_arr)

    def _loop_stream(self) -> C.c_void_p:
        """The decode stream (``_decode_stream``) ordered behind everything enqueued so far (the encoder stage); the generate call
        synchronises it before returning.  The caller's stream when it manages streams itself or no decode stream exists."""
        if self.raw_stream is None:
            ds = self._decode_stream()
            if ds is not None:
                torch.cuda.ExternalStream(ds, device=self.device).wait_stream(torch.cuda.current_stream(self.device))
                return C.c_void_p(ds)
        return self._sp()

    def _generate(self, name: str, prompt: np.ndarray, o, extras, max_length: int, pad_id: int, sp) -> Dict[str, np.ndarray]:
        """One call of the generate family: ``name(ctx, B, prompt, n0, &o, *extras, out, &out_len, stream)``, which every member is;
        ``extras``: the arguments between, ready for ctypes."""
        B, n0 = prompt.shape
        out = np.full((B, int(max_length)), pad_id, dtype=np.int32)
        out_len = C.c_int32(0)
        i32p = C.POINTER(C.c_int32)
        rc = getattr(self.lib, name)(self.ctx, B, prompt.ctypes.data_as(i32p), n0, C.byref(o), *extras, out.ctypes.data_as(i32p),
                                     C.byref(out_len), sp)
        self._chk(rc, name)
        self._release_held()   # the call returns after synchronising its stream, which is ordered after the encoder stage
        L = int(out_len.value)
        return {"sequences": out[:, :L].astype(np.int64), "length": L}

    def generate_greedy(
        self,
        prompt: np.ndarray,
        max_new_tokens: int = 128,
        min_new_tokens: int = 0,
        max_length: int = 448,
        eos_id: int = 50257,
        pad_id: int = 50257,
        timestamps: bool = False,
        no_timestamps_id: int = 50364,
        max_initial_timestamp_index: Optional[int] = 50,
        begin_suppress: Iterable[int] = (220, 50257),
        suppress: Iterable[int] = (),
        want_alignment: bool = False,
        n_forced: int = 0,
        n_draft: int = 0,
        sequence_bias=None,
        sequence_bias_rows=None,
        n_pad=None,
        repetition_penalty=None,
        no_repeat_ngram_size=None,
        penalty_ignore: int = 0,
    ) -> Dict[str, np.ndarray]:
        """``repetition_penalty`` / ``no_repeat_ngram_size``: HF's options of those names, a scalar for every row or one value per row
        (1.0 / 0 = off); ``penalty_ignore``: HF's ``prompt_ignore_length`` of the penalty.  The rule is tw_generate_greedy_repeat's
        (include/thewhisper.h): HF's two processors behind the sequence bias and ahead of Whisper's processors, per row, honoured under
        ``n_forced`` and ``n_draft``.  Not together with ``n_pad``.
        ``n_pad``: one integer per row - the first ``n_pad[b]`` entries of prompt row b are LEFT padding (tw_generate_greedy_ragged, where
        the rule is stated: the row is decoded as if alone with its real tokens; the returned rows keep their padding).  Not together
        with ``n_forced``, ``n_draft`` or a sequence bias.
        ``sequence_bias``: HF's ``sequence_bias`` (list or dict form) for every row; ``sequence_bias_rows``: one such list per row
        (None for a row without one) - not both.  The rule is tw_generate_greedy_biased's (include/thewhisper.h): HF's
        ``SequenceBiasLogitsProcessor`` ahead of Whisper's processors, per row, honoured under ``n_forced`` and ``n_draft``.
        ``n_forced``: the last ``n_forced`` tokens of every prompt row are forced OUTPUT tokens (they count as generated; a
        batched prefill processes them - tw_greedy_opts::n_forced); the returned sequences contain them like generated ones.
        ``n_draft``: the last ``n_draft`` tokens of every prompt row are GUESSES of the output (tw_greedy_opts::n_draft): verified in
        batched launches, the call returns what it returns without them; ``draft`` in the result says how many were confirmed."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        B = prompt.shape[0]
        pads = ragged_n_pad(n_pad, B, n_forced, n_draft, sequence_bias is not None or sequence_bias_rows is not None)
        if sequence_bias is not None and sequence_bias_rows is not None:
            raise ValueError("sequence_bias (every row) and sequence_bias_rows (per row): give one of the two")
        if sequence_bias is not None:
            sequence_bias_rows = [sequence_bias] * B
        packed = pack_sequence_bias(list(sequence_bias_rows), B) if sequence_bias_rows is not None else None
        if int(penalty_ignore) < 0:
            raise ValueError(f"penalty_ignore must be >= 0, got {penalty_ignore!r}")
        repeat = repeat_rows(repetition_penalty, no_repeat_ngram_size, B)
        if repeat is not None and pads is not None:
            raise ValueError("n_pad does not go with repetition_penalty / no_repeat_ngram_size (the ragged call takes no repeat options)")
        o, _keep = self._greedy_opts(eos_id, pad_id, timestamps, no_timestamps_id, max_initial_timestamp_index, begin_suppress, suppress,
                                     min_new_tokens, max_new_tokens, max_length, want_alignment, n_forced, n_draft)
        # (calls with a forced prefix stay on the caller's stream: their batched prefill - launches of up to 64 rows - wants the whole
        #  chip; measured on the reuse path's short calls: 16.1 ms per tick there, 19.9 on the 160-CU stream)
        sp = self._loop_stream() if int(n_forced) == 0 and int(n_draft) == 0 else self._sp()
        bo = _bias_opts(packed)
        if pads is not None:
            name, extras = "tw_generate_greedy_ragged", (pads.ctypes.data_as(C.POINTER(C.c_int32)),)
        elif repeat is not None:
            ro = _repeat_opts(repeat, penalty_ignore)
            name, extras = "tw_generate_greedy_repeat", (C.byref(bo) if bo is not None else None, C.byref(ro))
        elif bo is None:
            name, extras = "tw_generate_greedy", ()
        else:
            name, extras = "tw_generate_greedy_biased", (C.byref(bo),)
        res = self._generate(name, prompt, o, extras, max_length, pad_id, sp)
        if int(n_draft) > 0:
            v = [C.c_int32(0) for _ in range(4)]
            self._chk(self.lib.tw_last_draft(self.ctx, *[C.byref(x) for x in v]), "tw_last_draft")
            res["draft"] = {"offered": int(v[0].value), "accepted": int(v[1].value), "launches": int(v[2].value), "rounds": int(v[3].value)}
        return res

    def repeat_logits(self, logits: torch.Tensor, history, n_hist=None, *, repetition_penalty=None, no_repeat_ngram_size=None,
                      penalty_ignore: int = 0) -> torch.Tensor:
        """The repeat rule of tw_generate_greedy_repeat on caller-provided data (tw_repeat_logits): ``logits`` - a contiguous float32
        ``[rows, V]`` tensor on this engine's device - is edited IN PLACE and returned; row r is processed with the ids
        ``history[r, :n_hist[r]]`` (``history``: int ``[rows, ld]``; ``n_hist`` None = every row's whole ``ld``) and row r of the two
        options (a scalar or one value per row)."""
        if logits.dtype != torch.float32 or logits.dim() != 2 or not logits.is_contiguous() or logits.device != torch.device(self.device):
            raise ValueError("repeat_logits: logits must be a contiguous float32 [rows, V] tensor on the engine's device")
        rows, V = int(logits.shape[0]), int(logits.shape[1])
        hist = np.ascontiguousarray(history, dtype=np.int32).reshape(rows, -1)
        ld = int(hist.shape[1])
        nh = np.full(rows, ld, dtype=np.int32) if n_hist is None else np.ascontiguousarray(np.broadcast_to(np.asarray(n_hist, dtype=np.int32), (rows,)))
        rr = repeat_rows(repetition_penalty, no_repeat_ngram_size, rows)
        if rr is None:
            rr = (np.ones(rows, dtype=np.float32), np.zeros(rows, dtype=np.int32))
        ro = _repeat_opts(rr, penalty_ignore)
        if hist.size == 0:
            hist = np.zeros(1, dtype=np.int32)   # (a valid pointer for ld == 0)
        rc = self.lib.tw_repeat_logits(int(torch.device(self.device).index or 0), C.c_void_p(logits.data_ptr()), V, rows,
                                       hist.ctypes.data_as(C.POINTER(C.c_int32)), ld, nh.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(ro),
                                       self._sp())
        _cabi.check(self.lib, None, rc, "tw_repeat_logits")     # (context-free: the message is the library's, not the context's)
        return logits

    def generate_greedy_ragged(self, prompts, *, pad_id: int = 50257, **kw) -> Dict[str, np.ndarray]:
        """``generate_greedy`` for prompts of different lengths (a list of 1-D id sequences), in ONE call: the rows are left-padded with
        ``pad_id`` (``pack_ragged_prompts``) and decoded by the ragged rule - each as if it were alone.  ``sequences``: a list with one
        int64 array per row, the row's prompt and what it generated WITHOUT the padding; ``n_pad``: int32 [B]; ``length``: the common
        padded length.  Keywords as ``generate_greedy`` (``n_forced``, ``n_draft`` and a sequence bias are refused)."""
        prompt, n_pad = pack_ragged_prompts(prompts, pad_id)
        res = self.generate_greedy(prompt, pad_id=pad_id, n_pad=n_pad, **kw)
        seq = res["sequences"]
        return {"sequences": [seq[b, int(n_pad[b]):] for b in range(seq.shape[0])], "n_pad": n_pad, "length": res["length"]}

    # ---- beam search --------------------------------------------------------------------------
    def generate_beam(self, prompt: np.ndarray, num_beams: int, length_penalty: float = 1.0, early_stopping: bool = False, *,
                      max_new_tokens: int = 128, min_new_tokens: int = 0, max_length: int = 448, eos_id: int = 50257, pad_id: int = 50257,
                      timestamps: bool = False, no_timestamps_id: int = 50364, max_initial_timestamp_index: Optional[int] = 50,
                      begin_suppress: Iterable[int] = (220, 50257), suppress: Iterable[int] = (),
                      want_alignment: bool = False) -> Dict[str, np.ndarray]:
        """Beam search with ``num_beams`` (2..8) beams per row of ``prompt`` (tw_generate_beam, where the rule - HF's
        ``GenerationMixin._beam_search`` - is stated).  Needs ``max_batch >= rows x num_beams``.  ``sequences`` int64 [n, L]: the best
        hypotheses; ``scores`` float32 [n]; ``nbest_sequences`` int64 [n, K, Ln] and ``nbest_scores`` float32 [n, K]: every hypothesis in
        descending score (a score <= -1e9 marks a placeholder).  Everything behind a hypothesis's end is ``pad_id``.  The other
        keywords are ``generate_greedy``'s processors.  ``lengths`` int32 [n] and ``nbest_lengths`` int32 [n, K]: the tokens of every
        hypothesis, prompt included (the prompt's for a placeholder).
        ``want_alignment``: the call is tw_generate_beam_aligned - same ids and scores, and afterwards slot ``k * n + c`` of the
        alignment buffer holds the rows of hypothesis k of clip c (``beam_token_timestamps``, ``get_alignment``)."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        n, n0 = prompt.shape
        K = int(num_beams)
        if early_stopping not in (False, True, 0, 1):
            raise ValueError(f"early_stopping must be False or True, got {early_stopping!r}")
        o, _keep = self._greedy_opts(eos_id, pad_id, timestamps, no_timestamps_id, max_initial_timestamp_index, begin_suppress, suppress,
                                     min_new_tokens, max_new_tokens, max_length, bool(want_alignment))
        bo = _cabi.tw_beam_opts()
        bo.num_beams, bo.length_penalty, bo.early_stopping = K, float(length_penalty), 1 if early_stopping else 0
        ld = int(max_length)
        out = np.full((n, ld), pad_id, dtype=np.int32)
        nbest = np.full((n, max(K, 1), ld), pad_id, dtype=np.int32)
        score = np.zeros((n,), dtype=np.float32)
        nscore = np.zeros((n, max(K, 1)), dtype=np.float32)
        out_len = (C.c_int32 * 2)(0, 0)
        i32p, f32p = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        hyp_len = np.full((n, max(K, 1)), n0, dtype=np.int32)
        rc = self.lib.tw_generate_beam_aligned(self.ctx, n, prompt.ctypes.data_as(i32p), n0, C.byref(o), C.byref(bo),
                                               out.ctypes.data_as(i32p), out_len, score.ctypes.data_as(f32p), nbest.ctypes.data_as(i32p),
                                               nscore.ctypes.data_as(f32p), hyp_len.ctypes.data_as(i32p), self._loop_stream())
        self._chk(rc, "tw_generate_beam_aligned")
        self._release_held()
        L, Ln = int(out_len[0]), int(out_len[1])
        self._last_beam = {"n": n, "K": K, "n_prompt": n0, "lengths": hyp_len.copy(), "L": L, "Ln": Ln, "aligned": bool(want_alignment)}
        return {"sequences": out[:, :L].astype(np.int64), "scores": score, "nbest_sequences": nbest[:, :, :Ln].astype(np.int64),
                "nbest_scores": nscore, "length": L, "lengths": hyp_len[:, 0].copy(), "nbest_lengths": hyp_len}

    # ---- temperature sampling ----------------------------------------------------------------
    def generate_sample(self, prompt: np.ndarray, temperature, seed, offset=None, *, max_new_tokens: int = 128, min_new_tokens: int = 0,
                        max_length: int = 448, eos_id: int = 50257, pad_id: int = 50257, timestamps: bool = False,
                        no_timestamps_id: int = 50364, max_initial_timestamp_index: Optional[int] = 50,
                        begin_suppress: Iterable[int] = (220, 50257), suppress: Iterable[int] = (), want_alignment: bool = False,
                        n_forced: int = 0, n_draft: int = 0, top_k=None, top_p=None) -> Dict[str, np.ndarray]:
        """``generate_greedy`` with a draw from ``softmax(processed logits / temperature[b])`` per row (tw_generate_sample; the draw is
        defined in include/thewhisper.h).  ``temperature``, ``seed``, ``offset``: one value per row, or a scalar for every row.
        ``temperature[b] == 0``: the row is greedy; ``< 0``: the row sits the call out (``pad_id`` from the prompt on).  The noise is a
        function of (seed, offset, position, token id): a row's result does not depend on its slot or on its batch-mates.  ``n_forced`` /
        ``n_draft`` are refused by the library.  ``top_k`` / ``top_p`` (None, a scalar or one value per row; 0 / 1.0 = off): the draw is
        from the top-k ids and, of those, the smallest set of the largest whose mass reaches ``top_p`` (tw_generate_sample_filtered,
        where the rule is stated; ``top_k=50`` is HF's candidate set).  With both off the call is the unfiltered one."""
        prompt = np.ascontiguousarray(prompt, dtype=np.int32)
        B = prompt.shape[0]
        filt = filter_rows(top_k, top_p, B)
        rows = [None if x is None else np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=dt).reshape(-1), (B,)))
                for x, dt in ((temperature, np.float32), (seed, np.uint64), (offset, np.uint64))]
        so = _cabi.tw_sample_opts()
        so.temperature = rows[0].ctypes.data_as(C.POINTER(C.c_float))
        so.seed = rows[1].ctypes.data_as(C.POINTER(C.c_uint64))
        so.offset = rows[2].ctypes.data_as(C.POINTER(C.c_uint64)) if rows[2] is not None else None
        o, _keep = self._greedy_opts(eos_id, pad_id, timestamps, no_timestamps_id, max_initial_timestamp_index, begin_suppress, suppress,
                                     min_new_tokens, max_new_tokens, max_length, want_alignment, n_forced, n_draft)
        sp = self._loop_stream()     # the decode stream, as the plain greedy call
        if filt is None:
            return self._generate("tw_generate_sample", prompt, o, (C.byref(so),), max_length, pad_id, sp)
        fo = _cabi.tw_filter_opts()
        fo.top_k = filt[0].ctypes.data_as(C.POINTER(C.c_int32))
        fo.top_p = filt[1].ctypes.data_as(C.POINTER(C.c_float))
        return self._generate("tw_generate_sample_filtered", prompt, o, (C.byref(so), C.byref(fo)), max_length, pad_id, sp)

    # ---- scores of finished sequences --------------------------------------------------------
    def score_tokens(
        self,
        sequences: np.ndarray,
        n_prompt: int,
        *,
        no_speech_id: Optional[int] = None,
        no_speech_pos: int = 0,
        min_new_tokens: int = 0,
        eos_id: int = 50257,
        pad_id: int = 50257,
        timestamps: bool = False,
        no_timestamps_id: int = 50364,
        max_initial_timestamp_index: Optional[int] = 50,
        begin_suppress: Iterable[int] = (220, 50257),
        suppress: Iterable[int] = (),
        **ignored,
    ) -> Dict[str, Optional[np.ndarray]]:
        """Log-probability of every token of ``sequences`` [B, L] behind the first ``n_prompt`` given the tokens before it, by a
        teacher-forced pass (tw_score_tokens).  ``logprob``: after the logits processors the keywords describe - the ones
        ``generate_greedy`` takes; its other keywords (``max_new_tokens``, ``n_draft`` ...) are accepted and ignored - which is what HF
        averages into ``avg_logprob``; ``logprob_raw``: of the unprocessed logits.  Both float32 [B, L], 0 for the prompt and for the
        padding behind a row's first ``eos_id``.  ``no_speech_prob`` [B]: probability of ``no_speech_id`` at position ``no_speech_pos``
        (None when no id is given)."""
        seq = np.ascontiguousarray(sequences, dtype=np.int32)
        B, L = seq.shape
        o, _keep = self._greedy_opts(eos_id, pad_id, timestamps, no_timestamps_id, max_initial_timestamp_index, begin_suppress, suppress,
                                     min_new_tokens)
        lp = np.zeros((B, L), dtype=np.float32)
        raw = np.zeros((B, L), dtype=np.float32)
        ns = np.zeros((B,), dtype=np.float32) if no_speech_id is not None else None
        fp = C.POINTER(C.c_float)
        rc = self.lib.tw_score_tokens(self.ctx, B, seq.ctypes.data_as(C.POINTER(C.c_int32)), L, L, int(n_prompt), C.byref(o),
                                      -1 if no_speech_id is None else int(no_speech_id), int(no_speech_pos),
                                      lp.ctypes.data_as(fp), raw.ctypes.data_as(fp), ns.ctypes.data_as(fp) if ns is not None else None,
                                      self._sp())
        self._chk(rc, "tw_score_tokens")
        return {"logprob": lp, "logprob_raw": raw, "no_speech_prob": ns}

    # ---- A11 ---------------------------------------------------------------------------------
    def token_timestamps(self, B: int, n_prompt: int, seq_len: int, num_frames: Optional[Sequence[int]] = None,
                         time_precision: float = 0.02) -> np.ndarray:
        out = np.zeros((B, seq_len), dtype=np.float32)
        nf = None
        if num_frames is not None:
            nf = (C.c_int32 * B)(*[int(x) for x in num_frames])
        rc = self.lib.tw_token_timestamps(self.ctx, B, n_prompt, seq_len, nf, float(time_precision),
                                          out.ctypes.data_as(C.POINTER(C.c_float)), self._sp())
        self._chk(rc, "tw_token_timestamps")
        return out

    def token_timestamps_each(self, seq_lens: Sequence[int], n_prompt: int, num_frames: Optional[Sequence[int]] = None,
                              time_precision: float = 0.02, ld: Optional[int] = None) -> np.ndarray:
        """``token_timestamps`` for rows of different lengths (tw_token_timestamps_each): row b of the alignment buffer holds
        ``seq_lens[b]`` tokens; float32 [B, ld] (``ld``: the longest row unless given).  A row's first ``seq_lens[b]`` entries are what
        ``token_timestamps`` returns for it alone; the entries behind repeat its last one; a row with nothing generated is zeros."""
        lens = np.ascontiguousarray(np.asarray(seq_lens, dtype=np.int32).reshape(-1))
        B = int(lens.shape[0])
        ld = int(ld) if ld is not None else max(int(lens.max()), 1)
        out = np.zeros((B, ld), dtype=np.float32)
        nf = None
        if num_frames is not None:
            nf = (C.c_int32 * B)(*[int(x) for x in num_frames])
        rc = self.lib.tw_token_timestamps_each(self.ctx, B, int(n_prompt), lens.ctypes.data_as(C.POINTER(C.c_int32)), ld, nf,
                                               float(time_precision), out.ctypes.data_as(C.POINTER(C.c_float)), self._sp())
        self._chk(rc, "tw_token_timestamps_each")
        return out

    def beam_token_timestamps(self, nbest: bool = False, num_frames: Optional[Sequence[int]] = None,
                              time_precision: float = 0.02) -> np.ndarray:
        """Token timestamps of the most recent ``generate_beam(want_alignment=True)``: float32 [n, L] for the best hypotheses, or
        [n, K, Ln] for every hypothesis (``nbest``) - each by the rule of tw_generate_beam_aligned, i.e. on its own rows, as if its clip
        had been decoded alone.  ``num_frames``: one value per clip."""
        st = getattr(self, "_last_beam", None)
        if st is None or not st["aligned"]:
            raise RuntimeError("beam_token_timestamps needs a generate_beam(want_alignment=True) call before it")
        n, K, n0 = st["n"], st["K"], st["n_prompt"]
        if num_frames is not None and len(num_frames) != n:
            raise ValueError(f"num_frames has {len(num_frames)} entries for {n} clips")
        if not nbest:
            return self.token_timestamps_each(st["lengths"][:, 0], n0, num_frames, time_precision, ld=st["L"])
        lens = st["lengths"].T.reshape(-1)             # slot k * n + c
        nf = None if num_frames is None else [int(num_frames[c]) for _ in range(K) for c in range(n)]
        ts = self.token_timestamps_each(lens, n0, nf, time_precision, ld=st["Ln"])
        return np.ascontiguousarray(ts.reshape(K, n, -1).transpose(1, 0, 2))

    def get_alignment(self, B: int, n_rows: int) -> np.ndarray:
        out = np.zeros((B, len(self.alignment_heads), n_rows, self.T), dtype=np.float32)
        rc = self.lib.tw_get_alignment(self.ctx, B, n_rows, out.ctypes.data_as(C.POINTER(C.c_float)),
                                       self._sp())
        self._chk(rc, "tw_get_alignment")
        return out

    def set_alignment(self, arr: np.ndarray) -> None:
        """Debug/parity: put float32 [B, n_align_heads, n_rows, T] into rows 0 .. n_rows-1 of the recorded-alignment buffer."""
        a = np.ascontiguousarray(arr, dtype=np.float32)
        if a.ndim != 4 or a.shape[1] != len(self.alignment_heads) or a.shape[3] != self.T:
            raise ValueError(f"alignment rows must be [B, {len(self.alignment_heads)}, n_rows, {self.T}], got {a.shape}")
        rc = self.lib.tw_set_alignment(self.ctx, a.shape[0], a.shape[2], a.ctypes.data_as(C.POINTER(C.c_float)), self._sp())
        self._chk(rc, "tw_set_alignment")

    def last_prompt_rows(self) -> Dict[str, int]:
        """How the last generate call consumed its prompt (tw_last_prompt_rows): ``launches`` rows-mode launches (0: one position per
        step) that took ``positions`` prompt positions."""
        v = [C.c_int32(0) for _ in range(2)]
        self._chk(self.lib.tw_last_prompt_rows(self.ctx, *[C.byref(x) for x in v]), "tw_last_prompt_rows")
        return {"launches": int(v[0].value), "positions": int(v[1].value)}

    def last_timings(self) -> Dict[str, float]:
        ms = (C.c_float * 5)()
        steps = C.c_int32(0)
        self._chk(self.lib.tw_last_timings(self.ctx, ms, C.byref(steps)), "tw_last_timings")
        names = ["logmel_ms", "encode_ms", "cross_kv_ms", "greedy_ms", "token_timestamps_ms"]
        d = {n: float(ms[i]) for i, n in enumerate(names)}
        d["decode_steps"] = int(steps.value)
        return d
