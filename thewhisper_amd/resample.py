"""Sample-rate / sample-format front end on the MI355X: 8-96 kHz, float32 or int16, 1-8 channels -> 16 kHz mono float32.

The reference resamples a client's audio on the host with ``librosa.resample`` before its pipeline sees it
(R:thestage_speechkit/streaming/streams.py:103-105, R:examples/run_nvidia_asr.py:30).  Here that step is ``tw_resample``: a
rational polyphase Kaiser-windowed-sinc resampler of this project's own definition (csrc/k_resample.hip; NOT a port of librosa
or soxr), computed behind the C ABI like the log-mel and the voice-activity gate.

    y = resample(x48, 48000)                          # one-shot: [n] or [n, channels] (float32 / int16) -> [ceil(n L / M)]
    rs = StreamResampler(48000, channels=2, fmt="s16")
    for chunk in chunks: feed(rs.push(chunk))         # every output whose support has fully arrived
    feed(rs.flush())                                  # the tail; push + flush concatenated == the one-shot result, bit for bit

The kernel is a pure function of (input window, absolute indices), so a stream's state is the last ``ceil(2 half / L)`` input
frames and two counters, kept here.  ``kernel=`` replaces the GPU launch in the GPU-less tests (the numpy restatement of the
same definition): ``kernel(inp [B, frames, channels], in_first [B], in_count [B], out_first [B], n_out, sr_in, sr_out)
-> float32 [B, n_out]``.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _cabi

__all__ = ["plan", "taps", "resample", "StreamResampler", "BatchedResampler", "MAX_ROWS"]

MAX_ROWS = 64          # rows of one tw_resample launch
_FMT = {"f32": (np.float32, _cabi.TW_PCM_F32), "s16": (np.dtype("<i2"), _cabi.TW_PCM_S16)}
_ENCODINGS = {"f32": "f32", "f32le": "f32", "float32": "f32", "s16": "s16", "s16le": "s16", "int16": "s16"}


def _err(lib) -> str:
    msg = lib.tw_last_error(None)
    return msg.decode() if msg else "?"


def plan(sr_in: int, sr_out: int = 16000) -> Tuple[int, int, int, int]:
    """(L, M, half, taps per output) of the (sr_in -> sr_out) plan; ``ValueError`` for a rate pair the library does not support.
    Host arithmetic inside the library: no GPU needed."""
    lib = _cabi.load_library()
    v = [C.c_int32() for _ in range(4)]
    try:
        rc = lib.tw_resample_plan(int(sr_in), int(sr_out), *[C.byref(x) for x in v])
    except (C.ArgumentError, OverflowError, TypeError, ValueError) as e:
        raise ValueError(f"bad sample rate {sr_in!r} -> {sr_out!r}") from e
    if rc != 0:
        raise ValueError(f"unsupported sample rate: {_err(lib)}")
    return tuple(int(x.value) for x in v)


def taps(sr_in: int, sr_out: int = 16000) -> np.ndarray:
    """The 2*half+1 prototype taps in float64, exactly what the device table is rounded from."""
    _, _, half, _ = plan(sr_in, sr_out)
    lib = _cabi.load_library()
    h = np.zeros(2 * half + 1, np.float64)
    rc = lib.tw_resample_taps(int(sr_in), int(sr_out), h.ctypes.data_as(C.POINTER(C.c_double)), len(h))
    if rc != 0:
        raise RuntimeError(f"tw_resample_taps failed ({rc}): {_err(lib)}")
    return h


def normalise_encoding(encoding: str) -> str:
    try:
        return _ENCODINGS[str(encoding).lower()]
    except KeyError:
        raise ValueError(f"unsupported encoding {encoding!r} (f32le or s16le)") from None


def _device_kernel(device: int = 0) -> Callable:
    """The GPU launch with the ``kernel=`` calling contract; returns a DEVICE tensor [B, n_out]."""
    if not torch.cuda.is_available():
        raise RuntimeError("thewhisper_amd.resample needs an MI355X (no CPU fallback)")
    lib = _cabi.load_library()
    dev = torch.device("cuda", int(device))

    def launch(inp, in_first, in_count, out_first, n_out, sr_in, sr_out):
        x = inp if isinstance(inp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(inp))
        if x.dtype not in (torch.float32, torch.int16) or x.dim() != 3:
            raise ValueError(f"expected [rows, frames, channels] float32 or int16, got {tuple(x.shape)} {x.dtype}")
        B, frames, ch = x.shape
        if frames == 0:                       # (a row of nothing still needs an address)
            x = torch.zeros((B, 1, ch), dtype=x.dtype)
        x = x.to(dev).contiguous()
        out = torch.empty((B, int(n_out)), dtype=torch.float32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.tw_resample(dev.index, C.c_void_p(x.data_ptr()), _cabi.TW_PCM_S16 if x.dtype == torch.int16 else _cabi.TW_PCM_F32,
                             ch, x.shape[1], (C.c_int64 * B)(*[int(v) for v in in_first]), (C.c_int32 * B)(*[int(v) for v in in_count]),
                             int(sr_in), int(sr_out), (C.c_int64 * B)(*[int(v) for v in out_first]), int(n_out),
                             C.c_void_p(out.data_ptr()), out.stride(0) if B > 1 else int(n_out), B, C.c_void_p(int(st) if st else None))
        if rc != 0:
            raise RuntimeError(f"tw_resample failed ({rc}): {_err(lib)}")
        return out

    return launch


def _frames(a, channels: Optional[int], fmt: Optional[str] = None):
    """One stream's audio as [frames, channels] float32 / int16 (numpy, or a torch tensor left where it is)."""
    if isinstance(a, (bytes, bytearray, memoryview)):
        if fmt is None:
            raise ValueError("raw bytes need a format")
        a = np.frombuffer(a, dtype=_FMT[fmt][0])
    if isinstance(a, torch.Tensor):
        if a.dtype not in (torch.float32, torch.int16):
            a = a.to(torch.float32)
    else:
        a = np.asarray(a)
        if a.dtype != np.int16:
            a = a.astype(np.float32, copy=False)
    if fmt is not None and str(a.dtype).endswith("int16") != (fmt == "s16"):
        raise ValueError(f"expected {fmt} samples, got {a.dtype}")
    if a.ndim == 1:
        ch = int(channels or 1)
        if a.shape[0] % ch:
            raise ValueError(f"{a.shape[0]} interleaved samples are not a whole number of {ch}-channel frames")
        a = a.reshape(-1, ch)
    elif a.ndim != 2 or (channels is not None and a.shape[1] != channels):
        raise ValueError(f"expected [frames] or [frames, {channels or 'channels'}], got {tuple(a.shape)}")
    if not 1 <= a.shape[1] <= 8:
        raise ValueError(f"{a.shape[1]} channels: 1 to 8 are supported")
    return a


def _pack(windows: Sequence) -> "np.ndarray | torch.Tensor":
    """Rows of different lengths -> one zero-padded [B, frames, channels] block (the kernel reads in_count[b] frames of row b)."""
    n = max(int(w.shape[0]) for w in windows)
    if len(windows) == 1:
        return windows[0][None]
    if any(isinstance(w, torch.Tensor) for w in windows):
        dev = next(w.device for w in windows if isinstance(w, torch.Tensor))
        out = torch.zeros((len(windows), n, windows[0].shape[1]), dtype=torch.as_tensor(windows[0]).dtype, device=dev)
        for b, w in enumerate(windows):
            out[b, : w.shape[0]] = torch.as_tensor(w).to(dev)
        return out
    out = np.zeros((len(windows), n, windows[0].shape[1]), windows[0].dtype)
    for b, w in enumerate(windows):
        out[b, : w.shape[0]] = w
    return out


def resample(audio, sr_in: int, sr_out: int = 16000, kernel: Optional[Callable] = None, device: int = 0):
    """One-shot.  ``audio``: ``[n]`` (mono), ``[n, channels]`` or a list / tuple of such (a batch, rows of any lengths: one
    launch per 64 rows), float32 or int16, numpy or torch, host or device.  Returns float32 of length ``ceil(n L / M)`` per
    row: numpy for host input, a device tensor for device input, a list for a batch."""
    L, M, _, _ = plan(sr_in, sr_out)
    batch = isinstance(audio, (list, tuple))
    items = [_frames(a, None) for a in (audio if batch else [audio])]
    on_device = [isinstance(a, torch.Tensor) and a.is_cuda for a in items]
    run = kernel or _device_kernel(device)
    outs: List = [None] * len(items)
    by_kind = {}
    for i, a in enumerate(items):
        by_kind.setdefault((a.dtype, a.shape[1]), []).append(i)
    for idx in by_kind.values():
        for g in range(0, len(idx), MAX_ROWS):
            grp = idx[g : g + MAX_ROWS]
            n_outs = [-((-int(items[i].shape[0]) * L) // M) for i in grp]
            if max(n_outs) == 0:
                y = np.zeros((len(grp), 0), np.float32)
            else:
                inp = _pack([items[i] for i in grp])
                if kernel is not None and isinstance(inp, torch.Tensor):
                    inp = inp.cpu().numpy()
                y = run(inp, [0] * len(grp), [int(items[i].shape[0]) for i in grp], [0] * len(grp), max(n_outs), sr_in, sr_out)
            for r, i in enumerate(grp):
                o = y[r, : n_outs[r]]
                if on_device[i]:
                    outs[i] = o if isinstance(o, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(o)).to(items[i].device)
                else:
                    outs[i] = np.ascontiguousarray(o.cpu().numpy() if isinstance(o, torch.Tensor) else o, dtype=np.float32)
    return outs if batch else outs[0]


class BatchedResampler:
    """``n_streams`` independent streams of ONE plan and format; ``push`` advances all of them with one launch."""

    def __init__(self, n_streams: int, sr_in: int, sr_out: int = 16000, channels: int = 1, fmt: str = "f32",
                 kernel: Optional[Callable] = None, device: int = 0):
        self.sr_in, self.sr_out, self.channels = int(sr_in), int(sr_out), int(channels)
        self.fmt = normalise_encoding(fmt)
        if not 1 <= self.channels <= 8:
            raise ValueError(f"{channels} channels: 1 to 8 are supported")
        if not 1 <= int(n_streams) <= MAX_ROWS:
            raise ValueError(f"n_streams must be in [1, {MAX_ROWS}]")
        self.L, self.M, self.half, self.taps_per_output = plan(self.sr_in, self.sr_out)
        self.keep = -((-2 * self.half) // self.L)        # ceil(2 half / L) input frames of history per stream
        self.n = int(n_streams)
        self._host = kernel is not None
        self._run = kernel or _device_kernel(device)
        self.launches = 0
        self.reset()

    def reset(self, stream: Optional[int] = None):
        """Back to frame 0 (all streams, or one)."""
        empty = np.zeros((0, self.channels), _FMT[self.fmt][0])
        if stream is None:
            self._hist = [empty] * self.n
            self.frames_in = [0] * self.n      # input frames received
            self.samples_out = [0] * self.n    # output samples emitted
        else:
            self._hist[stream], self.frames_in[stream], self.samples_out[stream] = empty, 0, 0

    def _advance(self, chunks: Sequence, final: bool) -> List[np.ndarray]:
        if len(chunks) != self.n:
            raise ValueError(f"expected {self.n} chunks (None = nothing for that stream), got {len(chunks)}")
        L, M, half = self.L, self.M, self.half
        rows, windows, firsts, n_new = [], [], [], []
        for s, c in enumerate(chunks):
            w = self._hist[s]
            if c is not None:
                c = _frames(c, self.channels, self.fmt)
                if isinstance(c, torch.Tensor):
                    c = c.cpu().numpy()
                if len(c):
                    w = np.concatenate([w, c])
                    self.frames_in[s] += len(c)
            N = self.frames_in[s]
            first = N - len(w)
            # output n reaches input frame floor((n M + half) / L): complete once that is < N; at the end, all ceil(N L / M)
            end = -((-N * L) // M) if final else max(0, (N * L - 1 - half) // M + 1)
            if end > self.samples_out[s]:
                rows.append(s); windows.append(w); firsts.append(first); n_new.append(end - self.samples_out[s])
            self._hist[s] = w[len(w) - min(len(w), self.keep):]
        outs = [np.zeros(0, np.float32) for _ in range(self.n)]
        if rows:
            self.launches += 1
            y = self._run(_pack(windows), firsts, [len(w) for w in windows], [self.samples_out[s] for s in rows], max(n_new),
                          self.sr_in, self.sr_out)
            y = y.cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y, np.float32)
            for r, s in enumerate(rows):
                outs[s] = np.ascontiguousarray(y[r, : n_new[r]], dtype=np.float32)
                self.samples_out[s] += n_new[r]
        return outs

    def push(self, chunks: Sequence) -> List[np.ndarray]:
        """``chunks[s]``: the next frames of stream s (``[n]`` interleaved, ``[n, channels]``, raw bytes, or None).  Returns, per
        stream, every output sample whose support has fully arrived."""
        return self._advance(chunks, False)

    def flush(self) -> List[np.ndarray]:
        """The remaining outputs of every stream (inputs past the end read as zero), up to ``ceil(N L / M)`` in all; the streams
        then start again at frame 0."""
        outs = self._advance([None] * self.n, True)
        self.reset()
        return outs


class StreamResampler:
    """One stream: ``push(chunk) -> np.ndarray`` and ``flush() -> np.ndarray``; their concatenation is bit-identical to
    ``resample`` of the whole input, however it was cut."""

    def __init__(self, sr_in: int, sr_out: int = 16000, channels: int = 1, fmt: str = "f32", kernel: Optional[Callable] = None,
                 device: int = 0):
        self._b = BatchedResampler(1, sr_in, sr_out, channels, fmt, kernel, device)
        self.sr_in, self.sr_out, self.channels, self.fmt = self._b.sr_in, self._b.sr_out, self._b.channels, self._b.fmt
        self.L, self.M, self.half, self.keep = self._b.L, self._b.M, self._b.half, self._b.keep

    @property
    def frames_in(self) -> int:
        return self._b.frames_in[0]

    @property
    def samples_out(self) -> int:
        return self._b.samples_out[0]

    def push(self, chunk) -> np.ndarray:
        return self._b.push([chunk])[0]

    def flush(self) -> np.ndarray:
        return self._b.flush()[0]

    def reset(self):
        self._b.reset()
