"""TESTS ONLY: numpy restatement, in float64, of the resampler defined in thewhisper_amd/csrc/k_resample.hip.

    g = gcd(sr_in, sr_out)   L = sr_out / g   M = sr_in / g   F = max(L, M)   half = Z F   fc = RHO / F
    h[j] = L fc sinc(fc j) I0(BETA sqrt(1 - (j / half)^2)) / I0(BETA)        j = -half .. half
    x[k] = mean over the channels of frame k in float32 (channels added in order; int16 is v / 32767 first)
    y[n] = sum_k x[k] h[n M - k L]                                             x[k] = 0 outside [0, N)

``rows`` has the calling contract of the device kernel (a pure function of the input window and the absolute indices), so it
is what the GPU-less tests inject as ``kernel=``; ``resample`` is the one-shot form.  The sum runs over k in ascending order
with the zeros included, one product at a time, so a sample's bits do not depend on how a stream was cut.  Pinned to
``scipy.signal.resample_poly(x, L, M, window=h / L)`` in tests/test_resample.py.
"""
import math

import numpy as np

Z, BETA, RHO = 16, 8.6, 0.945
MAX_TAPS = 1 << 18
RATES = (8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 88200, 96000)


def plan(sr_in, sr_out=16000):
    """(L, M, half, taps per output)."""
    if sr_in < 4000 or sr_out < 4000:
        raise ValueError("sample rates must be >= 4000 Hz")
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    if L == M == 1:
        return 1, 1, 0, 1
    half = Z * max(L, M)
    if 2 * half + 1 > MAX_TAPS:
        raise ValueError("table too large")
    return L, M, half, 2 * half // L + 1


def taps(sr_in, sr_out=16000):
    L, M, half, _ = plan(sr_in, sr_out)
    if half == 0:
        return np.ones(1)
    j = np.arange(-half, half + 1, dtype=np.float64)
    fc = RHO / max(L, M)
    return L * fc * np.sinc(fc * j) * np.i0(BETA * np.sqrt(np.maximum(0.0, 1.0 - (j / half) ** 2))) / np.i0(BETA)


def to_mono_f32(x):
    """[..., frames, channels] float32 or int16 -> [..., frames] float32, as the kernel converts and down-mixes."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        x = x.astype(np.float32) / np.float32(32767.0)
    x = x.astype(np.float32, copy=False)
    s = x[..., 0].copy()
    for c in range(1, x.shape[-1]):
        s = s + x[..., c]
    return s / np.float32(x.shape[-1]) if x.shape[-1] > 1 else s


def rows(inp, in_first, in_count, out_first, n_out, sr_in, sr_out=16000, dtype=np.float32):
    """inp: [B, frames, channels]; row b holds in_count[b] frames starting at absolute frame in_first[b]; returns [B, n_out],
    outputs out_first[b] .. out_first[b] + n_out - 1 of every row."""
    L, M, half, tpo = plan(sr_in, sr_out)
    h = taps(sr_in, sr_out)
    x = to_mono_f32(inp).astype(np.float64)
    B = x.shape[0]
    out = np.zeros((B, n_out), np.float64)
    for b in range(B):
        n = int(out_first[b]) + np.arange(n_out, dtype=np.int64)
        c = n * M
        klo = -((half - c) // L)                 # ceil((c - half) / L)
        khi = (c + half) // L
        acc = np.zeros(n_out, np.float64)
        for j in range(tpo):
            k = klo + j
            t = c - k * L + half
            rel = k - int(in_first[b])
            ok = (k <= khi) & (k >= 0) & (rel >= 0) & (rel < int(in_count[b]))
            xv = np.where(ok, x[b, np.clip(rel, 0, max(x.shape[1] - 1, 0))] if x.shape[1] else 0.0, 0.0)
            hv = np.where(k <= khi, h[np.clip(t, 0, 2 * half)], 0.0)
            acc = acc + xv * hv
        out[b] = acc
    return out.astype(dtype)


def resample(x, sr_in, sr_out=16000, dtype=np.float64):
    """One-shot: x [n] or [n, channels] (float32 / int16) -> [ceil(n L / M)]."""
    x = np.asarray(x)
    if x.ndim == 1:
        x = x[:, None]
    L, M, _, _ = plan(sr_in, sr_out)
    n_out = -((-x.shape[0] * L) // M)
    if n_out == 0:
        return np.zeros(0, dtype)
    return rows(x[None], [0], [x.shape[0]], [0], n_out, sr_in, sr_out, dtype)[0]
