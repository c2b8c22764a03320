"""Batched encoder, launch by launch: every launch of one tapped encode (``WhisperEngine.encode_tapped``) at large-v3 width against
the float64 reference of THAT launch (tests/encoder_stage_ref.py) applied to the device's own taps of its inputs, at every row.

Why not more rows in test_gpu_parity.ENC_CASES: one relative L2 over the final hidden state dilutes a wrong output row of M = 7000 to
sqrt(2 / 7000) = 1.7e-2, under the 3e-2 bf16 bound.  The measure here is not diluted: the MAXIMUM over every (row, 64-column block) of
|got - ref|_2 / max(|ref|_2, floor), floor = 0.1 x the stage's median block norm (64 columns = one wavefront's slab = one head); for
attention the blocks are (stream, head, query), for the statistics taps (row, 32-column block) on both numbers.

No bound is fixed by hand.  For each stage and dtype the same measure E_emul is taken on the CPU between the EMULATED reference (the
float64 computation with the format's rounding where the kernels round; float32 contexts: the stage in float32) and the exact one, on
>= 512 rows spread over all tiles (the statistics: on every row); the kernel's bound is 4 x E_emul (summation order, fused
multiply-adds, the hardware 2^x).  Each case also proves through the plan query (tw_gemm_plan / tw_enc_attention_plan) which kernel
and tile height every launch took.

Measured on the MI355X: largest kernel error over the cases of a dtype / the E_emul of that case (largest error : E_emul ratio of
any case), bound 4:
              bf16                          f16                           f32
  conv1       2.86e-3 / 2.71e-3 (1.08)      3.70e-4 / 3.45e-4 (1.12)      1.31e-6 / 6.98e-7 (1.87)
  conv2       2.71e-3 / 2.71e-3 (1.07)      3.18e-4 / 2.80e-4 (1.14)      2.09e-6 / 1.02e-6 (2.04)
  stats_a     9.92e-7 / 3.51e-7 (2.82)      9.99e-7 / 4.21e-7 (2.37)      3.03e-6 / 3.15e-6 (0.96)
  q           3.74e-3 / 3.40e-3 (1.10)      4.52e-4 / 4.45e-4 (1.02)      1.57e-6 / 6.28e-7 (2.50)
  k           3.74e-3 / 3.38e-3 (1.11)      4.73e-4 / 4.34e-4 (1.09)      1.85e-6 / 6.07e-7 (3.04)
  vt          3.72e-3 / 3.49e-3 (1.07)      4.69e-4 / 4.50e-4 (1.07)      1.24e-6 / 6.30e-7 (1.97)
  attention   2.64e-3 / 2.47e-3 (1.07)      3.35e-4 / 3.13e-4 (1.07)      7.60e-7 / 3.52e-7 (2.16)
  out-proj    2.46e-3 / 2.33e-3 (1.07)      3.09e-4 / 2.88e-4 (1.07)      1.08e-6 / 5.51e-7 (1.96)
  stats_b     6.47e-7 / 3.53e-7 (3.18)      8.82e-7 / 4.80e-7 (2.00)      3.18e-6 / 2.38e-6 (1.33)
  fc1         4.90e-3 / 4.49e-3 (1.09)      6.75e-4 / 6.75e-4 (1.06)      2.03e-6 / 8.49e-7 (2.39)
  fc2         2.55e-3 / 2.33e-3 (1.09)      3.09e-4 / 2.94e-4 (1.05)      1.94e-6 / 8.58e-7 (2.27)
  final LN    2.56e-3 / 2.34e-3 (1.09)      3.01e-4 / 2.95e-4 (1.02)      1.84e-7 / 2.07e-7 (0.89)
In 16-bit contexts a block's error IS the one rounding of the stored value (2^-9 / 2^-12 relative per element); the kernels sit on it.

Two findings of the first run, both missing rounding points of the EMULATION, none in a kernel:
  * float32, 500 x 14: conv2 5.2 x, fc2 6.6 x, k 4.1 x a first E_emul that evaluated the stage with the CPU's blocked float32 matrix
    product.  The MFMA GEMM keeps ONE float32 accumulator per output and rounds it after every 4-wide k-step, K / 4 roundings in
    sequence (error ~ sqrt(K / 24) ulp: largest for fc2, K = 5120, and conv2, K = 3840); and the folded LayerNorm forms
    rstd (x W'^T - mean gw) + cb on the raw x, a cancellation the plain sequence does not have (k, q).  The emulation now does both
    (encoder_stage_ref._matmul_t, _ln_linear); the kernels' errors are the 2 - 3 x E_emul above.
  * the statistics, bf16 500 x 14: 6.4 x an E_emul taken on 640 sampled rows.  The measure is a maximum over 280000 sums whose worst
    cases cancel down to the floor; on every row E_emul is 2 - 4 x the sampled one.  It is now taken on every row.
"""
import math
import os

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import encoder_stage_ref as R
from tests.util import KINDS, clips, dims_variant, make_engine

pytestmark = pytest.mark.gpu

DIMS = dims_variant("large-v3", enc_layers=1, dec_layers=0)
D, H, F, NMEL = DIMS.d_model, DIMS.heads, DIMS.ffn, DIMS.n_mels
K1 = (1, 128)

# (T, B, dtype): what it is for, and the (kernel, tile height) every launch must take: conv1 | N = 1280 (conv2, out-proj, fc2) | QKV |
# fc1 | queries per attention workgroup
CASES = [
    # M = 7000: N = 1280 at 80 rows with a ragged last tile (7000 = 87 * 80 + 40), QKV and fc1 at 112 (ragged), conv1 at 96, the
    # 128-query attention with nbh = 280; the f32 run is the only strict-f32 coverage of kernel 2
    (500, 14, "bf16", ((2, 96), (2, 80), (2, 112), (2, 112), 128)),
    (500, 14, "f16", ((2, 96), (2, 80), (2, 112), (2, 112), 128)),
    (500, 14, "f32", ((2, 96), (2, 80), (2, 112), (2, 112), 64)),
    # the benchmark's shape: N = 1280 at 80 without a ragged tile, QKV and fc1 at 128, conv1 at 112
    (500, 16, "bf16", ((2, 112), (2, 80), (2, 128), (2, 128), 128)),
    # N = 1280 at 96; T % 4 = 2: the V segment takes the plain epilogue inside kernel 2; T no multiple of 64: a Tp pad
    (1250, 7, "bf16", ((2, 128), (2, 96), (2, 112), (2, 128), 128)),
    # M = 2500: QKV at 80 (MT = 5: the odd trailing chunk of the staged epilogues); nbh = 100: a padded attention grid
    (500, 5, "f16", (K1, K1, (2, 80), (2, 112), 64)),
    # M = 3000: QKV at 96
    (500, 6, "bf16", (K1, K1, (2, 96), (2, 128), 64)),
    # every 80-row tile spans two or three clips, T % 4 = 2; 128-query attention with fewer queries than a block, fewer keys than a tile
    (50, 50, "bf16", (K1, K1, (2, 80), (2, 112), 128)),
    # M = 3200, QKV at 96; Bmax at its limit
    (50, 64, "f16", (K1, K1, (2, 96), (2, 128), 128)),
    # the out-projection, fc2 and conv2 on the two remaining tile heights
    (500, 20, "bf16", ((2, 112), (2, 112), (2, 128), (2, 128), 128)),
    (500, 24, "bf16", ((2, 128), (2, 128), (2, 128), (2, 128), 128)),
    # fc1 (row-major + GELU) on 80-row tiles: M = 2000 = 25 * 80
    (500, 4, "bf16", (K1, K1, K1, (2, 80), 64)),
]
OVERRUN_CASES = [(500, 14, "bf16"), (50, 50, "bf16")]

_TW = {"f32": 0, "bf16": 1, "f16": 2}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))     # the float64 references are a handful of M x 1280 x 5120 products
    yield
    torch.set_num_threads(n)
    _cache.clear()


def _weights():
    if "w" not in _cache:
        _cache["w"] = wo.make_weights(DIMS, 1)
    return _cache["w"]


def _stage_weights(T, dtype):
    if ("W", T, dtype) not in _cache:
        _cache[("W", T, dtype)] = R.StageWeights(_weights(), DIMS, T, dtype)
    return _cache[("W", T, dtype)]


def _mel(T, B, seed0=0):
    pcm = np.stack([wo.synth_audio(T * 320, seed=seed0 + i, kind=KINDS[i % len(KINDS)]) for i in range(B)])
    if seed0 == 0:
        assert np.array_equal(pcm, clips(T * 320, B))   # the clips of test_gpu_parity.test_encoder
    return wo.log_mel(pcm, NMEL)


def plans(T, B, dtype):
    """What the library's dispatch picks for the launches of one encode, by the plan query."""
    from thewhisper_amd import _cabi as cabi

    dt, M = _TW[dtype], T * B
    n1280 = cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, D, D)
    assert n1280 == cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, D, 3 * D) == cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, D, F)
    return (cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, 2 * M, D, 3 * NMEL), n1280, cabi.gemm_plan(dt, cabi.TW_EPI_QKV_ENC, M, 3 * D, D),
            cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, F, D), cabi.enc_attention_plan(dt, B, H, T)[0])


def _sample(n_rows, n=640):
    """>= 512 rows spread evenly: with at most 24000 rows and tiles of >= 64 rows every tile has one."""
    return torch.unique(torch.linspace(0, n_rows - 1, min(n, n_rows)).round().long())


def check_stages(taps, mel, T, B, dtype):
    """taps: CPU float64 tensors in the layouts of encode_tapped (Bm >= B clips).  Returns {stage: (kernel error, E_emul)} over every
    launch, every element; raises on the conditions that are not measurements."""
    W = _stage_weights(T, dtype)
    M, Tp = B * T, W.Tp
    out = {}

    def gemm_stage(name, got, ref, emu_rows, rows, block=64):
        fl = R.norm_floor(ref, block)
        out[name] = (R.block_error(got, ref, fl, block), R.block_error(emu_rows, ref.reshape(-1, ref.shape[-1])[rows], fl, block))

    def stats_stage(name, got, x):
        # (emulated on EVERY row, which costs nothing here: the measure is a maximum over 40 M sums whose worst cases are those that
        #  cancel down to the floor, and a sample of rows misses them - on 640 rows E_emul came out 2 - 4 x smaller than on all)
        ref = R.block_stats(x)
        fl = R.stats_floor(ref)
        out[name] = (R.stats_error(got, ref, fl), R.stats_error(R.block_stats(x, dtype), ref, fl))

    mel_t = R.round_to(torch.from_numpy(mel).to(torch.float64), dtype)     # (mel_transpose rounds the float32 features to T)
    # conv1 + GELU: the padded layout, pad rows included
    h1 = taps["h1"][:B]
    ref = R.conv1_gelu(mel_t, W)
    rows = _sample(2 * M)
    fl = R.norm_floor(ref[:, 1:-1])
    out["conv1"] = (R.block_error(h1, ref, fl), R.block_error(R.conv1_gelu(mel_t, W, dtype, rows=rows), ref[:, 1:-1].reshape(2 * M, D)[rows], fl))
    assert not h1[:, 0].any() and not h1[:, -1].any(), "conv1 wrote into the pad rows conv2 reads as zeros"
    # conv2 + GELU + positions, from the device's h1
    rows = _sample(M)
    xa = taps["xa_in"][:M]
    gemm_stage("conv2", xa, R.conv2_gelu_pos(h1, W), R.conv2_gelu_pos(h1, W, dtype, rows=rows), rows)
    stats_stage("stats_a", taps["ln_stats_a"][:M], xa)
    # LayerNorm + QKV
    ref = R.ln_qkv_rows(xa, W)
    emu = R.ln_qkv_rows(xa[rows], W, dtype).reshape(len(rows), 3, H, 64)
    rq, rk, rvt = R.split_qkv(ref, B, T, H, Tp)
    refs = ref.reshape(M, 3, H, 64)[rows]
    q, k, vt = taps["q"][:B], taps["k"][:B], taps["vt"][:B]
    for i, (name, got, full) in enumerate((("q", q, rq), ("k", k, rk), ("vt", vt[..., :T].transpose(-1, -2), rvt[..., :T].transpose(-1, -2)))):
        fl = R.norm_floor(full)
        out[name] = (R.block_error(got, full, fl), R.block_error(emu[:, i], refs[:, i], fl))
    assert not taps["vt"][..., T:].any(), "V^T keys [T, Tp) must stay exactly zero: the attention kernel reads them"
    # attention, from the device's q, k, vt
    attn = taps["attn"][:M]
    ref = R.attention(q, k, vt, T)
    bs = torch.unique(torch.linspace(0, B - 1, min(B, max(2, math.ceil(512 / T)))).round().long())
    emu = R.attention(q[bs], k[bs], vt[bs], T, dtype)
    fl = R.norm_floor(ref)
    out["attn"] = (R.block_error(attn, ref, fl), R.block_error(emu, ref.reshape(B, T, D)[bs].reshape(-1, D), fl))
    # out-projection + residual
    xb = taps["xb"][:M]
    gemm_stage("out_proj", xb, R.out_proj_residual(attn, xa, W), R.out_proj_residual(attn[rows], xa[rows], W, dtype), rows)
    stats_stage("stats_b", taps["ln_stats_b"][:M], xb)
    # LayerNorm + fc1 + GELU
    ffnh = taps["ffnh"][:M]
    gemm_stage("fc1", ffnh, R.ln_fc1_gelu(xb, W), R.ln_fc1_gelu(xb[rows], W, dtype), rows)
    # fc2 + residual
    xo = taps["xa_out"][:M]
    gemm_stage("fc2", xo, R.fc2_residual(ffnh, xb, W), R.fc2_residual(ffnh[rows], xb[rows], W, dtype), rows)
    # the final LayerNorm
    gemm_stage("final_ln", taps["enc_out"][:M], R.final_layer_norm(xo, W), R.final_layer_norm(xo[rows], W, dtype), rows)
    return out


def _tapped(eng, mel):
    hidden, taps = eng.encode_tapped(torch.from_numpy(mel).cuda())
    torch.cuda.synchronize()
    return hidden, taps


@pytest.mark.parametrize("T,B,dtype,want", CASES, ids=[f"{T}x{B}-{dt}" for T, B, dt, _ in CASES])
def test_every_launch_against_its_float64_reference(T, B, dtype, want):
    assert plans(T, B, dtype) == want      # the launches of this case reach the kernels and tile heights it is here for
    eng = make_engine(DIMS, _weights(), T=T, max_batch=B, dtype=dtype)
    mel = _mel(T, B)
    hidden, taps = _tapped(eng, mel)
    plain = eng.encode(torch.from_numpy(mel).cuda(), return_hidden=True)
    torch.cuda.synchronize()
    eng.close()
    assert torch.equal(hidden, plain), "the tapped encode is the plain encode"
    assert torch.equal(hidden.reshape(B * T, D), taps["enc_out"].float()), "the hidden state is the enc_out tap"
    res = check_stages({k: v.cpu().to(torch.float64) for k, v in taps.items()}, mel, T, B, dtype)
    bad = []
    for name, (err, e_emul) in res.items():
        print(f"STAGE {T}x{B} {dtype} {name:9s} kernel {err:.3e}  E_emul {e_emul:.3e}  ratio {err / max(e_emul, 1e-300):.2f}")
        if not err <= 4.0 * e_emul:
            bad.append((name, err, e_emul))
    assert not bad, f"stages over 4 x E_emul: {bad}"


@pytest.mark.parametrize("T,B,dtype", OVERRUN_CASES)
def test_no_launch_writes_past_its_rows(T, B, dtype):
    """A context for B + 1 clips: encode B + 1 clips, then B other clips; what the first run left in the rows of clip B must survive
    the second bit for bit, in every tapped buffer (a ragged last tile that writes past M would not leave it)."""
    eng = make_engine(DIMS, _weights(), T=T, max_batch=B + 1, dtype=dtype)
    _, first = _tapped(eng, _mel(T, B + 1))
    _, second = _tapped(eng, _mel(T, B, seed0=100))
    eng.close()
    for name, a in first.items():
        # the residual buffer is written twice per encode: what the second run's layer input finds past its rows is the first run's
        # layer OUTPUT (one layer: the statistics of the input are written once, by conv2)
        a = first["xa_out"] if name == "xa_in" else a
        a, b = a.reshape(B + 1, -1), second[name].reshape(B + 1, -1)
        assert not torch.equal(first[name].reshape(B + 1, -1)[:B], b[:B]), name      # (other clips: the rows in use did change)
        assert torch.equal(a[B:].view(torch.uint8), b[B:].view(torch.uint8)), f"{name}: rows >= M changed"


def test_every_tile_height_is_covered_for_each_epilogue_kind():
    """If the dispatch is retuned, this says which coverage went instead of losing it silently."""
    seen = set()
    for T, B, dtype, _ in CASES:
        conv1, n1280, qkv, fc1, _ = plans(T, B, dtype)
        seen |= {("rowmajor+gelu",) + conv1, ("rowmajor+gelu",) + fc1, ("qkv_enc",) + qkv, ("rowmajor+residual+stats",) + n1280}
    missing = [(kind, 2, bm) for kind in ("qkv_enc", "rowmajor+residual+stats", "rowmajor+gelu") for bm in (80, 96, 112, 128)
               if (kind, 2, bm) not in seen]
    assert not missing, f"kernel-2 tile heights no case reaches: {missing}"
    # ... and in strict f32, the 64- and 128-query attention, a ragged and an exact last tile
    assert any(dt == "f32" and plans(T, B, dt)[2][0] == 2 for T, B, dt, _ in CASES)
    assert {plans(T, B, dt)[4] for T, B, dt, _ in CASES} == {64, 128}
    n1280_bm = {(T * B) % plans(T, B, dt)[1][1] == 0 for T, B, dt, _ in CASES if plans(T, B, dt)[1][0] == 2}
    assert n1280_bm == {True, False}
