"""The MXFP8 encoder GEMM (k_gemm_w8.hip: gemm_w8reg_kernel) launch by launch at large-v3 width: the instrument of
tests/test_gpu_encoder_stages.py - one tapped encode, every launch against the float64 reference of THAT launch on the device's own input
taps, the undiluted measure max over (row, 64-column block), bound 4 x E_emul taken on the CPU from the reference alone - in an
"fp8f16full" context (TW_F16_W8A16_FULL), whose references are tests/encoder_stage_ref.py's weight format "fp8f16full".

What the micro models of tests/test_gpu_fp8_encoder.py leave open and the cases here close: the 80 x 256 instantiation (4 wavefronts,
AV = 3) with more than one K tile - K = 1280 is 20 K tiles and 10 scale pairs, fc2's K = 5120 is 80 and 40, so the scale pair advances,
the three-stage activation ring wraps and the tail clamps are the end of a loop instead of all of it - at N = 1280, 3840 and 5120 (and,
in the on-grid test, the cross-K/V projection's 2560), with a ragged 80-row last tile, the out-projection and fc2 with their residual +
statistics epilogue at 80 rows, and K = 5120 on the two-wavefront 64 x 128 kernel.

  (a) test_every_fp8_launch_against_its_float64_reference: make_weights tensors, off the fp8 grid, the block scales of the quantised
      matrices spread over three values (below).  The exact reference of the two
      LayerNorm-folded launches is the context's algebra rstd (x Wq^T - mean gw) + cb in float64 (encoder_stage_ref._ln_linear_w8);
      E_emul is float16's - one rounding of the stored value: the weights a row sees are float16 values already.
  (b) test_no_fp8_launch_writes_past_its_rows: rows >= M keep their bits (a ragged 80-row tile: AV = 3 requests rows past the tile).
  (c) test_bits_on_grid_weights_at_real_width: weights ON the fp8 grid (tests/test_gpu_fp8_encoder.put_on_grid), where the quantiser is
      the identity: every tap equals the plain "f16" context's bit for bit, and - the cross-K/V projection has no tap - the logits of one
      decode step equal the "fp8f16" context's, which projects cross K/V with the 16-bit kernel.

Measured on the MI355X (profiles/r30_fp8_encoder_stages.log): the largest kernel error : E_emul ratio of any case of (a) per stage (bound 4),
with that case and its kernel error / E_emul.  The four MXFP8 launches (q | k | vt, out-proj, fc1, fc2) sit on the one float16 rounding of
the stored value, where the float16 kernels sit; the statistics are float32 sums, as there.
  conv1       1.14   500x16   3.699e-4 / 3.249e-4        attention   1.11   500x14   3.409e-4 / 3.084e-4
  conv2       1.14   500x14   3.184e-4 / 2.805e-4        out-proj    1.09   500x14   3.145e-4 / 2.898e-4
  stats_a     2.50   64x8     9.852e-7 / 3.941e-7        stats_b     2.55   500x1    5.645e-7 / 2.212e-7
  q           1.04   100x64   3.207e-4 / 3.096e-4        fc1         1.06   500x14   3.829e-4 / 3.615e-4
  k           1.04   50x50    3.032e-4 / 2.923e-4        fc2         1.06   50x50    3.154e-4 / 2.988e-4
  vt          1.07   100x64   3.278e-4 / 3.070e-4        final LN    1.13   500x16   3.376e-4 / 2.997e-4
(c): the largest magnitude of any tap of the on-grid model's float64 reference is 45 (the layer's output), 8.1 in the cross K | V projection.

Two findings on the way, none in a kernel:
  * The weights of (a).  A library whose K loop fetched the scale pair of the PREVIOUS two K tiles passed the first version of (a) with
    every figure unchanged: wo.make_weights draws a matrix uniformly in +-1.7 / sqrt(K), and at K = 1280 / 5120 the largest of a block's
    32 values misses its binade once in 1.5e-6, so every scale byte of a matrix is the same.  (a) now spreads the blocks by 2^-1, 2^0, 2^1
    (encoder_stage_ref.spread_block_scales, pinned on the CPU in tests/test_encoder_stage_ref.py); the same library then gives
    q, k, vt, out-proj, fc1 and fc2 errors of 0.8 - 1.5, 2600 - 4200 x E_emul, and (c) finds 17 M differing bytes in the q tap.
  * The float64 reference of tests/test_gpu_fp8_encoder.py (RefFull) was 1.4e-7 - 3.9e-7 off the composed stage references: see
    tests/test_encoder_stage_ref.py.
"""
import functools
import os

import pytest
import torch

from oracle import whisper_oracle as wo
from tests import encoder_stage_ref as R
from tests import test_gpu_encoder_stages as S
from tests.test_gpu_fp8_encoder import put_on_grid
from tests.util import PROMPT, dims_variant, make_engine

pytestmark = pytest.mark.gpu

D, F, H = S.D, S.F, S.H
FMT = "fp8f16full"
K64, K80 = (3, 64), (3, 80)

# (T, B): what it is for, and the tile of N = 1280 (out-projection, fc2) | QKV | fc1.  conv1, conv2, attention and the final LayerNorm are
# the float16 kernels, measured along the way.
CASES = [
    # M = 7000 = 87 * 80 + 40: all four linears at 80 x 256 with a ragged last tile; fc2 runs 80 K tiles; out-projection and fc2 write statistics
    (500, 14, (K80, K80, K80)),
    # the benchmark's shape: exact 80-row tiles
    (500, 16, (K80, K80, K80)),
    # M = 2000: fc1 at 80 (exact); QKV, out-projection and fc2 at 64 x 128 with a ragged tile (31 * 64 + 16), fc2's K = 5120 on two wavefronts
    (500, 4, (K64, K64, K80)),
    # one stream: M = 500 = 7 * 64 + 52, everything at 64 x 128
    (500, 1, (K64, K64, K64)),
    # M = 2500: QKV and fc1 at 80 (31 * 80 + 20), tiles spanning two or three clips; T % 4 = 2: the V segment takes the plain epilogue;
    # N = 1280 at 64 (39 * 64 + 4)
    (50, 50, (K64, K80, K80)),
    # max_batch at its limit: M = 6400, QKV and fc1 at 80 exact, N = 1280 at 64 exact
    (100, 64, (K64, K80, K80)),
    # M = 512 = 8 * 64: QKV and fc1 at 64 with an exact last tile (no other case has one)
    (64, 8, (K64, K64, K64)),
]
OVERRUN_CASES = [(500, 14), (50, 50)]
GRID_CASES = [
    # M = 3500: cross K/V (N = 2560), QKV and fc1 at 80; N = 1280 at 64
    (500, 7, (K64, K80, K80, K80)),
    # M = 7000: all at 80, ragged
    (500, 14, (K80, K80, K80, K80)),
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))     # the float64 references are a handful of M x 1280 x 5120 products
    yield
    torch.set_num_threads(n)
    S._cache.clear()
    grid_model.cache_clear()
    grid_reference.cache_clear()


def plans(T, B):
    """Tile of every MXFP8 launch of one encode + cross K/V, by the plan query: N = 1280 | QKV | fc1 | cross K/V."""
    from thewhisper_amd import _cabi as cabi

    dt, M = cabi.TW_F16_W8A16_FULL, T * B
    n1280 = cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, D, D)
    assert n1280 == cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, D, F)
    return (n1280, cabi.gemm_plan(dt, cabi.TW_EPI_QKV_ENC, M, 3 * D, D), cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, F, D),
            cabi.gemm_plan(dt, cabi.TW_EPI_KV_CROSS, M, 2 * D, D))


@pytest.mark.parametrize("T,B,want", CASES, ids=[f"{T}x{B}" for T, B, _ in CASES])
def test_every_fp8_launch_against_its_float64_reference(T, B, want):
    assert plans(T, B)[:3] == want      # the launches of this case reach the tiles it is here for
    S.check_every_launch(T, B, FMT)


@pytest.mark.parametrize("T,B", OVERRUN_CASES)
def test_no_fp8_launch_writes_past_its_rows(T, B):
    assert plans(T, B)[1:3] == (K80, K80) and (T * B) % 80 != 0
    S.check_no_launch_writes_past_its_rows(T, B, FMT)


def test_both_tiles_are_covered_for_each_epilogue_kind():
    """If the dispatch is retuned, this says which coverage went instead of losing it silently: every epilogue kind of the MXFP8 GEMM
    at 64 x 128 and at 80 x 256, each with a ragged and with an exact last tile."""
    seen = set()
    for T, B, _ in CASES:
        n1280, qkv, fc1, _ = plans(T, B)
        for kind, (kernel, bm) in (("rowmajor+residual+stats", n1280), ("qkv_enc", qkv), ("rowmajor+gelu", fc1)):
            seen.add((kind, kernel, bm, (T * B) % bm == 0))
    missing = [(kind, 3, bm, exact) for kind in ("qkv_enc", "rowmajor+gelu", "rowmajor+residual+stats") for bm in (64, 80)
               for exact in (False, True) if (kind, 3, bm, exact) not in seen]
    assert not missing, f"(epilogue kind, kernel, tile height, exact last tile) no case reaches: {missing}"
    # fc2's K = 5120 (80 K tiles, 40 scale pairs) on both instantiations, ragged at 80
    assert {plans(T, B)[0] for T, B, _ in CASES} == {K64, K80}
    assert all(plans(T, B) == want for T, B, want in GRID_CASES)


# ---- (c) weights on the fp8 grid --------------------------------------------------------------------------------------------------
GRID_DIMS = dims_variant("large-v3", enc_layers=1, dec_layers=1)
# Element exponents j of put_on_grid: its micro models take j in [-4, 5).  At K = 1280 / 5120 the same range keeps the composed float64
# reference far below the bound of grid_reference (the largest tap is printed by the test), so it is kept; the block scales are
# put_on_grid's three distinct values 2^-12, 2^-11, 2^-10 per matrix, which must not be narrowed: they are what a wrong scale byte shows on.
GRID_ELEM_EXP = (-4, 5)


@functools.lru_cache(maxsize=None)
def grid_model():
    return put_on_grid(GRID_DIMS, wo.make_weights(GRID_DIMS, 2), elem_exp=GRID_ELEM_EXP)


@functools.lru_cache(maxsize=None)
def grid_reference(T, B):
    """The largest magnitude of any tap (and of the cross K | V projection) in the composed float64 reference of the on-grid model over
    the B clips - the precondition of a bit comparison: no NaN, no Inf, nothing near the float16 maximum."""
    w = grid_model()
    W = R.StageWeights(w, GRID_DIMS, T, "f16")      # on the grid the quantiser is the identity (put_on_grid), gains 1.0: and so is the fold
    mel = R.round_to(torch.from_numpy(S._mel(T, B)).double(), "f16")
    # (float64 GELU of a very negative number is a denormal, and a matrix product over denormals runs several times slower: they are
    #  flushed to zero, which no maximum notices)
    flush = lambda t: t * (t.abs() >= 2.0 ** -1022)   # noqa: E731
    taps = {"h1": flush(R.conv1_gelu(mel, W))}
    x = taps["xa_in"] = R.conv2_gelu_pos(taps["h1"], W)
    taps["q"], taps["k"], taps["vt"] = R.ln_qkv(x, W, B)
    taps["attn"] = R.attention(taps["q"], taps["k"], taps["vt"], T)
    xb = taps["xb"] = R.out_proj_residual(taps["attn"], x, W)
    taps["ffnh"] = flush(R.ln_fc1_gelu(xb, W))
    xo = taps["xa_out"] = R.fc2_residual(taps["ffnh"], xb, W)
    enc = taps["enc_out"] = R.final_layer_norm(xo, W)
    p = "model.decoder.layers.0.encoder_attn."
    taps["cross_kv"] = enc @ torch.cat([R._t(w[p + "k_proj.weight"]), R._t(w[p + "v_proj.weight"])]).T
    assert all(bool(torch.isfinite(t).all()) for t in taps.values())
    return {k: float(t.abs().max()) for k, t in taps.items()}


def _grid_run(dtype, T, B, mel, tapped):
    eng = make_engine(GRID_DIMS, grid_model(), T=T, max_batch=B, dtype=dtype)
    try:
        if tapped:
            _, taps = S._tapped(eng, mel)
        else:
            taps = None
            eng.encode(torch.from_numpy(mel).cuda())
        n = min(B, 16)      # (a decode step takes at most 16 rows at this ffn: tests/test_gpu_fp8_encoder.run)
        eng.cross_kv(B)
        eng.decoder_reset(n)
        logits = eng.decode_step([PROMPT[0]] * n)
        torch.cuda.synchronize()
        return taps, logits
    finally:
        eng.close()


@pytest.mark.parametrize("T,B,want", GRID_CASES, ids=[f"{T}x{B}" for T, B, _ in GRID_CASES])
def test_bits_on_grid_weights_at_real_width(T, B, want):
    """Layout, scale indexing over 10 and 40 scale pairs, widening, K order and every epilogue at 80 x 256: on weights that lie on the
    fp8 grid every launch of the encoder gives the bits of the float16 kernels (k_gemm_w8.hip's header: whatever the tile height), and
    the logits behind the MXFP8 cross-K/V projection are those behind the 16-bit one.  Element exponents: GRID_ELEM_EXP; the three
    distinct block scales per matrix are put_on_grid's."""
    assert plans(T, B) == want
    # precondition, on the CPU: the float64 model keeps every tap finite and below a quarter of the float16 maximum
    # (computed once, over the clips of the largest case of this T: those of a smaller case are its first ones)
    Bref = max(b for t, b, _ in GRID_CASES if t == T)
    amax = grid_reference(T, Bref)
    print(f"GRID {T}x{Bref} largest magnitude per tap of the float64 reference: " + "  ".join(f"{k} {v:.3g}" for k, v in amax.items()))
    assert all(v < 65504.0 / 4 for v in amax.values()), amax
    mel = S._mel(T, B)
    new_taps, new_logits = _grid_run(FMT, T, B, mel, True)
    f16_taps, _ = _grid_run("f16", T, B, mel, True)
    _, old_logits = _grid_run("fp8f16", T, B, mel, False)
    assert set(new_taps) == set(f16_taps) and len(new_taps) == 12
    for name in new_taps:
        a, b = new_taps[name].contiguous().view(torch.uint8), f16_taps[name].contiguous().view(torch.uint8)
        assert torch.equal(a, b), f"tap {name}: {int((a != b).sum())} bytes differ from the float16 context's"
    assert bool(torch.isfinite(new_logits).all()) and float(new_logits.std()) > 0
    assert torch.equal(new_logits.view(torch.int32), old_logits.view(torch.int32)), "decode-step logits behind the MXFP8 cross K/V projection"
