"""The per-launch encoder references (tests/encoder_stage_ref.py) checked on the CPU: composed they are the float64 oracle, and a
hand-built case pins the head-split / transposed layouts and the measure.  (The judge / test_judge pattern: the GPU test trusts
these functions, so they are tested where no GPU is needed.)"""
import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import encoder_stage_ref as R
from tests.util import clips, dims_variant


def _compose(mel, w, dims, T, B, emul=None, dtype="f64"):
    Ws = [R.StageWeights(w, dims, T, dtype, layer=i) for i in range(dims.enc_layers)]
    x = R.conv2_gelu_pos(R.conv1_gelu(torch.from_numpy(mel), Ws[0], emul), Ws[0], emul)
    for W in Ws:
        q, k, vt = R.ln_qkv(x, W, B, emul)
        xb = R.out_proj_residual(R.attention(q, k, vt, T, emul), x, W, emul)
        x = R.fc2_residual(R.ln_fc1_gelu(xb, W, emul), xb, W, emul)
    return R.final_layer_norm(x, Ws[0], emul).reshape(B, T, -1).numpy()


@pytest.mark.parametrize("preset", ["micro", "micro80"])
@pytest.mark.parametrize("T", [50, 100])
def test_composed_stages_are_the_float64_oracle(preset, T):
    dims = dims_variant(preset, dec_layers=0)
    assert dims.enc_layers == 2
    w = wo.make_weights(dims, 1)
    B = 2
    mel = wo.log_mel(clips(T * 320, B), dims.n_mels)
    ref = wo.OracleWhisper(dims, w, T=T, dtype=np.float64).encode(mel)
    got = _compose(mel, w, dims, T, B)
    assert np.linalg.norm(got - ref) / np.linalg.norm(ref) < 1e-12
    assert np.abs(got - ref).max() < 1e-12 * np.abs(ref).max() * 100
    # the emulated variants are the same computation up to the format's rounding: close, and not identical
    for emul, lo, hi in (("f32", 1e-8, 1e-5), ("f16", 1e-5, 4e-3), ("bf16", 1e-4, 3e-2)):
        e = _compose(mel, w, dims, T, B, emul, emul)
        rel = np.linalg.norm(e - ref) / np.linalg.norm(ref)
        assert lo < rel < hi, (emul, rel)


def test_rows_argument_selects_rows_of_the_full_result():
    dims = dims_variant("micro", dec_layers=0)
    w = wo.make_weights(dims, 1)
    T, B = 50, 2
    W = R.StageWeights(w, dims, T, "bf16")
    mel = R.round_to(torch.from_numpy(wo.log_mel(clips(T * 320, B), dims.n_mels)).double(), "bf16")
    rows = torch.tensor([0, 1, 99, 100, 199])
    for emul in (None, "bf16"):
        h1 = R.conv1_gelu(mel, W, emul)
        assert h1.shape == (B, 2 * T + 2, dims.d_model) and not h1[:, 0].any() and not h1[:, -1].any()
        assert torch.allclose(R.conv1_gelu(mel, W, emul, rows=rows), h1[:, 1:-1].reshape(B * 2 * T, -1)[rows], rtol=0, atol=1e-12)
        xa = R.conv2_gelu_pos(h1, W, emul)
        assert torch.allclose(R.conv2_gelu_pos(h1, W, emul, rows=rows[:3]), xa[rows[:3]], rtol=0, atol=1e-12)


def test_three_row_case_pins_the_layouts():
    """B = 1, T = 3, H = 2 by hand: row t of the projection is q | k | v, each H x 64 wide."""
    T, H, Tp = 3, 2, 64
    y = torch.arange(T * 3 * H * 64, dtype=torch.float64).reshape(T, 3 * H * 64)
    q, k, vt = R.split_qkv(y, 1, T, H, Tp)
    assert q.shape == (1, H, T, 64) and k.shape == (1, H, T, 64) and vt.shape == (1, H, 64, Tp)
    for t in range(T):
        for h in range(H):
            for dd in (0, 1, 63):
                assert q[0, h, t, dd] == y[t, h * 64 + dd]
                assert k[0, h, t, dd] == y[t, H * 64 + h * 64 + dd]
                assert vt[0, h, dd, t] == y[t, 2 * H * 64 + h * 64 + dd]
    assert not vt[..., T:].any()
    # two streams: stream b owns rows b * T ..
    y2 = torch.cat([y, y + 10000.0])
    q2, _, vt2 = R.split_qkv(y2, 2, T, H, Tp)
    assert q2[1, 1, 2, 5] == y[2, 64 + 5] + 10000.0 and vt2[1, 0, 7, 1] == y[1, 2 * H * 64 + 7] + 10000.0
    # attention on it: one-hot values make the output the softmax weights themselves
    qq = torch.zeros(1, 1, T, 64, dtype=torch.float64)
    kk = torch.zeros(1, 1, T, 64, dtype=torch.float64)
    qq[0, 0, :, 0] = torch.tensor([0.0, 1.0, 2.0])
    kk[0, 0, :, 0] = torch.tensor([0.0, 1.0, -1.0])
    vv = torch.zeros(1, 1, 64, Tp, dtype=torch.float64)
    for t in range(T):
        vv[0, 0, t, t] = 1.0
    vv[0, 0, 5, T:] = 99.0     # the pad region is not a key
    out = R.attention(qq, kk, vv, T)
    for t in range(T):
        e = np.exp(float(qq[0, 0, t, 0]) * np.array([0.0, 1.0, -1.0]))
        assert np.allclose(out[t, :T].numpy(), e / e.sum(), atol=1e-15) and out[t, 5] == 0


def test_block_statistics_and_the_measure():
    x = torch.arange(2 * 64, dtype=torch.float64).reshape(2, 64)
    s = R.block_stats(x)
    assert s.shape == (2, 2, 2)
    assert s[1, 0, 0] == sum(range(64, 96)) and s[1, 1, 1] == sum(v * v for v in range(96, 128))
    # one garbage block among 7000 rows is the result, whatever the rest looks like
    ref = torch.randn(7000, 1280, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    got = ref.clone()
    fl = R.norm_floor(ref)
    assert R.block_error(got, ref, fl) == 0.0
    got[6999, 1216:] = torch.randn(64, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert R.block_error(got, ref, fl) > 0.5
    assert np.linalg.norm((got - ref).numpy()) / np.linalg.norm(ref.numpy()) < 1e-2    # ... which one relative L2 would not see
    got[0, 0] = float("nan")
    assert R.block_error(got, ref, fl) == float("inf")
    # an (almost) empty reference block is measured against the floor
    ref[5, :64] = 0.0
    got = ref.clone()
    got[5, 0] = fl
    assert abs(R.block_error(got, ref, fl) - 1.0) < 1e-12
    st = torch.ones(4, 2, 2, dtype=torch.float64)
    g2 = st.clone()
    g2[3, 1, 1] = 1.5
    assert abs(R.stats_error(g2, st, R.stats_floor(st)) - 0.5) < 1e-12


# ---- the plan query: the dispatch table of the batched encoder at d = 1280, as computed by hand ---------------------------------
# (T, B): kernel / tile height of [N = 1280 (out-proj, fc2, conv2), N = 2560 (cross K/V), N = 3840 (QKV), N = 5120 (fc1), conv1 (2M rows)]
K1 = (1, 128)
PLAN_TABLE = {
    (500, 4): [K1, K1, K1, (2, 80), K1],
    (500, 7): [K1, (2, 80), (2, 112), (2, 96), (2, 80)],
    (500, 14): [(2, 80), (2, 96), (2, 112), (2, 112), (2, 96)],
    (500, 16): [(2, 80), (2, 112), (2, 128), (2, 128), (2, 112)],
    (1250, 4): [K1, (2, 112), (2, 112), (2, 112), (2, 112)],
    (1250, 7): [(2, 96), (2, 128), (2, 112), (2, 128), (2, 128)],
}


def _plan_by_hand(M, N):
    """The rule of gemm_dispatch restated: kernel 2 from 512 tiles of 128 x 128 on when N % 256 == 0, its tile height by
    ceil(tiles / 256) * (bm + 48), first minimum in the order 128, 112, 96, 80; below that 64-row tiles up to 1000 rows, else 128."""
    if N % 256 == 0 and -(-M // 128) * -(-N // 128) >= 512:
        cost = {bm: -(-(-(-M // bm) * (N // 256)) // 256) * (bm + 48) for bm in (128, 112, 96, 80)}
        return 2, min(cost, key=lambda bm: (cost[bm], -bm))
    return 1, 64 if M <= 1000 else 128


def test_plan_query_agrees_with_the_dispatch_table(built_library):
    from thewhisper_amd import _cabi as cabi

    for dt in (cabi.TW_F32, cabi.TW_BF16, cabi.TW_F16):
        for (T, B), row in PLAN_TABLE.items():
            M = T * B
            got = [cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, 1280, 1280), cabi.gemm_plan(dt, cabi.TW_EPI_KV_CROSS, M, 2560, 1280),
                   cabi.gemm_plan(dt, cabi.TW_EPI_QKV_ENC, M, 3840, 1280), cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, M, 5120, 1280),
                   cabi.gemm_plan(dt, cabi.TW_EPI_ROWMAJOR, 2 * M, 1280, 384)]
            assert got == row, (T, B, got)
    # a sweep against the restated rule, through every threshold of the encoder's shapes
    for M in list(range(1, 2200, 7)) + list(range(2200, 26000, 61)) + [1000, 1001, 2000, 2500, 3000, 3200, 7000, 8000, 8750, 10000, 12000]:
        for N in (64, 128, 384, 1280, 2560, 3840, 5120):
            assert cabi.gemm_plan(cabi.TW_BF16, 0, M, N, 1280) == _plan_by_hand(M, N), (M, N)
    # encoder attention: 128 queries per workgroup from 512 such workgroups on, 16-bit contexts only; heads pinned from 64 heads on
    for B, H, T, want in ((6, 20, 500, (64, 1)), (7, 20, 500, (128, 1)), (14, 20, 500, (128, 1)), (50, 20, 50, (128, 1)),
                          (5, 20, 500, (64, 1)), (3, 20, 500, (64, 0)), (4, 20, 1500, (128, 1)), (1, 20, 1500, (64, 0))):
        assert cabi.enc_attention_plan(cabi.TW_BF16, B, H, T) == want, (B, H, T)
        assert cabi.enc_attention_plan(cabi.TW_F16, B, H, T) == want
        assert cabi.enc_attention_plan(cabi.TW_F32, B, H, T) == (64, want[1])
    with pytest.raises(RuntimeError):
        cabi.gemm_plan(cabi.TW_BF16, 0, 100, 100, 1280)      # N is no multiple of 64: launch_gemm refuses the shape too
