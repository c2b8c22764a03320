"""TW_F16_W8A16_FULL ("fp8f16full"): fp8 encoder linears and cross-K/V projection weights (k_gemm_w8.hip, gemm_w8reg_kernel) on the float16
base.  The rule: the encoder IS the float16 encoder over the de-quantised weights w = f16(e4m3 x 2^(sb-127)), bit for bit, and the decoder
side is "fp8f16"'s.  T = 100, heads = d_model / 64: M = 100 B rows; K = 128 is two K tiles, N = 128 one half-filled 256-column block."""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests.test_gpu_fp8_f16 import IDS, Ref, T, f16
from tests.util import PROMPT, clips, dims_variant, make_engine, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
SHAPES = [(128, 512), (256, 512), (128, 1536)]   # (d_model, ffn); ffn 1536: fc2 has 24 K tiles


@functools.lru_cache(maxsize=None)
def pool():
    return clips(T * 320, 64)


def quantised(dims):
    """names of the matrices the context stores as e4m3, and of the LayerNorms folded into them"""
    enc = [f"model.encoder.layers.{i}" for i in range(dims.enc_layers)]
    mats = [f"{p}.{m}.weight" for p in enc for m in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.out_proj", "fc1", "fc2")]
    mats += [f"model.decoder.layers.{i}.encoder_attn.{m}.weight" for i in range(dims.dec_layers) for m in ("k_proj", "v_proj")]
    return mats, [f"{p}.{n}.weight" for p in enc for n in ("self_attn_layer_norm", "final_layer_norm")]


def put_on_grid(dims, w, seed=5, elem_exp=(-4, 5)):
    """`w` with every matrix the context quantises ON the fp8 grid (in place; returns w): per block e4m3 normals (8 + r) 2^j x 2^s,
    j in [elem_exp), with one magnitude in [128, 240], so sb reproduces s and quantisation is the identity; three distinct block scales
    s per matrix; the folded LayerNorms' gains 1.0: the fold changes nothing"""
    rng = np.random.default_rng(seed)
    mats, gains = quantised(dims)
    for name in gains:
        w[name] = np.ones_like(w[name])
    for name in mats:
        N, K = w[name].shape
        shp = (N, K // 128, 2, 2, 2, 2, 8)                                   # [n, step, h, mm, u, kk, e]: block (step, h, u) = (mm, kk, e)
        v = (8 + rng.integers(0, 8, shp)) * np.ldexp(1.0, rng.integers(elem_exp[0], elem_exp[1], shp)) * rng.choice([-1.0, 0.0, 1.0], shp)
        v[:, :, :, 0, :, 0, 0] = (8 + rng.integers(0, 8, shp[:3] + shp[4:5])) * 16.0
        s = rng.integers(-12, -9, (N, K // 128, 2, 1, 2, 1, 1))
        w[name] = (v * np.ldexp(1.0, s)).reshape(N, K).astype(np.float32)
        assert np.array_equal(wo.mx8_quant_dequant(w[name]), w[name]) and np.array_equal(f16(w[name]), w[name])
    return w


@functools.lru_cache(maxsize=None)
def model(d_model, ffn, grid):
    dims = dims_variant("micro", d_model=d_model, heads=d_model // 64, ffn=ffn, enc_layers=2, dec_layers=1)
    w = wo.make_weights(dims, 2)
    return dims, put_on_grid(dims, w) if grid else w


class RefFull(Ref):
    """Ref(fp8=True) whose encoder linears and cross k_proj / v_proj are f16(mx8_quant_dequant(f16(g W))), gw / cb from the unquantised W'.
    The encoder's q_proj carries its 1/8 as the context holds it, f16(W / 8) rounded at load and folded after that: scaling the
    projection's result instead keeps the bits that float16 drops where W / 8 is subnormal (2e-7 of the encoder states at d_model 128,
    found when tests/test_encoder_stage_ref.py composed the per-launch references against this class)."""

    def __init__(self, dims, w, T=T):
        super().__init__(dims, w, True, T=T)
        for i in range(dims.enc_layers):
            for t in ("weight", "bias"):
                key = f"model.encoder.layers.{i}.self_attn.q_proj.{t}"
                self.w[key] = f16(np.asarray(w[key], dtype=np.float32) * np.float32(0.125))
        for i in range(dims.dec_layers):
            for m in ("k_proj", "v_proj"):
                key = f"model.decoder.layers.{i}.encoder_attn.{m}.weight"
                self.w[key] = f16(wo.mx8_quant_dequant(self.w[key]))

    def encoder_layer(self, x, i):
        p = f"model.encoder.layers.{i}"
        ln1, ln2 = p + ".self_attn_layer_norm", p + ".final_layer_norm"
        q = self._heads(self._dec_proj(x, ln1, p + ".self_attn.q_proj"))
        k = self._heads(self._dec_proj(x, ln1, p + ".self_attn.k_proj", bias=False))
        v = self._heads(self._dec_proj(x, ln1, p + ".self_attn.v_proj"))
        x = x + self._dec_lin(self._merge(wo.softmax(q @ k.transpose(0, 1, 3, 2)) @ v), p + ".self_attn.out_proj")
        return x + self._dec_lin(wo.gelu(self._dec_proj(x, ln2, p + ".fc1")), p + ".fc2")


def run(dims, w, dtype, rows, beams=False, max_batch=16):
    """the mel, encoder states [B, T, d], the logits of one decode step [min(B, 16), V] and - `beams` - generate_beam's (ids, scores)"""
    eng = make_engine(dims, w, T=T, max_batch=max_batch, dtype=dtype)
    try:
        mel = wo.log_mel(pool()[rows], dims.n_mels)
        enc = eng.encode(torch.from_numpy(mel).cuda(), return_hidden=True).cpu().numpy()
        eng.cross_kv(len(rows))
        n = min(len(rows), 16)   # (launch_gemv refuses ffn = 1536 above 16 rows: a limit of the decoder's fc2, in every context)
        eng.decoder_reset(n)
        logits = eng.decode_step(IDS[rows[:n], 0].tolist()).cpu().numpy()
        res = eng.generate_beam(np.tile(np.array(PROMPT, dtype=np.int32), (len(rows) // 2, 1)), 2, max_new_tokens=8) if beams else None
        return mel, enc, logits, res and (res["nbest_sequences"], res["nbest_scores"])
    finally:
        eng.close()


@pytest.mark.parametrize("d_model,ffn,B", [s + (B,) for s in SHAPES for B in (1, 3, 16)] + [(128, 1536, 64)])
def test_bits_on_grid_weights(d_model, ffn, B):
    """layout, scale indexing, widening, K order and every epilogue at once: on weights that lie on the fp8 grid the context is "fp8f16"
    over the same tensors, bit for bit.  B = 64 at ffn 1536 is the one launch here that takes 80 x 256 tiles (fc1: M = 6400, N = 1536)."""
    from thewhisper_amd import _cabi
    assert _cabi.gemm_plan(_cabi.TW_F16_W8A16_FULL, 0, 100 * B, ffn, d_model) == (3, 80 if B == 64 else 64)
    dims, w = model(d_model, ffn, True)
    rows = np.arange(B)
    new, old = (run(dims, w, dt, rows, beams=B in (3, 16), max_batch=B)[1:] for dt in ("fp8f16full", "fp8f16"))
    assert np.array_equal(new[0], old[0]), "encoder states"
    assert np.array_equal(new[1], old[1]), "decode-step logits"
    if new[2]:
        assert np.array_equal(new[2][0], old[2][0]) and np.array_equal(new[2][1], old[2][1]), "beam ids / scores"


@pytest.mark.parametrize("B", [1, 3, 16])
@pytest.mark.parametrize("d_model,ffn", SHAPES)
def test_quantiser_off_grid(d_model, ffn, B):
    """make_weights tensors against float64 (RefFull); bound: twice the plain "f16" context's own distance to ITS float64 reference
    (test_gpu_fp8_f16.test_projection_rule's rule), encoder states and decode-step logits, measured in the same run.
    Measured (encoder states; logits), the nine cases: fp8f16full 4.9-5.4e-4; 3.6-4.4e-4 against f16 5.4-6.0e-4; 4.2-4.9e-4."""
    dims, w = model(d_model, ffn, False)
    rows, dist = np.arange(B), {}
    for dtype, ref in (("f16", Ref(dims, w, False)), ("fp8f16full", RefFull(dims, w))):
        mel, enc, logits, _ = run(dims, w, dtype, rows, max_batch=B)
        want = ref.decode(IDS[rows, :1], ref.new_cache(enc.astype(np.float64)))[0][:, 0]
        dist[dtype] = rel_l2(enc, ref.encode(mel.astype(np.float64))), rel_l2(logits, want)
    print(f"d_model={d_model} ffn={ffn} B={B}: rel-L2 to float64 (encoder states, logits)  f16 {dist['f16'][0]:.3e} {dist['f16'][1]:.3e}"
          f"  fp8f16full {dist['fp8f16full'][0]:.3e} {dist['fp8f16full'][1]:.3e}")
    assert dist["fp8f16full"][0] <= 2 * dist["f16"][0] and dist["fp8f16full"][1] <= 2 * dist["f16"][1]


@pytest.mark.parametrize("d_model,ffn", SHAPES)
def test_a_clip_does_not_depend_on_its_batch(d_model, ffn):
    dims, w = model(d_model, ffn, False)
    many = run(dims, w, "fp8f16full", np.arange(16))[1]
    for r in (0, 7, 15):
        assert np.array_equal(many[r], run(dims, w, "fp8f16full", np.array([r]))[1][0]), r
