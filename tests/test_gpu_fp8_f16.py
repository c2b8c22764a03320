"""TW_F16_W8A16 ("fp8f16") against a float64 decoder over the parameters the context holds: tensors rounded to float16 as loaded, the fold
W' = f16(g W) with gW = sum W' and cb = W beta + b, the composed f16(W' Wo), the weight a row sees f16(e4m3 x 2^(sb-127)) (k_decode.hip:
sk_widen8<f16_t>) and the e4m3 cross K / V^T.  What is left is float16 activation rounding, which the plain TW_F16 context measures on
the same weights.  Heads = d_model / 64 (the library's head_dim): 2 at d_model 128, 4 at 256."""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests.util import PROMPT, clips, dims_variant, make_engine, rel_l2

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
T = 100
IDS = np.concatenate([np.tile(np.array(PROMPT), (64, 1)), np.random.default_rng(3).integers(0, 50000, size=(64, 2))], axis=1)


def f16(x):   # RNE with gradual underflow, like the widening convert
    return np.asarray(x, dtype=np.float64).astype(np.float16).astype(np.float64)


def kv8_f16(x):   # oracle.kv8_quant_dequant on float16: per (key, head) sb = max(E - 7, 1) of the float16 values, elements RNE to e4m3
    h = f16(np.clip(x, -63488.0, 63488.0))   # (the epilogue clamps to 248 x 2^8: the largest e4m3 image float16 holds)
    E = np.floor(np.log2(np.maximum(np.abs(h).max(axis=-1, keepdims=True), 2.0**-126))).astype(np.int64) + 127
    return wo.e4m3_rne(h / np.ldexp(1.0, np.maximum(E - 7, 1) - 127)) * np.ldexp(1.0, np.maximum(E - 7, 1) - 127)


class Ref(wo.OracleWhisper):
    def __init__(self, dims, w, fp8, T=T):
        super().__init__(dims, {k: f16(v) for k, v in w.items()}, T=T, dtype=np.float64)
        # (the context interpolates the float32 table as loaded and rounds the result: tw_finalize_weights, launch_interp_positions)
        self.enc_pos = f16(wo.interpolate_positions(np.asarray(w["model.encoder.embed_positions.weight"], dtype=np.float32), self.T))
        self.fp8, self.memo = fp8, {}

    def _q(self, key, make):   # the weight a row sees
        if key not in self.memo:
            self.memo[key] = f16(wo.mx8_quant_dequant(make())) if self.fp8 else make()
        return self.memo[key]

    def _dec_proj(self, x, ln, lin, bias=True):
        W, g, beta = self.w[lin + ".weight"], self.w[ln + ".weight"], self.w[ln + ".bias"]
        Wf = f16(W * g)
        u = x @ self._q(lin, lambda: Wf).T
        if lin.endswith("encoder_attn.q_proj"):   # cross query ahead: x0 W'^T + W' bo + attn (W' Wo)^T, the LayerNorm of x1 afterwards
            a, y, o = self.ahead
            u = u - y @ self.memo[lin].T + Wf @ self.w[o + ".bias"] + a @ self._q(o + "+q", lambda: f16(Wf @ self.w[o + ".weight"])).T
        mean, rstd = x.mean(-1, keepdims=True), 1.0 / np.sqrt(x.var(-1, keepdims=True) + 1e-5)
        return rstd * (u - mean * Wf.sum(1)) + W @ beta + (self.w[lin + ".bias"] if bias else 0.0)

    def _dec_lin(self, x, lin):
        y = x @ self._q(lin, lambda: self.w[lin + ".weight"]).T + self.w[lin + ".bias"]
        self.ahead = (x, y, lin)   # (read by the cross query, which follows the self-attention's out-projection)
        return y

    def _dec_logits(self, x):
        return self._dec_proj(x, "model.decoder.layer_norm", "model.decoder.embed_tokens", bias=False)

    def new_cache(self, enc):
        c = super().new_cache(enc)
        if self.fp8:   # K is widened with its scale (to float16), V^T unscaled
            c.cross_k, c.cross_v = [f16(kv8_f16(k)) for k in c.cross_k], [kv8_f16(v) for v in c.cross_v]
        return c


@functools.lru_cache(maxsize=None)
def model(d_model, layers, ffn):
    dims = dims_variant("micro", d_model=d_model, heads=d_model // 64, ffn=ffn, enc_layers=1, dec_layers=layers)
    w = wo.make_weights(dims, 2)
    return dims, w, Ref(dims, w, False), Ref(dims, w, True)


def run(dims, w, dtype, rows, ref=None):
    """rel-L2 of a context's teacher-forced logits [rows, 5, V] to `ref` on the context's own encoder states (no ref: the logits);
    rows: which of the 64 clips (and id rows) make up the launch"""
    eng = make_engine(dims, w, T=T, max_batch=64, dtype=dtype)
    try:
        B, mel = len(rows), wo.log_mel(clips(T * 320, 64)[rows], dims.n_mels)
        enc = eng.encode(torch.from_numpy(mel).cuda(), return_hidden=True).double().cpu().numpy()
        eng.cross_kv(B)
        eng.decoder_reset(B)
        got = np.stack([eng.decode_step(IDS[rows, s].tolist()).cpu().numpy() for s in range(5)], axis=1)
        if ref is None:
            return got
        cache = ref.new_cache(enc)
        return rel_l2(got, np.stack([ref.decode(IDS[rows, s : s + 1], cache)[0][:, 0] for s in range(5)], axis=1))
    finally:
        eng.close()


@pytest.mark.parametrize("B", [1, 16, 17, 64])
@pytest.mark.parametrize("d_model,layers,ffn", [(128, 2, 512), (256, 1, 512), (128, 1, 4096)])
def test_projection_rule(d_model, layers, ffn, B):
    """8 wavefronts over 1, 2 or 4 steps of 128 k (a partial last slice), one group of streams and several; ffn = 4096 is the long-K
    fc2: 16 wavefronts up to 16 rows, SPLIT2 above.  Bound: twice the TW_F16 context's own distance to float64 over the same weights
    (measured at ffn 512: 5.1-5.9e-4 against 5.3-6.1e-4)."""
    dims, w, ref16, ref8 = model(d_model, layers, ffn)
    plain, new = run(dims, w, "f16", np.arange(B), ref16), run(dims, w, "fp8f16", np.arange(B), ref8)
    print(f"d_model={d_model} layers={layers} ffn={ffn} B={B}: logits rel-L2 to float64  TW_F16 {plain:.3e}  TW_F16_W8A16 {new:.3e}")
    assert new <= 2 * plain


@pytest.mark.parametrize("layers,ffn", [(2, 512), (1, 4096)])
def test_a_row_does_not_depend_on_its_launch(layers, ffn):
    """first group / last group of a 64-row launch against the clip alone; ffn 4096: fc2's SPLIT2 against its 16-wavefront kernel"""
    dims, w, _, _ = model(128, layers, ffn)
    many = run(dims, w, "fp8f16", np.arange(64))
    for r in (0, 63):
        assert np.array_equal(many[r], run(dims, w, "fp8f16", np.array([r]))[0]), r


def test_the_bf16_flavour_is_farther_and_drafts_return_the_plain_ids():
    dims, w, _, ref8 = model(128, 2, 512)
    new, bf = run(dims, w, "fp8f16", np.arange(16), ref8), run(dims, w, "fp8a16", np.arange(16), ref8)   # the SAME float64 model
    print(f"logits rel-L2 to float64: TW_F16_W8A16 {new:.3e}  TW_BF16_W8A16 {bf:.3e}")
    assert new < bf
    eng = make_engine(dims, w, T=T, max_batch=3, dtype="fp8f16")   # rows launches: a verified draft returns the plain call's ids
    try:
        eng.encode(torch.from_numpy(wo.log_mel(clips(T * 320, 3), dims.n_mels)).cuda())
        eng.cross_kv(3)
        kw = dict(max_new_tokens=24, min_new_tokens=24)
        plain = eng.generate_greedy(np.tile(np.array(PROMPT, dtype=np.int32), (3, 1)), **kw)["sequences"]
        out = eng.generate_greedy(plain[:, :15].astype(np.int32), n_draft=12, **kw)
        assert np.array_equal(out["sequences"], plain) and out["draft"]["accepted"] == 36, out["draft"]
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,want", [(torch.float16, 5), (torch.bfloat16, 4)])
def test_dropin_selects_the_context_by_torch_dtype(dtype, want):
    from oracle import hf_reference as hr
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    pipe = ASRPipeline(hr.build_hf_model(dims, wo.make_weights(dims, 0)), feature_extractor=hr.build_feature_extractor(dims, 10),
                       tokenizer=hr.build_tokenizer(dims), chunk_length_s=10, device="cuda", torch_dtype=dtype, decoder_weights="fp8")
    try:
        assert pipe.model.engine.tw_dtype == want
    finally:
        pipe.model.engine.close()
