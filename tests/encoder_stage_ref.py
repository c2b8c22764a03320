"""Float64 references of the batched encoder, ONE FUNCTION PER LAUNCH, in the layouts ``WhisperEngine.encode_tapped`` returns.

Every function maps the inputs of one launch (``tw_encode`` in thewhisper_amd/csrc/api.hip: encode_core) to its output, so a test can
feed it the device's own taps and look at that launch alone.  Plain torch float64 on the CPU; nothing here touches the GPU or the
product package.  ``tests/test_encoder_stage_ref.py`` pins the functions: composed, they are ``oracle.whisper_oracle.OracleWhisper``
in float64, and a hand-built case fixes the head-split and transposed layouts.

``emul`` selects the EMULATED variant of a stage: the same computation with the context dtype's rounding applied where the kernels
round - the LayerNorm-folded weight ``W g`` rounded to T, the attention probabilities rounded to T in front of P.V (16-bit
contexts), the stored output rounded to T; in ``"f32"`` the whole stage is evaluated in float32, the matrix products with the
MFMA's one accumulator per output rounded after every 4-wide k-step (``_matmul_t``).  The LayerNorm-folded stages are emulated in the
kernels' algebra, rstd (x W'^T - mean gw) + cb (``_ln_linear``).  The emulated variant only sets tolerances (how far honest arithmetic in that format lands from the exact value); it is never the expected value.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from oracle import whisper_oracle as wo

TORCH_DTYPE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32, "f64": torch.float64}
F64 = torch.float64


def round_to(x: torch.Tensor, dtype: Optional[str]) -> torch.Tensor:
    """``x`` rounded to the storage format ``dtype`` (float16 saturates, as the kernels' stores do) and widened back; None / "f64": x."""
    if dtype in (None, "f64"):
        return x
    if dtype == "f16":
        x = x.clamp(-65504.0, 65504.0)
    return x.to(TORCH_DTYPE[dtype]).to(x.dtype)


def _t(a) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(F64)


class StageWeights:
    """The encoder's weights of one layer as the engine holds them after ``tw_load_weight``: every tensor rounded to the context
    dtype (``dtype="f64"``: not rounded - the float64 oracle's weights), the 1/8 query scale folded into q_proj (exact: a power of
    two), q | k | v stacked into one [3d, d] matrix whose k rows have no bias, the conv kernels as [d, 3 * C] matrices over windows
    of three consecutive token rows, and the positional table interpolated to T frames."""

    def __init__(self, weights: Dict[str, np.ndarray], dims: wo.WhisperDims, T: int, dtype: str, layer: int = 0):
        r = lambda a: round_to(_t(a), dtype)   # noqa: E731
        e, p = "model.encoder", f"model.encoder.layers.{layer}"
        self.dims, self.T, self.dtype = dims, T, dtype
        self.d, self.H, self.F = dims.d_model, dims.heads, dims.ffn
        assert self.d == self.H * 64, "the engine's attention kernels are built for head_dim 64"
        self.Tp = (T + 63) // 64 * 64
        # conv weight [co, ci, 3] -> [co, 3 * ci]: column k * ci + c multiplies channel c of window row k
        self.conv1_w = r(weights[e + ".conv1.weight"]).permute(0, 2, 1).reshape(self.d, -1).contiguous()
        self.conv1_b = r(weights[e + ".conv1.bias"])
        self.conv2_w = r(weights[e + ".conv2.weight"]).permute(0, 2, 1).reshape(self.d, -1).contiguous()
        self.conv2_b = r(weights[e + ".conv2.bias"])
        self.pos = r(wo.interpolate_positions(np.asarray(weights[e + ".embed_positions.weight"], dtype=np.float32), T))
        a = p + ".self_attn"
        self.wqkv = torch.cat([r(weights[a + ".q_proj.weight"] * np.float32(0.125)), r(weights[a + ".k_proj.weight"]),
                               r(weights[a + ".v_proj.weight"])])
        self.bqkv = torch.cat([r(weights[a + ".q_proj.bias"] * np.float32(0.125)), torch.zeros(self.d, dtype=F64),
                               r(weights[a + ".v_proj.bias"])])
        self.wo, self.bo = r(weights[a + ".out_proj.weight"]), r(weights[a + ".out_proj.bias"])
        self.ln1_g, self.ln1_b = r(weights[p + ".self_attn_layer_norm.weight"]), r(weights[p + ".self_attn_layer_norm.bias"])
        self.ln2_g, self.ln2_b = r(weights[p + ".final_layer_norm.weight"]), r(weights[p + ".final_layer_norm.bias"])
        self.w1, self.b1 = r(weights[p + ".fc1.weight"]), r(weights[p + ".fc1.bias"])
        self.w2, self.b2 = r(weights[p + ".fc2.weight"]), r(weights[p + ".fc2.bias"])
        self.lnf_g, self.lnf_b = r(weights[e + ".layer_norm.weight"]), r(weights[e + ".layer_norm.bias"])


# ---- arithmetic shared by the stages -----------------------------------------------------------------------------------------
def _work(emul: Optional[str]):
    """Working precision of a stage: float32 for the emulation of strict-f32 contexts, float64 otherwise."""
    return torch.float32 if emul == "f32" else F64


def gelu(x: torch.Tensor) -> torch.Tensor:
    return 0.5 * x * (1.0 + torch.special.erf(x * (1.0 / math.sqrt(2.0))))


def _matmul_t(x, w, emul):
    """x w^T in the stage's working precision.  Emulated float32: accumulated as the MFMA GEMM does, ONE float32 accumulator per
    output that takes the products of four consecutive k at a time (v_mfma_f32_16x16x4_f32) and is rounded after every such step -
    K / 4 roundings in sequence, whose error grows like sqrt(K / 4) ulp, where a blocked CPU sgemm keeps many partial sums."""
    wd = _work(emul)
    x, w = x.to(wd), w.to(wd)
    if emul != "f32":
        return x @ w.T
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=wd)
    wt = w.T.contiguous()
    for k0 in range(0, x.shape[1], 4):
        acc.addmm_(x[:, k0:k0 + 4], wt[k0:k0 + 4])
    return acc


def _linear(x, w, b, emul):
    y = _matmul_t(x, w, emul)
    return y if b is None else y + b.to(y.dtype)


def _layer_norm(x, g, b, wd):
    x = x.to(wd)
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g.to(wd) + b.to(wd)


def _ln_linear(x, g, beta, w, b, emul):
    """LayerNorm(x) W^T + b.  Exact: the plain sequence.  Emulated: as the folded kernels compute it (k_decode.hip fold_ln_kernel,
    k_gemm.hip gemm_ln_publish and the epilogues): rstd (x W'^T - mean gw) + cb on the RAW x, with W' = W g ROUNDED to T, gw the row
    sums of W', cb = W beta + b, mean = sum / K and rstd = 1 / sqrt(sumsq / K - mean^2 + eps) in the working precision."""
    wd = _work(emul)
    if emul is None:
        return _linear(_layer_norm(x, g, beta, wd), w, b, None)
    x = x.to(wd)
    K = x.shape[-1]
    mu = x.sum(-1, keepdim=True) / K
    rstd = 1.0 / torch.sqrt(((x * x).sum(-1, keepdim=True) / K - mu * mu).clamp_min(0.0) + 1e-5)
    wf = round_to((w * g[None, :]).to(wd), emul)
    cb = (w @ beta + (b if b is not None else 0.0)).to(wd)
    return rstd * (_matmul_t(x, wf, emul) - mu * wf.sum(-1)[None, :]) + cb


def _store(y, emul):
    return round_to(y, emul).to(F64)


# ---- one function per launch -------------------------------------------------------------------------------------------------
def conv1_gelu(mel: torch.Tensor, W: StageWeights, emul: Optional[str] = None, rows=None) -> torch.Tensor:
    """mel [B, n_mels, 2T] (as the engine holds it: rounded to the context dtype) -> h1 [B, 2T+2, d]: GELU(conv1d k=3 p=1) token-major,
    rows 0 and 2T+1 of every clip zero (the padding conv2 reads).  ``rows``: only these logical rows b * 2T + t, returned as [n, d]."""
    B, C, n = mel.shape
    xp = torch.nn.functional.pad(mel.to(F64).permute(0, 2, 1), (0, 0, 1, 1))               # [B, 2T+2, C]
    win = torch.cat([xp[:, 0:n], xp[:, 1:n + 1], xp[:, 2:n + 2]], dim=-1).reshape(B * n, 3 * C)
    if rows is not None:
        return _store(gelu(_linear(win[rows], W.conv1_w, W.conv1_b, emul)), emul)
    y = _store(gelu(_linear(win, W.conv1_w, W.conv1_b, emul)), emul).reshape(B, n, -1)
    return torch.nn.functional.pad(y, (0, 0, 1, 1))


def conv2_gelu_pos(h1: torch.Tensor, W: StageWeights, emul: Optional[str] = None, rows=None) -> torch.Tensor:
    """h1 [B, 2T+2, d] (padded) -> xa [B*T, d]: GELU(conv1d k=3 s=2 p=1) + positions; frame t reads padded rows 2t, 2t+1, 2t+2."""
    B, n2, d = h1.shape
    T = (n2 - 2) // 2
    h1 = h1.to(F64)
    win = torch.cat([h1[:, 0:2 * T:2], h1[:, 1:2 * T + 1:2], h1[:, 2:2 * T + 2:2]], dim=-1).reshape(B * T, 3 * d)
    pos = W.pos.repeat(B, 1)
    if rows is not None:
        win, pos = win[rows], pos[rows]
    return _store(gelu(_linear(win, W.conv2_w, W.conv2_b, emul)) + pos.to(_work(emul)), emul)


def block_stats(x: torch.Tensor, emul: Optional[str] = None) -> torch.Tensor:
    """x [rows, d] AS STORED -> [rows, d/32, 2]: (sum, sum of squares) of every 32-column block (the folded LayerNorm's partial row
    statistics).  Emulated (any context: the kernels keep these in float32): summed in float32."""
    wd = F64 if emul is None else torch.float32
    v = x.to(wd).reshape(x.shape[0], -1, 32)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1).to(F64)


def ln_qkv_rows(xa: torch.Tensor, W: StageWeights, emul: Optional[str] = None) -> torch.Tensor:
    """xa [M, d] -> [M, 3d] = q | k | v of LayerNorm(xa), q scaled by 1/8, k without bias, rounded as stored."""
    return _store(_ln_linear(xa.to(F64), W.ln1_g, W.ln1_b, W.wqkv, W.bqkv, emul), emul)


def split_qkv(y: torch.Tensor, B: int, T: int, H: int, Tp: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """[B*T, 3 * H * 64] -> q, k [B, H, T, 64] and vt [B, H, 64, Tp] (V transposed, keys [T, Tp) zero)."""
    v = y.reshape(B, T, 3, H, 64)
    q, k = v[:, :, 0].permute(0, 2, 1, 3).contiguous(), v[:, :, 1].permute(0, 2, 1, 3).contiguous()
    vt = torch.nn.functional.pad(v[:, :, 2].permute(0, 2, 3, 1), (0, Tp - T)).contiguous()
    return q, k, vt


def ln_qkv(xa: torch.Tensor, W: StageWeights, B: int, emul: Optional[str] = None):
    """The fused LayerNorm + QKV launch: xa [B*T, d] -> (q, k, vt) in the attention kernel's layouts."""
    return split_qkv(ln_qkv_rows(xa, W, emul), B, W.T, W.H, W.Tp)


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, T: int, emul: Optional[str] = None) -> torch.Tensor:
    """q, k [B, H, T, 64], vt [B, H, 64, Tp] -> [B*T, H*64]: softmax(q k^T) v per stream and head (q carries its scale).  Emulated, 16-bit:
    the unnormalised probabilities exp(s - max) are rounded to T for P.V and normalised by the sum of the unrounded ones."""
    wd = _work(emul)
    B, H = q.shape[:2]
    q, k, v = q.to(wd), k.to(wd), vt[..., :T].to(wd).transpose(-1, -2)
    s = q @ k.transpose(-1, -2)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    pr = round_to(p, emul) if emul in ("bf16", "f16") else p
    o = (pr @ v) / p.sum(-1, keepdim=True)
    return _store(o.permute(0, 2, 1, 3).reshape(B * T, H * 64), emul)


def out_proj_residual(attn: torch.Tensor, xa: torch.Tensor, W: StageWeights, emul: Optional[str] = None) -> torch.Tensor:
    """attn, xa [M, d] -> xb = xa + attn Wo^T + bo."""
    return _store(_linear(attn.to(F64), W.wo, W.bo, emul) + xa.to(_work(emul)), emul)


def ln_fc1_gelu(xb: torch.Tensor, W: StageWeights, emul: Optional[str] = None) -> torch.Tensor:
    """xb [M, d] -> GELU(LayerNorm(xb) W1^T + b1) [M, F]."""
    return _store(gelu(_ln_linear(xb.to(F64), W.ln2_g, W.ln2_b, W.w1, W.b1, emul)), emul)


def fc2_residual(ffnh: torch.Tensor, xb: torch.Tensor, W: StageWeights, emul: Optional[str] = None) -> torch.Tensor:
    """ffnh [M, F], xb [M, d] -> xb + ffnh W2^T + b2: the layer's output."""
    return _store(_linear(ffnh.to(F64), W.w2, W.b2, emul) + xb.to(_work(emul)), emul)


def final_layer_norm(xa: torch.Tensor, W: StageWeights, emul: Optional[str] = None) -> torch.Tensor:
    return _store(_layer_norm(xa.to(F64), W.lnf_g, W.lnf_b, _work(emul)), emul)


# ---- the undiluted error measure -----------------------------------------------------------------------------------------------
def block_norms(x: torch.Tensor, block: int = 64) -> torch.Tensor:
    """L2 norm of every ``block`` consecutive elements of the last axis (64 columns: one wavefront's slab of a GEMM tile, one head)."""
    return x.to(F64).reshape(*x.shape[:-1], -1, block).norm(dim=-1)


def norm_floor(ref: torch.Tensor, block: int = 64) -> float:
    """0.1 x the median block norm of a stage's reference: what a block's own norm is replaced by when it is (almost) empty."""
    return 0.1 * float(block_norms(ref, block).median())


def block_error(got: torch.Tensor, ref: torch.Tensor, floor: float, block: int = 64) -> float:
    """max over every (row, block) of |got - ref|_2 / max(|ref|_2, floor).  One wrong block anywhere is the result; NaN counts as inf."""
    err = block_norms(got.to(F64) - ref.to(F64), block) / block_norms(ref, block).clamp_min(floor)
    return float(torch.nan_to_num(err, nan=float("inf")).max()) if err.numel() else 0.0


def stats_error(got: torch.Tensor, ref: torch.Tensor, floor: Tuple[float, float]) -> float:
    """The measure for [rows, d/32, 2] statistics: per (row, block) and per number, |got - ref| / max(|ref|, floor of that number)."""
    fl = torch.tensor(floor, dtype=F64)
    err = (got.to(F64) - ref).abs() / torch.maximum(ref.abs(), fl)
    return float(torch.nan_to_num(err, nan=float("inf")).max())


def stats_floor(ref: torch.Tensor) -> Tuple[float, float]:
    return 0.1 * float(ref[..., 0].abs().median()), 0.1 * float(ref[..., 1].abs().median())
