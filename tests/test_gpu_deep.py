"""The decoder's self-attention kernels (k_decode.hip: attn_mfma_block through launch_dec_self_attn) against the numpy oracle at EVERY
position, in every element type and in each of the four instantiations the key bound selects:

    key bound <= 64: 1 wavefront | <= 128: 2 wavefronts | <= 256: 4 wavefronts, all single pass | <= 512: 4 wavefronts, two passes

`decoder_reset` sets the key bound to max_target_positions, so a model of P = 64, 128, 256, 448 positions steps through one instantiation
each (P = 200: a bound that is no multiple of 64); `score_tokens` picks the bucket of each launch's last position, so its rows-mode
launches walk through all of them on the same cache.  The model is tests/pointer_model.py: every query puts probability 1 - 1e-6 on one
key chosen by the test, so a key that is dropped, or paired with its neighbour's value, moves that query's logits by 0.24 relative L2 or
more (tests/test_pointer_model.py) - 8 times the bf16 tolerance - where on random weights it moves them by 2.5e-3.  The last test is the
complement: unchanged random weights, near-uniform attention, all 448 positions.

Per case: (a) `decode_step` over all P positions, relative L2 of every (stream, step) against the oracle within the suite's tolerances
(f32 2e-5, bf16 3e-2, f16 4e-3) and the oracle's top-1 wherever its margin is clear (bf16 0.25, f16 0.03); (b) `score_tokens` of the same
ids: `logprob_raw` equals the float64 log-softmax of (a)'s logits within test_gpu_score's 1e-4 (its argument: float32 log-sum-exp of
logits below 60), so the bucketed rows-mode launches give the stepping kernel's numbers at depth; in f32 also the oracle's log-softmax
within 1e-4, which is 13 times the float32 oracle's own distance from its float64 run (7.8e-6, tests/test_pointer_model.py).
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_deep.py -s`` prints each case's figures.

Measured on the MI355X, largest (stream, step) figure over the pointer cases: f32 6.0e-7, bf16 7.2e-3, f16 9.5e-4; random weights: f32
6.3e-7, bf16 8.6e-3, f16 1.2e-3; rows mode against the stepped logits 1.3e-6 at most, in f32 against the oracle 1.1e-5.  A library whose
two-pass kernel masks key 256 fails the three P = 448 pointer cases at (step 257, the stream that feeds id 256) with 0.49, and the
random-weight case in f32 and f16 only (bf16: 1.4e-2, inside its tolerance) - DESIGN.md 2.6.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import pointer_model as pm
from tests.util import clips, dims_variant, make_engine

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-5, "bf16": 3e-2, "f16": 4e-3}          # tests/test_gpu_parity.py
MARGIN = {"bf16": 0.25, "f16": 0.03}
ROWS_TOL = 1e-4                                         # tests/test_gpu_score.py: TOL
Z_MAX = 60.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    yield
    pm.build.cache_clear()          # up to 0.8 GB of oracle logits: not kept for the rest of the session
    random_model.cache_clear()


def step_and_rows(what, dims, weights, ids, mel, ref, dtype):
    """One engine: every position by `decode_step`, then the same ids by `score_tokens`; judged on the device, fetched once."""
    B, P = ids.shape
    eng = make_engine(dims, weights, T=pm.T, max_batch=B, dtype=dtype)
    try:
        eng.encode(torch.from_numpy(mel).cuda())
        eng.cross_kv(B)
        eng.decoder_reset(B)
        got = torch.empty((P, B, dims.vocab), dtype=torch.float32, device="cuda")
        for p in range(P):
            got[p] = eng.decode_step(ids[:, p].tolist())
        res = eng.score_tokens(ids, 1, begin_suppress=(), suppress=(), timestamps=False)
    finally:
        eng.close()
    ref_d = torch.from_numpy(ref).cuda()                               # [B, P, V]
    ids_d = torch.from_numpy(ids.astype(np.int64)).cuda()
    rel = torch.empty((P, B), dtype=torch.float64, device="cuda")      # per (step, stream)
    rel_step = torch.empty((P,), dtype=torch.float64, device="cuda")   # per step, all streams: test_decoder_teacher_forced's figure
    top_ok = torch.empty((P, B), dtype=torch.bool, device="cuda")
    lp_got = torch.zeros((B, P), dtype=torch.float64, device="cuda")   # float64 log-softmax of the step's logits at the next id
    lp_ref = torch.zeros((B, P), dtype=torch.float64, device="cuda")
    for p in range(P):
        g, r = got[p].double(), ref_d[:, p].double()
        rel[p] = torch.linalg.norm(g - r, dim=-1) / torch.linalg.norm(r, dim=-1)
        rel_step[p] = torch.linalg.norm(g - r) / torch.linalg.norm(r)
        top2 = torch.topk(r, 2, dim=-1)
        clear = (top2.values[:, 0] - top2.values[:, 1]) > MARGIN.get(dtype, float("inf"))
        top_ok[p] = ~clear | (g.argmax(-1) == top2.indices[:, 0])
        if p + 1 < P:
            lp_got[:, p + 1] = torch.log_softmax(g, -1).gather(1, ids_d[:, p + 1, None])[:, 0]
            lp_ref[:, p + 1] = torch.log_softmax(r, -1).gather(1, ids_d[:, p + 1, None])[:, 0]
    finite, z_max = bool(torch.isfinite(got).all()), float(got.abs().max())
    rel, rel_step, top_ok, lp_got, lp_ref = (t.cpu().numpy() for t in (rel, rel_step, top_ok, lp_got, lp_ref))
    raw = res["logprob_raw"].astype(np.float64)
    d_rows, d_oracle = np.abs(raw - lp_got), np.abs(raw - lp_ref)
    at = np.unravel_index(int(np.nanargmax(rel)), rel.shape)
    print(f"{what}: step mode, largest relative L2 {np.nanmax(rel):.2e} at (step {at[0]}, stream {at[1]}), per step over the streams {np.nanmax(rel_step):.2e} "
          f"(bound {TOL[dtype]:g}); top-1 differs at {int((~top_ok).sum())} clear steps; max |logit| {z_max:.1f}; rows mode against the stepped "
          f"logits {d_rows.max():.2e} (bound {ROWS_TOL:g}), against the oracle {d_oracle.max():.2e}")
    assert finite and z_max < Z_MAX
    bad = np.argwhere(~(rel < TOL[dtype]))
    assert not len(bad), (what, "first (step, stream) above the tolerance, the id fed there, the figure:", bad[0].tolist(),
                          int(ids[bad[0][1], bad[0][0]]), float(rel[tuple(bad[0])]))
    assert top_ok.all(), (what, "(step, stream) whose top-1 is not the oracle's:", np.argwhere(~top_ok)[:5].tolist())
    assert raw.shape == (B, P) and (raw[:, 0] == 0.0).all() and np.isfinite(raw).all()
    assert (d_rows <= ROWS_TOL).all(), (what, "rows mode differs from step mode at (stream, position):", np.argwhere(d_rows > ROWS_TOL)[:5].tolist())
    if dtype == "f32":
        assert (d_oracle <= ROWS_TOL).all(), (what, np.argwhere(d_oracle > ROWS_TOL)[:5].tolist())


def pointer_case(P, B, dtype):
    b = pm.build(P, B)
    step_and_rows(f"pointer P={P} B={B} {dtype}", b.dims, b.weights, b.ids, b.mel, b.logits, dtype)


# P outermost: the three types share one oracle run
@pytest.mark.parametrize("P,dtype", [(P, t) for P in (64, 128, 256, 448) for t in ("f32", "bf16", "f16")] + [(200, "bf16")])
def test_pointer_model_every_position_step_and_rows(P, dtype):
    pointer_case(P, len(pm.PATTERNS), dtype)


def test_pointer_model_second_group_of_sixteen_streams():
    """17 streams: the attention output's offset (b >> 4) * 16 * H * 64 of stream 16."""
    pointer_case(128, 17, "bf16")


@functools.lru_cache(maxsize=1)
def random_model():
    dims = dims_variant("micro", enc_layers=1, dec_layers=2)
    w = wo.make_weights(dims, 2)
    ids = np.random.default_rng(3).integers(0, 50000, size=(3, dims.max_target_positions)).astype(np.int32)
    mel = wo.log_mel(clips(pm.T * 320, 3), dims.n_mels)
    return dims, w, ids, mel, pm.oracle_logits(dims, w, ids, mel)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_random_weights_all_448_positions(dtype):
    """test_decoder_teacher_forced's model and tolerances, 448 positions instead of 9: near-uniform attention over up to 448 keys, where
    in f32 one wrong key (2.5e-3) is 100 times the bound."""
    step_and_rows(f"random weights {dtype}", *random_model(), dtype)
