"""The ROWS flavour of the fp8 contexts' cross attention (k_decode_kv8_rows.hip: dec_cross_attn_kv8_rows_kernel<T, G, FQ>) against the one-position
kernel, on tests/cross_pointer_model.py, by the stepped-reference pattern of tests/test_gpu_cross_rows.py ((a) - (e) as there):

    T        64 (one key group), 100 (masked tail inside a group), 500 (G = 1), 1000 (G = 2), 1500 (G = 3)
    types    fp8a16, fp8f16; fp8a8 (16 rows per launch) at T = 100 and 1500
    shapes   rs in 1, 2, 3, 16 streams x n in {2, 5, 16, 17, cap // rs} positions, n <= cap // rs >= 2 (cap = 64; 16 for fp8a8)

(a) forced prefix: rows launches reported, every alignment row on its target and array_equal to the stepped row.  A generate call ends
with one-position steps, so `last_cross_grid` reads (heads, rs, 1) behind it; the grid of the rows launch, (heads, rs, ceil(n / 16)), is
read behind (c) `score_tokens`, a call that ends with its rows launch - what fails without the kernel (its launches were (heads, rs * n,
1)).  (b) a confirmed draft == the plain call.  (c) `logprob_raw` within test_gpu_score's 1e-4 of the stepped logits' float64 log-softmax,
alignment rows untouched.  (f) per G: the rows' `logprob_raw` against OracleWhisperMXFP8 on the engine's encoder states, relative L2 per
position over the streams within tests/test_gpu_cross.py's FP8_TOL.  (e) near-uniform attention.  (d) TW_FUSE_CQ=0 in a child process.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import cross_pointer_model as xm
from tests.util import clips, make_engine

pytestmark = pytest.mark.gpu
P, N_REF, STREAMS = 96, 65, (1, 2, 3, 16)
ROWS_TOL = 1e-4                                         # tests/test_gpu_score.py: TOL
FP8_TOL = {"fp8a16": 4e-2, "fp8a8": 6e-2}               # tests/test_gpu_cross.py: FP8_TOL
ORACLE = {(500, "fp8a16"), (1000, "fp8a16"), (1500, "fp8a8")}   # G = 1, 2, 3
OFF = dict(begin_suppress=(), suppress=(), timestamps=False)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def shapes(cap):
    return [(rs, n) for rs in STREAMS if cap // rs >= 2 for n in sorted({2, 5, 16, 17, cap // rs}) if n <= cap // rs]


def rows_case(T, dtype, what, oracle=False):
    dims, w, g = xm.pointer_weights(T, P)
    ids = xm.pointer_ids(T, P)[:16]
    tg = xm.targets(ids, g)                                             # [16, 2, P]
    mel = torch.from_numpy(wo.log_mel(clips(T * 320, 16), dims.n_mels)).cuda()
    cap = 16 if dtype == "fp8a8" else 64
    eng = make_engine(dims, w, T=T, max_batch=16, dtype=dtype, heads=xm.HEADS)
    try:
        # ---- the reference: one position per launch ----
        enc = eng.encode(mel, return_hidden=oracle); eng.cross_kv(16); eng.decoder_reset(16)
        nxt = torch.from_numpy(ids[:, 1:N_REF].astype(np.int64)).cuda()
        lp = np.zeros((16, N_REF)); lpq = None
        for p in range(N_REF):
            z = eng.decode_step(ids[:, p].tolist()).double()
            if p + 1 < N_REF:
                lp[:, p + 1] = torch.log_softmax(z, -1).gather(1, nxt[:, p, None])[:, 0].cpu().numpy()
        assert eng.last_cross_grid() == (2, 16, 1), what
        if oracle:
            oq = wo.OracleWhisperMXFP8(dims, w, T=T, cross_q_ahead=True, act_quant=dtype == "fp8a8")
            zq = torch.from_numpy(oq.decode(ids[:, :N_REF - 1], oq.new_cache(enc.cpu().numpy()))[0]).cuda().double()
            lpq = np.zeros((16, N_REF))
            lpq[:, 1:] = torch.log_softmax(zq, -1).gather(2, nxt[..., None])[..., 0].cpu().numpy()
        al = eng.get_alignment(16, N_REF)
        assert np.isfinite(al).all() and np.array_equal(al.argmax(-1), tg[:, :, :N_REF]), (what, "the stepped rows miss their targets")
        worst = 0.0
        for rs, n in shapes(cap):
            w_ = f"{what} rs={rs} n={n}"
            eng.encode(mel[:rs]); eng.cross_kv(rs)
            # ---- (a) forced prefix: positions 0 .. n - 1 as rows, tokens chosen by the test ----
            eng.generate_greedy(ids[:rs, :n + 1], n_forced=n, max_new_tokens=n + 2, want_alignment=True, **OFF)
            assert eng.last_prompt_rows() == {"launches": 1, "positions": n}, (w_, eng.last_prompt_rows())
            assert eng.last_cross_grid() == (2, rs, 1), (w_, "the steps behind the prefix", eng.last_cross_grid())
            al2 = eng.get_alignment(rs, n)
            miss = np.argwhere(al2.argmax(-1) != tg[:rs, :, :n])
            assert not len(miss), (w_, "first (stream, head, position) whose row peaks elsewhere", miss[0].tolist())
            diff = np.argwhere((al2 != al[:rs, :, :n]).any(-1))
            assert not len(diff), (w_, "first (stream, head, position) whose row is not the stepped one", diff[0].tolist())
            # ---- (b) a draft call against the plain call ----
            kw = dict(max_new_tokens=n + 2, min_new_tokens=n + 2, want_alignment=True, **OFF)
            plain = eng.generate_greedy(ids[:rs, :1], **kw)
            assert eng.last_prompt_rows() == {"launches": 0, "positions": 0}, w_
            L, seq = plain["length"], plain["sequences"]
            al_p = eng.get_alignment(rs, L - 1)
            assert L == n + 3
            out = eng.generate_greedy(seq[:, :n].astype(np.int32), n_draft=n - 1, **kw)
            dr = out["draft"]
            assert dr["launches"] >= 1 and dr["rounds"] == 1 and dr["accepted"] == (n - 1) * rs, (w_, dr)
            assert out["length"] == L and np.array_equal(out["sequences"], seq), (w_, dr)
            diff = np.argwhere((eng.get_alignment(rs, L - 1) != al_p).any(-1))
            assert not len(diff), (w_, "first (stream, head, position) whose row differs between the draft and the plain call", diff[0].tolist())
            # ---- (c) a call that ends with its rows launch, and records no alignment ----
            raw = eng.score_tokens(ids[:rs, :n + 1], 1, **OFF)["logprob_raw"].astype(np.float64)
            assert eng.last_cross_grid() == (2, rs, -(-n // 16)), (w_, "one workgroup per (head, stream, 16 positions)", eng.last_cross_grid())
            d = np.abs(raw[:, 1:] - lp[:rs, 1:n + 1])
            assert np.isfinite(raw).all() and (d <= ROWS_TOL).all(), (w_, "score_tokens against the stepped logits", float(d.max()))
            assert np.array_equal(eng.get_alignment(rs, L - 1), al_p), (w_, "score_tokens wrote alignment rows")
            if oracle:   # ---- (f) relative L2 per position over the streams, as test_gpu_cross's figure against the restatement ----
                q = lpq[:rs, 1:n + 1]
                rel = np.linalg.norm(raw[:, 1:] - q, axis=0) / np.linalg.norm(q, axis=0)
                worst = max(worst, float(rel.max()))
                assert (rel < FP8_TOL[dtype]).all(), (w_, "rows against the restatement", float(rel.max()), FP8_TOL[dtype])
        eng.score_tokens(ids[:1, :82], 1, **OFF)      # several launches: 81 positions of one stream, the last launch holds the rest
        rest = 81 % cap or cap
        assert eng.last_cross_grid() == (2, 1, -(-rest // 16)), (what, "last of several launches", eng.last_cross_grid())
        print(f"{what}: {len(shapes(cap))} shapes, every row on its target and equal to the stepped row"
              + (f"; against the restatement {worst:.2e} (bound {FP8_TOL[dtype]:g})" if oracle else ""))
    finally:
        eng.close()


@pytest.mark.parametrize("T,dtype", [(T, t) for T in (64, 100, 500, 1000, 1500) for t in ("fp8a16", "fp8f16", "fp8a8")
                                     if t != "fp8a8" or T in (100, 1500)])
def test_fp8_cross_rows_every_shape_against_the_steps(T, dtype):
    rows_case(T, dtype, f"fp8 cross rows T={T} {dtype}", (T, dtype) in ORACLE)


@pytest.mark.parametrize("dtype", ["fp8a16", "fp8f16"])
def test_fp8_cross_rows_near_uniform_attention_rows_equal_the_steps(dtype):
    """(e): every key carries weight and the normaliser is not 1 - a normaliser taken from another lane than the single-query kernel's,
    or a scaled probability formed in another order, differs in the last bit of some rows."""
    dims = wo.PRESETS["micro"]
    T, n_ref = 500, 70
    eng = make_engine(dims, wo.make_weights(dims, 0), T=T, max_batch=3, dtype=dtype, heads=[(0, 1), (1, 0)])
    try:
        mel = torch.from_numpy(wo.log_mel(clips(T * 320, 3), dims.n_mels)).cuda()
        ids = np.random.default_rng(9).integers(0, 50000, size=(3, n_ref)).astype(np.int32)
        eng.encode(mel); eng.cross_kv(3); eng.decoder_reset(3)
        nxt = [eng.decode_step(ids[:, p].tolist()).argmax(-1).cpu().numpy() for p in range(n_ref)]
        al = eng.get_alignment(3, n_ref)
        for rs, n in ((1, 64), (3, 21), (2, 17)):
            what = f"near-uniform fp8 cross rows {dtype} rs={rs} n={n}"
            eng.encode(mel[:rs]); eng.cross_kv(rs)
            out = eng.generate_greedy(ids[:rs, :n + 1], n_forced=n, max_new_tokens=n + 1, want_alignment=True, **OFF)
            assert eng.last_prompt_rows()["positions"] == n, what
            diff = np.argwhere((eng.get_alignment(rs, n) != al[:rs, :, :n]).any(-1))
            assert not len(diff), (what, "first (stream, head, position) whose row is not the stepped one", diff[0].tolist(), len(diff))
            assert np.array_equal(out["sequences"][:, n + 1], nxt[n][:rs]), what
    finally:
        eng.close()


# the FQ = false instantiations of dec_cross_attn_kv8_rows_kernel - and, through the steps they are compared with, of
# dec_cross_attn_kv8_kernel - that (1000, "fp8a16") leaves out: G = 1 (T = 100), 2 (600), 3 (1100) in bf16 and float16
PLAIN_MORE = [(100, "fp8a16"), (1100, "fp8a16"), (100, "fp8f16"), (600, "fp8f16"), (1100, "fp8f16")]


def plain_child(cases=((1000, "fp8a16"),)):
    """(d), in the child: TW_FUSE_CQ=0 is read once per process."""
    assert os.environ.get("TW_FUSE_CQ") == "0"
    for T, dtype in cases:
        rows_case(T, dtype, f"fp8 cross rows T={T} {dtype} plain sequence")


def test_fp8_cross_rows_on_the_plain_launch_sequence():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_cross_rows_fp8 import plain_child; plain_child()"],
                         env=dict(os.environ, TW_FUSE_CQ="0"), cwd=root, timeout=600, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("plain sequence:") == 1


def test_fp8_cross_rows_on_the_plain_launch_sequence_other_instantiations():
    """The `FQ = false` instantiations the test above does not launch (PLAIN_MORE), same assertions, one child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_cross_rows_fp8 import plain_child; plain_child(PLAIN_MORE)".replace("PLAIN_MORE", repr(PLAIN_MORE))],
                         env=dict(os.environ, TW_FUSE_CQ="0"), cwd=root, timeout=600, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("plain sequence:") == len(PLAIN_MORE)
