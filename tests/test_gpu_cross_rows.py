"""The ROWS flavour of the decoder cross attention (k_decode.hip: dec_cross_attn_rows_kernel - one workgroup per stream, head and
group of up to 16 of the stream's positions, column j of the MFMA B operands = position j of the group) against the one-position
kernel, on the pointer model of tests/cross_pointer_model.py (every query puts its probability on one frame the test chooses):

    T                64 (one key group), 100 (a masked tail inside a 64-key group), 500 (of Tp = 512), 750 (the two-pass form)
    streams rs       1, 2, 3, 16 (the first rs clips of the model)
    positions n      2, 5, 16, 17, 64 // rs per stream: a partial group, a full group, a second group with one column; with rs = 16
                     the launches hold 4 positions and a last one of 1 (which is the one-position kernel's)
    types            f32, bf16, f16 (the fp8 contexts' kernel, dec_cross_attn_kv8_kernel, keeps one workgroup per row)

Per (T, type), on one 16-stream engine.  The reference is stepped: `decode_step` over 65 positions of all 16 streams (a stream's
bits do not depend on the other rows of its launch, tests/test_gpu_draft.py), whose alignment rows peak on the model's targets.
(a) forced prefix: `generate_greedy(ids[:rs, :n + 1], n_forced=n)` runs positions 0 .. n - 1 in rows launches (`last_prompt_rows`
says how many): every alignment row peaks on the frame the model points it at and the rows are array_equal to the stepped ones.
(b) draft against plain: a one-token prompt decoded by steps (`last_prompt_rows`: no rows launch), then the same call with its own
n - 1 first tokens offered as a draft - positions 0 .. n - 1 in rows launches with logits (`draft`: launches >= 1, every token
confirmed, i.e. every row's arg-max over logits that are computed from the rows kernel's context vectors is the step's): ids and
alignment rows array_equal.  (c) `score_tokens` (rows launches that record no alignment): `logprob_raw` within test_gpu_score's
1e-4 of the float64 log-softmax of the stepped logits, and the alignment rows in the context are left as they were.
(d) One child process under TW_FUSE_CQ=0 (the query is loaded, not formed in LDS) repeats (a) - (c) for f32 at T = 100 and bf16 at 750.
(e) The pointer's rows are saturated, so their normaliser is exactly 1: on `make_weights` (near-uniform attention, T = 500) the
forced-prefix rows are array_equal to the stepped rows as well.
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
P = 96                      # positions of the model: 64 in a launch, and a few to generate behind them
N_REF = 65                  # stepped positions
STREAMS = (1, 2, 3, 16)
ROWS_TOL = 1e-4             # tests/test_gpu_score.py: TOL
PLAIN = [(100, "f32"), (750, "bf16")]
OFF = dict(begin_suppress=(), suppress=(), timestamps=False)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def positions_per_stream(rs):
    return sorted({2, 5, 16, 17, 64 // rs})


def rows_case(T, dtype, what):
    dims, w, g = xm.pointer_weights(T, P)
    ids = xm.pointer_ids(T, P)[:16]
    tg = xm.targets(ids, g)                                             # [16, 2, P]
    mel = torch.from_numpy(wo.log_mel(clips(T * 320, 16), dims.n_mels)).cuda()
    eng = make_engine(dims, w, T=T, max_batch=16, dtype=dtype, heads=xm.HEADS)
    try:
        # ---- the reference: one position per launch ----
        eng.encode(mel); eng.cross_kv(16); eng.decoder_reset(16)
        lp = np.zeros((16, N_REF), np.float64)
        for p in range(N_REF):
            z = eng.decode_step(ids[:, p].tolist()).double()
            if p + 1 < N_REF:
                nxt = torch.from_numpy(ids[:, p + 1].astype(np.int64)).cuda()
                lp[:, p + 1] = torch.log_softmax(z, -1).gather(1, nxt[:, None])[:, 0].cpu().numpy()
        al = eng.get_alignment(16, N_REF)
        assert np.isfinite(al).all() and np.array_equal(al.argmax(-1), tg[:, :, :N_REF]), (what, "the stepped rows miss their targets")
        for rs in STREAMS:
            eng.encode(mel[:rs]); eng.cross_kv(rs)
            for n in positions_per_stream(rs):
                w_ = f"{what} rs={rs} n={n}"
                per_launch = 64 // rs
                # ---- (a) forced prefix: positions 0 .. n - 1 as rows, tokens chosen by the test ----
                eng.generate_greedy(ids[:rs, :n + 1], n_forced=n, max_new_tokens=n + 2, want_alignment=True, **OFF)
                pr = eng.last_prompt_rows()
                assert pr == {"launches": -(-n // per_launch), "positions": n}, (w_, pr)
                al2 = eng.get_alignment(rs, n)
                miss = np.argwhere(al2.argmax(-1) != tg[:rs, :, :n])
                assert not len(miss), (w_, "first (stream, head, position) whose row peaks elsewhere", miss[0].tolist(),
                                       "target", int(tg[tuple(miss[0])]), "peak", int(al2[tuple(miss[0])].argmax()))
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
                # ---- (c) rows launches that record no alignment ----
                raw = eng.score_tokens(ids[:rs, :n + 1], 1, **OFF)["logprob_raw"].astype(np.float64)
                d = np.abs(raw[:, 1:] - lp[:rs, 1:n + 1])
                assert np.isfinite(raw).all() and (d <= ROWS_TOL).all(), (w_, "score_tokens against the stepped logits", float(d.max()))
                assert np.array_equal(eng.get_alignment(rs, L - 1), al_p), (w_, "score_tokens wrote alignment rows")
        print(f"{what}: {sum(len(positions_per_stream(rs)) for rs in STREAMS)} shapes, every row on its target and equal to the stepped row")
    finally:
        eng.close()


@pytest.mark.parametrize("T,dtype", [(T, t) for T in (64, 100, 500, 750) for t in ("f32", "bf16", "f16")])
def test_cross_rows_every_shape_against_the_steps(T, dtype):
    rows_case(T, dtype, f"cross rows T={T} {dtype}")


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_cross_rows_near_uniform_attention_rows_equal_the_steps(dtype):
    """The pointer model's softmax rows are saturated: their normaliser is 1 whatever order it is added in.  On `make_weights` the cross
    attention is near-uniform over T = 500 frames, every key carries weight, and an alignment row is the probabilities x 1 / L as the
    kernel formed them: the rows of a forced-prefix call (rs = 1: 64 positions, four full groups; rs = 3: 21 positions, a group of 5
    columns) are array_equal to the stepped rows, and so are the ids generated behind them.  (A normaliser taken from another lane of the
    wavefront than the single-query kernel's differs in the last bit in some rows: tw_wave_sum's lanes do not all add in one order.)"""
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    heads = [(0, 1), (1, 0)]
    T, n_ref = 500, 70
    eng = make_engine(dims, w, T=T, max_batch=3, dtype=dtype, heads=heads)
    try:
        mel = torch.from_numpy(wo.log_mel(clips(T * 320, 3), dims.n_mels)).cuda()
        ids = np.random.default_rng(9).integers(0, 50000, size=(3, n_ref)).astype(np.int32)
        eng.encode(mel); eng.cross_kv(3); eng.decoder_reset(3)
        nxt = [eng.decode_step(ids[:, p].tolist()).argmax(-1).cpu().numpy() for p in range(n_ref)]
        al = eng.get_alignment(3, n_ref)
        for rs, n in ((1, 64), (3, 21), (2, 17)):
            what = f"near-uniform cross rows {dtype} rs={rs} n={n}"
            eng.encode(mel[:rs]); eng.cross_kv(rs)
            out = eng.generate_greedy(ids[:rs, :n + 1], n_forced=n, max_new_tokens=n + 1, want_alignment=True, **OFF)
            assert eng.last_prompt_rows()["positions"] == n, what
            al2 = eng.get_alignment(rs, n)
            diff = np.argwhere((al2 != al[:rs, :, :n]).any(-1))
            assert not len(diff), (what, "first (stream, head, position) whose row is not the stepped one", diff[0].tolist(), len(diff))
            # the token behind the prefix is the step's arg-max at position n (teacher-forced on the same ids)
            assert np.array_equal(out["sequences"][:, n + 1], nxt[n][:rs]), what
    finally:
        eng.close()


def plain_child():
    """(d), in the child: TW_FUSE_CQ=0 is read once per process."""
    assert os.environ.get("TW_FUSE_CQ") == "0"
    for T, dtype in PLAIN:
        rows_case(T, dtype, f"cross rows T={T} {dtype} plain sequence")


def test_cross_rows_on_the_plain_launch_sequence():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_cross_rows import plain_child; plain_child()"],
                         env=dict(os.environ, TW_FUSE_CQ="0"), cwd=root, timeout=600, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("plain sequence:") == len(PLAIN)
