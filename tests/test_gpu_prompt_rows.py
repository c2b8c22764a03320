"""The plain greedy call takes its prompt as ONE rows-mode launch (api.hip: generate_loop) when n_prompt >= 2 and n_prompt x B fits
the 64 rows of a launch, and the result is the step path's, bit for bit.

The reference needs no switch: a stream's bits do not depend on who else is in its launch, and a call whose
n_prompt x B exceeds 64 rows consumes its prompt one position per step.  So the same <= 16 clips are decoded twice - as a call of their
own (`last_prompt_rows`: one launch over n_prompt positions) and as the first streams of a 40-stream call (`last_prompt_rows`: none) -
and ids, length and token timestamps of those streams are array_equal.  Micro model (d = 128, 2 heads, 2 + 2 layers), T = 100, 12 new
tokens (<eos> masked up to there: the length is not set by the other 24 streams), per-stream prompts; timestamps on and off, graph replay
on and off, f32 / f16 / bf16.  Shapes (n_prompt, streams): (1, 16) - nothing to take as rows -, (2, 16), (3, 16), (4, 16) - exactly 64
rows -, (5, 12) and (5, 13) - 65 rows: the step path, asserted.  In strict f32 the ids are the numpy oracle's too.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests.util import PROMPT, clips, make_engine

pytestmark = pytest.mark.gpu
T, N_ALL, NEW = 100, 40, 12
HEADS = [(1, 0), (1, 1)]
SHAPES = [(1, 16), (2, 16), (3, 16), (4, 16), (5, 12), (5, 13)]
DIMS = wo.PRESETS["micro"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@functools.lru_cache(maxsize=None)
def _pcm():
    return clips(T * 320, N_ALL)


def _prompt(n):
    """int32 [N_ALL, n]: <sot>, then tokens that differ from stream to stream (a row table that mixes streams or positions shows)."""
    b = np.arange(N_ALL)
    cols = [np.full(N_ALL, PROMPT[0]), PROMPT[1] + b % 40, np.full(N_ALL, PROMPT[2]), 1000 + 7 * b, 2000 + 11 * b]
    return np.ascontiguousarray(np.stack(cols[:n], axis=1).astype(np.int32))


@functools.lru_cache(maxsize=None)
def _oracle_ids(n, B, ts_on):
    om = wo.OracleWhisper(DIMS, wo.make_weights(DIMS, 0), T=T)
    opt = wo.GreedyOptions(max_new_tokens=NEW, min_new_tokens=NEW, timestamps=ts_on, alignment_heads=HEADS)
    return wo.greedy_generate(om, om.encode(wo.log_mel(_pcm()[:B], DIMS.n_mels)), _prompt(n)[:B], opt)["sequences"]


@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("ts_on", [True, False])
def test_prompt_as_rows_is_the_step_path(ts_on, graph, dtype):
    eng = make_engine(DIMS, wo.make_weights(DIMS, 0), T=T, max_batch=N_ALL, dtype=dtype, heads=HEADS, use_graph=graph)
    try:
        mel = eng.logmel(torch.from_numpy(_pcm()).cuda(), out_dtype=torch.float32)
        kw = dict(max_new_tokens=NEW, min_new_tokens=NEW, timestamps=ts_on, want_alignment=True)
        for n, B in SHAPES:
            what = f"{dtype} graph={graph} timestamps={ts_on}: n_prompt={n} B={B}"
            prompt = _prompt(n)
            # the streams among 40: n x 40 rows do not fit a launch
            eng.encode(mel); eng.cross_kv(N_ALL)
            ref = eng.generate_greedy(prompt, **kw)
            assert eng.last_prompt_rows() == {"launches": 0, "positions": 0}, what
            L = ref["length"]
            ts_ref = eng.token_timestamps(N_ALL, n, L, [2 * T] * N_ALL)[:B]
            steps_ref = eng.last_timings()["decode_steps"]
            # the streams as a call of their own
            eng.encode(mel[:B]); eng.cross_kv(B)
            out = eng.generate_greedy(prompt[:B], **kw)
            want = {"launches": 1, "positions": n} if (n >= 2 and n * B <= 64) else {"launches": 0, "positions": 0}
            assert eng.last_prompt_rows() == want, (what, eng.last_prompt_rows())
            assert L == n + NEW and out["length"] == L, (what, out["length"], L)
            bad = np.argwhere(out["sequences"] != ref["sequences"][:B])
            assert not len(bad), (what, "first (stream, position) whose id differs", bad[0].tolist())
            assert np.array_equal(eng.token_timestamps(B, n, L, [2 * T] * B), ts_ref), what
            assert eng.last_timings()["decode_steps"] == steps_ref >= L - 1, what     # positions consumed, whichever way
            if dtype == "f32":
                assert np.array_equal(out["sequences"], _oracle_ids(n, B, ts_on)), (what, "the numpy oracle's ids")
    finally:
        eng.close()
