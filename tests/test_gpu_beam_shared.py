"""Beam search reads a clip's cross K / V^T once for all of its beams (the beams mode of dec_cross_attn_rows_kernel: beam k of clip c
is launch row k n + c and attends to SLOT c) and writes no cross-K/V slot.

  1. f32 against tests/beam_judge.py with FOREIGN clips in the slots behind the clips (a flavour that read slot k n + c fails);
  2. the slots behind the clips survive a beam call: a greedy call over all of them, before and after, without re-encoding;
  3. tw_last_cross_grid reads (heads, n_clips, 1) behind a beam call;
  4. f16 / bf16 with want_alignment: ids, score bits and gathered alignment rows do not depend on what the other slots hold.
"""
import dataclasses

import numpy as np
import pytest
import torch

from tests import beam_judge as bj
from tests import eos_model as em
from tests.test_gpu_beam import _score_tol
from tests.util import clips, make_engine
from oracle import whisper_oracle as wo

pytestmark = pytest.mark.gpu
POOL = 64      # clips(.., POOL): the first em.N_CLIPS are eos_model's; prompts are em.prompt's rows for every index
# (n_clips, K) -> (case of bj.CASE_LIST the options are taken from, {T: clips whose smallest decision gap by the judge, at THIS K and T,
# is >= the case's gap_min - asserted before the device is asked}).  T = 99: masked tail keys; T = 600: Tp = 640, several key chunks
SHAPES = {
    (1, 2): ("k2-ts", {em.T: [0], 99: [0]}),
    (1, 8): ("k5-ts", {em.T: [2], 99: [18]}),
    (3, 8): ("k5-ts", {em.T: [2, 7, 8], 99: [18, 22, 25], 600: [4, 6, 13]}),
    (8, 8): ("k5-ts", {em.T: [2, 7, 8, 10, 16, 30, 32, 36], 99: [18, 22, 25, 30, 49, 50, 51, 54]}),
    (5, 3): ("k3-ts-early", {em.T: [0, 1, 2, 4, 5], 99: [1, 2, 3, 4, 5]}),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(dtype="f32", T=em.T):
        if (dtype, T) not in made:
            dims, w = em.model(2.5)
            made[(dtype, T)] = make_engine(dims, w, T=T, max_batch=64, dtype=dtype, heads=em.HEADS)
        return made[(dtype, T)]

    yield get
    for e in made.values():
        e.close()


def _fill(eng, slots, T=em.T):
    """Slot i of the context <- clip slots[i] of the pool."""
    eng.encode(eng.logmel(torch.from_numpy(clips(T * 320, POOL)[list(slots)]).cuda(), out_dtype=torch.float32))
    eng.cross_kv(len(slots))


def _foreign(sel, rows):
    """`sel` in the first slots and `rows - len(sel)` OTHER clips behind them: slot k n + c, k >= 1, never holds clip sel[c]."""
    return list(sel) + [i for i in range(POOL) if i not in sel][: rows - len(sel)]


# ---- 1. foreign clips behind the clips, against the judge -------------------------------------------------------------------------
@pytest.mark.parametrize("shape,T", [(s, T) for s in SHAPES for T in SHAPES[s][1]], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"T{v}")
def test_f32_parity_with_the_judge_among_foreign_clips(engines, shape, T):
    n, K = shape
    name, sel = SHAPES[shape][0], SHAPES[shape][1][T]
    case = dataclasses.replace(bj.case(name), K=K)
    dims, w = em.model(case.es)
    om = wo.OracleWhisper(dims, w, T=T)
    enc = om.encode(wo.log_mel(clips(T * 320, POOL)[sel], dims.n_mels))
    refs = [bj.run_clip(om, enc[i : i + 1], em.prompt([c])[0], case.options(), K, case.length_penalty, case.early) for i, c in enumerate(sel)]
    assert all(bj.min_gap(r) >= case.gap_min and r["finite"] for r in refs), [bj.min_gap(r) for r in refs]
    eng = engines("f32", T)
    _fill(eng, _foreign(sel, n * K), T)
    res = eng.generate_beam(em.prompt(sel), **case.engine_kw())
    worst = 0.0
    for i, ref in enumerate(refs):
        for k, h in enumerate(ref["nbest"]):
            row = res["nbest_sequences"][i, k]
            assert row[: len(h)].tolist() == list(h) and (row[len(h):] == em.EOS).all(), (shape, T, sel[i], k, row.tolist(), list(h))
        live = ref["scores"] > -1e8
        assert (res["nbest_scores"][i][~live] <= -1e9).all(), (shape, T, sel[i])
        if live.any():
            worst = max(worst, float(np.abs(res["nbest_scores"][i].astype(np.float64) - ref["scores"].astype(np.float64))[live].max()))
    print(f"{n} clips x {K} beams, T = {T}: ids equal the judge's, largest score difference {worst:.3e} (tolerance {_score_tol(case):.1e})")
    assert worst <= _score_tol(case), (shape, T, worst)


# ---- 2. the other slots survive ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_slots_behind_the_clips_survive_a_beam_call(engines, dtype):
    (n, K), name, sel = (5, 3), SHAPES[(5, 3)][0], SHAPES[(5, 3)][1][em.T]
    slots = _foreign(sel, n * K)
    eng = engines(dtype)
    _fill(eng, slots)
    gkw = em.engine_kw(True, 12)
    before = eng.generate_greedy(em.prompt(slots), **gkw)["sequences"]
    assert len({tuple(r) for r in before.tolist()}) > n, "the slots must differ for the test to see anything"
    eng.generate_beam(em.prompt(sel), **bj.case(name).engine_kw())
    after = eng.generate_greedy(em.prompt(slots), **gkw)["sequences"]       # no re-encoding
    assert np.array_equal(before, after), (dtype, np.nonzero((before != after).any(axis=1))[0].tolist())


# ---- 3. grid ----------------------------------------------------------------------------------------------------------------------
def test_cross_grid_of_a_beam_step_is_heads_by_clips(engines):
    (n, K), name, sel = (3, 8), SHAPES[(3, 8)][0], SHAPES[(3, 8)][1][em.T]
    eng = engines("f32")
    _fill(eng, _foreign(sel, n * K))
    H = em.model(2.5)[0].heads
    eng.decoder_reset(n * K)
    eng.decode_step([3] * (n * K), want_logits=False)
    assert eng.last_cross_grid() == (H, n * K, 1)                         # a one-position step: one workgroup per (head, row)
    eng.generate_beam(em.prompt(sel), **dataclasses.replace(bj.case(name), K=K).engine_kw())
    assert eng.last_cross_grid() == (H, n, 1)


# ---- 4. bits do not depend on the other slots ---------------------------------------------------------------------------------------
def bits_case(get, shape, dtype, T=em.T):
    n, K = shape
    name, sel = SHAPES[shape][0], SHAPES[shape][1][T]
    kw = dataclasses.replace(bj.case(name), K=K).engine_kw()
    eng = get(dtype, T)
    got = []
    for slots in (_foreign(sel, n * K), [sel[c] for _ in range(K) for c in range(n)]):   # foreign clips | slot k n + c holds clip c
        _fill(eng, slots, T)
        res = eng.generate_beam(em.prompt(sel), **kw, want_alignment=True)
        got.append((res, eng.get_alignment(n * K, res["nbest_sequences"].shape[2] - 1)))
    (a, rows_a), (b, rows_b) = got
    for key in ("nbest_sequences", "nbest_scores", "nbest_lengths"):      # (tobytes: the scores bit for bit)
        assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), (shape, dtype, T, key)
    live = [(c, k, int(a["nbest_lengths"][c, k])) for c in range(n) for k in range(K) if a["nbest_scores"][c, k] > -1e9]
    assert len(live) >= n
    for c, k, L in live:
        assert np.array_equal(rows_a[k * n + c, :, : L - 1].view(np.int32), rows_b[k * n + c, :, : L - 1].view(np.int32)), (shape, dtype, T, c, k)
    print(f"beams bits {dtype} T={T} {n}x{K}: independent of the other slots")


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("shape", [(3, 8), (5, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_bits_do_not_depend_on_the_other_slots(engines, shape, dtype):
    bits_case(engines, shape, dtype)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_bits_do_not_depend_on_the_other_slots_two_pass(engines, dtype):
    """T = 600 -> Tp = 640: the two-pass (SINGLE = false) instantiations of the beams mode in the 16-bit types (f32: test 1)."""
    bits_case(engines, (3, 8), dtype, 600)


# ---- 5. the plain launch sequence (FQ = false: the query is loaded, not formed in LDS) ------------------------------------------------
PLAIN = [(t, T) for t in ("f32", "f16", "bf16") for T in (em.T, 600)]     # SINGLE and two-pass


def plain_child():
    """In the child: TW_FUSE_CQ=0 is read once per process."""
    import os
    assert os.environ.get("TW_FUSE_CQ") == "0"
    made = {}

    def get(dtype, T):
        if (dtype, T) not in made:
            dims, w = em.model(2.5)
            made[(dtype, T)] = make_engine(dims, w, T=T, max_batch=64, dtype=dtype, heads=em.HEADS)
        return made[(dtype, T)]

    try:
        for dtype, T in PLAIN:
            bits_case(get, (3, 8), dtype, T)
    finally:
        for e in made.values():
            e.close()


def test_bits_do_not_depend_on_the_other_slots_on_the_plain_launch_sequence():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_beam_shared import plain_child; plain_child()"],
                         env=dict(os.environ, TW_FUSE_CQ="0"), cwd=root, timeout=600, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("independent of the other slots") == len(PLAIN)
