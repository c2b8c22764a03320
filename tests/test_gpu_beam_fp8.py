"""Beam search in the float16 fp8 context ("fp8f16", TW_F16_W8A16): k_decode_kv8_beams.hip, dec_cross_attn_kv8_beams_kernel<f16_t, G, FQ>.
  1. ids and scores against float64: tests/beam_judge.py over test_gpu_fp8_f16.Ref(fp8=True) on the context's own encoder states;
  2. the context's own scoring pass (the pinned rows kernel) reproduces every live hypothesis's score at Tp = 128, 640, 1152 (G = 1, 2,
     3, each with a masked tail), up to 64 rows; the grid is (heads, clips, 1); no cross-K/V slot is written;
  3. ids, lengths, score bits and gathered alignment rows do not depend on the other slots, on batch-mates or on use_graph - also on
     the plain launch sequence (TW_FUSE_CQ=0: FQ = false), in a child process;  4. the pipeline seam.
D16: the largest |score - judge's score| of the EXISTING "f16" context against Ref(fp8=False) over every clip of the pool whose ids equal
the judge's, in the settings k2-ts (K = 2), k5-ts at K = 8, k3-ts-early (K = 3): 5.05e-4, 5.21e-4, 5.05e-4 on 2026-11-26 (fp8f16 that day:
3.3e-4, 5.4e-4, 5.5e-4).  TOL = 2 D16, the margin test_projection_rule gives fp8f16 over f16.  Test 1 takes the clips whose smallest
decision gap by the judge is >= 4 TOL = 4.2e-3: 16 and 49 at K = 2 (1.07e-2, 4.49e-3).  The pool's largest gap is 2.6e-3 at K = 3 and 3.8e-4
at K = 8, so the shapes (5, 3) and (3, 8) shrink to (2, 2); K = 3 and 8 are covered by tests 2 and 3, which are exact."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_judge as bj
from tests import eos_model as em
from tests.test_gpu_beam import STALE_TOL
from tests.test_gpu_beam_shared import POOL, _fill, _foreign
from tests.test_gpu_fp8_f16 import Ref
from tests.util import clips, make_engine

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="needs the MI355X")]
D16 = 5.21e-4          # 2026-11-26
TOL = 2 * D16
PARITY = {(1, 2): [16], (2, 2): [16, 49]}                                   # case k2-ts
EXACT = [(100, (3, 8)), (100, (5, 3)), (600, (3, 8)), (1100, (3, 8))]       # case k5-ts at the shape's K; clips 0 .. n - 1
ENGINES = {}                                                                # shared by the tests of the module (and of the child)


def engine(T=em.T, graph=False):
    if (T, graph) not in ENGINES:
        ENGINES[(T, graph)] = make_engine(*em.model(2.5), T=T, max_batch=64, dtype="fp8f16", heads=em.HEADS, use_graph=graph)
    return ENGINES[(T, graph)]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    while ENGINES:
        ENGINES.popitem()[1].close()


def _kw(K):
    return dataclasses.replace(bj.case("k5-ts"), K=K).engine_kw()


@pytest.mark.parametrize("shape", list(PARITY), ids=lambda s: f"{s[0]}x{s[1]}")
def test_float64_parity(shape):
    (n, K), sel, case = shape, PARITY[shape], bj.case("k2-ts")
    eng, ref = engine(), Ref(*em.model(case.es), True)
    mel = eng.logmel(torch.from_numpy(clips(em.T * 320, POOL)[_foreign(sel, n * K)]).cuda(), out_dtype=torch.float32)
    enc = eng.encode(mel, return_hidden=True).double().cpu().numpy()
    eng.cross_kv(n * K)
    refs = [bj.run_clip(ref, enc[i : i + 1], em.prompt([c])[0], case.options(), K, case.length_penalty, case.early) for i, c in enumerate(sel)]
    assert all(bj.min_gap(r) >= 4 * TOL and r["finite"] for r in refs), [bj.min_gap(r) for r in refs]
    res = eng.generate_beam(em.prompt(sel), **case.engine_kw())
    worst = 0.0
    for i, r in enumerate(refs):
        for k, h in enumerate(r["nbest"]):
            row = res["nbest_sequences"][i, k]
            assert row[: len(h)].tolist() == list(h) and (row[len(h):] == em.EOS).all(), (shape, sel[i], k, row.tolist(), list(h))
        live = r["scores"] > -1e8
        assert (res["nbest_scores"][i][~live] <= -1e9).all(), (shape, sel[i])
        worst = max(worst, float(np.abs(res["nbest_scores"][i].astype(np.float64) - r["scores"].astype(np.float64))[live].max(initial=0.0)))
    print(f"{n} clips x {K} beams: ids equal the float64 judge's, largest score difference {worst:.3e} (tolerance {TOL:.2e})")
    assert worst <= TOL, (shape, worst)


@pytest.mark.parametrize("T,shape", EXACT[:1] + [(100, (8, 8))] + EXACT[2:], ids=lambda v: str(v).replace(", ", "x"))
def test_scoring_pass_reproduces_every_hypothesis(T, shape):
    (n, K), eng, n0 = shape, engine(T), em.N_PROMPT
    slots = _foreign(range(n), 64)
    _fill(eng, slots, T)
    before = eng.generate_greedy(em.prompt(slots), **em.engine_kw(True, 12))["sequences"]
    res = eng.generate_beam(em.prompt(range(n)), **_kw(K))
    assert eng.last_cross_grid() == (em.model(2.5)[0].heads, n, 1)
    skw = {k: v for k, v in _kw(K).items() if k not in ("num_beams", "length_penalty", "early_stopping")}
    worst, n_live = 0.0, 0
    for k in range(K):   # hypothesis k of every clip: row c of the scoring pass attends to slot c
        raw = eng.score_tokens(res["nbest_sequences"][:, k], n0, **skw)["logprob_raw"]
        for c in range(n):
            L, s = int(res["nbest_lengths"][c, k]), float(res["nbest_scores"][c, k])
            if s > -1e9:
                total = np.float32(raw[c, n0:L].astype(np.float64).sum()) / bj.pen(L - n0, 1.0)
                worst, n_live = max(worst, abs(float(total) - s)), n_live + 1
    print(f"T = {T}, {n} x {K}: {n_live} live hypotheses, largest |rescored - returned| {worst:.3e} (tolerance {STALE_TOL['f16']['norm']:.1e})")
    assert n_live >= n and worst <= STALE_TOL["f16"]["norm"], (T, shape, n_live, worst)
    after = eng.generate_greedy(em.prompt(slots), **em.engine_kw(True, 12))["sequences"]
    assert np.array_equal(before, after), np.nonzero((before != after).any(axis=1))[0].tolist()


def _hyps(T, sel, K, slots, graph=False):
    """Per (clip, hypothesis) of a want_alignment call: ids, length, score bits and - if live - the gathered alignment rows as bytes."""
    eng, n = engine(T, graph), len(sel)
    _fill(eng, slots, T)
    res = eng.generate_beam(em.prompt(sel), **_kw(K), want_alignment=True)
    rows = eng.get_alignment(n * K, res["nbest_sequences"].shape[2] - 1)
    out = []
    for c in range(n):
        for k in range(K):
            L, s = int(res["nbest_lengths"][c, k]), res["nbest_scores"][c, k]
            out.append((res["nbest_sequences"][c, k, :L].tolist(), L, s.tobytes(), rows[k * n + c, :, : L - 1].tobytes() if s > -1e9 else b""))
    assert sum(1 for h in out if h[3]) >= n
    return out


def bits_case(T, shape):
    (n, K), sel = shape, list(range(shape[0]))
    a = _hyps(T, sel, K, _foreign(sel, n * K))
    assert a == _hyps(T, sel, K, [c for _ in range(K) for c in sel]), (T, shape, "slot k n + c holds clip c")
    assert a == _hyps(T, sel, K, _foreign(sel, n * K), graph=True), (T, shape, "use_graph")
    for c in (0, n - 1):
        assert a[c * K : (c + 1) * K] == _hyps(T, [c], K, [c]), (T, shape, c, "alone")
    print(f"fp8f16 beams bits T={T} {n}x{K}: independent of slots, batch-mates and use_graph")


@pytest.mark.parametrize("T,shape", EXACT, ids=lambda v: str(v).replace(", ", "x"))
def test_bits(T, shape):
    bits_case(T, shape)


def plain_child():
    assert os.environ.get("TW_FUSE_CQ") == "0"   # read once per process
    for T, shape in EXACT:
        bits_case(T, shape)


def test_bits_on_the_plain_launch_sequence():
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_beam_fp8 import plain_child; plain_child()"], timeout=600, text=True,
                         env=dict(os.environ, TW_FUSE_CQ="0"), cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), capture_output=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("independent of slots") == len(EXACT)


def test_pipeline_seam():
    from oracle import hf_reference as hr
    from oracle import whisper_oracle as wo
    from thewhisper_amd import ASRPipeline
    dims = wo.PRESETS["micro"]
    pipe = ASRPipeline(hr.build_hf_model(dims, wo.make_weights(dims, 0)), feature_extractor=hr.build_feature_extractor(dims, 10), batch_size=3,
                       tokenizer=hr.build_tokenizer(dims), chunk_length_s=10, device="cuda", torch_dtype=torch.float16, decoder_weights="fp8")
    eng = pipe.model.engine
    try:
        pipe.model.beam_search = True
        f = pipe.feature_extractor([wo.synth_audio(160000, 0, "speechlike")], sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        calls, inner = [], eng.generate_beam
        eng.generate_beam = lambda *a, **k: calls.append((a, k)) or inner(*a, **k)
        seq = pipe.model.generate(input_features=f.input_features.cuda(), attention_mask=f.attention_mask.cuda(), num_beams=3, do_sample=False,
                                  use_cache=True, language="en", max_new_tokens=12)
        seq = (seq["sequences"] if isinstance(seq, dict) else seq).tolist()
        assert eng.tw_dtype == 5 and len(calls) == 1 and calls[0][0][1] == 3 and eng.last_cross_grid()[1:] == (1, 1)
        direct = inner(*calls[0][0], **calls[0][1])["sequences"]     # the same prompt and options, on the engine: HF cuts the prompt off
        assert len(seq[0]) == 12 and seq == direct[:, calls[0][0][0].shape[1]:].tolist()
    finally:
        eng.close()
