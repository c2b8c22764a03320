"""Beam search on the device (tw_generate_beam; k_decode.hip: beam_part_kernel, beam_finish_kernel, beam_reorder_kernel) against
tests/beam_judge.py, the numpy restatement of the rule that tests/test_beam_judge.py pins to HF's own generate.

  1. strict f32 parity: every case of beam_judge.CASES, every selected clip, all K hypotheses id for id, scores within SCORE_TOL;
  2. batch and slot independence in f32, f16 and bf16: a clip alone, in a 7-clip K = 5 call (35 rows: three groups of 16), in an
     8-clip K = 3 call (a clip's rows on both sides of rows 15 / 16), with and without use_graph - ids and score BITS identical;
  3. the cache reorder on both sides of the 64-key bucket boundary (58-token prompt, 12 new tokens);
  4. stale-cache check in every dtype: tw_score_tokens on the best hypothesis right after the beam call, WITHOUT re-encoding, gives
     the returned score; a wrongly gathered cache row misses by orders of magnitude;
  5. every TW_EINVAL / TW_ESTATE of the header; after each a plain greedy call returns its usual ids;
  6. the HF seam and the pipeline on the real engine in strict f32: HF's own generate's ids with num_beams = 3.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_beam.py -s`` prints each case's figures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import beam_judge as bj
from tests import eos_model as em
from tests.util import make_engine
from thewhisper_amd import _cabi

pytestmark = pytest.mark.gpu
TW_EINVAL, TW_ESTATE = -1, -3     # include/thewhisper.h
# Largest |device score - judge score| seen on the first run (both float32, other summation orders), asserted at 4x:
#   length-normalised cases (scores of a few units)   1.43e-6 -> 5.8e-6, within GAP_MIN / 4 = 2.5e-5;
#   length_penalty 0 (plain sums near -100, where float32 has steps of 7.6e-6: the difference is three of them)   2.29e-5 -> 9.2e-5.
# The second exceeds 2.5e-5, so those cases select their clips at the larger gap GAP_MIN_SUM = 4e-4 (beam_judge.Case.gap_min): the
# tolerance stays a quarter of the gap condition, and equal ids still follow from it.
SCORE_TOL = 5.8e-6
SCORE_TOL_SUM = 9.2e-5


def _score_tol(case):
    return SCORE_TOL_SUM if case.length_penalty == 0.0 else SCORE_TOL


# |sum(raw log-probabilities of tw_score_tokens) / pen - returned score|, largest seen on the first run, asserted at 4x: f32 against
# the judge's figure too, f16 / bf16 against the same context's own scoring pass (same kernels, rows mode).  Seen: f32 4.8e-7 / 1.53e-5
# (length-normalised / plain sums near -100, i.e. two float32 steps there), f16 9.5e-7 / 1.53e-5, bf16 9.5e-7 / 2.29e-5.
STALE_TOL = {"f32": {"norm": 1.9e-6, "sum": 6.1e-5}, "f16": {"norm": 3.8e-6, "sum": 6.1e-5}, "bf16": {"norm": 3.8e-6, "sum": 9.2e-5}}
assert SCORE_TOL <= bj.GAP_MIN / 4 and SCORE_TOL_SUM <= bj.GAP_MIN_SUM / 4


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(es, dtype="f32", graph=False, max_batch=64):
        key = (es, dtype, graph, max_batch)
        if key not in made:
            dims, w = em.model(es)
            made[key] = make_engine(dims, w, T=em.T, max_batch=max_batch, dtype=dtype, heads=em.HEADS, use_graph=graph)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _fill(eng, sel):
    eng.encode(eng.logmel(torch.from_numpy(em.audio(sel)).cuda(), out_dtype=torch.float32))
    eng.cross_kv(len(sel))


def _hyp_len(row, n0, score, max_len):
    """Tokens of a returned hypothesis (pad == <eos> on this model): up to its first <eos> behind the prompt, else max_len; a pure
    placeholder (score <= -1e9 and nothing generated) is the prompt."""
    gen = np.nonzero(row[n0:] == em.EOS)[0]
    return n0 + int(gen[0]) + 1 if gen.size else min(len(row), max_len)


def _assert_ids(res, i, ref, what):
    """All K hypotheses of row i equal the judge's, id for id; everything behind a hypothesis's end is pad."""
    nb = res["nbest_sequences"][i]
    for k, h in enumerate(ref["nbest"]):
        assert nb.shape[1] >= len(h), (what, k, nb.shape, len(h))
        assert nb[k, : len(h)].tolist() == list(h), (what, k, nb[k].tolist(), list(h))
        assert (nb[k, len(h):] == em.EOS).all(), (what, k)
    best = res["sequences"][i]
    h = ref["nbest"][0]
    assert best[: len(h)].tolist() == list(h) and (best[len(h):] == em.EOS).all(), (what, "best")


# ---- 1. strict f32 parity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in bj.CASE_LIST])
def test_f32_parity_with_the_judge(engines, name):
    case = bj.case(name)
    sel = list(bj.CASES[name])[: 64 // case.K]
    eng = engines(case.es)
    _fill(eng, sel)
    res = eng.generate_beam(em.prompt(sel), **case.engine_kw())
    worst = 0.0
    for i, clip in enumerate(sel):
        ref = bj.run(case, clip)
        _assert_ids(res, i, ref, (name, clip))
        d = np.abs(res["nbest_scores"][i].astype(np.float64) - ref["scores"].astype(np.float64))
        live = ref["scores"] > -1e8
        worst = max(worst, float(d[live].max()) if live.any() else 0.0)
        assert np.array_equal(res["nbest_scores"][i][~live] <= -1e9, np.ones((~live).sum(), bool)), (name, clip)
        assert res["scores"][i] == res["nbest_scores"][i][0]
    print(f"{name}: {len(sel)} clips x {case.K} beams, largest score difference {worst:.3e} (tolerance {_score_tol(case):.1e})")
    assert worst <= _score_tol(case), (name, worst)
    assert res["sequences"].shape[1] == max(len(bj.run(case, c)["nbest"][0]) for c in sel)


# ---- 2. batch and slot independence, graph or not -----------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_result_does_not_depend_on_batch_slot_or_graph(engines, dtype):
    base = bj.case("k5-ts")
    for K, sel in ((5, [0, 1, 2, 5, 6, 7, 8]), (3, [0, 1, 2, 4, 5, 6, 8, 9])):   # 35 rows | rows 0 .. 23: clip 7 of 8 sits on rows 7, 15, 23
        kw = dict(base.engine_kw(), num_beams=K)
        outs = {}
        for graph in (False, True):
            eng = engines(base.es, dtype, graph)
            _fill(eng, sel)
            outs[graph] = eng.generate_beam(em.prompt(sel), **kw)
        for key in ("nbest_sequences", "nbest_scores", "sequences", "scores"):
            a, b = outs[False][key], outs[True][key]
            assert a.shape == b.shape and np.array_equal(a.view(np.int32) if a.dtype == np.float32 else a,
                                                         b.view(np.int32) if b.dtype == np.float32 else b), (dtype, K, key, "graph")
        eng = engines(base.es, dtype, False)
        n_alone = 0
        for i in (0, len(sel) - 1, 3):
            _fill(eng, [sel[i]])
            one = eng.generate_beam(em.prompt([sel[i]]), **kw)
            L = one["nbest_sequences"].shape[2]
            big = outs[False]["nbest_sequences"][i]
            assert np.array_equal(big[:, :L], one["nbest_sequences"][0]) and (big[:, L:] == em.EOS).all(), (dtype, K, sel[i], "ids")
            assert np.array_equal(outs[False]["nbest_scores"][i].view(np.int32), one["nbest_scores"][0].view(np.int32)), (dtype, K, sel[i], "bits")
            n_alone += 1
        print(f"{dtype} K={K}: {len(sel)} clips, {n_alone} of them alone: ids and score bits identical; graph on/off identical")


# ---- 3. the reorder across a 64-key bucket -------------------------------------------------------------------------------
def test_reorder_on_both_sides_of_the_64_key_boundary(engines):
    case = bj.Case("k3-long", 2.0, False, 3, False, 1.0, max_new=12)
    prompt = tuple(int(x) for x in np.random.default_rng(59).integers(0, 700, size=58))
    sel = [2, 3]
    refs = [bj.run(case, c, prompt) for c in sel]
    late = [s["pos"] for s in refs[0]["steps"] if s["nonid"] and s["pos"] >= 64]
    early = [s["pos"] for s in refs[0]["steps"] if s["nonid"] and s["pos"] < 64]
    assert late and early and all(bj.min_gap(r) >= case.gap_min for r in refs), (late, early, [bj.min_gap(r) for r in refs])
    eng = engines(case.es)
    _fill(eng, sel)
    res = eng.generate_beam(np.tile(np.asarray(prompt, dtype=np.int32), (2, 1)), **case.engine_kw())
    for i, ref in enumerate(refs):
        _assert_ids(res, i, ref, ("long", sel[i]))
        assert np.abs(res["nbest_scores"][i] - ref["scores"]).max() <= SCORE_TOL
    print(f"58-token prompt: non-identity permutations at positions {early + late}, ids equal the judge's")


# ---- 4. stale-cache check ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_scoring_pass_reproduces_the_returned_score(engines, dtype):
    worst, worst_ref, misses = {}, 0.0, []
    for name in ("k3-ts-early", "k5-ts", "k3-text-lp0"):
        case = bj.case(name)
        sel = list(bj.CASES[name])[:6]
        eng = engines(case.es, dtype)
        _fill(eng, sel)
        kw = case.engine_kw()
        res = eng.generate_beam(em.prompt(sel), **kw)
        seq = res["sequences"]
        n0 = em.N_PROMPT
        assert seq.shape[1] >= n0 + 2, (dtype, name, seq.shape)      # something was generated
        sc = eng.score_tokens(seq, n0, **{k: v for k, v in kw.items() if k not in ("num_beams", "length_penalty", "early_stopping")})   # no re-encoding
        n_nonid = 0
        for i, clip in enumerate(sel):
            L = _hyp_len(seq[i], n0, res["scores"][i], n0 + case.max_new)
            total = np.float32(sc["logprob_raw"][i, n0:L].astype(np.float64).sum()) / bj.pen(L - n0, case.length_penalty)
            d = abs(float(total) - float(res["scores"][i]))
            if dtype == "f32":     # against the judge's figure
                d = max(d, abs(float(total) - float(bj.run(case, clip)["scores"][0])))
            kind = "sum" if case.length_penalty == 0.0 else "norm"
            worst[kind] = max(worst.get(kind, 0.0), d)
            if d > STALE_TOL[dtype][kind]:
                misses.append((dtype, name, clip, float(total), float(res["scores"][i])))
        # the clips are still there for a plain call, too
        g = eng.generate_greedy(em.prompt(sel), **em.engine_kw(case.timestamps, 8))
        _fill(eng, sel)
        g2 = eng.generate_greedy(em.prompt(sel), **em.engine_kw(case.timestamps, 8))
        assert np.array_equal(g["sequences"], g2["sequences"]), (dtype, name, "greedy after beam without re-encoding")
    print(f"{dtype}: largest |rescored - returned| {worst} (tolerances {STALE_TOL[dtype]})")
    assert not misses, misses


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def _raw_beam(eng, n, prompt, K=3, lp=1.0, early=0, max_length=448, **opt_over):
    kw = dict(eos_id=em.EOS, pad_id=em.EOS, timestamps=False, no_timestamps_id=em.NO_TS, max_initial_timestamp_index=None,
              begin_suppress=(), suppress=(), min_new_tokens=0, max_new_tokens=6, max_length=max_length)
    extra = {k: opt_over.pop(k) for k in ("want_alignment", "n_forced", "n_draft") if k in opt_over}
    kw.update(opt_over)
    o, _keep = eng._greedy_opts(**kw, **extra)
    bo = _cabi.tw_beam_opts()
    bo.num_beams, bo.length_penalty, bo.early_stopping = K, lp, early
    prompt = np.ascontiguousarray(prompt, dtype=np.int32)
    out = np.zeros((n, max_length), np.int32)
    out_len = (C.c_int32 * 2)()
    i32p = C.POINTER(C.c_int32)
    return eng.lib.tw_generate_beam(eng.ctx, n, prompt.ctypes.data_as(i32p), prompt.shape[1], C.byref(o), C.byref(bo),
                                    out.ctypes.data_as(i32p), out_len, None, None, None, eng._sp())


def test_refusals_leave_the_context_usable(engines):
    eng = engines(2.5, "f32", False, 12)
    sel = [0, 1, 5]
    _fill(eng, sel)
    p = em.prompt(sel)
    usual = eng.generate_greedy(p, **em.engine_kw(True, 8))["sequences"]
    bad = [
        ("num_beams 1", dict(K=1)), ("num_beams 9", dict(K=9)), ("rows above max_batch", dict(K=5)),
        ("nan length_penalty", dict(lp=float("nan"))), ("inf length_penalty", dict(lp=float("inf"))),
        ("early_stopping 2", dict(early=2)), ("early_stopping -1", dict(early=-1)), ("want_alignment", dict(want_alignment=True)),
        ("n_forced", dict(n_forced=1)), ("n_draft", dict(n_draft=1)), ("eos outside the vocabulary", dict(eos_id=em.V)),
        ("nothing to generate", dict(max_new_tokens=0)),
    ]
    for what, over in bad:
        rc = _raw_beam(eng, len(sel), p, **over)
        assert rc == TW_EINVAL, (what, rc, eng.lib.tw_last_error(eng.ctx))
        assert np.array_equal(eng.generate_greedy(p, **em.engine_kw(True, 8))["sequences"], usual), what
    rc = _raw_beam(eng, 4, em.prompt([0, 1, 5, 7]), K=3)       # four clips asked for, three encoded
    assert rc == TW_ESTATE, rc
    assert np.array_equal(eng.generate_greedy(p, **em.engine_kw(True, 8))["sequences"], usual)
    assert _raw_beam(eng, len(sel), p, K=4) == 0               # 12 rows: exactly max_batch
    assert np.array_equal(eng.generate_greedy(p, **em.engine_kw(True, 8))["sequences"], usual)


@pytest.mark.parametrize("dtype", ["fp8a16", "fp8a8"])     # TW_BF16_W8A16, TW_BF16_MXFP8
def test_fp8_contexts_are_refused(dtype):
    dims, w = em.model(2.5)
    eng = make_engine(dims, w, T=em.T, max_batch=8, dtype=dtype, heads=em.HEADS)
    try:
        _fill(eng, [0, 1])
        assert _raw_beam(eng, 2, em.prompt([0, 1]), K=2) == TW_EINVAL
        assert eng.generate_greedy(em.prompt([0, 1]), **em.engine_kw(True, 6))["sequences"].shape[0] == 2
    finally:
        eng.close()


# ---- 6. the HF seam and the pipeline on the device -------------------------------------------------------------------------
def test_dropin_generate_and_pipeline_with_beams_equal_hf_in_strict_f32():
    """`model.beam_search = True`: generate(num_beams=3) on the real engine returns the ids of HF's own generate on the CPU, with
    return_timestamps False and True; the pipeline call with generate_kwargs={"num_beams": 3} returns the text of those ids; with the
    flag off the old refusal stands."""
    from oracle import hf_reference as hr
    from oracle import whisper_oracle as wo
    from thewhisper_amd import ASRPipeline

    chunk_s = 10
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), chunk_s)
    pipe = ASRPipeline(hr.build_hf_model(dims, wo.make_weights(dims, 0)), feature_extractor=hr.build_feature_extractor(dims, chunk_s),
                       tokenizer=hr.build_tokenizer(dims), chunk_length_s=chunk_s, device="cuda", torch_dtype=torch.float32, batch_size=9)
    try:
        pcm = [wo.synth_audio(chunk_s * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
        feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        ids = lambda out: (out["sequences"] if isinstance(out, dict) else out).tolist()  # noqa: E731
        cpu = dict(input_features=feats.input_features.cpu(), attention_mask=feats.attention_mask.cpu())      # HF's model, on the CPU
        io = dict(input_features=feats.input_features.cuda(), attention_mask=feats.attention_mask.cuda())
        gk = {"num_beams": 3, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 12}
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            pipe.model.generate(**io, **gk)
        pipe.model.beam_search = True
        for ts in (False, True):
            ref = ids(hf.generate(**cpu, **gk, return_timestamps=ts))
            assert ref != ids(hf.generate(**cpu, **dict(gk, num_beams=1), return_timestamps=ts)), "the beams must change HF's ids"
            assert ids(pipe.model.generate(**io, **gk, return_timestamps=ts)) == ref, ts
            text = pipe(pcm[0], generate_kwargs=dict(gk), return_timestamps=ts)["text"]
            assert text == pipe.tokenizer.decode(ref[0], skip_special_tokens=True), (ts, text)
    finally:
        pipe.model.engine.close()
