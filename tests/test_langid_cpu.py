"""Language detection and per-row languages on the fast path, on the CPU stand-ins of tests/lang_engines.py (their ``detect_language``
is THE RULE of include/thewhisper.h in numpy over the stand-in's own ``decode_step`` logits): the numpy rule against torch, the learned
plan with a language slot against HF, passes that mix given and detected languages, the options that ride on a pass, the backend, the
hub and the gateway."""
import json

import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests.lang_engines import LangMixin, LangStubEngine, lang_engine_factory, lang_rule
from tests.test_gpu_langid import KINDS, _expect, _lists, _plant
from tests.test_pipeline_glue import build_amd_pipeline, normalise

torch.set_grad_enabled(False)
CHUNK_S = 10
GK = dict(language=None, task="transcribe", num_beams=1, do_sample=False, max_new_tokens=16, return_timestamps=True)


@pytest.fixture(scope="module")
def ref():
    """The HF reference model, the three clips of tests/test_language_detection.py and HF's answers: computed once, never changed."""
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    model = hr.patch_chunk_length(hr.build_hf_model(dims, w), CHUNK_S)
    fe = hr.build_feature_extractor(dims, CHUNK_S)
    audio = [wo.synth_audio(160000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    feats = fe(audio, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    x, am = feats["input_features"], feats["attention_mask"]
    want_lang = model.detect_language(input_features=x)
    assert len(set(want_lang.tolist())) > 1
    return dict(dims=dims, model=model, audio=audio, x=x, am=am, want_lang=want_lang, want=model.generate(input_features=x, attention_mask=am, **GK))


def _pipe(batch_size=3, factory=lang_engine_factory):
    return build_amd_pipeline("micro", CHUNK_S, batch_size, engine_factory=factory)


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [51866, 1003])
@pytest.mark.parametrize("kind", ["range", "scattered"])
def test_numpy_rule_equals_torch_on_the_planted_cases(V, kind):
    rng = np.random.default_rng(V + len(kind))
    for n_lang in (1, 2, 63, 64, 65, 99, 100, 128):
        ids = _lists(rng, V, n_lang, kind)
        for rows, shift in ((1, 3), (1, 4), (5, 0), (2 * KINDS, 0)):
            x = _plant(rng, rows, V, ids, shift)
            got = lang_rule(x, ids)
            want_id, want_p = _expect(x, ids)
            assert np.array_equal(got["ids"], want_id)
            assert np.abs(got["probs"] - want_p).max() <= 1e-5
            live = want_p.sum(axis=1) > 0
            assert (got["probs"][~live] == 0).all() and np.abs(got["probs"][live].sum(axis=1) - 1).max(initial=0) <= 1e-5


# ---- the drop-in: learn, then the plan ------------------------------------------------------------------------------------------
def test_generate_learns_a_plan_with_a_language_slot(ref):
    pipe = _pipe()
    model, eng = pipe.model, pipe.model.engine
    x, am = ref["x"], ref["am"]
    first = model.generate(input_features=x, attention_mask=am, **GK)          # learns through HF
    assert torch.equal(first, ref["want"])
    plan = model.last_plan
    gc = model.generation_config
    assert plan is not None and plan.lang_slot == 1 and plan.lang_ids == tuple(sorted(gc.lang_to_id.values()))
    before = dict(eng.calls)
    model.last_languages = None
    second = model.generate(input_features=x, attention_mask=am, **GK)         # takes the plan
    assert torch.equal(second, ref["want"])
    assert model.last_languages == ref["want_lang"].tolist()
    passes = eng.calls["generate"] - before["generate"]
    assert passes >= 1 and eng.calls["encode"] - before["encode"] == passes     # one encoder call per pass: none for the detection
    assert eng.calls["detect"] - before.get("detect", 0) == 1                   # HF detects once per generate call; so does the plan
    assert torch.equal(model.detect_language(input_features=x), ref["want_lang"])
    with pytest.raises(NotImplementedError, match="encoder_outputs"):
        model.detect_language(encoder_outputs=(torch.zeros(3, 500, ref["dims"].d_model),))
    # a list of languages stays on HF's route; a given language keeps its plan without a slot
    assert model._plan_key(dict(GK, input_features=x, attention_mask=am, language=["en", "de", "fr"])) is None
    model.generate(input_features=x, attention_mask=am, **dict(GK, language="en"))
    assert model.last_plan.lang_slot is None and model.last_plan.lang_ids == ()


def _plan_of(pipe, ref):
    pipe.model.generate(input_features=ref["x"], attention_mask=ref["am"], **GK)
    return pipe.model.last_plan


def _works(ref, rows, languages):
    from thewhisper_amd.shortform import ChunkWork

    out = []
    for r, lang in zip(rows, languages):
        w = ChunkWork(ref["x"][r], None)
        w.language = lang
        out.append(w)
    return out


def _run_to_end(eng, plan, works, **kw):
    from thewhisper_amd import shortform

    while any(not w.done for w in works):
        shortform.run_pass(eng, plan, [w for w in works if not w.done], **kw)
    return [torch.cat([s["tokens"] for s in w.segments]).tolist() if w.segments else [] for w in works]


def test_a_pass_mixes_given_and_detected_languages(ref):
    pipe = _pipe()
    eng, plan = pipe.model.engine, _plan_of(pipe, ref)
    want_lang = ref["want_lang"].tolist()
    other = [i for i in plan.lang_ids if i not in want_lang][:2]
    given = [None, other[0], None]                     # rows 0 and 2 are detected, row 1 carries a language of its own
    works = _works(ref, (0, 1, 2), given)
    got = _run_to_end(eng, plan, works)
    assert [w.language for w in works] == [want_lang[0], other[0], want_lang[2]]
    assert works[1].language_probs is None and works[0].language_probs.shape == (len(plan.lang_ids),)
    assert abs(float(works[0].language_probs.sum()) - 1.0) <= 1e-5
    for r in range(3):                                 # every row = that row decoded alone with its language given
        alone = _works(ref, (r,), [works[r].language])
        before = eng.calls.get("detect", 0)
        assert _run_to_end(eng, plan, alone) == [got[r]]
        assert eng.calls.get("detect", 0) == before    # nothing to detect


class _TwoIterationEngine(LangStubEngine):
    """Scripted: the first seek iteration of a chunk closes a segment at 2.00 s, the second runs to the end."""
    T, max_batch = 500, 4

    def __init__(self):
        super().__init__()
        self.detects, self.prompts = 0, []

    def encode(self, mel, slot0=0, **kw):
        return None

    def cross_kv(self, B, slot0=0):
        pass

    def detect_language(self, B, sot_id, lang_ids):
        self.detects += 1
        out = super().detect_language(B, sot_id, lang_ids)
        out["ids"][:] = list(lang_ids)[3]
        return out

    def generate_greedy(self, prompt, **kw):
        self.prompts.append(np.asarray(prompt).copy())
        ts, eos = 50365, 50257
        tail = [ts, 1000, ts + 100, ts + 100, eos] if len(self.prompts) == 1 else [ts, 1001, eos, eos, eos]
        return {"sequences": np.concatenate([np.asarray(prompt, np.int64), np.tile(np.asarray(tail, np.int64), (len(prompt), 1))], axis=1)}


def test_a_chunk_with_two_seek_iterations_detects_once():
    from thewhisper_amd.shortform import ChunkWork, ShortFormPlan, run_pass

    lang_ids = tuple(range(50259, 50359))
    plan = ShortFormPlan(init_tokens=(50258, 50259, 50360), greedy={}, eos=50257, pad=50257, timestamp_begin=50365, return_timestamps=True,
                         return_token_timestamps=False, return_segments=False, result_is_dict=False, lang_slot=1, lang_ids=lang_ids)
    eng = _TwoIterationEngine()
    w = ChunkWork(torch.zeros((128, 1000)), None)
    run_pass(eng, plan, [w])
    assert not w.done and w.seek == 200 and w.language == lang_ids[3]
    run_pass(eng, plan, [w])
    assert w.done and w.passes == 2 and eng.detects == 1
    assert [p[0].tolist() for p in eng.prompts] == [[50258, lang_ids[3], 50360]] * 2
    # ... and a plan without a slot never asks
    flat = ShortFormPlan(**{**{f: getattr(plan, f) for f in ("init_tokens", "greedy", "eos", "pad", "timestamp_begin", "return_timestamps",
                                                             "return_token_timestamps", "return_segments", "result_is_dict")}})
    eng2 = _TwoIterationEngine()
    run_pass(eng2, flat, [ChunkWork(torch.zeros((128, 1000)), None)])
    assert eng2.detects == 0 and eng2.prompts[0][0].tolist() == [50258, 50259, 50360]


# ---- the options that ride on a pass ------------------------------------------------------------------------------------------------
def _sampling_factory():
    from tests.test_sample_cpu import SamplingOracleEngine

    class LangSamplingEngine(LangMixin, SamplingOracleEngine):
        pass

    return lambda dims, T, max_batch, dtype, heads, dev: LangSamplingEngine(dims, T, max_batch, dtype, heads, dev)


def test_fallback_scores_and_drafts_run_with_a_language_slot(ref):
    from thewhisper_amd import fallback as fb

    pipe = _pipe(factory=_sampling_factory())
    eng, plan = pipe.model.engine, _plan_of(pipe, ref)
    want_lang = ref["want_lang"].tolist()
    plain = _run_to_end(eng, plan, _works(ref, (0, 1, 2), [None] * 3))
    # token scores: the scored sequences carry every row's own language token
    works = _works(ref, (0, 1, 2), [None] * 3)
    assert _run_to_end(eng, plan, works, score=True, no_speech_id=None) == plain
    assert all(len(w.scores) == w.passes and np.isfinite(w.scores[0]["avg_logprob"]) for w in works)
    # the temperature ladder starts from prompt[:, :n_prompt], languages included: nothing fails at thresholds this loose -> the plain ids
    policy = fb.FallbackPolicy(temperatures=(0.0, 0.4), compression_ratio_threshold=1e9, logprob_threshold=-1e9, seed=3)
    works = _works(ref, (0, 1, 2), [None] * 3)
    assert _run_to_end(eng, plan, works, fallback=policy) == plain
    assert [w.language for w in works] == want_lang and all(t == 0.0 for w in works for t in w.temperatures)
    # ... and every row is redone with ITS language when everything fails at T = 0
    strict = fb.FallbackPolicy(temperatures=(0.0, 0.4), compression_ratio_threshold=1e9, logprob_threshold=1e9, seed=3)
    works = _works(ref, (0, 1, 2), [None] * 3)
    eng.log.clear()
    _run_to_end(eng, plan, works, fallback=strict)
    assert any(c[0] == "sample" for c in eng.log) and all(w.attempts[0] == 2 for w in works)
    # a draft (first iteration only) is verified against the row's own language prompt: the plain ids whatever was offered
    works = _works(ref, (0, 1, 2), [None] * 3)
    for w, ids in zip(works, plain):
        w.draft = np.asarray((ids + [50257] * 4)[:4], np.int32)
    assert _run_to_end(eng, plan, works) == plain
    assert all(w.draft is None and w.draft_result is not None for w in works)


# ---- backend, hub, gateway ----------------------------------------------------------------------------------------------------------
def _backend(batch_size=4, **kw):
    from thewhisper_amd import AMDWhisperBackend

    return AMDWhisperBackend(None, chunk_length_s=CHUNK_S, language=None, asr_pipeline=_pipe(batch_size), **kw)


def test_auto_backend_fills_last_language_and_sticks(ref):
    from thewhisper_amd import AMDWhisperBackend

    b = _backend()
    assert b.auto_language and b._generate_kwargs()["language"] is None
    assert AMDWhisperBackend(None, chunk_length_s=CHUNK_S, language="auto", asr_pipeline=b.asr_pipeline).auto_language
    want_lang = ref["want_lang"].tolist()
    for r in (0, 2):
        words = b.transcribe(ref["audio"][r].copy(), 0.0, 16000)
        assert isinstance(words, list)
        (entry,) = b.last_language
        assert entry["id"] == want_lang[r] and entry["code"] == b.asr_pipeline.tokenizer.convert_ids_to_tokens(want_lang[r])[2:-2]
        assert 0.0 < entry["prob"] <= 1.0
        assert b.language_id(entry["code"]) == entry["id"]
    assert b._reuse_codec.plan.lang_slot == 1
    with pytest.raises(ValueError, match="unknown language"):
        b.language_id("xx")
    with pytest.raises(ValueError, match="unknown language"):
        b.transcribe(ref["audio"][0].copy(), 0.0, 16000, language="xx")
    # a request's own language: not detected, and the words are those of a backend built for that language
    code = b.language_entry(want_lang[2])["code"]
    fixed = AMDWhisperBackend(None, chunk_length_s=CHUNK_S, language=code, asr_pipeline=_pipe(4))
    assert normalise(b.transcribe(ref["audio"][0].copy(), 0.0, 16000, language=code)) == normalise(fixed.transcribe(ref["audio"][0].copy(), 0.0, 16000))
    assert b.last_language == [{"id": want_lang[2], "code": code, "prob": None}]
    with pytest.raises(ValueError, match="one language prompt"):
        fixed.transcribe(ref["audio"][0].copy(), 0.0, 16000, language="en" if code != "en" else "de")
    # sticky: the first chunk's language of the first call is stamped on every later chunk until reset()
    s = _backend(sticky_language=True)
    s.transcribe(ref["audio"][0].copy(), 0.0, 16000)
    assert s.last_language[0]["id"] == want_lang[0] and s._sticky_id == want_lang[0]
    s.transcribe(ref["audio"][2].copy(), 0.0, 16000)
    assert s.last_language == [{"id": want_lang[0], "code": s.language_entry(want_lang[0])["code"], "prob": None}]
    s.reset()
    s.transcribe(ref["audio"][2].copy(), 0.0, 16000)
    assert s.last_language[0]["id"] == want_lang[2] and s.last_language[0]["prob"] is not None


def test_hub_mixes_languages_in_one_pass(ref):
    from thewhisper_amd.serving import BatchingHub

    b = _backend()
    want_lang = ref["want_lang"].tolist()
    codes = [b.language_entry(i)["code"] for i in want_lang]
    alone = [b.transcribe(ref["audio"][r].copy(), 0.0, 16000, language=codes[2 - r]) for r in (0, 2)]
    hub = BatchingHub(b, max_batch=4, max_wait_s=1.0)
    try:
        futs = [hub.submit(ref["audio"][r].copy(), 0.0, 16000, language=codes[2 - r]) for r in (0, 2)]
        futs.append(hub.submit(ref["audio"][1].copy(), 0.0, 16000))                      # ... and one that is detected
        got = [f.result(300) for f in futs]
    finally:
        hub.close()
    assert normalise(got[:2]) == normalise(alone)
    assert [f.language_result[0]["id"] for f in futs] == [want_lang[2], want_lang[0], want_lang[1]]
    assert futs[2].language_result[0]["prob"] is not None and futs[0].language_result[0]["prob"] is None
    assert max(hub.batches) > 1                                                          # different languages shared a pass
    sb = hub.stream_backend(language=codes[0])
    assert sb.language == codes[0]


def test_gateway_honours_the_request_language():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from tests.test_gateway import wav_bytes
    from thewhisper_amd import AMDWhisperBackend
    from thewhisper_amd.gateway import build_host, create_app, decode_wav, words_to_response
    from thewhisper_amd.serving import BatchingHub

    b = _backend()
    audio = wo.synth_audio(16000 * 7, 5, "speechlike")
    q, _ = decode_wav(wav_bytes(audio))
    files = {"file": ("chunk.wav", wav_bytes(audio), "audio/wav")}
    hub = BatchingHub(b, max_batch=4, max_wait_s=0.05)
    try:
        client = TestClient(create_app(hub, model_name="micro", lang_id=None))
        r = client.post("/transcribe", files=files)                                    # no header: detected
        assert r.status_code == 200, r.text
        detected = r.json()["language"]
        want = b.transcribe(q.copy(), 0.0, 16000)
        assert b.last_language[0]["code"] == detected
        assert r.json()["metadata"] == normalise(words_to_response(want, "micro"))["metadata"]
        other = "de" if detected != "de" else "fr"
        r2 = client.post("/transcribe", files=files, headers={"X-Lang-Id": other})     # the header is honoured per request
        assert r2.status_code == 200 and r2.json()["language"] == other
        want2 = b.transcribe(q.copy(), 0.0, 16000, language=other)
        assert r2.json()["metadata"] == normalise(words_to_response(want2, "micro"))["metadata"]
        assert client.post("/transcribe", files=files, headers={"X-Lang-Id": "xx"}).status_code == 400
    finally:
        hub.close()
    # a gateway started with a fixed language: the answer it has always given, byte for byte, and its 400 for another language
    fixed = AMDWhisperBackend(None, chunk_length_s=CHUNK_S, language="en", asr_pipeline=_pipe(4))
    hub = BatchingHub(fixed, max_batch=4, max_wait_s=0.05)
    try:
        client = TestClient(create_app(hub, model_name="micro", lang_id="en"))
        r = client.post("/transcribe", files=files, headers={"X-Lang-Id": "en"})
        assert r.status_code == 200
        want = words_to_response(fixed.transcribe(q.copy(), 0.0, 16000), "micro")
        assert r.content == json.dumps(want, ensure_ascii=False, allow_nan=False, indent=None, separators=(",", ":")).encode("utf-8")
        assert "language" not in r.json()
        assert client.post("/transcribe", files=files, headers={"X-Lang-Id": "de"}).status_code == 400
    finally:
        hub.close()
    assert build_host is not None
