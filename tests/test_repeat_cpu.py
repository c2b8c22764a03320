"""`generate(repetition_penalty=..., no_repeat_ngram_size=...)` through the drop-in, on the CPU: the seeded micro model behind the numpy
stand-in engine that knows the rule (tests/repeat_judge.RepeatOracleEngine) returns the ids of the HF model with the same weights, on
the slow path (HF's control flow; the mixin reads the generation config) and on the fast path (the learned short-form plan carries the
keywords), and those ids differ from the plain call's.  Also: the processor-list forms and every refusal of the mixin, the engine's
keyword checks, the C ABI (struct size, exported symbols, NULL arguments refused without a device) and the backend's keyword checks."""
import copy
import ctypes

import numpy as np
import pytest
import torch
from transformers.generation.logits_process import (NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor,
                                                    SequenceBiasLogitsProcessor, SuppressTokensLogitsProcessor,
                                                    WhisperTimeStampLogitsProcessor)

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests import repeat_judge as rj
from tests.test_bias_dropin_cpu import CHUNK_S, SB, _inner_generate, _mixin_model, build, features, ids_of

torch.set_grad_enabled(False)
# 48 new tokens: long enough for a bigram of the plain run to come round again, so that no_repeat_ngram_size=2 alone changes the ids
GK = {"num_beams": 1, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 48, "return_timestamps": True}
OPTIONS = {
    "penalty": dict(repetition_penalty=1.3),
    "ngram": dict(no_repeat_ngram_size=2),
    "both": dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
    "both, with a sequence bias": dict(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias=SB),
}


def test_generate_with_the_repeat_options_returns_hfs_ids_on_both_paths():
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), CHUNK_S)
    pipe = build(rj.repeat_oracle_engine_factory)
    model = pipe.model
    feats = features(pipe)
    io = dict(input_features=feats.input_features, attention_mask=feats.attention_mask)
    ref_plain = ids_of(hf.generate(**io, **GK))
    assert ids_of(model.generate(**io, **GK)) == ref_plain
    refs = {}
    for what, kw in OPTIONS.items():
        ref = refs[what] = ids_of(hf.generate(**io, **GK, **kw))
        assert ref != ref_plain and ref[0] != ref_plain[0], f"{what}: the option must change HF's ids (clip 0 at least)"
        n_plans = len(model._plans)
        slow = ids_of(model.generate(**io, **GK, **kw))          # first call of its kind: HF's flow, the plan is learned
        assert len(model._plans) == n_plans + 1 and model.last_plan is not None, what
        for k in ("repetition_penalty", "no_repeat_ngram_size"):
            assert model.last_plan.greedy.get(k) == kw.get(k), (what, k)
        calls = model.engine.calls["generate"]
        fast = ids_of(model.generate(**io, **GK, **kw))          # the restated short-form loop replays the keywords
        assert model.engine.calls["generate"] > calls
        assert slow == ref and fast == ref, what
    assert len({str(r) for r in refs.values()}) >= 3, "the options differ from one another"
    assert ids_of(model.generate(**io, **GK)) == ref_plain


def test_the_mixin_reads_the_options_from_the_generation_config_and_from_processors():
    m = _mixin_model()
    gc = copy.deepcopy(m.generation_config)
    gc.max_new_tokens = 4
    _inner_generate(m, gc)
    assert not {"repetition_penalty", "no_repeat_ngram_size", "penalty_ignore"} & set(m._engine.kw[-1])
    gc.repetition_penalty, gc.no_repeat_ngram_size = 1.0, 0          # HF's "off" values: the plain call
    _inner_generate(m, gc)
    assert not {"repetition_penalty", "no_repeat_ngram_size"} & set(m._engine.kw[-1])
    gc.repetition_penalty, gc.no_repeat_ngram_size = 1.3, 2
    _inner_generate(m, gc)
    assert m._engine.kw[-1]["repetition_penalty"] == 1.3 and m._engine.kw[-1]["no_repeat_ngram_size"] == 2
    assert "penalty_ignore" not in m._engine.kw[-1]
    gc.repetition_penalty, gc.no_repeat_ngram_size = None, None
    ts = WhisperTimeStampLogitsProcessor(gc, begin_index=3)
    sup = SuppressTokensLogitsProcessor([5, 6])
    pen, ngr = RepetitionPenaltyLogitsProcessor(1.7, prompt_ignore_length=2), NoRepeatNGramLogitsProcessor(3)
    _inner_generate(m, gc, [SequenceBiasLogitsProcessor(SB), pen, ngr, sup, ts])
    kw = m._engine.kw[-1]
    assert (kw["repetition_penalty"], kw["penalty_ignore"], kw["no_repeat_ngram_size"]) == (1.7, 2, 3)
    assert kw["sequence_bias"] == {(1705, 7): 50.0, (9,): -50.0} and kw["timestamps"] is True and kw["suppress"] == (5, 6)
    _inner_generate(m, gc, [ngr, ts])
    assert m._engine.kw[-1]["no_repeat_ngram_size"] == 3 and "repetition_penalty" not in m._engine.kw[-1]
    n = len(m._engine.kw)
    for procs in ([sup, ts, pen], [ts, ngr]):
        with pytest.raises(NotImplementedError, match="behind the WhisperTimeStampLogitsProcessor"):
            _inner_generate(m, gc, procs)
    for procs in ([pen, SequenceBiasLogitsProcessor(SB), ts], [ngr, SequenceBiasLogitsProcessor(SB)]):
        with pytest.raises(NotImplementedError, match="ahead of a SequenceBiasLogitsProcessor"):
            _inner_generate(m, gc, procs)
    with pytest.raises(NotImplementedError, match="given twice"):
        _inner_generate(m, gc, [pen, RepetitionPenaltyLogitsProcessor(1.2), ts])
    gc.no_repeat_ngram_size = 2
    with pytest.raises(NotImplementedError, match="given twice"):
        _inner_generate(m, gc, [ngr, ts])
    gc.no_repeat_ngram_size = None
    gc.repetition_penalty = 1.3
    with pytest.raises(NotImplementedError, match="given twice"):
        _inner_generate(m, gc, [pen, ts])
    # token scores and padded prompts do not go with the options, as with a sequence bias
    m.score_sink = {"entries": [], "no_speech_id": None}
    with pytest.raises(ValueError, match="token scores"):
        _inner_generate(m, gc)
    m.score_sink = None
    m.ragged_decoder_prompts = True
    from thewhisper_amd.model import _EngineGreedyMixin

    with pytest.raises(ValueError, match="padded decoder_attention_mask"):
        _EngineGreedyMixin.generate(m, torch.zeros(2, 128, 1000), generation_config=gc, decoder_input_ids=torch.tensor([[50258, 50259, 50360]] * 2),
                                    decoder_attention_mask=torch.tensor([[0, 1, 1], [1, 1, 1]]))
    assert len(m._engine.kw) == n, "a refused call reaches no engine"


def test_engine_keyword_forms_and_refusals():
    from thewhisper_amd.engine import repeat_rows

    assert repeat_rows(None, None, 3) is None and repeat_rows(1.0, 0, 3) is None and repeat_rows([1.0] * 3, [0] * 3, 3) is None
    pen, ngr = repeat_rows(1.3, None, 3)
    assert pen.dtype == np.float32 and ngr.dtype == np.int32 and pen.tolist() == [np.float32(1.3)] * 3 and ngr.tolist() == [0, 0, 0]
    pen, ngr = repeat_rows([1.0, 2.0], 2, 2)
    assert pen.tolist() == [1.0, 2.0] and ngr.tolist() == [2, 2] and pen.flags.c_contiguous and ngr.flags.c_contiguous
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty=float("inf")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5),
                dict(repetition_penalty=[1.0, 2.0]), dict(no_repeat_ngram_size=[1, 2])):
        with pytest.raises(ValueError):
            repeat_rows(bad.get("repetition_penalty"), bad.get("no_repeat_ngram_size"), 3)
    # with n_pad, and a negative penalty_ignore: ValueError before the library is reached
    from thewhisper_amd.engine import WhisperEngine

    class _Lib:
        def __getattr__(self, name):
            raise AssertionError(f"{name}: a refused call reaches the library")

    eng = WhisperEngine.__new__(WhisperEngine)
    eng.lib, eng.ctx = _Lib(), None
    prompt = np.array([[1, 2, 3], [1, 2, 3]], np.int32)
    with pytest.raises(ValueError, match="n_pad"):
        eng.generate_greedy(prompt, n_pad=[1, 0], repetition_penalty=1.3)
    with pytest.raises(ValueError, match="n_pad"):
        eng.generate_greedy(prompt, n_pad=[1, 0], no_repeat_ngram_size=[0, 2])
    with pytest.raises(ValueError, match="penalty_ignore"):
        eng.generate_greedy(prompt, repetition_penalty=1.3, penalty_ignore=-1)


def test_cabi_struct_symbols_and_null_arguments(built_library):
    from thewhisper_amd import _cabi

    # tw_repeat_opts: two pointers and an int32, padded to the pointer's alignment
    assert ctypes.sizeof(_cabi.tw_repeat_opts) == 8 + 8 + 8
    assert ctypes.sizeof(_cabi.tw_greedy_opts) == 80, "the new options live in a struct of their own"
    lib = _cabi.load_library()
    names = {n for n, _, _ in _cabi.SYMBOLS}
    assert {"tw_generate_greedy_repeat", "tw_repeat_logits"} <= names
    raw = ctypes.CDLL(built_library)
    assert hasattr(raw, "tw_generate_greedy_repeat") and hasattr(raw, "tw_repeat_logits")
    TW_EINVAL = -1
    ro = _cabi.tw_repeat_opts()
    o = _cabi.tw_greedy_opts()
    ids, n = (ctypes.c_int32 * 4)(), ctypes.c_int32(0)
    assert lib.tw_generate_greedy_repeat(None, 1, ids, 1, ctypes.byref(o), None, ctypes.byref(ro), ids, ctypes.byref(n), None) == TW_EINVAL
    assert b"null argument" in lib.tw_last_error(None)
    # tw_repeat_logits checks everything on the host before it touches a device
    hist, nh = (ctypes.c_int32 * 8)(*range(8)), (ctypes.c_int32 * 2)(4, 4)
    fake = ctypes.c_void_p(4096)       # never dereferenced: every call below is refused
    assert lib.tw_repeat_logits(0, None, 100, 2, hist, 4, nh, ctypes.byref(ro), None) == TW_EINVAL
    assert lib.tw_repeat_logits(0, fake, 100, 2, None, 4, nh, ctypes.byref(ro), None) == TW_EINVAL
    assert lib.tw_repeat_logits(0, fake, 100, 2, hist, 4, None, ctypes.byref(ro), None) == TW_EINVAL
    assert lib.tw_repeat_logits(0, fake, 100, 2, hist, 4, nh, None, None) == TW_EINVAL
    assert lib.tw_repeat_logits(0, fake, 100, 0, hist, 4, nh, ctypes.byref(ro), None) == TW_EINVAL          # rows outside 1 .. 64
    assert lib.tw_repeat_logits(0, fake, 100, 65, hist, 4, nh, ctypes.byref(ro), None) == TW_EINVAL
    assert lib.tw_repeat_logits(0, fake, 4, 2, hist, 4, nh, ctypes.byref(ro), None) == TW_EINVAL            # a history id outside [0, V)
    bad_n = (ctypes.c_int32 * 2)(4, 5)
    assert lib.tw_repeat_logits(0, fake, 100, 2, hist, 4, bad_n, ctypes.byref(ro), None) == TW_EINVAL       # n_hist outside [0, ld]
    bad_n = (ctypes.c_int32 * 2)(-1, 4)
    assert lib.tw_repeat_logits(0, fake, 100, 2, hist, 4, bad_n, ctypes.byref(ro), None) == TW_EINVAL
    for pen, ngr, ign in (((0.0, 1.0), None, 0), ((float("nan"), 1.0), None, 0), ((float("inf"), 1.0), None, 0), ((-2.0, 1.0), None, 0),
                          (None, (-1, 0), 0), (None, (0, 513), 0), (None, None, -1)):
        r = _cabi.tw_repeat_opts()
        keep = (ctypes.c_float * 2)(*pen) if pen else None, (ctypes.c_int32 * 2)(*ngr) if ngr else None
        if pen:
            r.penalty = keep[0]
        if ngr:
            r.no_repeat_ngram = keep[1]
        r.penalty_ignore = ign
        assert lib.tw_repeat_logits(0, fake, 100, 2, hist, 4, nh, ctypes.byref(r), None) == TW_EINVAL, (pen, ngr, ign)
        assert lib.tw_last_error(None)


def test_backend_keyword_checks():
    from thewhisper_amd import AMDWhisperBackend

    pipe = build(rj.repeat_oracle_engine_factory, batch_size=1)
    mk = lambda **kw: AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe, **kw)  # noqa: E731
    kw0 = mk()._generate_kwargs()
    assert "repetition_penalty" not in kw0 and "no_repeat_ngram_size" not in kw0, "off by default"
    assert mk(repetition_penalty=1.0, no_repeat_ngram_size=0)._generate_kwargs() == kw0
    be = mk(repetition_penalty=1.3, no_repeat_ngram_size=2)
    assert be.draft_previous_tick, "drafts stay on: the result is exact"
    assert be._generate_kwargs() == {**kw0, "repetition_penalty": 1.3, "no_repeat_ngram_size": 2}
    assert mk(repetition_penalty=1.3, hotwords=["w5 w17"], hotword_boost=2.0)._hotword_bias
    for bad in (dict(temperature_fallback=(0.0, 0.4)), dict(token_scores=True)):
        for opt in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2)):
            with pytest.raises(ValueError, match="do not go together"):
                mk(**opt, **bad)
    for opt in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(repetition_penalty=float("inf")),
                dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=1.5)):
        with pytest.raises(ValueError):
            mk(**opt)
    # two growing ticks of one buffer: the keywords reach the engine, and drafts do not change the words
    audio = wo.synth_audio(6 * 16000, 3, "speechlike")
    seen = []
    eng = pipe.model.engine
    inner = eng.generate_greedy

    def recording(prompt, **kw):
        seen.append((kw.get("repetition_penalty"), kw.get("no_repeat_ngram_size"), kw.get("n_draft", 0)))
        return inner(prompt, **kw)

    eng.generate_greedy = recording
    try:
        words = {}
        for draft in (True, False):
            b = mk(repetition_penalty=1.3, no_repeat_ngram_size=2, draft_previous_tick=draft)
            b.transcribe(audio[:16000], 0.0, 16000)
            b.reset()
            seen.clear()
            words[draft] = [b.transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
            assert seen and all(s[:2] == (1.3, 2) for s in seen)
            assert any(s[2] > 0 for s in seen) == draft
        assert words[True] == words[False]
        seen.clear()
        plain = [mk(draft_previous_tick=False).transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
        assert all(s[:2] == (None, None) for s in seen)
        assert plain != words[False], "the options must change the transcript"
    finally:
        eng.generate_greedy = inner
