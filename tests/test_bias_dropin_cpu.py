"""`generate(sequence_bias=...)` through the drop-in, on the CPU: the seeded micro model behind the numpy stand-in engine that knows the
bias (tests/bias_judge.BiasedOracleEngine) returns the ids of the HF model with the same weights - on the slow path (HF's control flow,
the mixin reads generation_config.sequence_bias) and on the fast path (the learned short-form plan carries the bias) - and those ids
differ from the unbiased ones.  On the stand-in that does NOT know the bias the same call does not return HF's ids, which is what the
drop-in silently did before it read the option.  Also: where the mixin finds the bias, the refusal of a misplaced processor, the
per-chunk lists of a pass, and the backend's option checks."""
import dataclasses

import numpy as np
import pytest
import torch
from transformers.generation.logits_process import (SequenceBiasLogitsProcessor, SuppressTokensLogitsProcessor,
                                                    WhisperTimeStampLogitsProcessor)

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests import bias_judge as bj
from tests.oracle_engine import oracle_engine_factory
from tests.stub_engine import StubEngine

torch.set_grad_enabled(False)
CHUNK_S = 10
SB = [[[1705, 7], 50.0], [[9], -50.0]]
GK = {"num_beams": 1, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 16, "return_timestamps": True}


def build(engine_factory, batch_size=3):
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    model = hr.build_hf_model(dims, wo.make_weights(dims, 0))
    return ASRPipeline(model, feature_extractor=hr.build_feature_extractor(dims, CHUNK_S), tokenizer=hr.build_tokenizer(dims),
                       chunk_length_s=CHUNK_S, device="cpu", torch_dtype=torch.float32, batch_size=batch_size, engine_factory=engine_factory)


def features(pipe):
    pcm = [wo.synth_audio(CHUNK_S * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    return pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)


def ids_of(out):
    return (out["sequences"] if isinstance(out, dict) else out).tolist()


def test_generate_with_sequence_bias_returns_hfs_ids_on_both_paths():
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), CHUNK_S)
    pipe = build(bj.biased_oracle_engine_factory)
    model = pipe.model
    feats = features(pipe)
    io = dict(input_features=feats.input_features, attention_mask=feats.attention_mask)
    ref = ids_of(hf.generate(**io, **GK, sequence_bias=SB))
    ref_plain = ids_of(hf.generate(**io, **GK))
    assert ref != ref_plain and ref[0] != ref_plain[0], "the bias must change HF's ids (clip 0 at least)"
    assert ids_of(model.generate(**io, **GK)) == ref_plain
    n_plans = len(model._plans)
    slow = ids_of(model.generate(**io, **GK, sequence_bias=SB))          # first call of its kind: HF's flow, the plan is learned
    assert len(model._plans) == n_plans + 1 and model.last_plan is not None
    assert model.last_plan.greedy["sequence_bias"] == {(1705, 7): 50.0, (9,): -50.0}
    calls = model.engine.calls["generate"]
    fast = ids_of(model.generate(**io, **GK, sequence_bias=SB))          # the restated short-form loop
    assert model.engine.calls["generate"] > calls
    assert slow == ref and fast == ref
    assert ids_of(model.generate(**io, **GK)) == ref_plain               # the unbiased plan is another plan
    # another list is another plan, not the first list's ids
    other = [[[1705, 7], 50.0]]
    assert ids_of(model.generate(**io, **GK, sequence_bias=other)) == ids_of(hf.generate(**io, **GK, sequence_bias=other))
    # the stand-in that does not know the bias cannot return HF's ids: it refuses the keyword (before this option was read, it was
    # handed nothing and returned the unbiased ids)
    blind = build(oracle_engine_factory).model
    with pytest.raises(TypeError, match="sequence_bias"):
        blind.generate(**io, **GK, sequence_bias=SB)


class _Recorder(StubEngine):
    """tests/stub_engine.StubEngine, keeping what generate_greedy was asked."""

    def __init__(self):
        super().__init__()
        self.kw = []

    def generate_greedy(self, prompt, max_new_tokens=128, **kw):
        self.kw.append(dict(kw))
        return super().generate_greedy(prompt, max_new_tokens=max_new_tokens, **kw)


def _mixin_model():
    from thewhisper_amd.model import AMDWhisperForConditionalGeneration

    dims = wo.PRESETS["micro"]
    m = AMDWhisperForConditionalGeneration.from_hf(hr.build_hf_model(dims, wo.make_weights(dims, 0)))
    m._engine = _Recorder()
    return m


def _inner_generate(m, gc=None, processors=None):
    from thewhisper_amd.model import _EngineGreedyMixin

    return _EngineGreedyMixin.generate(m, torch.zeros(2, 128, 1000), generation_config=gc, logits_processor=processors,
                                       decoder_input_ids=torch.tensor([[50258, 50259, 50360]] * 2))


def test_the_mixin_reads_the_bias_from_the_generation_config_and_from_a_processor():
    import copy

    m = _mixin_model()
    gc = copy.deepcopy(m.generation_config)
    gc.max_new_tokens = 4
    _inner_generate(m, gc)
    assert "sequence_bias" not in m._engine.kw[-1]
    gc.sequence_bias = SB
    _inner_generate(m, gc)
    assert m._engine.kw[-1]["sequence_bias"] == {(1705, 7): 50.0, (9,): -50.0}
    gc.sequence_bias = None
    ts = WhisperTimeStampLogitsProcessor(gc, begin_index=3)
    sup = SuppressTokensLogitsProcessor([5, 6])
    _inner_generate(m, gc, [sup, SequenceBiasLogitsProcessor(SB), ts])
    assert m._engine.kw[-1]["sequence_bias"] == {(1705, 7): 50.0, (9,): -50.0} and m._engine.kw[-1]["timestamps"] is True
    assert m._engine.kw[-1]["suppress"] == (5, 6)
    n = len(m._engine.kw)
    with pytest.raises(NotImplementedError, match="behind the WhisperTimeStampLogitsProcessor"):
        _inner_generate(m, gc, [sup, ts, SequenceBiasLogitsProcessor(SB)])
    gc.sequence_bias = SB
    with pytest.raises(NotImplementedError, match="more than one sequence bias"):
        _inner_generate(m, gc, [SequenceBiasLogitsProcessor(SB), ts])
    assert len(m._engine.kw) == n, "a refused call reaches no engine"


def test_a_pass_hands_the_engine_one_list_per_chunk_plan_level_first():
    from thewhisper_amd import shortform

    class Eng(_Recorder):
        def generate_greedy(self, prompt, **kw):
            self.kw.append(dict(kw))
            raise StopIteration          # the call itself is what is looked at

    plan = shortform.ShortFormPlan(init_tokens=(1, 2, 3), greedy={"eos_id": 9, "pad_id": 9, "sequence_bias": {(4,): 1.0, (5, 6): 2.0}}, eos=9,
                                   pad=9, timestamp_begin=100, return_timestamps=False, return_token_timestamps=False, return_segments=False,
                                   result_is_dict=False)
    for biases, expect in (([None, None], None),
                           ([{(5, 6): 7.0, (8,): 3.0}, None], [{(4,): 1.0, (5, 6): 7.0, (8,): 3.0}, {(4,): 1.0, (5, 6): 2.0}])):
        eng = Eng()
        p = shortform.Pass.__new__(shortform.Pass)
        p.engine, p.plan, p.fallback, p.score = eng, plan, None, False
        p.works, p.snf = [], []
        for b in biases:
            w = shortform.ChunkWork(torch.zeros(4, 20), None)
            w.bias = b
            p.works.append(w)
        with pytest.raises(StopIteration):
            p.run()
        kw = eng.kw[-1]
        if expect is None:       # no bias in any chunk: exactly the plan's own keywords
            assert kw == plan.greedy
        else:
            assert "sequence_bias" not in kw and kw["sequence_bias_rows"] == expect
            assert [list(r) for r in kw["sequence_bias_rows"]] == [list(e) for e in expect]      # order: the plan-level list first
    assert plan.greedy["sequence_bias"] == {(4,): 1.0, (5, 6): 2.0}
    # token scores are those of the unbiased distribution: a scoring pass refuses a bias, from the plan or from a chunk
    for plan_bias, chunk_bias in (({(4,): 1.0}, None), (None, {(4,): 1.0})):
        eng = Eng()
        p = shortform.Pass.__new__(shortform.Pass)
        greedy = {"eos_id": 9, "pad_id": 9, **({"sequence_bias": plan_bias} if plan_bias else {})}
        p.engine, p.plan, p.fallback, p.score = eng, dataclasses.replace(plan, greedy=greedy), None, True
        w = shortform.ChunkWork(torch.zeros(4, 20), None)
        w.bias = chunk_bias
        p.works, p.snf = [w], []
        with pytest.raises(ValueError, match="token scores"):
            p.run()
        assert not eng.kw


def test_backend_hotword_options_are_checked():
    from thewhisper_amd import AMDWhisperBackend

    pipe = build(bj.biased_oracle_engine_factory, batch_size=1)
    mk = lambda **kw: AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe, **kw)  # noqa: E731
    plain = mk()
    kw0 = plain._generate_kwargs()
    with pytest.raises(ValueError, match="hotword_boost"):
        mk(hotwords=["w5 w17"])
    with pytest.raises(ValueError, match="without hotwords"):
        mk(hotword_boost=2.0)
    for bad in (dict(temperature_fallback=(0.0, 0.4)), dict(token_scores=True), dict(reuse_committed_prefix=True)):
        with pytest.raises(ValueError, match="do not go together"):
            mk(hotwords=["w5 w17"], hotword_boost=2.0, **bad)
    be = mk(hotwords=["w5 w17"], hotword_boost=2.0)
    assert be.draft_previous_tick and be._generate_kwargs() == kw0
    tok = pipe.tokenizer
    assert be._hotword_bias[tuple(tok.encode(" w5 w17", add_special_tokens=False))] == 2.0
    # the list travels on the works JobCodec.open makes, so a scheduler that opens the jobs itself (serving.BatchingHub) decodes with it
    job = be.job_codec().open(wo.synth_audio(2 * 16000, 3, "speechlike"), 0.0, 16000)
    assert job.works and all(w.bias == be._hotword_bias for w in job.works)
    be.set_hotwords(None, None)
    assert be._hotword_bias is None and be.hotwords == []
    assert all(w.bias is None for w in be.job_codec().open(wo.synth_audio(2 * 16000, 3, "speechlike"), 0.0, 16000).works)
    # two growing ticks of one buffer: the words of a backend without drafts, and the hotwords reach the engine per chunk
    audio = wo.synth_audio(6 * 16000, 3, "speechlike")
    seen = []
    eng = pipe.model.engine
    inner = eng.generate_greedy

    def recording(prompt, **kw):
        seen.append(kw.get("sequence_bias_rows"))
        return inner(prompt, **kw)

    eng.generate_greedy = recording
    try:
        words = {}
        for draft in (True, False):
            b = mk(hotwords=["w5 w17", "w9"], hotword_boost=30.0, draft_previous_tick=draft)
            b.transcribe(audio[:16000], 0.0, 16000)
            b.reset()
            seen.clear()
            words[draft] = [b.transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
            assert seen and all(r is not None and len(r) == 1 and r[0] == b._hotword_bias for r in seen)
        assert words[True] == words[False]
        seen.clear()
        unbiased = [plain.transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
        assert all(r is None for r in seen)
        assert unbiased != words[False], "a boost of 30 on the filler words must change the transcript"
    finally:
        eng.generate_greedy = inner
