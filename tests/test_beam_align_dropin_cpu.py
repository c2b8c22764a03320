"""`generate(num_beams=K, return_token_timestamps=True)` through the drop-in, on the CPU: with `model.beam_search` and
`model.beam_token_timestamps` on, the seeded micro model behind a numpy stand-in engine - beam search by tests/beam_judge.py, token
timestamps by the rule of tests/beam_align_judge.py (every hypothesis teacher-forced on its own) - returns HF's ids and HF's
`token_timestamps` for each clip decoded alone; the pipeline returns HF's words; `AMDWhisperBackend(num_beams=K)` switches it all on and
refuses by name what does not go with beams.  Fails without the feature (the seam raises NotImplementedError)."""
import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests import beam_align_judge as baj
from tests import beam_judge as bj
from tests.oracle_engine import OracleEngine

torch.set_grad_enabled(False)
CHUNK_S = 10
GK = {"do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 12, "num_beams": 3}
TS = {"return_timestamps": True, "return_token_timestamps": True}
TOL_S = 1e-6


class BeamAlignOracleEngine(OracleEngine):
    """The stand-in engine with `WhisperEngine.generate_beam(want_alignment=...)` and `token_timestamps_each`, by the judges."""

    def generate_beam(self, prompt, num_beams, length_penalty=1.0, early_stopping=False, *, max_new_tokens=128, min_new_tokens=0,
                      max_length=448, eos_id=50257, pad_id=50257, timestamps=False, no_timestamps_id=50364, max_initial_timestamp_index=50,
                      begin_suppress=(220, 50257), suppress=(), want_alignment=False):
        self.calls["generate"] += 1
        self.calls["beam"] = self.calls.get("beam", 0) + 1
        self.calls["beam_aligned"] = self.calls.get("beam_aligned", 0) + int(bool(want_alignment))
        opt = wo.GreedyOptions(eos=eos_id, pad=pad_id, max_new_tokens=max_new_tokens, min_new_tokens=min_new_tokens, max_length=max_length,
                               begin_suppress=tuple(begin_suppress), suppress=tuple(suppress), timestamps=timestamps,
                               no_timestamps_id=no_timestamps_id, max_initial_timestamp_index=max_initial_timestamp_index)
        prompt = np.asarray(prompt)
        assert prompt.shape[0] * num_beams <= self.max_batch
        runs = [bj.run_clip(self.model, self._enc[b : b + 1], prompt[b], opt, num_beams, length_penalty, early_stopping)
                for b in range(prompt.shape[0])]
        best = bj.pad_nbest([r["nbest"][0] for r in runs], pad_id)
        L = max(len(h) for r in runs for h in r["nbest"])
        nbest = np.stack([bj.pad_nbest([list(h) + [pad_id] * (L - len(h)) for h in r["nbest"]], pad_id) for r in runs])
        lens = np.asarray([[len(h) for h in r["nbest"]] for r in runs], dtype=np.int32)
        self._beam_best = [list(r["nbest"][0]) for r in runs] if want_alignment else None    # (no rows without want_alignment)
        return {"sequences": best, "scores": np.asarray([r["scores"][0] for r in runs], np.float32), "nbest_sequences": nbest,
                "nbest_scores": np.stack([r["scores"] for r in runs]), "length": int(best.shape[1]), "lengths": lens[:, 0].copy(),
                "nbest_lengths": lens}

    def token_timestamps_each(self, seq_lens, n_prompt, num_frames=None, time_precision=0.02, ld=None):
        self.calls["dtw"] += 1
        assert self._beam_best is not None, "token_timestamps_each without an aligned beam call before it"
        lens = [int(x) for x in seq_lens]
        ld = max(lens) if ld is None else int(ld)
        out = np.zeros((len(lens), ld), dtype=np.float32)
        for b, (h, n) in enumerate(zip(self._beam_best, lens)):
            assert len(h) == n, (b, len(h), n)
            if n - 1 - n_prompt <= 0:
                continue
            _, cross = self.model.decode(np.asarray(h, dtype=np.int64)[None, :-1], self.model.new_cache(self._enc[b : b + 1]),
                                         want_cross=self.alignment_heads)
            cols = None
            if num_frames is not None:   # the C ABI's rule: ONE Python-slice crop `[: n // 2]` per row
                T, k = cross.shape[-1], int(num_frames[b]) // 2
                cols = [min(T, k) if k >= 0 else max(0, T + k)]
            out[b] = baj.padded(wo.token_timestamps(cross, n_prompt, None, time_precision, columns=cols)[0], ld)
        return out


def factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return BeamAlignOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


def build(batch_size=9):
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    model = hr.build_hf_model(dims, wo.make_weights(dims, 0))
    return ASRPipeline(model, feature_extractor=hr.build_feature_extractor(dims, CHUNK_S), tokenizer=hr.build_tokenizer(dims),
                       chunk_length_s=CHUNK_S, device="cpu", torch_dtype=torch.float32, batch_size=batch_size, engine_factory=factory)


@pytest.fixture(scope="module")
def setup():
    from transformers import AutomaticSpeechRecognitionPipeline

    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), CHUNK_S)
    pipe = build()
    pcm = [wo.synth_audio(CHUNK_S * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    hf_pipe = AutomaticSpeechRecognitionPipeline(model=hf, feature_extractor=hr.build_feature_extractor(dims, CHUNK_S),
                                                 tokenizer=hr.build_tokenizer(dims), chunk_length_s=CHUNK_S, device="cpu")
    # HF's result for each clip decoded ALONE: the reference of the rule
    alone = []
    for i in range(3):
        ref = hf.generate(input_features=feats.input_features[i : i + 1], attention_mask=feats.attention_mask[i : i + 1], **GK, **TS)
        alone.append((ref["sequences"][0].tolist(), ref["token_timestamps"][0].numpy()))
    return hf, hf_pipe, pipe, pcm, dict(input_features=feats.input_features, attention_mask=feats.attention_mask), alone


@pytest.fixture()
def flags(setup):
    model = setup[2].model
    model.beam_search = model.beam_token_timestamps = True
    yield model
    model.beam_search = model.beam_token_timestamps = False


def _check_row(out, i, alone, pad):
    ids, ts = alone
    seq, got = out["sequences"][i].tolist(), out["token_timestamps"][i].numpy()
    L = len(ids)
    assert seq[:L] == ids and all(t == pad for t in seq[L:]), (i, seq, ids)
    assert np.abs(got[:L] - ts).max() <= TOL_S, (i, got.tolist(), ts.tolist())
    assert (got[L:] == got[L - 1]).all(), (i, "behind a row's end its last jump time repeats")


def test_one_clip_returns_hfs_ids_and_token_timestamps(setup, flags):
    hf, _, pipe, _, io, alone = setup
    one = {k: v[:1] for k, v in io.items()}
    before = flags.engine.calls.get("beam_aligned", 0)
    out = flags.generate(**one, **GK, **TS)
    assert flags.engine.calls["beam_aligned"] == before + 1
    assert out["sequences"].shape == out["token_timestamps"].shape == (1, len(alone[0][0]))
    _check_row(out, 0, alone[0], flags.generation_config.pad_token_id)
    assert np.abs(alone[0][1]).max() > 0.1, "the reference timestamps must not be trivial"
    greedy = hf.generate(**one, **dict(GK, num_beams=1), **TS)
    assert greedy["sequences"][0].tolist() != alone[0][0], "the beams must change HF's ids"


def test_every_row_of_a_batch_equals_hf_for_that_clip_alone(setup, flags):
    """Three clips in one call: every row is what HF gives that clip alone (this model's hypotheses all run to max_new_tokens; rows of
    different lengths are the business of tests/test_gpu_beam_align.py on tests/eos_model.py's model)."""
    _, _, _, _, io, alone = setup
    out = flags.generate(**io, **GK, **TS)
    assert out["sequences"].shape[0] == 3
    for i in range(3):
        _check_row(out, i, alone[i], flags.generation_config.pad_token_id)


def test_pipeline_returns_hfs_words(setup, flags):
    _, hf_pipe, pipe, pcm, _, _ = setup
    got = pipe(pcm[0].copy(), return_timestamps="word", generate_kwargs=dict(GK))
    want = hf_pipe(pcm[0].copy(), return_timestamps="word", generate_kwargs=dict(GK))
    assert got["text"] == want["text"] and len(want["chunks"]) > 2
    assert [c["text"] for c in got["chunks"]] == [c["text"] for c in want["chunks"]]
    for a, b in zip(got["chunks"], want["chunks"]):
        for x, y in zip(a["timestamp"], b["timestamp"]):
            assert (x is None) == (y is None) and (x is None or abs(x - y) <= TOL_S), (a, b)


def test_with_the_new_flag_off_the_old_refusal_stands(setup):
    _, _, pipe, _, io, _ = setup
    model = pipe.model
    assert model.beam_token_timestamps is False
    model.beam_search = True
    try:
        with pytest.raises(NotImplementedError, match="return_token_timestamps with num_beams > 1: a beam result has no alignment rows"):
            model.generate(**io, **GK, **TS)
    finally:
        model.beam_search = False
    model.beam_token_timestamps = True       # ... and the new flag alone does not switch beams on
    try:
        with pytest.raises(NotImplementedError, match="num_beams > 1"):
            model.generate(**io, **GK, **TS)
    finally:
        model.beam_token_timestamps = False


def test_backend_with_beams(setup):
    from thewhisper_amd import AMDWhisperBackend

    _, hf_pipe, pipe, pcm, _, _ = setup
    try:
        backend = AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe, num_beams=3)
        assert pipe.model.beam_search is True and pipe.model.beam_token_timestamps is True
        assert backend.draft_previous_tick is False and backend.reuse_committed_prefix is False      # None resolved to off
        assert backend._generate_kwargs()["num_beams"] == 3 and backend.job_codec() is None
        assert pipe.model._plan_key(dict(input_features=torch.zeros(1, 128, 1000), **backend._generate_kwargs())) is None
        words = backend.transcribe(pcm[0].copy(), 2.0, 16000)
        want = hf_pipe(pcm[0].copy(), return_timestamps="word", generate_kwargs=dict(backend._generate_kwargs()))
        want = AMDWhisperBackend._to_tokens(want, len(pcm[0]) / 16000, 2.0)
        assert [w["text"] for w in words] == [w["text"] for w in want] and len(words) > 2
        for a, b in zip(words, want):
            assert abs(a["start"] - b["start"]) <= TOL_S and abs(a["end"] - b["end"]) <= TOL_S, (a, b)
        with pytest.raises(ValueError, match="hotwords"):
            backend.set_hotwords(["abc"], 2.0)
    finally:
        pipe.model.beam_search = pipe.model.beam_token_timestamps = False


def test_backend_refusals(setup):
    from thewhisper_amd import AMDWhisperBackend

    _, _, pipe, _, _, _ = setup
    mk = lambda **kw: AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=kw.pop("pipe", pipe), num_beams=3, **kw)  # noqa: E731
    try:
        for kw, match in [(dict(hotwords=["abc"], hotword_boost=2.0), "hotwords"), (dict(repetition_penalty=1.2), "repetition_penalty"),
                          (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"), (dict(token_scores=True), "token_scores"),
                          (dict(temperature_fallback=(0.0, 0.4)), "temperature_fallback"),
                          (dict(reuse_committed_prefix=True), "reuse_committed_prefix"), (dict(draft_previous_tick=True), "draft_previous_tick")]:
            with pytest.raises(ValueError, match=match):
                mk(**kw)
        assert pipe.model.beam_search is False, "a refused construction must not switch the model's flags"
        for bad in (9, 0, 2.5, True):
            with pytest.raises(ValueError, match="num_beams"):
                AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe, num_beams=bad)
        with pytest.raises(ValueError, match="batch_size=3"):
            mk(pipe=build(batch_size=2))
        assert AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe, num_beams=None).num_beams is None
        assert AMDWhisperBackend(None, chunk_length_s=CHUNK_S, asr_pipeline=pipe).draft_previous_tick is True      # unchanged default
        assert pipe.model.beam_search is False
    finally:
        pipe.model.beam_search = pipe.model.beam_token_timestamps = False
