"""`generate(num_beams=K)` through the drop-in, on the CPU: with `model.beam_search = True` the seeded micro model behind a numpy stand-in
engine that searches by tests/beam_judge.py returns the ids of HF's own `WhisperForConditionalGeneration.generate`; with the flag off
the old NotImplementedError stands; everything the beam call cannot do is refused by name."""
import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests import beam_judge as bj
from tests.oracle_engine import OracleEngine

torch.set_grad_enabled(False)
CHUNK_S = 10
GK = {"do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 12}


class BeamOracleEngine(OracleEngine):
    """The stand-in engine with `WhisperEngine.generate_beam`, by the judge."""

    def generate_beam(self, prompt, num_beams, length_penalty=1.0, early_stopping=False, *, max_new_tokens=128, min_new_tokens=0,
                      max_length=448, eos_id=50257, pad_id=50257, timestamps=False, no_timestamps_id=50364, max_initial_timestamp_index=50,
                      begin_suppress=(220, 50257), suppress=()):
        self.calls["generate"] += 1
        self.calls["beam"] = self.calls.get("beam", 0) + 1
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
        return {"sequences": best, "scores": np.asarray([r["scores"][0] for r in runs], np.float32), "nbest_sequences": nbest,
                "nbest_scores": np.stack([r["scores"] for r in runs]), "length": int(best.shape[1])}


def beam_engine_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return BeamOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


def build(batch_size=9):
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    model = hr.build_hf_model(dims, wo.make_weights(dims, 0))
    return ASRPipeline(model, feature_extractor=hr.build_feature_extractor(dims, CHUNK_S), tokenizer=hr.build_tokenizer(dims),
                       chunk_length_s=CHUNK_S, device="cpu", torch_dtype=torch.float32, batch_size=batch_size,
                       engine_factory=beam_engine_factory)


@pytest.fixture(scope="module")
def setup():
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), CHUNK_S)
    pipe = build()
    pcm = [wo.synth_audio(CHUNK_S * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    return hf, pipe, dict(input_features=feats.input_features, attention_mask=feats.attention_mask)


def ids_of(out):
    return (out["sequences"] if isinstance(out, dict) else out).tolist()


@pytest.mark.parametrize("timestamps", [False, True])
def test_generate_with_beams_returns_hfs_ids(setup, timestamps):
    hf, pipe, io = setup
    model = pipe.model
    model.beam_search = True
    try:
        kw = dict(GK, num_beams=3, return_timestamps=timestamps)
        ref = ids_of(hf.generate(**io, **kw))
        assert ref != ids_of(hf.generate(**io, **dict(kw, num_beams=1))), "the beams must change HF's ids"
        before = model.engine.calls.get("beam", 0)
        assert ids_of(model.generate(**io, **kw)) == ref
        assert ids_of(model.generate(**io, **kw)) == ref          # no short-form plan is learned for a beam call
        assert model.engine.calls["beam"] >= before + 2
        out = model.generate(**io, **kw, return_dict_in_generate=True)
        assert ids_of(out) == ids_of(hf.generate(**io, **kw, return_dict_in_generate=True))
    finally:
        model.beam_search = False


def test_without_the_flag_beams_are_refused_as_before(setup):
    _, pipe, io = setup
    assert pipe.model.beam_search is False
    with pytest.raises(NotImplementedError, match="num_beams > 1"):
        pipe.model.generate(**io, **GK, num_beams=3)


def test_what_the_beam_call_cannot_do_is_refused_by_name(setup):
    _, pipe, io = setup
    model = pipe.model
    model.beam_search = True
    try:
        kw = dict(GK, num_beams=3)
        for extra, exc, match in [
            (dict(return_token_timestamps=True, return_timestamps=True), NotImplementedError, "return_token_timestamps"),
            (dict(sequence_bias=[[[9], -5.0]]), NotImplementedError, "sequence_bias"),
            (dict(repetition_penalty=1.3), NotImplementedError, "repetition_penalty"),
            (dict(no_repeat_ngram_size=2), NotImplementedError, "no_repeat_ngram_size"),
            (dict(early_stopping="never"), NotImplementedError, "early_stopping"),
            (dict(num_beams=9), NotImplementedError, "2..8"),
            (dict(num_beams=4), ValueError, "batch_size=12"),
        ]:
            with pytest.raises(exc, match=match):
                model.generate(**io, **dict(kw, **extra))
        model.score_sink = {"entries": [], "no_speech_id": None}
        try:
            with pytest.raises(NotImplementedError, match="score_sink"):
                model.generate(**io, **kw)
        finally:
            model.score_sink = None
        assert model._plan_key(dict(io, **kw)) is None
    finally:
        model.beam_search = False


def test_a_padded_decoder_mask_with_beams_is_refused(setup):
    """A left-padded `decoder_attention_mask` with num_beams = 3: with `ragged_decoder_prompts = True` the beam refusal names it; with
    the flag False the user sees the ragged-prompt message (which comes first and names the attribute)."""
    from thewhisper_amd.engine import pack_ragged_prompts

    _, pipe, io = setup
    model = pipe.model
    init = [50258, 50259, 50360]
    ids, n_pad = pack_ragged_prompts([[50361, 1200, 1201, 1202] + init, [50361, 1300] + init, init], 50257)
    assert n_pad.tolist() == [0, 2, 4]
    ids_t = torch.from_numpy(ids).long()
    kw = dict(GK, num_beams=3, task="transcribe", return_timestamps=False, decoder_input_ids=ids_t, decoder_attention_mask=ids_t != 50257)
    model.beam_search = True
    try:
        assert model.ragged_decoder_prompts is False
        with pytest.raises(NotImplementedError, match="ragged_decoder_prompts"):
            model.generate(**io, **kw)
        model.ragged_decoder_prompts = True
        try:
            calls = model.engine.calls["generate"]
            with pytest.raises(NotImplementedError, match="padded decoder_attention_mask with num_beams > 1"):
                model.generate(**io, **kw)
            assert model.engine.calls["generate"] == calls
        finally:
            model.ragged_decoder_prompts = False
    finally:
        model.beam_search = False
