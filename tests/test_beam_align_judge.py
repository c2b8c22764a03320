"""tests/beam_align_judge.py against HF's own token timestamps of a beam result, and what the fixtures must exercise.  No GPU.

The reference is HF with the clip decoded ALONE: `GenerationMixin.generate(..., num_beams=K, output_attentions=True)` on one clip with eager
attention, then `_extract_token_timestamps(out, HEADS, num_input_ids=N_PROMPT)` - HF gathers the cross-attention rows along `beam_indices`.
(In a batch HF fills `beam_indices == -1` behind a hypothesis's end with 0, the batch's row 0, and those rows enter the shorter
hypotheses' z-score and DTW: include/thewhisper.h, tw_generate_beam_aligned.)  This test passes without the device feature: it pins the
reference the GPU tests use.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import beam_align_judge as baj
from tests import beam_judge as bj
from tests import eos_model as em

TOL_S = 1e-6


@functools.lru_cache(maxsize=None)
def hf_model(es: float):
    """tests/test_beam_judge.py's model of eos_model's weights, with eager attention (the only one that returns attention weights)."""
    from transformers import WhisperConfig, WhisperForConditionalGeneration

    dims, w = em.model(es)
    cfg = WhisperConfig(vocab_size=dims.vocab, num_mel_bins=dims.n_mels, d_model=dims.d_model, encoder_layers=dims.enc_layers,
                        decoder_layers=dims.dec_layers, encoder_attention_heads=dims.heads, decoder_attention_heads=dims.heads,
                        encoder_ffn_dim=dims.ffn, decoder_ffn_dim=dims.ffn, max_source_positions=em.T,
                        max_target_positions=dims.max_target_positions, bos_token_id=em.EOS, eos_token_id=em.EOS, pad_token_id=em.EOS,
                        decoder_start_token_id=3, activation_function="gelu", dropout=0.0, attention_dropout=0.0,
                        activation_dropout=0.0, use_cache=True, suppress_tokens=None, begin_suppress_tokens=None,
                        attn_implementation="eager")
    model = WhisperForConditionalGeneration(cfg)
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in w.items()}
    sd["model.encoder.embed_positions.weight"] = torch.from_numpy(
        wo.interpolate_positions(np.asarray(w["model.encoder.embed_positions.weight"], dtype=np.float32), em.T))
    sd["proj_out.weight"] = sd["model.decoder.embed_tokens.weight"]
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all("proj_out" in m for m in missing), (missing, unexpected)
    model.tie_weights()
    return model.eval()


def hf_generate(case: bj.Case, clips, n_return: int, attentions: bool):
    from transformers import GenerationConfig
    from transformers.generation.logits_process import (LogitsProcessorList, SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.utils import GenerationMixin

    model = hf_model(case.es)
    dims, _ = em.model(case.es)
    mel = torch.from_numpy(wo.log_mel(em.audio(clips), dims.n_mels))
    gc = GenerationConfig(eos_token_id=em.EOS, pad_token_id=em.EOS, bos_token_id=em.EOS, decoder_start_token_id=3,
                          max_new_tokens=case.max_new, min_new_tokens=case.min_new or None, num_beams=case.K, num_return_sequences=n_return,
                          early_stopping=case.early, length_penalty=case.length_penalty, do_sample=False, use_cache=True,
                          return_dict_in_generate=True, output_scores=True, output_attentions=attentions)
    gc.no_timestamps_token_id = em.NO_TS
    gc.max_initial_timestamp_index = 50
    procs = LogitsProcessorList()
    if case.begin_suppress:
        procs.append(SuppressTokensAtBeginLogitsProcessor(list(case.begin_suppress), begin_index=em.N_PROMPT))
    if case.suppress:
        procs.append(SuppressTokensLogitsProcessor(list(case.suppress)))
    if case.timestamps:
        procs.append(WhisperTimeStampLogitsProcessor(gc, begin_index=em.N_PROMPT))
    with torch.no_grad():
        return model, GenerationMixin.generate(model, input_features=mel, decoder_input_ids=torch.from_numpy(em.prompt(clips)).long(),
                                               generation_config=gc, logits_processor=procs)


def hf_alone(case: bj.Case, clip: int):
    """(ids, token timestamps float32) of HF's best hypothesis for this clip decoded alone."""
    model, out = hf_generate(case, [clip], 1, True)
    ts = model._extract_token_timestamps(out, baj.HEADS, num_input_ids=em.N_PROMPT)
    return out.sequences[0].tolist(), ts[0].numpy().astype(np.float32)


@pytest.mark.parametrize("name", [c.name for c in bj.CASE_LIST])
def test_judge_equals_hf_decoding_the_clip_alone(name):
    case = bj.case(name)
    worst, n_tok = 0.0, 0
    for clip in bj.CASES[name]:
        ids, ts = hf_alone(case, clip)
        ref = baj.run(case, clip)
        h = ref["nbest"][0]
        assert ids == list(h), (name, clip, ids, list(h))      # batch of one: no padding behind the best hypothesis
        assert ts.shape == ref["timestamps"][0].shape, (name, clip)
        d = float(np.abs(ts.astype(np.float64) - ref["timestamps"][0].astype(np.float64)).max())
        worst = max(worst, d)
        n_tok += len(h) - em.N_PROMPT
        assert d <= TOL_S, (name, clip, ts.tolist(), ref["timestamps"][0].tolist())
    print(f"{name}: {len(bj.CASES[name])} clips, {n_tok} generated tokens, largest |judge - HF alone| {worst:.2e} s")


@functools.lru_cache(maxsize=None)
def hf_paths(name: str):
    """Per fixture clip of the case: HF's beam_indices of its K returned hypotheses as slots 0 .. K-1 (-1 behind the end), int [K, steps],
    from ONE batched call (the paths of a clip do not depend on its batch-mates: tests/test_beam_judge.py)."""
    case = bj.case(name)
    clips = list(bj.CASES[name])
    _, out = hf_generate(case, clips, case.K, False)
    bi = out.beam_indices.numpy().reshape(len(clips), case.K, -1)
    local = np.where(bi >= 0, bi % case.K, -1)
    assert all(((bi[i] < 0) | (bi[i] // case.K == i)).all() for i in range(len(clips)))     # a path stays inside its clip
    return {clip: local[i] for i, clip in enumerate(clips)}


def _slot_changes(path) -> int:
    p = path[path >= 0]
    return int((np.diff(p) != 0).sum())


@pytest.mark.parametrize("name", [c.name for c in bj.CASE_LIST])
def test_fixtures_exercise_the_ancestry(name):
    """From HF's beam_indices alone: at least three clips whose best path changes slot at least twice (a gather that took every row from
    the hypothesis's final slot would fail on them), and a clip whose hypotheses end at different lengths."""
    paths = hf_paths(name)
    movers = [c for c, p in paths.items() if _slot_changes(p[0]) >= 2]
    assert len(movers) >= 3, (name, {c: _slot_changes(p[0]) for c, p in paths.items()})
    ragged = [c for c, p in paths.items() if len({int((row >= 0).sum()) for row in p if (row >= 0).any()}) > 1]
    assert ragged, name
    print(f"{name}: best path changes slot twice or more on clips {movers}; hypotheses of different lengths on clips {ragged}")


def test_some_clip_has_paths_that_share_a_slot_and_part():
    """In at least one case a clip in which two n-best paths sit in the same slot at one step and in different slots at another: the
    gather has to serve two destinations from one source, and a destination can be another hypothesis's source."""
    found = []
    for case in bj.CASE_LIST:
        for clip, p in hf_paths(case.name).items():
            for a in range(case.K):
                for b in range(a + 1, case.K):
                    both = (p[a] >= 0) & (p[b] >= 0)
                    if (both & (p[a] == p[b])).any() and (both & (p[a] != p[b])).any():
                        found.append((case.name, clip, a, b))
    assert found
    print(f"{len(found)} (case, clip, hypothesis pair) share a slot at one step and differ at another, e.g. {found[:3]}")
