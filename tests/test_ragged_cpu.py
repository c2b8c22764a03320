"""Ragged decoder prompts (tw_generate_greedy_ragged) above the library, on the CPU: the packing helper, the engine-side and drop-in
validation, the mask parser, and the drop-in on a numpy stand-in engine that decodes every padded row ALONE - which is the rule.

Reference = the installed HF model with the same seeded weights.  For a left-padded batch the drop-in (opt-in:
``model.ragged_decoder_prompts``) returns HF's BATCH-1 ids of every row, not HF's ids for the padded batch (HF keeps absolute positions
there; DESIGN.md, "Ragged decoder prompts").  With an all-ones mask - what HF's long-form ``condition_on_prev_tokens=True`` sets at batch
size 1 - nothing is padded and the ids are HF's outright."""
import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests.oracle_engine import OracleEngine

torch.set_grad_enabled(False)
CHUNK_S = 10
PAD = 50257
INIT = [50258, 50259, 50360]          # <|startoftranscript|><|en|><|transcribe|>


class RaggedOracleEngine(OracleEngine):
    """tests/oracle_engine.OracleEngine that takes ``n_pad`` by the rule's own words: every padded row is decoded alone, with its real
    tokens and ``max_length - n_pad[b]``, and put back behind its padding.  Keeps what it was asked (``asked``)."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.asked = []

    def generate_greedy(self, prompt, n_pad=None, **kw):
        from thewhisper_amd.engine import ragged_n_pad

        prompt = np.asarray(prompt)
        B, n = prompt.shape
        self.asked.append({"prompt": prompt.copy(), "n_pad": None if n_pad is None else tuple(int(x) for x in n_pad)})
        pads = ragged_n_pad(n_pad, B, kw.get("n_forced", 0), kw.get("n_draft", 0))
        if pads is None:
            return super().generate_greedy(prompt, **kw)
        assert ((pads >= 0) & (pads < n)).all(), "the library refuses these (TW_EINVAL)"
        enc, rows = self._enc, []
        pad_id, max_length = kw.get("pad_id", PAD), kw.get("max_length", 448)
        try:
            for b in range(B):
                self._enc = enc[b:b + 1]
                alone = super().generate_greedy(prompt[b:b + 1, pads[b]:], **{**kw, "max_length": max_length - int(pads[b])})
                rows.append(np.concatenate([prompt[b, :pads[b]], alone["sequences"][0]]))
        finally:
            self._enc = enc
        L = max(len(r) for r in rows)
        seq = np.full((B, L), pad_id, dtype=np.int64)
        for b, r in enumerate(rows):
            seq[b, :len(r)] = r
        return {"sequences": seq, "length": L}


def ragged_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return RaggedOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


def build(batch_size=3, engine_factory=ragged_factory, device="cpu"):
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    ref = hr.patch_chunk_length(hr.build_hf_model(dims, w), CHUNK_S)
    kw = {} if engine_factory is None else {"engine_factory": engine_factory}
    pipe = ASRPipeline(hr.build_hf_model(dims, w), feature_extractor=hr.build_feature_extractor(dims, CHUNK_S), tokenizer=hr.build_tokenizer(dims),
                       chunk_length_s=CHUNK_S, device=device, torch_dtype=torch.float32, batch_size=batch_size, **kw)
    return dims, ref, pipe


def ragged_rows():
    """Three decoder prompts - 0, 3 and 6 pads in a batch of length 9 - : `previous text` of different lengths in front of the init tokens."""
    prev = [[50361, 1200, 1201, 1202, 1203, 1204], [50361, 1300, 1301], []]
    return [p + INIT for p in prev]


def check_dropin_against_hf_batch_1(device, engine_factory):
    """Shared with tests/test_gpu_ragged.py (there: the MI355X engine in strict f32)."""
    from thewhisper_amd.engine import pack_ragged_prompts

    dims, ref, pipe = build(3, engine_factory, device)
    model = pipe.model
    clips = [wo.synth_audio(CHUNK_S * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    feats = pipe.feature_extractor(clips, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    x, am = feats["input_features"].cpu(), feats["attention_mask"].cpu()      # (the reference model lives on the CPU)
    rows = ragged_rows()
    ids, n_pad = pack_ragged_prompts(rows, PAD)
    assert n_pad.tolist() == [0, 3, 6] and ids.shape == (3, 9)
    ids_t = torch.from_numpy(ids).long()
    mask = ids_t != PAD
    n_new = 12
    dev = model.device
    io = dict(input_features=x.to(dev), attention_mask=am.to(dev), decoder_input_ids=ids_t.to(dev))
    gk0 = dict(num_beams=1, do_sample=False, language="en", task="transcribe", max_new_tokens=n_new, min_new_tokens=n_new)
    # without the opt-in: refused, naming the attribute
    assert model.ragged_decoder_prompts is False
    with pytest.raises(NotImplementedError, match="ragged_decoder_prompts"):
        model.generate(**io, decoder_attention_mask=mask.to(dev), return_timestamps=False, **gk0)
    for ts in (False, True):
        gk = dict(gk0, return_timestamps=ts)
        model.ragged_decoder_prompts = True
        try:
            got = model.generate(**io, decoder_attention_mask=mask.to(dev), **gk).cpu()
            # a padded call made while token scores are collected is refused
            model.score_sink = {"entries": [], "no_speech_id": None}
            try:
                with pytest.raises(ValueError, match="score_sink"):
                    model.generate(**io, decoder_attention_mask=mask.to(dev), **gk)
            finally:
                model.score_sink = None
        finally:
            model.ragged_decoder_prompts = False
        # (HF's generate returns the new tokens without the decoder_input_ids; with timestamps it cuts every row behind its last complete
        #  segment and pads the batch to its longest row, so a batch-1 row may be shorter than its row of a batch: padding behind it)
        assert got.shape[0] == 3 and (ts or got.shape[1] == n_new), got.shape
        for b, row in enumerate(rows):
            alone = ref.generate(input_features=x[b:b + 1], attention_mask=am[b:b + 1], decoder_input_ids=torch.tensor([row]), **gk)[0]
            n = alone.shape[0]
            assert (ts or n == n_new) and n <= got.shape[1]
            assert torch.equal(got[b, :n], alone) and (got[b, n:] == PAD).all(), (ts, b, got[b], alone)
        assert len({tuple(r.tolist()) for r in got}) == 3, "the rows must decode to different ids, or the comparison says nothing about rows"
        # (the deviation is real: HF's ids for the padded BATCH are not its batch-1 ids - a padded row keeps absolute positions there)
        padded_hf = ref.generate(input_features=x, attention_mask=am, decoder_input_ids=ids_t, decoder_attention_mask=mask, **gk)
        assert not torch.equal(padded_hf, got)
    gk = dict(gk0, return_timestamps=True)
    # an all-ones mask needs no opt-in, and equals HF with the same mask (rows of equal length: nothing is padded)
    same = torch.tensor([rows[1]] * 3)
    ones = torch.ones_like(same, dtype=torch.bool)
    want = ref.generate(input_features=x, attention_mask=am, decoder_input_ids=same, decoder_attention_mask=ones, **gk)
    have = model.generate(input_features=x.to(dev), attention_mask=am.to(dev), decoder_input_ids=same.to(dev),
                          decoder_attention_mask=ones.to(dev), **gk).cpu()
    assert torch.equal(want, have), (want, have)
    return model


def test_pack_ragged_prompts_round_trips():
    from thewhisper_amd.engine import pack_ragged_prompts

    rows = [[5, 6, 7], [9], np.array([1, 2, 3, 4, 5]), (8, 8)]
    ids, n_pad = pack_ragged_prompts(rows, 77)
    assert ids.dtype == np.int32 and n_pad.dtype == np.int32 and ids.shape == (4, 5)
    assert n_pad.tolist() == [2, 4, 0, 3]
    for b, r in enumerate(rows):
        assert ids[b, n_pad[b]:].tolist() == list(r) and (ids[b, : n_pad[b]] == 77).all()
    one, z = pack_ragged_prompts([[1, 2]], 0)
    assert one.tolist() == [[1, 2]] and z.tolist() == [0]
    for bad in ([], [[1], []]):
        with pytest.raises(ValueError, match="pack_ragged_prompts"):
            pack_ragged_prompts(bad, 0)


def test_engine_side_validation_needs_no_context():
    """`WhisperEngine.generate_greedy` checks ``n_pad`` before it touches its context: the refusals are reachable on an object without one."""
    from thewhisper_amd.engine import WhisperEngine, ragged_n_pad

    eng = WhisperEngine.__new__(WhisperEngine)          # no context, no library: the checks come first
    prompt = np.array([[PAD, 50258, 50259]] * 2)
    for kw in (dict(n_forced=1), dict(n_draft=1), dict(sequence_bias=[[[5], 1.0]]), dict(sequence_bias_rows=[None, [[[5], 1.0]]])):
        with pytest.raises(ValueError, match="n_pad does not go together"):
            eng.generate_greedy(prompt, n_pad=[1, 0], **kw)
    for bad in ([1], [[1, 0]], [0.5, 0.0], 1):
        with pytest.raises(ValueError, match="one integer per row"):
            eng.generate_greedy(prompt, n_pad=bad)
    with pytest.raises(ValueError, match="n_pad does not go together"):
        eng.generate_greedy_ragged([[50258], [50258, 50259]], n_forced=1)
    assert ragged_n_pad(None, 2) is None
    got = ragged_n_pad((1, 0), 2)
    assert got.dtype == np.int32 and got.tolist() == [1, 0]
    eng.ctx = None                                       # (what close() leaves behind: __del__ has nothing to release)


def test_mask_parser():
    from thewhisper_amd.model import decoder_mask_n_pad

    assert decoder_mask_n_pad(torch.ones(2, 4, dtype=torch.bool), 2, 4) is None
    assert decoder_mask_n_pad(torch.ones(1, 1, dtype=torch.long), 1, 1) is None
    m = torch.tensor([[1, 1, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]])
    assert decoder_mask_n_pad(m, 3, 4) == (0, 2, 1)
    assert decoder_mask_n_pad(m.bool().numpy(), 3, 4) == (0, 2, 1)
    with pytest.raises(ValueError, match="zero behind a one"):
        decoder_mask_n_pad(torch.tensor([[1, 1, 0, 1]]), 1, 4)
    with pytest.raises(ValueError, match="zero behind a one"):
        decoder_mask_n_pad(torch.tensor([[0, 1, 0, 1], [1, 1, 1, 1]]), 2, 4)
    with pytest.raises(ValueError, match="zero behind a one"):
        decoder_mask_n_pad(torch.tensor([[1, 1, 1, 0]]), 1, 4)          # right padding
    with pytest.raises(ValueError, match="without a real token"):
        decoder_mask_n_pad(torch.tensor([[0, 0], [1, 1]]), 2, 2)
    with pytest.raises(ValueError, match="shape"):
        decoder_mask_n_pad(torch.ones(2, 3), 2, 4)


def test_dropin_padded_rows_are_hfs_batch_1_rows():
    model = check_dropin_against_hf_batch_1("cpu", ragged_factory)
    asked = model.engine.asked
    assert [a["n_pad"] for a in asked] == [(0, 3, 6), (0, 3, 6), None], "two padded engine calls, one plain one (the all-ones mask)"


def test_encoder_outputs_and_the_rest_of_the_list_stay_refused():
    _, _, pipe = build(1)
    ids = torch.tensor([INIT])
    for k in ("assistant_model", "encoder_outputs", "streamer", "past_key_values"):
        with pytest.raises(NotImplementedError, match=k):
            pipe.model.__class__.__mro__[3].generate(pipe.model, torch.zeros(1, 128, 1000), decoder_input_ids=ids, **{k: object()})


def test_longform_previous_text_conditioning_at_batch_1():
    """HF's long-form loop with ``condition_on_prev_tokens=True`` prepends the previous segments' text to every chunk's prompt and sets
    an (all-ones, at batch 1) decoder_attention_mask: it used to end in NotImplementedError on this backend."""
    dims, ref, pipe = build(1)
    model = pipe.model
    # (the seeded micro model emits timestamps up to 29.7 s whatever the chunk length, and HF seeks by them: 65 s give three chunks)
    clip = wo.synth_audio(65 * 16000, 5, "speechlike")
    feats = pipe.feature_extractor([clip], sampling_rate=16000, return_tensors="pt", truncation=False, padding="longest",
                                   return_attention_mask=True)
    gk = dict(num_beams=1, do_sample=False, language="en", task="transcribe", return_timestamps=True, condition_on_prev_tokens=True,
              max_new_tokens=24)
    io = dict(input_features=feats["input_features"], attention_mask=feats["attention_mask"])
    assert io["input_features"].shape[-1] > 2 * 50 * CHUNK_S, "longer than one chunk"
    want = ref.generate(**io, **gk)
    model._plan_probe = []               # record what the engine is asked, as a learning call does
    try:
        got = model.generate(**io, **gk)
        recs = model._plan_probe
    finally:
        model._plan_probe = None
    assert torch.equal(want, got), (want, got)
    longest = max(r["prompt"].shape[1] for r in recs)
    assert len(recs) >= 2 and longest > len(INIT) + 1, ("no call carried previous text: choose another clip", [r["prompt"].shape for r in recs])
    assert all("n_pad" not in r["greedy"] for r in recs), "batch 1: nothing is padded"
