"""HF-shaped model object whose arithmetic runs in libthewhisper_gfx950.so.

The reference slots a foreign engine under Hugging Face ``generate()`` in two ways: a whole-class
swap (``elastic_models...WhisperForConditionalGeneration``, R:thestage_speechkit/nvidia/asr_pipeline.py:48-56)
and an encoder/decoder module swap (R:thestage_speechkit/apple/model.py:601-614).  This backend keeps
Whisper's *control flow* from HF (``WhisperGenerationMixin.generate``: init tokens, seek loop, segment
slicing - per chunk, host side) and replaces everything underneath it:

* ``_EngineGreedyMixin.generate`` is inserted in the MRO between ``WhisperGenerationMixin`` and
  ``GenerationMixin``; it is what ``generate_with_fallback`` reaches through ``super().generate``
  (HF:models/whisper/generation_whisper.py:1027) and runs encoder + cross-K/V + the whole greedy
  loop with the Whisper logits processors on the GPU (A2-A10).
* ``_extract_token_timestamps`` is overridden with the on-device median-filter + DTW (A11).

Beam search (``num_beams`` 2..8) runs on the device once ``model.beam_search = True`` (opt-in; ``_beam_generate``); with
``model.beam_token_timestamps = True`` as well, token / word timestamps of a beam call are served from per-row lengths.  Unsupported
generation options (sampling through this seam, custom processors ...) raise ``NotImplementedError``: there is no eager/CPU fallback.
"""
from __future__ import annotations

import logging
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from transformers import WhisperConfig, WhisperForConditionalGeneration
from transformers.generation.logits_process import (
    NoRepeatNGramLogitsProcessor,
    RepetitionPenaltyLogitsProcessor,
    SequenceBiasLogitsProcessor,
    SuppressTokensAtBeginLogitsProcessor,
    SuppressTokensLogitsProcessor,
    WhisperTimeStampLogitsProcessor,
)
from transformers.generation.utils import GenerateEncoderDecoderOutput, GenerationMixin
from transformers.modeling_outputs import Seq2SeqLMOutput

logger = logging.getLogger(__name__)


def dims_from_config(cfg: WhisperConfig) -> Dict[str, int]:
    if cfg.encoder_attention_heads != cfg.decoder_attention_heads or cfg.encoder_ffn_dim != cfg.decoder_ffn_dim:
        raise NotImplementedError("encoder/decoder head or FFN sizes differ")
    return dict(
        d_model=cfg.d_model, enc_layers=cfg.encoder_layers, dec_layers=cfg.decoder_layers,
        heads=cfg.encoder_attention_heads, ffn=cfg.encoder_ffn_dim, vocab=cfg.vocab_size, n_mels=cfg.num_mel_bins,
        max_source_positions=1500, max_target_positions=cfg.max_target_positions,
    )


def _default_engine_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    from .engine import WhisperEngine

    return WhisperEngine(dims, T, max_batch=max_batch, dtype=dtype, alignment_heads=alignment_heads, device=device_index)


def decoder_mask_n_pad(mask, B: int, n_prompt: int) -> Optional[Tuple[int, ...]]:
    """HF's ``decoder_attention_mask`` [B, n_prompt] of a generate call as the engine's per-row padding lengths.  All ones: None (nothing
    is padded; HF's long-form ``condition_on_prev_tokens`` sets such a mask even at batch size 1).  Left padding - zeros, then ones, as
    HF batches previous-text prompts - : the number of zeros per row.  Anything else (a zero behind a one, a row without a real
    token, another shape) is a ``ValueError``: the engine has no rule for it."""
    m = np.asarray(mask.detach().to("cpu").numpy() if isinstance(mask, torch.Tensor) else mask)
    if m.shape != (B, n_prompt):
        raise ValueError(f"decoder_attention_mask of shape {tuple(m.shape)} for decoder_input_ids of shape {(B, n_prompt)}")
    on = m != 0
    if on.all():
        return None
    n_pad = (~on).sum(axis=1)
    if (on != (np.arange(n_prompt)[None, :] >= n_pad[:, None])).any():
        raise ValueError("decoder_attention_mask: only left padding (zeros, then ones) is supported - a row has a zero behind a one")
    if (n_pad >= n_prompt).any():
        raise ValueError("decoder_attention_mask: a row without a real token")
    return tuple(int(x) for x in n_pad)


class _EngineGreedyMixin(GenerationMixin):
    """Replaces ``GenerationMixin.generate`` (-> ``_sample``, HF:generation/utils.py:2783-2946) for the one
    configuration Whisper transcription uses: greedy, num_beams=1, short-form segment in, token ids out."""

    def generate(  # type: ignore[override]
        self,
        inputs: Optional[torch.Tensor] = None,
        generation_config=None,
        logits_processor=None,
        stopping_criteria=None,
        prefix_allowed_tokens_fn=None,
        synced_gpus=None,
        decoder_input_ids: Optional[torch.Tensor] = None,
        attention_mask: Optional[torch.Tensor] = None,
        **kwargs,
    ):
        eng = self._require_engine()
        gc = generation_config if generation_config is not None else self.generation_config
        num_beams = int(kwargs.get("num_beams") or getattr(gc, "num_beams", 1) or 1)
        beams = num_beams > 1 and bool(getattr(self, "beam_search", False))
        self._check_supported(gc, stopping_criteria, prefix_allowed_tokens_fn, kwargs, beams_ok=beams)
        if inputs is None:
            inputs = kwargs.pop("input_features", None)
        if inputs is None or decoder_input_ids is None:
            raise NotImplementedError("the MI355X engine needs `input_features` and `decoder_input_ids`")
        B = int(inputs.shape[0])
        if beams and num_beams > 8:
            raise NotImplementedError(f"num_beams={num_beams}: the MI355X engine searches with 2..8 beams")
        if beams and B * num_beams > eng.max_batch:
            raise ValueError(f"num_beams={num_beams} on a batch of {B} chunks needs {B * num_beams} engine rows, the engine holds "
                             f"max_batch={eng.max_batch}: construct ASRPipeline with batch_size={B * num_beams}")
        if B > eng.max_batch:
            raise ValueError(f"batch of {B} chunks exceeds the engine capacity max_batch={eng.max_batch}; "
                             "construct ASRPipeline with a matching batch_size")
        n_prompt = int(decoder_input_ids.shape[1])
        opts = self._parse_logits_processors(logits_processor, n_prompt)
        bias = self._sequence_bias(gc, logits_processor)
        repeat = self._repeat_options(gc, logits_processor)
        max_target = int(self.config.max_target_positions)
        if getattr(gc, "max_new_tokens", None) is not None:
            max_len = n_prompt + int(gc.max_new_tokens)
        else:
            max_len = int(gc.max_length)
        max_len = min(max_len, max_target)
        min_new = int(getattr(gc, "min_new_tokens", None) or 0)
        if getattr(gc, "min_length", 0) and int(gc.min_length) > n_prompt:
            min_new = max(min_new, int(gc.min_length) - n_prompt)
        eos = gc.eos_token_id
        if isinstance(eos, (list, tuple)):
            if len(eos) != 1:
                raise NotImplementedError("multiple eos_token_id values")
            eos = eos[0]
        pad = gc.pad_token_id if gc.pad_token_id is not None else eos
        n_pad = None
        if kwargs.get("decoder_attention_mask") is not None:
            n_pad = decoder_mask_n_pad(kwargs["decoder_attention_mask"], B, n_prompt)
        if n_pad is not None:
            if not getattr(self, "ragged_decoder_prompts", False):
                raise NotImplementedError(
                    "a left-padded decoder_attention_mask is honoured only with model.ragged_decoder_prompts = True: the MI355X engine decodes "
                    "a padded row as that row alone (HF's batch-1 result for it), NOT with HF's arithmetic for a padded batch, which keeps "
                    "absolute positions so that a row's result depends on its batch-mates' prompt lengths")
            if getattr(self, "score_sink", None) is not None:
                raise ValueError("token scores (score_sink) and a padded decoder_attention_mask do not go together: re-scoring takes no padding")
            if bias:
                raise ValueError("sequence_bias and a padded decoder_attention_mask do not go together")
            if repeat:
                raise ValueError("repetition_penalty / no_repeat_ngram_size and a padded decoder_attention_mask do not go together")
        if repeat and getattr(self, "score_sink", None) is not None:
            raise ValueError("repetition_penalty / no_repeat_ngram_size and token scores (score_sink) do not go together: the re-scoring "
                             "pass does not know the rule")

        if beams:
            return self._beam_generate(eng, gc, inputs, decoder_input_ids, num_beams, opts, bias, repeat, n_pad, kwargs,
                                       dict(max_new_tokens=max_len - n_prompt, min_new_tokens=min_new, max_length=max_target,
                                            eos_id=int(eos), pad_id=int(pad)))
        eng.encode(inputs)
        eng.cross_kv(B)
        want_align = bool(getattr(gc, "return_token_timestamps", False))
        prompt = decoder_input_ids.detach().to("cpu", torch.int32).numpy()
        greedy_kw = dict(max_new_tokens=max_len - n_prompt, min_new_tokens=min_new, max_length=max_target, eos_id=int(eos),
                         pad_id=int(pad), want_alignment=want_align, **opts)
        if bias:
            greedy_kw["sequence_bias"] = bias
        greedy_kw.update(repeat)
        if n_pad is not None:
            greedy_kw["n_pad"] = n_pad
        probe = getattr(self, "_plan_probe", None)
        if probe is not None:   # a call that is learning its short-form plan (shortform.py): what was the engine asked to do?
            probe.append({"prompt": prompt.copy(), "greedy": dict(greedy_kw),
                          "dict": bool(getattr(gc, "return_dict_in_generate", False))})
        out = eng.generate_greedy(prompt, **greedy_kw)
        sink = getattr(self, "score_sink", None)
        if sink is not None:    # AMDWhisperBackend(token_scores=True): the calls HF's own control flow makes are scored too
            from . import shortform

            sink["entries"].extend(shortform.score_entries(eng, out["sequences"], n_prompt, greedy_kw, sink.get("no_speech_id")))
        seq = torch.from_numpy(out["sequences"]).to(decoder_input_ids.device, torch.long)
        self._last_greedy = {"B": B, "n_prompt": n_prompt, "len": int(seq.shape[1])}
        if getattr(gc, "return_dict_in_generate", False):
            return GenerateEncoderDecoderOutput(sequences=seq)
        return seq

    def _beam_generate(self, eng, gc, inputs, decoder_input_ids, num_beams, opts, bias, repeat, n_pad, kwargs, limits):
        """``num_beams`` > 1 with ``beam_search = True``: HF's ``_beam_search`` on the device (tw_generate_beam), the best hypothesis per
        row.  What the beam call cannot do is refused by name.  ``return_token_timestamps`` with ``beam_token_timestamps = True``: the
        call records and gathers the alignment rows (tw_generate_beam_aligned) and leaves the rows' lengths for
        ``_extract_token_timestamps``."""
        want_align = bool(getattr(gc, "return_token_timestamps", False) or kwargs.get("return_token_timestamps"))
        if want_align and not getattr(self, "beam_token_timestamps", False):
            raise NotImplementedError("return_token_timestamps with num_beams > 1: a beam result has no alignment rows on the MI355X engine")
        if bias:
            raise NotImplementedError("sequence_bias with num_beams > 1")
        if repeat:
            raise NotImplementedError("repetition_penalty / no_repeat_ngram_size with num_beams > 1")
        if n_pad is not None:
            raise NotImplementedError("a padded decoder_attention_mask with num_beams > 1")
        if getattr(self, "score_sink", None) is not None:
            raise NotImplementedError("token scores (score_sink) with num_beams > 1")
        early = getattr(gc, "early_stopping", False)
        if early not in (False, True):
            raise NotImplementedError(f"early_stopping={early!r} with num_beams > 1: the MI355X engine implements False and True")
        lp = getattr(gc, "length_penalty", None)
        B = int(inputs.shape[0])
        eng.encode(inputs)
        eng.cross_kv(B)
        prompt = decoder_input_ids.detach().to("cpu", torch.int32).numpy()
        if want_align:   # (only then: an engine without the keyword keeps serving the plain beam call)
            opts = dict(opts, want_alignment=True)
        out = eng.generate_beam(prompt, num_beams, 1.0 if lp is None else float(lp), bool(early), **limits, **opts)
        seq = torch.from_numpy(out["sequences"]).to(decoder_input_ids.device, torch.long)
        self._last_greedy = {"B": B, "n_prompt": int(prompt.shape[1]), "len": int(seq.shape[1])}
        if want_align:   # _extract_token_timestamps serves this call from per-row lengths
            self._last_greedy["lengths"] = [int(x) for x in out["lengths"]]
        if getattr(gc, "return_dict_in_generate", False):
            from transformers.generation.utils import GenerateBeamEncoderDecoderOutput

            return GenerateBeamEncoderDecoderOutput(sequences=seq, sequences_scores=torch.from_numpy(out["scores"]).to(seq.device))
        return seq

    # -- helpers ---------------------------------------------------------------------------------
    @staticmethod
    def _check_supported(gc, stopping_criteria, prefix_allowed_tokens_fn, kwargs, beams_ok=False):
        bad = []
        if not beams_ok and (getattr(gc, "num_beams", 1) not in (None, 1) or kwargs.get("num_beams", 1) not in (None, 1)):
            bad.append("num_beams > 1")
        if getattr(gc, "do_sample", False):
            bad.append("do_sample")
        if stopping_criteria:
            bad.append("custom stopping_criteria")
        if prefix_allowed_tokens_fn is not None:
            bad.append("prefix_allowed_tokens_fn")
        for k in ("assistant_model", "encoder_outputs", "streamer", "past_key_values"):   # (decoder_attention_mask: decoder_mask_n_pad)
            if kwargs.get(k) is not None:
                bad.append(k)
        # (repetition_penalty, no_repeat_ngram_size: _repeat_options)
        if getattr(gc, "num_return_sequences", 1) not in (None, 1):
            bad.append("num_return_sequences > 1")
        if bad:
            raise NotImplementedError("not supported by the MI355X greedy engine: " + ", ".join(bad))

    @staticmethod
    def _sequence_bias(gc, processors) -> Optional[Dict[Tuple[int, ...], float]]:
        """HF's ``sequence_bias`` of the call as the dict ``SequenceBiasLogitsProcessor`` holds: from ``generation_config.sequence_bias``
        (HF builds that processor at the head of its list, HF:generation/utils.py:1154-1155, so Whisper's processors see the biased
        scores - the order the engine applies) or from one such processor in a custom list, which must not stand behind the
        ``WhisperTimeStampLogitsProcessor`` (the timestamp rule would then read unbiased scores)."""
        from .engine import sequence_bias_dict

        found, seen_ts = [], False
        for p in processors or []:
            if isinstance(p, WhisperTimeStampLogitsProcessor):
                seen_ts = True
            elif isinstance(p, SequenceBiasLogitsProcessor):
                if seen_ts:
                    raise NotImplementedError("a SequenceBiasLogitsProcessor behind the WhisperTimeStampLogitsProcessor: the MI355X engine "
                                              "applies the bias ahead of Whisper's processors, as generation_config.sequence_bias does")
                found.append(p.sequence_bias)
        gc_bias = getattr(gc, "sequence_bias", None)
        if gc_bias:
            found.append(gc_bias)
        if len(found) > 1:
            raise NotImplementedError("more than one sequence bias (generation_config.sequence_bias and / or several processors)")
        return sequence_bias_dict(found[0]) if found else None

    @staticmethod
    def _repeat_options(gc, processors) -> Dict[str, Any]:
        """HF's ``repetition_penalty`` / ``no_repeat_ngram_size`` of the call as ``generate_greedy`` keywords (empty: both off): from the
        generation config (HF builds the two processors behind the sequence bias and ahead of Whisper's, HF:generation/utils.py:1154-1183
        - the order the engine applies) or from a ``RepetitionPenaltyLogitsProcessor`` / ``NoRepeatNGramLogitsProcessor`` in a custom
        list, which must stand ahead of the ``WhisperTimeStampLogitsProcessor`` and not ahead of a ``SequenceBiasLogitsProcessor``."""
        pen, ngr, ignore, seen_ts, seen_rep = [], [], 0, False, False
        for p in processors or []:
            if isinstance(p, WhisperTimeStampLogitsProcessor):
                seen_ts = True
            elif isinstance(p, SequenceBiasLogitsProcessor):
                if seen_rep:
                    raise NotImplementedError("a repetition-penalty / no-repeat-n-gram processor ahead of a SequenceBiasLogitsProcessor: the "
                                              "MI355X engine applies the bias first, as HF's generate orders them")
            elif isinstance(p, (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor)):
                if seen_ts:
                    raise NotImplementedError(f"a {type(p).__name__} behind the WhisperTimeStampLogitsProcessor: the MI355X engine applies "
                                              "it ahead of Whisper's processors, as the generation config's option does")
                seen_rep = True
                if isinstance(p, RepetitionPenaltyLogitsProcessor):
                    if getattr(p, "logits_indices", None) is not None:
                        raise NotImplementedError("a RepetitionPenaltyLogitsProcessor with logits_indices")
                    pen.append(float(p.penalty))
                    ignore = int(getattr(p, "prompt_ignore_length", None) or 0)
                else:
                    ngr.append(int(p.ngram_size))
        if getattr(gc, "repetition_penalty", None) not in (None, 1.0):
            pen.append(float(gc.repetition_penalty))
        if getattr(gc, "no_repeat_ngram_size", None) not in (None, 0):
            ngr.append(int(gc.no_repeat_ngram_size))
        if len(pen) > 1 or len(ngr) > 1:
            raise NotImplementedError("repetition_penalty / no_repeat_ngram_size given twice (the generation config and / or several processors)")
        out: Dict[str, Any] = {}
        if pen and pen[0] != 1.0:
            out["repetition_penalty"] = pen[0]
            if ignore:
                out["penalty_ignore"] = ignore
        if ngr and ngr[0] != 0:
            out["no_repeat_ngram_size"] = ngr[0]
        return out

    @staticmethod
    def _parse_logits_processors(processors, n_prompt: int) -> Dict[str, Any]:
        opts: Dict[str, Any] = dict(timestamps=False, begin_suppress=(), suppress=(), no_timestamps_id=0,
                                    max_initial_timestamp_index=None)
        for p in processors or []:
            if isinstance(p, SuppressTokensAtBeginLogitsProcessor):
                if p.begin_index != n_prompt:
                    raise NotImplementedError("begin_index differs from the prompt length")
                opts["begin_suppress"] = tuple(int(x) for x in p.begin_suppress_tokens.tolist())
            elif isinstance(p, SuppressTokensLogitsProcessor):
                opts["suppress"] = tuple(int(x) for x in p.suppress_tokens.tolist())
            elif isinstance(p, WhisperTimeStampLogitsProcessor):
                if p.begin_index != n_prompt or not p._detect_timestamp_from_logprob:
                    raise NotImplementedError("unsupported WhisperTimeStampLogitsProcessor configuration")
                opts["timestamps"] = True
                opts["no_timestamps_id"] = int(p.no_timestamps_token_id)
                opts["max_initial_timestamp_index"] = p.max_initial_timestamp_index
            elif isinstance(p, SequenceBiasLogitsProcessor):
                pass      # read by _sequence_bias
            elif isinstance(p, (RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor)):
                pass      # read by _repeat_options
            else:
                raise NotImplementedError(f"logits processor {type(p).__name__} is not implemented on the MI355X engine")
        return opts


class AMDWhisperForConditionalGeneration(WhisperForConditionalGeneration, _EngineGreedyMixin):
    """``WhisperForConditionalGeneration`` with the hot path on the MI355X engine.

    MRO: AMDWhisper -> WhisperForConditionalGeneration -> WhisperGenerationMixin -> _EngineGreedyMixin ->
    GenerationMixin -> ...; the HF torch modules are kept only as the container the checkpoint loads
    into - after ``build_engine`` their storage is released.
    """

    _engine = None
    _engine_factory: Callable = staticmethod(_default_engine_factory)

    # -- engine lifetime ---------------------------------------------------------------------------
    def build_engine(self, chunk_length_s: int = 30, max_batch: int = 1, dtype: Optional[torch.dtype] = None,
                     engine_factory: Optional[Callable] = None, release_torch_weights: bool = True,
                     decoder_weights: Optional[str] = None):
        """Create the context for T = 50*chunk_length_s encoder frames and upload the weights (A0 is applied by
        the library: tw_finalize_weights interpolates the positional table like patch_hf_model)."""
        if chunk_length_s > 30 or chunk_length_s < 1:
            raise ValueError("chunk_length_s must be in [1, 30]")
        T = int(1500 * (chunk_length_s / 30))  # same expression as R:thestage_speechkit/nvidia/asr_pipeline.py:16
        p0 = next(self.parameters())
        dt = dtype or p0.dtype
        # float16 requests run in a float16 context since round 4 (the reference's streaming default,
        # R:thestage_speechkit/streaming/streaming_pipeline.py:369-370); THEWHISPER_FP16_AS_BF16=1 restores the bf16 mapping
        import os

        eng_dtype = {torch.float32: "f32", torch.float16: "f16"}.get(dt, "bf16")
        if eng_dtype == "f16" and os.environ.get("THEWHISPER_FP16_AS_BF16", "0") == "1":
            logger.warning("fp16 requested: THEWHISPER_FP16_AS_BF16=1, the MI355X engine computes in bf16")
            eng_dtype = "bf16"
        if decoder_weights == "fp8":
            if eng_dtype == "f32":
                raise ValueError("decoder_weights='fp8' needs a bf16 (or fp16) torch_dtype")
            eng_dtype = "fp8"
        heads = getattr(self.generation_config, "alignment_heads", None) or []
        factory = engine_factory or type(self)._engine_factory
        dev_index = p0.device.index if p0.device.type == "cuda" and p0.device.index is not None else 0
        eng = factory(dims_from_config(self.config), T, int(max_batch), eng_dtype, [tuple(h) for h in heads], dev_index)
        sd = {k: v for k, v in self.state_dict().items() if k != "proj_out.weight"}
        eng.load_state_dict(sd)
        self._engine = eng
        self._engine_T = T
        # mirror what patch_hf_model leaves behind, so HF's short-form test `frames <= 2*max_source_positions` holds
        self.config.max_source_positions = T
        if release_torch_weights:
            for p in self.parameters():
                p.data = torch.empty(0, dtype=p.dtype, device=p.device)
        return eng

    def attach_engine(self, engine):
        """Run on an engine whose weights were loaded elsewhere (weights generated on the device, or one context shared by
        several pipelines); the torch modules of this object are then only the container HF's generate() needs."""
        self._engine = engine
        self._engine_T = int(engine.T)
        self.config.max_source_positions = int(engine.T)
        return engine

    def _require_engine(self):
        if self._engine is None:
            raise RuntimeError("AMDWhisperForConditionalGeneration has no engine: call build_engine() "
                               "(thewhisper_amd.ASRPipeline does it); there is no eager fallback")
        return self._engine

    @property
    def engine(self):
        return self._require_engine()

    # -- Whisper control flow: short-form fast path ---------------------------------------------------
    #: False = every call goes through HF's WhisperGenerationMixin.generate (A/B switch; THEWHISPER_FAST_GENERATE=0 too)
    fast_generate: bool = True
    _plans: Optional[Dict[Any, Any]] = None
    _plan_probe: Optional[list] = None
    last_plan = None   # the ShortFormPlan of the most recent eligible call (serving.py picks it up after its warm-up call)
    #: opt-in (streaming.py, token_scores): {"entries": list, "no_speech_id": id or None} - every greedy call made while it is set
    #: appends its token scores (shortform.score_entries) to ``entries``; None = nothing is scored
    score_sink: Optional[Dict[str, Any]] = None
    #: opt-in: honour a LEFT-PADDED ``decoder_attention_mask`` (rows with prompts of different lengths in one generate call) by the ragged
    #: rule of tw_generate_greedy_ragged - every row is decoded as if it were alone, which is HF's batch-1 result for it and NOT HF's
    #: result for the padded batch (HF keeps absolute positions there; DESIGN.md, "Ragged decoder prompts").  An all-ones mask needs no opt-in.
    ragged_decoder_prompts: bool = False
    #: opt-in: ``num_beams`` 2..8 runs HF's beam search on the device (tw_generate_beam) and returns the best hypothesis per row; False:
    #: ``num_beams > 1`` raises NotImplementedError as before.  Needs an engine with ``max_batch >= batch x num_beams``.
    beam_search: bool = False
    #: opt-in, with ``beam_search``: ``return_token_timestamps`` of a beam call is served (tw_generate_beam_aligned records every beam's
    #: alignment rows and gathers them along the ancestry; each row is timed as HF times it when its clip is decoded alone - NOT as HF's
    #: batched beam call, which mixes row 0 of the batch into the shorter hypotheses).  False: the NotImplementedError as before.
    beam_token_timestamps: bool = False

    _FAST_KW = {"input_features", "attention_mask", "generation_config", "return_timestamps", "return_token_timestamps",
                "return_segments", "language", "task", "is_multilingual", "use_cache", "num_beams", "do_sample",
                "max_new_tokens", "min_new_tokens", "max_length", "temperature", "return_dict_in_generate", "sequence_bias", "repetition_penalty",
                "no_repeat_ngram_size"}
    _GC_FIELDS = ("max_new_tokens", "max_length", "min_new_tokens", "min_length", "eos_token_id", "pad_token_id", "suppress_tokens",
                  "begin_suppress_tokens", "no_timestamps_token_id", "max_initial_timestamp_index", "return_timestamps", "task",
                  "language", "num_beams", "do_sample", "temperature", "no_speech_threshold", "logprob_threshold",
                  "compression_ratio_threshold", "condition_on_prev_tokens", "prompt_condition_type", "forced_decoder_ids",
                  "is_multilingual", "return_dict_in_generate", "force_unique_generate_call", "num_return_sequences",
                  "repetition_penalty", "no_repeat_ngram_size", "decoder_start_token_id", "prev_sot_token_id", "sequence_bias")

    def _plan_key(self, kwargs) -> Optional[Tuple]:
        """Hashable fingerprint of everything that shapes a short-form call, or None if the call is not eligible for the
        restated control flow (it then runs HF's own ``generate``)."""
        import os

        if not self.fast_generate or os.environ.get("THEWHISPER_FAST_GENERATE", "1") == "0" or self._engine is None:
            return None
        if any(k not in self._FAST_KW for k in kwargs):
            return None           # prompt_ids, thresholds, logits_processor, stopping criteria, assistant model, ...
        feats = kwargs.get("input_features")
        if not isinstance(feats, torch.Tensor) or feats.dim() != 3 or int(feats.shape[-1]) != 2 * int(self._engine_T):
            return None           # long-form (or malformed) input: HF's loop (and its error messages)
        if int(feats.shape[0]) > self._engine.max_batch or int(feats.shape[0]) < 1:
            return None
        gc = kwargs.get("generation_config") or self.generation_config
        if (kwargs.get("num_beams") or getattr(gc, "num_beams", 1) or 1) > 1:
            return None           # beam calls always run HF's Whisper control flow around the engine call
        lang = kwargs.get("language", getattr(gc, "language", None))
        if isinstance(lang, (list, tuple)):
            return None           # one language per row, given by the caller: HF's route
        auto = lang is None and bool(getattr(gc, "is_multilingual", False))
        if auto and not (hasattr(self._engine, "detect_language") and getattr(gc, "lang_to_id", None)):
            return None           # an engine without tw_detect_language: detection stays HF's forward pass
        if kwargs.get("temperature") not in (None, 0, 0.0) or kwargs.get("return_dict_in_generate"):
            return None
        if kwargs.get("return_token_timestamps") and kwargs.get("attention_mask") is None:
            return None
        def frz(v):
            if isinstance(v, (list, tuple)):
                return tuple(frz(x) for x in v)
            if isinstance(v, dict):
                return tuple(sorted((str(k), frz(x)) for k, x in v.items()))
            if isinstance(v, torch.Tensor):
                return tuple(v.flatten().tolist())
            return v if isinstance(v, (int, float, str, bool, type(None))) else repr(v)
        kw = tuple(sorted((k, frz(v)) for k, v in kwargs.items() if k not in ("input_features", "attention_mask", "generation_config")))
        gcf = tuple(frz(getattr(gc, f, None)) for f in self._GC_FIELDS)
        ah = getattr(gc, "alignment_heads", None)
        if auto:                  # the language is detected per row (tw_detect_language): a plan of its own, with a language slot
            return (kw, gcf, frz(ah), kwargs.get("attention_mask") is None, "auto")
        return (kw, gcf, frz(ah), kwargs.get("attention_mask") is None)

    def generate(self, *args, **kwargs):  # type: ignore[override]
        """``WhisperGenerationMixin.generate`` with a fast path: once a set of call options has been seen, eligible short-form
        batches run the restated seek loop of ``thewhisper_amd.shortform`` (identical results, see that module); the first
        call of each kind - and every call that is not eligible - runs HF's code unchanged."""
        from . import shortform

        key = None if args else self._plan_key(kwargs)
        if key is None:
            return super().generate(*args, **kwargs)
        if self._plans is None:
            self._plans = {}
        plan = self._plans.get(key, False)
        if plan is None:          # learned before: HF's flow did something the plan cannot express
            return super().generate(**kwargs)
        if plan is False:         # first call of this kind: run HF's flow and learn from what it asked the engine to do
            self._plan_probe = []
            try:
                out = super().generate(**kwargs)
                recs = self._plan_probe
            finally:
                self._plan_probe = None
            self._plans[key] = self._learn_plan(kwargs, recs)
            self.last_plan = self._plans[key]
            return out
        self.last_plan = plan
        sink = self.score_sink
        if plan.lang_slot is not None:     # every row's first pass detects its language (shortform.Pass.run)
            langs: List[Optional[int]] = []
            kw = {} if sink is None else dict(scores_out=sink["entries"], no_speech_id=sink.get("no_speech_id"))
            out = shortform.generate_shortform(self._require_engine(), plan, kwargs["input_features"], kwargs.get("attention_mask"),
                                               languages_out=langs, **kw)
            self.last_languages = [int(x) for x in langs]
            return out
        if sink is not None:
            return shortform.generate_shortform(self._require_engine(), plan, kwargs["input_features"], kwargs.get("attention_mask"),
                                                scores_out=sink["entries"], no_speech_id=sink.get("no_speech_id"))
        return shortform.generate_shortform(self._require_engine(), plan, kwargs["input_features"], kwargs.get("attention_mask"))

    def _learn_plan(self, kwargs, recs):
        from . import shortform

        if not recs:
            return None
        g0, p0 = recs[0]["greedy"], recs[0]["prompt"][0]
        if any("n_pad" in r["greedy"] for r in recs):
            return None   # padded rows: the plan tiles ONE prompt over the batch
        gc = kwargs.get("generation_config") or self.generation_config
        # a call whose language was detected (_plan_key: "auto"): the rows' prompts may differ at index 1, by language tokens only
        lang_to_id = getattr(gc, "lang_to_id", None) or {}
        auto = kwargs.get("language", getattr(gc, "language", None)) is None and bool(getattr(gc, "is_multilingual", False)) and bool(lang_to_id)
        lang_ids = tuple(sorted(int(v) for v in lang_to_id.values())) if auto else ()
        for r in recs:   # every inner call of the seek loop must have been the same request, every row the same prompt
            if r["greedy"] != g0 or r["dict"] != recs[0]["dict"] or r["prompt"].shape[1] != len(p0):
                return None
            diff = r["prompt"] != p0[None]
            if auto and len(p0) > 1:
                if not np.isin(r["prompt"][:, 1], lang_ids).all():
                    return None
                diff[:, 1] = False
            if diff.any():
                return None
        if auto and (len(p0) < 2 or len(lang_ids) > 128):
            return None
        nts = getattr(gc, "no_timestamps_token_id", None)
        rt = kwargs.get("return_timestamps")
        if rt is None:
            rt = getattr(gc, "return_timestamps", False)
        return shortform.ShortFormPlan(
            init_tokens=tuple(int(x) for x in p0), greedy=dict(g0), eos=int(g0["eos_id"]), pad=int(g0["pad_id"]),
            timestamp_begin=(int(nts) + 1) if nts is not None else int(self.config.vocab_size) + 1,   # HF:...:1409-1415
            return_timestamps=bool(rt), return_token_timestamps=bool(kwargs.get("return_token_timestamps")),
            return_segments=bool(kwargs.get("return_segments", False)), result_is_dict=bool(recs[0]["dict"]),
            **(dict(lang_slot=1, lang_ids=lang_ids) if auto else {}))

    # -- language detection on the device ---------------------------------------------------------
    #: the language token ids of the most recent detection (``detect_language`` or a ``generate(language=None)`` call), one per row
    last_languages: Optional[List[int]] = None

    def detect_language(self, input_features=None, encoder_outputs=None, generation_config=None, num_segment_frames: int = 3000):  # type: ignore[override]
        """HF's ``detect_language`` (HF:models/whisper/generation_whisper.py:1610-1683) without the full-vocabulary logits: the first
        ``num_segment_frames`` frames are encoded, and tw_detect_language runs the step at ``decoder_start_token_id`` and picks the language
        on the device.  Returns the ``LongTensor`` HF returns.  An engine without the entry answers through ``forward``, as HF does."""
        eng = self._require_engine()
        if not hasattr(eng, "detect_language"):
            return super().detect_language(input_features=input_features, encoder_outputs=encoder_outputs,
                                           generation_config=generation_config, num_segment_frames=num_segment_frames)
        if input_features is None and encoder_outputs is None:
            raise ValueError("You have to specify either `input_features` or `encoder_outputs`")
        if input_features is not None and encoder_outputs is not None:
            raise ValueError("Make sure to specify only one of `input_features` or `encoder_outputs` - not both!")
        if input_features is None:
            raise NotImplementedError("forward() needs input_features: the MI355X engine keeps the encoder states internally and "
                                      "does not accept `encoder_outputs`")
        gc = generation_config or self.generation_config
        B = int(input_features.shape[0])
        eng.encode(input_features[:, :, :num_segment_frames])
        eng.cross_kv(B)
        res = eng.detect_language(B, int(gc.decoder_start_token_id), sorted(int(v) for v in gc.lang_to_id.values()))
        self.last_languages = [int(x) for x in res["ids"][:B]]
        return torch.tensor(self.last_languages, dtype=torch.long, device=input_features.device)

    # -- teacher-forced forward (language detection, parity tests) ---------------------------------
    def forward(self, input_features=None, decoder_input_ids=None, encoder_outputs=None, **kwargs):  # type: ignore[override]
        eng = self._require_engine()
        if decoder_input_ids is None:
            raise NotImplementedError("forward() needs decoder_input_ids")
        if input_features is not None:
            B = int(input_features.shape[0])
            eng.encode(input_features)
            eng.cross_kv(B)
        else:
            # the encoder states live inside the engine (A2-A5): a tensor of `encoder_outputs` cannot be handed to it, and decoding
            # against whatever the engine encoded LAST would silently answer for other audio.  HF's own callers of this form
            # (detect_language, HF:models/whisper/generation_whisper.py:1610-1683) pass input_features whenever they have them.
            raise NotImplementedError("forward() needs input_features: the MI355X engine keeps the encoder states internally and "
                                      "does not accept `encoder_outputs`")
        B = int(decoder_input_ids.shape[0])
        eng.decoder_reset(B)
        ids = decoder_input_ids.detach().to("cpu").numpy()
        cols = []
        for j in range(ids.shape[1]):
            cols.append(eng.decode_step(ids[:, j].tolist()))
        logits = torch.stack(cols, dim=1)
        return Seq2SeqLMOutput(logits=logits)

    # -- A11 -------------------------------------------------------------------------------------
    def _extract_token_timestamps(self, generate_outputs, alignment_heads, time_precision=0.02, num_frames=None,
                                  num_input_ids=None):
        """On-device replacement of HF:models/whisper/generation_whisper.py:241-381 (5.15.0 semantics)."""
        eng = self._require_engine()
        st = self._last_greedy
        seq = generate_outputs["sequences"]
        B, L = int(seq.shape[0]), int(seq.shape[1])
        if st["B"] != B or st["len"] != L:
            raise RuntimeError("token timestamps requested for a generate() call the engine no longer holds")
        n_in = int(num_input_ids if num_input_ids is not None else st["n_prompt"])
        # which columns HF keeps depends on the type and uniformity of `num_frames` (shortform.hf_kept_columns); the engine crops once per row
        from .shortform import columns_as_num_frames, hf_kept_columns

        nf = None if num_frames is None else columns_as_num_frames(hf_kept_columns(num_frames, B, int(eng.T)))
        if st.get("lengths") is not None:
            # a beam call (beam_token_timestamps): every best hypothesis on its own rows, as HF times it when its clip is decoded alone
            # (tw_generate_beam_aligned, THE RULE; HF's batched call mixes global row 0 into the shorter hypotheses)
            ts = eng.token_timestamps_each(st["lengths"], n_in, nf, time_precision, ld=L)
            return torch.from_numpy(ts).to(seq.device)
        if L - 1 <= n_in:  # one generated token: no cross-attention rows after the prompt -> zeros (HF :341-344)
            return torch.zeros((B, L), dtype=torch.float32, device=seq.device)
        ts = eng.token_timestamps(B, n_in, L, nf, time_precision)
        return torch.from_numpy(ts).to(seq.device)

    # -- construction helpers --------------------------------------------------------------------
    @classmethod
    def from_hf(cls, hf_model: WhisperForConditionalGeneration) -> "AMDWhisperForConditionalGeneration":
        """Re-class an already loaded HF model (weights shared, no copy)."""
        if isinstance(hf_model, cls):
            return hf_model
        if not isinstance(hf_model, WhisperForConditionalGeneration):
            raise TypeError("expected a transformers WhisperForConditionalGeneration")
        hf_model.__class__ = cls
        hf_model._engine = None
        return hf_model
