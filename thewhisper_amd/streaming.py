"""``AMDWhisperBackend`` - the ``platform="amd"`` transcription backend for the reference's StreamingPipeline.

Implements the ``TranscriptionBackend.transcribe(audio, buffer_start_time, sample_rate) -> [{"text","start","end"}]``
contract (R:thestage_speechkit/streaming/streaming_pipeline.py:51-64) exactly as ``LocalWhisperBackend`` does
for the other platforms (R:...:340-435): fixed greedy generate kwargs with ``max_new_tokens=128``, word
timestamps always on, the zlib gibberish filter (>2.2 -> ``[]``) and the open-ended last-word fix-up.
Use it through the reference's injection seam ``StreamingPipeline(backend=AMDWhisperBackend(...))`` or via the
three-line ``platform == "amd"`` patch shown in INTEGRATION.md.
"""
from __future__ import annotations

import zlib
from typing import Any, Dict, List, Optional

import numpy as np
import torch


def _compression_ratio(text: str) -> float:
    """R:thestage_speechkit/streaming/streaming_pipeline.py:41-43."""
    text_bytes = text.encode("utf-8")
    return len(text_bytes) / len(zlib.compress(text_bytes))


class AMDWhisperBackend:
    """Duck-typed ``TranscriptionBackend`` (the ABC lives in the reference package)."""

    def __init__(
        self,
        model,
        model_size: str = "S",
        chunk_length_s: int = 10,
        torch_dtype: "torch.dtype | None" = None,
        language: Optional[str] = "en",
        feature_extractor=None,
        tokenizer=None,
        revision: str = "main",
        asr_pipeline=None,
        reuse_committed_prefix: bool = False,
        reuse_margin_s: float = 1.0,
        draft_previous_tick: Optional[bool] = None,
        resample_kernel=None,
        token_scores: bool = False,
        temperature_fallback=None,
        hotwords=None,
        hotword_boost: Optional[float] = None,
        repetition_penalty: Optional[float] = None,
        no_repeat_ngram_size: Optional[int] = None,
        num_beams: Optional[int] = None,
        sticky_language: bool = False,
        **pipeline_kwargs,
    ):
        """``reuse_committed_prefix`` (never the default): the reference scheduler hands over, every 0.5 s,
        a rolling buffer most of which the previous call already transcribed (R:...streaming_pipeline.py:770-796 re-decodes all
        of it).  With the option on, a call whose buffer EXTENDS the previous call's (same ``buffer_start_time``, at least as
        long, one chunk) hands the previous call's tokens whose word timestamps end at least ``reuse_margin_s`` before the old
        buffer's end to the greedy loop as forced output - one batched prefill (tw_greedy_opts::n_forced) instead of one decode
        step each - and decodes only the tail.  The audio those tokens belong to is unchanged, but the encoder is not causal and
        the log-mel clamp is global, so the forced tokens need not be what a fresh decode would pick: an approximation, whose
        delta bench.py / tests measure.  ``reuse_stats`` counts calls, reused calls and forced tokens.
        The option needs ONE BACKEND PER STREAM (the state of the previous call lives in the backend): besides the start time and the
        length, a call must begin with exactly the samples of its predecessor's buffer to reuse anything - a backend shared between
        sessions (gateway._LockedBackend, two schedulers on one pipeline) therefore never forces tokens of other audio, it just
        decodes afresh - and ``reset()`` (what a scheduler's ``clear()`` should call) forgets the previous call.

        ``draft_previous_tick`` (round 6): the EXACT form of the same idea.  The previous call's tokens - all of them, no margin -
        are handed to the greedy loop as a DRAFT (tw_greedy_opts::n_draft): the engine runs prompt + draft through the decoder in
        batched launches WITH the logits and Whisper's logits processors of every position, keeps the draft up to the first
        position where its own arg-max differs, takes that arg-max, offers the rest of the draft again behind it and decodes
        step by step from where nothing more is confirmed.  The call returns what the plain backend returns - same ids, same
        word timestamps - whatever the draft was (a draft of other audio only costs time), so the eligibility test is a matter
        of speed, not of correctness.  ``reuse_stats`` counts drafted and confirmed tokens.  Not together with
        ``reuse_committed_prefix``.  Because the result is the plain call's, this is ON by default (``None`` = on unless
        ``reuse_committed_prefix`` was asked for); ``False`` gives the reference's behaviour literally - every tick decoded from
        scratch (R:thestage_speechkit/streaming/streaming_pipeline.py:388-435).

        ``token_scores`` (opt-in): every greedy call of a ``transcribe`` / ``transcribe_many`` is followed by a re-scoring pass
        (tw_score_tokens) and ``last_scores`` holds, for the most recent call, one entry per seek iteration of every chunk -
        ``{tokens, logprob, logprob_raw, avg_logprob, no_speech_prob}`` (shortform.score_entries).  The returned words are what
        they are with the option off: the scores travel beside them.

        ``temperature_fallback`` (opt-in; None | ``fallback.FallbackPolicy`` | a tuple of temperatures): Whisper's own repair of a
        segment that loops or hallucinates (HF ``generate_with_fallback``) instead of only dropping a looping tick in ``_to_tokens``:
        every seek iteration is measured (compression ratio, average log-probability, optionally the no-speech probability) and the
        chunks that fail are decoded again at the next temperature by the engine's sampler (fallback.py, ``shortform.Pass(fallback=)``).
        The call then ALWAYS runs the restated short-form loop; a backend whose call is not eligible for it (``job_codec()`` is None)
        raises ``ValueError`` rather than run without the option.  A draft (``draft_previous_tick``) applies to the first attempt only;
        not together with ``reuse_committed_prefix`` (a forced token is not redrawn).  ``last_fallback``: for the most recent call, one
        ``{temperature, attempts}`` per seek iteration of every chunk, with the policy's ``top_k`` / ``top_p`` beside them when it sets one
        (``FallbackPolicy(top_k=50)``: the sampled attempts draw from HF's candidate set).

        ``hotwords`` (opt-in; a list of phrases) with ``hotword_boost`` (required with it, no default; in NATURAL-LOG UNITS ON THE
        LOGITS: a boost of ``b`` multiplies a token's odds by ``exp(b)`` at the steps where it applies): the decoder is pushed towards
        the phrases by the on-device sequence bias (tw_generate_greedy_biased; ``hotwords.sequence_bias_for`` turns the phrases into
        sequences, every prefix of a phrase boosted once the tokens before it were produced).  ``set_hotwords(phrases, boost)`` changes
        the list between calls.  With hotwords set the call ALWAYS runs the restated short-form loop; a backend whose call is not
        eligible for it raises ``ValueError``.  ``draft_previous_tick`` stays on: the biased call returns the same ids whatever the
        draft.  Not together with ``temperature_fallback``, ``token_scores`` or ``reuse_committed_prefix``: the sampler and the
        re-scoring pass do not know the bias.

        ``repetition_penalty`` / ``no_repeat_ngram_size`` (opt-in; HF's generate options of those names, off by default): every decode of
        this backend applies them on the device (tw_generate_greedy_repeat, where the rule is stated: HF's two processors behind the
        sequence bias and ahead of Whisper's own).  They travel as generate options, so they are part of the learned short-form plan.
        ``draft_previous_tick`` stays on - the call returns the same ids whatever the draft - and hotwords go with them.  Not together
        with ``temperature_fallback`` or ``token_scores``: the sampler and the re-scoring pass do not know the rule.

        ``num_beams`` (opt-in; 2..8): every decode is a beam search on the device with word timestamps of the best hypothesis
        (tw_generate_beam_aligned; the model's ``beam_search`` and ``beam_token_timestamps`` are switched on and ``num_beams`` goes into
        the generate options).  One chunk takes ``num_beams`` engine rows: ``batch_size >= num_beams`` is needed.  The calls run HF's
        control flow around the engine call.  ``draft_previous_tick=None`` resolves to off (a draft does not go with beams), an explicit
        ``True`` raises ``ValueError``; hotwords, the repeat options, ``token_scores``, ``temperature_fallback`` and
        ``reuse_committed_prefix`` are refused by name.

        ``language=None`` (or ``"auto"``): the language of every chunk is detected on the device (tw_detect_language) by the pass that
        decodes it - the generate options carry ``language=None`` and the learned short-form plan has a language slot (model.py), so
        drafts, the temperature fallback, hotwords and token scores keep working.  ``last_language``: for the most recent call, one
        ``{"id", "code", "prob"}`` per chunk (the language token's id, the inner text of its ``<|xx|>`` token, the winner's probability -
        None for a chunk whose language was given).  ``sticky_language`` (default False): the first chunk's language of the first call
        after construction or ``reset()`` is stamped on every later chunk of the stream - a rolling buffer re-detected every 0.5 s can
        otherwise flip language mid-sentence.  ``language_id(code)`` resolves a two-letter code."""
        from .asr_pipeline import ASRPipeline

        self.num_beams: Optional[int] = None
        if num_beams is not None and (isinstance(num_beams, bool) or num_beams != 1):
            if isinstance(num_beams, bool) or int(num_beams) != num_beams or not 2 <= int(num_beams) <= 8:
                raise ValueError(f"num_beams must be an integer in 2..8 (or None / 1 for greedy), got {num_beams!r}")
            K = int(num_beams)
            for name, on in (("hotwords", hotwords is not None or hotword_boost is not None),
                             ("repetition_penalty", repetition_penalty is not None),
                             ("no_repeat_ngram_size", no_repeat_ngram_size is not None), ("token_scores", bool(token_scores)),
                             ("temperature_fallback", temperature_fallback is not None),
                             ("reuse_committed_prefix", bool(reuse_committed_prefix))):
                if on:
                    raise ValueError(f"num_beams={K} and {name} do not go together (the beam call takes none of these options)")
            if draft_previous_tick:
                raise ValueError(f"num_beams={K} and draft_previous_tick do not go together (a draft is verified against the greedy choice)")
            draft_previous_tick = False
            have = (asr_pipeline.model.engine.max_batch if asr_pipeline is not None else int(pipeline_kwargs.get("batch_size") or 1))
            if have < K:
                raise ValueError(f"num_beams={K} needs {K} engine rows per chunk, the pipeline holds {have}: construct it with batch_size={K} "
                                 "(or more, for several chunks per call)")
            self.num_beams = K
        if torch_dtype is None:
            # as the reference (R:...:369-370): float16 - a float16 context since round 4 (model.py: build_engine); bf16 before
            torch_dtype = torch.float16
        self.chunk_length_s: float = chunk_length_s
        self.sample_rate: int = 16000
        self.device: str = "cuda"  # ROCm exposes MI355X as "cuda", as on the nvidia platform (R:...:365)
        self.auto_language = language is None or language == "auto"
        self.language: Optional[str] = None if self.auto_language else language
        self.sticky_language = bool(sticky_language)
        self._sticky_id: Optional[int] = None     # sticky_language: the stream's language once its first chunk has been detected
        self._auto_route = self.auto_language     # transcribe() goes through the job codec (False while the codec learns, or cannot)
        self.last_language: List[Dict[str, Any]] = []
        self.asr_pipeline = asr_pipeline or ASRPipeline(
            model,
            model_size=model_size,
            chunk_length_s=chunk_length_s,
            torch_dtype=torch_dtype,
            device=pipeline_kwargs.pop("device", self.device),
            feature_extractor=feature_extractor,
            tokenizer=tokenizer,
            revision=revision,
            **pipeline_kwargs,
        )
        if self.num_beams is not None:
            self.asr_pipeline.model.beam_search = True
            self.asr_pipeline.model.beam_token_timestamps = True
        if draft_previous_tick is None:
            draft_previous_tick = not reuse_committed_prefix
        if reuse_committed_prefix and draft_previous_tick:
            raise ValueError("reuse_committed_prefix (approximate) and draft_previous_tick (exact) are alternatives")
        self.reuse_committed_prefix = bool(reuse_committed_prefix)
        self.draft_previous_tick = bool(draft_previous_tick)
        self.reuse_margin_s = float(reuse_margin_s)
        self.reuse_stats = {"calls": 0, "reused": 0, "forced_tokens": 0, "decoded_tokens": 0, "draft_tokens": 0, "confirmed_tokens": 0,
                            "verify_launches": 0}
        self._reuse_codec = None      # JobCodec (learned plan), built on the first reuse-enabled call
        self._last = None             # what the previous call left: start time, samples, first-iteration tokens + timestamps
        self._resample_kernel = resample_kernel   # tests: the numpy restatement in place of tw_resample (resample.py)
        self.token_scores = bool(token_scores)
        self.last_scores: List[Dict[str, Any]] = []
        from .fallback import as_policy

        self.temperature_fallback = as_policy(temperature_fallback)
        if self.temperature_fallback is not None and self.reuse_committed_prefix:
            raise ValueError("temperature_fallback and reuse_committed_prefix do not go together (a forced token is not redrawn)")
        self.last_fallback: List[Dict[str, Any]] = []
        self._no_speech_id: Any = False           # not looked up yet
        self.repetition_penalty: Optional[float] = None
        self.no_repeat_ngram_size: Optional[int] = None
        if repetition_penalty is not None:
            r = float(repetition_penalty)
            if not (r > 0.0 and r <= float(np.finfo(np.float32).max)):      # (NaN fails the comparison too)
                raise ValueError(f"repetition_penalty must be a finite float > 0, got {repetition_penalty!r}")
            self.repetition_penalty = r if r != 1.0 else None
        if no_repeat_ngram_size is not None:
            if isinstance(no_repeat_ngram_size, bool) or int(no_repeat_ngram_size) != no_repeat_ngram_size or int(no_repeat_ngram_size) < 0:
                raise ValueError(f"no_repeat_ngram_size must be an integer >= 0, got {no_repeat_ngram_size!r}")
            self.no_repeat_ngram_size = int(no_repeat_ngram_size) or None
        if self.repetition_penalty is not None or self.no_repeat_ngram_size is not None:
            for name in ("temperature_fallback", "token_scores"):
                if getattr(self, name, None):
                    raise ValueError(f"repetition_penalty / no_repeat_ngram_size and {name} do not go together (the sampler and the "
                                     "re-scoring pass do not know the rule)")
        self.hotwords: List[str] = []
        self.hotword_boost: Optional[float] = None
        self._hotword_bias: Optional[Dict[Any, float]] = None     # what every chunk of a call carries (shortform.ChunkWork.bias)
        if hotwords is not None or hotword_boost is not None:
            self.set_hotwords(hotwords, hotword_boost)

    def set_hotwords(self, phrases, boost: Optional[float]) -> None:
        """The phrases the decoder is pushed towards from the next call on, ``boost`` in natural-log units on the logits (see
        ``__init__``); ``set_hotwords(None, None)`` switches the option off."""
        phrases = [] if phrases is None else list(phrases)
        if not phrases:
            if boost is not None:
                raise ValueError("hotword_boost without hotwords")
            self.hotwords, self.hotword_boost, self._hotword_bias = [], None, None
            return
        if boost is None:
            raise ValueError("hotwords need hotword_boost (natural-log units on the logits; there is no default)")
        if getattr(self, "num_beams", None):
            raise ValueError(f"num_beams={self.num_beams} and hotwords do not go together (the beam call takes no sequence bias)")
        for name in ("temperature_fallback", "token_scores", "reuse_committed_prefix"):
            if getattr(self, name, None):
                raise ValueError(f"hotwords and {name} do not go together (the sampler and the re-scoring pass do not know the bias)")
        from .hotwords import sequence_bias_for

        tok = getattr(self.asr_pipeline, "tokenizer", None)
        if tok is None:
            raise ValueError("hotwords need the pipeline's tokenizer")
        self._hotword_bias = sequence_bias_for(tok, phrases, float(boost))
        self.hotwords, self.hotword_boost = phrases, float(boost)

    # -- languages ---------------------------------------------------------------------------------------------------------
    def language_id(self, code: str) -> int:
        """The token id of a two-letter language code (``generation_config.lang_to_id["<|xx|>"]``); ``ValueError`` for an unknown one."""
        table = getattr(getattr(self.asr_pipeline.model, "generation_config", None), "lang_to_id", None) or {}
        key = code if isinstance(code, str) and code.startswith("<|") else f"<|{code}|>"
        if key not in table:
            raise ValueError(f"unknown language code {code!r}")
        return int(table[key])

    def language_entry(self, token_id: Optional[int], prob: Optional[float] = None) -> Dict[str, Any]:
        """``{"id", "code", "prob"}`` of a language token: ``code`` is the inner text of the tokenizer's ``<|xx|>`` token."""
        if token_id is None:
            return {"id": None, "code": None, "prob": None}
        tok = getattr(self.asr_pipeline, "tokenizer", None)
        text = tok.convert_ids_to_tokens(int(token_id)) if tok is not None else None
        code = text[2:-2] if isinstance(text, str) and text.startswith("<|") and text.endswith("|>") else text
        return {"id": int(token_id), "code": code, "prob": None if prob is None else float(prob)}

    def to_engine_rate(self, audio, sample_rate: int):
        """``(audio, sample_rate)`` as the engine wants it: a buffer at another rate (or int16 / multi-channel) goes through
        ``tw_resample`` first (resample.py; the reference does this with librosa before its backend is called,
        R:thestage_speechkit/streaming/streams.py:103-105).  16 kHz buffers pass untouched.  A buffer that grew is resampled from
        its first frame again, so the previous result is a prefix of the new one up to the filter's reach: drafts keep matching."""
        if int(sample_rate) == self.sample_rate:
            return audio, self.sample_rate
        from .resample import resample

        return resample(audio, int(sample_rate), self.sample_rate, kernel=self._resample_kernel), self.sample_rate

    def _generate_kwargs(self) -> Dict[str, Any]:
        kw = {"use_cache": True, "num_beams": self.num_beams or 1, "do_sample": False, "max_new_tokens": 128, "language": self.language}
        if self.repetition_penalty is not None:
            kw["repetition_penalty"] = self.repetition_penalty
        if self.no_repeat_ngram_size is not None:
            kw["no_repeat_ngram_size"] = self.no_repeat_ngram_size
        return kw

    @property
    def no_speech_id(self) -> Optional[int]:
        """Id of ``<|nospeech|>`` (``<|nocaptions|>`` on older vocabularies) in the pipeline's tokenizer, or None."""
        if self._no_speech_id is False:
            tok = getattr(self.asr_pipeline, "tokenizer", None)
            found = None
            for name in ("<|nospeech|>", "<|nocaptions|>"):
                try:
                    i = tok.convert_tokens_to_ids(name)
                    if i is not None and int(i) >= 0 and tok.convert_ids_to_tokens(int(i)) == name:
                        found = int(i)
                        break
                except Exception:  # noqa: BLE001 - no tokenizer, or one without the token
                    continue
            self._no_speech_id = found
        return self._no_speech_id

    def _run_pipeline(self, *args, **kwargs):
        """``self.asr_pipeline(...)``; with ``token_scores`` the model object scores every greedy call it makes meanwhile."""
        model = getattr(self.asr_pipeline, "model", None)
        if not self.token_scores or model is None:
            return self.asr_pipeline(*args, **kwargs)
        entries: List[Dict[str, Any]] = []
        model.score_sink = {"entries": entries, "no_speech_id": self.no_speech_id}
        try:
            return self.asr_pipeline(*args, **kwargs)
        finally:
            model.score_sink = None
            self.last_scores = entries

    def transcribe(self, audio: np.ndarray, buffer_start_time: float, sample_rate: int, language: Optional[str] = None) -> List[Dict[str, Any]]:
        """``language`` (a two-letter code; an auto-language backend only): this request's own language - nothing is detected."""
        if language is not None and not self._auto_route:
            if language != self.language:
                raise ValueError(f"this backend serves language '{self.language}' (the engine is built for one language prompt)")
            language = None
        audio, sample_rate = self.to_engine_rate(audio, sample_rate)
        if (self.reuse_committed_prefix or self.draft_previous_tick or self.temperature_fallback is not None or self._hotword_bias
                or self._auto_route):
            words = self._transcribe_with_reuse(np.asarray(audio), float(buffer_start_time), int(sample_rate), language)
            if words is not None:
                return words
            if language is not None:
                raise ValueError("a per-request language needs the restated short-form loop, and this backend's call is not eligible "
                                 "for it (job_codec() is None)")
            if self._hotword_bias:
                raise ValueError("hotwords need the restated short-form loop, and this backend's call is not eligible for it "
                                 "(job_codec() is None)")
            if self.temperature_fallback is not None:
                raise ValueError("temperature_fallback needs the restated short-form loop, and this backend's call is not eligible for it "
                                 "(job_codec() is None)")
        result: Dict[str, Any] = self._run_pipeline(
            audio,
            return_timestamps="word",
            generate_kwargs=self._generate_kwargs(),
            chunk_length_s=self.chunk_length_s,
        )
        if self.auto_language:     # HF's control flow around the engine: what the model object detected last
            model = getattr(self.asr_pipeline, "model", None)
            self.last_language = [self.language_entry(i) for i in (getattr(model, "last_languages", None) or [])]
        return self._to_tokens(result, len(audio) / sample_rate, buffer_start_time)

    # -- decoder-side reuse between the ticks of one stream (opt-in) -------------------------------
    def reset(self) -> None:
        """Forget the previous call (``reuse_committed_prefix``): the next buffer is decoded afresh.  For the owner of the stream to
        call when its scheduler restarts at t = 0 (R:thestage_speechkit/streaming/streaming_pipeline.py:953-976 ``clear``)."""
        self._last = None
        self._sticky_id = None      # sticky_language: the next call detects again

    def _forced_prefix(self, audio: np.ndarray, buffer_start_time: float, sample_rate: int) -> Optional[np.ndarray]:
        """Tokens of the previous call that may be forced in this one, or None.  Eligible: same buffer start, buffer not shorter
        (the scheduler appended audio; a trimmed buffer starts elsewhere and is decoded afresh).  Kept: the longest prefix whose
        token timestamps (DTW, seconds from the buffer start) end ``reuse_margin_s`` before the OLD buffer's end - the audio
        behind them has had its right context for at least that long."""
        last = self._last
        n_samples = len(audio)
        if last is None or abs(last["start"] - buffer_start_time) > 1e-6 or n_samples < last["n_samples"] or last["sr"] != sample_rate:
            return None
        # ... and it must BE the previous buffer plus new audio: same start and length alone also match another session's buffer or
        # a restarted stream (0.64 MB compared per 10 s: ~0.1 ms)
        prev = last["audio"]
        if audio.dtype != prev.dtype or not np.array_equal(audio[: len(prev)], prev):
            return None
        ids, ts = last["ids"], last["ts"]
        if ids is None or len(ids) == 0:
            return None
        if self.draft_previous_tick:      # exact whatever is offered: everything the previous call produced
            return np.asarray(ids, dtype=np.int32)
        if ts is None:
            return None
        limit = last["n_samples"] / sample_rate - self.reuse_margin_s
        keep = 0
        for i in range(len(ids)):
            if ts[i] > limit:
                break
            keep = i + 1
        if keep < 2:
            return None
        return np.asarray(ids[:keep], dtype=np.int32)

    def _transcribe_with_reuse(self, audio: np.ndarray, buffer_start_time: float, sample_rate: int, language: Optional[str] = None):
        """The call through the restated short-form loop (shortform.py) with a forced prefix on the first seek iteration; None
        when this backend cannot (no learned plan, a buffer longer than one chunk): the ordinary call then runs."""
        from . import shortform

        if self._reuse_codec is None:
            codec = self.job_codec()
            if codec is None or not codec.learn():        # (the plan is learned from one ORDINARY call of this backend: JobCodec.learn)
                self.reuse_committed_prefix = self.draft_previous_tick = False
                self._auto_route = False                  # (an auto backend then detects inside HF's generate, call by call)
                return None                               # not eligible on this pipeline: stays the plain backend
            self._reuse_codec = codec
        codec = self._reuse_codec
        self.reuse_stats["calls"] += 1
        # (the hotword bias travels on the works: JobCodec.open; so does a request's own language)
        job = codec.open(audio, buffer_start_time, sample_rate) if language is None else codec.open(audio, buffer_start_time, sample_rate, language=language)
        eng = self.asr_pipeline.model.engine
        if len(job.works) != 1:
            self._last = None
            forced = None
        elif not (self.reuse_committed_prefix or self.draft_previous_tick):     # (here for temperature_fallback alone)
            forced = None
        else:
            forced = self._forced_prefix(audio, buffer_start_time, sample_rate)
            budget = int(codec.plan.greedy.get("max_new_tokens", 128))
            if forced is not None and len(forced) >= budget - 1:
                forced = forced[: max(0, budget - 2)]
            if forced is not None and self.draft_previous_tick:
                if len(forced) >= 1:
                    job.works[0].draft = forced
                    self.reuse_stats["reused"] += 1
                    self.reuse_stats["draft_tokens"] += int(len(forced))
                forced = None
            elif forced is not None and len(forced) >= 2:
                job.works[0].forced = forced
                self.reuse_stats["reused"] += 1
                self.reuse_stats["forced_tokens"] += int(len(forced))
        while not job.done:
            for w in [w for w in job.works if not w.done]:
                shortform.run_pass(eng, codec.plan, [w], score=codec.score, no_speech_id=codec.no_speech_id, fallback=codec.fallback)
                if self.sticky_language and self._sticky_id is None and job.works[0].language is not None:
                    self._sticky_id = int(job.works[0].language)      # the stream's first chunk: every later chunk carries it
                    for later in job.works[1:]:
                        if later.language is None:
                            later.language = self._sticky_id
                if w.passes > shortform.MAX_SEEK_PASSES:
                    raise RuntimeError(f"a chunk needed more than {shortform.MAX_SEEK_PASSES} seek passes")
        if len(job.works) == 1 and job.works[0].first_pass is not None and (self.reuse_committed_prefix or self.draft_previous_tick):
            ids, ts = job.works[0].first_pass
            dr = job.works[0].draft_result
            if dr is not None:
                self.reuse_stats["confirmed_tokens"] += int(dr["accepted"])
                self.reuse_stats["verify_launches"] += int(dr["launches"])
            self.reuse_stats["decoded_tokens"] += int(len(ids)) - (int(len(forced)) if forced is not None else 0) - (int(dr["accepted"]) if dr else 0)
            self._last = {"start": buffer_start_time, "n_samples": len(audio), "sr": sample_rate, "ids": ids, "ts": ts,
                          "audio": np.array(audio, copy=True)}
        words = codec.close(job)
        if self.token_scores:
            self.last_scores = job.scores
        self.last_fallback = job.fallback
        self.last_language = job.language
        return words

    def transcribe_many(self, requests, batch_size: Optional[int] = None) -> List[List[Dict[str, Any]]]:
        """Several streams' rolling buffers in ONE pipeline call: [(audio, buffer_start_time, sample_rate), ...].
        HF collates the chunks of different buffers into batched engine calls; per-stream results are unchanged."""
        if self.temperature_fallback is not None or self._hotword_bias or self._auto_route:      # (HF's batched call knows nothing of the options: one short-form call per request)
            out, log, langs = [], [], []
            for a, t0, sr in requests:
                out.append(self.transcribe(a, t0, sr))
                log.extend(self.last_fallback)
                langs.extend(self.last_language)
            self.last_fallback = log
            self.last_language = langs
            return out
        requests = [(self.to_engine_rate(a, sr)[0], t0, self.sample_rate) for a, t0, sr in requests]
        audios = [np.asarray(a) for a, _, _ in requests]
        kw = {} if batch_size is None else {"batch_size": int(batch_size)}
        results = self._run_pipeline(
            audios, return_timestamps="word", generate_kwargs=self._generate_kwargs(), chunk_length_s=self.chunk_length_s, **kw
        )
        return [self._to_tokens(res, len(a) / sr, t0) for res, (a, t0, sr) in zip(results, requests)]

    def job_codec(self) -> "Optional[JobCodec]":
        """Per-request pre/post-processing around ``shortform.run_pass`` (what ``serving.BatchingHub`` schedules), or None
        when this backend's call cannot run the restated short-form loop (it then serves whole-call batches)."""
        if self.num_beams is not None:
            return None       # beam calls run HF's control flow (model._plan_key is None for them)
        try:
            return JobCodec(self)
        except _NotEligible:
            return None

    @staticmethod
    def _to_tokens(result: Dict[str, Any], audio_duration: float, buffer_start_time: float) -> List[Dict[str, Any]]:
        if _compression_ratio(result["text"]) > 2.2:
            return []
        generated_tokens: List[Dict[str, Any]] = []
        max_word_duration: float = 1.0
        for token in result["chunks"]:
            if token["timestamp"][1] is None:
                if audio_duration - token["timestamp"][0] < max_word_duration:
                    token["timestamp"] = (token["timestamp"][0], audio_duration)
                else:
                    token["timestamp"] = (token["timestamp"][0], token["timestamp"][0] + max_word_duration)
            generated_tokens.append(
                {
                    "text": token["text"],
                    "start": token["timestamp"][0] + buffer_start_time,
                    "end": token["timestamp"][1] + buffer_start_time,
                }
            )
        return generated_tokens


class _NotEligible(Exception):
    pass


class BufferJob:
    """One ``transcribe`` request on its way through the hub: its chunks' decoding states and what post-processing needs."""

    __slots__ = ("works", "meta", "audio_duration", "buffer_start_time", "future", "t_submit", "scores", "fallback", "language")

    def __init__(self, works, meta, audio_duration, buffer_start_time):
        self.works = works                        # [shortform.ChunkWork] - one per <= chunk_length_s piece of the buffer
        self.meta = meta                          # [(is_last, stride)] as HF's chunk iterator produced them
        self.audio_duration = audio_duration
        self.buffer_start_time = buffer_start_time
        self.future = None
        self.t_submit = 0.0
        self.scores: List[Dict[str, Any]] = []     # JobCodec.close: the chunks' score entries when the backend asked for them
        self.fallback: List[Dict[str, Any]] = []   # JobCodec.close: {temperature, attempts} per seek iteration (temperature_fallback)
        self.language: List[Dict[str, Any]] = []   # JobCodec.close: {id, code, prob} per chunk (a plan with a language slot)

    @property
    def done(self) -> bool:
        return all(w.done for w in self.works)


class JobCodec:
    """Splits ``AMDWhisperBackend.transcribe`` into the three stages HF's pipeline runs per call - ``preprocess`` (chunking +
    log-mel), the model, ``postprocess`` (tokenizer state machine, word timestamps, LCS merge) - so that a scheduler can put
    the model stage of MANY requests into shared passes (``shortform.run_pass``).  Stages 1 and 3 are HF's own methods on
    the backend's pipeline object, called with exactly the parameters ``pipeline.__call__`` would derive; the model stage's
    output dictionaries have the shape HF's un-batching hands to ``postprocess`` for a batch of one."""

    def __init__(self, backend: AMDWhisperBackend):
        pipe = backend.asr_pipeline
        model = getattr(pipe, "model", None)
        if model is None or not hasattr(model, "last_plan") or not hasattr(pipe, "_sanitize_parameters"):
            raise _NotEligible()
        self.backend = backend
        self.pipe = pipe
        pre, _fwd, post = pipe._sanitize_parameters(return_timestamps="word", generate_kwargs=backend._generate_kwargs(),
                                                     chunk_length_s=backend.chunk_length_s)
        self.pre = {**pipe._preprocess_params, **pre}
        self.post = {**pipe._postprocess_params, **post}
        self.plan = None
        # AMDWhisperBackend(token_scores=True): whoever runs this codec's jobs builds its passes with Pass(score=..., no_speech_id=...)
        self.score = bool(getattr(backend, "token_scores", False))
        # AMDWhisperBackend(temperature_fallback=...): ... and with Pass(fallback=...); chunk i of a request draws with seed policy.seed + i
        self.fallback = getattr(backend, "temperature_fallback", None)
        needs_ns = self.score or (self.fallback is not None and self.fallback.no_speech_threshold is not None)
        self.no_speech_id = backend.no_speech_id if needs_ns else None

    def learn(self) -> bool:
        """One short request through the ordinary pipeline call: HF's ``generate`` runs once with this backend's options and
        the model object records the short-form plan (model.py).  False if the call turned out not to be eligible."""
        model = self.pipe.model
        model.last_plan = None
        b = self.backend
        mode = (b.reuse_committed_prefix, b.draft_previous_tick)     # (the ORDINARY call: the reuse / draft paths bypass HF's generate)
        auto = getattr(b, "_auto_route", False)                      # (... and an auto-language backend's route through this codec)
        b._auto_route = False
        policy = getattr(b, "temperature_fallback", None)            # (... and so does the temperature fallback)
        bias = getattr(b, "_hotword_bias", None)                     # (... and the hotword bias: a per-chunk list, not part of the plan)
        b.reuse_committed_prefix = b.draft_previous_tick = False
        b.temperature_fallback = None
        b._hotword_bias = None
        try:
            b.transcribe(np.zeros(b.sample_rate, dtype=np.float32), 0.0, b.sample_rate)
        finally:
            b.reuse_committed_prefix, b.draft_previous_tick = mode
            b.temperature_fallback = policy
            b._hotword_bias = bias
            b._auto_route = auto
        plan = model.last_plan
        if plan is None or not plan.return_token_timestamps or not plan.return_segments:
            return False
        self.plan = plan
        return True

    def open(self, audio: np.ndarray, buffer_start_time: float, sample_rate: int, language: Optional[str] = None) -> BufferJob:
        """Stage 1 (HF:pipelines/automatic_speech_recognition.py:346-482 via ``pipe.preprocess``).  ``language`` (a two-letter code; a
        plan with a language slot only): the request's own language - its chunks are not detected.  None: the backend's sticky language
        if it has one, else every chunk is detected by the pass that decodes it first."""
        from .shortform import ChunkWork

        lang_id = None
        if getattr(self.plan, "lang_slot", None) is not None:
            if language is not None:
                lang_id = self.backend.language_id(language)
            elif getattr(self.backend, "sticky_language", False):
                lang_id = self.backend._sticky_id
        elif language is not None and language != getattr(self.backend, "language", None):
            raise ValueError(f"this backend serves language '{getattr(self.backend, 'language', None)}' (the engine is built for one language prompt)")

        audio, sample_rate = self.backend.to_engine_rate(audio, sample_rate)
        audio = np.asarray(audio)
        works, meta = [], []
        for item in self.pipe.preprocess(audio, **self.pre):
            feats = item["input_features"]
            am = item.get("attention_mask")
            nf = int(am.sum()) if am is not None else None
            works.append(ChunkWork(feats[0], nf))
            works[-1].chunk_index = len(works) - 1
            # AMDWhisperBackend(hotwords=...): every chunk carries the backend's list, whoever builds the passes (this backend's own
            # loop or a hub that opens the jobs itself); read per job, so set_hotwords takes effect from the next buffer on
            works[-1].bias = getattr(self.backend, "_hotword_bias", None)
            works[-1].language = lang_id
            meta.append((item["is_last"], item.get("stride")))
        if not works:
            raise ValueError("empty audio buffer")
        return BufferJob(works, meta, len(audio) / sample_rate, buffer_start_time)

    def close(self, job: BufferJob) -> List[Dict[str, Any]]:
        """Stage 3 (``pipe.postprocess`` + the reference backend's word fix-ups, R:...:412-433)."""
        from .shortform import work_tokens

        outs = []
        for w, (is_last, stride) in zip(job.works, job.meta):
            seq, _raw, seg = work_tokens(self.plan, w)
            o = {"is_last": is_last, "tokens": seq.unsqueeze(0), "token_timestamps": seg.unsqueeze(0)}
            if stride is not None:
                o["stride"] = stride
            outs.append(o)
        job.scores = [e for w in job.works for e in w.scores]
        # (a policy that filters the candidate set: its top_k / top_p beside every entry)
        pol = self.fallback
        flt = {"top_k": pol.top_k, "top_p": pol.top_p} if pol is not None and (pol.top_k is not None or pol.top_p is not None) else {}
        job.fallback = [{"temperature": t, "attempts": a, **flt} for w in job.works for t, a in zip(w.temperatures, w.attempts)]
        if getattr(self.plan, "lang_slot", None) is not None:
            ids = self.plan.lang_ids
            job.language = [self.backend.language_entry(w.language, None if w.language_probs is None or w.language not in ids
                                                        else w.language_probs[ids.index(w.language)]) for w in job.works]
            if getattr(self.backend, "sticky_language", False) and self.backend._sticky_id is None and job.works[0].language is not None:
                self.backend._sticky_id = int(job.works[0].language)
        result = self.pipe.postprocess(outs, **self.post)
        return AMDWhisperBackend._to_tokens(result, job.audio_duration, job.buffer_start_time)
