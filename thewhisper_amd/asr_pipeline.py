"""``thewhisper_amd.ASRPipeline`` - the MI355X sibling of ``thestage_speechkit.nvidia.ASRPipeline``.

Mirrors R:thestage_speechkit/nvidia/asr_pipeline.py:30-92 argument for argument (same constructor
names and meaning, same ValueErrors, same call contract): a subclass of HF's
``AutomaticSpeechRecognitionPipeline`` (chunking, batching and the stride-aware LCS merge stay on
the host, exactly as in the reference), with the model object replaced by
``AMDWhisperForConditionalGeneration`` and the feature extractor by ``AMDWhisperFeatureExtractor``.
"""
from __future__ import annotations

import os
from typing import Callable, Optional, Union

import torch
from transformers import (
    AutomaticSpeechRecognitionPipeline,
    PreTrainedTokenizer,
    SequenceFeatureExtractor,
    WhisperFeatureExtractor,
    WhisperTokenizer,
)
from transformers import WhisperForConditionalGeneration as HFWhisperForConditionalGeneration

from . import lcs_patch  # noqa: F401  (installs the reference's chunk-merge fix, R:thestage_speechkit/__init__.py:137-139)
from .feature_extraction import AMDWhisperFeatureExtractor
from .model import AMDWhisperForConditionalGeneration
from .tokenizer_cache import cache_special_ids


class ASRPipeline(AutomaticSpeechRecognitionPipeline):
    def __init__(
        self,
        model: Union[str, HFWhisperForConditionalGeneration],
        feature_extractor: Optional[SequenceFeatureExtractor] = None,
        tokenizer: Optional[PreTrainedTokenizer] = None,
        model_size: str = None,
        chunk_length_s: int = 30,
        device: str = "cuda",
        torch_dtype: Optional[torch.dtype] = None,
        **kwargs,
    ):
        revision = kwargs.pop("revision", "main")
        # THEWHISPER_DEVICE overrides a plain "cuda" (the reference's streaming backend hard-codes device="cuda" for GPU
        # platforms, R:thestage_speechkit/streaming/streaming_pipeline.py:365): pick one MI355X of the node ("cuda:3"), or
        # "cpu" together with an injected engine factory in the GPU-less tests of the host glue
        if device == "cuda" and os.environ.get("THEWHISPER_DEVICE"):
            device = os.environ["THEWHISPER_DEVICE"]
        engine_factory: Optional[Callable] = kwargs.pop("engine_factory", None)  # test seam only
        decoder_weights: Optional[str] = kwargs.pop("decoder_weights", None)     # MI355X-only option: "fp8" = MXFP8 decoder weights
        encoder_weights: Optional[str] = kwargs.pop("encoder_weights", None)     # MI355X-only option: "fp8" with decoder_weights="fp8" and float16
        shared_engine = kwargs.pop("engine", None)  # MI355X-only option: an already loaded WhisperEngine (shared context)
        if model_size not in (None, "S", "M", "L", "XL"):
            raise ValueError(f"Invalid model_size: {model_size}")
        # model_size selects a TheStage engine flavour on NVIDIA (S = quantised, XL = fp16).  On MI355X every size maps to the
        # bf16 kernels (results identical to the reference arithmetic within the bf16 tolerance); the quantised flavour is an
        # explicit opt-in, ``decoder_weights="fp8"`` (BASELINE config 5: MXFP8 decoder projection weights) - or, for callers
        # that cannot change their code, the deployment switch THEWHISPER_SIZE_S=fp8, which gives model_size="S" that meaning.
        if decoder_weights not in (None, "bf16", "fp8"):
            raise ValueError(f"Invalid decoder_weights: {decoder_weights}")
        if decoder_weights is None and model_size == "S" and os.environ.get("THEWHISPER_SIZE_S", "").lower() == "fp8":
            decoder_weights = "fp8"

        if type(model) is str:
            model_name = model
            model = AMDWhisperForConditionalGeneration.from_pretrained(model_name, torch_dtype=torch_dtype, revision=revision)
            if feature_extractor is None:
                feature_extractor = WhisperFeatureExtractor.from_pretrained(
                    model_name, torch_dtype=torch_dtype, chunk_length=chunk_length_s
                )
            if tokenizer is None:
                tokenizer = WhisperTokenizer.from_pretrained(model_name, torch_dtype=torch_dtype)
        else:
            if feature_extractor is None:
                raise ValueError("feature_extractor must be provided when passing a model instance")
            if tokenizer is None:
                raise ValueError("tokenizer must be provided when passing a model instance")
            model = AMDWhisperForConditionalGeneration.from_hf(model)

        feature_extractor = AMDWhisperFeatureExtractor.from_hf(feature_extractor)
        tokenizer = cache_special_ids(tokenizer)   # host-side post-processing cost only; values unchanged
        if feature_extractor.chunk_length != chunk_length_s:
            raise ValueError(
                f"feature_extractor.chunk_length={feature_extractor.chunk_length} must equal chunk_length_s={chunk_length_s}: "
                "the encoder sees exactly 50*chunk_length_s frames"
            )

        super().__init__(
            model,
            feature_extractor=feature_extractor,
            tokenizer=tokenizer,
            device=device,
            chunk_length_s=chunk_length_s,
            torch_dtype=torch_dtype,
            **kwargs,
        )
        # A0 (patch_hf_model) happens inside the library when the engine is built for T = 50*chunk_length_s.
        batch_size = int(kwargs.get("batch_size") or 1)
        if shared_engine is not None:
            if shared_engine.T != int(1500 * (chunk_length_s / 30)):
                raise ValueError(f"engine was built for {shared_engine.T} encoder frames, chunk_length_s={chunk_length_s} needs "
                                 f"{int(1500 * (chunk_length_s / 30))}")
            if batch_size > shared_engine.max_batch:
                raise ValueError(f"batch_size={batch_size} exceeds the engine capacity max_batch={shared_engine.max_batch}")
            self.feature_extractor.attach_engine(self.model.attach_engine(shared_engine))
            return
        engine = self.model.build_engine(
            chunk_length_s=chunk_length_s, max_batch=max(1, min(64, batch_size)), dtype=torch_dtype,
            engine_factory=engine_factory, decoder_weights=decoder_weights, encoder_weights=encoder_weights,
        )
        self.feature_extractor.attach_engine(engine)
