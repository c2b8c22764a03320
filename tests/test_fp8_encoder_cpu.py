"""TW_F16_W8A16_FULL without a GPU: the enum value, the plan of its GEMMs (host arithmetic) and the pipeline option that selects it."""
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests.oracle_engine import oracle_engine_factory


def test_enum_and_plan(built_library):
    from thewhisper_amd import _cabi

    assert _cabi.TW_F16_W8A16_FULL == 6
    # kernel 3; 80 x 256 tiles where the 16-bit weights get bm x 256 tiles, 64 x 128 below: one stream, 16 x 10 s (large-v3: fc2, QKV, cross K|V)
    assert _cabi.gemm_plan(_cabi.TW_F16_W8A16_FULL, _cabi.TW_EPI_ROWMAJOR, 500, 1280, 5120) == (3, 64)
    assert _cabi.gemm_plan(_cabi.TW_F16_W8A16_FULL, _cabi.TW_EPI_QKV_ENC, 8000, 3840, 1280) == (3, 80)
    assert _cabi.gemm_plan(_cabi.TW_F16_W8A16_FULL, _cabi.TW_EPI_KV_CROSS, 8000, 2560, 1280) == (3, 80)
    with pytest.raises(RuntimeError):
        _cabi.gemm_plan(_cabi.TW_F16_W8A16_FULL, _cabi.TW_EPI_ROWMAJOR, 500, 1280, 64)      # K is no multiple of 128


def selected(dtype, **opts):
    """the engine dtype string a pipeline built with these options asks its engine factory for"""
    from thewhisper_amd import ASRPipeline

    seen, dims = [], wo.PRESETS["micro"]

    def factory(dims, T, max_batch, eng_dtype, alignment_heads, device_index):
        seen.append(eng_dtype)
        return oracle_engine_factory(dims, T, max_batch, "f32", alignment_heads, device_index)

    ASRPipeline(hr.build_hf_model(dims, wo.make_weights(dims, 0)), feature_extractor=hr.build_feature_extractor(dims, 10),
                tokenizer=hr.build_tokenizer(dims), chunk_length_s=10, device="cpu", torch_dtype=dtype, engine_factory=factory, **opts)
    return seen


def test_encoder_weights_selects_the_dtype():
    assert selected(torch.float16) == ["f16"]
    assert selected(torch.float16, decoder_weights="fp8") == ["fp8f16"]
    assert selected(torch.float16, decoder_weights="fp8", encoder_weights="fp8") == ["fp8f16full"]


@pytest.mark.parametrize("dtype,opts", [(torch.float16, dict(encoder_weights="fp8")),
                                        (torch.bfloat16, dict(decoder_weights="fp8", encoder_weights="fp8")),
                                        (torch.float32, dict(decoder_weights="bf16", encoder_weights="fp8")),
                                        (torch.float16, dict(decoder_weights="fp8", encoder_weights="int4"))])
def test_invalid_combinations_raise(dtype, opts):
    with pytest.raises(ValueError, match="encoder_weights"):
        selected(dtype, **opts)
