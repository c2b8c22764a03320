"""The resampling front end without a GPU: the numpy restatement (tests/resample_ref.py) against SciPy, the library's plan and
taps against the restatement, argument checks of the C ABI, the streaming state machine on the restatement as its kernel, and
the gateway's opt-in routes with a fake backend."""
import base64
import ctypes as C
import io
import wave

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import resample_ref as rr

RATES = rr.RATES


def _signals(sr, seed):
    rng = np.random.default_rng(seed)
    imp = np.zeros(777, np.float32)
    imp[300] = 1.0
    return {
        "noise": rng.standard_normal(sr // 3 + 17).astype(np.float32),
        "speechlike": wo.synth_audio(sr // 2 + 5, seed, "speechlike").astype(np.float32),
        "impulse": imp,
        "one": np.array([0.75], np.float32),
        "none": np.zeros(0, np.float32),
    }


@pytest.mark.parametrize("sr", RATES)
def test_restatement_equals_scipy_resample_poly(sr):
    ss = pytest.importorskip("scipy.signal")
    L, M, half, tpo = rr.plan(sr)
    h = rr.taps(sr)
    assert len(h) == 2 * half + 1 and tpo == 2 * half // L + 1
    for name, x in _signals(sr, sr % 97).items():
        y = rr.resample(x, sr)
        assert y.dtype == np.float64 and len(y) == -((-len(x) * L) // M), name
        if len(x) == 0:
            continue      # (scipy refuses an empty input; the length is what the definition says: 0)
        z = ss.resample_poly(x.astype(np.float64), L, M, window=h / L)
        assert len(z) == len(y), (name, len(z), len(y))
        err = np.abs(y - z).max()
        print(f"{sr} Hz {name}: max |restatement - scipy| = {err:.3g}")
        assert err <= 1e-12, (name, err)


def test_taps_per_output_of_the_common_rates():
    assert rr.plan(8000)[3] == 33 and rr.plan(44100)[3] == 89 and rr.plan(48000)[3] == 97
    assert [len(rr.taps(sr)) for sr in (48000, 44100, 11025)] == [97, 14113, 20481]


@pytest.mark.parametrize("sr", RATES + (16000,))
def test_library_plan_and_taps_equal_the_restatement(sr, built_library):
    from thewhisper_amd import _cabi

    lib = _cabi.load_library()
    v = [C.c_int32() for _ in range(4)]
    assert lib.tw_resample_plan(sr, 16000, *[C.byref(x) for x in v]) == 0
    assert tuple(x.value for x in v) == rr.plan(sr)
    want = rr.taps(sr)
    got = np.zeros(len(want), np.float64)
    assert lib.tw_resample_taps(sr, 16000, got.ctypes.data_as(C.POINTER(C.c_double)), len(got)) == 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert lib.tw_resample_taps(sr, 16000, got.ctypes.data_as(C.POINTER(C.c_double)), len(got) + 1) == _cabi_einval()
    # the Python wrapper hands out the same
    from thewhisper_amd import resample as rs

    assert rs.plan(sr) == rr.plan(sr) and np.array_equal(rs.taps(sr), got)


def _cabi_einval():
    return -1      # TW_EINVAL (include/thewhisper.h)


def test_unsupported_and_malformed_requests_return_einval_with_a_message(built_library):
    from thewhisper_amd import _cabi

    lib = _cabi.load_library()
    v = [C.c_int32() for _ in range(4)]
    for bad in (0, 16001, -48000, 3999):
        assert lib.tw_resample_plan(bad, 16000, *[C.byref(x) for x in v]) == _cabi_einval()
        assert str(bad).lstrip("-") in lib.tw_last_error(None).decode()
        assert lib.tw_resample_taps(bad, 16000, (C.c_double * 4)(), 4) == _cabi_einval()
    assert b"table" in lib.tw_last_error(None) or b"4000" in lib.tw_last_error(None)
    assert lib.tw_resample_plan(16001, 16000, None, None, None, None) == _cabi_einval() and b"taps" in lib.tw_last_error(None)
    assert lib.tw_resample_plan(48000, 16000, None, None, None, None) == 0          # (any out pointer may be NULL)

    # tw_resample: the argument checks come before anything touches a device, so they answer the same with and without one
    buf = (C.c_float * 64)()
    first, count, ofirst = (C.c_int64 * 65)(), (C.c_int32 * 65)(*([16] * 65)), (C.c_int64 * 65)()
    p = C.cast(buf, C.c_void_p)

    def call(in_dev=p, fmt=0, channels=1, stride=16, in_first=first, in_count=count, sr_in=48000, sr_out=16000, out_first=ofirst,
             n_out=4, out_dev=p, out_stride=4, B=1):
        rc = lib.tw_resample(0, in_dev, fmt, channels, stride, in_first, in_count, sr_in, sr_out, out_first, n_out, out_dev, out_stride, B, None)
        return rc, lib.tw_last_error(None).decode()

    for kw, word in ((dict(sr_in=0), "4000"), (dict(sr_in=16001), "taps"), (dict(channels=9), "channels"), (dict(channels=0), "channels"),
                     (dict(B=65), "B=65"), (dict(B=0), "B=0"), (dict(n_out=0), "n_out"), (dict(in_dev=None), "null"),
                     (dict(out_dev=None), "null"), (dict(in_first=None), "null"), (dict(in_count=None), "null"),
                     (dict(out_first=None), "null"), (dict(fmt=2), "in_fmt"), (dict(out_stride=3), "stride"),
                     (dict(in_count=(C.c_int32 * 1)(17)), "in_count"), (dict(in_count=(C.c_int32 * 1)(-1)), "in_count"),
                     (dict(out_first=(C.c_int64 * 1)(-1)), "out_first")):
        rc, msg = call(**kw)
        assert rc == _cabi_einval() and word in msg, (kw, rc, msg)
    if not torch.cuda.is_available():
        rc, msg = call()
        assert rc < 0 and "no HIP device" in msg
        from thewhisper_amd.resample import resample

        with pytest.raises(RuntimeError, match="no CPU fallback"):
            resample(np.zeros(480, np.float32), 48000)
    from thewhisper_amd import resample as rs

    for bad in (0, 16001):
        with pytest.raises(ValueError, match="unsupported sample rate"):
            rs.plan(bad)
    with pytest.raises(ValueError):
        rs.StreamResampler(48000, channels=9, kernel=rr.rows)
    with pytest.raises(ValueError):
        rs.StreamResampler(48000, fmt="mulaw", kernel=rr.rows)
    with pytest.raises(ValueError):
        rs.BatchedResampler(65, 48000, kernel=rr.rows)


def _cuts(n, sr, seed):
    rng = np.random.default_rng(seed)
    out = {}
    for name, size in (("1", 1), ("7", 7), ("160", 160), ("4410", 4410), ("half_second", sr // 2)):
        out[name] = [size] * (n // size + 1)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(0, 3000)))
    out["random"] = sizes
    return out


@pytest.mark.parametrize("sr", (8000, 44100, 48000))
def test_stream_resampler_equals_one_shot_however_the_input_is_cut(sr, built_library):
    from thewhisper_amd.resample import StreamResampler, resample

    n = sr + 123 if sr > 8000 else 4000 + 77       # (size-1 pushes are one kernel call each: keep that case short)
    x = wo.synth_audio(n, 3, "speechlike").astype(np.float32)
    L, M, half, _ = rr.plan(sr)
    one = resample(x, sr, kernel=rr.rows)
    assert one.dtype == np.float32 and np.array_equal(one, rr.resample(x, sr, dtype=np.float32))
    assert len(one) == -((-n * L) // M)
    for name, sizes in _cuts(n, sr, sr).items():
        xs = x if name != "1" else x[:2000]
        want = one if name != "1" else resample(xs, sr, kernel=rr.rows)
        rs = StreamResampler(sr, kernel=rr.rows)
        assert rs.keep == -((-2 * half) // L)
        parts, pos = [], 0
        for s in sizes:
            parts.append(rs.push(xs[pos : pos + s]))
            pos = min(pos + s, len(xs))
            assert rs.frames_in == pos and rs.samples_out == sum(len(p) for p in parts)
            # latency: output n (input time n M / L) is out once half / L + 1 more input frames have arrived
            due = (pos * L - half - L) // M + 1 if pos * L - half - L >= 0 else 0
            assert rs.samples_out >= min(due, len(want)), (name, pos, rs.samples_out, due)
            assert len(rs._b._hist[0]) <= rs.keep
        parts.append(rs.flush())
        got = np.concatenate(parts)
        assert got.dtype == np.float32 and len(got) == -((-len(xs) * L) // M), name
        assert np.array_equal(got, want), name
        assert rs.frames_in == 0 and rs.samples_out == 0      # flushed: the stream starts again


def test_int16_stereo_stream_and_batched_streams(built_library):
    from thewhisper_amd.resample import BatchedResampler, StreamResampler, resample

    rng = np.random.default_rng(11)
    clips = [(rng.standard_normal((4800 + 531 * s, 2)) * 9000).astype(np.int16) for s in range(3)]
    ones = resample(clips, 48000, kernel=rr.rows)
    for c, o in zip(clips, ones):
        assert np.array_equal(o, rr.resample(c, 48000, dtype=np.float32))
    br = BatchedResampler(3, 48000, channels=2, fmt="s16", kernel=rr.rows)
    got = [[] for _ in clips]
    for i in range(0, max(len(c) for c in clips), 997):
        # stream 1 sends interleaved raw bytes, as a WebSocket client does; a stream with nothing new sends None
        chunks = [clips[0][i : i + 997], clips[1][i : i + 997].tobytes(), clips[2][i : i + 2 * 997] if (i // 997) % 2 == 0 else None]
        for s, o in enumerate(br.push(chunks)):
            got[s].append(o)
    for s, o in enumerate(br.flush()):
        got[s].append(o)
    for s in range(3):
        assert np.array_equal(np.concatenate(got[s]), ones[s]), s
    assert br.launches <= len(range(0, max(len(c) for c in clips), 997)) + 1      # one launch per tick for all streams
    # same rate: a bit-exact copy of the converted, down-mixed input, with no latency
    rs = StreamResampler(16000, channels=2, fmt="s16", kernel=rr.rows)
    assert np.array_equal(rs.push(clips[0]), rr.to_mono_f32(clips[0])) and len(rs.flush()) == 0


class _FakeBackend:
    sample_rate, chunk_length_s = 16000, 10

    def __init__(self):
        self.calls = []

    def transcribe(self, audio, t0, sr):
        self.calls.append((np.asarray(audio), t0, sr))
        return [{"text": f" n{len(audio)}", "start": 0.0, "end": len(audio) / sr}]


class _RecordingScheduler:
    made = []

    def __init__(self, backend, chunk_length_s):
        self.chunks = []
        _RecordingScheduler.made.append(self)

    def add_new_chunk(self, a):
        self.chunks.append(np.array(a, copy=True))

    def process_new_chunk(self):
        return [], [{"text": " x", "start": 0.0, "end": float(sum(len(c) for c in self.chunks)) / 16000}]

    def clear(self):
        self.chunks = []


def _wav(pcm_i16, sr):
    buf = io.BytesIO()
    with wave.open(buf, "wb") as wf:
        wf.setnchannels(pcm_i16.shape[1]); wf.setsampwidth(2); wf.setframerate(sr); wf.writeframes(pcm_i16.tobytes())
    return buf.getvalue()


def test_gateway_resample_is_opt_in(built_library):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from thewhisper_amd.gateway import create_app

    rng = np.random.default_rng(4)
    stereo8k = (rng.standard_normal((4000, 2)) * 8000).astype(np.int16)
    f = {"file": ("chunk.wav", _wav(stereo8k, 8000), "audio/wav")}

    # default app: exactly as before - another rate is a 400, and sessions cannot declare a format
    plain_backend = _FakeBackend()
    plain = TestClient(create_app(plain_backend, scheduler_factory=_RecordingScheduler))
    assert plain.post("/transcribe", files=f).status_code == 400 and plain_backend.calls == []
    assert plain.post("/session/create/", params={"sample_rate": 48000, "encoding": "s16le"}).status_code == 400
    assert plain.get("/health").json()["sessions"] == 0

    backend = _FakeBackend()
    client = TestClient(create_app(backend, scheduler_factory=_RecordingScheduler, resample=True, resample_kernel=rr.rows))
    r = client.post("/transcribe", files=f)
    assert r.status_code == 200, r.text
    audio, t0, sr = backend.calls[-1]
    assert sr == 8000 and audio.dtype == np.int16 and np.array_equal(audio, stereo8k)       # the backend sees the rate (and the frames)
    assert client.post("/transcribe", files={"file": ("chunk.wav", _wav(stereo8k, 16001), "audio/wav")}).status_code == 400
    assert client.post("/transcribe", files={"file": ("chunk.wav", _wav(stereo8k, 2000), "audio/wav")}).status_code == 400
    assert client.post("/transcribe", files={"file": ("chunk.wav", _wav(stereo8k[:, :1], 16000), "audio/wav")}).status_code == 200
    assert backend.calls[-1][2] == 16000 and backend.calls[-1][0].dtype == np.float32       # 16 kHz: the old path

    # a 48 kHz int16 session: its scheduler gets exactly the restatement's samples of the same audio
    x48 = (wo.synth_audio(48000, 8, "speechlike") * 20000).astype(np.int16)
    _RecordingScheduler.made.clear()
    sid = client.post("/session/create/", params={"sample_rate": 48000, "encoding": "s16le"}).json()["session_id"]
    for i in range(0, len(x48), 4800):
        chunk = base64.b64encode(x48[i : i + 4800].tobytes()).decode("ascii")
        assert client.post(f"/session/{sid}/add_chunk", params={"audio_data": chunk}).json() == {"status": "success"}
    assert client.post(f"/session/{sid}/process").status_code == 200
    got = np.concatenate(_RecordingScheduler.made[-1].chunks)
    want = rr.resample(x48, 48000, dtype=np.float32)
    half_l = rr.plan(48000)[2] // rr.plan(48000)[0]
    assert got.dtype == np.float32 and len(want) - len(got) <= half_l // 3 + 1        # all but the tail still waiting for its right context
    assert np.array_equal(got, want[: len(got)])
    assert client.post(f"/session/{sid}/clear").json() == {"status": "success"}
    assert client.app.state.host.sessions[sid]["resampler"].frames_in == 0            # clear resets the resampler
    # sessions at 16 kHz mono float32 create no resampler; unsupported formats are refused at creation
    sid2 = client.post("/session/create/").json()["session_id"]
    sid3 = client.post("/session/create/", params={"sample_rate": 16000, "encoding": "f32le", "channels": 1}).json()["session_id"]
    assert client.app.state.host.sessions[sid2]["resampler"] is None and client.app.state.host.sessions[sid3]["resampler"] is None
    f32 = np.arange(8, dtype=np.float32)
    client.post(f"/session/{sid2}/add_chunk", params={"audio_data": base64.b64encode(f32.tobytes()).decode("ascii")})
    assert np.array_equal(_RecordingScheduler.made[-2].chunks[-1], f32)
    for bad in ({"sample_rate": 16001}, {"encoding": "mulaw"}, {"channels": 9}, {"sample_rate": 100}):
        assert client.post("/session/create/", params=bad).status_code == 400, bad

    # the WebSocket form: stereo int16 at 44.1 kHz
    x441 = (rng.standard_normal((8820, 2)) * 6000).astype(np.int16)
    _RecordingScheduler.made.clear()
    with client.websocket_connect("/ws/stream?sample_rate=44100&encoding=s16le&channels=2") as ws:
        for i in range(0, len(x441), 2205):
            ws.send_bytes(x441[i : i + 2205].tobytes())
            assert set(ws.receive_json()) == {"words", "uncommited_words"}
        ws.send_text("end")
    got = np.concatenate(_RecordingScheduler.made[-1].chunks)
    want = rr.resample(x441, 44100, dtype=np.float32)
    assert 0 < len(got) <= len(want) and np.array_equal(got, want[: len(got)])
    with plain.websocket_connect("/ws/stream?sample_rate=44100") as ws:
        assert "error" in ws.receive_json()


def test_backend_resamples_other_rates_before_the_engine(built_library):
    """AMDWhisperBackend on the CPU stand-in engine: a 48 kHz buffer gives the words of its resampled 16 kHz form, directly
    and through the hub; 16 kHz buffers are untouched."""
    from tests.test_pipeline_glue import build_amd_pipeline, normalise
    from thewhisper_amd import AMDWhisperBackend
    from thewhisper_amd.resample import resample
    from thewhisper_amd.serving import BatchingHub

    torch.set_grad_enabled(False)
    pipe = build_amd_pipeline("micro", 10, 2)
    backend = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=pipe, resample_kernel=rr.rows)
    x48 = wo.synth_audio(48000 * 3, 6, "speechlike").astype(np.float32)
    x16 = resample(x48, 48000, kernel=rr.rows)
    want = normalise(backend.transcribe(x16, 0.0, 16000))
    assert len(want) > 0
    assert normalise(backend.transcribe(x48, 0.0, 48000)) == want
    assert normalise(backend.transcribe_many([(x48, 0.0, 48000), (x16, 0.0, 16000)])[0]) == want
    a, sr = backend.to_engine_rate(x16, 16000)
    assert a is x16 and sr == 16000
    hub = BatchingHub(backend, max_batch=2, max_wait_s=0.05)
    try:
        assert normalise(hub.submit(x48, 0.0, 48000).result(timeout=300)) == want
    finally:
        hub.close()
