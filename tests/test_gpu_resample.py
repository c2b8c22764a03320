"""-m gpu: tw_resample on the MI355X against the float64 restatement (tests/resample_ref.py), its bit-exactness statements
(cuts, launch shape, pass-through), the backend and the gateway's 48 kHz int16 sessions on the real engine, and misuse."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import resample_ref as rr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _rows(rng, sr, fmt, ch, B):
    """B ragged rows of [frames, ch]: between 1/40 and 1/10 s each (several blocks of outputs); wide batches also carry an
    empty row and a one-frame row."""
    lens = [int(v) for v in rng.integers(sr // 40, sr // 10, size=B)]
    if B >= 16:
        lens[1], lens[2] = 0, 1
    out = []
    for n in lens:
        x = rng.uniform(-1.0, 1.0, size=(n, ch))
        out.append((x * 32767).astype(np.int16) if fmt == "s16" else x.astype(np.float32))
    return out


def _bound(sr, x_max):
    """(taps_per_output + 2) 2^-24 max_phase sum|h| max|x|  +  2^-24 sum|h| max|x| (float32 rounding of the taps), from the
    plan's own table."""
    L, M, half, tpo = rr.plan(sr)
    h = np.abs(rr.taps(sr))
    phase = max(h[p::L].sum() for p in range(L))
    return ((tpo + 2) * 2.0 ** -24 * phase + 2.0 ** -24 * phase) * x_max


@pytest.mark.parametrize("sr", rr.RATES)
def test_parity_with_the_float64_restatement(sr):
    from thewhisper_amd.resample import resample

    L, M, _, _ = rr.plan(sr)
    rng = np.random.default_rng(sr)
    for fmt in ("f32", "s16"):
        for ch in (1, 2):
            for B in (1, 3, 16, 64):
                clips = _rows(rng, sr, fmt, ch, B)
                got = resample(clips, sr)
                worst = 0.0
                for c, g in zip(clips, got):
                    want = rr.resample(c, sr)
                    assert g.dtype == np.float32 and len(g) == len(want) == -((-len(c) * L) // M)
                    if len(c) == 0:
                        continue
                    tol = _bound(sr, float(np.abs(rr.to_mono_f32(c)).max()))
                    err = float(np.abs(g.astype(np.float64) - want).max())
                    worst = max(worst, err / tol)
                    assert err <= tol, (sr, fmt, ch, B, err, tol)
                print(f"{sr} Hz {fmt} ch={ch} B={B}: worst error / bound = {worst:.3f}")


def test_a_rate_whose_window_does_not_fit_lds_takes_the_unstaged_path():
    """400 kHz (L=1, M=25): a block's input window is larger than the LDS buffer, so the kernel reads global memory directly -
    same chain, same bound."""
    from thewhisper_amd.resample import resample

    sr = 400000
    x = np.random.default_rng(2).uniform(-1, 1, size=(30011, 2)).astype(np.float32)
    got, want = resample(x, sr), rr.resample(x, sr)
    assert len(got) == len(want) and np.abs(got - want).max() <= _bound(sr, float(np.abs(rr.to_mono_f32(x)).max()))


@pytest.mark.parametrize("sr", (8000, 44100, 48000))
def test_cuts_do_not_matter_in_bits(sr):
    from thewhisper_amd.resample import BatchedResampler, StreamResampler, resample

    n = sr + 123
    x = (wo.synth_audio(n, 3, "speechlike") * 30000).astype(np.int16)
    one = resample(x, sr)
    assert np.array_equal(one, resample(torch.from_numpy(x).cuda(), sr).cpu().numpy())      # device input: same launch
    rng = np.random.default_rng(sr)
    rand = []
    while sum(rand) < n:
        rand.append(int(rng.integers(0, 3000)))
    for name, sizes in (("7", [7] * (600 // 7 + 1)), ("160", [160] * (n // 160 + 1)), ("4410", [4410] * (n // 4410 + 1)),
                        ("half_second", [sr // 2] * 3), ("random", rand), ("1", [1] * 300)):
        xs = x[: sum(sizes)] if name in ("1", "7") else x
        want = one if len(xs) == len(x) else resample(xs, sr)
        rs = StreamResampler(sr, fmt="s16")
        parts, pos = [], 0
        for s in sizes:
            parts.append(rs.push(xs[pos : pos + s]))
            pos += s
        parts.append(rs.flush())
        assert np.array_equal(np.concatenate(parts), want), (sr, name)
    # several streams in one launch per tick, each cut differently from its one-shot run
    clips = [x[: n - 1000 * s] for s in range(5)]
    br = BatchedResampler(5, sr, fmt="s16")
    got = [[] for _ in clips]
    for i in range(0, n, 3001):
        for s, o in enumerate(br.push([c[i : i + 3001] for c in clips])):
            got[s].append(o)
    for s, o in enumerate(br.flush()):
        got[s].append(o)
    for s, c in enumerate(clips):
        assert np.array_equal(np.concatenate(got[s]), resample(c, sr)), (sr, s)


@pytest.mark.parametrize("sr", (8000, 11025, 44100, 48000, 96000))
def test_launch_shape_does_not_matter_in_bits(sr):
    from thewhisper_amd.resample import resample

    rng = np.random.default_rng(sr + 1)
    clips = _rows(rng, sr, "f32", 2, 64)
    together = resample(clips, sr)
    for b in (0, 5, 63):
        assert np.array_equal(resample(clips[b], sr), together[b]), (sr, b)


@pytest.mark.parametrize("fmt,ch", (("f32", 1), ("f32", 2), ("s16", 1), ("s16", 2), ("s16", 8), ("f32", 3)))
def test_same_rate_is_a_bit_exact_copy_of_the_converted_downmixed_input(fmt, ch):
    from thewhisper_amd.resample import StreamResampler, resample

    x = _rows(np.random.default_rng(ch), 16000, fmt, ch, 1)[0]
    want = rr.to_mono_f32(x)
    assert np.array_equal(resample(x, 16000), want)
    rs = StreamResampler(16000, channels=ch, fmt=fmt)
    assert np.array_equal(np.concatenate([rs.push(x[:700]), rs.push(x[700:]), rs.flush()]), want)


def test_end_to_end_on_the_synthetic_checkpoint():
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from tests.node_factory import TinyScheduler
    from tests.test_pipeline_glue import build_amd_pipeline, normalise
    from thewhisper_amd import AMDWhisperBackend
    from thewhisper_amd.gateway import create_app
    from thewhisper_amd.resample import StreamResampler, resample
    from thewhisper_amd.serving import BatchingHub

    pipe = build_amd_pipeline("micro", 10, 4, device="cuda", engine_factory=None)
    backend = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=pipe)
    x48 = wo.synth_audio(48000 * 4, 12, "speechlike").astype(np.float32)
    x16 = resample(x48, 48000)
    plain = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=pipe, draft_previous_tick=False)
    want = backend.transcribe(x16, 0.0, 16000)
    assert len(want) > 0
    assert normalise(want) == normalise(plain.transcribe(x16.copy(), 0.0, 16000))        # the 16 kHz call is what it was
    backend.reset()
    assert backend.transcribe(x48, 0.0, 48000) == want
    assert backend.transcribe_many([(x48, 0.0, 48000)])[0] == plain.transcribe_many([(x16, 0.0, 16000)])[0]

    # a WebSocket session fed 48 kHz int16 chunks answers, reply by reply, what a 16 kHz float32 session answers when fed
    # StreamResampler's output for the same chunks
    hub = BatchingHub(backend, max_batch=4, max_wait_s=0.05)
    client = TestClient(create_app(hub, scheduler_factory=TinyScheduler, resample=True))
    s48 = (np.clip(x48, -1, 1) * 32767).astype(np.int16)
    stereo = np.stack([s48, s48], axis=1)
    try:
        with client.websocket_connect("/ws/stream?sample_rate=48000&encoding=s16le&channels=2") as ws:
            got = []
            for i in range(0, len(stereo), 24000):
                ws.send_bytes(stereo[i : i + 24000].tobytes())
                got.append(ws.receive_json())
            ws.send_text("end")
        rs = StreamResampler(48000, channels=2, fmt="s16")
        with client.websocket_connect("/ws/stream") as ws:
            ref = []
            for i in range(0, len(stereo), 24000):
                ws.send_bytes(rs.push(stereo[i : i + 24000]).tobytes())
                ref.append(ws.receive_json())
            ws.send_text("end")
    finally:
        hub.close()
    assert got == ref and all("error" not in r for r in got) and any(r["uncommited_words"] for r in got)


def test_misuse_gives_error_codes_and_no_fault():
    from thewhisper_amd import _cabi
    from thewhisper_amd import resample as rs

    lib = _cabi.load_library()
    x = torch.zeros(64, dtype=torch.float32, device="cuda")
    y = torch.zeros(64, dtype=torch.float32, device="cuda")
    first, count, ofirst = (C.c_int64 * 65)(), (C.c_int32 * 65)(*([16] * 65)), (C.c_int64 * 65)()
    px, py = C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr())

    def call(device=0, in_dev=px, fmt=0, channels=1, stride=16, in_first=first, in_count=count, sr_in=48000, sr_out=16000,
             out_first=ofirst, n_out=4, out_dev=py, out_stride=4, B=1):
        return lib.tw_resample(device, in_dev, fmt, channels, stride, in_first, in_count, sr_in, sr_out, out_first, n_out, out_dev,
                               out_stride, B, None)

    assert call() == 0
    torch.cuda.synchronize()
    for kw in (dict(sr_in=0), dict(sr_in=16001), dict(sr_out=0), dict(channels=9), dict(channels=0), dict(B=65), dict(B=0),
               dict(n_out=0), dict(n_out=-3), dict(in_dev=None), dict(out_dev=None), dict(in_first=None), dict(in_count=None),
               dict(out_first=None), dict(fmt=7), dict(out_stride=3), dict(in_count=(C.c_int32 * 1)(17)),
               dict(in_count=(C.c_int32 * 1)(-1)), dict(out_first=(C.c_int64 * 1)(-1)), dict(device=-1), dict(device=4096),
               dict(in_dev=C.c_void_p(x.data_ptr() + 1))):
        assert call(**kw) == -1 and len(lib.tw_last_error(None)) > 0, kw
    assert lib.tw_resample_taps(48000, 16000, None, 97) == -1
    assert lib.tw_resample_taps(48000, 16000, (C.c_double * 97)(), 96) == -1
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        rs.resample(np.zeros((10, 9), np.float32), 48000)
    with pytest.raises(ValueError):
        rs.resample(np.zeros(10, np.float32), 16001)
    with pytest.raises(ValueError):
        rs.StreamResampler(48000, channels=2, fmt="s16").push(np.zeros(3, np.int16))       # half a frame
    with pytest.raises(ValueError):
        rs.StreamResampler(48000, fmt="s16").push(np.zeros(4, np.float32))                 # the wrong sample type
    assert len(rs.resample(np.zeros(0, np.float32), 48000)) == 0
