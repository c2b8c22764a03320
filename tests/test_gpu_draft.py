"""Round 6 (`-m gpu`, through the C ABI):

* a stream's results do not depend on the other rows of its launch - 1, 16, 17 and 64 rows, an ordinary step or the rows mode of
  the batched prefill - BIT FOR BIT, in every context dtype, at the REAL width (d = 1280, ffn = 5120: the long-K projection takes
  16 wavefronts per tile with one group of streams and 8 with several; k_decode.hip gives both the same sixteen K slices and the
  same order of additions);
* tw_greedy_opts::n_draft (draft-and-verify): whatever is offered as a draft - the true continuation, a corrupted
  one, rubbish - the call returns what it returns without it: ids against the oracle's `greedy_generate` (strict f32) and ids,
  alignment rows and token timestamps against the engine's own plain call (every dtype), with the expected number of confirmed tokens;
* the same with drafts that run on BEHIND a stream's <eos> while other streams go on (`test_draft_past_eos_*`, on tests/eos_model.py, a
  micro model with decoder layers whose rows end at different steps and some never): the finished row is padded, the length is set by
  the last <eos>, and every case first shows on the engine's own plain call that its rows end where the case needs them to;
* `AMDWhisperBackend(draft_previous_tick=True)` on the reference scheduler's call sequence: every call's words identical to the
  plain backend's."""
import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import eos_model as em
from tests.util import PROMPT, clips, dims_variant, make_engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


REAL = dict(enc_layers=1, dec_layers=2)


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32", "fp8a16"])
def test_rows_of_a_launch_do_not_matter(dtype):
    """The same clip (slot 0) teacher-forced through 7 positions alone, among 16, 17 and 64 rows, and again from another slot of
    the 64-row launch: identical logits, bit for bit.  Then the rows mode: a forced-prefix call (positions in launches of up to 64
    rows) must leave exactly the alignment rows and produce exactly the ids of the step-by-step call."""
    dims = dims_variant("large-v3", **REAL)
    w = wo.make_weights(dims, 2)
    heads = [(1, 0), (1, 3)]
    T, Bmax = 100, 64
    eng = make_engine(dims, w, T=T, max_batch=Bmax, dtype=dtype, heads=heads, use_graph=False)
    try:
        pcm = clips(T * 320, Bmax)
        pcm[40] = pcm[0]                                      # the same audio in another group of 16 rows
        mel = eng.logmel(torch.from_numpy(pcm).cuda())
        ids = np.concatenate([np.tile(np.array(PROMPT), (Bmax, 1)), np.random.default_rng(3).integers(0, 50000, size=(Bmax, 4))], axis=1)
        ids[40] = ids[0]

        def run(B):
            eng.encode(mel[:B]); eng.cross_kv(B); eng.decoder_reset(B)
            return np.stack([eng.decode_step(ids[:B, s].tolist()).cpu().numpy() for s in range(ids.shape[1])], axis=1)

        one = run(1)
        for B in (16, 17, 64, 33):
            got = run(B)
            assert np.array_equal(got[0], one[0]), f"{dtype}: row 0 of a {B}-row launch differs from the one-row launch"
            if B == 64:
                assert np.array_equal(got[40], one[0]), f"{dtype}: slot 40 differs from slot 0 on the same audio"
        # rows mode (prefill launches of 16-64 rows) against the one-position steps: free-running ids, alignment rows, timestamps
        for B in (1, 3):
            eng.encode(mel[:B]); eng.cross_kv(B)
            prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
            kw = dict(max_new_tokens=40, min_new_tokens=40, timestamps=True, want_alignment=True)
            full = eng.generate_greedy(prompt, **kw)
            L = full["length"]
            al_full = eng.get_alignment(B, L - 1)
            forced = full["sequences"][:, : 3 + 30].astype(np.int32)
            out = eng.generate_greedy(forced, n_forced=30, **kw)
            assert np.array_equal(out["sequences"], full["sequences"]), dtype
            assert np.array_equal(eng.get_alignment(B, L - 1), al_full), dtype
    finally:
        eng.close()


@pytest.mark.parametrize("dtype,T", [("bf16", 500), ("f16", 1000), ("bf16", 1500), ("f32", 500)])
def test_streams_of_a_pass_do_not_matter_encoder_included(dtype, T):
    """The encoder side of the same statement: a clip's encoder states - and with them its logits - are bit for bit the same whether it
    is encoded alone (M = T rows: 64 x 64 tiles, plain epilogue), with two others, or among 16 / 40 clips (M >= 8000 rows: the
    large-M kernel with its LDS-staged epilogue, 128-query attention workgroups).  Until round 6 the two epilogues summed the
    LayerNorm statistics they leave for the next GEMM in different orders (18 % of the 16-bit encoder states differed between a
    one-clip and a 16-clip pass); tw_common.h: tw_stat4."""
    dims = dims_variant("large-v3", enc_layers=2, dec_layers=1)
    w = wo.make_weights(dims, 2)
    eng = make_engine(dims, w, T=T, max_batch=40, dtype=dtype, heads=[(0, 0)], use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(clips(T * 320, 40)).cuda())
        ids = np.array(PROMPT + [1234, 777])
        ref = None
        for B in (1, 3, 16, 40):
            enc = eng.encode(mel[:B], return_hidden=True)[0].float().cpu().numpy()
            eng.cross_kv(B); eng.decoder_reset(B)
            lg = np.stack([eng.decode_step([int(t)] * B).cpu().numpy()[0] for t in ids])
            if ref is None:
                ref = (enc, lg)
                continue
            assert np.array_equal(enc, ref[0]), f"{dtype} T={T}: encoder states of clip 0 among {B} clips differ from the one-clip pass"
            assert np.array_equal(lg, ref[1]), f"{dtype} T={T}: logits of clip 0 among {B} clips differ from the one-clip pass"
    finally:
        eng.close()


def _corrupt(seq, n0, where, rng, V=50000):
    d = seq[:, n0:].copy()
    for b in range(d.shape[0]):
        for j in where:
            if j < d.shape[1]:
                d[b, j] = (int(d[b, j]) + 1 + int(rng.integers(0, V - 2))) % V
    return d


DRAFT_CASES = [
    # preset, layers, T, B, max_new, forced length?, dtype, graph
    ("micro", None, 100, 1, 60, True, "f32", True), ("micro", None, 100, 1, 60, False, "f32", False), ("micro", None, 500, 3, 40, True, "f32", True),
    ("micro", None, 100, 16, 30, True, "f32", True), ("micro", None, 100, 1, 120, True, "bf16", True), ("micro", None, 750, 2, 40, True, "fp8a16", True),
    ("micro", None, 100, 5, 90, True, "f16", False), ("micro", None, 100, 2, 40, True, "fp8a8", True),
    ("large-v3", REAL, 100, 1, 100, True, "bf16", True), ("large-v3", REAL, 100, 1, 100, False, "f16", True), ("large-v3", REAL, 100, 2, 48, True, "f32", True),
    ("large-v3", REAL, 100, 4, 48, True, "fp8a16", True), ("large-v3", REAL, 100, 20, 24, True, "bf16", True),
]


@pytest.mark.parametrize("preset,layers,T,B,max_new,fixed_len,dtype,graph", DRAFT_CASES)
def test_draft_and_verify_returns_the_plain_result(preset, layers, T, B, max_new, fixed_len, dtype, graph):
    dims = dims_variant(preset, **layers) if layers else wo.PRESETS[preset]
    w = wo.make_weights(dims, 0 if layers is None else 2)
    heads = [(dims.dec_layers - 1, 0), (dims.dec_layers - 1, 1)]
    eng = make_engine(dims, w, T=T, max_batch=B, dtype=dtype, heads=heads, use_graph=graph)
    try:
        pcm = clips(T * 320, B)
        mel = eng.logmel(torch.from_numpy(pcm).cuda(), out_dtype=torch.float32)
        eng.encode(mel); eng.cross_kv(B)
        prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
        kw = dict(max_new_tokens=max_new, min_new_tokens=max_new if fixed_len else 0, timestamps=True, want_alignment=True)
        full = eng.generate_greedy(prompt, **kw)
        L = full["length"]
        seq = full["sequences"]
        al_full = eng.get_alignment(B, L - 1)
        nf = [2 * T] * B
        ts_full = eng.token_timestamps(B, 3, L, nf)
        if dtype == "f32" and preset == "micro":
            om = wo.OracleWhisper(dims, w, T=T)
            opt = wo.GreedyOptions(max_new_tokens=max_new, min_new_tokens=max_new if fixed_len else 0, timestamps=True, alignment_heads=heads)
            ref = wo.greedy_generate(om, om.encode(wo.log_mel(pcm, dims.n_mels)), prompt, opt)
            assert np.array_equal(seq, ref["sequences"])
        # what may be offered: generated tokens before any <eos> / padding of any row
        gen = seq[:, 3:]
        n_ok = int(min([np.nonzero(r == 50257)[0][0] if (r == 50257).any() else len(r) for r in gen]))
        n_ok = min(n_ok, max_new - 2)
        assert n_ok >= 4, "the case needs a few tokens to offer"
        rng = np.random.default_rng(5)
        variants = {
            "true continuation": (gen[:, :n_ok].copy(), n_ok),
            "half of it": (gen[:, : n_ok // 2].copy(), n_ok // 2),
            "one token": (gen[:, :1].copy(), 1),
            "wrong from the start": (_corrupt(seq[:, : 3 + n_ok], 3, range(n_ok), rng), None),
            "one wrong token": (_corrupt(seq[:, : 3 + n_ok], 3, [n_ok // 3], rng), None),
            "three wrong tokens": (_corrupt(seq[:, : 3 + n_ok], 3, [2, n_ok // 2, n_ok - 1], rng), None),
        }
        if B > 1:       # only ONE stream's draft is wrong: the round ends there for everybody, the others' drafts are offered again
            d = gen[:, :n_ok].copy()
            d[B - 1, n_ok // 2] = (int(d[B - 1, n_ok // 2]) + 7) % 50000
            variants["one stream wrong"] = (d, None)
        for name, (draft, want_acc) in variants.items():
            draft = np.where(draft == 50257, 0, draft).astype(np.int32)
            out = eng.generate_greedy(np.concatenate([prompt, draft], axis=1), n_draft=draft.shape[1], **kw)
            what = f"{preset} {dtype} B={B}: draft = {name}"
            assert out["length"] == L and np.array_equal(out["sequences"], seq), what
            assert np.array_equal(eng.get_alignment(B, L - 1), al_full), what
            assert np.array_equal(eng.token_timestamps(B, 3, L, nf), ts_full), what
            dr = out["draft"]
            assert dr["offered"] == draft.shape[1] * B and dr["launches"] >= 1 and dr["rounds"] >= 1
            n_same = int(np.min([np.argmax(np.append(draft[b] != gen[b, : draft.shape[1]], True)) for b in range(B)]))
            assert dr["accepted"] >= n_same * B, (what, dr, n_same)          # round 1 confirms the common prefix, later rounds may add
            if want_acc is not None:
                assert dr["accepted"] == want_acc * B and dr["rounds"] == 1, (what, dr)
            if name == "one wrong token" and B <= 4:       # the rest of the draft is confirmed by the rounds that follow
                assert dr["accepted"] == (n_ok - 1) * B and dr["rounds"] >= 2, (what, dr)
        # misuse
        with pytest.raises(RuntimeError, match="n_draft"):
            eng.generate_greedy(np.concatenate([prompt, gen[:, :4].astype(np.int32)], axis=1), n_draft=4, n_forced=2, **kw)
        with pytest.raises(RuntimeError, match="n_draft"):
            eng.generate_greedy(prompt, n_draft=3, **kw)
        bad = np.concatenate([prompt, gen[:, :4].astype(np.int32)], axis=1); bad[0, -1] = 50257
        with pytest.raises(RuntimeError, match="draft token"):
            eng.generate_greedy(bad, n_draft=4, **kw)
        # and the context is as usable as before
        again = eng.generate_greedy(prompt, **kw)
        assert np.array_equal(again["sequences"], seq)
    finally:
        eng.close()


def test_backend_with_drafts_reproduces_the_plain_backend_on_the_scheduler_sequence():
    """`AMDWhisperBackend(draft_previous_tick=True)` on the golden stream's call sequence (ragged rolling buffers as the reference
    scheduler sends them): every call returns the plain backend's words - text, start, end - exactly."""
    import json
    import os

    from tests.test_pipeline_glue import build_amd_pipeline, normalise
    from thewhisper_amd import AMDWhisperBackend

    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "pipeline_golden.json")))["streaming_micro_c10"]
    audio = wo.synth_audio(16000 * gold["seconds"], gold["seed"], gold["kind"])
    plain = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=build_amd_pipeline("micro", 10, 1, device="cuda", engine_factory=None),
                              draft_previous_tick=False)
    draft = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=build_amd_pipeline("micro", 10, 1, device="cuda", engine_factory=None),
                              draft_previous_tick=True)
    for c in gold["calls"]:
        buf = audio[c["offset"] : c["offset"] + c["n"]]
        a = plain.transcribe(buf.copy(), c["t0"], 16000)
        b = draft.transcribe(buf.copy(), c["t0"], 16000)
        assert normalise(a) == normalise(b), c
        assert [(w["start"], w["end"]) for w in a] == [(w["start"], w["end"]) for w in b], c
    st = draft.reuse_stats
    print(f"\nDRAFT (MI355X, micro model, golden stream): {st['reused']} of {st['calls']} calls offered a draft, {st['draft_tokens']} tokens offered, "
          f"{st['confirmed_tokens']} confirmed, {st['verify_launches']} verify launches")
    assert st["reused"] >= 1 and st["draft_tokens"] > 0


@pytest.mark.parametrize("dtype,layers,n_calls", [("f16", 2, 60), ("bf16", 2, 60), ("f16", 32, 30)])
def test_config3_trace_at_the_real_width_draft_ids_equal_plain_ids(dtype, layers, n_calls):
    """BASELINE config 3's call pattern (tests/golden/config3_trace.json: the rolling buffers the REFERENCE'S scheduler hands its
    backend for a 60 s stream, R:thestage_speechkit/streaming/streaming_pipeline.py:388-435, :770-796) at whisper-large-v3's width
    (d = 1280, ffn = 5120, 20 heads, full vocabulary; 2 + 2 layers so that the case takes seconds, and the first 30 calls at the
    FULL 32 + 32 layers in float16): the first calls of the trace through the
    plain backend and through `draft_previous_tick=True` on the same engine - the token ids the engine decoded (every seek pass,
    before tokenizer / filter / merge) are IDENTICAL call by call, the words too, and drafts were offered and confirmed.  What
    bench.py reports for the full depth (`config3.with_draft_previous_tick.token_identity_mean` = 1.0) is asserted here."""
    import json
    import os

    import bench
    from thewhisper_amd import AMDWhisperBackend, ASRPipeline, synthetic
    from thewhisper_amd.engine import WhisperEngine
    from transformers import WhisperFeatureExtractor

    dims = dict(bench.DIMS["large-v3"], enc_layers=layers, dec_layers=layers)
    heads = [(layers - 1, 0), (layers - 1, 3)]
    trace = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "config3_trace.json")))
    chunk_s = trace["chunk_length_s"]
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}[dtype]
    eng = WhisperEngine(dims, 50 * chunk_s, max_batch=1, dtype=dtype, alignment_heads=heads, use_graph=True)
    try:
        eng.load_state_dict(bench.random_state_dict(dims, torch.device("cuda", 0), seed=0))
        model = synthetic.skeleton_model(dims, device="cuda:0", dtype=tdt, alignment_heads=heads)
        pipe = ASRPipeline(model, feature_extractor=WhisperFeatureExtractor(feature_size=dims["n_mels"], chunk_length=chunk_s),
                           tokenizer=synthetic.build_tokenizer(dims["vocab"]), chunk_length_s=chunk_s, device="cuda:0", torch_dtype=tdt,
                           batch_size=1, engine=eng)
        stream = (np.random.default_rng(trace["seed"]).standard_normal(16000 * trace["seconds"]) * 0.1).clip(-1, 1).astype(np.float32)
        seen = []
        inner = eng.generate_greedy

        def recording(prompt, **kw):
            out = inner(prompt, **kw)
            for row in out["sequences"][:, 3:]:
                hit = np.nonzero(row == int(kw.get("eos_id", 50257)))[0]
                seen.append(np.asarray(row[: int(hit[0])] if len(hit) else row, dtype=np.int64))
            return out

        eng.generate_greedy = recording
        got = {}
        for variant in ("plain", "draft"):
            be = AMDWhisperBackend(None, chunk_length_s=chunk_s, asr_pipeline=pipe, draft_previous_tick=(variant == "draft"))
            be.transcribe(stream[:16000], 0.0, 16000)      # plan learning outside the compared calls
            be.reset()
            ids, words = [], []
            for c in trace["calls"][:n_calls]:
                seen.clear()
                words.append(be.transcribe(stream[c["offset"] : c["offset"] + c["n"]], c["t0"], 16000))
                ids.append(np.concatenate(seen) if seen else np.zeros(0, np.int64))
            got[variant] = (ids, words, dict(be.reuse_stats))
        for i, (a, b) in enumerate(zip(got["plain"][0], got["draft"][0])):
            assert len(a) == len(b) and (a == b).all(), f"{dtype}: call {i} of the trace decodes other ids with a draft"
        assert got["plain"][1] == got["draft"][1]
        st = got["draft"][2]
        print(f"\nCONFIG3 {dtype} (large-v3 width, {layers} + {layers} layers, {n_calls} calls): {st['reused']} calls offered a draft, {st['draft_tokens']} tokens offered, "
              f"{st['confirmed_tokens']} confirmed, {st['verify_launches']} verify launches; ids identical on every call")
        assert st["reused"] >= n_calls // 2 and st["confirmed_tokens"] > 0
    finally:
        eng.generate_greedy = inner
        eng.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "fp8a16", "fp8a8"])
def test_draft_fuzz_random_drafts_never_change_the_result(dtype):
    """Property test of `n_draft`, graph replay on and off, on two micro models.
    make_weights(micro, 0): 60 random situations per dtype - 1 ... 16 streams, 6 ... 90 new tokens, <eos> masked up to the full length or
    not (no row of this model emits <eos> within 90 tokens either way, so both are fixed-length runs and the draft stops short of nothing),
    timestamp grammar on or off, a suppress list or none, drafts of random length whose tokens are corrupted at a random rate (0 = the
    true continuation ... 1 = rubbish, sometimes in one stream only).
    tests/eos_model.py (rows end at different steps, some never): 40 more - 1 ... 16 of its clips, 16 ... 40 new tokens, free length, a
    setting of its table; the draft's length is drawn up to the LONGEST row's end (max_new - 2 where a row never ends), with filler that
    is not <eos> behind each shorter row's end, corrupted as above.  At least 10 of them have a row ending inside the drafted span.
    In every situation the call returns the plain call's ids, length, alignment rows and token timestamps."""
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    heads = [(1, 0), (1, 1)]
    T = 100
    rng = np.random.default_rng({"f32": 1, "bf16": 2, "f16": 3, "fp8a16": 4, "fp8a8": 5}[dtype])
    engines = {g: make_engine(dims, w, T=T, max_batch=16, dtype=dtype, heads=heads, use_graph=g) for g in (True, False)}
    try:
        pcm = clips(T * 320, 16)
        n_engaged = 0
        for case in range(60):
            eng = engines[bool(case % 2)]
            B = int(rng.choice([1, 1, 2, 3, 5, 16]))
            sel = rng.permutation(16)[:B]
            mel = eng.logmel(torch.from_numpy(pcm[sel]).cuda(), out_dtype=torch.float32)
            eng.encode(mel); eng.cross_kv(B)
            max_new = int(rng.integers(6, 91))
            ts_on = bool(rng.integers(0, 2))
            kw = dict(max_new_tokens=max_new, min_new_tokens=max_new if rng.integers(0, 2) else 0, timestamps=ts_on, want_alignment=True)
            if rng.integers(0, 3) == 0:
                kw["suppress"] = tuple(int(x) for x in rng.integers(0, 50000, size=20))
            prompt = np.tile(np.array(PROMPT if ts_on else PROMPT + [50364], dtype=np.int32), (B, 1))
            n0 = prompt.shape[1]
            full = eng.generate_greedy(prompt, **kw)
            L, seq = full["length"], full["sequences"]
            al = eng.get_alignment(B, L - 1)
            ts = eng.token_timestamps(B, n0, L, [2 * T] * B)
            gen = seq[:, n0:]
            n_ok = int(min([np.nonzero(r == 50257)[0][0] if (r == 50257).any() else len(r) for r in gen]))
            n_ok = min(n_ok, max_new - 2)
            if n_ok < 1:
                continue
            nd = int(rng.integers(1, n_ok + 1))
            draft = gen[:, :nd].copy().astype(np.int32)
            rate = float(rng.choice([0.0, 0.0, 0.03, 0.15, 0.5, 1.0]))
            rows = range(B) if rng.integers(0, 2) else [int(rng.integers(0, B))]
            for b in rows:
                for j in range(nd):
                    if rng.random() < rate:
                        draft[b, j] = int(rng.integers(0, 50000))
            draft = np.where(draft == 50257, 0, draft).astype(np.int32)
            out = eng.generate_greedy(np.concatenate([prompt, draft], axis=1), n_draft=nd, **kw)
            what = f"{dtype} case {case}: B={B} max_new={max_new} ts={ts_on} nd={nd} rate={rate} graph={bool(case % 2)}"
            assert out["length"] == L and np.array_equal(out["sequences"], seq), what
            assert np.array_equal(eng.get_alignment(B, L - 1), al), what
            assert np.array_equal(eng.token_timestamps(B, n0, L, [2 * T] * B), ts), what
            n_engaged += 1
        assert n_engaged >= 40
    finally:
        for e in engines.values():
            e.close()
    # ---- the model whose rows end: the draft runs past them ----
    n_engaged, n_past = _fuzz_past_eos(dtype)
    print(f"\nfuzz {dtype}, rows that end: {n_engaged} situations, {n_past} with a row ending inside the drafted span")
    assert n_engaged >= 40 and n_past >= 10, (n_engaged, n_past)


def _fuzz_past_eos(dtype):
    engines = {(es, g): make_engine(*em.model(es), T=em.T, max_batch=16, dtype=dtype, heads=em.HEADS, use_graph=g)
               for es in sorted({es for es, _ in em.SETTINGS}) for g in (True, False)}
    n_engaged = n_past = 0
    try:
        pcm = em.audio(range(16))
        rng = np.random.default_rng(em.FUZZ_EOS_SEED[dtype] + 1000)          # filler and corruption: these draws may depend on results
        for case, sit in enumerate(em.fuzz_eos_situations(dtype)):
            eng = engines[(sit["es"], sit["graph"])]
            sel, B, max_new = list(sit["sel"]), len(sit["sel"]), sit["max_new"]
            eng.encode(eng.logmel(torch.from_numpy(pcm[sel]).cuda(), out_dtype=torch.float32)); eng.cross_kv(B)
            kw = em.engine_kw(sit["timestamps"], max_new)
            prompt = em.prompt(sel)
            full = eng.generate_greedy(prompt, **kw)
            L, seq = full["length"], full["sequences"]
            nf = [2 * em.T] * B
            al = eng.get_alignment(B, L - 1)
            ts = eng.token_timestamps(B, em.N_PROMPT, L, nf)
            gen = np.concatenate([seq[:, em.N_PROMPT:], np.full((B, max_new), em.EOS)], axis=1)[:, :max_new]
            steps = em.eos_steps(gen)
            nd, past = em.fuzz_eos_draft_length(steps, max_new, sit["u"])
            if nd < 1:
                continue
            draft = em.filled_draft(gen, nd, rng, repeat_last=sit["repeat"])
            for b in (range(B) if not sit["one_row"] else [int(rng.integers(0, B))]):
                for j in range(nd):
                    if rng.random() < sit["rate"]:
                        draft[b, j] = int(rng.integers(0, em.EOS))
            out = eng.generate_greedy(np.concatenate([prompt, draft], axis=1), n_draft=nd, **kw)
            what = f"{dtype} case {case}: {sit} rows end after {steps} nd={nd}"
            assert out["length"] == L and np.array_equal(out["sequences"], seq), (what, out["draft"])
            assert np.array_equal(eng.get_alignment(B, L - 1), al), what
            assert np.array_equal(eng.token_timestamps(B, em.N_PROMPT, L, nf), ts), what
            n_engaged += 1
            n_past += int(past)
    finally:
        for e in engines.values():
            e.close()
    return n_engaged, n_past


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_batch_composition_fuzz_at_the_real_width(dtype):
    """Property form of "who else is in the batch does not matter" (large-v3 width, 1 + 2 layers, T = 500 so that a 16-clip pass reaches
    the large-M encoder kernel): 12 random passes - 1 ... 40 clips drawn at random, in random slots - and in every one of them each
    clip's encoder states and teacher-forced logits are bit for bit those of the clip alone."""
    dims = dims_variant("large-v3", enc_layers=1, dec_layers=2)
    w = wo.make_weights(dims, 2)
    T, N = 500, 40
    eng = make_engine(dims, w, T=T, max_batch=N, dtype=dtype, heads=[(1, 0)], use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(clips(T * 320, N)).cuda())
        ids = PROMPT + [4242, 99]
        rng = np.random.default_rng(7)

        def run(sel):
            B = len(sel)
            enc = eng.encode(mel[torch.as_tensor(sel)], return_hidden=True).float().cpu().numpy()
            eng.cross_kv(B); eng.decoder_reset(B)
            lg = np.stack([eng.decode_step([int(t)] * B).cpu().numpy() for t in ids], axis=1)
            return enc, lg

        alone = {}
        for case in range(12):
            B = int(rng.choice([1, 2, 3, 7, 15, 16, 17, 31, 33, 40]))
            sel = rng.permutation(N)[:B].tolist()
            enc, lg = run(sel)
            for slot in {0, B - 1, int(rng.integers(0, B))}:
                c = sel[slot]
                if c not in alone:
                    alone[c] = run([c])
                    enc, lg = run(sel)      # (the one-clip pass overwrote the context)
                assert np.array_equal(enc[slot], alone[c][0][0]), f"{dtype}: clip {c} in slot {slot} of a {B}-clip pass: encoder states differ"
                assert np.array_equal(lg[slot], alone[c][1][0]), f"{dtype}: clip {c} in slot {slot} of a {B}-clip pass: logits differ"
    finally:
        eng.close()


# --------------------------------------------------------------------------------------------------------------------
# drafts that run past a stream's <eos> (tests/eos_model.py: a micro model with decoder layers whose rows end at different steps)
# --------------------------------------------------------------------------------------------------------------------
def _past_eos_variants(gen, max_new, rng):
    """name -> draft [B, n] (one length for all rows, no <eos>), from the plain call's generated tokens `gen`:
      (a)  every row's true continuation up to the LONGEST row's <eos> step (max_new - 2 where a row never ends), filler - random
           text ids - behind each shorter row's end; (a') the same with the row's own last tokens repeated as filler;
      (b)  (a) with one token of the longest row corrupted BEFORE any row's <eos>: retry rounds are running when the short row ends;
      (c)  (a) with one token of the longest row corrupted BEHIND the short rows' ends;
      (d)  right for every row up to the earliest <eos> step, rubbish behind it in all rows."""
    steps = em.eos_steps(gen)
    n = em.draft_span(gen, max_new)
    first = min(s for s in steps if s is not None)
    long_row = int(np.argmax([max_new if s is None else s for s in steps]))
    long_end = n if steps[long_row] is None else min(n, steps[long_row])
    a = em.filled_draft(gen, n, rng)
    out = {"(a) true continuations, random filler": a, "(a') true continuations, own last tokens repeated": em.filled_draft(gen, n, rng, repeat_last=True)}
    if len(steps) > 1:
        assert 1 <= first < long_end - 1, (steps, n)
        out["(b) one token wrong before the first <eos>"] = em.corrupt(a, long_row, first // 2)
        out["(c) one token wrong behind the short rows' ends"] = em.corrupt(a, long_row, long_end - 1)
    d = a.copy()
    d[:, first:] = rng.integers(0, em.EOS, size=d[:, first:].shape)
    out["(d) right up to the first <eos>, rubbish behind"] = d
    return out


def _drafts_past_eos(eng, b, what, strict_f32, bias=False):
    """One batch of tests/eos_model.py on `eng`: the plain call, its premise (which rows end where - asserted on the ENGINE's result),
    then every draft variant and a second plain call: length, ids (pad included), alignment rows and token timestamps are the plain
    call's.  Returns {variant: tw_last_draft figures}."""
    B = len(b.sel)
    pcm = em.audio(b.sel)
    prompt = em.prompt(b.sel)
    kw = em.engine_kw(b.timestamps)
    mel = eng.logmel(torch.from_numpy(pcm).cuda(), out_dtype=torch.float32)
    eng.encode(mel); eng.cross_kv(B)
    if bias:            # the list is derived from the UNBIASED run; the reference is the biased plain call
        kw["sequence_bias_rows"] = em.bias_rows(eng.generate_greedy(prompt, **kw)["sequences"][:, em.N_PROMPT:], b.es, b.timestamps)
    full = eng.generate_greedy(prompt, **kw)
    L, seq = full["length"], full["sequences"]
    nf = [2 * em.T] * B
    al = eng.get_alignment(B, L - 1)
    ts = eng.token_timestamps(B, em.N_PROMPT, L, nf)
    gen = seq[:, em.N_PROMPT:]
    steps = em.eos_steps(gen)
    print(f"\n{what}: rows end after {['-' if s is None else s for s in steps]} tokens, length {L}")
    em.check_batch(b, steps)
    longest = max(em.MAX_NEW if s is None else s + 1 for s in steps)
    assert L == em.N_PROMPT + min(em.MAX_NEW, longest), (what, "the length is set by the last <eos>", L, steps)
    for r, s in zip(gen, steps):
        assert s is None or (r[s:] == em.EOS).all(), (what, "a finished row is not padded")
    if strict_f32:
        if bias:
            from tests import bias_judge as bj
            dims, w = em.model(b.es)
            om = wo.OracleWhisper(dims, w, T=em.T)
            ref = bj.biased_greedy(om, om.encode(wo.log_mel(pcm, dims.n_mels)), prompt, em.options(b.timestamps), kw["sequence_bias_rows"])["sequences"]
            assert em.eos_steps(ref[:, em.N_PROMPT:]) == [em.BIAS_CASE[(b.es, b.timestamps)][1], None], what
        else:
            ref = em.oracle_run(b.es, b.timestamps, b.sel)
            assert steps == b.steps(), what
        assert np.array_equal(seq, ref), what
    figures = {}
    drafts = _past_eos_variants(gen, em.MAX_NEW, np.random.default_rng(11))
    for name, draft in drafts.items():
        out = eng.generate_greedy(np.concatenate([prompt, draft], axis=1), n_draft=draft.shape[1], **kw)
        w_ = f"{what}: draft = {name} ({draft.shape[1]} tokens)"
        dr = out["draft"]
        print(f"  {name}: {dr}")
        assert out["length"] == L, (w_, out["length"], L, dr)
        assert np.array_equal(out["sequences"], seq), (w_, dr, [(r, out["sequences"][r].tolist(), seq[r].tolist()) for r in range(B) if not np.array_equal(out["sequences"][r], seq[r])][:2])
        assert np.array_equal(eng.get_alignment(B, L - 1), al), w_
        assert np.array_equal(eng.token_timestamps(B, em.N_PROMPT, L, nf), ts), w_
        assert dr["offered"] == draft.shape[1] * B and dr["launches"] >= 1 and dr["rounds"] >= 1, (w_, dr)
        figures[name] = dr
    assert figures, what
    again = eng.generate_greedy(prompt, **kw)
    assert again["length"] == L and np.array_equal(again["sequences"], seq), what
    assert np.array_equal(eng.get_alignment(B, L - 1), al) and np.array_equal(eng.token_timestamps(B, em.N_PROMPT, L, nf), ts), what
    return figures


def _eos_engines(settings, B, dtype, graph):
    """One engine per <eos> scale among `settings` (the model differs), closed by the caller."""
    return {es: make_engine(*em.model(es), T=em.T, max_batch=B, dtype=dtype, heads=em.HEADS, use_graph=graph) for es in sorted({es for es, _ in settings})}


def _run_past_eos(prefix, B, dtype, graph, settings=None, **kw):
    settings = em.SETTINGS if settings is None else settings
    engines = _eos_engines(settings, B, dtype, graph)
    try:
        for es, ts_on in settings:
            b = em.batch(f"{prefix}-es{es}-ts{int(ts_on)}") if prefix != "b5" else em.batch("b5-all-end")
            _drafts_past_eos(engines[es], b, f"{b.name} {dtype} graph={graph}", strict_f32=(dtype == "f32"), **kw)
    finally:
        for e in engines.values():
            e.close()


@pytest.mark.parametrize("graph", [False, True])
def test_draft_past_eos_two_rows_one_ends_one_never(graph):
    """The smallest shape in which a draft is pending while a row reaches <eos>: clips 5 and 2 - row 0 ends after 6, 12 or 18 tokens,
    row 1 never - in strict f32 (plain ids = the oracle's).  Whatever stands behind row 0's end in its draft, the call returns the plain
    call's length, ids with row 0 padded, alignment rows and token timestamps."""
    _run_past_eos("b2", 2, "f32", graph)


def test_draft_past_eos_every_row_ends_at_another_step():
    """Clips 0, 1, 3, 4, 5 at <eos> scale 2.5: every row ends, each at another step, so the call's length is set by the last <eos>
    (17 tokens), not by max_new_tokens - with a draft as without."""
    _run_past_eos("b5", 5, "f32", True, settings=[(2.5, True)])


@pytest.mark.parametrize("dtype", ["bf16", "f16", "fp8a16", "fp8a8"])
def test_draft_past_eos_sixteen_rows_in_every_dtype(dtype):
    """Clips 0 .. 15 (fp8a8's cap of 16 rows: one position per verify launch).  The reference is the engine's own plain call in that
    type, and the premise - at least two different end steps, the earliest not before 3 tokens, some row that never ends - is
    asserted on it."""
    _run_past_eos("b16", 16, dtype, True)


def test_draft_past_eos_twenty_rows():
    """More than one group of 16 rows, three positions per first-round launch (bf16, the engine's own plain call as reference)."""
    _run_past_eos("b20", 20, "bf16", True)


def test_draft_past_eos_with_a_sequence_bias():
    """tw_generate_greedy_biased promises the same under n_draft: one short sequence on the row that ends, none on the other (strict
    f32; the biased plain call is the reference and equals the numpy statement of the rule, where the row ends after 32, 9 and 23 tokens)."""
    _run_past_eos("b2", 2, "f32", True, bias=True)


@pytest.mark.parametrize("graph", [False, True])
def test_draft_past_eos_one_row_ends_inside_the_verify_rounds(graph):
    """(e) B = 1: the true continuation followed by 1, 5 and 20 filler tokens behind the row's <eos> step - the call ends inside the
    verify rounds.  Every token before <eos> is confirmed, by at least one round."""
    engines = _eos_engines(em.SETTINGS, 1, "f32", graph)
    try:
        for es, ts_on in em.SETTINGS:
            b = em.batch(f"b1-es{es}-ts{int(ts_on)}")
            eng = engines[es]
            kw = em.engine_kw(ts_on)
            prompt = em.prompt(b.sel)
            eng.encode(eng.logmel(torch.from_numpy(em.audio(b.sel)).cuda(), out_dtype=torch.float32)); eng.cross_kv(1)
            full = eng.generate_greedy(prompt, **kw)
            L, seq = full["length"], full["sequences"]
            assert np.array_equal(seq, em.oracle_run(es, ts_on, b.sel))
            s = em.eos_steps(seq[:, em.N_PROMPT:])[0]
            print(f"\n{b.name} graph={graph}: the row ends after {s} tokens, length {L}")
            assert s == b.steps()[0] and s >= 3 and L == em.N_PROMPT + s + 1
            al, ts = eng.get_alignment(1, L - 1), eng.token_timestamps(1, em.N_PROMPT, L, [2 * em.T])
            rng = np.random.default_rng(13)
            for k in (1, 5, 20):
                for repeat in (False, True):
                    draft = em.filled_draft(np.concatenate([seq[:, em.N_PROMPT:], np.full((1, 20), em.EOS)], axis=1), s + k, rng, repeat_last=repeat)
                    out = eng.generate_greedy(np.concatenate([prompt, draft], axis=1), n_draft=s + k, **kw)
                    what = f"{b.name} graph={graph}: {k} filler tokens behind <eos>, repeat={repeat}"
                    dr = out["draft"]
                    print(f"  {k} filler tokens (repeat={repeat}): {dr}")
                    assert out["length"] == L and np.array_equal(out["sequences"], seq), (what, dr)
                    assert np.array_equal(eng.get_alignment(1, L - 1), al), what
                    assert np.array_equal(eng.token_timestamps(1, em.N_PROMPT, L, [2 * em.T]), ts), what
                    assert dr["offered"] == s + k and dr["accepted"] == s and dr["rounds"] >= 1, (what, dr)
            again = eng.generate_greedy(prompt, **kw)
            assert again["length"] == L and np.array_equal(again["sequences"], seq)
    finally:
        for e in engines.values():
            e.close()
