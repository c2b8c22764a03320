"""Token timestamps of beam hypotheses on the device (tw_generate_beam_aligned, beam_align_gather_kernel, tw_token_timestamps_each)
against the stepped teacher-forced path (tw_decoder_reset + one tw_decode_step per token, which records the same alignment rows) and
tests/beam_align_judge.py, the numpy restatement that tests/test_beam_align_judge.py pins to HF decoding each clip alone.

  1. rows, bit for bit, f32 / f16 / bf16: after generate_beam(want_alignment=True) slot k n + c holds rows 0 .. len - 2 of hypothesis k
     of clip c, np.array_equal to the stepped pass over that hypothesis (clips re-encoded so that slot k n + c holds clip c); with
     use_graph; with the 58-token prompt of the reorder test; on a T = 99 engine (rows that do not start on 16-byte boundaries);
  2. ids and scores are those of want_alignment=False, bit for bit;
  3. timestamps: best and n-best bit-equal to tw_token_timestamps on the stepped rows of each hypothesis alone; f32 within one frame
     of the judge; unchanged by score_tokens; the same bits for a clip alone, in the 35-row call and in an 8-clip K = 3 call;
  4. tw_token_timestamps_each on injected surfaces: rows of different lengths and bounds, each bit-equal to the row alone;
  5. every new TW_EINVAL, with a plain greedy call after each;
  6. the HF seam and the pipeline on the real engine in strict f32.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_beam_align.py -s`` prints the figures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import align_surfaces as al
from tests import beam_align_judge as baj
from tests import beam_judge as bj
from tests import eos_model as em
from tests.util import clips, make_engine
from thewhisper_amd import _cabi

pytestmark = pytest.mark.gpu
TW_EINVAL = -1
FRAME_TOL = 0.0201          # one frame: the tolerance DESIGN.md section 6 states for the DTW
N0 = em.N_PROMPT
DTYPES = ["f32", "f16", "bf16"]
SEL = {"k5-ts": [0, 1, 2, 5, 6, 7, 8], "k3-ts-early": [0, 1, 2, 4, 5, 6, 8, 9]}     # 35 rows | 24 rows (test_gpu_beam.py's selections)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture(scope="module")
def engines():
    made = {}

    def get(es, dtype="f32", graph=False, max_batch=64, T=em.T, heads=True):
        key = (es, dtype, graph, max_batch, T, heads)
        if key not in made:
            dims, w = em.model(es)
            made[key] = make_engine(dims, w, T=T, max_batch=max_batch, dtype=dtype, heads=em.HEADS if heads else (), use_graph=graph)
        return made[key]

    yield get
    for e in made.values():
        e.close()


def _audio(sel, T):
    return em.audio(sel) if T == em.T else clips(T * 320, em.N_CLIPS)[list(sel)]


def _fill(eng, sel, T=em.T):
    eng.encode(eng.logmel(torch.from_numpy(_audio(sel, T)).cuda(), out_dtype=torch.float32))
    eng.cross_kv(len(sel))


def _bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def _beam(eng, sel, kw, prompt=None, T=em.T, want=True):
    """One aligned beam call: (result, alignment rows float32 [n K, Ha, Ln - 1, T] by slot)."""
    _fill(eng, sel, T)
    p = em.prompt(sel) if prompt is None else np.tile(np.asarray(prompt, dtype=np.int32), (len(sel), 1))
    res = eng.generate_beam(p, **kw, want_alignment=want)
    rows = eng.get_alignment(len(sel) * kw["num_beams"], res["nbest_sequences"].shape[2] - 1) if want else None
    return res, rows


def _stepped(eng, sel, res, K, T=em.T):
    """The parent commit's path to the same rows: slot k n + c holds clip c and is stepped through hypothesis k of clip c, token by
    token (a shorter hypothesis is fed its padding; those rows are not compared).  float32 [n K, Ha, Ln - 1, T]."""
    n = len(sel)
    nb = res["nbest_sequences"]
    _fill(eng, [sel[c] for _ in range(K) for c in range(n)], T)
    eng.decoder_reset(n * K)
    for p in range(nb.shape[2] - 1):
        eng.decode_step([int(nb[c, k, p]) for k in range(K) for c in range(n)], want_logits=False)
    return eng.get_alignment(n * K, nb.shape[2] - 1)


def _live(res):
    """(clip index, k, length) of every hypothesis that is not a placeholder."""
    n, K = res["nbest_scores"].shape
    return [(c, k, int(res["nbest_lengths"][c, k])) for c in range(n) for k in range(K) if res["nbest_scores"][c, k] > -1e9]


def _assert_rows(rows, ref, res, what):
    n, K = res["nbest_scores"].shape
    live = _live(res)
    assert len(live) >= n, what
    for c, k, L in live:
        assert L >= N0 + 1, (what, c, k, L)
        a, b = rows[k * n + c, :, : L - 1], ref[k * n + c, :, : L - 1]
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), (what, "clip", c, "hypothesis", k, "rows differ at positions",
                                                                    np.unique(np.nonzero(a != b)[1]).tolist())
    return len(live)


def _alone_timestamps(eng, ref_rows, res):
    """tw_token_timestamps on the stepped rows of each hypothesis ALONE (slot 0, its own seq_len): dict (c, k) -> float32 [len]."""
    n, K = res["nbest_scores"].shape
    out = {}
    for c, k, L in _live(res):
        eng.set_alignment(ref_rows[k * n + c : k * n + c + 1, :, : L - 1])
        out[(c, k)] = eng.token_timestamps(1, N0, L)[0]
    return out


@pytest.fixture(scope="module")
def runs(engines):
    """Per (case, dtype), computed once and shared: the plain and the aligned beam call, the gathered rows, the timestamps before and
    after a scoring pass, the stepped reference rows and the per-hypothesis timestamps on them."""
    made = {}

    def get(name, dtype):
        key = (name, dtype)
        if key in made:
            return made[key]
        case, sel = bj.case(name), SEL[name]
        kw = case.engine_kw()
        eng = engines(case.es, dtype)
        plain, _ = _beam(eng, sel, kw, want=False)
        res, rows = _beam(eng, sel, kw)
        ts_best, ts_nbest = eng.beam_token_timestamps(), eng.beam_token_timestamps(nbest=True)
        eng.score_tokens(res["sequences"], N0, **{k: v for k, v in kw.items() if k not in ("num_beams", "length_penalty", "early_stopping")})
        ts_after = eng.beam_token_timestamps(nbest=True)
        rows_after = eng.get_alignment(len(sel) * case.K, res["nbest_sequences"].shape[2] - 1)
        ref = _stepped(eng, sel, res, case.K)
        alone = _alone_timestamps(eng, ref, res)
        made[key] = dict(case=case, sel=sel, kw=kw, plain=plain, res=res, rows=rows, ts_best=ts_best, ts_nbest=ts_nbest, ts_after=ts_after,
                         rows_after=rows_after, ref=ref, alone=alone)
        return made[key]

    return get


# ---- 1. rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SEL))
def test_gathered_rows_equal_the_stepped_rows_bit_for_bit(engines, runs, name, dtype):
    r = runs(name, dtype)
    n_live = _assert_rows(r["rows"], r["ref"], r["res"], (name, dtype))
    lens = {L for _, _, L in _live(r["res"])}
    assert len(lens) > 1, (name, dtype, "every hypothesis has the same length")
    # the same with use_graph (beam steps are not captured; the context's greedy graphs stay as they are)
    g_res, g_rows = _beam(engines(r["case"].es, dtype, True), r["sel"], r["kw"])
    assert np.array_equal(g_res["nbest_sequences"], r["res"]["nbest_sequences"]), (name, dtype, "graph ids")
    _assert_rows(g_rows, r["ref"], r["res"], (name, dtype, "graph"))
    # tw_score_tokens left the rows alone
    _assert_rows(r["rows_after"], r["ref"], r["res"], (name, dtype, "after score_tokens"))
    print(f"{name} {dtype}: {n_live} hypotheses of lengths {sorted(lens)}: rows 0 .. len - 2 bit-equal to the stepped pass, graph on and off")


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_with_the_58_token_prompt(engines, dtype):
    """The reorder test's prompt: 58 prompt steps record rows too, and the paths cross the 64-key bucket boundary."""
    case = bj.Case("k3-long", 2.0, False, 3, False, 1.0, max_new=12)
    prompt = tuple(int(x) for x in np.random.default_rng(59).integers(0, 700, size=58))
    sel = [2, 3]
    eng = engines(case.es, dtype)
    res, rows = _beam(eng, sel, case.engine_kw(), prompt=prompt)
    if dtype == "f32":
        for i, c in enumerate(sel):
            assert [list(map(int, res["nbest_sequences"][i, k, : len(h)])) for k, h in enumerate(bj.run(case, c, prompt)["nbest"])] == \
                [list(h) for h in bj.run(case, c, prompt)["nbest"]]
    ref = _stepped(eng, sel, res, case.K)
    n, K = res["nbest_scores"].shape
    for c, k, L in _live(res):
        assert L >= 59
        assert np.array_equal(rows[k * n + c, :, : L - 1].view(np.int32), ref[k * n + c, :, : L - 1].view(np.int32)), (dtype, c, k)
    print(f"58-token prompt {dtype}: {len(_live(res))} hypotheses, rows bit-equal")


def test_rows_on_an_engine_whose_rows_are_not_16_byte_aligned(engines):
    """T = 99: a row is 396 bytes, so only every fourth row starts on a 16-byte boundary - the gather must take its scalar path."""
    case = bj.case("k5-ts")
    sel = [0, 1, 2, 5]
    eng = engines(case.es, "f32", False, 64, 99)
    res, rows = _beam(eng, sel, case.engine_kw(), T=99)
    assert rows.shape[3] == 99
    ref = _stepped(eng, sel, res, case.K, T=99)
    n_live = _assert_rows(rows, ref, res, "T=99")
    print(f"T = 99: {n_live} hypotheses, rows bit-equal")


# ---- 2. ids and scores ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SEL))
def test_ids_and_scores_are_those_of_the_plain_beam_call(runs, name, dtype):
    r = runs(name, dtype)
    for key in ("sequences", "scores", "nbest_sequences", "nbest_scores", "lengths", "nbest_lengths"):
        a, b = r["plain"][key], r["res"][key]
        assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (name, dtype, key)
    assert r["plain"]["length"] == r["res"]["length"]
    res = r["res"]
    for c in range(res["nbest_scores"].shape[0]):
        for k in range(res["nbest_scores"].shape[1]):
            L, row = int(res["nbest_lengths"][c, k]), res["nbest_sequences"][c, k]
            assert (row[L:] == em.EOS).all(), (name, dtype, c, k)
            if res["nbest_scores"][c, k] <= -1e9:
                assert L == N0, (name, dtype, c, k, L)
            else:
                gen = np.nonzero(row[N0:L] == em.EOS)[0]
                assert gen.size == 0 or gen[0] == L - N0 - 1, (name, dtype, c, k, "length is not the first <eos>")
    assert np.array_equal(res["lengths"], res["nbest_lengths"][:, 0])


# ---- 3. timestamps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SEL))
def test_timestamps_equal_the_per_hypothesis_call_on_the_stepped_rows(runs, name, dtype):
    r = runs(name, dtype)
    res, nb, best = r["res"], r["ts_nbest"], r["ts_best"]
    n, K = res["nbest_scores"].shape
    assert nb.shape == res["nbest_sequences"].shape and best.shape == res["sequences"].shape
    exact = total = 0
    for c in range(n):
        for k in range(K):
            L = int(res["nbest_lengths"][c, k])
            if (c, k) not in r["alone"]:
                assert not nb[c, k].any(), (name, dtype, c, k, "a placeholder's timestamps are zeros")
                continue
            want = baj.padded(r["alone"][(c, k)], nb.shape[2])
            assert np.array_equal(nb[c, k].view(np.int32), want.view(np.int32)), (name, dtype, c, k, nb[c, k].tolist(), want.tolist())
            if k == 0:
                assert np.array_equal(best[c].view(np.int32), want[: best.shape[1]].view(np.int32)), (name, dtype, c, "best")
            if dtype == "f32":        # ... and the judge (HF decoding the clip alone), within one frame
                ref = baj.run(r["case"], r["sel"][c])
                assert list(res["nbest_sequences"][c, k, :L]) == list(ref["nbest"][k]), (name, c, k)
                d = np.abs(nb[c, k, :L].astype(np.float64) - ref["timestamps"][k].astype(np.float64))
                assert d.max() <= FRAME_TOL, (name, c, k, nb[c, k, :L].tolist(), ref["timestamps"][k].tolist())
                exact += int((d[N0:] <= 1e-6).sum())
                total += L - N0
    assert np.array_equal(r["ts_after"].view(np.int32), nb.view(np.int32)), (name, dtype, "timestamps moved under score_tokens")
    if dtype == "f32":
        print(f"{name} f32: {exact} of {total} generated tokens ({100.0 * exact / max(total, 1):.1f} %) exactly the judge's, all within one frame")


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_clips_timestamps_do_not_depend_on_its_batch(engines, runs, dtype):
    """A clip alone (K = 5), in the 35-row call; and K = 3: alone against the 8-clip call."""
    for name in SEL:
        r = runs(name, dtype)
        eng = engines(r["case"].es, dtype)
        for i in (0, len(r["sel"]) - 1, 3):
            one, rows1 = _beam(eng, [r["sel"][i]], r["kw"])
            ts1 = eng.beam_token_timestamps(nbest=True)[0]
            assert np.array_equal(one["nbest_lengths"][0], r["res"]["nbest_lengths"][i]), (name, dtype, i)
            for k in range(r["case"].K):
                L = int(one["nbest_lengths"][0, k])
                assert np.array_equal(ts1[k, :L].view(np.int32), r["ts_nbest"][i, k, :L].view(np.int32)), (name, dtype, i, k)
                if one["nbest_scores"][0, k] > -1e9:
                    n = len(r["sel"])
                    assert np.array_equal(rows1[k, :, : L - 1].view(np.int32), r["rows"][k * n + i, :, : L - 1].view(np.int32)), (name, dtype, i, k)


# ---- 4. tw_token_timestamps_each on injected surfaces --------------------------------------------------------------------------
def test_each_on_injected_surfaces_equals_every_row_alone():
    dims = wo.PRESETS["micro"]
    heads = [(1, 0), (1, 1)]
    T, P = 300, dims.max_target_positions
    eng = make_engine(dims, wo.make_weights(dims, 0), T=T, max_batch=8, dtype="f32", heads=heads)
    try:
        n_max = P - 1 - 3
        # (N_b, num_frames): N = 0, 1 and the maximum; all columns, a cropped bound, a bound of 0 columns, a negative bound
        spec = [(0, None), (1, None), (n_max, None), (16, 2 * 57), (23, 1), (32, -2 * 120), (7, 2 * 300 + 5), (48, 2 * 133 + 1)]
        surf = [al.surface(al.Case(f"each{i}", Ha=2, N=max(N, 1), M=T, T=T, kind="peaky" if i % 2 else "diffuse", seed=900 + i))
                for i, (N, _) in enumerate(spec)]
        lens = [3 + N + 1 for N, _ in spec]
        frames = [2 * T if f is None else f for _, f in spec]
        buf = np.full((len(spec), 2, P, T), np.nan, dtype=np.float32)                        # NaN behind every row's own rows
        for i, (N, _) in enumerate(spec):
            buf[i, :, : 3 + N] = surf[i][:, : 3 + N]
        eng.set_alignment(buf)
        ld = max(lens) + 3
        got = eng.token_timestamps_each(lens, 3, frames, ld=ld)
        assert got.shape == (len(spec), ld)
        for i, L in enumerate(lens):
            eng.set_alignment(buf[i : i + 1])
            want = eng.token_timestamps(1, 3, L, [frames[i]])[0]
            assert np.array_equal(got[i, :L].view(np.int32), want.view(np.int32)), (i, spec[i], got[i, :L].tolist(), want.tolist())
            assert (got[i, L:] == want[-1]).all() and not got[i, :3].any(), (i, spec[i])
        assert not got[0].any()                                              # N = 0: zeros
        assert (got[4, 3:] == np.float32(-0.02)).all()                       # 0 columns kept: HF's DTW on the empty matrix
        # N_b < 0 (a placeholder: nothing behind the prompt) is zeros, whatever its neighbours hold
        eng.set_alignment(buf)
        short = eng.token_timestamps_each([3, 2, 0, lens[3]], 3, None, ld=lens[3])
        assert not short[:3].any()
        eng.set_alignment(buf[3:4])
        assert np.array_equal(short[3].view(np.int32), eng.token_timestamps(1, 3, lens[3])[0].view(np.int32))
        # every length equal: the call is tw_token_timestamps
        same = [al.surface(al.Case(f"same{i}", Ha=2, N=24, M=T, T=T, kind="peaky", seed=950 + i)) for i in range(5)]
        eng.set_alignment(np.stack(same))
        fr = [2 * T, 2 * 80, 2 * 211 + 1, -100, 0]
        a = eng.token_timestamps(5, 3, 28, fr)
        b = eng.token_timestamps_each([28] * 5, 3, fr)
        assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        eng.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------
def _raw_beam_aligned(eng, n, prompt, K=3, lp=1.0, early=0, max_length=448, **opt_over):
    kw = dict(eos_id=em.EOS, pad_id=em.EOS, timestamps=False, no_timestamps_id=em.NO_TS, max_initial_timestamp_index=None,
              begin_suppress=(), suppress=(), min_new_tokens=0, max_new_tokens=6, max_length=max_length)
    extra = {k: opt_over.pop(k) for k in ("want_alignment", "n_forced", "n_draft") if k in opt_over}
    kw.update(opt_over)
    o, _keep = eng._greedy_opts(**kw, **extra)
    bo = _cabi.tw_beam_opts()
    bo.num_beams, bo.length_penalty, bo.early_stopping = K, lp, early
    prompt = np.ascontiguousarray(prompt, dtype=np.int32)
    out = np.zeros((n, max_length), np.int32)
    out_len = (C.c_int32 * 2)()
    i32p = C.POINTER(C.c_int32)
    return eng.lib.tw_generate_beam_aligned(eng.ctx, n, prompt.ctypes.data_as(i32p), prompt.shape[1], C.byref(o), C.byref(bo),
                                            out.ctypes.data_as(i32p), out_len, None, None, None, None, eng._sp())


def _raw_each(eng, lens, n_prompt, ld):
    lens = np.ascontiguousarray(lens, dtype=np.int32)
    out = np.zeros((len(lens), max(ld, 1)), np.float32)
    return eng.lib.tw_token_timestamps_each(eng.ctx, len(lens), n_prompt, lens.ctypes.data_as(C.POINTER(C.c_int32)), ld, None, 0.02,
                                            out.ctypes.data_as(C.POINTER(C.c_float)), eng._sp())


def test_refusals_leave_the_context_usable(engines):
    sel = [0, 1, 5]
    p = em.prompt(sel)
    for heads in (True, False):
        eng = engines(2.5, "f32", False, 12, em.T, heads)
        _fill(eng, sel)
        gkw = dict(em.engine_kw(True, 8), want_alignment=heads)
        usual = eng.generate_greedy(p, **gkw)["sequences"]
        bad = [("num_beams 1", dict(K=1)), ("num_beams 9", dict(K=9)), ("rows above max_batch", dict(K=5)),
               ("nan length_penalty", dict(lp=float("nan"))), ("early_stopping 2", dict(early=2)), ("n_forced", dict(n_forced=1)),
               ("n_draft", dict(n_draft=1)), ("nothing to generate", dict(max_new_tokens=0))]
        if not heads:
            bad.append(("want_alignment without alignment heads", dict(want_alignment=True)))
        for what, over in bad:
            for want in ((False, True) if heads else (False,)):
                rc = _raw_beam_aligned(eng, len(sel), p, **dict({"want_alignment": want}, **over))
                assert rc == TW_EINVAL, (what, want, rc, eng.lib.tw_last_error(eng.ctx))
                assert np.array_equal(eng.generate_greedy(p, **gkw)["sequences"], usual), what
        P = em.model(2.5)[0].max_target_positions
        each_bad = [("a length above ld", ([5, 9], 3, 8)), ("a length above target_positions", ([5, P + 1], 3, P + 2)),
                    ("n_prompt 0", ([5, 6], 0, 8)), ("ld 0", ([0, 0], 3, 0))]
        for what, (lens, n0, ld) in each_bad:
            rc = _raw_each(eng, lens, n0, ld)
            assert rc == TW_EINVAL, (what, heads, rc, eng.lib.tw_last_error(eng.ctx))
            assert np.array_equal(eng.generate_greedy(p, **gkw)["sequences"], usual), what
        if not heads:
            assert _raw_each(eng, [5, 6], 3, 8) == TW_EINVAL               # a context without alignment heads
        else:
            assert _raw_each(eng, [5, 6], 3, 8) == 0
            assert _raw_beam_aligned(eng, len(sel), p, K=4, want_alignment=True) == 0      # 12 rows: exactly max_batch
        assert np.array_equal(eng.generate_greedy(p, **gkw)["sequences"], usual)


# ---- 6. the HF seam and the pipeline on the device ------------------------------------------------------------------------------
def test_dropin_beam_token_timestamps_against_hf_in_strict_f32():
    """Both flags on: generate(num_beams=3, return_token_timestamps=True) on the real engine returns HF's ids, and every row's token
    timestamps lie within one frame of HF's for that clip decoded alone; the pipeline returns HF's words."""
    from oracle import hf_reference as hr
    from thewhisper_amd import ASRPipeline

    chunk_s = 10
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), chunk_s)
    pipe = ASRPipeline(hr.build_hf_model(dims, wo.make_weights(dims, 0)), feature_extractor=hr.build_feature_extractor(dims, chunk_s),
                       tokenizer=hr.build_tokenizer(dims), chunk_length_s=chunk_s, device="cuda", torch_dtype=torch.float32, batch_size=9)
    try:
        pcm = [wo.synth_audio(chunk_s * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
        feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        gk = {"num_beams": 3, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 12, "return_timestamps": True,
              "return_token_timestamps": True}
        io = dict(input_features=feats.input_features.cuda(), attention_mask=feats.attention_mask.cuda())
        pipe.model.beam_search = True
        with pytest.raises(NotImplementedError, match="return_token_timestamps with num_beams > 1"):
            pipe.model.generate(**io, **gk)
        pipe.model.beam_token_timestamps = True
        out = pipe.model.generate(**io, **gk)
        seq, ts = out["sequences"].cpu().numpy(), out["token_timestamps"].cpu().numpy()
        worst = 0.0
        for i in range(3):
            ref = hf.generate(input_features=feats.input_features[i : i + 1].cpu(), attention_mask=feats.attention_mask[i : i + 1].cpu(), **gk)
            ids, rts = ref["sequences"][0].numpy(), ref["token_timestamps"][0].numpy()
            L = len(ids)
            assert seq[i, :L].tolist() == ids.tolist() and (seq[i, L:] == pipe.model.generation_config.pad_token_id).all(), i
            d = float(np.abs(ts[i, :L] - rts).max())
            worst = max(worst, d)
            assert d <= FRAME_TOL, (i, ts[i, :L].tolist(), rts.tolist())
        print(f"seam: ids equal HF's, token timestamps within {worst:.4f} s of HF's per-clip result")
        from transformers import pipeline as hf_pipeline

        ref_pipe = hf_pipeline("automatic-speech-recognition", model=hf, tokenizer=pipe.tokenizer,
                               feature_extractor=hr.build_feature_extractor(dims, chunk_s), device="cpu")
        pk = {k: v for k, v in gk.items() if k not in ("return_timestamps", "return_token_timestamps")}
        got = pipe(pcm[0], return_timestamps="word", generate_kwargs=dict(pk))
        want = ref_pipe(pcm[0], return_timestamps="word", generate_kwargs=dict(pk))
        assert got["text"] == want["text"]
        assert [c["text"] for c in got["chunks"]] == [c["text"] for c in want["chunks"]]
        for a, b in zip(got["chunks"], want["chunks"]):
            for x, y in zip(a["timestamp"], b["timestamp"]):
                assert (x is None) == (y is None) and (x is None or abs(x - y) <= FRAME_TOL), (a, b)
    finally:
        pipe.model.engine.close()
