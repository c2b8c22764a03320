"""The repetition penalty and the no-repeat n-gram rule (tw_generate_greedy_repeat, tw_repeat_logits; k_decode.hip: repeat_kernel).

  1. bits: tw_repeat_logits on planted logits and histories equals HF's two processors on the CPU as raw 32-bit patterns;
  2. picks: on the crafted zero-layer models of tests/sampler_judge.py the sequence a call returned, fed back through `decode_step`,
     reproduces the raw logits its steps saw; tests/repeat_judge.py turns them into x' with HF's own processor classes and hands x' to
     `sampler_judge.judge`: no step wrong, at most 1 % undecided (the sampler suite's cap), every event of repeat_judge.EVENTS decisive
     in the ENGINE's run, the off row its row of the plain call, every row decoded alone its row of the batch;
  3. a row in which every unmasked id is banned returns id 0;
  4. n_forced and n_draft (true and corrupted drafts) return the processed plain call's ids and alignment rows;
  5. the trivial forms are the plain call; 6. every TW_EINVAL leaves the context usable; 7. the drop-in and the streaming backend.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_repeat.py -s`` prints each case's figures.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import repeat_judge as rj
from tests import sampler_judge as sj
from tests.util import PROMPT, clips, make_engine

pytestmark = pytest.mark.gpu
N_PROMPT = rj.N_PROMPT
TW_EINVAL = -1          # include/thewhisper.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _fill(eng, built, B):
    eng.encode(torch.zeros((B, built.dims.n_mels, 2 * sj.T_FRAMES), dtype=torch.float32).cuda())     # the zero-layer decoder never reads it
    eng.cross_kv(B)


def _engine(built, B=None):
    c = built.case
    B = B or c.B
    eng = make_engine(built.dims, built.weights, T=sj.T_FRAMES, max_batch=B, dtype=c.dtype, use_graph=c.graph)
    _fill(eng, built, B)
    return eng


def _replay(eng, seqs):
    B, L = seqs.shape
    eng.decoder_reset(B)
    return np.stack([eng.decode_step(seqs[:, s].tolist()).cpu().numpy() for s in range(L - 1)])


def _kw(rows, bias=None, ignore=rj.IGNORE):
    kw = dict(repetition_penalty=[r.penalty for r in rows], no_repeat_ngram_size=[r.ngram for r in rows], penalty_ignore=ignore)
    if bias is not None:
        kw["sequence_bias_rows"] = bias
    return kw


def _check(v, what):
    print(f"{what}: {v.summary()}")
    assert v.count("wrong") == 0, (what, v.wrong[:3])
    assert v.count("undecided") * 100 <= v.judged, (what, v.count("undecided"), v.judged)


def _rows_equal(a, b, pad):
    n = min(len(a), len(b))
    return np.array_equal(a[:n], b[:n]) and (a[n:] == pad).all() and (b[n:] == pad).all()


# ---- 1. bits ---------------------------------------------------------------------------------------------------------
def _planted_logits(rng, rows, V, hists):
    x = (rng.standard_normal((rows, V)) * 8.0).astype(np.float32)
    special = np.array([0.0, -0.0, -np.inf, 1e-42, -1e-42, 1.4e-45, 65504.0, -65504.0, 65503.99, -65503.99, 3e38, -3e38], np.float32)
    for r in range(rows):
        at = rng.choice(V, 3 * len(special), replace=False)
        x[r, at] = np.tile(special, 3)
        h = np.unique(hists[r])
        if h.size:                          # ... and on ids of the history, where the rule acts
            k = min(h.size, len(special))
            x[r, rng.choice(h, k, replace=False)] = rng.permutation(special)[:k]
    return x


@pytest.mark.parametrize("V", [51866, 1003])
def test_repeat_logits_equals_hfs_processors_bit_for_bit(V):
    built = rj.build(rj.REPEAT_CASES[0])
    eng = _engine(built)
    rng = np.random.default_rng(V)
    rows, ld = 3, 448
    pens = [1.1, 1.3, 0.7, 2.0, 1.0000001, 1.0]
    calls = differ = 0
    try:
        for N in (0, 1, 2, 3, 5):
            for lens in ((0, 1, 448), (max(N - 1, 0), N, 448), (448, 37, 5)):
                for ign_kind in (0, 2, "n"):
                    for mix in range(2):
                        hist = np.zeros((rows, ld), np.int32)
                        for r in range(rows):      # duplicates: a few ids only in one row, the whole vocabulary in another
                            hist[r] = rng.integers(0, (7, 40, V)[(r + mix) % 3], ld)
                        n_hist = np.array(lens, np.int32)
                        pen = [pens[(calls + r * (1 + mix)) % len(pens)] for r in range(rows)] if mix else [pens[calls % len(pens)]] * rows
                        ngr = [N] * rows if not mix else [N, (N + 1) % 4, 0]
                        ignore = int(n_hist.max()) if ign_kind == "n" else ign_kind
                        x = _planted_logits(rng, rows, V, [hist[r, : n_hist[r]] for r in range(rows)])
                        want = np.stack([rj.HFRepeat(rj.Row(pen[r], ngr[r]), ignore)(x[r], hist[r, : n_hist[r]]) for r in range(rows)])
                        got = eng.repeat_logits(torch.from_numpy(x).cuda(), hist, n_hist, repetition_penalty=pen, no_repeat_ngram_size=ngr,
                                                penalty_ignore=ignore).cpu().numpy()
                        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (V, N, lens, ignore, pen, ngr)
                        # the reciprocal form is another function: where it differs from HF the kernel has to side with HF
                        r32 = np.asarray(pen, np.float32)[:, None]
                        with np.errstate(all="ignore"):
                            recip = np.where(x < 0, x * r32, x * (np.float32(1.0) / r32))
                        differ += int(((recip != want) & (want != x) & np.isfinite(want)).sum())
                        calls += 1
    finally:
        eng.close()
    print(f"V={V}: {calls} calls; {differ} values where a reciprocal multiply would have differed")
    assert differ > 0, "the data must separate a correctly rounded division from a multiply by a reciprocal"


# ---- 2. picks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", [c.id for c in rj.REPEAT_CASES])
def test_picks_are_hfs_picks_from_the_engines_own_logits(case_id):
    rc = next(c for c in rj.REPEAT_CASES if c.id == case_id)
    built = rj.build(rc)
    rows, bias = rj.rows_of(rc.B), rj.bias_rows_of(built, rc.B)
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        seqs = eng.generate_greedy(built.prompt, **_kw(rows, bias), **built.kw)["sequences"]
        lg = _replay(eng, seqs)
        alone = []
        for b in range(rc.B):                              # every row alone, in slot 0, with its setting
            _fill(eng, built, 1)
            alone.append(eng.generate_greedy(built.prompt[b:b + 1], **_kw(rows[b:b + 1], bias[b:b + 1]), **built.kw)["sequences"][0])
    finally:
        eng.close()
    assert np.isfinite(lg).all() and np.array_equal(seqs[:, :N_PROMPT], built.prompt)
    v = rj.judge_repeat(lg, seqs, N_PROMPT, built.opt, rows, rj.IGNORE, bias)
    _check(v, case_id)
    assert v.judged == rc.B * (seqs.shape[1] - N_PROMPT)
    seen = rj.events_seen(rows, rj.IGNORE, seqs, lg, N_PROMPT, built.opt, bias)
    print(f"{case_id}: events {sorted(seen)}")
    assert set(rj.EVENTS) <= seen, (case_id, "events never decisive:", sorted(set(rj.EVENTS) - seen))
    off = rows.index(rj.OFF)
    assert _rows_equal(seqs[off], plain[off], built.opt.pad), "the off row is its row of the plain call"
    assert sum(not _rows_equal(seqs[b], plain[b], built.opt.pad) for b in range(rc.B)) >= min(4, rc.B - 1)
    for b, row in enumerate(alone):
        assert _rows_equal(row, seqs[b], built.opt.pad), f"row {b} decoded alone differs from its row of the batch"


# ---- 3. everything banned --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_a_row_with_every_unmasked_id_banned_returns_id_0(graph):
    built = sj.build_case(dataclasses.replace(sj.case_by_name("v127-no-timestamps"), B=2, graph=graph))
    V = built.dims.vocab
    keep = (3, 5, 9)                                       # the only ids the suppress list leaves; all of them in the prompt
    kw = dict(built.kw, suppress=tuple(i for i in range(V) if i not in keep), begin_suppress=(), max_new_tokens=6)
    prompt = np.array([keep, keep], np.int32)
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(prompt, **kw)["sequences"]
        got = eng.generate_greedy(prompt, no_repeat_ngram_size=[1, 0], **kw)["sequences"]
    finally:
        eng.close()
    assert set(plain[:, 3:].ravel().tolist()) <= set(keep)
    assert got.shape == plain.shape and (got[0, 3:] == 0).all(), got[0]
    assert np.array_equal(got[1], plain[1])


# ---- 4. drafts and forced tokens -------------------------------------------------------------------------------------
SB = [[[1705, 7], 50.0], [[9], -50.0]]


@pytest.mark.parametrize("what,opts", [("penalty", dict(repetition_penalty=1.3)), ("ngram", dict(no_repeat_ngram_size=2)),
                                       ("both-bias", dict(repetition_penalty=[1.3, 1.1, 2.0], no_repeat_ngram_size=[2, 3, 1], sequence_bias=SB))])
def test_forced_and_draft_calls_equal_the_processed_plain_call(what, opts):
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T, B, max_new = 100, 3, 40
    heads = [(dims.dec_layers - 1, 0), (dims.dec_layers - 1, 1)]
    eng = make_engine(dims, w, T=T, max_batch=B, dtype="f32", heads=heads, use_graph=(what != "ngram"))
    try:
        mel = eng.logmel(torch.from_numpy(clips(T * 320, B)).cuda(), out_dtype=torch.float32)
        eng.encode(mel); eng.cross_kv(B)
        prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
        kw = dict(max_new_tokens=max_new, min_new_tokens=max_new, timestamps=True, want_alignment=True, **opts)
        base = eng.generate_greedy(prompt, max_new_tokens=max_new, min_new_tokens=max_new, timestamps=True)["sequences"]
        full = eng.generate_greedy(prompt, **kw)
        L, seq = full["length"], full["sequences"]
        assert not np.array_equal(seq, base), "the options must change the ids"
        al = eng.get_alignment(B, L - 1)
        gen = seq[:, 3:]
        n_ok = max_new - 2
        variants = {"true": gen[:, :n_ok].copy()}
        for name, j in (("first", 0), ("middle", n_ok // 2), ("last", n_ok - 1)):
            d = gen[:, :n_ok].copy()
            d[:, j] = (d[:, j] + 7) % 50000
            variants[f"corrupted at the {name} position"] = d
        for name, draft in variants.items():
            out = eng.generate_greedy(np.concatenate([prompt, draft.astype(np.int32)], axis=1), n_draft=n_ok, **kw)
            assert out["length"] == L and np.array_equal(out["sequences"], seq), (what, name)
            assert np.array_equal(eng.get_alignment(B, L - 1), al), (what, name)
            assert out["draft"]["offered"] == n_ok * B and (out["draft"]["accepted"] == n_ok * B) == (name == "true"), (what, name, out["draft"])
        for n_forced in (1, 9):
            out = eng.generate_greedy(seq[:, : 3 + n_forced].astype(np.int32), n_forced=n_forced, **kw)
            assert out["length"] == L and np.array_equal(out["sequences"], seq), (what, "forced", n_forced)
            assert np.array_equal(eng.get_alignment(B, L - 1)[:, :, 3 + n_forced:], al[:, :, 3 + n_forced:]), (what, "forced", n_forced)
    finally:
        eng.close()


# ---- 5. / 6. the trivial forms and the refusals ----------------------------------------------------------------------
def _raw_call(eng, prompt, kw, ropts, bopts=None):
    """tw_generate_greedy_repeat itself: (rc, sequences, decode steps)."""
    prompt = np.ascontiguousarray(prompt, dtype=np.int32)
    B, n0 = prompt.shape
    o, _keep = eng._greedy_opts(kw["eos_id"], kw["pad_id"], kw["timestamps"], kw["no_timestamps_id"], kw["max_initial_timestamp_index"],
                                kw["begin_suppress"], kw["suppress"], kw["min_new_tokens"], kw["max_new_tokens"], 448)
    out = np.full((B, 448), kw["pad_id"], dtype=np.int32)
    n = C.c_int32(0)
    rc = eng.lib.tw_generate_greedy_repeat(eng.ctx, B, prompt.ctypes.data_as(C.POINTER(C.c_int32)), n0, C.byref(o),
                                           None if bopts is None else C.byref(bopts), None if ropts is None else C.byref(ropts),
                                           out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n), eng._sp())
    return rc, out[:, : int(n.value)].astype(np.int64), (eng.last_timings()["decode_steps"] if rc == 0 else None)


def _ropts(pen=None, ngr=None, ignore=0):
    from thewhisper_amd import _cabi

    ro = _cabi.tw_repeat_opts()
    ro._keep = (None if pen is None else np.asarray(pen, np.float32), None if ngr is None else np.asarray(ngr, np.int32))
    if pen is not None:
        ro.penalty = ro._keep[0].ctypes.data_as(C.POINTER(C.c_float))
    if ngr is not None:
        ro.no_repeat_ngram = ro._keep[1].ctypes.data_as(C.POINTER(C.c_int32))
    ro.penalty_ignore = ignore
    return ro


@pytest.mark.parametrize("graph", [False, True])
def test_trivial_forms_are_the_plain_call_and_every_refusal_leaves_the_context_usable(graph):
    built = rj.build(dataclasses.replace(rj.REPEAT_CASES[0], B=2, graph=graph))
    eng = _engine(built)
    sib = None
    try:
        plain = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        steps = eng.last_timings()["decode_steps"]
        for what, ro in (("NULL", None), ("null arrays", _ropts()), ("all rows off", _ropts([1.0, 1.0], [0, 0])),
                         ("all rows off, ignore set", _ropts([1.0, 1.0], None, 3))):
            rc, got, st = _raw_call(eng, built.prompt, built.kw, ro)
            assert rc == 0 and np.array_equal(got, plain) and st == steps, what
        assert np.array_equal(eng.generate_greedy(built.prompt, repetition_penalty=1.0, no_repeat_ngram_size=[0, 0], **built.kw)["sequences"], plain)
        rows = [rj.Row(2.0, 1), rj.OFF]
        rc, proc, _ = _raw_call(eng, built.prompt, built.kw, _ropts([2.0, 1.0], [1, 0]))
        assert rc == 0 and not np.array_equal(proc[0], plain[0][: proc.shape[1]]) and _rows_equal(proc[1], plain[1], built.opt.pad)
        P = built.dims.max_target_positions
        bad = {
            "a zero penalty": _ropts([0.0, 1.0]), "a negative penalty": _ropts([1.0, -1.3]), "a NaN penalty": _ropts([float("nan"), 1.0]),
            "an infinite penalty": _ropts([1.0, float("inf")]), "N < 0": _ropts(None, [0, -1]), "N > target_positions": _ropts(None, [P + 1, 0]),
            "penalty_ignore < 0": _ropts([1.3, 1.3], None, -1),
        }
        for what, ro in bad.items():
            rc, _, _ = _raw_call(eng, built.prompt, built.kw, ro)
            assert rc == TW_EINVAL, (what, rc)
            assert eng.lib.tw_last_error(eng.ctx), what
            assert np.array_equal(eng.generate_greedy(built.prompt, **built.kw)["sequences"], plain), f"the context after: {what}"
        rc, got, _ = _raw_call(eng, built.prompt, built.kw, _ropts(None, [P, 0]))      # N == target_positions is accepted (and never fires)
        assert rc == 0 and np.array_equal(got, plain)
        # the sibling context owns its own table: its result is the owner's
        sib = eng.sibling()
        _fill(sib, built, 2)
        got = sib.generate_greedy(built.prompt, **_kw(rows, ignore=0), **built.kw)["sequences"]
        assert np.array_equal(got, proc)
        assert np.array_equal(sib.generate_greedy(built.prompt, **built.kw)["sequences"], plain)
        assert np.array_equal(eng.generate_greedy(built.prompt, **_kw(rows, ignore=0), **built.kw)["sequences"], proc)
        with pytest.raises(ValueError):
            eng.generate_greedy(built.prompt, repetition_penalty=1.3, n_pad=[1, 0], **built.kw)
    finally:
        if sib is not None:
            sib.close()
        eng.close()


def test_more_than_64_streams_are_refused():
    built = rj.build(dataclasses.replace(rj.REPEAT_CASES[0], B=2))
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        rc, _, _ = _raw_call(eng, np.tile(built.prompt[:1], (65, 1)), built.kw, _ropts([1.3] * 65, None))
        assert rc == TW_EINVAL and b"65 streams" in eng.lib.tw_last_error(eng.ctx)
        assert np.array_equal(eng.generate_greedy(built.prompt, **built.kw)["sequences"], plain)
    finally:
        eng.close()


# ---- 7. layers above -------------------------------------------------------------------------------------------------
def test_dropin_generate_with_the_repeat_options_equals_hf_in_strict_f32():
    from oracle import hf_reference as hr
    from tests.test_gpu_bias import _micro_pipeline

    chunk_s = 10
    gk = {"num_beams": 1, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 48, "return_timestamps": True}
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), chunk_s)
    pipe = _micro_pipeline(chunk_s, 3)
    try:
        pcm = [wo.synth_audio(chunk_s * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
        feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        ids = lambda out: (out["sequences"] if isinstance(out, dict) else out).tolist()  # noqa: E731
        cpu = dict(input_features=feats.input_features.cpu(), attention_mask=feats.attention_mask.cpu())      # HF's model, on the CPU
        io = dict(input_features=feats.input_features.cuda(), attention_mask=feats.attention_mask.cuda())
        ref_plain = ids(hf.generate(**cpu, **gk))
        for kw in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.3, no_repeat_ngram_size=2),
                   dict(repetition_penalty=1.3, no_repeat_ngram_size=2, sequence_bias=SB)):
            ref = ids(hf.generate(**cpu, **gk, **kw))
            slow = ids(pipe.model.generate(**io, **gk, **kw))
            fast = ids(pipe.model.generate(**io, **gk, **kw))
            assert ref != ref_plain, kw
            assert slow == ref and fast == ref, kw
        assert ids(pipe.model.generate(**io, **gk)) == ref_plain
    finally:
        pipe.model.engine.close()


def test_backend_with_drafts_returns_the_words_of_the_backend_without_drafts():
    from tests.test_gpu_bias import _micro_pipeline
    from thewhisper_amd import AMDWhisperBackend

    chunk_s = 10
    pipe = _micro_pipeline(chunk_s, 1)
    try:
        audio = wo.synth_audio(8 * 16000, 3, "speechlike")
        ticks = (3 * 16000, 4 * 16000, 5 * 16000, 6 * 16000, 8 * 16000)
        words, stats = {}, {}
        for draft in (True, False):
            be = AMDWhisperBackend(None, chunk_length_s=chunk_s, asr_pipeline=pipe, repetition_penalty=1.3, no_repeat_ngram_size=2,
                                   draft_previous_tick=draft)
            be.transcribe(audio[:16000], 0.0, 16000)      # plan learning outside the compared calls
            be.reset()
            words[draft] = [be.transcribe(audio[:n], 0.0, 16000) for n in ticks]
            stats[draft] = dict(be.reuse_stats)
        plain = AMDWhisperBackend(None, chunk_length_s=chunk_s, asr_pipeline=pipe, draft_previous_tick=False)
        unprocessed = [plain.transcribe(audio[:n], 0.0, 16000) for n in ticks]
        print(f"repeat options with drafts: {stats[True]}")
        assert words[True] == words[False]
        assert stats[True]["draft_tokens"] > 0 and stats[True]["confirmed_tokens"] > 0
        assert unprocessed != words[False], "the options must change the transcript"
    finally:
        pipe.model.engine.close()
