"""The per-stream sequence bias (tw_generate_greedy_biased; k_decode.hip: seq_bias_kernel) judged on the engine's OWN logits.

On the crafted zero-layer models of tests/sampler_judge.py the sequence a call returned, fed back through `decode_step`, reproduces the
raw logits x its steps saw.  tests/bias_judge.py turns them into x' with HF's own SequenceBiasLogitsProcessor - per step and row, from
that row's history and that row's list - and hands x' to `sampler_judge.judge`: every appended token must be the one HF's processors +
argmax pick from x'.  The lists are grown from the engine's own runs (`bias_judge.build_lists`), one event at a time, each margin at
least 1.5 over the gap it closes; every case asserts
  * no step wrong, at most 1 % undecided (the sampler suite's cap);
  * every event of the case decisive in the ENGINE's run (`bias_judge.events_seen`, recomputed from the final run through HF): a
    length-1 positive bias, a length-1 negative bias removing the winner, a sequence of length >= 3, two sequences onto one id neither of
    which decides alone, a bias on a timestamp id that flips the mass rule, a bias on a suppressed id that changes nothing, and a
    sequence of length n_prompt + 1 whose prefix is the whole prompt, which must NOT be applied at the first step;
  * the row without a list equals its row of the plain call; every row decoded alone at B = 1 with its list equals its row of the batch.
Further: the bit-level order of the sum, n_forced / n_draft (true and corrupted drafts), the n_seq = 0 and NULL forms, every TW_EINVAL,
the drop-in against HF on the micro model in strict f32, and the streaming backend's hotwords with drafts on.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_bias.py -s`` prints each case's figures.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from tests import bias_judge as bj
from tests import sampler_judge as sj
from tests.util import make_engine

pytestmark = pytest.mark.gpu
N_PROMPT = 3
TW_EINVAL = -1          # include/thewhisper.h


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _engine(built, B=None):
    c = built.case
    B = B or c.B
    eng = make_engine(built.dims, built.weights, T=sj.T_FRAMES, max_batch=B, dtype=c.dtype, use_graph=c.graph)
    _fill(eng, built, B)
    return eng


def _fill(eng, built, B):
    eng.encode(torch.zeros((B, built.dims.n_mels, 2 * sj.T_FRAMES), dtype=torch.float32).cuda())     # the zero-layer decoder never reads it
    eng.cross_kv(B)


def _replay(eng, seqs):
    B, L = seqs.shape
    eng.decoder_reset(B)
    return np.stack([eng.decode_step(seqs[:, s].tolist()).cpu().numpy() for s in range(L - 1)])


def _runner(eng, built, prompt=None, **extra):
    prompt = built.prompt if prompt is None else prompt

    def run(rows):
        seqs = eng.generate_greedy(prompt, sequence_bias_rows=rows, **built.kw, **extra)["sequences"]
        return seqs, _replay(eng, seqs)

    return run


def _check(v, what):
    print(f"{what}: {v.summary()}")
    assert v.count("wrong") == 0, (what, v.wrong[:3])
    assert v.count("undecided") * 100 <= v.judged, (what, v.count("undecided"), v.judged)


def _rows_equal(a, b, pad):
    """Two results of the same row from calls of different common length: equal where both have tokens, padding behind."""
    n = min(len(a), len(b))
    return np.array_equal(a[:n], b[:n]) and (a[n:] == pad).all() and (b[n:] == pad).all()


@pytest.mark.parametrize("case_id", [c.id for c in bj.BIAS_CASES])
def test_biased_picks_are_hfs_picks_from_the_engines_own_logits(case_id):
    bc = next(c for c in bj.BIAS_CASES if c.id == case_id)
    built = bj.build(bc)
    eng = _engine(built)
    try:
        run = _runner(eng, built)
        plain, _ = run([None] * bc.B)
        rows, events, seqs, lg = bj.build_lists(run, built, N_PROMPT, bc.expect)
        alone = []
        if bc.B > 1:
            for b in range(bc.B):                              # every row alone, in slot 0, with its list
                _fill(eng, built, 1)
                alone.append(eng.generate_greedy(built.prompt[b:b + 1], sequence_bias_rows=[rows[b]], **built.kw)["sequences"][0])
    finally:
        eng.close()
    assert np.isfinite(lg).all() and np.array_equal(seqs[:, :N_PROMPT], built.prompt)
    v = bj.judge_biased(lg, seqs, N_PROMPT, built.opt, rows)
    _check(v, case_id)
    assert v.judged == bc.B * (seqs.shape[1] - N_PROMPT)
    seen = bj.events_seen(events, rows, seqs, lg, N_PROMPT, built.opt)
    print(f"{case_id}: events {sorted(seen)}; sequences per row {[len(r) if r else 0 for r in rows]}")
    assert set(bc.expect) <= seen, (case_id, "events never decisive:", sorted(set(bc.expect) - seen))
    listed = bj.listed_rows(bc.B)
    assert len({tuple(sorted(rows[b].items())) for b in listed}) == len(listed), "lists differ per row"
    for b in range(bc.B):
        if b not in listed:
            assert rows[b] is None and _rows_equal(seqs[b], plain[b], built.opt.pad), "the row without a list is its row of the plain call"
        else:
            assert not _rows_equal(seqs[b], plain[b], built.opt.pad)
    for b, row in enumerate(alone):
        assert _rows_equal(row, seqs[b], built.opt.pad), f"row {b} decoded alone differs from its row of the batch"


def test_the_sum_runs_in_list_order_bit_for_bit():
    """A planted duplicate pair (bit-equal logits): lo gets three active sequences, hi the single float32 (b1 + b2) + b3; b1 + (b2 + b3) is
    one ulp smaller.  Summed in list order - the length-1 member first although it is listed last - the tie survives and lo wins."""
    built = bj.build(bj.BIAS_CASES[0])
    eng = _engine(built)
    try:
        run = _runner(eng, built)
        plain, _ = run([None] * built.case.B)
        lo, hi, lst = bj.sum_order_lists(built, plain, N_PROMPT)
        rows = [lst] + [None] * (built.case.B - 1)
        seqs, lg = run(rows)
    finally:
        eng.close()
    s = N_PROMPT - 1
    assert lg[s, 0, lo] == lg[s, 0, hi], "the duplicated rows must be bit-equal columns of the logits"
    x1 = bj.HFBias(lst)(lg[s, 0], seqs[0, :N_PROMPT])
    assert x1[lo] == x1[hi] == x1.max() and lo < hi
    assert int(seqs[0, N_PROMPT]) == lo, (int(seqs[0, N_PROMPT]), lo, hi)
    _check(bj.judge_biased(lg, seqs, N_PROMPT, built.opt, rows), "sum order")
    assert all(_rows_equal(seqs[b], plain[b], built.opt.pad) for b in range(1, built.case.B))


@pytest.mark.parametrize("graph", [False, True])
def test_forced_and_draft_calls_equal_the_biased_plain_call(graph):
    bc = dataclasses.replace(bj.BIAS_CASES[0], graph=graph)
    built = bj.build(bc)
    eng = _engine(built)
    try:
        rows, events, plain, lg = bj.build_lists(_runner(eng, built), built, N_PROMPT, bc.expect)
        v = bj.judge_biased(lg, plain, N_PROMPT, built.opt, rows)
        _check(v, f"biased plain graph={graph}")
        gen = plain[:, N_PROMPT:]
        n_ok = min(int(np.argmax(np.append(r == built.opt.eos, True))) for r in gen)       # tokens before any row's eos / padding
        n_ok = min(n_ok, bj.MAX_NEW - 2)
        # an event whose match lies inside the draft, as late as the draft allows: its context tokens are draft tokens
        inside = [e for e in events if e.kind in ("len3", "two_onto_one", "ts_flip") and N_PROMPT + 1 <= e.step < N_PROMPT + n_ok - 1]
        assert inside, ("no conditional event inside the draft", n_ok, [(e.kind, e.step) for e in events])
        ev = max(inside, key=lambda e: e.step)
        n_forced = ev.step + 1 - N_PROMPT                      # the forced prefix ends with the event's context: the match is on forced tokens
        calls = {"forced": (plain[:, : N_PROMPT + n_forced], dict(n_forced=n_forced))}
        draft = plain[:, : N_PROMPT + n_ok].copy()
        calls["draft, all correct"] = (draft, dict(n_draft=n_ok))
        bad = draft.copy()
        bad[ev.row, ev.step] = 1 if bad[ev.row, ev.step] != 1 else 2      # the last context token of an active match
        calls["draft, one token corrupted inside an active match"] = (bad, dict(n_draft=n_ok))
        for what, (prompt, kw) in calls.items():
            out = eng.generate_greedy(prompt.astype(np.int32), sequence_bias_rows=rows, **built.kw, **kw)
            assert np.array_equal(out["sequences"], plain), what
            if "n_draft" in kw:
                dr = out["draft"]
                assert dr["offered"] == n_ok * bc.B, (what, dr)
                assert (dr["accepted"] == n_ok * bc.B) == (prompt is draft), (what, dr)
            lg2 = _replay(eng, out["sequences"])
            assert np.array_equal(lg2, lg), what
            _check(bj.judge_biased(lg2, out["sequences"], N_PROMPT, built.opt, rows), f"{what} graph={graph}")
    finally:
        eng.close()


def _raw_call(eng, prompt, kw, bopts):
    """tw_generate_greedy_biased itself: (rc, sequences)."""
    from thewhisper_amd import _cabi

    prompt = np.ascontiguousarray(prompt, dtype=np.int32)
    B, n0 = prompt.shape
    o, _keep = eng._greedy_opts(kw["eos_id"], kw["pad_id"], kw["timestamps"], kw["no_timestamps_id"], kw["max_initial_timestamp_index"],
                                kw["begin_suppress"], kw["suppress"], kw["min_new_tokens"], kw["max_new_tokens"], 448)
    out = np.full((B, 448), kw["pad_id"], dtype=np.int32)
    n = C.c_int32(0)
    rc = eng.lib.tw_generate_greedy_biased(eng.ctx, B, prompt.ctypes.data_as(C.POINTER(C.c_int32)), n0, C.byref(o),
                                           None if bopts is None else C.byref(bopts), out.ctypes.data_as(C.POINTER(C.c_int32)),
                                           C.byref(n), eng._sp())
    return rc, out[:, : int(n.value)].astype(np.int64)


def _bopts(row_off, seq_off, tokens, bias, n_seq=None):
    from thewhisper_amd import _cabi

    keep = [np.asarray(row_off, np.int32), np.asarray(seq_off, np.int32), np.asarray(tokens if len(tokens) else [0], np.int32),
            np.asarray(bias if len(bias) else [0], np.float32)]
    bo = _cabi.tw_bias_opts()
    bo.n_seq = len(bias) if n_seq is None else n_seq
    bo.row_off, bo.seq_off, bo.tokens = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep[:3])
    bo.bias = keep[3].ctypes.data_as(C.POINTER(C.c_float))
    bo._keep = keep
    return bo


def test_no_sequences_is_the_plain_call_and_every_refusal_leaves_the_context_usable():
    from thewhisper_amd import _cabi

    built = bj.build(dataclasses.replace(bj.BIAS_CASES[0], B=2))
    V = built.dims.vocab
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        for what, bo in (("NULL", None), ("n_seq = 0", _bopts([0, 0, 0], [0], [], [])), ("n_seq = 0, null arrays", _cabi.tw_bias_opts())):
            rc, got = _raw_call(eng, built.prompt, built.kw, bo)
            assert rc == 0 and np.array_equal(got, plain), what
        assert np.array_equal(eng.generate_greedy(built.prompt, sequence_bias_rows=[None, []], **built.kw)["sequences"], plain)
        many = 16385
        bad = {
            "row_off does not start at 0": _bopts([1, 1, 1], [0, 1], [5], [1.0]),
            "row_off decreases": _bopts([0, 2, 1], [0, 1, 2], [5, 6], [1.0, 1.0]),
            "row_off does not end at n_seq": _bopts([0, 1, 1], [0, 1, 2], [5, 6], [1.0, 1.0]),
            "seq_off does not start at 0": _bopts([0, 1, 1], [1, 2], [5, 6], [1.0]),
            "an empty sequence": _bopts([0, 2, 2], [0, 1, 1], [5], [1.0, 1.0]),
            "seq_off decreases": _bopts([0, 2, 2], [0, 2, 1], [5, 6], [1.0, 1.0]),
            "a sequence of 33 tokens": _bopts([0, 1, 1], [0, 33], [5] * 33, [1.0]),
            "a token == V": _bopts([0, 1, 1], [0, 2], [5, V], [1.0]),
            "a negative token": _bopts([0, 1, 1], [0, 2], [-1, 5], [1.0]),
            "a NaN bias": _bopts([0, 1, 1], [0, 1], [5], [float("nan")]),
            "an infinite bias": _bopts([0, 1, 1], [0, 1], [5], [float("inf")]),
            "the same sequence twice in one row": _bopts([0, 2, 2], [0, 2, 4], [5, 6, 5, 6], [1.0, 2.0]),
            "more than 16384 sequences": _bopts([0, many, many], list(range(many + 1)), [5 + (i % 900) for i in range(many)], [1.0] * many),
            "more than 65536 tokens": _bopts([0, 2049, 2049], [32 * i for i in range(2050)], [5 + (i % 900) for i in range(32 * 2049)],
                                              [1.0] * 2049),
            "a negative n_seq": _bopts([0, 0, 0], [0], [], [], n_seq=-1),
        }
        for what, bo in bad.items():
            rc, _ = _raw_call(eng, built.prompt, built.kw, bo)
            assert rc == TW_EINVAL, (what, rc)
            assert eng.lib.tw_last_error(eng.ctx), what
            assert np.array_equal(eng.generate_greedy(built.prompt, **built.kw)["sequences"], plain), f"the context after: {what}"
        # the same sequence in two DIFFERENT rows is fine, and the full capacities are accepted
        rc, _ = _raw_call(eng, built.prompt, built.kw, _bopts([0, 1, 2], [0, 2, 4], [5, 6, 5, 6], [1.0, 2.0]))
        assert rc == 0
        n = 16384
        rc, got = _raw_call(eng, built.prompt, built.kw, _bopts([0, n, n], [4 * i for i in range(n + 1)],
                                                               [(i * 7 + j) % 600 + 1 for i in range(n) for j in (0, i // 600, 2, 3)], [1e-3] * n))
        assert rc == 0 and got.shape[0] == 2 and np.array_equal(got[:, :N_PROMPT], built.prompt)
        assert np.array_equal(eng.generate_greedy(built.prompt, **built.kw)["sequences"], plain)
        with pytest.raises(ValueError):
            eng.generate_greedy(built.prompt, sequence_bias={(5,): 1.0}, sequence_bias_rows=[None, None], **built.kw)
    finally:
        eng.close()


def _micro_pipeline(chunk_s, batch_size, dtype=torch.float32):
    from oracle import hf_reference as hr
    from oracle import whisper_oracle as wo
    from thewhisper_amd import ASRPipeline

    dims = wo.PRESETS["micro"]
    model = hr.build_hf_model(dims, wo.make_weights(dims, 0))
    return ASRPipeline(model, feature_extractor=hr.build_feature_extractor(dims, chunk_s), tokenizer=hr.build_tokenizer(dims),
                       chunk_length_s=chunk_s, device="cuda", torch_dtype=dtype, batch_size=batch_size)


def test_dropin_generate_with_sequence_bias_equals_hf_in_strict_f32():
    from oracle import hf_reference as hr
    from oracle import whisper_oracle as wo

    chunk_s = 10
    sb = [[[1705, 7], 50.0], [[9], -50.0]]
    gk = {"num_beams": 1, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 16, "return_timestamps": True}
    dims = wo.PRESETS["micro"]
    hf = hr.patch_chunk_length(hr.build_hf_model(dims, wo.make_weights(dims, 0)), chunk_s)
    pipe = _micro_pipeline(chunk_s, 3)
    try:
        pcm = [wo.synth_audio(chunk_s * 16000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
        feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
        ids = lambda out: (out["sequences"] if isinstance(out, dict) else out).tolist()  # noqa: E731
        cpu = dict(input_features=feats.input_features.cpu(), attention_mask=feats.attention_mask.cpu())      # HF's model, on the CPU
        ref = ids(hf.generate(**cpu, **gk, sequence_bias=sb))
        ref_plain = ids(hf.generate(**cpu, **gk))
        io = dict(input_features=feats.input_features.cuda(), attention_mask=feats.attention_mask.cuda())
        slow = ids(pipe.model.generate(**io, **gk, sequence_bias=sb))
        fast = ids(pipe.model.generate(**io, **gk, sequence_bias=sb))
        assert ref != ref_plain
        assert slow == ref and fast == ref
        assert ids(pipe.model.generate(**io, **gk)) == ref_plain
    finally:
        pipe.model.engine.close()


def test_backend_hotwords_with_drafts_return_the_words_of_the_backend_without_drafts():
    from oracle import whisper_oracle as wo
    from thewhisper_amd import AMDWhisperBackend

    chunk_s = 10
    pipe = _micro_pipeline(chunk_s, 1)
    try:
        audio = wo.synth_audio(6 * 16000, 3, "speechlike")
        words, stats = {}, {}
        for draft in (True, False):
            be = AMDWhisperBackend(None, chunk_length_s=chunk_s, asr_pipeline=pipe, hotwords=["w5 w17", "w9"], hotword_boost=30.0,
                                   draft_previous_tick=draft)
            be.transcribe(audio[:16000], 0.0, 16000)      # plan learning outside the compared calls
            be.reset()
            words[draft] = [be.transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
            stats[draft] = dict(be.reuse_stats)
        plain = AMDWhisperBackend(None, chunk_length_s=chunk_s, asr_pipeline=pipe, draft_previous_tick=False)
        unbiased = [plain.transcribe(audio[:n], 0.0, 16000) for n in (4 * 16000, 6 * 16000)]
        print(f"hotwords: {stats[True]}")
        assert words[True] == words[False]
        assert stats[True]["confirmed_tokens"] > 0
        assert unbiased != words[False], "a boost of 30 on the filler words must change the transcript"
    finally:
        pipe.model.engine.close()
