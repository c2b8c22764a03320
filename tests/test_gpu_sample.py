"""The temperature sampler (k_decode.hip: sample_part_kernel, sample_finish_kernel; tw_generate_sample) on the MI355X.

Every case of tests/sample_judge.py: the sequences `generate_sample` returned, fed back through `decode_step` on the crafted zero-layer
model, reproduce the logits its sampler read; `judge_sampled` redraws every step from THOSE logits with the numpy mirror of the draw
and must find none wrong, at most 1 % undecided (mass rule inside MASS_BAND, or the two best perturbed scores within SAMPLE_BAND), at
least 40 judged, and the token different from the processors' argmax at 25 % or more of the drawn steps (the noise is applied).
Then what the draw promises beyond single steps: a stream's ids do not depend on its slot, its batch-mates or graph replay; rows with
temperature 0 are the greedy call's rows and rows with a negative temperature sit the call out; the error paths; token timestamps
after a sampling call; the fallback ladder in `shortform.Pass`.  Run on the MI355X box: ``pytest -m gpu tests/test_gpu_sample.py -s`` prints each case's figures.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import sample_judge as sm
from tests import sampler_judge as sj
from tests.util import PROMPT, clips, make_engine

pytestmark = pytest.mark.gpu
N_PROMPT = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _engine(built, B=None, graph=None):
    c = built.case
    B = B or c.B
    eng = make_engine(built.dims, built.weights, T=sj.T_FRAMES, max_batch=B, dtype=c.dtype, use_graph=c.graph if graph is None else graph)
    eng.encode(torch.zeros((B, built.dims.n_mels, 2 * sj.T_FRAMES), dtype=torch.float32).cuda())     # the zero-layer decoder never reads it
    eng.cross_kv(B)
    return eng


def _replay(eng, seqs):
    B, L = seqs.shape
    eng.decoder_reset(B)
    return np.stack([eng.decode_step(seqs[:, s].tolist()).cpu().numpy() for s in range(L - 1)])


@pytest.mark.parametrize("name", [c.name for c in sm.SAMPLE_CASES])
def test_sampled_tokens_are_the_mirror_s_draw_from_the_engine_s_own_logits(name):
    bs = sm.build_sample_case(sm.sample_case_by_name(name))
    built = bs.built
    eng = _engine(built)
    try:
        out = eng.generate_sample(built.prompt, bs.temperature, bs.seed, bs.offset, **built.kw)
        seqs = out["sequences"]
        assert seqs.shape == (built.case.B, out["length"]) and np.array_equal(seqs[:, :N_PROMPT], built.prompt)
        lg = _replay(eng, seqs)
    finally:
        eng.close()
    assert np.isfinite(lg).all()
    v = sm.judge_sampled(lg, seqs, N_PROMPT, built.opt, bs.temperature, bs.seed, bs.offset)
    print(f"{name}: {v.summary()}")
    sm.check_conditions(v, name)
    assert v.judged == built.case.B * (seqs.shape[1] - N_PROMPT)


def _alone_and_in_a_batch(make, prompt_row, others, kw, temperature, seed, offset):
    """ids of one stream sampled alone (B = 1) and at slot 4 of a batch of 6, with graph replay off and on: four runs."""
    runs = {}
    for graph in (False, True):
        eng = make(1, graph, [0])
        try:
            runs[f"alone graph={graph}"] = eng.generate_sample(prompt_row[None], temperature, seed, offset, **kw)["sequences"][0]
        finally:
            eng.close()
        eng = make(6, graph, [1, 2, 3, 4, 0, 5])
        try:
            prompt = np.stack([others[0], others[1], others[2], others[3], prompt_row, others[4]])
            t = np.asarray([0.3, 1.0, 0.0, 0.8, temperature, 0.5], dtype=np.float32)
            s = np.asarray([11, 12, 13, 14, seed, 15], dtype=np.uint64)
            o = np.asarray([1, 2, 3, 4, offset, 5], dtype=np.uint64)
            runs[f"slot 4 of 6 graph={graph}"] = eng.generate_sample(prompt, t, s, o, **kw)["sequences"][4]
        finally:
            eng.close()
    return runs


def _same_ids(runs, eos):
    def gen(r):     # a row of a longer batch carries more padding: compare up to the first <eos>
        r = r[N_PROMPT:]
        stop = np.flatnonzero(r == eos)
        return r[: int(stop[0]) + 1] if stop.size else r
    ref_name, ref = next(iter(runs.items()))
    assert len(gen(ref)) >= 20, "the stream ends too early to show anything"
    for what, r in runs.items():
        a, b = gen(ref), gen(r)
        n = min(len(a), len(b))
        # (a batch whose other rows end early may stop before this row does: the common part must be equal and neither cut short)
        assert np.array_equal(a[:n], b[:n]) and len(a) == len(b), (ref_name, what, a, b)


def test_a_stream_does_not_depend_on_slot_batch_or_graph_zero_layer_f32():
    built = sj.build_case(sj.case_by_name("v1000-ts-odd"))
    kw = dict(built.kw, min_new_tokens=0)

    def make(B, graph, _clips):
        return _engine(built, B=B, graph=graph)

    runs = _alone_and_in_a_batch(make, built.prompt[2], [built.prompt[i] for i in (0, 1, 3, 4, 5)], kw, 0.6, 0xDEADBEEF12345, 0x300000009)
    _same_ids(runs, built.case.eos)


def test_a_stream_does_not_depend_on_slot_batch_or_graph_micro_model():
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T = 100
    pcm = clips(T * 320, 6)
    kw = dict(max_new_tokens=40, min_new_tokens=40, timestamps=True)       # every row runs the whole budget: equal lengths

    def make(B, graph, which):
        eng = make_engine(dims, w, T=T, max_batch=B, dtype="f32", heads=[(dims.dec_layers - 1, 0)], use_graph=graph)
        mel = eng.logmel(torch.from_numpy(pcm[which]).cuda(), out_dtype=torch.float32)
        eng.encode(mel)
        eng.cross_kv(B)
        return eng

    row = np.array(PROMPT, dtype=np.int32)
    runs = _alone_and_in_a_batch(make, row, [row] * 5, kw, 0.8, 77, 16 * 3 + 1)
    _same_ids(runs, 50257)
    ref = next(iter(runs.values()))
    eng = make(1, False, [0])
    try:
        greedy = eng.generate_greedy(row[None], **kw)["sequences"][0]
    finally:
        eng.close()
    assert not np.array_equal(greedy, ref), "sampling at T = 0.8 returned the greedy ids"


def test_mixed_call_greedy_rows_frozen_rows_and_the_seed():
    built = sj.build_case(sj.case_by_name("v1000-ts-odd"))
    c = built.case
    eng = _engine(built)
    try:
        greedy = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        t = np.asarray([0.0, -1.0, 0.7, 0.0, -2.0, 1.0], dtype=np.float32)
        seed = np.arange(6, dtype=np.uint64) + 5
        off = np.arange(6, dtype=np.uint64) * 16
        out = eng.generate_sample(built.prompt, t, seed, off, **built.kw)
        seqs, L = out["sequences"], out["length"]
        assert np.array_equal(seqs[:, :N_PROMPT], built.prompt)

        def trimmed(r):
            stop = np.flatnonzero(r[N_PROMPT:] == c.eos)
            return r[: N_PROMPT + int(stop[0]) + 1] if stop.size else r

        for b in (0, 3):                                   # T = 0: the greedy call's rows, bit for bit
            assert np.array_equal(trimmed(seqs[b]), trimmed(greedy[b])), (b, seqs[b], greedy[b])
        for b in (1, 4):                                   # T < 0: pad from n_prompt on
            assert (seqs[b, N_PROMPT:] == c.eos).all(), seqs[b]
        # the call ends when the LIVE rows end: its length is the longest live row's (eos included) or the budget
        live_len = max(len(trimmed(seqs[b])) for b in (0, 2, 3, 5))
        assert L == live_len and L <= N_PROMPT + c.max_new, (L, live_len)
        only = eng.generate_sample(built.prompt, np.asarray([-1, -1, 0.7, -1, -1, -1], dtype=np.float32), seed, off, **built.kw)
        assert only["length"] == len(trimmed(only["sequences"][2])) and np.array_equal(trimmed(only["sequences"][2]), trimmed(seqs[2]))
        again = eng.generate_sample(built.prompt, t, seed, off, **built.kw)["sequences"]
        assert np.array_equal(again, seqs)
        other_seed = eng.generate_sample(built.prompt, t, seed + np.uint64(100), off, **built.kw)["sequences"]
        other_off = eng.generate_sample(built.prompt, t, seed, off + np.uint64(1), **built.kw)["sequences"]
        for what, x in (("seed", other_seed), ("offset", other_off)):
            assert x.shape != seqs.shape or not np.array_equal(x[[2, 5]], seqs[[2, 5]]), f"another {what} changed no live row"
            for b in (0, 3):                               # ... and leaves the greedy rows alone
                assert np.array_equal(trimmed(x[b]), trimmed(seqs[b])), (what, b)
    finally:
        eng.close()


def test_error_paths_return_einval_with_a_message():
    built = sj.build_case(dataclasses.replace(sj.case_by_name("v66"), B=2))
    eng = _engine(built)
    try:
        p3 = np.concatenate([built.prompt, built.prompt[:, :2]], axis=1)
        for what, call in (
            ("n_draft", lambda: eng.generate_sample(p3, 0.5, 1, **built.kw, n_draft=2)),
            ("n_forced", lambda: eng.generate_sample(p3, 0.5, 1, **built.kw, n_forced=2)),
            ("negative temperature", lambda: eng.generate_sample(built.prompt, [-1.0, -1.0], 1, **built.kw)),
            ("not finite", lambda: eng.generate_sample(built.prompt, [0.5, float("nan")], 1, **built.kw)),
            ("not finite", lambda: eng.generate_sample(built.prompt, [float("inf"), 0.5], 1, **built.kw)),
        ):
            with pytest.raises(RuntimeError, match=r"tw_generate_sample failed \(-1\).*" + what):
                call()
        out = eng.generate_sample(built.prompt, 0.5, 1, **built.kw)       # the context is usable afterwards
        assert out["sequences"].shape[0] == 2
    finally:
        eng.close()


def test_token_timestamps_after_a_sampling_call_micro_model():
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T, B = 100, 3
    heads = [(dims.dec_layers - 1, 0), (dims.dec_layers - 1, 1)]
    eng = make_engine(dims, w, T=T, max_batch=B, dtype="f32", heads=heads, use_graph=True)
    try:
        mel = eng.logmel(torch.from_numpy(clips(T * 320, B)).cuda(), out_dtype=torch.float32)
        eng.encode(mel)
        eng.cross_kv(B)
        prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
        out = eng.generate_sample(prompt, [0.6, 0.0, 1.0], [1, 2, 3], [0, 16, 32], max_new_tokens=40, min_new_tokens=40, timestamps=True,
                                  want_alignment=True)
        L = out["length"]
        assert L == 3 + 40
        ts = eng.token_timestamps(B, 3, L, [2 * T] * B)
        tm = eng.last_timings()
        assert ts.shape == (B, L) and np.isfinite(ts).all() and (np.diff(ts[:, 3:], axis=1) >= 0).all(), ts
        assert (ts >= 0).all() and (ts <= T * 0.02 + 1e-6).all()
        assert tm["greedy_ms"] > 0 and tm["decode_steps"] >= L - 1, tm
    finally:
        eng.close()


# ---- the fallback ladder in shortform.Pass ---------------------------------------------------------------------------------------
def _plan(kw, init, timestamp_begin, token_timestamps=False):
    from thewhisper_amd.shortform import ShortFormPlan

    return ShortFormPlan(init_tokens=tuple(init), greedy=dict(kw), eos=kw["eos_id"], pad=kw["pad_id"], timestamp_begin=timestamp_begin,
                         return_timestamps=bool(kw.get("timestamps")), return_token_timestamps=token_timestamps, return_segments=True,
                         result_is_dict=True)


def test_pass_with_a_policy_on_the_crafted_repeating_model():
    """Every row of a pass starts from the plan's prompt, so on a zero-layer model the rows agree at T = 0: with the prompt ending in a
    sticky id all of them repeat and are redone, with seeds that differ by the chunk index.  The rows redone and the temperature each
    ends at are what `need_fallback` says of the engine's OWN sequences and `score_tokens` numbers; every attempt is judged on its own
    logits; a redone row is `generate_sample` alone with the same seed and offset; with a prompt that does not repeat, the pass is the
    pass without a policy."""
    from thewhisper_amd import fallback as fb
    from thewhisper_amd import shortform

    dims, w, prompt, opt, kw = sm.repeating_model()
    B, V = 4, dims.vocab
    policy = fb.FallbackPolicy(temperatures=(0.0, 0.2, 0.4, 0.6), compression_ratio_threshold=1.35, logprob_threshold=-10.0, seed=40)
    eng = make_engine(dims, w, T=sj.T_FRAMES, max_batch=B, dtype="f32", use_graph=True)
    calls = []
    greedy_call, sample_call = eng.generate_greedy, eng.generate_sample

    def log_greedy(p, **k):
        out = greedy_call(p, **k)
        calls.append((np.zeros(len(p), np.float32), np.zeros(len(p), np.uint64), np.zeros(len(p), np.uint64), out["sequences"].copy()))
        return out

    def log_sample(p, t, s, o=None, **k):
        out = sample_call(p, t, s, o, **k)
        calls.append((np.asarray(t, np.float32).copy(), np.asarray(s, np.uint64).copy(), np.asarray(o, np.uint64).copy(), out["sequences"].copy()))
        return out

    eng.generate_greedy, eng.generate_sample = log_greedy, log_sample

    def run(init, n, fallback):
        works = [shortform.ChunkWork(torch.zeros((dims.n_mels, 2 * sj.T_FRAMES), device="cuda"), None, tag=i) for i in range(n)]
        for i, x in enumerate(works):
            x.chunk_index = i
        p = shortform.Pass(eng, _plan(kw, init, V), score=True, fallback=fallback)
        p.add(works)
        p.run()
        return works

    try:
        init = (3, 5, sm.STICKY[0])
        works = run(init, B, policy)
        print("temperatures:", [x.temperatures for x in works], "attempts:", [x.attempts for x in works])
        assert len(calls) >= 2 and (calls[0][0] == 0).all(), "nothing was redone: the crafted model does not repeat on the engine"
        # the ladder the engine's own numbers prescribe
        live, want = list(range(B)), {}
        for k, (t, s, o, seqs) in enumerate(calls):
            assert set(np.flatnonzero(t >= 0).tolist()) == set(live) and np.allclose(t[live], policy.temperatures[k])
            if k:
                assert np.array_equal(s, np.arange(B, dtype=np.uint64) + np.uint64(policy.seed)) and (o == np.uint64(k)).all()     # seek 0: offset = attempt
            entries = shortform.score_entries(eng, seqs, N_PROMPT, kw, None)
            lg = _replay(eng, seqs)
            v = sm.judge_sampled(lg, seqs, N_PROMPT, opt, t, s, o)
            print(f"attempt {k}: {v.summary()}")
            assert v.count("wrong") == 0 and v.count("undecided") * 100 <= v.judged
            nxt = []
            for b in live:
                needs, skip = fb.need_fallback(fb._row_tokens(entries[b], opt.eos), V, entries[b]["avg_logprob"], None, policy)
                assert not skip
                if needs and k < len(policy.temperatures) - 1:
                    nxt.append(b)
                else:
                    want[b] = (policy.temperatures[k], k + 1, seqs[b])
            live = nxt
            if not live:
                assert k == len(calls) - 1
                break
        assert sorted(want) == list(range(B))
        for b, x in enumerate(works):
            T, n, row = want[b]
            assert x.temperatures == [T] and x.attempts == [n] and x.passes == 1 and x.done
            toks, _ = shortform.generated_tokens(row[N_PROMPT:], opt.pad, opt.eos)
            assert np.array_equal(shortform.work_tokens(_plan(kw, init, V), x)[0].numpy(), toks) and np.array_equal(x.scores[0]["tokens"], toks)
            if n > 1:       # the same draw alone: frozen batch-mates and the slot do not matter
                alone = sample_call(np.asarray([init], dtype=np.int32), T, policy.seed + b, n - 1, **kw)["sequences"][0]
                t_alone, _ = shortform.generated_tokens(alone[N_PROMPT:], opt.pad, opt.eos)
                assert np.array_equal(t_alone, toks), b
        assert any(n > 1 for _, n, _ in want.values()) and len({T for T, _, _ in want.values()}) > 1
        # a prompt that does not repeat: one greedy call, the pass without a policy
        calls.clear()
        a = run((3, 5, 9), 3, policy)
        assert len(calls) == 1 and all(x.temperatures == [0.0] and x.attempts == [1] for x in a)
        b_ = run((3, 5, 9), 3, None)
        for x, y in zip(a, b_):
            assert torch.equal(shortform.work_tokens(_plan(kw, init, V), x)[0], shortform.work_tokens(_plan(kw, init, V), y)[0]) and x.seek == y.seek
            assert np.array_equal(x.scores[0]["logprob"], y.scores[0]["logprob"])
    finally:
        eng.close()


def test_pass_with_a_policy_on_the_micro_model_redoes_some_rows_and_keeps_the_others_with_their_token_timestamps():
    """Real decoder layers, alignment heads, six clips, HF's default compression threshold: some rows fail at T = 0 and are redone by
    sampling calls, which overwrite the alignment rows of the whole batch.  Rows that pass at T = 0 must still carry the ids AND the token
    timestamps of the pass without a policy (taken right after the attempt that accepted them); a redone row is `generate_sample` of its
    clip alone with the pass's seed and offset, with the token timestamps of that call."""
    from thewhisper_amd import fallback as fb
    from thewhisper_amd import shortform

    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T, B = 100, 6
    eng = make_engine(dims, w, T=T, max_batch=B, dtype="f32", heads=[(dims.dec_layers - 1, 0), (dims.dec_layers - 1, 1)], use_graph=True)
    try:
        mel = eng.logmel(torch.from_numpy(clips(T * 320, B)).cuda(), out_dtype=torch.float32)
        kw = dict(max_new_tokens=32, min_new_tokens=0, max_length=448, eos_id=50257, pad_id=50257, timestamps=True, no_timestamps_id=50364,
                  max_initial_timestamp_index=50, begin_suppress=(220, 50257), suppress=(), want_alignment=True)
        plan = _plan(kw, PROMPT, 50365, token_timestamps=True)
        policy = fb.FallbackPolicy(temperatures=(0.0, 0.4, 0.8), logprob_threshold=-10.0, seed=7)      # compression ratio: HF's 1.35

        def run(fallback):
            works = [shortform.ChunkWork(mel[i], 2 * T, tag=i) for i in range(B)]
            for i, x in enumerate(works):
                x.chunk_index = i
            p = shortform.Pass(eng, plan, score=True, fallback=fallback)
            p.add(works)
            p.run()
            return works, p

        plain, _ = run(None)
        works, p = run(policy)
        attempts = [x.attempts[0] for x in works]
        print("temperatures:", [x.temperatures[0] for x in works], "attempts:", attempts)
        kept, redone = [b for b in range(B) if attempts[b] == 1], [b for b in range(B) if attempts[b] > 1]
        assert kept and redone, "the case needs rows that pass at T = 0 and rows that do not"
        for b in range(B):          # what the engine's own T = 0 numbers say: need_fallback of the plain pass's score entry
            e = plain[b].scores[0]
            needs, _ = fb.need_fallback(fb._row_tokens(e, 50257), dims.vocab, e["avg_logprob"], None, policy)
            assert needs == (b in redone), b
        for b in kept:
            for x, y in zip(shortform.work_tokens(plan, works[b]), shortform.work_tokens(plan, plain[b])):
                assert x.numel() > 0 and torch.equal(x, y), b
            assert works[b].seek == plain[b].seek and works[b].temperatures == [0.0]
        for b in redone:            # the clip alone in slot 0, the pass's seed and offset (seek 0: offset = attempt index)
            r = p.last_fallback[b]
            eng.encode(mel[b:b + 1])
            eng.cross_kv(1)
            out = eng.generate_sample(np.asarray([PROMPT], dtype=np.int32), r["temperature"], policy.seed + b, r["attempts"] - 1, **kw)
            L = out["length"]
            ts = eng.token_timestamps(1, N_PROMPT, L, [2 * T])[0]
            assert np.array_equal(r["sequence"][:L], out["sequences"][0]) and (r["sequence"][L:] == 50257).all(), b
            toks, _ = shortform.generated_tokens(out["sequences"][0, N_PROMPT:], 50257, 50257)
            ids, raw, _ = shortform.work_tokens(plan, works[b])
            n = ids.numel()          # (the segments keep the tokens up to the last closed timestamp pair)
            assert n > 0 and np.array_equal(ids.numpy(), toks[:n]) and np.array_equal(raw.numpy(), ts[N_PROMPT:N_PROMPT + n]), b
    finally:
        eng.close()
