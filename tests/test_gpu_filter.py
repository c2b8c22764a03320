"""Top-k / top-p filtering in the temperature sampler (k_decode.hip: sample_filter_kernel, sample_choice_finish_kernel;
tw_generate_sample_filtered) on the MI355X.

Every case of tests/filter_judge.py: the sequences `generate_sample(top_k=, top_p=)` returned, fed back through `decode_step` on the
crafted zero-layer model, reproduce the logits its sampler read; `judge_filtered` redraws every step from THOSE logits with the numpy
mirror of the rule and must find none wrong, at most 1 % undecided, at least 40 judged, the token different from the processors'
argmax at 25 % or more of the drawn steps, and the unfiltered draw of the same seed outside the kept set at 25 % or more of the
filtered steps (an engine that ignored the filter would be wrong there).  Then: off means off, degenerate filters are greedy, a stream
does not depend on slot, batch or graph, the error paths, token timestamps after a filtered call, the fallback ladder with a filter.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_filter.py -s`` prints each case's figures.
"""
import dataclasses

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import filter_judge as fj
from tests import sample_judge as sm
from tests import sampler_judge as sj
from tests.test_gpu_sample import _engine, _plan, _replay, _same_ids
from tests.util import PROMPT, clips, make_engine

pytestmark = pytest.mark.gpu
N_PROMPT = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.mark.parametrize("name", [c.name for c in fj.FILTER_CASES])
def test_filtered_tokens_are_the_mirror_s_draw_from_the_engine_s_own_logits(name):
    bf = fj.build_filter_case(fj.filter_case_by_name(name))
    built, s = bf.built, bf.sample
    eng = _engine(built)
    try:
        out = eng.generate_sample(built.prompt, s.temperature, s.seed, s.offset, **built.kw, top_k=bf.top_k, top_p=bf.top_p)
        seqs = out["sequences"]
        assert seqs.shape == (built.case.B, out["length"]) and np.array_equal(seqs[:, :N_PROMPT], built.prompt)
        lg = _replay(eng, seqs)
    finally:
        eng.close()
    assert np.isfinite(lg).all()
    v = fj.judge_case(bf, lg, seqs, N_PROMPT)
    print(f"{name}: {v.summary()}")
    fj.check_conditions(v, name)
    assert v.judged == built.case.B * (seqs.shape[1] - N_PROMPT)
    assert not bf.case.tau_inf or v.tau_inf_mass > 0, "no step where the mass rule fired with fewer than k ids left"
    assert not bf.case.ties or v.tie_at_tau > 0, "no step with ties at the top-k threshold"
    if name == "v1000-b33-mixed":
        assert v.k_above_open > 0


@pytest.mark.parametrize("graph", [False, True])
def test_off_means_off(graph):
    """Rows with (0, 1.0) inside a filtered call are `generate_sample`'s rows for the same seeds, bit for bit; a call with every row
    off is `generate_sample` exactly."""
    bs = sm.build_sample_case(sm.SampleCase("off", "v1000-ts-odd", 1.0, graph=graph))
    built = bs.built
    kw = dict(built.kw, min_new_tokens=built.case.max_new)       # every row runs the whole budget: equal lengths in every call
    eng = _engine(built)
    try:
        plain = eng.generate_sample(built.prompt, bs.temperature, bs.seed, bs.offset, **kw)["sequences"]
        k = np.asarray([0, 8, 0, 50, 0, 3], dtype=np.int32)
        p = np.asarray([1.0, 1.0, 1.0, 0.9, 1.0, 0.5], dtype=np.float32)
        mixed = eng.generate_sample(built.prompt, bs.temperature, bs.seed, bs.offset, **kw, top_k=k, top_p=p)["sequences"]
        assert mixed.shape == plain.shape
        for b in (0, 2, 4):
            assert np.array_equal(mixed[b], plain[b]), b
        assert all(not np.array_equal(mixed[b], plain[b]) for b in (1, 3, 5)), "a filtered row equals the unfiltered one"
        for tk, tp in ((0, 1.0), (None, 1.0), (0, None), (np.zeros(6, np.int32), np.ones(6, np.float32))):
            off = eng.generate_sample(built.prompt, bs.temperature, bs.seed, bs.offset, **kw, top_k=tk, top_p=tp)["sequences"]
            assert np.array_equal(off, plain)
        again = eng.generate_sample(built.prompt, bs.temperature, bs.seed, bs.offset, **kw)["sequences"]      # ... and the filtered graph was not kept for it
        assert np.array_equal(again, plain)
        # rows whose temperature is 0 ignore their filter: the call is the unfiltered one
        t0 = np.asarray([0.0, 0.0, 1.0, 0.0, 1.0, 0.0], dtype=np.float32)
        a = eng.generate_sample(built.prompt, t0, bs.seed, bs.offset, **kw)["sequences"]
        b_ = eng.generate_sample(built.prompt, t0, bs.seed, bs.offset, **kw, top_k=[5, 5, 0, 5, 0, 5], top_p=[0.5, 1.0, 1.0, 0.5, 1.0, 1.0])["sequences"]
        assert np.array_equal(a, b_)
    finally:
        eng.close()


def _micro(B, graph, which, heads=None):
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T = 100
    eng = make_engine(dims, w, T=T, max_batch=B, dtype="f32", heads=heads or [(dims.dec_layers - 1, 0)], use_graph=graph)
    mel = eng.logmel(torch.from_numpy(clips(T * 320, 6)[which]).cuda(), out_dtype=torch.float32)
    eng.encode(mel)
    eng.cross_kv(B)
    return eng


def test_degenerate_filters_are_greedy_micro_model():
    """Real layers, no planted ties, T = 1.0: top_k = 1 keeps the maximum alone, top_p = 1e-6 keeps the maximum alone."""
    B = 3
    eng = _micro(B, True, [0, 1, 2])
    try:
        prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
        kw = dict(max_new_tokens=40, min_new_tokens=40, timestamps=True)
        greedy = eng.generate_greedy(prompt, **kw)["sequences"]
        free = eng.generate_sample(prompt, 1.0, [1, 2, 3], **kw)["sequences"]
        assert not np.array_equal(free, greedy), "sampling at T = 1 returned the greedy ids"
        k1 = eng.generate_sample(prompt, 1.0, [1, 2, 3], **kw, top_k=1)["sequences"]
        p0 = eng.generate_sample(prompt, 1.0, [1, 2, 3], **kw, top_p=1e-6)["sequences"]
        assert np.array_equal(k1, greedy) and np.array_equal(p0, greedy)
    finally:
        eng.close()


def _alone_and_in_a_batch(make, prompt_row, others, kw, temperature, seed, offset):
    """tests/test_gpu_sample.py's four runs with k = 8, p = 0.9 on the tested row and other filters on its batch-mates."""
    runs = {}
    for graph in (False, True):
        eng = make(1, graph, [0])
        try:
            runs[f"alone graph={graph}"] = eng.generate_sample(prompt_row[None], temperature, seed, offset, **kw, top_k=8, top_p=0.9)["sequences"][0]
        finally:
            eng.close()
        eng = make(6, graph, [1, 2, 3, 4, 0, 5])
        try:
            prompt = np.stack([others[0], others[1], others[2], others[3], prompt_row, others[4]])
            t = np.asarray([0.3, 1.0, 0.0, 0.8, temperature, 0.5], dtype=np.float32)
            s = np.asarray([11, 12, 13, 14, seed, 15], dtype=np.uint64)
            o = np.asarray([1, 2, 3, 4, offset, 5], dtype=np.uint64)
            k = np.asarray([0, 50, 3, 1, 8, 2000], dtype=np.int32)
            p = np.asarray([0.5, 1.0, 0.7, 1.0, 0.9, 0.3], dtype=np.float32)
            runs[f"slot 4 of 6 graph={graph}"] = eng.generate_sample(prompt, t, s, o, **kw, top_k=k, top_p=p)["sequences"][4]
        finally:
            eng.close()
    return runs


def test_a_filtered_stream_does_not_depend_on_slot_batch_or_graph_zero_layer_f32():
    built = sj.build_case(sj.case_by_name("v1000-ts-odd"))
    kw = dict(built.kw, min_new_tokens=0)

    def make(B, graph, _clips):
        return _engine(built, B=B, graph=graph)

    runs = _alone_and_in_a_batch(make, built.prompt[2], [built.prompt[i] for i in (0, 1, 3, 4, 5)], kw, 0.6, 0xDEADBEEF12345, 0x300000009)
    _same_ids(runs, built.case.eos)


def test_a_filtered_stream_does_not_depend_on_slot_batch_or_graph_micro_model():
    kw = dict(max_new_tokens=40, min_new_tokens=40, timestamps=True)       # every row runs the whole budget: equal lengths
    row = np.array(PROMPT, dtype=np.int32)
    runs = _alone_and_in_a_batch(_micro, row, [row] * 5, kw, 0.8, 77, 16 * 3 + 1)
    _same_ids(runs, 50257)
    ref = next(iter(runs.values()))
    eng = _micro(1, False, [0])
    try:
        plain = eng.generate_sample(row[None], 0.8, 77, 16 * 3 + 1, **kw)["sequences"][0]
    finally:
        eng.close()
    assert not np.array_equal(plain, ref), "the filtered stream equals the unfiltered one"


def test_error_paths_return_einval_with_a_message():
    built = sj.build_case(dataclasses.replace(sj.case_by_name("v66"), B=2))
    eng = _engine(built)
    try:
        from thewhisper_amd import _cabi
        import ctypes as C

        def raw(top_k, top_p):      # past the host checks of generate_sample: the library's own
            t = np.asarray([0.5, 0.5], np.float32)
            sd = np.asarray([1, 2], np.uint64)
            so = _cabi.tw_sample_opts()
            so.temperature, so.seed, so.offset = t.ctypes.data_as(C.POINTER(C.c_float)), sd.ctypes.data_as(C.POINTER(C.c_uint64)), None
            k, p = np.asarray(top_k, np.int32), np.asarray(top_p, np.float32)
            fo = _cabi.tw_filter_opts()
            fo.top_k, fo.top_p = k.ctypes.data_as(C.POINTER(C.c_int32)), p.ctypes.data_as(C.POINTER(C.c_float))
            kw = built.kw
            o, _keep = eng._greedy_opts(kw["eos_id"], kw["pad_id"], kw["timestamps"], kw["no_timestamps_id"], kw["max_initial_timestamp_index"],
                                        kw["begin_suppress"], kw["suppress"], kw.get("min_new_tokens", 0), kw["max_new_tokens"], 448)
            prompt = np.ascontiguousarray(built.prompt, dtype=np.int32)
            out, n = np.zeros((2, 448), np.int32), C.c_int32(0)
            rc = eng.lib.tw_generate_sample_filtered(eng.ctx, 2, prompt.ctypes.data_as(C.POINTER(C.c_int32)), prompt.shape[1], C.byref(o), C.byref(so),
                                                     C.byref(fo), out.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(n), None)
            return rc, eng.lib.tw_last_error(eng.ctx).decode()

        for what, k, p in (("negative top_k", [3, -1], [1.0, 1.0]), ("top_p", [0, 0], [0.0, 1.0]), ("top_p", [0, 0], [0.5, 1.5]),
                           ("top_p", [0, 0], [float("nan"), 1.0])):
            rc, msg = raw(k, p)
            assert rc == -1 and "tw_generate_sample_filtered" in msg and what in msg, (rc, msg)
        for bad in (dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan"))):       # ... and the host's, before any call
            with pytest.raises(ValueError):
                eng.generate_sample(built.prompt, 0.5, 1, **built.kw, **bad)
        with pytest.raises(RuntimeError, match=r"tw_generate_sample_filtered failed \(-1\).*n_draft"):
            eng.generate_sample(np.concatenate([built.prompt, built.prompt[:, :2]], axis=1), 0.5, 1, **built.kw, n_draft=2, top_k=3)
        out = eng.generate_sample(built.prompt, 0.5, 1, **built.kw, top_k=3)       # the context is usable afterwards
        assert out["sequences"].shape[0] == 2
    finally:
        eng.close()


def test_token_timestamps_after_a_filtered_call_micro_model():
    """want_alignment under the filtered call: the token timestamps equal the oracle's DTW on the alignment rows of the sequence
    actually sampled (the oracle, teacher-forced on the engine's ids), within one frame as everywhere else."""
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    T, B = 100, 3
    heads = [(dims.dec_layers - 1, 0), (dims.dec_layers - 1, 1)]
    eng = _micro(B, True, [0, 1, 2], heads=heads)
    try:
        prompt = np.tile(np.array(PROMPT, dtype=np.int32), (B, 1))
        out = eng.generate_sample(prompt, [0.6, 0.0, 1.0], [1, 2, 3], [0, 16, 32], max_new_tokens=40, min_new_tokens=40, timestamps=True,
                                  want_alignment=True, top_k=[8, 5, 0], top_p=[1.0, 1.0, 0.8])
        L = out["length"]
        assert L == 3 + 40
        ts = eng.token_timestamps(B, 3, L, [2 * T] * B)
        tm = eng.last_timings()
    finally:
        eng.close()
    assert ts.shape == (B, L) and np.isfinite(ts).all() and (np.diff(ts[:, 3:], axis=1) >= 0).all(), ts
    assert tm["greedy_ms"] > 0 and tm["decode_steps"] >= L - 1, tm
    om = wo.OracleWhisper(dims, w, T=T)
    enc = om.encode(wo.log_mel(clips(T * 320, 6)[[0, 1, 2]], dims.n_mels))
    _, cross = om.decode(out["sequences"][:, :-1], om.new_cache(enc), want_cross=heads)
    ref = wo.token_timestamps(cross, 3, [2 * T] * B)
    assert np.abs(ts - ref[:, :L]).max() <= 0.0201, (ts, ref)


def test_pass_with_a_filtering_policy_on_the_crafted_repeating_model():
    """`Pass` with `FallbackPolicy(top_k=8)`: the sticky rows are redone, every sampled attempt carries the filter and passes the
    filter judge on its own logits, rows that do not repeat are kept, and `last_fallback` reports the filter."""
    from thewhisper_amd import fallback as fb
    from thewhisper_amd import shortform

    dims, w, prompt, opt, kw = sm.repeating_model()
    B, V = 4, dims.vocab
    policy = fb.FallbackPolicy(temperatures=(0.0, 0.2, 0.4, 0.6), compression_ratio_threshold=1.35, logprob_threshold=-10.0, seed=40, top_k=8)
    eng = make_engine(dims, w, T=sj.T_FRAMES, max_batch=B, dtype="f32", use_graph=True)
    calls = []
    sample_call = eng.generate_sample

    def log_sample(p, t, s, o=None, **k):
        out = sample_call(p, t, s, o, **k)
        calls.append((np.asarray(t, np.float32).copy(), np.asarray(s, np.uint64).copy(), np.asarray(o, np.uint64).copy(), k.get("top_k"), k.get("top_p"),
                      out["sequences"].copy()))
        return out

    eng.generate_sample = log_sample

    def run(init, n):
        works = [shortform.ChunkWork(torch.zeros((dims.n_mels, 2 * sj.T_FRAMES), device="cuda"), None, tag=i) for i in range(n)]
        for i, x in enumerate(works):
            x.chunk_index = i
        p = shortform.Pass(eng, _plan(kw, init, V), score=True, fallback=policy)
        p.add(works)
        p.run()
        return works, p

    try:
        works, p = run((3, 5, sm.STICKY[0]), B)
        print("temperatures:", [x.temperatures for x in works], "attempts:", [x.attempts for x in works])
        assert calls and all(x.attempts[0] > 1 for x in works), "nothing was redone: the crafted model does not repeat on the engine"
        for n, (t, s, o, k, pp, seqs) in enumerate(calls, start=1):
            assert k == 8 and pp is None
            lg = _replay(eng, seqs)
            v = fj.judge_filtered(lg, seqs, N_PROMPT, opt, t, s, o, 8, 1.0)
            print(f"attempt {n}: {v.summary()}")
            assert v.count("wrong") == 0 and v.count("undecided") * 100 <= v.judged and v.filtered > 0
        assert len(p.last_fallback) == B and all(r["top_k"] == 8 and r["top_p"] is None for r in p.last_fallback)
        for b, x in enumerate(works):       # the accepted row is the filtered draw of its (seed, offset) alone
            r = p.last_fallback[b]
            alone = sample_call(np.asarray([(3, 5, sm.STICKY[0])], dtype=np.int32), r["temperature"], policy.seed + b, r["attempts"] - 1, **kw, top_k=8)
            toks, _ = shortform.generated_tokens(alone["sequences"][0, N_PROMPT:], opt.pad, opt.eos)
            assert np.array_equal(shortform.work_tokens(_plan(kw, (3, 5, sm.STICKY[0]), V), x)[0].numpy(), toks), b
        calls.clear()
        kept, _ = run((3, 5, 9), 3)        # a prompt that does not repeat: kept at T = 0, no sampling call
        assert not calls and all(x.temperatures == [0.0] and x.attempts == [1] for x in kept)
    finally:
        eng.close()
