"""Temperature sampling and the temperature fallback, the parts that need no GPU: the numpy mirror of the draw (tests/sample_judge.py)
against Philox4x32-10's known answers and against the softmax it claims to draw from; the mirror's own run of every case the GPU
test replays (the conditions demanded there hold for a correct sampler); thewhisper_amd/fallback.py against HF's helpers; the C ABI's
new struct and symbol; the fallback ladder in `shortform.Pass` on a stand-in engine (tests/oracle_engine.OracleEngine + the mirror)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sample_judge as sm
from tests import sampler_judge as sj
from tests.oracle_engine import OracleEngine

N_PROMPT = 3


# ---- the generator and the draw ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,expected", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, expected):
    assert " ".join(f"{int(x):08x}" for x in sm.philox4x32_10(counter, key)) == expected


def test_u_is_exact_in_float32_and_never_0_or_1():
    lo, hi = float(sm.u_of(0)), float(sm.u_of(0xFFFFFFFF))
    assert lo == 2.0 ** -24 and hi == 1.0 - 2.0 ** -24
    assert float(np.float32(lo)) == lo and float(np.float32(hi)) == hi and 0.0 < np.float32(lo) and np.float32(hi) < 1.0
    w = np.random.default_rng(0).integers(0, 2 ** 32, size=4096, dtype=np.uint64)
    u = sm.u_of(w)
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u) and u.min() > 0 and u.max() < 1


def test_the_mirror_draws_from_the_softmax():
    """20 000 draws on a fixed 16-logit vector at T = 0.6, key (123, 456), position = draw index: chi-square against softmax(x / T)
    below 37.7, the 0.001 point for 15 degrees of freedom."""
    x = np.random.default_rng(11).standard_normal(16).astype(np.float32) * 1.5
    T, n = 0.6, 20000
    seed = 123 | (456 << 32)
    counts = np.zeros(16)
    for p in range(n):
        counts[int(np.argmax(sm.scores(x, T, p, seed, 0)))] += 1
    z = x.astype(np.float64) * float(sm.inv_t32(T))
    prob = np.exp(z - z.max())
    prob /= prob.sum()
    chi2 = float(((counts - n * prob) ** 2 / (n * prob)).sum())
    print(f"chi-square {chi2:.1f} (15 degrees of freedom)")
    assert chi2 < 37.7, chi2


@pytest.mark.parametrize("name", [c.name for c in sm.SAMPLE_CASES])
def test_the_mirror_s_own_run_meets_what_the_gpu_test_demands(name):
    bs = sm.build_sample_case(sm.sample_case_by_name(name))
    seqs, lg = sm.mirror_run(bs)
    v = sm.judge_sampled(lg, seqs, N_PROMPT, bs.built.opt, bs.temperature, bs.seed, bs.offset)
    print(f"{name}: {v.summary()}")
    sm.check_conditions(v, name)
    t = bs.temperature
    assert np.array_equal(seqs[:, :N_PROMPT], bs.built.prompt) and (seqs[t < 0, N_PROMPT:] == bs.built.opt.pad).all()
    if (t == 0).any():      # greedy rows of a mixed call are the greedy call's rows
        greedy, _ = sj.oracle_run(bs.built.dims, bs.built.weights, bs.built.prompt, bs.built.opt)
        n = min(greedy.shape[1], seqs.shape[1])
        assert np.array_equal(seqs[t == 0, :n], greedy[t == 0, :n])


# ---- fallback.py against HF ----------------------------------------------------------------------------------------------------
def test_compression_ratio_equals_hf():
    from transformers.models.whisper.generation_whisper import WhisperGenerationMixin as M

    from thewhisper_amd.fallback import compression_ratio

    rng = np.random.default_rng(3)
    for vocab in (1000, 51865, 51866, 70000):
        for toks in (rng.integers(0, vocab, size=57), np.tile(rng.integers(0, vocab, size=3), 40), np.full(100, vocab - 1), np.array([5])):
            assert compression_ratio(toks, vocab) == M._retrieve_compression_ratio(torch.from_numpy(toks), vocab)
    assert compression_ratio(np.tile([7, 8], 60), 51865) > 2.4 > 1.35 > compression_ratio(rng.integers(0, 51865, size=120), 51865)


def test_need_fallback_truth_table():
    from thewhisper_amd.fallback import FallbackPolicy, need_fallback

    rep, rnd = np.tile([7, 8], 60), np.random.default_rng(3).integers(0, 51865, size=120)
    V = 51865
    p = FallbackPolicy()
    assert need_fallback(rnd, V, -0.5, None, p) == (False, False)
    assert need_fallback(rep, V, -0.5, None, p) == (True, False)                  # compression ratio
    assert need_fallback(rnd, V, -1.5, None, p) == (True, False)                  # average log-probability
    assert need_fallback(rnd, V, -1.0, None, p) == (False, False)                 # strict comparison, as HF's
    q = FallbackPolicy(no_speech_threshold=0.6)
    assert need_fallback(rnd, V, -1.5, 0.7, q) == (False, True)                   # low log-probability AND silence: skip, no fallback
    assert need_fallback(rep, V, -1.5, 0.7, q) == (False, True)                   # ... whatever the compression ratio said
    assert need_fallback(rnd, V, -1.5, 0.6, q) == (True, False)
    assert need_fallback(rnd, V, -0.5, 0.9, q) == (False, False)
    assert need_fallback(rep, V, -0.5, 0.9, q) == (True, False)
    none = FallbackPolicy(compression_ratio_threshold=None, logprob_threshold=None)
    assert need_fallback(rep, V, None, None, none) == (False, False)
    with pytest.raises(ValueError):
        need_fallback(rnd, V, None, None, p)
    with pytest.raises(ValueError):
        FallbackPolicy(temperatures=(0.0, -0.2))


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_sizes_and_the_symbol(built_library):
    from thewhisper_amd import _cabi

    assert ctypes.sizeof(_cabi.tw_sample_opts) == 24
    assert ctypes.sizeof(_cabi.tw_greedy_opts) == 80
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "tw_generate_sample") and "tw_generate_sample" in [n for n, _, _ in _cabi.SYMBOLS]
    lib = _cabi.load_library()
    assert lib.tw_generate_sample(None, 1, None, 3, None, None, None, None, None) == -1     # refused before any device call
    assert b"tw_generate_sample" in lib.tw_last_error(None)


# ---- the ladder on a stand-in engine -------------------------------------------------------------------------------------------
class SamplingOracleEngine(OracleEngine):
    """OracleEngine + `generate_sample` from the mirror + `score_tokens` from the oracle; every engine call is logged."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log = []

    def generate_greedy(self, prompt, **kw):
        self.log.append(("greedy", np.asarray(prompt).shape[0], int(kw.get("n_draft", 0))))
        return super().generate_greedy(prompt, **kw)

    def generate_sample(self, prompt, temperature, seed, offset=None, **kw):
        assert not kw.get("n_forced") and not kw.get("n_draft")
        self.calls["generate"] += 1
        B = np.asarray(prompt).shape[0]
        t = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (B,))
        self.log.append(("sample", t.copy(), np.asarray(seed).copy(), np.asarray(offset).copy()))
        import dataclasses

        opt = dataclasses.replace(sm.options_of(kw), alignment_heads=self.alignment_heads if kw.get("want_alignment") else None)
        cross = []
        seqs, _ = sm.mirror_generate(self.model, self._enc[:B], prompt, opt, t, seed, offset, cross_out=cross)
        self._cross = cross[0] if cross else None
        return {"sequences": seqs, "length": int(seqs.shape[1])}

    def score_tokens(self, sequences, n_prompt, *, no_speech_id=None, no_speech_pos=0, **kw):
        return sm.oracle_scores(self.model, self._enc[: np.asarray(sequences).shape[0]], sequences, n_prompt, kw, no_speech_id)


def sampling_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return SamplingOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


def repeating_engine(B=6):
    import dataclasses

    dims, w, prompt, opt, kw = sm.repeating_model()
    eng = SamplingOracleEngine(dataclasses.asdict(dims), sj.T_FRAMES, B, "f32", [])
    eng.model = sj._OracleExactTies(dims, w, T=sj.T_FRAMES)
    eng.encode(torch.zeros((B, dims.n_mels, 2 * sj.T_FRAMES)))
    return eng, dims, prompt, opt, kw


LADDER = dict(temperatures=(0.0, 0.2, 0.4, 0.6), compression_ratio_threshold=1.35, logprob_threshold=-10.0, seed=40)


def test_generate_with_fallback_redoes_only_the_failing_rows():
    from thewhisper_amd import fallback as fb

    eng, dims, prompt, opt, kw = repeating_engine()
    V, eos = dims.vocab, opt.eos
    policy = fb.FallbackPolicy(**LADDER)
    greedy = OracleEngine.generate_greedy(eng, prompt, **kw)["sequences"]
    ratio0 = [fb.compression_ratio(fb._row_tokens({"tokens": r[N_PROMPT:], "logprob": r[N_PROMPT:]}, eos), V) for r in greedy]
    print("compression ratios at T = 0:", [round(x, 2) for x in ratio0])
    # the conditions the crafted model must meet: rows 0-2 repeat, rows 3-5 do not
    assert all(x > 1.35 for x in ratio0[:3]) and all(x < 1.35 for x in ratio0[3:]), ratio0
    seen = []
    seeds, offsets = [40 + b for b in range(6)], [16 * b for b in range(6)]
    res = fb.generate_with_fallback(eng, prompt, kw, policy, None, seeds, offsets, on_attempt=lambda k, T, out, rows: seen.append((k, T, list(rows))))
    print("temperature / attempts per row:", [(r["temperature"], r["attempts"]) for r in res])
    for b in (3, 4, 5):         # passed at T = 0: the greedy rows, never redrawn
        assert res[b]["temperature"] == 0.0 and res[b]["attempts"] == 1 and np.array_equal(res[b]["sequence"], greedy[b])
    assert all(res[b]["attempts"] > 1 for b in (0, 1, 2))
    assert len({res[b]["temperature"] for b in (0, 1, 2)}) > 1, "every repeating row ended at the same temperature"
    assert any(res[b]["needs_fallback"] and res[b]["temperature"] == 0.6 for b in (0, 1, 2)), "no row is still failing at the last temperature"
    assert eng.log[0][0] == "greedy"
    live = {0, 1, 2}
    for k, call in enumerate(eng.log[1:], start=1):       # attempt k: only rows still failing are live, with (seed, offset + k)
        assert call[0] == "sample"
        t = call[1]
        assert set(np.flatnonzero(t >= 0).tolist()) == live and (t[t >= 0] == np.float32(policy.temperatures[k])).all() and (t[t < 0] == -1).all()
        assert np.array_equal(call[2], np.asarray(seeds, dtype=np.uint64)) and np.array_equal(call[3], np.asarray(offsets, dtype=np.uint64) + np.uint64(k))
        live -= {b for b in live if res[b]["attempts"] == k + 1}
    assert len(eng.log) == max(r["attempts"] for r in res) <= len(policy.temperatures)
    assert [s[0] for s in seen] == list(range(len(eng.log))) and sorted(b for s in seen for b in s[2]) == list(range(6))
    for b in (0, 1, 2):         # a redone row is the draw of its (seed, offset + attempt) ALONE: frozen batch-mates do not matter
        k = res[b]["attempts"] - 1
        alone, _ = sm.mirror_generate(eng.model, eng._enc[:1], prompt[b:b + 1], opt, res[b]["temperature"], seeds[b], offsets[b] + k)
        n = alone.shape[1]
        assert np.array_equal(res[b]["sequence"][:n], alone[0]) and (res[b]["sequence"][n:] == eos).all()
        e = res[b]["score"]
        needs, skip = fb.need_fallback(fb._row_tokens(e, eos), V, e["avg_logprob"], e["no_speech_prob"], policy)
        assert needs == res[b]["needs_fallback"] and not skip and (not needs or k == len(policy.temperatures) - 1)


def _plan(kw, init, V):
    from thewhisper_amd.shortform import ShortFormPlan

    return ShortFormPlan(init_tokens=tuple(init), greedy=dict(kw), eos=kw["eos_id"], pad=kw["pad_id"], timestamp_begin=V, return_timestamps=False,
                         return_token_timestamps=False, return_segments=True, result_is_dict=True)


def _run_pass(eng, plan, dims, n, fallback, score=False):
    from thewhisper_amd import shortform

    works = [shortform.ChunkWork(torch.zeros((dims.n_mels, 2 * sj.T_FRAMES)), None, tag=i) for i in range(n)]
    for i, w in enumerate(works):
        w.chunk_index = i
    p = shortform.Pass(eng, plan, score=score, fallback=fallback)
    p.add(works)
    p.run()
    return works, p


def test_pass_with_a_policy_merges_rows_of_different_attempts():
    """Every row of a pass starts from the plan's prompt, so on a zero-layer model the rows agree at T = 0; with the prompt ending in a
    sticky id they all repeat, are all redone, and - their seeds differ by the chunk index - leave the ladder at different rungs."""
    from thewhisper_amd import fallback as fb
    from thewhisper_amd import shortform

    eng, dims, prompt, opt, kw = repeating_engine(4)
    V = dims.vocab
    policy = fb.FallbackPolicy(**LADDER)
    plan = _plan(kw, (3, 5, sm.STICKY[0]), V)
    works, p = _run_pass(eng, plan, dims, 4, policy, score=True)
    temps = [w.temperatures[0] for w in works]
    print("temperatures:", temps, "attempts:", [w.attempts[0] for w in works])
    assert all(t > 0 for t in temps) and len(set(temps)) > 1, temps
    assert [c[0] for c in eng.log] == ["greedy"] + ["sample"] * (max(w.attempts[0] for w in works) - 1)
    for i, w in enumerate(works):
        assert w.passes == 1 and w.done and len(w.scores) == 1 and w.attempts[0] == policy.temperatures.index(temps[i]) + 1
        k = w.attempts[0] - 1
        alone, _ = sm.mirror_generate(eng.model, eng._enc[:1], np.asarray([plan.init_tokens]), opt, temps[i], policy.seed + i, 0 * 16 + k)
        toks, _ = shortform.generated_tokens(alone[0, N_PROMPT:], opt.pad, opt.eos)
        assert np.array_equal(shortform.work_tokens(plan, w)[0].numpy(), toks), i
        assert np.array_equal(w.scores[0]["tokens"], toks)
    # a prompt that does not repeat: nothing is redone, and the pass is the pass without a policy
    plan2 = _plan(kw, (3, 5, 9), V)
    eng.log.clear()
    with_policy, _ = _run_pass(eng, plan2, dims, 3, policy)
    assert [c[0] for c in eng.log] == ["greedy"] and all(w.temperatures == [0.0] and w.attempts == [1] for w in with_policy)
    eng.log.clear()
    without, _ = _run_pass(eng, plan2, dims, 3, None)
    assert [c[0] for c in eng.log] == ["greedy"] and all(w.temperatures == [] for w in without)
    for a, b in zip(with_policy, without):
        assert torch.equal(shortform.work_tokens(plan2, a)[0], shortform.work_tokens(plan2, b)[0]) and a.seek == b.seek


def test_pass_skips_a_row_hf_would_skip_as_silence():
    from thewhisper_amd import fallback as fb

    eng, dims, prompt, opt, kw = repeating_engine(2)
    plan = _plan(kw, (3, 5, 9), dims.vocab)
    # every row's average log-probability is below -1 here (a 1000-way random walk) and any no-speech probability is above 0
    policy = fb.FallbackPolicy(temperatures=(0.0, 0.4), logprob_threshold=-1.0, no_speech_threshold=0.0, seed=1)
    from thewhisper_amd import shortform

    works = [shortform.ChunkWork(torch.zeros((dims.n_mels, 2 * sj.T_FRAMES)), None) for _ in range(2)]
    p = shortform.Pass(eng, plan, no_speech_id=5, fallback=policy)
    p.add(works)
    p.run()
    assert [c[0] for c in eng.log] == ["greedy"]
    assert all(w.segments == [] and w.done and w.passes == 1 and w.temperatures == [0.0] for w in works)
    assert all(r["should_skip"] for r in p.last_fallback)


def test_generate_shortform_with_a_policy_that_never_fires_is_the_plain_call():
    from oracle import hf_reference as hr
    from oracle import whisper_oracle as wo
    from thewhisper_amd import ASRPipeline, shortform
    from thewhisper_amd.fallback import FallbackPolicy

    dims = wo.PRESETS["micro"]
    model = hr.build_hf_model(dims, wo.make_weights(dims, 0))
    pipe = ASRPipeline(model, feature_extractor=hr.build_feature_extractor(dims, 10), tokenizer=hr.build_tokenizer(dims), chunk_length_s=10,
                       device="cpu", torch_dtype=torch.float32, batch_size=3, engine_factory=sampling_factory)
    pcm = [wo.synth_audio(160000 - 1000 * i, i, k) for i, k in enumerate(["speechlike", "noise", "sine"])]
    feats = pipe.feature_extractor(pcm, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    gk = {"num_beams": 1, "do_sample": False, "use_cache": True, "language": "en", "max_new_tokens": 16, "return_timestamps": True,
          "return_token_timestamps": True, "return_segments": True}
    pipe.model.generate(input_features=feats.input_features, attention_mask=feats.attention_mask, generation_config=pipe.generation_config, **gk)
    plan, eng = pipe.model.last_plan, pipe.model.engine
    runs = {}
    for what, policy in (("none", None), ("never", FallbackPolicy(compression_ratio_threshold=None, logprob_threshold=None))):
        eng.log.clear()
        before = dict(eng.calls)
        out = shortform.generate_shortform(eng, plan, feats.input_features, feats.attention_mask, fallback=policy)
        runs[what] = (out, [c[0] for c in eng.log], {k: eng.calls[k] - before[k] for k in before})
    assert runs["none"][1] == runs["never"][1] and set(runs["none"][1]) == {"greedy"} and runs["none"][2] == runs["never"][2]
    a, b = runs["none"][0], runs["never"][0]
    assert torch.equal(a["sequences"], b["sequences"]) and torch.equal(a["token_timestamps"], b["token_timestamps"])


# ---- the backend option ----------------------------------------------------------------------------------------------------------
def test_backend_option_runs_the_ladder_reports_it_and_refuses_an_ineligible_backend():
    from oracle import whisper_oracle as wo
    from tests.oracle_engine import oracle_engine_factory
    from tests.test_score_cpu import build_amd_pipeline, normalise
    from thewhisper_amd import AMDWhisperBackend
    from thewhisper_amd.fallback import FallbackPolicy

    def backend(factory, **kw):
        return AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=build_amd_pipeline("micro", 10, 1, engine_factory=factory), **kw)

    audio = wo.synth_audio(16000 * 7, 7, "speechlike")
    plain = backend(oracle_engine_factory)
    never = backend(sampling_factory, temperature_fallback=FallbackPolicy(compression_ratio_threshold=None, logprob_threshold=None))
    always = backend(sampling_factory, temperature_fallback=(0.0, 0.4, 0.8))       # default thresholds: a random-weight model fails them
    assert isinstance(always.temperature_fallback, FallbackPolicy) and always.temperature_fallback.temperatures == (0.0, 0.4, 0.8)
    for n in (16000 * 6, 16000 * 6 + 8000):            # two ticks: the second carries a draft, which applies to attempt 0 only
        a = plain.transcribe(audio[:n].copy(), 3.0, 16000)
        b = never.transcribe(audio[:n].copy(), 3.0, 16000)
        assert normalise(a) == normalise(b)
        assert never.last_fallback and all(e == {"temperature": 0.0, "attempts": 1} for e in never.last_fallback)
        eng = always.asr_pipeline.model.engine
        eng.log.clear()
        always.transcribe(audio[:n].copy(), 3.0, 16000)
        kinds = [c[0] for c in eng.log]
        assert always.last_fallback and all(e["attempts"] == 3 and e["temperature"] == 0.8 for e in always.last_fallback), always.last_fallback
        assert kinds.count("sample") == 2 * len(always.last_fallback), kinds
    assert never.reuse_stats["draft_tokens"] > 0 and always.reuse_stats["draft_tokens"] > 0
    with pytest.raises(ValueError):
        AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=plain.asr_pipeline, temperature_fallback=(0.0, 0.2), reuse_committed_prefix=True)

    class NoPlanPipeline:       # a pipeline object the short-form loop cannot be restated for: job_codec() is None
        tokenizer = None

        def __call__(self, *a, **k):
            return {"text": "", "chunks": []}

    odd = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=NoPlanPipeline(), temperature_fallback=(0.0, 0.2))
    assert odd.job_codec() is None
    with pytest.raises(ValueError, match="not eligible"):
        odd.transcribe(audio[:16000].copy(), 0.0, 16000)
