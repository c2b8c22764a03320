"""Top-k / top-p filtering of the temperature sampler, the parts that need no GPU: the numpy mirror of the rule (tests/filter_judge.py)
against the warpers of the installed transformers and against the renormalised softmax it claims to draw from; the mirror's own run
of every case the GPU test replays (the conditions demanded there hold for a correct sampler, and an engine that ignored the filter
would be found wrong); host validation of `generate_sample(top_k=, top_p=)` and of `FallbackPolicy`; the policy's filter on its way
through `generate_with_fallback`, `Pass` and the backend on stand-in engines; the C ABI's new struct and symbol."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import filter_judge as fj
from tests import sample_judge as sm
from tests import sampler_judge as sj
from tests.stub_engine import StubEngine

N_PROMPT = 3


# ---- the mirror is HF's rule ---------------------------------------------------------------------------------------------------
def _planted_row(V: int, rng) -> np.ndarray:
    x = (rng.standard_normal(V) * 3.0).astype(np.float32)
    x[rng.random(V) < 0.1] = -np.inf
    order = np.argsort(-np.where(np.isfinite(x), x, -np.inf))
    for k in (8, 50):                 # exact ties at the k-th value: the (k+1)-th and (k+2)-th largest repeat it
        x[order[k]] = x[order[k + 1]] = x[order[k - 1]]
        order = np.argsort(-np.where(np.isfinite(x), x, -np.inf), kind="stable")
    return x


@pytest.mark.parametrize("V", [66, 1000, 51865])
def test_the_mirror_s_kept_set_is_hf_s(V):
    """TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper of the installed transformers on seeded float32 rows with
    masked entries and planted exact ties at the 8th and 50th value: their finite entries are the mirror's kept set.  A case is left
    out only when a membership lies inside TOPP_BAND (HF's cumulative sum is float32 arithmetic): at most 1 % of the cases.
    One difference is the rule's own, not arithmetic: HF's top-p walks a SORTED row, so of several exactly equal values it may keep
    some and drop the others (whichever its sort put first), where this project's rule lets equal values share their fate - it keeps
    the whole group iff HF keeps its first member.  With planted ties that happens (V = 66, T = 1, k = 8, p = 0.9 cuts through the
    three equal values at the 8th place), so the comparison is with HF's set closed under equality of y, which is HF's set itself
    whenever no group of equal values straddles its cut."""
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

    rng = np.random.default_rng(1000 + V)
    rows = [_planted_row(V, rng) for _ in range(3)]
    cases = left_out = ties_kept = straddled = 0
    for x, (T, k, p) in itertools.product(rows, itertools.product((0.2, 0.6, 1.0), (0, 1, 8, 50, V + 5), (1.0, 0.9, 0.3))):
        cases += 1
        s = TemperatureLogitsWarper(float(T))(None, torch.from_numpy(x)[None].clone())
        if k > 0:
            s = TopKLogitsWarper(top_k=int(k))(None, s)
        if p < 1:
            s = TopPLogitsWarper(top_p=float(p))(None, s)
        hf = torch.isfinite(s[0]).numpy()
        keep, margin = fj.kept_margins(x, sm.inv_t32(T), k, p)
        if p < 1:
            y = (x * sm.inv_t32(T)).astype(np.float32)
            straddled += int((fj.kept(x, sm.inv_t32(T), k, 1.0) & ~hf & np.isin(y, y[hf])).any())
            hf = hf | (fj.kept(x, sm.inv_t32(T), k, 1.0) & np.isin(y, y[hf]))
        if (margin <= fj.TOPP_BAND).any() and not np.array_equal(hf, keep):
            left_out += 1
            continue
        assert np.array_equal(hf, keep), (V, T, k, p, np.flatnonzero(hf != keep)[:5])
        if k in (8, 50) and p == 1.0:
            assert int(keep.sum()) == k + 2, (k, int(keep.sum()))      # the planted ties at the k-th value are kept, by both
            ties_kept += 1
    print(f"V = {V}: {cases} cases, {left_out} left out, planted ties kept in {ties_kept}, HF's cut inside a group of equal values in {straddled}")
    assert left_out * 100 <= cases and ties_kept == 3 * 3 * 2


def test_top_k_edges():
    x = np.asarray([1.0, -np.inf, 3.0, 3.0, 2.0, -0.0, 0.0], dtype=np.float32)
    assert fj.kept(x, 1.0, 1, 1.0).tolist() == [False, False, True, True, False, False, False]      # ties at the maximum
    assert fj.kept(x, 1.0, 6, 1.0).tolist() == [True, False, True, True, True, True, True]          # k = |S|: tau is the minimum
    assert fj.kept(x, 1.0, 5, 1.0).tolist() == [True, False, True, True, True, True, True]          # -0 and +0 tie
    assert fj.kept(x, 1.0, 100, 1.0).tolist() == (x > -np.inf).tolist() == fj.kept(x, 1.0, 0, 1.0).tolist()
    assert fj.kept(x, 1.0, 0, 1e-6).tolist() == [False, False, True, True, False, False, False]      # the maximum is always kept
    assert not fj.kept(np.full(5, -np.inf, np.float32), 1.0, 2, 0.5).any()


def test_the_mirror_draws_from_the_renormalised_softmax_over_the_kept_set():
    """tests/test_sample_cpu.py's chi-square with a filter: 20 000 draws on a fixed 16-logit vector at T = 0.6, k = 9, p = 0.9, key
    (123, 456), position = draw index, against softmax(x / T) renormalised over the kept set; nothing outside it is ever drawn."""
    x = np.random.default_rng(11).standard_normal(16).astype(np.float32) * 1.5
    T, n = 0.6, 20000
    seed = 123 | (456 << 32)
    keep = fj.kept(x, sm.inv_t32(T), 9, 0.9)
    assert 3 <= int(keep.sum()) < 9, keep
    counts = np.zeros(16)
    for p in range(n):
        counts[int(np.argmax(np.where(keep, sm.scores(x, T, p, seed, 0), -np.inf)))] += 1
    z = x.astype(np.float64) * float(sm.inv_t32(T))
    prob = np.where(keep, np.exp(z - z.max()), 0.0)
    prob /= prob.sum()
    assert counts[~keep].sum() == 0
    chi2 = float(((counts[keep] - n * prob[keep]) ** 2 / (n * prob[keep])).sum())
    dof = int(keep.sum()) - 1
    bound = {2: 13.8, 3: 16.3, 4: 18.5, 5: 20.5, 6: 22.5, 7: 24.3}[dof]          # the 0.001 points
    print(f"chi-square {chi2:.1f} ({dof} degrees of freedom)")
    assert chi2 < bound, chi2


# ---- the cases carry -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in fj.FILTER_CASES if not c.graph])
def test_the_mirror_s_own_run_meets_what_the_gpu_test_demands(name):
    bf = fj.build_filter_case(fj.filter_case_by_name(name))
    seqs, lg = fj.mirror_run(bf)
    v = fj.judge_case(bf, lg, seqs, N_PROMPT)
    print(f"{name}: {v.summary()}")
    fj.check_conditions(v, name)
    assert not bf.case.tau_inf or v.tau_inf_mass > 0, "no step where the mass rule fired with fewer than k ids left"
    assert not bf.case.ties or v.tie_at_tau > 0, "no step with ties at the top-k threshold"
    t = bf.sample.temperature
    assert np.array_equal(seqs[:, :N_PROMPT], bf.built.prompt) and (seqs[t < 0, N_PROMPT:] == bf.built.opt.pad).all()
    # an engine that ignores the filter: the unfiltered mirror's sequences, judged as a filtered call's, are wrong
    plain, lg_plain = sm.mirror_run(bf.sample)
    w = fj.judge_case(bf, lg_plain, plain, N_PROMPT)
    assert w.count("wrong") > 0, "the judge does not see an ignored filter"


def test_between_them_the_cases_reach_the_corners():
    cases = {c.name: c for c in fj.FILTER_CASES}
    assert any(c.tau_inf for c in cases.values()) and any(c.ties for c in cases.values())
    mixed = fj.build_filter_case(cases["v1000-b33-mixed"])
    assert int(mixed.top_k.max()) > mixed.built.dims.vocab                      # k above the number of ids there are
    assert {(int(k), float(np.float32(p))) for k, p in zip(mixed.top_k, mixed.top_p)} == {(k, float(np.float32(p))) for k, p in fj.MIXED_FILTERS}
    t = mixed.sample.temperature
    assert (mixed.top_k[t == np.float32(0.2)] == 2000).all() and (mixed.top_k[t == np.float32(0.6)] == 8).all() and (mixed.top_k[t == 1.0] == 50).all()


# ---- host validation ------------------------------------------------------------------------------------------------------------
def test_filter_rows_validates_with_the_library_s_rules():
    from thewhisper_amd.engine import filter_rows

    assert filter_rows(None, None, 4) is None and filter_rows(0, 1.0, 4) is None and filter_rows([0, 0], [1.0, 1.0], 2) is None
    k, p = filter_rows(50, None, 3)
    assert k.dtype == np.int32 and k.tolist() == [50, 50, 50] and p.dtype == np.float32 and p.tolist() == [1.0, 1.0, 1.0]
    k, p = filter_rows(None, [0.5, 1.0], 2)
    assert k.tolist() == [0, 0] and p.tolist() == [0.5, 1.0]
    k, p = filter_rows([0, 8, 2 ** 40], 0.25, 3)
    assert k.tolist() == [0, 8, 2 ** 31 - 1] and k.flags["C_CONTIGUOUS"] and p.flags["C_CONTIGUOUS"]
    for bad in (dict(top_k=-1, top_p=None), dict(top_k=[1, -2], top_p=None), dict(top_k=1.5, top_p=None), dict(top_k=[1, 2, 3], top_p=None),
                dict(top_k=None, top_p=0.0), dict(top_k=None, top_p=1.5), dict(top_k=None, top_p=float("nan")), dict(top_k=None, top_p=[0.5, -0.1]),
                dict(top_k=None, top_p=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError):
            filter_rows(bad["top_k"], bad["top_p"], 2)


def test_fallback_policy_validates_and_defaults_to_off():
    from thewhisper_amd.fallback import FallbackPolicy, as_policy

    d = FallbackPolicy()
    assert d.top_k is None and d.top_p is None and as_policy((0.0, 0.4)).top_k is None
    q = FallbackPolicy(top_k=50, top_p=0.9)
    assert (q.top_k, q.top_p) == (50, 0.9) and as_policy(q) is q
    for bad in (dict(top_k=-1), dict(top_k=2.5), dict(top_k=True), dict(top_p=0.0), dict(top_p=1.01), dict(top_p=float("nan"))):
        with pytest.raises(ValueError):
            FallbackPolicy(**bad)


class _LadderStub(StubEngine):
    """tests/stub_engine.StubEngine with the sampling and scoring surface `generate_with_fallback` drives: every row fails the
    compression check (one token repeated), so every temperature is tried; the keywords of every sampling call are logged."""
    vocab = 1000

    def __init__(self):
        super().__init__()
        self.sample_kw = []

    def generate_greedy(self, prompt, max_new_tokens=128, **kw):
        B, n0 = np.asarray(prompt).shape
        return {"sequences": np.full((B, n0 + 40), 7, np.int64), "length": n0 + 40}

    def generate_sample(self, prompt, temperature, seed, offset=None, **kw):
        self.sample_kw.append(dict(kw))
        return self.generate_greedy(prompt)

    def score_tokens(self, sequences, n_prompt, **kw):
        B, L = np.asarray(sequences).shape
        return {"logprob": np.full((B, L), -0.1, np.float32), "logprob_raw": np.full((B, L), -0.1, np.float32), "no_speech_prob": None}


def test_generate_with_fallback_hands_the_filter_to_every_sampled_attempt():
    from thewhisper_amd import fallback as fb

    prompt = np.full((2, 3), 5, np.int32)
    kw = dict(max_new_tokens=40, eos_id=999, pad_id=999)
    for policy, want in ((fb.FallbackPolicy(temperatures=(0.0, 0.4, 0.8)), {}),
                         (fb.FallbackPolicy(temperatures=(0.0, 0.4, 0.8), top_k=50), {"top_k": 50}),
                         (fb.FallbackPolicy(temperatures=(0.0, 0.4, 0.8), top_k=8, top_p=0.9), {"top_k": 8, "top_p": 0.9})):
        eng = _LadderStub()
        res = fb.generate_with_fallback(eng, prompt, kw, policy, None, [1, 2], [0, 16])
        assert len(eng.sample_kw) == 2 and all({n: k[n] for n in ("top_k", "top_p") if n in k} == want for k in eng.sample_kw), eng.sample_kw
        assert all(r["attempts"] == 3 and r["top_k"] == policy.top_k and r["top_p"] == policy.top_p for r in res)


def _filtering_factory():
    from tests.test_sample_cpu import SamplingOracleEngine

    class FilteringOracleEngine(SamplingOracleEngine):
        def generate_sample(self, prompt, temperature, seed, offset=None, top_k=None, top_p=None, **kw):
            B = np.asarray(prompt).shape[0]
            t = np.broadcast_to(np.asarray(temperature, dtype=np.float32), (B,))
            self.calls["generate"] += 1
            self.log.append(("sample", t.copy(), np.asarray(seed).copy(), np.asarray(offset).copy(), top_k, top_p))
            seqs, _ = fj.mirror_generate(self.model, self._enc[:B], prompt, sm.options_of(kw), t, seed, offset, top_k or 0, top_p or 1.0)
            return {"sequences": seqs, "length": int(seqs.shape[1])}

    return FilteringOracleEngine


def test_pass_and_the_backend_pick_the_policy_s_filter_up():
    import dataclasses

    from tests.test_sample_cpu import LADDER, _plan, _run_pass
    from thewhisper_amd import fallback as fb

    dims, w, prompt, opt, kw = sm.repeating_model()
    eng = _filtering_factory()(dataclasses.asdict(dims), sj.T_FRAMES, 4, "f32", [])
    eng.model = sj._OracleExactTies(dims, w, T=sj.T_FRAMES)
    eng.encode(torch.zeros((4, dims.n_mels, 2 * sj.T_FRAMES)))
    policy = fb.FallbackPolicy(**LADDER, top_k=8)
    works, p = _run_pass(eng, _plan(kw, (3, 5, sm.STICKY[0]), dims.vocab), dims, 4, policy, score=True)
    sampled = [c for c in eng.log if c[0] == "sample"]
    assert sampled and all(c[4] == 8 and c[5] is None for c in sampled)
    assert all(r["top_k"] == 8 and r["top_p"] is None for r in p.last_fallback)
    assert any(x.attempts[0] > 1 for x in works)


def test_the_backend_reports_the_filter_in_last_fallback():
    from oracle import whisper_oracle as wo
    from tests.test_score_cpu import build_amd_pipeline
    from thewhisper_amd import AMDWhisperBackend
    from thewhisper_amd.fallback import FallbackPolicy

    Eng = _filtering_factory()
    pipe = build_amd_pipeline("micro", 10, 1, engine_factory=lambda *a: Eng(*a))
    be = AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=pipe, temperature_fallback=FallbackPolicy(temperatures=(0.0, 0.4), top_k=50))
    be.transcribe(wo.synth_audio(16000 * 6, 7, "speechlike"), 3.0, 16000)
    eng = pipe.model.engine
    sampled = [c for c in eng.log if c[0] == "sample"]
    assert sampled and all(c[4] == 50 for c in sampled), eng.log
    assert be.last_fallback and all(e["top_k"] == 50 and e["top_p"] is None and e["attempts"] == 2 for e in be.last_fallback), be.last_fallback


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_struct_size_and_the_symbol(built_library):
    from thewhisper_amd import _cabi

    assert ctypes.sizeof(_cabi.tw_filter_opts) == 16 and ctypes.sizeof(_cabi.tw_sample_opts) == 24
    lib = ctypes.CDLL(built_library)
    assert hasattr(lib, "tw_generate_sample_filtered") and "tw_generate_sample_filtered" in [n for n, _, _ in _cabi.SYMBOLS]
    lib = _cabi.load_library()
    assert lib.tw_generate_sample_filtered(None, 1, None, 3, None, None, None, None, None, None) == -1     # refused before any device call
    assert b"tw_generate_sample_filtered" in lib.tw_last_error(None)
