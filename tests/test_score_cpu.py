"""Token scores (tw_score_tokens), the parts that need no GPU: the symbol and its argument checks that come before any device call, and
the host plumbing - `shortform.Pass(score=True)`, `generate_shortform(scores_out=...)`, `AMDWhisperBackend(token_scores=True)` on its
plain, `draft_previous_tick` and `reuse_committed_prefix` paths - against stand-in engines whose `score_tokens` returns a KNOWN table:
entry (b, p) = -(p + 1) / 8 - b / 1024 masked, twice that raw, so every number an entry holds says which row and position it came from."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests.oracle_engine import OracleEngine
from tests.stub_engine import StubEngine
from tests.test_pipeline_glue import build_amd_pipeline, normalise

torch.set_grad_enabled(False)


# ---- the library ------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_null_arguments_are_refused_without_a_device(built_library):
    from thewhisper_amd import _cabi

    assert hasattr(ctypes.CDLL(built_library), "tw_score_tokens")
    assert "tw_score_tokens" in [n for n, _, _ in _cabi.SYMBOLS]
    lib = _cabi.load_library()
    ids = (ctypes.c_int32 * 8)(*range(8))
    out = (ctypes.c_float * 8)()
    fp = ctypes.POINTER(ctypes.c_float)
    # a null context, with and without ids: TW_EINVAL before anything touches a device (this machine may have none)
    assert lib.tw_score_tokens(None, 1, ids, 8, 8, 3, None, -1, 0, None, ctypes.cast(out, fp), None, None) == -1
    assert lib.tw_score_tokens(None, 1, None, 8, 8, 3, None, -1, 0, None, None, None, None) == -1
    assert b"tw_score_tokens" in lib.tw_last_error(None)
    assert list(out) == [0.0] * 8


# ---- the known table --------------------------------------------------------------------------------------------------------
def table(seq: np.ndarray, n_prompt: int, eos: int):
    """What tw_score_tokens lays out: 0 for the prompt and behind a row's first eos, the eos itself scored."""
    B, L = seq.shape
    lp = np.zeros((B, L), np.float32)
    for b in range(B):
        for p in range(n_prompt, L):
            lp[b, p] = -(p + 1) / 8 - b / 1024
            if seq[b, p] == eos:
                break
    return lp


class ScoreMixin:
    def score_tokens(self, sequences, n_prompt, *, no_speech_id=None, no_speech_pos=0, eos_id=50257, **kw):
        seq = np.asarray(sequences)
        self.score_calls.append(dict(seq=seq.copy(), n_prompt=int(n_prompt), no_speech_id=no_speech_id, no_speech_pos=no_speech_pos,
                                     eos_id=eos_id, kw=dict(kw)))
        lp = table(seq, n_prompt, eos_id)
        ns = None if no_speech_id is None else np.array([0.25 + b / 64 for b in range(seq.shape[0])], np.float32)
        return {"logprob": lp, "logprob_raw": 2 * lp, "no_speech_prob": ns}


EOS, PAD, TS0 = 90, 90, 100      # the stub's vocabulary: text below 90, timestamps from 100


class ScriptedEngine(ScoreMixin, StubEngine):
    """StubEngine whose greedy call returns the next scripted batch of sequences (prompt included, padded with eos)."""
    T = 50
    max_batch = 4

    def __init__(self, script):
        super().__init__()
        self.script, self.score_calls, self.order = list(script), [], []

    def encode(self, mel, **kw):
        return None

    def cross_kv(self, B, **kw):
        pass

    def generate_greedy(self, prompt, **kw):
        self.order.append("greedy")
        seq = np.asarray(self.script.pop(0), np.int64)
        assert seq.shape[0] == prompt.shape[0] and np.array_equal(seq[:, : prompt.shape[1]], prompt)
        return {"sequences": seq, "length": seq.shape[1]}

    def token_timestamps(self, B, n_prompt, L, nf, *a):
        self.order.append("dtw")
        return np.zeros((B, L), np.float32)

    def score_tokens(self, *a, **kw):
        self.order.append("score")
        return super().score_tokens(*a, **kw)


def scripted_plan():
    from thewhisper_amd.shortform import ShortFormPlan

    greedy = dict(max_new_tokens=8, min_new_tokens=0, max_length=448, eos_id=EOS, pad_id=PAD, want_alignment=True, timestamps=True,
                  no_timestamps_id=TS0 - 1, max_initial_timestamp_index=50, begin_suppress=(7, EOS), suppress=(1, 2))
    return ShortFormPlan(init_tokens=(3, 4, 5), greedy=greedy, eos=EOS, pad=PAD, timestamp_begin=TS0, return_timestamps=True,
                         return_token_timestamps=True, return_segments=True, result_is_dict=True)


# iteration 1: row 0 ends with eos early (padding behind it), row 1 fills the budget WITHOUT an eos and closes a segment at 0.20 s
# (frame 20 of 100), so that its chunk needs a second iteration; iteration 2 (row 1 alone): one short segment, eos
IT1 = [[3, 4, 5, 100, 11, 12, 110, EOS, PAD, PAD, PAD],
       [3, 4, 5, 100, 21, 110, 110, 22, 23, 24, 25]]
IT2 = [[3, 4, 5, 100, 31, 150, EOS]]


def test_pass_appends_one_entry_per_seek_iteration_and_changes_nothing_else():
    from thewhisper_amd import shortform

    plan = scripted_plan()

    def run(score):
        eng = ScriptedEngine([IT1, IT2])
        works = [shortform.ChunkWork(torch.zeros(8, 100), 100) for _ in range(2)]
        shortform.run_pass(eng, plan, works, score=score, no_speech_id=77 if score else None)
        assert works[0].done and not works[1].done and works[1].seek == 20
        shortform.run_pass(eng, plan, [works[1]], score=score, no_speech_id=77 if score else None)
        assert works[1].done
        return eng, works

    eng0, plain = run(False)
    eng, works = run(True)
    assert eng0.score_calls == [] and all(w.scores == [] for w in plain)
    assert eng0.order == ["greedy", "dtw", "greedy", "dtw"]
    assert eng.order == ["greedy", "dtw", "score", "greedy", "dtw", "score"]       # after the greedy call AND the token timestamps
    # the decoding state is what it is without the option
    for a, b in zip(plain, works):
        assert a.seek == b.seek and a.passes == b.passes and len(a.segments) == len(b.segments)
        for sa, sb in zip(a.segments, b.segments):
            assert torch.equal(sa["tokens"], sb["tokens"]) and float(sa["start"]) == float(sb["start"]) and float(sa["end"]) == float(sb["end"])
    # what the engine was asked: the call's sequences, the plan's prompt length as begin index, the plan's processors
    c1, c2 = eng.score_calls
    assert np.array_equal(c1["seq"], np.asarray(IT1)) and np.array_equal(c2["seq"], np.asarray(IT2))
    for c in (c1, c2):
        assert c["n_prompt"] == 3 and c["no_speech_id"] == 77 and c["no_speech_pos"] == 0 and c["eos_id"] == EOS
        assert c["kw"]["timestamps"] is True and c["kw"]["suppress"] == (1, 2) and c["kw"]["begin_suppress"] == (7, EOS)
    assert [len(w.scores) for w in works] == [1, 2]
    # row 0: four tokens and the eos; the padding behind it is in no entry
    e = works[0].scores[0]
    assert e["tokens"].tolist() == [100, 11, 12, 110]
    want = np.array([-(p + 1) / 8 for p in range(3, 8)], np.float32)
    assert np.array_equal(e["logprob"], want) and np.array_equal(e["logprob_raw"], 2 * want)
    assert e["avg_logprob"] == pytest.approx(float(want.astype(np.float64).sum()) / 5, abs=0, rel=1e-12)
    assert e["no_speech_prob"] == 0.25
    # row 1, iteration 1: the budget ran out, no eos: eight tokens, eight numbers, the divisor stays n_tokens + 1
    e = works[1].scores[0]
    assert e["tokens"].tolist() == IT1[1][3:]
    want = np.array([-(p + 1) / 8 - 1 / 1024 for p in range(3, 11)], np.float32)
    assert np.array_equal(e["logprob"], want)
    assert e["avg_logprob"] == pytest.approx(float(want.astype(np.float64).sum()) / 9, abs=0, rel=1e-12)
    assert e["no_speech_prob"] == 0.25 + 1 / 64
    # row 1, iteration 2 (row 0 of its own pass)
    e = works[1].scores[1]
    assert e["tokens"].tolist() == [100, 31, 150] and len(e["logprob"]) == 4
    assert e["avg_logprob"] == pytest.approx(sum(-(p + 1) / 8 for p in range(3, 7)) / 4, abs=0, rel=1e-12)


def test_generate_shortform_collects_the_entries_row_by_row():
    from thewhisper_amd import shortform

    plan = scripted_plan()
    feats, mask = torch.zeros(2, 8, 100), torch.ones(2, 100, dtype=torch.long)
    plain = shortform.generate_shortform(ScriptedEngine([IT1, IT2]), plan, feats, mask)
    got: list = []
    eng = ScriptedEngine([IT1, IT2])
    out = shortform.generate_shortform(eng, plan, feats, mask, scores_out=got, no_speech_id=None)
    assert torch.equal(out["sequences"], plain["sequences"]) and torch.equal(out["token_timestamps"], plain["token_timestamps"])
    assert [e["tokens"].tolist() for e in got] == [[100, 11, 12, 110], IT1[1][3:], [100, 31, 150]]
    assert all(e["no_speech_prob"] is None for e in got) and all(c["no_speech_id"] is None for c in eng.score_calls)


# ---- the backend ------------------------------------------------------------------------------------------------------------
class ScoringOracleEngine(ScoreMixin, OracleEngine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.score_calls = []

    def generate_greedy(self, prompt, **kw):
        out = super().generate_greedy(prompt, **kw)
        self.last_sequences = np.asarray(out["sequences"]).copy()
        return out


def scoring_factory(dims, T, max_batch, dtype, alignment_heads, device_index):
    return ScoringOracleEngine(dims, T, max_batch, dtype, alignment_heads, device_index)


def backend(token_scores, factory, **kw):
    from thewhisper_amd import AMDWhisperBackend

    return AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=build_amd_pipeline("micro", 10, 1, engine_factory=factory),
                             token_scores=token_scores, **kw)


def check_entries(b, eng, n_before):
    """`last_scores` = one entry per greedy call this `transcribe` made, each the table's numbers for that call's sequences."""
    n = len(b.last_scores)
    assert 1 <= n <= len(eng.score_calls) - n_before         # (a backend's first reuse / draft call also learns its plan from a call of its own)
    calls = eng.score_calls[-n:]
    for e, c in zip(b.last_scores, calls):
        seq, n0 = c["seq"], c["n_prompt"]
        assert seq.shape[0] == 1 and c["no_speech_id"] == b.no_speech_id
        row = seq[0, n0:]
        stop = np.flatnonzero(row == c["eos_id"])
        n_tok = int(stop[0]) if stop.size else len(row)
        assert e["tokens"].tolist() == row[:n_tok].tolist()
        lp = table(seq, n0, c["eos_id"])[0, n0 : n0 + n_tok + (1 if stop.size else 0)]
        assert np.array_equal(e["logprob"], lp) and np.array_equal(e["logprob_raw"], 2 * lp)
        assert e["avg_logprob"] == pytest.approx(float(lp.astype(np.float64).sum()) / (n_tok + 1), abs=0, rel=1e-12)
        assert e["no_speech_prob"] == (None if b.no_speech_id is None else 0.25)


@pytest.mark.parametrize("mode", [dict(draft_previous_tick=False), dict(draft_previous_tick=True), dict(reuse_committed_prefix=True)],
                         ids=["plain", "draft_previous_tick", "reuse_committed_prefix"])
def test_backend_scores_travel_beside_identical_words(mode):
    from tests.oracle_engine import oracle_engine_factory

    off = backend(False, oracle_engine_factory, **mode)
    on = backend(True, scoring_factory, **mode)
    assert off.token_scores is False and off.last_scores == [] and on.last_scores == []
    vocab = on.asr_pipeline.tokenizer.get_vocab()
    want_id = vocab.get("<|nospeech|>", vocab.get("<|nocaptions|>"))
    assert on.no_speech_id == want_id
    eng = on.asr_pipeline.model.engine
    audio = wo.synth_audio(16000 * 7, 7, "speechlike")
    for n in (16000 * 6, 16000 * 6 + 8000, 16000 * 7):           # three ticks of one stream: the buffer grows by 0.5 s
        n_before = len(eng.score_calls)
        a = off.transcribe(audio[:n].copy(), 3.0, 16000)
        b = on.transcribe(audio[:n].copy(), 3.0, 16000)
        assert normalise(a) == normalise(b) and all(set(w) == {"text", "start", "end"} for w in b)
        check_entries(on, eng, n_before)
        if mode.get("draft_previous_tick") or mode.get("reuse_committed_prefix"):
            assert on.last_scores[0]["tokens"].tolist() == on._last["ids"].tolist()      # the call's first-pass tokens
    assert off.last_scores == [] and off.asr_pipeline.model.score_sink is None and on.asr_pipeline.model.score_sink is None
    if mode.get("draft_previous_tick") or mode.get("reuse_committed_prefix"):
        assert on.reuse_stats["reused"] >= 1
        # forced / drafted tokens count as generated: the begin index stays the plan's prompt length
        assert {c["n_prompt"] for c in eng.score_calls} == {on._reuse_codec.plan.n_prompt}


def test_transcribe_many_scores_every_request():
    from tests.oracle_engine import oracle_engine_factory

    off, on = backend(False, oracle_engine_factory), backend(True, scoring_factory)
    eng = on.asr_pipeline.model.engine
    reqs = [(wo.synth_audio(16000 * 4, s, "speechlike"), 1.0 * s, 16000) for s in (1, 2)]
    assert normalise(off.transcribe_many(reqs)) == normalise(on.transcribe_many(reqs))
    assert len(on.last_scores) == len(eng.score_calls) >= 2
    n_before = len(eng.score_calls)
    on.transcribe(reqs[0][0], 0.0, 16000)                        # `last_scores` is of the MOST RECENT call only
    check_entries(on, eng, n_before)
    assert len(on.last_scores) == 1
