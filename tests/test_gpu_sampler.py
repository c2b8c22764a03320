"""The greedy sampler (k_decode.hip: sampler_part_kernel, sampler_merge, sampler_finish_kernel, sampler_rows_finish_kernel,
suppress_bitmap_kernel) judged on the engine's OWN logits, on the crafted zero-layer models of tests/sampler_judge.py.

With no decoder layer a step's logits are a function of the input token and its position, so the sequence `generate_greedy` returned, fed
back through `decode_step`, reproduces the logits its sampler read.  `sampler_judge.judge` then says per step and stream whether the
appended token is the one HF's processors + argmax pick from THOSE logits: equality of ids, ties included, GEMM rounding out of the
comparison.  Every case asserts
  * no step wrong, at most 1 % undecided (|logsumexp(timestamps) - max(text)| <= 1e-4, the one float32-summation-order decision);
  * the rules and planted ties the case is there for were decisive in the ENGINE's run (a case that exercises nothing fails);
  * the duplicated embedding rows are bit-equal columns of the replayed logits, so the ties exist;
  * where the case asks: the replayed logits against a float64 restatement, rel_l2 < 2e-5 (the suite's strict-f32 bound).
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_sampler.py -s`` prints each case's figures.
"""
import numpy as np
import pytest
import torch

from tests import sampler_judge as sj
from tests.util import make_engine, rel_l2

pytestmark = pytest.mark.gpu
N_PROMPT = 3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _engine(built):
    c = built.case
    eng = make_engine(built.dims, built.weights, T=sj.T_FRAMES, max_batch=c.B, dtype=c.dtype, use_graph=c.graph)
    eng.encode(torch.zeros((c.B, built.dims.n_mels, 2 * sj.T_FRAMES), dtype=torch.float32).cuda())     # the zero-layer decoder never reads it
    eng.cross_kv(c.B)
    return eng


def _replay(eng, seqs):
    """[L-1, B, V] float32: the logits of positions 0 .. L-2 of `seqs`, by teacher-forced steps."""
    B, L = seqs.shape
    eng.decoder_reset(B)
    return np.stack([eng.decode_step(seqs[:, s].tolist()).cpu().numpy() for s in range(L - 1)])


def _check_verdict(built, v, what):
    print(f"{what}: {v.summary()}")
    assert v.count("wrong") == 0, (what, v.wrong[:3])
    assert v.count("undecided") * 100 <= v.judged, (what, v.count("undecided"), v.judged)


def _check_planted_columns(built, lg, what):
    for kind, pairs in built.planted.items():
        for lo, hi in pairs:
            assert np.array_equal(lg[..., lo], lg[..., hi]), f"{what}: duplicated rows {lo} and {hi} ({kind}) are not bit-equal columns of the logits"


@pytest.mark.parametrize("name", [c.name for c in sj.CASES])
def test_sampler_picks_what_the_processors_pick_from_its_own_logits(name):
    built = sj.build_case(sj.case_by_name(name))
    c = built.case
    eng = _engine(built)
    try:
        out = eng.generate_greedy(built.prompt, **built.kw)
        seqs = out["sequences"]
        assert seqs.shape == (c.B, out["length"]) and np.array_equal(seqs[:, :N_PROMPT], built.prompt)
        lg = _replay(eng, seqs)
    finally:
        eng.close()
    assert np.isfinite(lg).all()
    v = sj.judge(lg, seqs, N_PROMPT, built.opt)
    _check_verdict(built, v, name)
    assert v.judged == c.B * (seqs.shape[1] - N_PROMPT) and v.judged >= 40
    _check_planted_columns(built, lg, name)
    got = {r for r, at in v.decisive.items() if at}
    assert set(c.expect) <= got, (name, "rules never decisive:", sorted(set(c.expect) - got))
    seen = sj.tie_kinds_seen(built, v)
    assert set(c.expect_ties) <= seen, (name, "planted ties never at the maximum:", sorted(set(c.expect_ties) - seen))
    if c.suppress == "all":                                  # everything masked: token 0 until max_new
        assert seqs.shape[1] == N_PROMPT + c.max_new and (seqs[:, N_PROMPT:] == 0).all()
    if c.min_new:                                            # eos held back to the last step
        assert seqs.shape[1] == N_PROMPT + c.max_new and not (seqs[:, N_PROMPT:-1] == c.eos).any()
    if c.check_logits:                                       # the vocabulary edge of the logits projection, strict f32
        worst = max(rel_l2(lg[s], sj.logits_f64(built.weights, seqs[:, s], s)) for s in range(seqs.shape[1] - 1))
        print(f"{name}: logits vs float64 restatement, worst step rel_l2 {worst:.2e}")
        assert worst < 2e-5, (name, worst)


@pytest.mark.parametrize("graph", [False, True])
def test_forced_and_draft_calls_are_judged_ok_and_equal_the_plain_call(graph):
    """tw_greedy_opts::n_forced with a forced prefix that ends in an opening timestamp (the call seeds the last timestamp from forced
    tokens; the closing timestamp and a text token follow), tw_greedy_opts::n_draft with the true continuation and with one token of it
    corrupted (sampler_rows_finish_kernel recomputes the last timestamp per row): the plain call's sequences, judged all ok."""
    import dataclasses
    built = sj.build_case(dataclasses.replace(sj.case_by_name("v1000-ts-odd"), graph=graph))
    c = built.case
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        lg = _replay(eng, plain)
        v = sj.judge(lg, plain, N_PROMPT, built.opt)
        _check_verdict(built, v, f"plain graph={graph}")
        _check_planted_columns(built, lg, "plain")

        # the forced prefix ends in stream 0's first opening timestamp (a text token before it) behind which the open pair or the last
        # timestamp DECIDES the token in the engine's own run: a call that did not seed them from the forced / redone tokens would pick
        # another token there.  The closing timestamp and then a text token follow
        seeded = sorted(s for r in ("pair_ts_text", "mono_same") for s, b in v.decisive[r] if b == 0)
        assert seeded, "no step of stream 0 is decided by pair_ts_text or mono_same"
        n_forced = seeded[0] + 1 - N_PROMPT
        r = plain[0, N_PROMPT + n_forced - 2: N_PROMPT + n_forced + 2]
        assert r[0] <= c.no_ts < r[1] and r[2] > c.no_ts and r[3] <= c.no_ts, r
        gen = plain[:, N_PROMPT:]
        n_ok = min(int(np.argmax(np.append(r == c.eos, True))) for r in gen)       # tokens before any row's eos / padding
        n_ok = min(n_ok, c.max_new - 2)
        assert n_forced <= n_ok, "the case needs every stream unfinished at the end of the forced prefix"
        calls = {"forced": (plain[:, : N_PROMPT + n_forced], dict(n_forced=n_forced))}
        draft = plain[:, : N_PROMPT + n_ok].copy()
        calls["draft, all correct"] = (draft, dict(n_draft=n_ok))
        bad = draft.copy()
        at = N_PROMPT + n_forced - 1                                                 # stream 0's opening timestamp becomes a text token
        assert bad[0, at] > c.no_ts
        bad[0, at] = 1
        calls["draft, one token corrupted"] = (bad, dict(n_draft=n_ok))
        for what, (prompt, kw) in calls.items():
            out = eng.generate_greedy(prompt.astype(np.int32), **built.kw, **kw)
            assert np.array_equal(out["sequences"], plain), what
            if "n_draft" in kw:
                dr = out["draft"]
                assert dr["offered"] == n_ok * c.B, (what, dr)
                assert (dr["accepted"] == n_ok * c.B) == (prompt is draft), (what, dr)
            lg2 = _replay(eng, out["sequences"])
            assert np.array_equal(lg2, lg), what
            v2 = sj.judge(lg2, out["sequences"], N_PROMPT, built.opt)
            _check_verdict(built, v2, f"{what} graph={graph}")
            assert v2.judged == v.judged and v2.count("ok") + v2.count("undecided") == v2.judged
    finally:
        eng.close()


@pytest.mark.parametrize("pad", ["eos", 5])
def test_drafts_behind_a_finished_row_are_judged_ok_and_equal_the_plain_call(pad):
    """tw_greedy_opts::n_draft with drafts that run past a row's <eos>, on case v127-b6: by the oracle (tests/test_eos_model.py) rows 1, 3
    and 4 end after 9 tokens and rows 0, 2 and 5 never.  Every row's true continuation up to max_new - 2 with filler that is not <eos>
    behind the finished rows' ends, and the same with one token of a row that goes on corrupted behind those ends: the plain call's
    sequences, no step judged wrong, and in rows 1, 3 and 4 it is the padding rule that decides steps (the arg-max there is not pad).
    pad = 5: this model answers <eos> with <eos>, so with pad_id = eos_id (the case as it stands) a call that decoded a finished row on
    would return the same ids; with another pad_id it does not."""
    import dataclasses

    from tests import eos_model as em
    built = sj.build_case(sj.case_by_name("v127-b6"))
    c = built.case
    pad = c.eos if pad == "eos" else int(pad)
    kw = dict(built.kw, pad_id=pad)
    opt = dataclasses.replace(built.opt, pad=pad)
    eng = _engine(built)
    try:
        plain = eng.generate_greedy(built.prompt, **kw)["sequences"]
        lg = _replay(eng, plain)
        v = sj.judge(lg, plain, N_PROMPT, opt)
        _check_verdict(built, v, f"plain v127-b6 pad={pad}")
        gen = plain[:, N_PROMPT:]
        steps = em.eos_steps(gen, c.eos)
        print(f"v127-b6: rows end after {['-' if s is None else s for s in steps]} tokens")
        assert steps == [None, 9, None, 9, 9, None], steps
        for b in (1, 3, 4):
            assert (gen[b, 10:] == pad).all()
        padded = {b for _, b in v.decisive["pad_after_eos"]}
        assert {1, 3, 4} <= padded, ("pad_after_eos never decisive in a finished row", sorted(padded))
        n = em.draft_span(gen, c.max_new, c.eos)
        assert n == c.max_new - 2
        a = em.filled_draft(gen, n, np.random.default_rng(17), eos=c.eos)
        calls = {"(a) true continuations, filler behind the finished rows": a,
                 "(c) one token of row 0 wrong behind the finished rows' ends": em.corrupt(a, 0, 9 + (n - 9) // 2, c.eos)}
        for what, draft in calls.items():
            out = eng.generate_greedy(np.concatenate([built.prompt, draft], axis=1).astype(np.int32), n_draft=n, **kw)
            print(f"  {what}: {out['draft']}")
            assert out["draft"]["offered"] == n * c.B and out["draft"]["rounds"] >= 1
            lg2 = _replay(eng, out["sequences"])           # judged on its own before it is compared: a token behind <eos> is `wrong`
            v2 = sj.judge(lg2, out["sequences"], N_PROMPT, opt)
            _check_verdict(built, v2, what)
            assert np.array_equal(out["sequences"], plain), (what, out["draft"])
            assert np.array_equal(lg2, lg), what
            assert v2.judged == v.judged and v2.count("ok") + v2.count("undecided") == v2.judged
            assert {1, 3, 4} <= {b for _, b in v2.decisive["pad_after_eos"]}, what
        again = eng.generate_greedy(built.prompt, **kw)["sequences"]
        assert np.array_equal(again, plain)
    finally:
        eng.close()
