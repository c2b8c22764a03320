"""The sampler judge (tests/sampler_judge.py) on the CPU: it accepts the numpy oracle's own run of every crafted case of its table - with no
undecided step, every rule decisive somewhere and every planted tie at a maximum, which proves that the conditions a GPU replay of these
cases has to meet can be met by the reference alone - and it rejects mutated runs at the mutated step."""
import functools

import numpy as np
import pytest

from tests import sampler_judge as sj


@functools.lru_cache(maxsize=None)
def oracle_verdict(name):
    built = sj.build_case(sj.case_by_name(name))
    seqs, lg = sj.oracle_run(built.dims, built.weights, built.prompt, built.opt)
    return built, seqs, lg, sj.judge(lg, seqs, built.prompt.shape[1], built.opt)


@pytest.mark.parametrize("name", [c.name for c in sj.CASES])
def test_the_judge_accepts_the_oracles_own_run(name):
    built, seqs, lg, v = oracle_verdict(name)
    c = built.case
    print(f"{name}: {v.summary()}")
    assert v.judged == c.B * (seqs.shape[1] - 3) and v.judged >= 40
    assert v.count("wrong") == 0, v.wrong[:3]
    assert v.count("undecided") == 0
    got = {r for r, at in v.decisive.items() if at}
    assert set(c.expect) <= got, sorted(set(c.expect) - got)
    seen = sj.tie_kinds_seen(built, v)
    assert set(c.expect_ties) <= seen, sorted(set(c.expect_ties) - seen)
    for pairs in built.planted.values():                      # duplicated rows are exact ties at every step
        for lo, hi in pairs:
            assert np.array_equal(lg[..., lo], lg[..., hi])
    # the float64 restatement of a zero-layer step (the yardstick for an engine's replayed logits) is the oracle's step
    ref = np.stack([sj.logits_f64(built.weights, seqs[:, s], s) for s in range(0, seqs.shape[1] - 1, 7)])
    assert np.abs(ref - lg[::7]).max() < 1e-4


def test_every_rule_and_every_kind_of_tie_is_decisive_in_some_case():
    rules, ties = set(), set()
    for c in sj.CASES:
        built, _, _, v = oracle_verdict(c.name)
        assert set(c.expect) <= {r for r, at in v.decisive.items() if at}
        rules |= set(c.expect)
        ties |= set(c.expect_ties)
    assert rules == set(sj.RULES), sorted(set(sj.RULES) - rules)
    # lanes, wavefronts, passes of a thread, slices; text and timestamp ids; text against timestamp; the lower id masked
    assert {"text_pair", "text_lane", "text_wave", "text_wave2", "text_slice", "text_far", "ts_pair", "ts_lane", "ts_slice", "text_ts",
            "masked_lower"} <= ties


def test_layouts_reach_the_slice_geometry_the_cases_are_named_for():
    assert sj.sampler_chunk(1000) == 32 and (sj.V1000B[2] + 1) % 32 == 0          # ts_begin on a slice boundary
    assert (sj.V1000A[2] + 1) % 2 == 1 and (sj.V1000A[2] + 1) % 32 != 0           # ts_begin odd, inside a bitmap word
    assert sj.sampler_chunk(66) * 31 > 66                                        # most slices empty
    assert sj.REAL[0] % 2 == 1 and sj.REAL[0] % 16 == 9


def test_forced_prefixes_are_judged_from_the_begin_index():
    built, seqs, lg, v = oracle_verdict("v1000-ts-odd")
    n_forced = sj.forced_after_open_timestamp(seqs, 3, built.case.no_ts)
    forced = seqs[:, : 3 + n_forced]
    seqs2, lg2 = sj.oracle_run(built.dims, built.weights, forced, built.opt, begin_index=3)
    assert np.array_equal(seqs2, seqs)
    v2 = sj.judge(lg2, seqs2, 3, built.opt)
    assert v2.judged == v.judged and v2.count("ok") == v2.judged
    # judged as if the forced tokens were prompt, the grammar sees no open pair: the step behind the prefix is wrong
    v3 = sj.judge(lg2, seqs2, 3 + n_forced, built.opt)
    assert v3.status[3 + n_forced - 1, 0] == "wrong"


def _cut(seqs, lg, s):
    """The run up to and including the token that step s produced."""
    return seqs[:, : s + 2].copy(), lg[: s + 1]


def _only_wrong_at(v, s, b):
    assert [(w["step"], w["stream"]) for w in v.wrong] == [(s, b)], v.wrong
    assert v.status[s, b] == "wrong" and v.count("wrong") == 1


def test_the_judge_rejects_a_tie_resolved_to_the_higher_index():
    built, seqs, lg, v = oracle_verdict("v1000-ts-odd")
    for kind in ("text_slice", "ts_pair"):
        pairs = set(built.planted[kind])
        s, b, ids = next(t for t in v.ties if (t[2][0], t[2][1]) in pairs)
        m, l = _cut(seqs, lg, s)
        assert m[b, s + 1] == ids[0]
        m[b, s + 1] = ids[1]
        _only_wrong_at(sj.judge(l, m, 3, built.opt), s, b)


def test_the_judge_rejects_a_token_from_a_masked_range():
    built, seqs, lg, v = oracle_verdict("v1000-ts-odd")
    tb = built.case.no_ts + 1
    s, b = v.decisive["pair_ts_ts"][0]                 # two timestamps behind: every timestamp is masked
    m, l = _cut(seqs, lg, s)
    m[b, s + 1] = tb + int(np.argmax(l[s, b, tb:]))
    _only_wrong_at(sj.judge(l, m, 3, built.opt), s, b)
    s, b = v.masked_ties[0][:2]                        # the suppressed lower copy of a duplicated row
    m, l = _cut(seqs, lg, s)
    m[b, s + 1] = v.masked_ties[0][2]
    _only_wrong_at(sj.judge(l, m, 3, built.opt), s, b)


def test_the_judge_rejects_a_text_token_where_the_mass_rule_forces_a_timestamp():
    built, seqs, lg, v = oracle_verdict("v1000-ts-odd")
    tb = built.case.no_ts + 1
    s, b = v.decisive["mass"][0]
    m, l = _cut(seqs, lg, s)
    assert m[b, s + 1] >= tb
    text = sj.wo.apply_logits_processors(np.where(np.arange(built.case.V) >= tb, -1e30, l[s, b]).astype(np.float32), list(m[b, : s + 1]), 3, built.opt)
    m[b, s + 1] = int(np.argmax(text))                 # the best text token the grammar allows: what a sampler without the rule appends
    assert m[b, s + 1] < tb
    _only_wrong_at(sj.judge(l, m, 3, built.opt), s, b)


def test_the_judge_rejects_a_token_behind_eos():
    built, seqs, lg, v = oracle_verdict("v1000-b33")
    s, b = v.decisive["pad_after_eos"][0]
    m, l = _cut(seqs, lg, s)
    m[b, s + 1] = 5
    _only_wrong_at(sj.judge(l, m, 3, built.opt), s, b)


def test_a_step_inside_the_band_is_undecided_and_accepts_both_outcomes():
    built, seqs, lg, v = oracle_verdict("v1000-ts-odd")
    tb = built.case.no_ts + 1
    s, b = v.decisive["mass"][0]
    m, l = _cut(seqs, lg, s)
    l = l.copy()
    pre = np.isneginf(sj.wo.apply_logits_processors(np.where(np.arange(built.case.V) >= tb, -1e30, 0).astype(np.float32), list(m[b, : s + 1]), 3, built.opt))
    d = sj._mass_margin(l[s, b], np.concatenate([pre[:tb], np.zeros(built.case.V - tb, bool)]) | _ts_mask(built, m, s, b), tb)
    best_text = int(np.argmax(np.where(pre[:tb], -np.inf, l[s, b, :tb])))
    l[s, b, best_text] += np.float32(d)                # lift the best text token to the timestamp mass: d becomes ~0
    for tok in (m[b, s + 1], best_text):
        m[b, s + 1] = tok
        v2 = sj.judge(l, m, 3, built.opt)
        assert v2.status[s, b] == "undecided" and v2.count("wrong") == 0


def _ts_mask(built, m, s, b):
    tb = built.case.no_ts + 1
    probe = np.zeros(built.case.V, np.float32)
    probe[:tb] = -1e30
    x = np.isneginf(sj.wo.apply_logits_processors(probe, list(m[b, : s + 1]), 3, built.opt))
    x[:tb] = False
    return x
