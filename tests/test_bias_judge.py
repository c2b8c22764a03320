"""The sequence-bias reference (tests/bias_judge.py) on the CPU: the numpy oracle's own biased run of every case - the rule of
include/thewhisper.h restated in numpy - is judged through HF's SequenceBiasLogitsProcessor with no step wrong, at most 1 % undecided
and every event the GPU test demands decisive, which proves that the conditions tests/test_gpu_bias.py asserts can be met by the
reference alone.  Also: the packing of the per-row lists, the list-to-dict rule, and the hotword helper on the synthetic tokenizer."""
import functools

import numpy as np
import pytest

from tests import bias_judge as bj

N_PROMPT = 3


@functools.lru_cache(maxsize=None)
def oracle_case(case_id):
    bc = next(c for c in bj.BIAS_CASES if c.id == case_id)
    built = bj.build(bc)

    def run(rows):
        return bj.oracle_biased_run(built.dims, built.weights, built.prompt, built.opt, rows)

    rows, events, seqs, lg = bj.build_lists(run, built, N_PROMPT, bc.expect)
    plain, _ = run([None] * bc.B)
    return bc, built, rows, events, seqs, lg, plain


@pytest.mark.parametrize("case_id", [c.id for c in bj.BIAS_CASES if not c.graph])
def test_the_oracles_biased_run_is_judged_ok_through_hf_and_every_event_is_decisive(case_id):
    bc, built, rows, events, seqs, lg, plain = oracle_case(case_id)
    v = bj.judge_biased(lg, seqs, N_PROMPT, built.opt, rows)
    seen = bj.events_seen(events, rows, seqs, lg, N_PROMPT, built.opt)
    print(f"{case_id}: {v.summary()} | events {sorted(seen)} | sequences per row {[len(r) if r else 0 for r in rows]}")
    assert v.count("wrong") == 0, v.wrong[:3]
    assert v.count("undecided") * 100 <= v.judged, (v.count("undecided"), v.judged)
    assert v.judged == bc.B * (seqs.shape[1] - N_PROMPT)
    assert set(bc.expect) <= seen, sorted(set(bc.expect) - seen)
    listed = bj.listed_rows(bc.B)
    assert all(rows[b] for b in listed)
    assert len({tuple(sorted(rows[b].items())) for b in listed}) == len(listed)              # lists differ per row
    assert all(min(t for k in rows[b] for t in k) >= 1 for b in listed)       # HF's list form refuses id 0
    for b in range(bc.B):
        if b not in listed:                                    # the row without a list: its row of the plain run
            L = min(seqs.shape[1], plain.shape[1])
            assert rows[b] is None and np.array_equal(seqs[b, :L], plain[b, :L])
        else:
            assert seqs[b].tolist() != plain[b].tolist()


def test_the_numpy_rule_is_hfs_processor_bit_for_bit():
    rng = np.random.default_rng(0)
    V = 97
    lst = {(5,): 1.25, (7, 5): 0.1, (3, 7, 5): 0.7, (9,): -2.0, (1, 2, 3, 4, 11): 3.0, (7, 11): 0.3, (3, 7, 12): 1e-3, (8, 3, 7, 5): 1e8}
    hf = bj.HFBias(lst)
    for hist in ([3, 7], [7], [1, 2, 3, 4], [8, 3, 7], [2, 3, 4], [0, 8, 3, 7]):
        x = (rng.standard_normal(V) * 20).astype(np.float32)
        assert np.array_equal(bj.add_bias(x, hist, lst).view(np.uint32), hf(x, hist).view(np.uint32)), hist


def test_sum_order_triple_distinguishes_the_two_associations():
    b1, b2, b3 = (np.float32(b) for b in bj.sum_order_betas())
    assert np.float32(np.float32(b1 + b2) + b3) > np.float32(b1 + np.float32(b2 + b3))
    bc, built, *_ , plain = oracle_case(bj.BIAS_CASES[0].id)
    lo, hi, lst = bj.sum_order_lists(built, plain, N_PROMPT)
    rows = [lst] + [None] * (bc.B - 1)
    seqs, lg = bj.oracle_biased_run(built.dims, built.weights, built.prompt, built.opt, rows)
    x1 = bj.HFBias(lst)(lg[N_PROMPT - 1, 0], seqs[0, :N_PROMPT])
    assert lg[N_PROMPT - 1, 0, lo] == lg[N_PROMPT - 1, 0, hi] and x1[lo] == x1[hi] and lo < hi
    assert int(seqs[0, N_PROMPT]) == lo
    assert bj.judge_biased(lg, seqs, N_PROMPT, built.opt, rows).count("wrong") == 0


def test_pack_sequence_bias_groups_by_row_and_keeps_the_dict_order():
    from thewhisper_amd.engine import merge_sequence_bias, pack_sequence_bias, sequence_bias_dict

    # list form -> dict as HF's _convert_list_arguments_into_dict: a later duplicate wins and keeps the first one's place
    d = sequence_bias_dict([[[4, 5], 1.0], [[6], 2.0], [[4, 5], 3.0]])
    assert list(d.items()) == [((4, 5), 3.0), ((6,), 2.0)]
    from transformers.generation.logits_process import SequenceBiasLogitsProcessor
    assert SequenceBiasLogitsProcessor([[[4, 5], 1.0], [[6], 2.0], [[4, 5], 3.0]]).sequence_bias == d
    assert sequence_bias_dict(None) == {} and sequence_bias_dict({(1, 2): 0.5}) == {(1, 2): 0.5}
    p = pack_sequence_bias([[[[4, 5], 1.0], [[6], 2.0]], None, {(7, 8, 9): -1.5}, []], 4)
    assert p["row_off"].tolist() == [0, 2, 2, 3, 3] and p["seq_off"].tolist() == [0, 2, 3, 6]
    assert p["tokens"].tolist() == [4, 5, 6, 7, 8, 9] and p["bias"].tolist() == [1.0, 2.0, -1.5]
    assert p["row_off"].dtype == p["seq_off"].dtype == p["tokens"].dtype == np.int32 and p["bias"].dtype == np.float32
    assert pack_sequence_bias([None, []], 2) is None
    assert list(merge_sequence_bias([[[1], 1.0], [[2, 3], 2.0]], {(2, 3): 5.0, (4,): 6.0}).items()) == [((1,), 1.0), ((2, 3), 5.0), ((4,), 6.0)]
    with pytest.raises(ValueError):
        pack_sequence_bias([None], 2)
    with pytest.raises(ValueError):
        sequence_bias_dict([[[1], float("nan")]])
    with pytest.raises(ValueError):
        sequence_bias_dict([[[], 1.0]])


def test_hotwords_on_the_synthetic_tokenizer():
    from thewhisper_amd import synthetic
    from thewhisper_amd.hotwords import sequence_bias_for

    tok = synthetic.build_tokenizer(51866)
    d = sequence_bias_for(tok, ["w5 w17", "w5"], 2.5)
    for phrase in ("w5 w17", "w5"):
        for variant in (" {}", "{}"):
            ids = tok.encode(variant.format(phrase), add_special_tokens=False)
            assert len(ids) >= 1
            for n in range(1, len(ids) + 1):
                assert d[tuple(ids[:n])] == 2.5
    keys = list(d)
    assert len(keys) == len(set(keys)) and all(len(k) >= 1 for k in keys)
    n_expected = len({tuple(tok.encode(v.format(p), add_special_tokens=False)[:n]) for p in ("w5 w17", "w5") for v in (" {}", "{}")
                      for n in range(1, len(tok.encode(v.format(p), add_special_tokens=False)) + 1)})
    assert len(keys) == n_expected
    assert sequence_bias_for(tok, ["w5"], -1.0, variants=("{}",)) == {tuple(tok.encode("w5", add_special_tokens=False)[:n]): -1.0
                                                                       for n in range(1, len(tok.encode("w5", add_special_tokens=False)) + 1)}
    with pytest.raises(ValueError):
        sequence_bias_for(tok, ["w5"], float("inf"))
    with pytest.raises(ValueError):
        sequence_bias_for(tok, [" "], 1.0)
