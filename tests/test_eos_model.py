"""The premises of the GPU tests that run drafts and padding past a row's <eos> (tests/eos_model.py), shown on the numpy oracle: which
clip of the recipe model ends after how many tokens.  If `make_weights`, `synth_audio` or the crafted sampler tables move, this fails
here, on the CPU, instead of the GPU tests going vacuous (they assert the same premises on the engine's own plain call as well)."""
import numpy as np
import pytest

from oracle import whisper_oracle as wo
from tests import eos_model as em
from tests import sampler_judge as sj


@pytest.fixture(scope="module")
def table():
    """(ES, timestamps) -> (sequences [20, L], <eos> steps) of ONE oracle run over all clips, shared by the tests below."""
    out = {}
    for es, ts in em.SETTINGS:
        seq = em.oracle_run(es, ts, range(em.N_CLIPS))
        out[(es, ts)] = (seq, em.eos_steps(seq[:, em.N_PROMPT:]))
    return out


def test_the_table_of_eos_steps_is_the_oracles(table):
    for key, (_, steps) in table.items():
        print(f"ES {key[0]} timestamps {key[1]}: " + " ".join("-" if s is None else str(s) for s in steps))
        assert tuple(steps) == em.TABLE[key], key


def test_a_rows_eos_step_does_not_depend_on_its_batch(table):
    for b in (em.batch("b2-es2.5-ts1"), em.batch("b5-all-end")):
        seq = em.oracle_run(b.es, b.timestamps, b.sel)
        assert em.eos_steps(seq[:, em.N_PROMPT:]) == b.steps(), b.name
        full = table[(b.es, b.timestamps)][0][list(b.sel), : seq.shape[1]]
        assert np.array_equal(seq, full), b.name


@pytest.mark.parametrize("name", [b.name for b in em.BATCHES])
def test_every_batch_the_gpu_tests_use_has_the_rows_it_relies_on(name):
    b = em.batch(name)
    em.check_batch(b, b.steps())


def test_finished_rows_are_padded_and_their_drafts_hold_no_eos(table):
    seq, steps = table[(2.5, True)]
    gen = seq[:, em.N_PROMPT:]
    for r, s in zip(gen, steps):
        if s is not None:
            assert (r[s:] == em.EOS).all() and not (r[:s] == em.EOS).any()
    n = em.draft_span(gen, em.MAX_NEW)
    assert n == em.MAX_NEW - 2
    for repeat in (False, True):
        d = em.filled_draft(gen, n, np.random.default_rng(0), repeat_last=repeat)
        assert d.shape == (em.N_CLIPS, n) and not (d == em.EOS).any()
        for b, s in enumerate(steps):
            k = n if s is None else s
            assert np.array_equal(d[b, :k], gen[b, :k])
    sel = list(em.batch("b5-all-end").sel)
    assert em.draft_span(gen[sel], em.MAX_NEW) == 17          # the longest row's <eos> step
    c = em.corrupt(d, 2, 5)
    assert (c != d).sum() == 1 and c[2, 5] != d[2, 5]


def test_sampler_case_v127_b6_has_rows_that_end_and_rows_that_do_not():
    """The zero-layer judged case of tests/test_gpu_sampler.py: rows 1, 3 and 4 end after 9 tokens, rows 0, 2 and 5 never."""
    built = sj.build_case(sj.case_by_name("v127-b6"))
    seqs, _ = sj.oracle_run(built.dims, built.weights, built.prompt, built.opt)
    steps = [int(np.nonzero(r == built.case.eos)[0][0]) if (r == built.case.eos).any() else None for r in seqs[:, 3:]]
    assert steps == [None, 9, None, 9, 9, None], steps


@pytest.mark.parametrize("dtype", sorted(em.FUZZ_EOS_SEED))
def test_the_fuzz_has_rows_ending_inside_its_drafts(dtype):
    """tests/test_gpu_draft.py's fuzz asserts that at least 10 of its 40 situations on this model have a row ending inside the drafted
    span; by the oracle's table (strict float32 figures; the other types' runs differ in a few rows) each seed gives many more."""
    n_past = 0
    for sit in em.fuzz_eos_situations(dtype):
        steps = [s if s is not None and s < sit["max_new"] else None for s in (em.TABLE[(sit["es"], sit["timestamps"])][i] for i in sit["sel"])]
        nd, past = em.fuzz_eos_draft_length(steps, sit["max_new"], sit["u"])
        assert 1 <= nd <= sit["max_new"] - 2
        n_past += int(past)
    print(f"{dtype}: {n_past} of 40 situations have a row ending inside the drafted span")
    assert n_past >= 20, n_past          # twice what the GPU test asks: the 16-bit and fp8 runs move a few rows


def test_the_biased_two_row_case_still_has_a_row_that_ends():
    """tests/test_gpu_draft.py's biased case: the list of `em.bias_rows` changes row 0's path, the row still ends (not before 3 tokens),
    and decoded on behind its <eos> it would NOT get <eos> again - so a call that does that returns other ids than the plain call."""
    import dataclasses

    from tests import bias_judge as bj
    for es, ts in em.SETTINGS:
        b = em.batch(f"b2-es{es}-ts{int(ts)}")
        plain = em.oracle_run(es, ts, b.sel)
        rows = em.bias_rows(plain[:, em.N_PROMPT:], es, ts)
        _, end, behind = em.BIAS_CASE[(es, ts)]
        dims, w = em.model(es)
        om = wo.OracleWhisper(dims, w, T=em.T)
        enc = om.encode(wo.log_mel(em.audio(b.sel), dims.n_mels))
        out = bj.biased_greedy(om, enc, em.prompt(b.sel), em.options(ts), rows)["sequences"]
        assert em.eos_steps(out[:, em.N_PROMPT:]) == [end, None] and end >= 3, (es, ts)
        assert not np.array_equal(out[0, :9], plain[0, :9]) and np.array_equal(out[1], plain[1][: out.shape[1]])
        # the generation continued from row 0's <eos> as if it were an ordinary token
        on = bj.biased_greedy(om, enc, out[:, : em.N_PROMPT + end + 1], dataclasses.replace(em.options(ts), max_new_tokens=end + 2), rows,
                              begin_index=em.N_PROMPT)["sequences"]
        assert int(on[0, em.N_PROMPT + end + 1]) == behind != em.EOS, (es, ts, on[0, em.N_PROMPT + end + 1])
