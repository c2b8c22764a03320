"""Ragged decoder prompts on the MI355X (tw_generate_greedy_ragged; the rule is in include/thewhisper.h): a left-padded row is that row
decoded alone.  Everything here compares the engine with itself bit for bit - generated ids, recorded alignment rows, token timestamps -
or, through the drop-in in strict f32, with the ids of the HF model: there is no tolerance.  `micro` preset, 1 s chunks (T = 50).
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_ragged.py``."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests.util import clips, make_engine

pytestmark = pytest.mark.gpu
T = 50
PAD = 50257
INIT = [50258, 50259, 50360]
HEADS = [(1, 0), (1, 1)]
DIMS = wo.PRESETS["micro"]
REFUSED = r"tw_generate_greedy_ragged failed \(-1\)"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture(scope="module")
def weights():
    return wo.make_weights(DIMS, 0)


@pytest.fixture(scope="module")
def pcm():
    return clips(T * 320, 17)


def padded_batch(n_pad, n_prompt, seed=1):
    """Row b: n_pad[b] pad tokens, then `previous text` (<|startofprev|> + random text ids), then the init tokens."""
    rng = np.random.default_rng(seed)
    out = np.full((len(n_pad), n_prompt), PAD, dtype=np.int32)
    for b, k in enumerate(n_pad):
        real = n_prompt - int(k)
        if real >= len(INIT) + 1:
            out[b, k:] = [50361] + rng.integers(0, 50000, size=real - len(INIT) - 1).tolist() + INIT
        else:
            out[b, k:] = INIT[len(INIT) - real:]
    return out


def fill(eng, mel, rows):
    """Slots 0 .. len(rows)-1 <- clips `rows` of `mel`."""
    eng.encode(mel[list(rows)])
    eng.cross_kv(len(rows))


def results(eng, B, n_prompt, out):
    """(ids, alignment rows [B, Ha, L - 1, T], token timestamps [B, L]) of the call that has just returned `out`."""
    L = out["length"]
    return out["sequences"], eng.get_alignment(B, L - 1), eng.token_timestamps(B, n_prompt, L)


def assert_row_is_the_row_alone(eng, mel, clip, row, k, n_prompt, got, b, kw, what):
    """Row b of `got` (a padded call's results) against `row[k:]` decoded alone on clip `clip` with max_length - k."""
    fill(eng, mel, [clip])
    real = n_prompt - k
    out = eng.generate_greedy(row[None, k:], **{**kw, "max_length": kw.get("max_length", 448) - k})
    ids, al, ts = results(eng, 1, real, out)
    L = got[0].shape[1]
    assert out["length"] == L - k, (what, out["length"], L, k)
    assert np.array_equal(got[0][b, :k], row[:k]), (what, "the padding is returned as given")
    assert np.array_equal(got[0][b, k:], ids[0]), (what, "ids", got[0][b, n_prompt:], ids[0, real:])
    assert np.array_equal(got[1][b, :, n_prompt:], al[0, :, real:]), (what, "alignment rows")
    assert np.isfinite(got[1][b, :, n_prompt:]).all() and got[1][b, :, n_prompt:].max() > 0
    assert np.array_equal(got[2][b, n_prompt:], ts[0, real:]), (what, "token timestamps", got[2][b, n_prompt:], ts[0, real:])


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16", "fp8a16", "fp8a8"])
def test_a_padded_row_is_the_row_alone_bit_for_bit(dtype, weights, pcm):
    """The heavily padded rows' real prompts are under 64 tokens: alone they stay in the first 64-key bucket of the self attention
    while the padded call crosses into the second at absolute position 64 and past 128 before it ends (76 + 60 = 136)."""
    n_pad, n_prompt = [0, 3, 40, 70, 1], 76
    B = len(n_pad)
    prompt = padded_batch(n_pad, n_prompt)
    kw = dict(max_new_tokens=60, min_new_tokens=60, timestamps=True, want_alignment=True)
    eng = make_engine(DIMS, weights, T=T, max_batch=B, dtype=dtype, heads=HEADS, use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:B]).cuda())
        fill(eng, mel, range(B))
        got = results(eng, B, n_prompt, eng.generate_greedy(prompt, n_pad=n_pad, **kw))
        assert got[0].shape == (B, n_prompt + 60)
        assert len({tuple(r[n_prompt:].tolist()) for r in got[0]}) > 1, "the rows decode to different ids"
        for b in range(B):
            assert_row_is_the_row_alone(eng, mel, b, prompt[b], n_pad[b], n_prompt, got, b, kw, f"{dtype} row {b} (n_pad {n_pad[b]})")
        # the same through the list form: sequences without their padding
        fill(eng, mel, range(B))
        rag = eng.generate_greedy_ragged([prompt[b, n_pad[b]:] for b in range(B)], **kw)
        assert rag["n_pad"].tolist() == n_pad and rag["length"] == n_prompt + 60
        assert all(np.array_equal(rag["sequences"][b], got[0][b, n_pad[b]:]) for b in range(B))
    finally:
        eng.close()


def test_a_padded_row_in_the_second_group_of_sixteen(weights, pcm):
    B, n_prompt = 17, 8
    n_pad = [0] * 16 + [5]
    prompt = padded_batch(n_pad, n_prompt, seed=2)
    kw = dict(max_new_tokens=10, min_new_tokens=10, timestamps=True, want_alignment=True)
    eng = make_engine(DIMS, weights, T=T, max_batch=B, dtype="bf16", heads=HEADS, use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:B]).cuda())
        fill(eng, mel, range(B))
        got = results(eng, B, n_prompt, eng.generate_greedy(prompt, n_pad=n_pad, **kw))
        plain = results(eng, B, n_prompt, eng.generate_greedy(prompt, **kw))      # (the pads of row 16 taken for tokens)
        for a, b in zip(got, plain):
            assert np.array_equal(a[:16], b[:16]), "the unpadded rows are their rows of the plain call"
        assert not np.array_equal(got[0][16], plain[0][16])
        assert_row_is_the_row_alone(eng, mel, 16, prompt[16], 5, n_prompt, got, 16, kw, "row 16 of 17")
    finally:
        eng.close()


@pytest.mark.parametrize("graph", [False, True])
def test_nothing_padded_is_the_plain_call_and_the_plain_call_is_undisturbed(graph, weights, pcm):
    B, n_prompt = 3, 6
    prompt = padded_batch([0, 0, 0], n_prompt, seed=3)
    kw = dict(max_new_tokens=12, min_new_tokens=12, timestamps=True, want_alignment=True)
    eng = make_engine(DIMS, weights, T=T, max_batch=B, dtype="bf16", heads=HEADS, use_graph=graph)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:B]).cuda())
        fill(eng, mel, range(B))
        plain = results(eng, B, n_prompt, eng.generate_greedy(prompt, **kw))
        for n_pad in ([0, 0, 0], np.zeros(3, dtype=np.int64)):
            same = results(eng, B, n_prompt, eng.generate_greedy(prompt, n_pad=n_pad, **kw))
            assert all(np.array_equal(a, b) for a, b in zip(plain, same))
        rc_out = np.zeros((B, 448), dtype=np.int32)           # n_pad_host == NULL, through the C ABI itself
        o, _keep = eng._greedy_opts(50257, 50257, True, 50364, 50, (220, 50257), (), 12, 12, 448, True)
        n = C.c_int32(0)
        ip = C.POINTER(C.c_int32)
        rc = eng.lib.tw_generate_greedy_ragged(eng.ctx, B, prompt.ctypes.data_as(ip), n_prompt, C.byref(o), None, rc_out.ctypes.data_as(ip),
                                               C.byref(n), eng._sp())
        assert rc == 0 and n.value == plain[0].shape[1] and np.array_equal(rc_out[:, : n.value], plain[0])
        assert np.array_equal(eng.get_alignment(B, n.value - 1), plain[1])
        # a padded call in between (its step graphs are keyed apart), then the plain call again: the same ids and rows
        padded = prompt.copy()
        padded[0, :2], padded[2, :4] = PAD, PAD
        mid = eng.generate_greedy(padded, n_pad=[2, 0, 4], **kw)["sequences"]
        assert np.array_equal(mid[1], plain[0][1]) and not np.array_equal(mid[0], plain[0][0])
        again = results(eng, B, n_prompt, eng.generate_greedy(prompt, **kw))
        assert all(np.array_equal(a, b) for a, b in zip(plain, again))
    finally:
        eng.close()


def test_a_row_does_not_depend_on_its_batch_mates_or_their_padding(weights, pcm):
    n_prompt = 20
    kw = dict(max_new_tokens=30, min_new_tokens=30, timestamps=True, want_alignment=True)
    eng = make_engine(DIMS, weights, T=T, max_batch=6, dtype="f16", heads=HEADS, use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:6]).cuda())
        row = padded_batch([3], n_prompt, seed=4)[0]
        seen = []
        for slot, mates, pads, seed in ((1, [0, 2], [0, 3, 12], 5), (3, [3, 4, 5], [7, 1, 0, 3], 6), (0, [], [3], 7)):
            clip_rows = mates[:slot] + [1] + mates[slot:]
            prompt = padded_batch(pads, n_prompt, seed=seed)
            prompt[slot] = row
            fill(eng, mel, clip_rows)
            got = results(eng, len(pads), n_prompt, eng.generate_greedy(prompt, n_pad=pads, **kw))
            seen.append([g[slot] for g in got])
        for other in seen[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(seen[0], other))
    finally:
        eng.close()


def test_graph_replay_equals_plain_launches_and_a_sibling_owns_its_table(weights, pcm):
    n_prompt, B = 70, 3
    kw = dict(max_new_tokens=24, min_new_tokens=24, timestamps=True, want_alignment=True)
    got = {}
    for graph in (False, True):
        eng = make_engine(DIMS, weights, T=T, max_batch=B, dtype="bf16", heads=HEADS, use_graph=graph)
        try:
            mel = eng.logmel(torch.from_numpy(pcm[:B]).cuda())
            fill(eng, mel, range(B))
            runs = []
            for pads in ([0, 30, 66], [9, 0, 1]):           # the second call replays the first one's graphs with another table
                prompt = padded_batch(pads, n_prompt, seed=8)
                runs.append(results(eng, B, n_prompt, eng.generate_greedy(prompt, n_pad=pads, **kw)))
            if graph:                                        # a sibling context: its own table, its own graphs, the owner's weights
                sib = eng.sibling()
                fill(sib, mel, range(B))
                pads = [0, 30, 66]
                runs.append(results(sib, B, n_prompt, sib.generate_greedy(padded_batch(pads, n_prompt, seed=8), n_pad=pads, **kw)))
                again = results(eng, B, n_prompt, eng.generate_greedy(padded_batch([9, 0, 1], n_prompt, seed=8), n_pad=[9, 0, 1], **kw))
                assert all(np.array_equal(a, b) for a, b in zip(runs[1], again)), "the owner's table is its own"
            got[graph] = runs
        finally:
            eng.close()
    for a, b in zip(got[False], got[True][:2]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), "use_graph = 1 equals use_graph = 0"
    assert all(np.array_equal(x, y) for x, y in zip(got[True][0], got[True][2])), "the sibling's result is the owner's"


def test_refusals_leave_the_context_usable(weights, pcm):
    """Every TW_EINVAL of tw_generate_greedy_ragged is raised before any work is enqueued: nothing is launched by a refused call."""
    B, n_prompt = 2, 6
    kw = dict(max_new_tokens=8, min_new_tokens=8, timestamps=True)
    eng = make_engine(DIMS, weights, T=T, max_batch=B, dtype="bf16", heads=HEADS, use_graph=False)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:B]).cuda())
        fill(eng, mel, range(B))
        prompt = padded_batch([2, 0], n_prompt, seed=9)
        good = eng.generate_greedy(prompt, n_pad=[2, 0], **kw)["sequences"]
        for bad in ([-1, 0], [0, -3], [n_prompt, 0], [0, n_prompt + 5]):
            with pytest.raises(RuntimeError, match=REFUSED):
                eng.generate_greedy(prompt, n_pad=bad, **kw)
        ip = C.POINTER(C.c_int32)
        out, n = np.zeros((65, 448), dtype=np.int32), C.c_int32(0)
        pads = np.array([2, 0], dtype=np.int32)

        def raw(B_, prompt_, pads_, **over):
            o, _keep = eng._greedy_opts(50257, 50257, True, 50364, 50, (220, 50257), (), 8, 8, 448, False, **over)
            return eng.lib.tw_generate_greedy_ragged(eng.ctx, B_, prompt_.ctypes.data_as(ip), prompt_.shape[1], C.byref(o),
                                                     pads_.ctypes.data_as(ip), out.ctypes.data_as(ip), C.byref(n), eng._sp())

        for over in (dict(n_forced=1), dict(n_draft=1)):
            assert raw(B, prompt, pads, **over) == -1
            with pytest.raises(RuntimeError, match=REFUSED):
                eng._chk(-1, "tw_generate_greedy_ragged")
            assert b"n_forced" in eng.lib.tw_last_error(eng.ctx)
        big = np.full((65, n_prompt), 50258, dtype=np.int32)
        assert raw(65, big, np.zeros(65, dtype=np.int32)) == -1 and b"65 streams" in eng.lib.tw_last_error(eng.ctx)
        # the entry points that take no padding have no such keyword
        with pytest.raises(TypeError):
            eng.generate_sample(prompt, 0.5, 1, n_pad=[2, 0], **kw)
        assert np.array_equal(eng.generate_greedy(prompt, n_pad=[2, 0], **kw)["sequences"], good), "the context decodes as before"
    finally:
        eng.close()


def test_the_dropin_returns_hfs_batch_1_rows_in_strict_f32():
    from tests.test_ragged_cpu import check_dropin_against_hf_batch_1

    check_dropin_against_hf_batch_1("cuda", None)
