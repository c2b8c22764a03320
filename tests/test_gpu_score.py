"""tw_score_tokens (k_decode.hip: score_part_kernel, score_finish_kernel; api.hip) on the MI355X, judged on the engine's OWN logits.

A finished `generate_greedy` result is replayed through `decoder_reset` + `decode_step`; from those logits z[b, p] the host computes in
float64 the log-softmax of the next token, raw and after `oracle.whisper_oracle.apply_logits_processors`, and `score_tokens` must give
the same numbers.  Tolerance 1e-4 absolute on finite entries, -inf exactly: the only arithmetic under test is a float32 log-sum-exp over
at most 51866 terms merged in a fixed number of parts, which for logits below 60 in magnitude (asserted first) is off by a few 1e-5 at
worst - the argument behind `sampler_judge.MASS_BAND`.  A larger difference would mean that the rows-mode logits are not the step's.
The one decision inside the masked number that depends on summation order is the timestamp-mass rule: where
|logsumexp(timestamps) - max(text)| <= MASS_BAND the judge calls the step undecided, and so does this file (either outcome's number).
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_score.py -s`` prints each case's figures.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import sampler_judge as sj
from tests.util import PROMPT, clips, dims_variant, make_engine

pytestmark = pytest.mark.gpu
TOL = 1e-4
Z_MAX = 60.0
TW_EINVAL, TW_ESTATE = -1, -3


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


# ---- host side ----------------------------------------------------------------------------------------------------------------
def replay(eng, seqs):
    """[L-1, B, V] float32: the logits of positions 0 .. L-2 of `seqs`, by teacher-forced steps."""
    B, L = seqs.shape
    eng.decoder_reset(B)
    return np.stack([eng.decode_step(seqs[:, s].tolist()).cpu().numpy() for s in range(L - 1)])


def lse64(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return m + np.log(np.exp(x - m).sum()) if np.isfinite(m) else -np.inf


def pre_mask(V, seq, n_begin, opt):
    """What the processors mask ahead of the mass rule, read off apply_logits_processors itself (as sampler_judge.judge does)."""
    tb = opt.no_timestamps_id + 1 if opt.timestamps else V
    probe = np.zeros(V, np.float32)
    probe[tb:] = -1e30
    pre = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))
    probe = np.zeros(V, np.float32)
    probe[:tb] = -1e30
    pre[tb:] = np.isneginf(wo.apply_logits_processors(probe, seq, n_begin, opt))[tb:]
    return pre, tb


def host_scores(z, seqs, n_prompt, opt):
    """(masked, alternative, raw) float64 [B, L]: 0 for the prompt and behind a row's first eos.  `alternative` differs from `masked`
    only at steps whose timestamp-mass decision is within MASS_BAND (nan elsewhere): the number under the other decision."""
    B, L = seqs.shape
    V = z.shape[2]
    masked, raw, alt = np.zeros((B, L)), np.zeros((B, L)), np.full((B, L), np.nan)
    for b in range(B):
        for p in range(n_prompt, L):
            lg, t, seq = z[p - 1, b], int(seqs[b, p]), [int(x) for x in seqs[b, :p]]
            raw[b, p] = float(lg[t]) - lse64(lg)
            nat = wo.apply_logits_processors(lg, seq, n_prompt, opt)
            masked[b, p] = -np.inf if np.isneginf(nat[t]) else float(nat[t]) - lse64(nat)
            if opt.timestamps:
                pre, tb = pre_mask(V, seq, n_prompt, opt)
                d = sj._mass_margin(lg, pre, tb)
                if np.isfinite(d) and abs(d) <= sj.MASS_BAND and int((~pre[tb:]).sum()) != 1:
                    other = np.where(pre, -np.inf, lg.astype(np.float64))
                    if not np.isneginf(nat[:tb]).all():      # the oracle kept the text: the other decision drops it
                        other[:tb] = -np.inf
                    alt[b, p] = -np.inf if np.isneginf(other[t]) else other[t] - lse64(other)
            if t == opt.eos:
                break
    return masked, alt, raw


def compare(what, got, want, alt=None):
    """finite entries within TOL, -inf exactly; returns the largest finite difference.  Prints before it asserts."""
    got = np.asarray(got, np.float64)
    ok = np.zeros(got.shape, bool)
    worst = 0.0
    for w in ([want] if alt is None else [want, alt]):
        inf = np.isneginf(w)
        fin = np.isfinite(w) & np.isfinite(got)
        diff = np.where(fin, np.abs(got - np.where(fin, w, 0.0)), np.inf)
        ok |= (inf & np.isneginf(got)) | (fin & (diff <= TOL))
        if w is want:
            worst = float(diff[fin].max()) if fin.any() else 0.0
    n_inf = int(np.isneginf(want).sum())
    print(f"{what}: max |difference| over finite entries {worst:.2e} (bound {TOL:g}), -inf entries {n_inf}, undecided {0 if alt is None else int((~np.isnan(alt)).sum())}")
    assert not np.isnan(got).any() and not np.isposinf(got).any(), what
    assert ok.all(), (what, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])
    return worst


def options(kw):
    return wo.GreedyOptions(eos=kw.get("eos_id", 50257), pad=kw.get("pad_id", 50257), max_new_tokens=kw.get("max_new_tokens", 128),
                            min_new_tokens=kw.get("min_new_tokens", 0), max_length=448, begin_suppress=tuple(kw.get("begin_suppress", (220, 50257))),
                            suppress=tuple(kw.get("suppress", ())), timestamps=kw.get("timestamps", False),
                            no_timestamps_id=kw.get("no_timestamps_id", 50364), max_initial_timestamp_index=kw.get("max_initial_timestamp_index", 50))


def check_layout(seqs, n_prompt, eos, res):
    """Prompt and padding entries exactly 0.0, every entry of a generated token (the eos included) scored: masked finite and <= 1e-6,
    raw <= 1e-6, masked >= raw - 1e-5 (masking only removes mass)."""
    lp, raw = res["logprob"], res["logprob_raw"]
    assert lp.shape == seqs.shape == raw.shape and lp.dtype == np.float32
    n_eos = 0
    for b in range(seqs.shape[0]):
        stop = np.flatnonzero(seqs[b, n_prompt:] == eos)
        last = n_prompt + int(stop[0]) if stop.size else seqs.shape[1] - 1
        n_eos += int(stop.size > 0)
        for a in (lp, raw):
            assert (a[b, :n_prompt] == 0.0).all() and (a[b, last + 1:] == 0.0).all(), b
        g, r = lp[b, n_prompt:last + 1].astype(np.float64), raw[b, n_prompt:last + 1].astype(np.float64)
        assert np.isfinite(g).all() and (g <= 1e-6).all() and np.isfinite(r).all() and (r <= 1e-6).all(), b
        assert (g >= r - 1e-5).all(), (b, float((r - g).max()))
        if stop.size:
            assert lp[b, last] != 0.0 and raw[b, last] != 0.0, "the eos is scored"
    return n_eos


# ---- (a) the crafted zero-layer models: every grammar rule binds a generated token ------------------------------------------------
NEED = ("pair_ts_ts", "pair_ts_text", "mono_next", "mono_same", "initial", "max_initial", "mass", "no_ts", "min_new", "begin_suppress", "suppress")
CRAFTED = {   # found on the CPU with the judge (numpy oracle's run): every rule of NEED decides steps of all five streams, f32 and bf16 tables
    1000: dict(gain=1.0, eos_scale=4.0, min_new=12, max_initial=5),
    1001: dict(gain=2.0, eos_scale=2.5, min_new=6, max_initial=2),       # odd V: the scalar path of score_part_kernel
}


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("V", [1000, 1001])
def test_crafted_model_every_rule_binds(V, dtype):
    c = sj.Case(f"score-v{V}-{dtype}", V, 700, 720, B=5, max_new=36, seed=0, ts_dir=0.25, pos_scale=2.0, no_ts_scale=3.0, begin_suppress="pick",
                suppress="picks", ties=False, dtype=dtype, **CRAFTED[V])
    built = sj.build_case(c)
    assert built.opt.min_new_tokens > 0 and built.opt.suppress and built.opt.begin_suppress and built.opt.timestamps
    eng = make_engine(built.dims, built.weights, T=sj.T_FRAMES, max_batch=c.B, dtype=dtype)
    try:
        eng.encode(torch.zeros((c.B, built.dims.n_mels, 2 * sj.T_FRAMES), dtype=torch.float32).cuda())
        eng.cross_kv(c.B)
        seqs = eng.generate_greedy(built.prompt, **built.kw)["sequences"]
        z = replay(eng, seqs)
        res = eng.score_tokens(seqs, 3, **built.kw)
    finally:
        eng.close()
    assert np.isfinite(z).all() and np.abs(z).max() < Z_MAX
    v = sj.judge(z, seqs, 3, built.opt)
    print(f"{c.name}: {v.summary()}")
    assert v.count("wrong") == 0
    got = {r for r, at in v.decisive.items() if at}
    assert set(NEED) <= got, ("rules that never decided a step of the engine's run:", sorted(set(NEED) - got))
    masked, alt, raw = host_scores(z, seqs, 3, built.opt)
    compare(f"{c.name} raw", res["logprob_raw"], raw)
    compare(f"{c.name} masked", res["logprob"], masked, alt)
    check_layout(seqs, 3, c.eos, res)
    differ = int((np.abs(res["logprob"].astype(np.float64) - res["logprob_raw"]) > 1e-3).sum())
    print(f"{c.name}: masked differs from raw by more than 1e-3 at {differ} of {int((raw != 0).sum())} entries")
    assert differ >= 1


# ---- (b) large-v3 width, one encoder and two decoder layers --------------------------------------------------------------------
REAL = dict(enc_layers=1, dec_layers=2)
T = 100
KW = dict(max_new_tokens=20, timestamps=True)
NO_SPEECH = 50363


@functools.lru_cache(maxsize=1)
def real_model():
    dims = dims_variant("large-v3", **REAL)
    return dims, wo.make_weights(dims, 2), clips(T * 320, 64)


def fill(eng, mel, B):
    eng.encode(mel[:B])
    eng.cross_kv(B)


@pytest.mark.parametrize("dtype,batches", [("bf16", (1, 3, 17)), ("f16", (1, 3, 17)), ("f32", (1, 3, 17)), ("fp8a16", (1, 3, 17)), ("fp8", (3,))])
def test_real_width_scores_equal_the_float64_numbers_of_the_engines_own_logits(dtype, batches):
    """B = 17: launches of 3 positions with a ragged last launch.  Also the inequalities on the engine's own output and the
    no-speech probability at positions 0 and 1 (1e-6 relative against softmax of the replayed logits)."""
    dims, w, pcm = real_model()
    Bmax = max(batches)
    eng = make_engine(dims, w, T=T, max_batch=Bmax, dtype=dtype)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:Bmax]).cuda())
        opt = options(KW)
        for B in batches:
            fill(eng, mel, B)
            seqs = eng.generate_greedy(np.tile(np.array(PROMPT, np.int32), (B, 1)), **KW)["sequences"]
            z = replay(eng, seqs)
            assert np.isfinite(z).all() and np.abs(z).max() < Z_MAX, float(np.abs(z).max())
            res = eng.score_tokens(seqs, 3, no_speech_id=NO_SPEECH, no_speech_pos=0, **KW)
            again = eng.score_tokens(seqs, 3, no_speech_id=NO_SPEECH, no_speech_pos=1, **KW)
            for k in ("logprob", "logprob_raw"):
                assert np.array_equal(res[k].view(np.uint32), again[k].view(np.uint32)), f"{dtype} B={B}: scoring twice, {k}"
            masked, alt, raw = host_scores(z, seqs, 3, opt)
            what = f"{dtype} B={B} L={seqs.shape[1]} max|z|={np.abs(z).max():.1f}"
            compare(what + " raw", res["logprob_raw"], raw)
            compare(what + " masked", res["logprob"], masked, alt)
            check_layout(seqs, 3, 50257, res)
            for pos, r in ((0, res), (1, again)):
                zz = z[pos].astype(np.float64)
                want = np.exp(zz[:, NO_SPEECH] - np.array([lse64(x) for x in zz]))
                rel = np.abs(r["no_speech_prob"].astype(np.float64) - want) / want
                print(f"{what}: no_speech_prob at position {pos}: max relative difference {rel.max():.2e} (bound 1e-6)")
                assert r["no_speech_prob"].dtype == np.float32 and (rel <= 1e-6).all(), (pos, rel.max())
    finally:
        eng.close()


def score_raw_call(eng, seqs, n_prompt, opts=None, ns_id=-1, ns_pos=0, B=None, ld=None, seq_len=None, want=("lp", "raw", "ns")):
    """tw_score_tokens itself: (return code, logprob, logprob_raw, no_speech) with the output buffers pre-filled with 7."""
    import ctypes as C

    seqs = np.ascontiguousarray(seqs, np.int32)
    B = seqs.shape[0] if B is None else B
    ld = seqs.shape[1] if ld is None else ld
    seq_len = seqs.shape[1] if seq_len is None else seq_len
    lp, raw, ns = (np.full((max(B, 1), max(seq_len, 1)), 7, np.float32), np.full((max(B, 1), max(seq_len, 1)), 7, np.float32),
                   np.full((max(B, 1),), 7, np.float32))
    fp = C.POINTER(C.c_float)
    rc = eng.lib.tw_score_tokens(eng.ctx, B, seqs.ctypes.data_as(C.POINTER(C.c_int32)), ld, seq_len, n_prompt,
                                 None if opts is None else C.byref(opts), ns_id, ns_pos,
                                 lp.ctypes.data_as(fp) if "lp" in want else None, raw.ctypes.data_as(fp) if "raw" in want else None,
                                 ns.ctypes.data_as(fp) if "ns" in want else None, eng._sp())
    return rc, lp, raw, ns


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32", "fp8a16"])
def test_a_rows_numbers_do_not_depend_on_its_companions(dtype, batches=(1, 3, 17, 64)):
    """Stream 0's rows are bit-identical whether scored alone or among 3, 17, 64 streams (launches of 64, 21, 3, 1 positions); slots
    filled as in test_gpu_draft.test_rows_of_a_launch_do_not_matter.  With no options (NULL) the raw numbers are the same bits too."""
    dims, w, pcm = real_model()
    Bmax = max(batches)
    eng = make_engine(dims, w, T=T, max_batch=Bmax, dtype=dtype)
    try:
        mel = eng.logmel(torch.from_numpy(pcm[:Bmax]).cuda())
        fill(eng, mel, Bmax)
        seqs = eng.generate_greedy(np.tile(np.array(PROMPT, np.int32), (Bmax, 1)), **KW)["sequences"]
        ref = None
        for B in batches:
            fill(eng, mel, B)
            res = eng.score_tokens(seqs[:B], 3, no_speech_id=NO_SPEECH, **KW)
            row = {k: res[k][0].view(np.uint32).copy() for k in ("logprob", "logprob_raw")}
            row["no_speech_prob"] = res["no_speech_prob"][:1].view(np.uint32).copy()
            if ref is None:
                ref = row
                rc, _, raw, ns = score_raw_call(eng, seqs[:B], 3, None, want=("raw", "ns"))
                assert rc == 0 and (ns == 7).all(), "no_speech_id < 0: the output is left untouched"
                # without options no eos is known: every position behind the prompt is scored; up to stream 0's eos the same bits
                n = int(np.count_nonzero(res["logprob_raw"][0]))
                assert np.array_equal(raw[0, 3:3 + n].view(np.uint32), ref["logprob_raw"][3:3 + n]) and (raw[0, 3:] != 0).all()
            for k in ref:
                assert np.array_equal(row[k], ref[k]), f"{dtype}: stream 0's {k} among {B} streams differs from {batches[0]}"
    finally:
        eng.close()


# ---- arbitrary ids, non-interference, errors: the micro model --------------------------------------------------------------------
MICRO_HEADS = [(1, 0), (1, 1)]


def micro_engine(max_batch, dtype="f32", use_graph=False):
    dims = wo.PRESETS["micro"]
    eng = make_engine(dims, wo.make_weights(dims, 0), T=T, max_batch=max_batch, dtype=dtype, heads=MICRO_HEADS, use_graph=use_graph)
    return dims, eng


def micro_fill(eng, B):
    pcm = np.stack([wo.synth_audio(32000, s, "speechlike") for s in range(B)])
    eng.encode(eng.logmel(torch.from_numpy(pcm).cuda()))
    eng.cross_kv(B)


def test_arbitrary_ids_masked_tokens_score_minus_infinity():
    """A suppressed id, and a text token behind an unpaired timestamp (a text token, ONE timestamp, a text token): -inf masked and a
    finite raw value at exactly those positions; everything else as the float64 numbers say."""
    dims, eng = micro_engine(2)
    assert dims.vocab > 50400
    ts = 50365
    kw = dict(timestamps=True, suppress=(1234,), begin_suppress=(220, 50257), max_new_tokens=16)
    seqs = np.array([PROMPT + [ts, 400, 1234, 401, ts + 5, ts + 5, 402, ts + 6, 50257],       # position 5: the suppressed id
                     PROMPT + [ts, 400, 401, ts + 7, 402, 50257, 50257, 50257, 50257]],       # position 7: text behind one timestamp; padding
                    dtype=np.int32)
    try:
        micro_fill(eng, 2)
        z = replay(eng, seqs)
        res = eng.score_tokens(seqs, 3, **kw)
    finally:
        eng.close()
    assert np.abs(z).max() < Z_MAX
    masked, alt, raw = host_scores(z, seqs, 3, options(kw))
    compare("arbitrary ids raw", res["logprob_raw"], raw)
    compare("arbitrary ids masked", res["logprob"], masked, alt)
    got_inf = np.isneginf(res["logprob"])
    assert got_inf[0, 5] and got_inf[1, 7]
    # the suppress list and the grammar mask the token at exactly those two positions.  (-inf elsewhere, checked position by position
    # against apply_logits_processors by `compare`, is the timestamp mass beating every text token of this random model.)
    opt = options(kw)
    for b, last in ((0, 11), (1, 8)):
        for p in range(3, last + 1):
            pre, tb = pre_mask(dims.vocab, [int(x) for x in seqs[b, :p]], 3, opt)
            assert bool(pre[seqs[b, p]]) == ((b, p) in ((0, 5), (1, 7))), (b, p)
            assert not got_inf[b, p] or pre[seqs[b, p]] or seqs[b, p] < tb, (b, p)
    print(f"arbitrary ids: -inf at {np.argwhere(got_inf).tolist()}")
    assert np.isfinite(res["logprob_raw"]).all() and (res["logprob_raw"][got_inf] < 0).all()
    for a in (res["logprob"], res["logprob_raw"]):
        assert (a[:, :3] == 0.0).all() and (a[1, 9:] == 0.0).all() and a[1, 8] != 0.0 and a[0, 11] != 0.0


@pytest.mark.parametrize("use_graph", [False, True])
def test_scoring_leaves_alignment_timestamps_and_the_next_generate_alone(use_graph):
    B = 2
    _, eng = micro_engine(B, use_graph=use_graph)
    kw = dict(max_new_tokens=12, min_new_tokens=6, timestamps=True, want_alignment=True)
    prompt = np.array([PROMPT] * B, dtype=np.int32)
    try:
        micro_fill(eng, B)
        out = eng.generate_greedy(prompt, **kw)
        seqs, L = out["sequences"], out["length"]
        al = eng.get_alignment(B, L - 1)
        ts = eng.token_timestamps(B, 3, L, [2 * T] * B)
        timings = eng.last_timings()
        res = eng.score_tokens(seqs, 3, no_speech_id=NO_SPEECH, **kw)
        assert np.array_equal(eng.get_alignment(B, L - 1), al)
        assert np.array_equal(eng.token_timestamps(B, 3, L, [2 * T] * B), ts)
        t2 = eng.last_timings()
        assert all(t2[k] == timings[k] for k in ("logmel_ms", "encode_ms", "cross_kv_ms", "greedy_ms", "decode_steps"))
        assert np.array_equal(eng.generate_greedy(prompt, **kw)["sequences"], seqs)
        assert np.array_equal(eng.get_alignment(B, L - 1), al)
        # ... and with a draft: the previous result offered as guesses, scored in between
        n_ok = min(int(np.argmax(np.append(r == 50257, True))) for r in seqs[:, 3:])
        n_ok = min(n_ok, kw["max_new_tokens"] - 2)
        assert n_ok >= 2
        draft = seqs[:, :3 + n_ok].astype(np.int32)
        first = eng.generate_greedy(draft, n_draft=n_ok, **kw)
        res2 = eng.score_tokens(first["sequences"], 3, no_speech_id=NO_SPEECH, **kw)
        second = eng.generate_greedy(draft, n_draft=n_ok, **kw)
        assert np.array_equal(first["sequences"], seqs) and np.array_equal(second["sequences"], seqs) and second["draft"] == first["draft"]
        assert np.array_equal(eng.get_alignment(B, L - 1), al)
        for k in res:
            assert np.array_equal(res[k], res2[k]), k
    finally:
        eng.close()


def test_argument_checks_leave_the_context_usable():
    """TW_ESTATE before cross_kv, TW_EINVAL for every argument check of the header, and a good call afterwards."""
    import ctypes as C
    from thewhisper_amd import _cabi

    dims, eng = micro_engine(2)
    P, V = 448, dims.vocab
    seqs = np.array([PROMPT + [50365, 400, 401, 50370, 50257]] * 2, dtype=np.int32)

    def opts(**over):
        o = _cabi.tw_greedy_opts()
        o.eos_id = o.pad_id = 50257
        o.timestamps, o.no_timestamps_id, o.max_initial_timestamp_index = 1, 50364, 50
        keep = []
        for name, n in (("begin_suppress", over.pop("n_begin_suppress", 2)), ("suppress", over.pop("n_suppress", 0))):
            arr = (C.c_int32 * max(1, n))(*([220] * n))
            keep.append(arr)
            setattr(o, "n_" + name, n)
            setattr(o, name, arr)
        for k, v in over.items():
            setattr(o, k, v)
        o._keep = keep
        return o

    try:
        rc, *_ = score_raw_call(eng, seqs, 3, opts())
        assert rc == TW_ESTATE, "before cross_kv"
        micro_fill(eng, 2)
        bad_id, neg_id = seqs.copy(), seqs.copy()
        bad_id[1, 5] = V
        neg_id[0, 0] = -1
        long_seq = np.tile(seqs[:1, :1], (64, P))
        cases = {
            "id >= vocab": dict(seqs=bad_id), "id < 0": dict(seqs=neg_id),
            "seq_len == n_prompt": dict(seqs=seqs, n_prompt=8), "seq_len > P": dict(seqs=np.tile(seqs, (1, 60)), seq_len=P + 1),
            "n_prompt < 1": dict(seqs=seqs, n_prompt=0), "ld < seq_len": dict(seqs=seqs, ld=7),
            "B = 0": dict(seqs=seqs, B=0), "B above the rows of a launch": dict(seqs=np.tile(seqs[:1], (65, 1))),
            "positions x streams above the row table": dict(seqs=long_seq),
            "begin-suppress list too long": dict(seqs=seqs, opts=opts(n_begin_suppress=65)),
            "suppress list too long": dict(seqs=seqs, opts=opts(n_suppress=1025)),
            "suppress count without its list": dict(seqs=seqs, opts=opts(n_suppress=3, suppress=None)),
            "negative begin-suppress count": dict(seqs=seqs, opts=opts(n_begin_suppress=-1)),
            "eos outside the vocabulary": dict(seqs=seqs, opts=opts(eos_id=V)), "pad outside the vocabulary": dict(seqs=seqs, opts=opts(pad_id=-1)),
            "no_speech_pos == seq_len - 1": dict(seqs=seqs, ns_id=NO_SPEECH, ns_pos=7), "no_speech_pos < 0": dict(seqs=seqs, ns_id=NO_SPEECH, ns_pos=-1),
            "no_speech_id >= vocab": dict(seqs=seqs, ns_id=V),
        }
        for what, kw in cases.items():
            kw.setdefault("opts", opts())
            kw.setdefault("n_prompt", 3)
            rc, lp, raw, ns = score_raw_call(eng, kw.pop("seqs"), kw.pop("n_prompt"), kw.pop("opts"), **kw)
            assert rc == TW_EINVAL, (what, rc)
            assert (lp == 7).all() and (raw == 7).all() and (ns == 7).all(), what
            assert eng.lib.tw_last_error(eng.ctx), what
        rc, lp, _, _ = score_raw_call(eng, seqs, 3, None)
        assert rc == TW_EINVAL, "masked numbers without options"
        rc, *_ = score_raw_call(eng, np.tile(seqs[:1], (3, 1)), 3, opts())
        assert rc == TW_ESTATE, "more streams than cross K/V slots"
        # still usable, and only the buffers asked for are written
        rc, lp, raw, ns = score_raw_call(eng, seqs, 3, opts(), ns_id=NO_SPEECH, ns_pos=6, want=("lp", "ns"))
        assert rc == 0 and (raw == 7).all() and (lp[:, :3] == 0).all() and not np.isnan(lp).any() and (lp[:, 3:] < 0).all()
        assert ((ns > 0) & (ns < 1)).all()
        good = eng.score_tokens(seqs, 3, timestamps=True)
        assert np.array_equal(good["logprob"], lp)
    finally:
        eng.close()


# ---- the backend ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draft", [False, True])
def test_backend_scores_beside_identical_words(draft):
    """Three consecutive ticks of one stream: words identical with the option on and off, `last_scores` holds the first pass's tokens
    (what a draft backend without the option remembers of the same call) and their numbers reproduce `avg_logprob`."""
    from tests.test_pipeline_glue import build_amd_pipeline, normalise
    from thewhisper_amd import AMDWhisperBackend

    def make(token_scores, draft_previous_tick=draft):
        return AMDWhisperBackend(None, chunk_length_s=10, asr_pipeline=build_amd_pipeline("micro", 10, 1, device="cuda", engine_factory=None),
                                 draft_previous_tick=draft_previous_tick, token_scores=token_scores)

    off, on = make(False), make(True)
    probe = off if draft else make(False, True)
    try:
        audio = wo.synth_audio(16000 * 7, 7, "speechlike")
        vocab = on.asr_pipeline.tokenizer.get_vocab()
        assert on.no_speech_id == vocab.get("<|nospeech|>", vocab.get("<|nocaptions|>"))
        for n in (16000 * 6, 16000 * 6 + 8000, 16000 * 7):
            a = off.transcribe(audio[:n].copy(), 3.0, 16000)
            b = on.transcribe(audio[:n].copy(), 3.0, 16000)
            assert normalise(a) == normalise(b) and [(w["start"], w["end"]) for w in a] == [(w["start"], w["end"]) for w in b]
            assert off.last_scores == [] and len(on.last_scores) >= 1
            for e in on.last_scores:
                n_tok = len(e["tokens"])
                assert n_tok <= len(e["logprob"]) <= n_tok + 1 and len(e["logprob_raw"]) == len(e["logprob"])
                assert np.isfinite(e["logprob"]).all() and (e["logprob"] <= 1e-6).all()
                assert e["avg_logprob"] == pytest.approx(float(e["logprob"].astype(np.float64).sum()) / (n_tok + 1), abs=0, rel=1e-12)
                assert (e["no_speech_prob"] is None) == (on.no_speech_id is None)
                if e["no_speech_prob"] is not None:
                    assert 0.0 < e["no_speech_prob"] < 1.0
            if not draft:
                assert normalise(probe.transcribe(audio[:n].copy(), 3.0, 16000)) == normalise(a)
            assert len(on.last_scores) == 1 and on.last_scores[0]["tokens"].tolist() == probe._last["ids"].tolist()      # the call's first-pass tokens
        if draft:
            assert on.reuse_stats["reused"] >= 1 and on.reuse_stats == off.reuse_stats
    finally:
        off.asr_pipeline.model.engine.close()
        on.asr_pipeline.model.engine.close()
        if probe is not off:
            probe.asr_pipeline.model.engine.close()
