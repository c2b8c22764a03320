"""Language detection on the device (tw_language_logits, tw_detect_language; k_decode.hip: lang_detect_kernel; THE RULE is in
include/thewhisper.h).

  1. the rule on planted logits: ids = torch.argmax of the row masked as HF's detect_language masks it (two stated exceptions: a row with
     nothing finite in the list answers the smallest listed id, a NaN counts as -inf), |p - softmax_float64| <= 1e-5, |sum p - 1| <= 1e-5
     (at most 128 float32 additions at 2^-24 each plus a few ulp of exp stay under 8e-6 relative on values <= 1), a row alone has the bit
     patterns it has among 64 rows;
  2. the context call on the three clips of tests/test_language_detection.py: strict f32 = hf_reference's detect_language; f16 / bf16 =
     the rule in numpy on the logits decode_step returns for <sot> on the same context; rows together = rows alone, bit for bit; two
     groups through slot0; generate_greedy after a detection = without it; use_graph 0 and 1;
  3. every TW_EINVAL / TW_ESTATE leaves the context usable;
  4. the drop-in: generate(language=None) learns through HF, then takes the plan (lang_slot = 1), one encoder call per pass.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_langid.py -s`` prints each case's figures.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import hf_reference as hr
from oracle import whisper_oracle as wo
from tests.lang_engines import lang_rule
from tests.util import make_engine

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TW_EINVAL, TW_ESTATE = -1, -3          # include/thewhisper.h
TW_LANG_MAX = 128
CHUNK_S, T_FRAMES = 10, 500


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.fixture(scope="module")
def setup():
    """The micro preset, the three clips and the HF reference's answers: computed once, shared, never changed."""
    dims = wo.PRESETS["micro"]
    w = wo.make_weights(dims, 0)
    ref = hr.patch_chunk_length(hr.build_hf_model(dims, w), CHUNK_S)
    fe = hr.build_feature_extractor(dims, CHUNK_S)
    audio = [wo.synth_audio(160000, s, k) for s, k in ((0, "speechlike"), (1, "noise"), (2, "sine"))]
    feats = fe(audio, sampling_rate=16000, return_tensors="pt", return_attention_mask=True)
    x, am = feats["input_features"], feats["attention_mask"]
    want_lang = ref.detect_language(input_features=x)
    assert len(set(want_lang.tolist())) > 1       # (the rows do get more than one language)
    gc = ref.generation_config
    return dict(dims=dims, w=w, ref=ref, x=x, am=am, want_lang=want_lang, sot=int(gc.decoder_start_token_id),
                lang_ids=sorted(int(v) for v in gc.lang_to_id.values()))


def _engine(setup, dtype="f32", use_graph=False, max_batch=3):
    return make_engine(setup["dims"], setup["w"], T=T_FRAMES, max_batch=max_batch, dtype=dtype, heads=[(0, 0)], use_graph=use_graph)


def _fill(eng, setup, rows=(0, 1, 2)):
    x = setup["x"][list(rows)].cuda()
    eng.encode(x)
    eng.cross_kv(len(rows))


# ---- 1. the rule on planted logits ------------------------------------------------------------------------------------
KINDS = 6     # row kinds: two-way tie, three-way tie, special values, everything -inf, a NaN on the largest, plain


def _lists(rng, V, n_lang, kind):
    if kind == "range":        # contiguous, as Whisper's
        lo = int(rng.integers(0, V - n_lang + 1))
        return np.arange(lo, lo + n_lang, dtype=np.int64)
    ids = {0, V - 1} if n_lang >= 2 else {V - 1}
    while len(ids) < n_lang:
        ids.add(int(rng.integers(1, V - 1)))
    return rng.permutation(np.array(sorted(ids), dtype=np.int64))


def _plant(rng, rows, V, ids, shift):
    x = (rng.standard_normal((rows, V)) * 4.0).astype(np.float32)
    n = len(ids)
    other = np.setdiff1d(np.arange(V), ids)
    for r in range(rows):
        k = (r + shift) % KINDS
        top = np.float32(np.abs(x[r, ids]).max() + 1.0)
        if k == 0 and n >= 2:
            a = rng.choice(n, 2, replace=False)
            x[r, ids[a]] = top
        elif k == 1 and n >= 3:
            a = rng.choice(n, 3, replace=False)
            x[r, ids[a]] = top
        elif k == 2:
            special = np.array([-np.inf, -0.0, 1e-42, 65504.0, -65504.0], np.float32)
            m = min(n, len(special))
            x[r, ids[rng.choice(n, m, replace=False)]] = rng.permutation(special)[:m]
        elif k == 3:
            x[r, ids] = -np.inf
        elif k == 4:
            x[r, ids[int(np.argmax(x[r, ids]))]] = np.nan
        x[r, other[rng.choice(len(other), 2, replace=False)]] = np.float32(1e6)     # non-listed logits above every listed one
    return x


def _expect(x, ids):
    """(ids, float64 softmax) per row: torch.argmax of HF's masked row, with the two stated exceptions."""
    rows, V = x.shape
    want_id = np.zeros(rows, np.int64)
    want_p = np.zeros((rows, len(ids)), np.float64)
    mask = torch.ones(V, dtype=torch.bool)
    mask[torch.from_numpy(ids)] = False
    for r in range(rows):
        row = torch.from_numpy(x[r].copy())
        row[torch.isnan(row) & ~mask] = -np.inf            # exception: a NaN counts as -inf
        row[mask] = -np.inf                                # HF:models/whisper/generation_whisper.py (detect_language)
        if torch.isinf(row).all():
            want_id[r] = int(ids.min())                    # exception: nothing finite - the smallest listed id, every p = 0
            continue
        want_id[r] = int(row.argmax(-1))
        want_p[r] = torch.softmax(row[torch.from_numpy(ids)].double(), -1).numpy()
    return want_id, want_p


@pytest.mark.parametrize("V", [51866, 1003])
@pytest.mark.parametrize("kind", ["range", "scattered"])
def test_rule_on_planted_logits(setup, V, kind):
    eng = _engine(setup, max_batch=1)
    rng = np.random.default_rng(V + len(kind))
    worst_p = worst_s = 0.0
    try:
        for n_lang in (1, 2, 63, 64, 65, 99, 100, 128):
            ids = _lists(rng, V, n_lang, kind)
            for rows in (1, 5, 64):
                for shift in (range(KINDS) if rows == 1 else (0, 3) if rows == 5 else (0,)):
                    x = _plant(rng, rows, V, ids, shift)
                    xd = torch.from_numpy(x).cuda()
                    got = eng.language_logits(xd, ids)
                    want_id, want_p = _expect(x, ids)
                    assert np.array_equal(got["ids"], want_id), (n_lang, rows, shift, got["ids"], want_id)
                    live = want_p.sum(axis=1) > 0
                    worst_p = max(worst_p, float(np.abs(got["probs"] - want_p).max()))
                    worst_s = max(worst_s, float(np.abs(got["probs"][live].astype(np.float64).sum(axis=1) - 1.0).max()) if live.any() else 0.0)
                    assert (got["probs"][~live] == 0.0).all()
                    if rows > 1:       # a row computed alone has the bit patterns it has in the batch
                        for r in range(rows):
                            one = eng.language_logits(xd[r : r + 1].contiguous(), ids)
                            assert int(one["ids"][0]) == int(got["ids"][r])
                            assert np.array_equal(one["probs"][0].view(np.uint32), got["probs"][r].view(np.uint32)), (n_lang, rows, r)
        print(f"V={V} {kind}: worst |p - softmax64| = {worst_p:.3e}, worst |sum p - 1| = {worst_s:.3e}")
        assert worst_p <= 1e-5
        assert worst_s <= 1e-5
    finally:
        eng.close()


# ---- 2. the context call ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_detect_language_on_the_context(setup, dtype, use_graph):
    sot, ids = setup["sot"], setup["lang_ids"]
    eng = _engine(setup, dtype, use_graph)
    try:
        _fill(eng, setup)
        got = eng.detect_language(3, sot, ids)
        if dtype == "f32":
            assert got["ids"].tolist() == setup["want_lang"].tolist()
        # self-consistency: the rule in numpy on the logits decode_step returns for <sot> on the same context
        eng.decoder_reset(3)
        lg = eng.decode_step([sot] * 3).cpu().numpy()
        want = lang_rule(lg, ids)
        assert np.array_equal(got["ids"], want["ids"])
        dev = float(np.abs(got["probs"].astype(np.float64) - want["probs"]).max())
        print(f"{dtype} graph={use_graph}: ids {got['ids'].tolist()}, winners {got['probs'].max(axis=1)}, |p - numpy rule| = {dev:.3e}")
        assert dev <= 1e-5 and np.abs(got["probs"].sum(axis=1) - 1.0).max() <= 1e-5
        again = eng.detect_language(3, sot, ids)
        assert np.array_equal(again["ids"], got["ids"]) and np.array_equal(again["probs"].view(np.uint32), got["probs"].view(np.uint32))
        # generate_greedy after a detection returns the ids it returns without it
        kw = dict(max_new_tokens=8, eos_id=50257, pad_id=50257, timestamps=True, no_timestamps_id=50364, begin_suppress=(220, 50257))
        prompt = np.array([[sot, int(got["ids"][b]), 50360] for b in range(3)], np.int32)
        _fill(eng, setup)
        plain = eng.generate_greedy(prompt, **kw)["sequences"].copy()
        _fill(eng, setup)
        eng.detect_language(3, sot, ids)
        after = eng.generate_greedy(prompt, **kw)["sequences"]
        assert np.array_equal(plain, after)
        # rows filled in two groups through slot0
        eng.encode(setup["x"][[0]].cuda())
        eng.cross_kv(1)
        eng.encode(setup["x"][[1, 2]].cuda(), slot0=1)
        eng.cross_kv(2, slot0=1)
        two = eng.detect_language(3, sot, ids)
        assert np.array_equal(two["ids"], got["ids"]) and np.array_equal(two["probs"].view(np.uint32), got["probs"].view(np.uint32))
        # three rows together = each row alone, bit for bit
        for b in range(3):
            _fill(eng, setup, rows=(b,))
            one = eng.detect_language(1, sot, ids)
            assert int(one["ids"][0]) == int(got["ids"][b])
            assert np.array_equal(one["probs"][0].view(np.uint32), got["probs"][b].view(np.uint32)), (dtype, b)
    finally:
        eng.close()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------
def _raw_detect(eng, B, sot, ids, n=None, null=None):
    arr = np.ascontiguousarray(np.asarray(ids, np.int32))
    out_id = np.zeros(64, np.int32)
    out_p = np.zeros(64 * TW_LANG_MAX, np.float32)
    p_ids = None if null == "ids" else arr.ctypes.data_as(C.POINTER(C.c_int32))
    p_out = None if null == "out" else out_id.ctypes.data_as(C.POINTER(C.c_int32))
    return eng.lib.tw_detect_language(eng.ctx, B, sot, p_ids, len(arr) if n is None else n, p_out, out_p.ctypes.data_as(C.POINTER(C.c_float)), eng._sp())


def _raw_logits(eng, xd, rows, V, ids, n=None, null=None):
    arr = np.ascontiguousarray(np.asarray(ids, np.int32))
    out_id = np.zeros(64, np.int32)
    p_x = None if null == "logits" else C.c_void_p(xd.data_ptr())
    p_ids = None if null == "ids" else arr.ctypes.data_as(C.POINTER(C.c_int32))
    p_out = None if null == "out" else out_id.ctypes.data_as(C.POINTER(C.c_int32))
    return eng.lib.tw_language_logits(0, p_x, V, rows, p_ids, len(arr) if n is None else n, p_out, None, eng._sp())


def test_refusals_leave_the_context_usable(setup):
    sot, ids, V = setup["sot"], setup["lang_ids"], setup["dims"].vocab
    eng = _engine(setup)
    try:
        assert _raw_detect(eng, 1, sot, ids) == TW_ESTATE          # nothing encoded yet
        eng.encode(setup["x"][[0, 1]].cuda())
        eng.cross_kv(2)
        assert _raw_detect(eng, 3, sot, ids) == TW_ESTATE          # three rows, the cross K/V hold two
        _fill(eng, setup)
        want = eng.detect_language(3, sot, ids)
        many = list(range(TW_LANG_MAX + 1))
        for rc in (_raw_detect(eng, 3, sot, ids, null="ids"), _raw_detect(eng, 3, sot, ids, null="out"),
                   _raw_detect(eng, 3, sot, ids, n=0), _raw_detect(eng, 3, sot, many), _raw_detect(eng, 3, sot, ids[:-1] + [V]),
                   _raw_detect(eng, 3, sot, [-1] + ids[1:]), _raw_detect(eng, 3, V, ids), _raw_detect(eng, 3, -1, ids),
                   _raw_detect(eng, 3, sot, ids[:-1] + [ids[0]]), _raw_detect(eng, 0, sot, ids), _raw_detect(eng, 4, sot, ids)):
            assert rc == TW_EINVAL
        xd = torch.zeros((2, V), dtype=torch.float32).cuda()
        for rc in (_raw_logits(eng, xd, 2, V, ids, null="logits"), _raw_logits(eng, xd, 2, V, ids, null="ids"),
                   _raw_logits(eng, xd, 2, V, ids, null="out"), _raw_logits(eng, xd, 2, V, ids, n=0), _raw_logits(eng, xd, 2, V, many),
                   _raw_logits(eng, xd, 2, V, ids[:-1] + [V]), _raw_logits(eng, xd, 2, V, [-1] + ids[1:]),
                   _raw_logits(eng, xd, 2, V, ids[:-1] + [ids[0]]), _raw_logits(eng, xd, 0, V, ids)):
            assert rc == TW_EINVAL
        with pytest.raises(RuntimeError, match="tw_detect_language"):
            eng.detect_language(3, sot, [])
        # ... and the context still detects and decodes
        again = eng.detect_language(3, sot, ids)
        assert np.array_equal(again["ids"], want["ids"]) and np.array_equal(again["probs"].view(np.uint32), want["probs"].view(np.uint32))
        prompt = np.array([[sot, int(want["ids"][b]), 50360] for b in range(3)], np.int32)
        out = eng.generate_greedy(prompt, max_new_tokens=4, eos_id=50257, pad_id=50257, timestamps=True, no_timestamps_id=50364)
        assert out["sequences"].shape[0] == 3
    finally:
        eng.close()


# ---- 4. the drop-in ---------------------------------------------------------------------------------------------------
def test_dropin_generate_detects_on_the_plan(setup):
    from thewhisper_amd import ASRPipeline

    dims, ref, x, am = setup["dims"], setup["ref"], setup["x"], setup["am"]
    pipe = ASRPipeline(hr.build_hf_model(dims, setup["w"]), feature_extractor=hr.build_feature_extractor(dims, CHUNK_S),
                       tokenizer=hr.build_tokenizer(dims), chunk_length_s=CHUNK_S, device="cuda", torch_dtype=torch.float32, batch_size=3)
    model = pipe.model
    gk = dict(language=None, task="transcribe", num_beams=1, do_sample=False, max_new_tokens=16, return_timestamps=True)
    want = ref.generate(input_features=x, attention_mask=am, **gk)
    first = model.generate(input_features=x.cuda(), attention_mask=am.cuda(), **gk).cpu()      # learns through HF
    assert torch.equal(want, first), (want, first)
    assert model.last_plan is not None and model.last_plan.lang_slot == 1
    assert model.last_plan.lang_ids == tuple(setup["lang_ids"])
    from thewhisper_amd import shortform

    eng = model.engine
    calls = {"encode": 0, "pass": 0}
    real_encode, real_run = eng.encode, shortform.Pass.run

    def counting_encode(*a, **k):
        calls["encode"] += 1
        return real_encode(*a, **k)

    def counting_run(self, *a, **k):
        calls["pass"] += 1
        return real_run(self, *a, **k)

    eng.encode, shortform.Pass.run = counting_encode, counting_run
    try:
        model.last_languages = None
        second = model.generate(input_features=x.cuda(), attention_mask=am.cuda(), **gk).cpu()  # takes the plan
    finally:
        del eng.encode
        shortform.Pass.run = real_run
    assert torch.equal(want, second), (want, second)
    assert model.last_plan.lang_slot == 1
    assert model.last_languages == setup["want_lang"].tolist()
    assert calls["pass"] >= 1 and calls["encode"] == calls["pass"]      # one encoder call per pass: none for the detection
    got_lang = model.detect_language(input_features=x.cuda()).cpu()
    assert torch.equal(got_lang, setup["want_lang"])
