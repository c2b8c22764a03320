"""The decoder's cross-attention kernels (k_decode.hip: dec_cross_attn_kernel over attn_mfma_block, dec_cross_attn_kv8_kernel over
attn_mfma_block_kv8) against the numpy oracle at EVERY encoder frame, in every element type and in every form the frame count selects:

    T = 50    Tp 64: one 64-key group, seven wavefronts clamped and masked          f32 bf16 fp8a16
    T = 500   Tp 512: single pass, 12 masked keys; fp8: G = 1                      f32 bf16 f16 fp8a16 fp8a8
    T = 750   Tp 768: two chunks, half of the second clamped; G = 2                f32 bf16 f16
    T = 1000  Tp 1024: two full chunks, masked tail; G = 2                         bf16 f16 fp8a16
    T = 1450  Tp 1472: third chunk partial                                         bf16 fp8a16
    T = 1500  Tp 1536: three chunks; G = 3                                         f32 bf16 f16 fp8a16 fp8a8

The model is tests/cross_pointer_model.py: every query puts probability 1 (to float32) on one frame chosen by the test - head 0 on the
frame whose index is the token id fed, head 1 on a fixed map of the position that cycles through the frames on either side of every
16-, 32-, 64- and 512-key edge - so a key that is dropped, read from the neighbouring slot or paired with the wrong value or scale byte
moves that query's logits by 0.31 relative L2 or more (tests/test_cross_pointer_model.py: 10 times the bf16 tolerance, 3 times the fp8
bound), where on random weights it moves them by 1e-3.  17 streams x P positions (16 x P >= T; 16 streams in fp8a8 contexts, which hold
no more) point at every frame.

Per case, on one engine: (a) `decode_step` over all P positions - relative L2 of every (stream, step) against the oracle within the
suite's tolerances (f32 2e-5, bf16 3e-2, f16 4e-3) and the oracle's top-1 wherever its margin is clear (bf16 0.25, f16 0.03, fp8 1.0);
fp8: per step over the streams against OracleWhisperMXFP8 on the engine's encoder states within test_decoder_mxfp8_teacher_forced's
4e-2 (a16) / 6e-2 (a8), per (stream, step) against the f32 oracle within 0.1; (b) `get_alignment`: every row's arg-max is the target
frame, its value is >= 1 - T exp(-(m_min - 1)) (m_min: the smallest score margin of the reference, > 24), the row sums to 1 within
1e-4 and is finite and >= 0, in f32 within 1e-4 of the oracle's row; (c) `score_tokens` of the same ids on the same cache: `logprob_raw`
equals the float64 log-softmax of (a)'s logits within test_gpu_score's 1e-4 (f32: the oracle's too), and - bf16, f32, fp8a16 at T = 500
and 1500 - a `generate_greedy` call that takes the first P - 1 ids as prompt with P - 2 of them forced (a prompt of all P leaves the
model's P positions nothing to generate) leaves alignment rows array_equal to the stepped ones; (e) - bf16 at T = 750, fp8a16 at
T = 1500 - stream 16's logits and alignment rows are array_equal to the same clip and ids alone in a one-stream engine.  (d) One child
process under TW_FUSE_CQ=0 (the plain launch sequence: the query is loaded, not formed in LDS) repeats (a) and (b) for four cases.
Run on the MI355X box: ``pytest -m gpu tests/test_gpu_cross.py -s`` prints each case's figures.

Measured on the MI355X, largest (stream, step) figure over the cases of a type: f32 6.9e-7, bf16 7.4e-3, f16 8.5e-4; fp8a16 6.7e-2 against
the f32 oracle and 1.4e-3 per step against its restatement, fp8a8 7.5e-2 and 1.2e-2.  Alignment rows: every arg-max on its target, value
there 1.0 in every context (floor >= 0.99999997), |row sum - 1| <= 8.1e-11, f32 rows 1.1e-16 from the oracle's, the others <= 6.9e-12.
Rows mode against the stepped logits 1.2e-6 at most, f32 against the oracle 1.3e-5; forced-prefix rows, the stream alone and the plain
sequence as asserted.  A library that masks key 512 in the two-pass attn_mfma_block and pairs key 1024's value with key 1025's
probability in attn_mfma_block_kv8<8, 3> fails every case above 512 keys (f32, bf16, f16: 0.48 ... 0.55 at the first query pointing at
512) and the three G = 3 fp8 cases (0.60 ... 0.74 at the first pointing at 1024); test_decoder_teacher_forced fails under it in f32 only,
test_decoder_mxfp8_teacher_forced not at all - DESIGN.md 2.7.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import whisper_oracle as wo
from tests import cross_pointer_model as xm
from tests.util import make_engine

pytestmark = pytest.mark.gpu
TOL = {"f32": 2e-5, "bf16": 3e-2, "f16": 4e-3}          # tests/test_gpu_parity.py: test_decoder_teacher_forced
FP8_TOL = {"fp8a16": 4e-2, "fp8a8": 6e-2}               # ... test_decoder_mxfp8_teacher_forced, against the restatement
FP8_EXACT = 0.1                                         # ... its widest figure against exact arithmetic
MARGIN = {"bf16": 0.25, "f16": 0.03, "fp8a16": 1.0, "fp8a8": 1.0}
ALIGN_TOL = 1e-4                                        # test_greedy_ids_alignment_and_timestamps
ROWS_TOL = 1e-4                                         # tests/test_gpu_score.py: TOL
Z_MAX = 60.0
CASES = {50: ("f32", "bf16", "fp8a16"), 500: ("f32", "bf16", "f16", "fp8a16", "fp8a8"), 750: ("f32", "bf16", "f16"),
         1000: ("bf16", "f16", "fp8a16"), 1450: ("bf16", "fp8a16"), 1500: ("f32", "bf16", "f16", "fp8a16", "fp8a8")}
FORCED = {(T, t) for T in (500, 1500) for t in ("bf16", "f32", "fp8a16")}
ALONE = {(750, "bf16"), (1500, "fp8a16")}
PLAIN = [(500, "f32"), (750, "bf16"), (1500, "f16"), (1000, "fp8a16")]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    yield
    xm.build.cache_clear()          # 0.34 GB of oracle logits at T = 1500: not kept for the rest of the session


def n_streams(dtype):
    return 16 if dtype == "fp8a8" else xm.B          # TW_BF16_MXFP8 contexts hold 16 streams


def step_all(b, T, dtype, rows):
    """A `len(rows)`-stream engine on streams `rows` of the model: encode, cross_kv, decoder_reset, every position by `decode_step`.
    (engine - the caller closes it -, logits [P, B, V] on the device, alignment rows [B, 2, P, T], the engine's encoder states or None)."""
    ids = b.ids[rows]
    B, P = ids.shape
    eng = make_engine(b.dims, b.weights, T=T, max_batch=B, dtype=dtype, heads=xm.HEADS)
    try:
        enc = eng.encode(torch.from_numpy(b.mel[rows]).cuda(), return_hidden=dtype in FP8_TOL)
        eng.cross_kv(B)
        eng.decoder_reset(B)
        got = torch.empty((P, B, b.dims.vocab), dtype=torch.float32, device="cuda")
        for p in range(P):
            got[p] = eng.decode_step(ids[:, p].tolist())
        return eng, got, eng.get_alignment(B, P), enc.cpu().numpy() if enc is not None else None
    except BaseException:
        eng.close()
        raise


def judge(what, b, T, dtype, rows, got, al, enc, fused=True):
    """(a) and (b) of one stepped run; returns the float64 log-softmax of the stepped logits at the next id and the oracle's, [B, P] each."""
    ids, ref, g = b.ids[rows], b.logits[rows], b.g
    B, P = ids.shape
    tg = xm.targets(ids, g)
    fp8, dev = dtype in FP8_TOL, got.device
    ref_cross, refq_d = b.cross[rows], None
    if fp8:   # the restatement of the quantised arithmetic, on the ENGINE's encoder states as in test_decoder_mxfp8_teacher_forced
        oq = wo.OracleWhisperMXFP8(b.dims, b.weights, T=T, cross_q_ahead=fused, act_quant=dtype == "fp8a8")
        refq, ref_cross = oq.decode(ids, oq.new_cache(enc), want_cross=xm.HEADS)
        refq_d = torch.from_numpy(np.ascontiguousarray(refq, dtype=np.float32)).to(dev)
    ref_d = torch.from_numpy(ref).to(dev)                               # [B, P, V]
    ids_d = torch.from_numpy(ids.astype(np.int64)).to(dev)
    rel = torch.empty((P, B), dtype=torch.float64, device=dev)      # per (step, stream) against the float32 oracle
    rel_q = torch.zeros((P,), dtype=torch.float64, device=dev)      # per step over the streams against the restatement
    top_ok = torch.empty((P, B), dtype=torch.bool, device=dev)
    lp_got = torch.zeros((B, P), dtype=torch.float64, device=dev)
    lp_ref = torch.zeros((B, P), dtype=torch.float64, device=dev)
    for p in range(P):
        z, r = got[p].double(), ref_d[:, p].double()
        rel[p] = torch.linalg.norm(z - r, dim=-1) / torch.linalg.norm(r, dim=-1)
        if fp8:
            q = refq_d[:, p].double()
            rel_q[p] = torch.linalg.norm(z - q) / torch.linalg.norm(q)
        top2 = torch.topk(r, 2, dim=-1)
        clear = (top2.values[:, 0] - top2.values[:, 1]) > MARGIN.get(dtype, float("inf"))
        top_ok[p] = ~clear | (z.argmax(-1) == top2.indices[:, 0])
        if p + 1 < P:
            lp_got[:, p + 1] = torch.log_softmax(z, -1).gather(1, ids_d[:, p + 1, None])[:, 0]
            lp_ref[:, p + 1] = torch.log_softmax(r, -1).gather(1, ids_d[:, p + 1, None])[:, 0]
    finite, z_max = bool(torch.isfinite(got).all()), float(got.abs().max())
    rel, rel_q, top_ok, lp_got, lp_ref = (t.cpu().numpy() for t in (rel, rel_q, top_ok, lp_got, lp_ref))
    # (b) the alignment rows
    m_min = float(xm.margins(ref_cross, tg).min())
    floor = xm.floor_probability(T, m_min)
    on = np.take_along_axis(al, tg[..., None], axis=-1)[..., 0]
    sums = np.abs(al.astype(np.float64).sum(-1) - 1.0)
    d_al = float(np.abs(al - b.cross[rows]).max())
    bound = FP8_EXACT if fp8 else TOL[dtype]
    at = np.unravel_index(int(np.nanargmax(rel)), rel.shape)
    print(f"{what}: step mode, largest relative L2 {np.nanmax(rel):.2e} at (step {at[0]}, stream {at[1]}) (bound {bound:g})"
          + (f", per step over the streams against the restatement {np.nanmax(rel_q):.2e} (bound {FP8_TOL[dtype]:g})" if fp8 else "")
          + f"; top-1 differs at {int((~top_ok).sum())} clear steps; max |logit| {z_max:.1f}; alignment rows: smallest value on a target "
          f"{on.min():.8f} (floor {floor:.8f}, m_min {m_min:.2f}), largest |row sum - 1| {sums.max():.1e}, against the float32 oracle's rows {d_al:.1e}")
    assert finite and z_max < Z_MAX

    def where(bad):
        p, s = (int(x) for x in bad[0])
        return f"first (step, stream) {(p, s)}, id fed there {int(ids[s, p])}, frame g(p) {int(g[p])}"

    bad = np.argwhere(~(rel < bound))
    assert not len(bad), (what, where(bad), "relative L2", float(rel[tuple(bad[0])]), "bound", bound)
    if fp8:
        bad = np.argwhere(~(rel_q < FP8_TOL[dtype]))
        assert not len(bad), (what, "first step above the restatement's bound", int(bad[0][0]), float(rel_q[bad[0][0]]), FP8_TOL[dtype])
    assert top_ok.all(), (what, "top-1 is not the oracle's:", where(np.argwhere(~top_ok)))
    assert floor >= 0.999, (what, floor, m_min)
    assert al.shape == (B, 2, P, T) and np.isfinite(al).all() and (al >= 0).all(), what
    miss = np.argwhere(al.argmax(-1) != tg)                            # (stream, head, position)
    assert not len(miss), (what, "first (stream, head, position) whose alignment row peaks elsewhere", miss[0].tolist(),
                           "target", int(tg[tuple(miss[0])]), "peak", int(al[tuple(miss[0])].argmax()))
    assert (on >= floor).all(), (what, "(stream, head, position) below the floor", np.argwhere(on < floor)[:3].tolist(), float(on.min()), floor)
    assert (sums <= ALIGN_TOL).all(), (what, float(sums.max()))
    if dtype == "f32":
        assert d_al < ALIGN_TOL, (what, d_al)
    return lp_got, lp_ref


def rows_mode(what, eng, b, dtype, rows, al, lp_got, lp_ref, forced):
    """(c): `score_tokens`, then - `forced` - the forced-prefix prefill, on the cache the steps ran on."""
    ids = b.ids[rows]
    B, P = ids.shape
    off = dict(begin_suppress=(), suppress=(), timestamps=False)
    raw = eng.score_tokens(ids, 1, **off)["logprob_raw"].astype(np.float64)
    d_rows, d_oracle = np.abs(raw - lp_got), np.abs(raw - lp_ref)
    note = ""
    if forced:
        eng.generate_greedy(ids[:, :P - 1], n_forced=P - 2, max_new_tokens=P, want_alignment=True, **off)
        al2 = eng.get_alignment(B, P - 1)
        same = np.array_equal(al2, al[:, :, :P - 1])
        note = f"; forced-prefix alignment rows {'identical to' if same else 'DIFFER from'} the stepped ones"
    print(f"{what}: rows mode against the stepped logits {d_rows.max():.2e} (bound {ROWS_TOL:g}), against the oracle {d_oracle.max():.2e}{note}")
    assert raw.shape == (B, P) and (raw[:, 0] == 0.0).all() and np.isfinite(raw).all()
    assert (d_rows <= ROWS_TOL).all(), (what, "rows mode differs from step mode at (stream, position):", np.argwhere(d_rows > ROWS_TOL)[:5].tolist())
    if dtype == "f32":
        assert (d_oracle <= ROWS_TOL).all(), (what, np.argwhere(d_oracle > ROWS_TOL)[:5].tolist())
    if forced:
        diff = np.argwhere((al2 != al[:, :, :P - 1]).any(-1))
        assert same, (what, "first (stream, head, position) whose forced-prefix alignment row is not the stepped one", diff[0].tolist())


def pointer_case(T, dtype, fused=True):
    b = xm.build(T)
    rows = np.arange(n_streams(dtype))
    what = f"cross pointer T={T} B={len(rows)} {dtype}" + ("" if fused else " plain sequence")
    eng, got, al, enc = step_all(b, T, dtype, rows)
    try:
        lp_got, lp_ref = judge(what, b, T, dtype, rows, got, al, enc, fused)
        if fused:
            rows_mode(what, eng, b, dtype, rows, al, lp_got, lp_ref, (T, dtype) in FORCED)
    finally:
        eng.close()
    if fused and (T, dtype) in ALONE:          # (e) the last stream - the second group of sixteen's first - alone in a one-stream engine
        last = rows[-1:]
        one, got1, al1, _ = step_all(b, T, dtype, last)
        one.close()
        same_z, same_al = bool(torch.equal(got1[:, 0], got[:, -1])), np.array_equal(al1[0], al[-1])
        print(f"{what}: stream {int(last[0])} alone: logits {'identical' if same_z else 'DIFFER'}, alignment rows {'identical' if same_al else 'DIFFER'}")
        assert same_z, (what, "first step at which the stream alone differs", int(torch.nonzero((got1[:, 0] != got[:, -1]).any(-1))[0]))
        assert same_al, what


# T outermost: the types share one oracle run
@pytest.mark.parametrize("T,dtype", [(T, t) for T, types in CASES.items() for t in types])
def test_cross_pointer_every_frame_step_rows_and_alignment(T, dtype):
    pointer_case(T, dtype)


def plain_child():
    """(d), in the child: TW_FUSE_CQ=0 is read once per process."""
    assert os.environ.get("TW_FUSE_CQ") == "0"
    for T, dtype in PLAIN:
        pointer_case(T, dtype, fused=False)


def test_cross_pointer_on_the_plain_launch_sequence():
    """`FQ = false`: dec_cross_attn_kernel / dec_cross_attn_kv8_kernel load the query the separate projection launch wrote instead of forming
    it in LDS from the accumulated one.  (a) and (b) for f32 at T = 500, bf16 at 750, f16 at 1500, fp8a16 at 1000, in one child process."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run([sys.executable, "-c", "from tests.test_gpu_cross import plain_child; plain_child()"], env=dict(os.environ, TW_FUSE_CQ="0"),
                         cwd=root, timeout=600, capture_output=True, text=True)
    print(run.stdout)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-4000:])
    assert run.stdout.count("plain sequence: step mode") == len(PLAIN)
