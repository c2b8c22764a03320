"""Time per decode step of the greedy loop with a per-stream sequence bias (tw_generate_greedy_biased) against the unbiased call
(tw_generate_greedy), by the number of sequences per row.  Device events around the loop (tw_last_timings[3]), large-v3 shapes by
default, seeded synthetic weights and audio, forced-length decoding; every list size in turn within each repetition so that drift hits
all of them alike; prints the median, minimum and maximum per size and one JSON line.

A context keeps the captured step graphs of ONE flavour of call: a biased call behind an unbiased one (or the reverse) destroys them and
captures its own again, inside the window the device events time.  So every timed call here follows an UNTIMED call of the same size
directly: the timed one replays graphs that exist.  Beside the device time per step the wall time of the whole timed call is reported
(`wall_ms_per_call`): it contains what the device events do not - normalising and packing the lists in Python, checking and grouping them
in the library, the upload of the table.

    python tools/bench_bias.py --streams 16 --new-tokens 128 --per-row 0 100 1000 --reps 9
    python tools/bench_bias.py --streams 4 --per-row 0 4000        # 4000 per row fits the 16384 sequences of a call at 4 streams

Sequences are random text ids, 4 tokens each (65536 tokens per call hold 16384 of them), a tenth of them of length 1; biases are
+-0.001, so the decoded ids stay those of the unbiased call and the two loops do the same work but for the extra launch."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def random_lists(B, per_row, rng, text_ids=50000):
    rows = []
    for _ in range(B):
        d = {}
        while len(d) < per_row:
            n = 1 if rng.random() < 0.1 else 4
            d[tuple(int(t) for t in rng.integers(1, text_ids, size=n))] = float(rng.choice([-1e-3, 1e-3]))
        rows.append(d)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--chunk-s", type=int, default=10)
    ap.add_argument("--new-tokens", type=int, default=128)
    ap.add_argument("--per-row", type=int, nargs="+", default=[0, 100, 1000])
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch

    from thewhisper_amd import synthetic
    from thewhisper_amd.engine import WhisperEngine

    dims = synthetic.DIMS[args.model]
    B, T = args.streams, 50 * args.chunk_s
    dev = torch.device("cuda", 0)
    heads = [tuple(h) for h in synthetic.default_alignment_heads(dims["dec_layers"], dims["heads"])]
    eng = WhisperEngine(dims, T, max_batch=B, dtype=args.dtype, alignment_heads=heads, device=0, use_graph=True)
    try:
        eng.load_state_dict(synthetic.random_state_dict(dims, dev, seed=0))
        torch.cuda.empty_cache()
        g = torch.Generator(device=dev)
        g.manual_seed(2000)
        pcm = (torch.randn((B, args.chunk_s * 16000), device=dev, generator=g, dtype=torch.float32) * 0.1).clamp_(-1, 1)
        eng.encode(eng.logmel(pcm))
        eng.cross_kv(B)
        prompt = np.tile(np.array([[50258, 50259, 50360]], dtype=np.int32), (B, 1))
        kw = dict(max_new_tokens=args.new_tokens, min_new_tokens=args.new_tokens, timestamps=True)
        rng = np.random.default_rng(0)
        lists = {n: (random_lists(B, n, rng) if n else None) for n in args.per_row}
        ms = {n: [] for n in args.per_row}
        wall = {n: [] for n in args.per_row}
        same = {}
        ref = eng.generate_greedy(prompt, **kw)["sequences"]
        for rep in range(args.reps):
            for n, rows in lists.items():
                eng.generate_greedy(prompt, sequence_bias_rows=rows, **kw)     # untimed: leaves this flavour's step graphs captured
                t0 = time.perf_counter()
                out = eng.generate_greedy(prompt, sequence_bias_rows=rows, **kw)
                wall[n].append((time.perf_counter() - t0) * 1e3)
                tm = eng.last_timings()
                ms[n].append(tm["greedy_ms"] / tm["decode_steps"])
                if rep == 0:
                    same[n] = bool(np.array_equal(out["sequences"], ref))
    finally:
        eng.close()
    res = {"model": args.model, "streams": B, "new_tokens": args.new_tokens, "dtype": args.dtype, "reps": args.reps, "ms_per_step": {},
           "wall_ms_per_call": {},
           "ids_equal_unbiased": {str(k): v for k, v in same.items()}}
    for n, v in ms.items():
        res["ms_per_step"][str(n)] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        w = wall[n]
        res["wall_ms_per_call"][str(n)] = {"median": statistics.median(w), "min": min(w), "max": max(w)}
        print(f"{n:6d} sequences per row: {statistics.median(v):.4f} ms per step (min {min(v):.4f}, max {max(v):.4f}); "
              f"wall {statistics.median(w):.2f} ms per call (min {min(w):.2f}, max {max(w):.2f})")
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
