"""Time per decode step of the greedy loop with the repeat options (tw_generate_greedy_repeat: repetition penalty, no-repeat n-gram)
against the plain call (tw_generate_greedy).  Device events around the loop (tw_last_timings[3]), large-v3 shapes by default, seeded
synthetic weights and audio, forced-length decoding, graph replay and plain launches; the settings in turn within each repetition so
that drift hits all of them alike; prints the median, minimum and maximum per setting and one JSON line.

A context keeps the captured step graphs of ONE flavour of call, so every timed call follows an UNTIMED call of the same setting
directly (tools/bench_bias.py): the first call after a change of flavour is dropped.

    python tools/bench_repeat.py --streams 16 --new-tokens 128 --reps 9

Settings: "plain"; "one-row" - row 0 with penalty 1.3 and N = 3, the others off; "all-rows" - every row so.  The options change the
decoded ids (that is their purpose), but every step does the same work whatever the ids: the loop has a fixed length."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--model", default="large-v3")
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--chunk-s", type=int, default=10)
    ap.add_argument("--new-tokens", type=int, default=128)
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
    settings = {
        "plain": {},
        "one-row": dict(repetition_penalty=[1.3] + [1.0] * (B - 1), no_repeat_ngram_size=[3] + [0] * (B - 1)),
        "all-rows": dict(repetition_penalty=1.3, no_repeat_ngram_size=3),
    }
    res = {"model": args.model, "streams": B, "new_tokens": args.new_tokens, "dtype": args.dtype, "reps": args.reps, "ms_per_step": {}}
    for graph in (True, False):
        eng = WhisperEngine(dims, T, max_batch=B, dtype=args.dtype, alignment_heads=heads, device=0, use_graph=graph)
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
            ms = {n: [] for n in settings}
            for _ in range(args.reps):
                for n, extra in settings.items():
                    eng.generate_greedy(prompt, **extra, **kw)     # untimed: leaves this flavour's step graphs captured
                    eng.generate_greedy(prompt, **extra, **kw)
                    tm = eng.last_timings()
                    ms[n].append(tm["greedy_ms"] / tm["decode_steps"])
        finally:
            eng.close()
        mode = "graph" if graph else "launches"
        res["ms_per_step"][mode] = {}
        for n, v in ms.items():
            res["ms_per_step"][mode][n] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            print(f"{mode:8s} {n:9s}: {statistics.median(v):.4f} ms per step (min {min(v):.4f}, max {max(v):.4f})", flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
