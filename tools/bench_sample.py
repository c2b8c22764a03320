"""Time per decode step of the sampling loop, by sampler flavour: greedy, temperature sampling, and sampling with top-k / top-p
filters (tw_generate_greedy / tw_generate_sample / tw_generate_sample_filtered).  Device events around the loop (tw_last_timings[3]),
large-v3 shapes by default, seeded synthetic weights and audio, every flavour in turn within each repetition so that drift hits all
of them alike; prints the median, minimum and maximum per flavour and one JSON line.

    python tools/bench_sample.py --streams 16 --new-tokens 128 --reps 9
    python tools/bench_sample.py --lib /path/to/an/older/libthewhisper_gfx950.so --no-filter      # a build without the filtered call

Compare two builds by running the two commands alternately (A B A B): the spread between the runs of one build is the yardstick for
the difference between the builds."""
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
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--lib", default=None, help="another build of the library (default: the tree's)")
    ap.add_argument("--no-filter", action="store_true", help="greedy and unfiltered sampling only (a library without the filtered call)")
    ap.add_argument("--label", default="this build")
    args = ap.parse_args()

    if args.lib:
        os.environ["THEWHISPER_LIB"] = args.lib
    import torch

    from thewhisper_amd import _cabi, synthetic
    from thewhisper_amd.engine import WhisperEngine

    if args.no_filter:
        _cabi.SYMBOLS[:] = [s for s in _cabi.SYMBOLS if s[0] != "tw_generate_sample_filtered"]
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
        seed = np.arange(B, dtype=np.uint64) + 1
        t = args.temperature
        flavours = {"greedy": lambda: eng.generate_greedy(prompt, **kw), "sample": lambda: eng.generate_sample(prompt, t, seed, **kw)}
        if not args.no_filter:
            flavours["sample top_k=50"] = lambda: eng.generate_sample(prompt, t, seed, **kw, top_k=50)
            flavours["sample top_p=0.9"] = lambda: eng.generate_sample(prompt, t, seed, **kw, top_p=0.9)
            flavours["sample top_k=50 top_p=0.9"] = lambda: eng.generate_sample(prompt, t, seed, **kw, top_k=50, top_p=0.9)
        ms = {name: [] for name in flavours}
        for rep in range(args.reps + 1):       # repetition 0 captures the graphs and is not counted
            for name, call in flavours.items():
                call()
                tm = eng.last_timings()
                if rep:
                    ms[name].append(tm["greedy_ms"] / tm["decode_steps"])
    finally:
        eng.close()
    out = {"label": args.label, "model": args.model, "streams": B, "new_tokens": args.new_tokens, "dtype": args.dtype, "reps": args.reps,
           "ms_per_step": {}}
    for name, v in ms.items():
        out["ms_per_step"][name] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        print(f"{args.label:12s} {name:28s} median {statistics.median(v):.4f} ms/step  (min {min(v):.4f}, max {max(v):.4f}, {len(v)} runs)")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
