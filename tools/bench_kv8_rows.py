"""Times the rows launches of the fp8 contexts (k_decode_kv8_rows.hip: dec_cross_attn_kv8_rows_kernel) through the public interface: large-v3
dimensions, random weights, 10 s chunks, `dtype` "fp8f16" and "fp8".

    (a) verify64   one stream: a greedy call that offers its own 61 generated tokens as a draft behind a 3-token prompt - one 64-row
                   verify launch (every token confirmed, no step behind it)
    (b) score16x64 `score_tokens` over 16 streams x 64 tokens: 16 launches of 16 streams x 4 positions

Each figure is the median wall time of `--reps` calls (a call ends with a stream synchronisation) after `--warmup` calls.  The script
imports the package of the tree it runs in, so two checkouts are compared by running it from each, alternated (`--compare OTHER_TREE`
does that: child processes A B A B, one JSON line per child, then the ratio of the medians).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(dtype, reps, warmup):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from bench import DIMS, alignment_heads, random_state_dict
    from thewhisper_amd.engine import WhisperEngine

    dims, T, B = DIMS["large-v3"], 500, 16
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(dims, T, max_batch=B, dtype=dtype, alignment_heads=alignment_heads(dims), device=0)
    try:
        eng.load_state_dict(random_state_dict(dims, dev, seed=0))
        g = torch.Generator(device=dev)
        g.manual_seed(2000)
        pcm = (torch.randn((B, 10 * 16000), device=dev, generator=g, dtype=torch.float32) * 0.1).clamp_(-1, 1)
        eng.encode(eng.logmel(pcm))
        eng.cross_kv(B)
        prompt = np.tile(np.array([[50258, 50259, 50360]], dtype=np.int32), (B, 1))
        kw = dict(max_new_tokens=62, min_new_tokens=62)
        seq = eng.generate_greedy(prompt, **kw)["sequences"][:, :64].astype(np.int32)
        grid = {}

        def timed(fn):
            for _ in range(warmup):
                fn()
            ts = []
            for _ in range(reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ts), min(ts)

        def verify():
            out = eng.generate_greedy(seq[:1], n_draft=61, **kw)
            assert out["draft"]["launches"] == 1 and out["draft"]["accepted"] == 61, out["draft"]

        def score():
            eng.score_tokens(seq, 3)
            if hasattr(eng, "last_cross_grid"):
                grid["score16x64"] = eng.last_cross_grid()

        v, s = timed(verify), timed(score)
        return {"dtype": dtype, "verify64_ms": round(v[0], 4), "verify64_min_ms": round(v[1], 4), "score16x64_ms": round(s[0], 4),
                "score16x64_min_ms": round(s[1], 4), "cross_grid": grid}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--compare", default=None, help="another checkout of the project (built): run A = that tree, B = this tree, alternated")
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    if not a.compare:
        for dtype in ("fp8f16", "fp8"):
            print(json.dumps(measure(dtype, a.reps, a.warmup)), flush=True)
        return 0
    got = {"A": [], "B": []}
    for _ in range(a.rounds):
        for tag, tree in (("A", os.path.abspath(a.compare)), ("B", ROOT)):
            env = {k: v for k, v in os.environ.items() if k != "THEWHISPER_LIB"}
            run = subprocess.run([sys.executable, os.path.join(tree, "tools", "bench_kv8_rows.py"), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                 cwd=tree, env=env, capture_output=True, text=True, timeout=900)
            if run.returncode != 0:
                print(run.stdout[-2000:], run.stderr[-4000:], flush=True)
                return run.returncode
            for line in run.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    got[tag].append(r)
                    print(tag, line, flush=True)
    for dtype in ("fp8f16", "fp8"):
        for key in ("verify64_ms", "score16x64_ms"):
            m = {t: statistics.median(r[key] for r in got[t] if r["dtype"] == dtype) for t in got}
            print(f"{dtype} {key}: A {m['A']:.4f}  B {m['B']:.4f}  B / A {m['B'] / m['A']:.3f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
