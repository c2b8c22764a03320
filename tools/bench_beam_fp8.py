"""Times a beam call of the float16 fp8 context (k_decode_kv8_beams.hip: dec_cross_attn_kv8_beams_kernel) beside the same call of the plain
float16 context, through the public interface: large-v3 dimensions, random weights, 10 s chunks (T = 500, Tp = 512), 8 clips x 8 beams =
64 rows, `--tokens` new tokens with <eos> held back (min_new_tokens), so every call runs the same number of steps.

One JSON line per dtype: the median and the smallest `greedy_ms / decode_steps` of `tw_last_timings` (device time of the beam loop
between two events, per step) over `--reps` calls after `--warmup` calls, the cross-attention grid of a step, and the bytes of cross
K / V^T (scale bytes included) a workgroup streams per step, head and clip.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure(dtype, reps, warmup, tokens):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from bench import DIMS, alignment_heads, random_state_dict
    from thewhisper_amd.engine import WhisperEngine

    dims, T, n, K = DIMS["large-v3"], 500, 8, 8
    dev = torch.device("cuda", 0)
    eng = WhisperEngine(dims, T, max_batch=n * K, dtype=dtype, alignment_heads=alignment_heads(dims), device=0)
    try:
        eng.load_state_dict(random_state_dict(dims, dev, seed=0))
        g = torch.Generator(device=dev)
        g.manual_seed(2000)
        pcm = (torch.randn((n, 10 * 16000), device=dev, generator=g, dtype=torch.float32) * 0.1).clamp_(-1, 1)
        eng.encode(eng.logmel(pcm))
        eng.cross_kv(n)
        prompt = np.tile(np.array([[50258, 50259, 50360]], dtype=np.int32), (n, 1))
        per_step = []
        for i in range(warmup + reps):
            eng.generate_beam(prompt, K, max_new_tokens=tokens, min_new_tokens=tokens)
            t = eng.last_timings()
            if i >= warmup:
                per_step.append(t["greedy_ms"] / t["decode_steps"])
        Tp = (T + 63) // 64 * 64
        kv = 2 * Tp * 64 * (1 if dtype == "fp8f16" else 2) + (2 * Tp if dtype == "fp8f16" else 0)
        return {"dtype": dtype, "clips": n, "beams": K, "steps": t["decode_steps"], "step_ms": round(statistics.median(per_step), 5),
                "step_min_ms": round(min(per_step), 5), "cross_grid": eng.last_cross_grid(), "cross_kv_bytes_per_step_head_clip": kv}
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=32)
    a = ap.parse_args()
    for dtype in ("f16", "fp8f16", "f16", "fp8f16"):   # alternated: two lines per dtype
        print(json.dumps(measure(dtype, a.reps, a.warmup, a.tokens)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
