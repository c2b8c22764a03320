"""Device time of one tw_resample launch at serving-tick sizes (not part of bench.py).

16 rows x 0.5 s of int16 stereo at 48, 44.1 and 8 kHz -> 16 kHz mono float32: what a tick of 16 resampled sessions costs in
front of the log-mel.  HIP events around ``--iters`` back-to-back launches after a warm-up, repeated ``--repeats`` times; the
figure to hold it against is the draft tick of BASELINE config 3.

    python tools/resample_timing.py --out profiles/resample_timing.json
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_timing.py measures on the MI355X: no GPU here, nothing measured")
    from thewhisper_amd import resample as rs

    launch = rs._device_kernel(0)
    rng = np.random.default_rng(0)
    results = []
    for sr in (48000, 44100, 8000):
        L, M, half, tpo = rs.plan(sr)
        n = int(sr * args.seconds)
        n_out = -((-n * L) // M)
        x = torch.from_numpy(rng.integers(-20000, 20000, size=(args.rows, n, 2), dtype=np.int16)).cuda()
        zeros, counts = [0] * args.rows, [n] * args.rows
        for _ in range(20):                       # warm-up: code object, tap table upload, clocks
            launch(x, zeros, counts, zeros, n_out, sr, 16000)
        torch.cuda.synchronize()
        per = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                launch(x, zeros, counts, zeros, n_out, sr, 16000)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        # one launch alone between two events: what a tick sees, launch latency included
        single = []
        for _ in range(20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch(x, zeros, counts, zeros, n_out, sr, 16000)
            e1.record()
            e1.synchronize()
            single.append(e0.elapsed_time(e1) * 1e3)
        r = {"sr_in": sr, "rows": args.rows, "seconds": args.seconds, "format": "s16 stereo", "taps_per_output": tpo, "n_out": n_out,
             "us_per_launch_back_to_back": {"min": round(min(per), 2), "median": round(float(np.median(per)), 2), "max": round(max(per), 2)},
             "us_single_launch_between_events": {"min": round(min(single), 2), "median": round(float(np.median(single)), 2),
                                                 "max": round(max(single), 2)},
             "iters": args.iters, "repeats": args.repeats}
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
