#!/usr/bin/env python3
"""Cost of the per-frame window statistics (rfa_set_windows) on the flagship step: config 3,
500 frames of 64 K s8 IQ per call, ring 500, EMA and peak-hold on, the raw frames in a device
pool larger than the 256 MB Infinity Cache.

For each window list the step is timed with and without the list, alternating in one process
(boxes differ by several percent), with device events around --calls calls on one stream; the
added time per step is the difference of the round medians.  The yardstick is the state pass
(peak-hold + EMA), which reads the same rows once: its time is taken the same way, as the
difference between the step of this engine and of one with peak-hold and EMA off.  The form the
kernel replaces -- a (window, frame) grid of the one-workgroup-per-window reduction -- is timed
alone by tools/window_grid_bench for the 1 600-window list.

Window lists: one whole-row window; 30 IEM channel windows (+-max(5, 100 kHz / resolution)
bins); a +-2-bin scan grid of 1 600 and of 4 000 windows (scanner.scan_windows).

Prints one JSON line and, with --out, writes the same object to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, FRAMES, F0, SR = 65536, 500, 433_920_000, 20_000_000


def window_lists():
    import numpy as np
    from rfanalyzer_amd import scanner as sc

    def grid(count):
        step = SR // count
        _, lo, hi = sc.scan_windows(F0, SR, N, SR, step, 0, 10 ** 12)
        return lo[:count], hi[:count]

    _, ilo, ihi = sc.iem_windows(F0, SR, N, [F0 - 9_000_000 + k * 600_000 for k in range(30)])
    return [("whole_row", (np.array([0], np.int32), np.array([N - 1], np.int32))),
            ("iem_30", (ilo, ihi)),
            ("scan_grid_1600", grid(1600)),
            ("scan_grid_4000", grid(4000))]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MB Infinity Cache)")
    p.add_argument("--calls", type=int, default=40, help="steps per timed round")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("window_stats_bench: no GPU visible (this measurement has no CPU fallback)")
    import rfanalyzer_amd as rfa

    dev = torch.device("cuda", 0)
    step_bytes = FRAMES * 2 * N
    slices = max(2, (args.pool_mb << 20) // step_bytes)
    pool = torch.randint(-128, 128, (slices, step_bytes), dtype=torch.int8, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))
    stream = torch.cuda.Stream()
    eng = rfa.SpectrumEngine(N, "blackman", "s8", avg="ema", ema_alpha=0.1, peak_hold=True, ring_rows=FRAMES)
    bare = rfa.SpectrumEngine(N, "blackman", "s8", ring_rows=FRAMES)  # the same step without the state pass
    for e in (eng, bare):
        e.set_stream(stream.cuda_stream)
        e.set_tuning(F0, SR)
    torch.cuda.synchronize()
    pos = [0]

    def timed(e):
        with torch.cuda.stream(stream):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                e.process_device(pool[pos[0] % slices].data_ptr(), FRAMES, 0, None)
                pos[0] += 1
            b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / args.calls  # us per step

    def med3(ts):
        return [round(min(ts), 2), round(statistics.median(ts), 2), round(max(ts), 2)]

    entries = []
    for name, (lo, hi) in window_lists():
        t_off, t_on, t_bare = [], [], []
        for r in range(args.warmup + args.repeats):  # alternating, so drift hits all alike
            eng.set_windows([], [])
            off = timed(eng)
            eng.set_windows(lo, hi)
            on = timed(eng)
            pk, av = eng.window_stats()
            assert pk.shape == (FRAMES, lo.size) and av.shape == pk.shape
            br = timed(bare)
            if r >= args.warmup:
                t_off.append(off), t_on.append(on), t_bare.append(br)
        added = statistics.median(t_on) - statistics.median(t_off)
        state = statistics.median(t_off) - statistics.median(t_bare)
        covered = int((hi.astype("int64") - lo + 1).sum())
        entries.append({
            "windows": name, "count": int(lo.size), "bins_covered": covered,
            "step_us_without_min_median_max": med3(t_off), "step_us_with_min_median_max": med3(t_on),
            "step_us_no_state_pass_min_median_max": med3(t_bare),
            "added_us_per_step": round(added, 2), "state_pass_us_per_step": round(state, 2),
            "added_over_state_pass": round(added / state, 3) if state > 0 else None,
        })
    res = {
        "bench": "window_stats",
        "workload": f"config 3: {FRAMES} x {N} s8 per step, ring {FRAMES}, EMA + peak-hold, pool {slices * step_bytes >> 20} MiB",
        "calls_per_round": args.calls, "repeats": args.repeats,
        "timing": "device events around the steps of a round on one stream; added = median with - median without; "
                  "state pass = median without - median of the same step with peak-hold and EMA off",
        "lists": entries,
    }
    grid_tool = os.path.join(ROOT, "tools", "window_grid_bench")
    if os.path.exists(grid_tool):
        out = subprocess.run([grid_tool, str(N), str(FRAMES), "1600"], capture_output=True, text=True, check=True).stdout
        res["window_frame_grid_of_row_window_kernel"] = json.loads(out.strip().splitlines()[-1])
    eng.close()
    bare.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
