#!/usr/bin/env python3
"""Rate of K front-end channels on one raw IQ stream, in two forms that alternate in
one process: (a) K ``demod.FrontEnd`` handles called in turn on one stream, each fed
the same raw slice, and (b) one ``demod.FrontEndBank`` of K slots.

Inputs: u8 at 2.4 Msps -> 96 kHz through the Resampler and through the Decimator, and
s8 at 20 Msps -> 384 kHz through the Resampler; K in --channels; calls of --samples
complex samples (16 384 is the app's packet, launch-bound; 2^24 times the kernels).
The raw samples sit in a device pool larger than the 256 MB Infinity Cache and every
call takes the next slice, so the input comes from HBM.  Times are device events
around the calls of a round on one stream, after --warmup untimed rounds; reported is
the median of --repeats rounds with min and max beside it, in channel-samples per
second (input samples x channels), and bank / handles.

Prints one JSON line per cell and, with --out, writes all cells to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INPUTS = [("u8", 2_400_000, 96_000, True), ("u8", 2_400_000, 96_000, False), ("s8", 20_000_000, 384_000, True)]
CENTER = 100_000_000


def offsets(k, sample_rate):
    """K distinct channels spread over +-40 % of the band (none at 0)."""
    span = int(0.8 * sample_rate)
    return [-span // 2 + (2 * i + 1) * span // (2 * k) for i in range(k)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, nargs="+", default=[16_384, 1 << 24], help="complex samples per call")
    p.add_argument("--channels", type=int, nargs="+", default=[1, 8, 32])
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MB Infinity Cache)")
    p.add_argument("--round-samples", type=int, default=1 << 28,
                   help="input samples per timed round (calls = this / samples, between 4 and 256)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ddc_bank_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    pool = torch.randint(0, 256, (args.pool_mb << 20,), dtype=torch.uint8, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))
    stream = torch.cuda.Stream()
    cells = []
    for S in args.samples:
        slices = max(2, pool.numel() // (2 * S))
        calls = max(4, min(256, args.round_samples // S))
        for fmt, sr, out, resampler in INPUTS:
            for K in args.channels:
                chans = [CENTER + o for o in offsets(K, sr)]
                fes = [demod.FrontEnd(fmt, sr, out, resampler=resampler) for _ in range(K)]
                bank = demod.FrontEndBank(fmt, sr, out, K, resampler=resampler)
                bank.set_frequencies(CENTER, chans)
                bank.set_stream(stream.cuda_stream)
                for fe, ch in zip(fes, chans):
                    fe.set_frequencies(CENTER, ch)
                    fe.set_stream(stream.cuda_stream)
                cap = bank.max_outputs(S)
                o_re = torch.empty((K, cap), device=dev)
                o_im = torch.empty((K, cap), device=dev)
                torch.cuda.synchronize()
                pos = [0]

                def raw_ptr():
                    ptr = pool.data_ptr() + (pos[0] % slices) * 2 * S
                    pos[0] += 1
                    return ptr

                def handles():
                    ptr = raw_ptr()
                    for k, fe in enumerate(fes):
                        fe.process_device(ptr, S, o_re[k].data_ptr(), o_im[k].data_ptr(), cap)

                def banked():
                    bank.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)

                def timed(fn):
                    with torch.cuda.stream(stream):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(calls):
                            fn()
                        b.record()
                    b.synchronize()
                    return a.elapsed_time(b) * 1e-3

                for _ in range(args.warmup):
                    timed(handles)
                    timed(banked)
                t_h, t_b = [], []
                for _ in range(args.repeats):          # alternating, so drift hits both alike
                    t_h.append(timed(handles))
                    t_b.append(timed(banked))
                work = calls * S * K

                def rate(ts):
                    return work / statistics.median(ts) / 1e6

                def mmm(ts):
                    return [round(min(ts), 6), round(statistics.median(ts), 6), round(max(ts), 6)]

                cell = {
                    "input": f"{fmt} {sr} sps -> {'resampler' if resampler else 'decimator'} {out}",
                    "channels": K, "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats,
                    "ratio": bank.ratio(),
                    "handles_channel_msps": round(rate(t_h), 1),
                    "bank_channel_msps": round(rate(t_b), 1),
                    "bank_over_handles": round(rate(t_b) / rate(t_h), 4),
                    "handles_round_s_min_median_max": mmm(t_h),
                    "bank_round_s_min_median_max": mmm(t_b),
                    "handles_spread": round((max(t_h) - min(t_h)) / statistics.median(t_h), 4),
                    "bank_spread": round((max(t_b) - min(t_b)) / statistics.median(t_b), 4),
                }
                print(json.dumps(cell), flush=True)
                cells.append(cell)
                bank.close()
                for fe in fes:
                    fe.close()
    res = {"bench": "ddc_bank", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats",
           "forms": {"handles": "K demod.FrontEnd handles in turn on one stream (2 K launches per call)",
                     "bank": "one demod.FrontEndBank of K slots (2 launches per call)"},
           "cells": cells}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
