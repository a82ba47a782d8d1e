#!/usr/bin/env python3
"""Rate of the polyphase channelizer against the front-end channel bank on the same raster,
candidates alternating in one process.

Case: u8 at 2.4 Msps, 25 kHz raster (M = 96 channels), 96 kHz out (D = 25), the
``Channelizer.for_raster`` prototype.  Candidates:

* ``chan32`` / ``chan96``: ``demod.Channelizer`` with 32 channels selected and with all 96;
* ``bank32``: ``demod.FrontEndBank(resampler=True)`` with the same 32 raster channels;
* ``raster_rx32`` / ``bank_rx32``: ``demod.RasterReceiverBank`` and ``demod.ReceiverBank``,
  32 NFM channels, raw bytes to audio.

Calls of --samples complex samples (16 384 is the app's packet, launch-bound; 2^24 times the
kernels).  The raw samples sit in a device pool larger than the 256 MiB Infinity Cache and
every call takes the next slice.  Times are device events around the calls of a round on one
stream, after --warmup untimed rounds of every candidate; reported is the median of --repeats
rounds in raw Gsamples/s (input samples) and Gchannel-samples/s (input samples x channels).

Prints one JSON line per cell and writes all cells to --out.

``--rational`` measures the rational-rate channelizer instead and writes
``profiles/channelizer/bench_rational.json``: s8 at 20 Msps, 25 kHz raster (M = 800), 96 kHz out
(L / D = 3 / 625), the ``Channelizer.for_raster_resampled`` prototype.  Candidates, same protocol:

* ``rat32`` / ``rat800``: the rational ``Channelizer`` with 32 channels selected and with all 800;
* ``bank32``: ``demod.FrontEndBank(resampler=True)`` with the same 32 raster channels;
* ``int208_32``: the integer ``Channelizer`` with M = 800, D = 208 (96.2 kHz out) and the same
  design at the input rate (as many taps per output), 32 selected: the integer fold on this shape;
* ``rat1_208_32``: the rational entry with L = 1, D = 208 and those taps: the rational kernel
  with a one-row tap table.  ``rat32`` against it is what L = 3 phase rows cost, and it against
  ``int208_32`` what the rational fold's indexing costs;
* ``chan32``: the integer channelizer's 2.4 Msps u8 line of the default run, in the same process
  (the check that the integer path did not move).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FMT, FS, SPACING, QRATE, CENTER = "u8", 2_400_000, 25_000, 96_000, 100_000_000
RFMT, RFS = "s8", 20_000_000                                      # --rational: the HackRF rate


def timed(torch, stream, calls, fn):
    with torch.cuda.stream(stream):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3


def run_rational(args, torch, demod, dev, pool, stream):
    M, L, D = demod.Channelizer.raster_ratio(RFS, SPACING, QRATE)
    sel32 = [(k - 16) % M for k in range(32)]
    freqs32 = [CENTER + (k if k < M // 2 else k - M) * SPACING for k in sel32]
    M24 = FS // SPACING
    sel24 = [(k - 16) % M24 for k in range(32)]
    taps1 = demod.create_low_pass_taps(1, RFS, 0.375 * SPACING, 0.25 * SPACING, 60)
    cells = []
    for S in args.samples:
        slices = max(2, pool.numel() // (2 * S))
        calls = max(4, min(256, args.round_samples // S))
        rat32 = demod.Channelizer.for_raster_resampled(RFMT, RFS, SPACING, QRATE)
        rat32.set_channels(sel32)
        rat800 = demod.Channelizer.for_raster_resampled(RFMT, RFS, SPACING, QRATE)
        bank32 = demod.FrontEndBank(RFMT, RFS, QRATE, 32, resampler=True)
        bank32.set_frequencies(CENTER, freqs32)
        int208 = demod.Channelizer(RFMT, M, 208, taps1)
        int208.set_channels(sel32)
        rat1 = demod.Channelizer.rational(RFMT, M, 1, 208, taps1)
        rat1.set_channels(sel32)
        chan32 = demod.Channelizer.for_raster(FMT, FS, SPACING, QRATE)
        chan32.set_channels(sel24)
        handles = (rat32, rat800, bank32, int208, rat1, chan32)
        for h in handles:
            h.set_stream(stream.cuda_stream)
        cap = max(rat800.max_outputs(S) + 1, bank32.max_outputs(S), int208.max_outputs(S) + 1, rat1.max_outputs(S) + 1,
                  chan32.max_outputs(S) + 1)
        o_re = torch.empty((M, cap), device=dev)
        o_im = torch.empty((M, cap), device=dev)
        torch.cuda.synchronize()
        pos = [0]

        def raw_ptr():
            ptr = pool.data_ptr() + (pos[0] % slices) * 2 * S
            pos[0] += 1
            return ptr

        def call(h):
            return lambda: h.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)

        cands = {"rat32": (32, call(rat32)), "rat800": (M, call(rat800)), "bank32": (32, call(bank32)),
                 "int208_32": (32, call(int208)), "rat1_208_32": (32, call(rat1)), "chan32": (32, call(chan32))}
        for _ in range(args.warmup):
            for _, fn in cands.values():
                timed(torch, stream, calls, fn)
        times = {name: [] for name in cands}
        for _ in range(args.repeats):                  # alternating, so drift hits all alike
            for name, (_, fn) in cands.items():
                times[name].append(timed(torch, stream, calls, fn))
        raw = {name: calls * S / statistics.median(ts) / 1e9 for name, ts in times.items()}
        cell = {
            "input": f"{RFMT} {RFS} sps, raster {SPACING} Hz (M = {M}), out {QRATE} (L / D = {L} / {D}), "
                     f"{rat800.plan()['num_taps']} taps ({rat800.ratio[2]} per output), radices {rat800.plan()['radices']}; "
                     f"int208_32 / rat1_208_32: {taps1.size} taps, D = 208; chan32: {FMT} {FS} sps, M = {M24}, D = {FS // QRATE}",
            "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats,
            "raw_gsps": {n: round(v, 3) for n, v in raw.items()},
            "channel_gsps": {n: round(v * cands[n][0], 2) for n, v in raw.items()},
            "rat32_over_bank32": round(raw["rat32"] / raw["bank32"], 3),
            "rat800_over_rat32_raw": round(raw["rat800"] / raw["rat32"], 3),
            "rat32_over_rat1_208_32": round(raw["rat32"] / raw["rat1_208_32"], 3),
            "rat1_208_32_over_int208_32": round(raw["rat1_208_32"] / raw["int208_32"], 3),
            "round_s_min_median_max": {n: [round(min(ts), 6), round(statistics.median(ts), 6), round(max(ts), 6)]
                                       for n, ts in times.items()},
            "spread": {n: round((max(ts) - min(ts)) / statistics.median(ts), 4) for n, ts in times.items()},
        }
        print(json.dumps(cell), flush=True)
        cells.append(cell)
        for h in handles:
            h.close()
    return {"bench": "channelizer_rational", "pool_mib": pool.numel() >> 20,
            "timing": "device events around the calls of a round on one stream; median of the repeats",
            "candidates": {"rat32": "rational demod.Channelizer (for_raster_resampled), 32 of 800 channels selected",
                           "rat800": "rational demod.Channelizer, all 800 channels",
                           "bank32": "demod.FrontEndBank(resampler=True), the same 32 channels",
                           "int208_32": "integer demod.Channelizer, M = 800, D = 208, the input-rate design, 32 selected",
                           "rat1_208_32": "rational entry with L = 1, D = 208, the same taps, 32 selected",
                           "chan32": "integer demod.Channelizer.for_raster, u8 2.4 Msps, 32 of 96 selected "
                                     "(the line of bench.json)"},
            "cells": cells}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, nargs="+", default=[16_384, 1 << 24], help="complex samples per call")
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MiB Infinity Cache)")
    p.add_argument("--round-samples", type=int, default=1 << 28,
                   help="input samples per timed round (calls = this / samples, between 4 and 256)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default=None, help="default profiles/channelizer/bench.json (bench_rational.json)")
    p.add_argument("--rational", action="store_true", help="measure the rational-rate channelizer at 20 Msps")
    args = p.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "channelizer", "bench_rational.json" if args.rational else "bench.json")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pfb_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    pool = torch.randint(0, 256, (args.pool_mb << 20,), dtype=torch.uint8, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))
    stream = torch.cuda.Stream()
    if args.rational:
        res = run_rational(args, torch, demod, dev, pool, stream)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
        return
    M = FS // SPACING
    sel32 = [(k - 16) % M for k in range(32)]                     # offsets -16 ... +15 raster steps
    freqs32 = [CENTER + (k if k < M // 2 else k - M) * SPACING for k in sel32]
    cells = []
    for S in args.samples:
        slices = max(2, pool.numel() // (2 * S))
        calls = max(4, min(256, args.round_samples // S))
        chan32 = demod.Channelizer.for_raster(FMT, FS, SPACING, QRATE)
        chan32.set_channels(sel32)
        chan96 = demod.Channelizer.for_raster(FMT, FS, SPACING, QRATE)
        bank32 = demod.FrontEndBank(FMT, FS, QRATE, 32, resampler=True)
        bank32.set_frequencies(CENTER, freqs32)
        raster_rx = demod.RasterReceiverBank(FMT, FS, SPACING, ["nfm"] * 32, sel32)
        bank_rx = demod.ReceiverBank(FMT, FS, ["nfm"] * 32)
        bank_rx.set_frequencies(CENTER, freqs32)
        for h in (chan32, chan96, bank32, raster_rx, bank_rx):
            h.set_stream(stream.cuda_stream)
        cap = max(chan96.max_outputs(S) + 1, bank32.max_outputs(S))
        o_re = torch.empty((M, cap), device=dev)
        o_im = torch.empty((M, cap), device=dev)
        torch.cuda.synchronize()
        pos = [0]

        def raw_ptr():
            ptr = pool.data_ptr() + (pos[0] % slices) * 2 * S
            pos[0] += 1
            return ptr

        cands = {
            "chan32": (32, lambda: chan32.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)),
            "chan96": (96, lambda: chan96.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)),
            "bank32": (32, lambda: bank32.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)),
            "raster_rx32": (32, lambda: raster_rx.process_device(raw_ptr(), S)),
            "bank_rx32": (32, lambda: bank_rx.process_device(raw_ptr(), S)),
        }

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
            for _, fn in cands.values():
                timed(fn)
        times = {name: [] for name in cands}
        for _ in range(args.repeats):                  # alternating, so drift hits all alike
            for name, (_, fn) in cands.items():
                times[name].append(timed(fn))
        raw = {name: calls * S / statistics.median(ts) / 1e9 for name, ts in times.items()}
        cell = {
            "input": f"{FMT} {FS} sps, raster {SPACING} Hz (M = {M}), out {QRATE} (D = {FS // QRATE}), "
                     f"{chan96.plan()['num_taps']} taps, radices {chan96.plan()['radices']}",
            "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats,
            "raw_gsps": {n: round(v, 3) for n, v in raw.items()},
            "channel_gsps": {n: round(v * cands[n][0], 2) for n, v in raw.items()},
            "chan32_over_bank32": round(raw["chan32"] / raw["bank32"], 3),
            "chan96_over_chan32_raw": round(raw["chan96"] / raw["chan32"], 3),
            "raster_rx32_over_bank_rx32": round(raw["raster_rx32"] / raw["bank_rx32"], 3),
            "round_s_min_median_max": {n: [round(min(ts), 6), round(statistics.median(ts), 6), round(max(ts), 6)]
                                       for n, ts in times.items()},
            "spread": {n: round((max(ts) - min(ts)) / statistics.median(ts), 4) for n, ts in times.items()},
        }
        print(json.dumps(cell), flush=True)
        cells.append(cell)
        for h in (chan32, chan96, bank32, raster_rx, bank_rx):
            h.close()
    res = {"bench": "channelizer", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats",
           "candidates": {"chan32": "demod.Channelizer, 32 of 96 channels selected (2 launches per call)",
                          "chan96": "demod.Channelizer, all 96 channels (2 launches per call)",
                          "bank32": "demod.FrontEndBank(resampler=True), the same 32 channels (2 launches per call)",
                          "raster_rx32": "demod.RasterReceiverBank, 32 NFM channels (2 + 4 launches per call)",
                          "bank_rx32": "demod.ReceiverBank, 32 NFM channels (2 + 4 launches per call)"},
           "cells": cells}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
