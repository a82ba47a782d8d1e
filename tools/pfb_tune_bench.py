#!/usr/bin/env python3
"""What the channelizer's fine tuning costs and what it buys, by the protocol of
tools/pfb_bench.py: device events around the calls of a round, the candidates alternating in one
process on one stream, --warmup untimed rounds, the median of --repeats rounds with min and max
beside it, a raw pool above the 256 MiB Infinity Cache of which every call takes the next slice.

Input: u8 at 2.4 Msps, 25 kHz raster (M = 96), 96 kHz out, 32 NFM slots at raster channels
-16 ... +15 plus 1 ... 12 kHz (alternating sign), calls of --samples raw samples (16 384 is the
app's packet, launch-bound; 2^24 times the kernels).  Candidates:

  chan_tuned / chan_untuned   the ``Channelizer.for_channels`` handle with those 32 slots, with the
                              offsets set and without: the cost of the fused rotation;
  tuned_rx32 / bank_rx32      ``TunedReceiverBank`` against ``ReceiverBank`` on the same 32
                              frequencies, raw bytes to audio;
  raster_rx32 / chan32        ``RasterReceiverBank`` and the untuned ``for_raster`` channelizer on the
                              32 raster channels: the lines of profiles/channelizer/bench.json.

``tuned_rx32`` against ``raster_rx32`` is what the shorter prototype gives (both are a channelizer
into the same demodulators), ``raster_rx32`` against ``bank_rx32`` what the channelizer gives.

With --parent-root DIR (a built checkout of the parent commit) ``raster_rx32`` and ``chan32`` are
also measured alone, with the package and library found in DIR and with this commit's, a fresh
process each, before and after this one's rounds: the check that a handle without a tuning did
not move.

Prints one JSON line per cell and writes all cells to --out.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

FMT, FS, SPACING, QRATE, CENTER, K = "u8", 2_400_000, 25_000, 96_000, 100_000_000, 32


def main():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, nargs="+", default=[16_384, 1 << 24], help="complex samples per call")
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MiB Infinity Cache)")
    p.add_argument("--round-samples", type=int, default=1 << 28,
                   help="input samples per timed round (calls = this / samples, between 4 and 256)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--package-root", default=here, help="where rfanalyzer_amd is imported from")
    p.add_argument("--untuned-only", action="store_true", help="only raster_rx32 and chan32 (what the parent commit has)")
    p.add_argument("--parent-root", default="", help="a built checkout of the parent commit to compare the untuned lines with")
    p.add_argument("--out", default=os.path.join(here, "profiles", "channelizer", "bench_tuned.json"))
    args = p.parse_args()

    def untuned_run(root):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "untuned.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", root, "--untuned-only",
                   "--out", out, "--pool-mb", str(args.pool_mb), "--round-samples", str(args.round_samples),
                   "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--samples", *map(str, args.samples)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
            with open(out) as f:
                return json.load(f)["cells"]

    def ab_run():                                                 # like for like: two candidates, a fresh process each
        return {"parent": untuned_run(args.parent_root), "this": untuned_run(args.package_root)}

    ab = [ab_run()] if args.parent_root else []                   # before this process opens the device

    sys.path.insert(0, args.package_root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pfb_tune_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    pool = torch.randint(0, 256, (args.pool_mb << 20,), dtype=torch.uint8, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))
    stream = torch.cuda.Stream()
    M = FS // SPACING
    sel32 = [(k - 16) % M for k in range(K)]                      # offsets -16 ... +15 raster steps
    raster32 = [CENTER + (k if k < M // 2 else k - M) * SPACING for k in sel32]
    deltas = [(1 + j % 12) * 1000 * (1 if j % 2 == 0 else -1) for j in range(K)]
    freqs32 = [f + d for f, d in zip(raster32, deltas)]
    cells = []
    for S in args.samples:
        slices = max(2, pool.numel() // (2 * S))
        calls = max(4, min(256, args.round_samples // S))
        handles, cands, info = [], {}, {}
        cap = S // (FS // QRATE) + 2
        o_re = torch.empty((M, cap), device=dev)
        o_im = torch.empty((M, cap), device=dev)
        pos = [0]

        def raw_ptr():
            ptr = pool.data_ptr() + (pos[0] % slices) * 2 * S
            pos[0] += 1
            return ptr

        def front(h):
            handles.append(h)
            return lambda: h.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)

        def chain(h):
            handles.append(h)
            return lambda: h.process_device(raw_ptr(), S)

        if not args.untuned_only:
            tuned_rx = demod.TunedReceiverBank(FMT, FS, SPACING, ["nfm"] * K)
            tuned_rx.set_frequencies(CENTER, freqs32)
            assert tuned_rx.channels == sel32 and tuned_rx.offsets == deltas
            chan_tuned = demod.Channelizer.for_channels(FMT, FS, SPACING, QRATE, tuned_rx.passband_hz)
            chan_tuned.set_channels(sel32)
            chan_tuned.set_offsets(deltas, QRATE)
            chan_untuned = demod.Channelizer.for_channels(FMT, FS, SPACING, QRATE, tuned_rx.passband_hz)
            chan_untuned.set_channels(sel32)
            bank_rx = demod.ReceiverBank(FMT, FS, ["nfm"] * K)
            bank_rx.set_frequencies(CENTER, freqs32)
            cands.update({"chan_tuned": front(chan_tuned), "chan_untuned": front(chan_untuned),
                          "tuned_rx32": chain(tuned_rx), "bank_rx32": chain(bank_rx)})
            info = {"passband_hz": tuned_rx.passband_hz, "for_channels_taps": chan_tuned.plan()["num_taps"],
                    "tuning_q": chan_tuned.tuning[0]}
        raster_rx = demod.RasterReceiverBank(FMT, FS, SPACING, ["nfm"] * K, sel32)
        chan32 = demod.Channelizer.for_raster(FMT, FS, SPACING, QRATE)
        chan32.set_channels(sel32)
        cands.update({"raster_rx32": chain(raster_rx), "chan32": front(chan32)})
        info["for_raster_taps"] = chan32.plan()["num_taps"]
        for h in handles:
            h.set_stream(stream.cuda_stream)
        torch.cuda.synchronize()

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
            for fn in cands.values():
                timed(fn)
        times = {name: [] for name in cands}
        for _ in range(args.repeats):                  # alternating, so drift hits all alike
            for name, fn in cands.items():
                times[name].append(timed(fn))
        raw = {name: calls * S / statistics.median(ts) / 1e9 for name, ts in times.items()}
        cell = {
            "input": f"{FMT} {FS} sps, raster {SPACING} Hz (M = {M}), out {QRATE} (D = {FS // QRATE}), {K} NFM slots "
                     f"1 ... 12 kHz off the raster",
            **info,
            "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats,
            "raw_gsps": {n: round(v, 3) for n, v in raw.items()},
            "round_s_min_median_max": {n: [round(min(ts), 6), round(statistics.median(ts), 6), round(max(ts), 6)]
                                       for n, ts in times.items()},
            "spread": {n: round((max(ts) - min(ts)) / statistics.median(ts), 4) for n, ts in times.items()},
        }
        if not args.untuned_only:
            cell.update({"chan_tuned_over_chan_untuned": round(raw["chan_tuned"] / raw["chan_untuned"], 3),
                         "tuned_rx32_over_bank_rx32": round(raw["tuned_rx32"] / raw["bank_rx32"], 3),
                         "tuned_rx32_over_raster_rx32": round(raw["tuned_rx32"] / raw["raster_rx32"], 3),
                         "raster_rx32_over_bank_rx32": round(raw["raster_rx32"] / raw["bank_rx32"], 3)})
        print(json.dumps(cell), flush=True)
        cells.append(cell)
        for h in handles:
            h.close()
    res = {"bench": "channelizer_tuned", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats",
           "candidates": {"chan_tuned": "Channelizer.for_channels, 32 of 96 slots, offsets set (2 launches per call)",
                          "chan_untuned": "the same handle design and selection without a tuning",
                          "tuned_rx32": "TunedReceiverBank, 32 NFM channels off the raster (2 + 4 launches per call)",
                          "bank_rx32": "ReceiverBank on the same 32 frequencies (2 + 4 launches per call)",
                          "raster_rx32": "RasterReceiverBank on the 32 raster channels (2 + 4 launches per call)",
                          "chan32": "Channelizer.for_raster, 32 of 96 selected, no tuning"},
           "cells": cells}
    if args.parent_root:
        del pool, o_re, o_im
        torch.cuda.empty_cache()
        ab.append(ab_run())
        res["untuned_ab"] = {
            "what": "raster_rx32 and chan32 alone (--untuned-only) with the parent commit's package and library and "
                    "with this commit's, a fresh process each, in the order parent, this before and parent, this after "
                    "the rounds above; this_over_parent is the ratio of the rates from the mean of the two medians",
            "before": ab[0], "after": ab[1], "this_over_parent": []}
        for i, cell in enumerate(cells):
            med = lambda who, name: statistics.mean(r[who][i]["round_s_min_median_max"][name][1] for r in ab)  # noqa: E731
            res["untuned_ab"]["this_over_parent"].append(
                {"samples_per_call": cell["samples_per_call"],
                 **{name: round(med("parent", name) / med("this", name), 4) for name in ("raster_rx32", "chan32")}})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
