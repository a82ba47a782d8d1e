#!/usr/bin/env python3
"""What the audio IIR bank costs in the bank chains and alone, by the protocol of tools/audio_fir_bench.py
(DESIGN 5.7m): device events around the calls of a round, the candidates alternating in one process on
one stream, --warmup untimed rounds, the median of --repeats rounds with min and max beside it, a raw
pool above the 256 MB Infinity Cache of which every call takes the next slice.

Input: u8 at 2.4 Msps, 32 NFM slots on channels of the 25 kHz raster, Gaussian noise with carriers
on the channels of 8 of the 32 slots.  Chains: ``demod.TunedReceiverBank`` and ``demod.ReceiverBank``;
calls of --samples raw samples (16 384 is the app's packet; 2^24 times the kernels).  Candidates:

  none             no audio stage behind the demodulators;
  iir_voice        audio_iir="voice" on all 32 slots: the 8th-order Chebyshev II tone strip, 4 sections;
  fir_voice        audio_filter="voice" on all 32 slots: the 1309-tap FIR tone strip, in the same process;
  iir_voice_deemph audio_iir="voice+deemphasis" on all 32 slots: 5 sections;
  iir_pass_through audio_iir=[None] * 32: the same launch, every slot a bitwise copy.

The IIR kernel alone is timed on the rows of the large call (32 rows of samples * 48000 / 2400000
floats) with 1, 4 and 5 sections, next to a device copy of the same rows: a floor that reads every
sample once and writes it once.

With --parent-root DIR the ``none`` candidate is also measured with the package and library found in
DIR (a checkout of the parent commit, built), in a fresh process before and after this one's rounds.

Prints one JSON line per cell and, with --out, writes all cells to a file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

FMT, RATE, SPACING, MODE, K = "u8", 2_400_000, 25_000, "nfm", 32
CENTER = 100_000_000
RASTER = [2 + 3 * i for i in range(K)]                        # 2 .. 95: neither 0 (the u8 offset) nor 48
OFFSETS = [(c if c < 48 else c - 96) * SPACING for c in RASTER]
CARRIER_SLOTS = list(range(0, K, 4))                          # 8 of 32
CARRIER, NOISE = 0.08, 0.02
AUDIO_RATE = 48000


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, nargs="+", default=[16_384, 1 << 24], help="raw complex samples per call")
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MB Infinity Cache)")
    p.add_argument("--round-samples", type=int, default=1 << 26,
                   help="raw samples per timed round (calls = this / samples, between 4 and 256)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--package-root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                   help="where rfanalyzer_amd is imported from")
    p.add_argument("--none-only", action="store_true", help="only the candidate without an audio stage")
    p.add_argument("--parent-root", default="", help="a built checkout of the parent commit to compare `none` with")
    p.add_argument("--out", default="")
    args = p.parse_args()

    def parent_run():
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "parent.json")
            cmd = [sys.executable, os.path.abspath(__file__), "--package-root", args.parent_root, "--none-only",
                   "--out", out, "--pool-mb", str(args.pool_mb), "--round-samples", str(args.round_samples),
                   "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--samples", *map(str, args.samples)]
            subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=900)
            with open(out) as f:
                return json.load(f)["cells"]

    parent_cells = [parent_run()] if args.parent_root else []     # before this process opens the device

    sys.path.insert(0, args.package_root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("audio_iir_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    n_pool = (args.pool_mb << 20) // 2                           # complex samples of the pool
    pool = torch.empty(2 * n_pool, dtype=torch.uint8, device=dev)
    chunk = 1 << 22
    for s in range(0, n_pool, chunk):
        n = min(chunk, n_pool - s)
        t = torch.arange(s, s + n, device=dev, dtype=torch.float64)
        re = NOISE * torch.randn(n, device=dev, generator=gen, dtype=torch.float32)
        im = NOISE * torch.randn(n, device=dev, generator=gen, dtype=torch.float32)
        for k in CARRIER_SLOTS:
            ph = (2 * torch.pi * ((OFFSETS[k] * t) % RATE) / RATE).to(torch.float32)   # exact phase, then fp32
            re += CARRIER * torch.cos(ph)
            im += CARRIER * torch.sin(ph)
        iq = torch.stack((re, im), dim=1).reshape(-1)
        pool[2 * s:2 * (s + n)] = torch.clamp(torch.round(iq * 128 + 127.4), 0, 255).to(torch.uint8)
    del t, re, im, iq, ph
    stream = torch.cuda.Stream()
    cells = []

    def timed(fn, calls):
        with torch.cuda.stream(stream):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    candidates = {"none": {}}
    if not args.none_only:
        candidates["iir_voice"] = {"audio_iir": ["voice"] * K}
        candidates["fir_voice"] = {"audio_filter": ["voice"] * K}
        candidates["iir_voice_deemph"] = {"audio_iir": ["voice+deemphasis"] * K}
        candidates["iir_pass_through"] = {"audio_iir": [None] * K}

    def make(chain, kw):
        if chain == "ReceiverBank":
            rx = demod.ReceiverBank(FMT, RATE, [MODE] * K, **kw)
        else:
            rx = demod.TunedReceiverBank(FMT, RATE, SPACING, [MODE] * K, **kw)
        rx.set_frequencies(CENTER, [CENTER + o for o in OFFSETS])
        rx.set_stream(stream.cuda_stream)
        return rx

    for S in args.samples:
        calls = max(4, min(256, args.round_samples // S))
        slices = max(2, n_pool // S)
        for chain in ("TunedReceiverBank", "ReceiverBank"):
            rxs = {name: make(chain, kw) for name, kw in candidates.items()}
            pos = {name: 0 for name in rxs}

            def call(name):
                rx = rxs[name]

                def fn():
                    rx.process_device(pool.data_ptr() + (pos[name] % slices) * 2 * S, S)
                    pos[name] += 1
                return fn

            fns = {name: call(name) for name in rxs}
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                for fn in fns.values():
                    timed(fn, calls)
            times = {name: [] for name in rxs}
            for _ in range(args.repeats):                          # alternating, so drift hits all alike
                for name, fn in fns.items():
                    times[name].append(timed(fn, calls))
            med = {name: statistics.median(ts) for name, ts in times.items()}
            cell = {"chain": chain, "input": f"{FMT} {RATE} sps, {K} {MODE} slots, carriers on {len(CARRIER_SLOTS)}",
                    "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats}
            for name, ts in times.items():
                cell[name] = {
                    "us_per_call": round(med[name] / calls * 1e6, 2),
                    "us_per_call_min_max": [round(min(ts) / calls * 1e6, 2), round(max(ts) / calls * 1e6, 2)],
                    "added_us_per_call": round((med[name] - med["none"]) / calls * 1e6, 2),
                    "channel_msps": round(calls * S * K / med[name] / 1e6, 1),
                    "round_s_min_median_max": [round(min(ts), 6), round(med[name], 6), round(max(ts), 6)],
                    "spread": round((max(ts) - min(ts)) / med[name], 4),
                    "over_none": round(med[name] / med["none"], 4),
                }
            if not args.none_only:
                cell["iir_voice_adds_less_than_fir_voice"] = bool(med["iir_voice"] < med["fir_voice"])
            print(json.dumps(cell), flush=True)
            cells.append(cell)
            for rx in rxs.values():
                rx.close()
    kernel_cells = []
    if not args.none_only:
        n = max(args.samples) * AUDIO_RATE // RATE
        rows = 0.3 * torch.randn(K, n, device=dev, generator=gen, dtype=torch.float32)
        out = torch.empty_like(rows)

        def measure(fn):
            torch.cuda.synchronize()
            for _ in range(args.warmup):
                timed(fn, 4)
            ts = [timed(fn, 4) / 4 for _ in range(args.repeats)]
            return [round(min(ts) * 1e6, 1), round(statistics.median(ts) * 1e6, 1), round(max(ts) * 1e6, 1)]

        floor = measure(lambda: out.copy_(rows))
        cell = {"kernel": "device copy of the rows", "slots": K, "samples_per_slot": n, "bytes_moved": 8 * K * n,
                "us_per_call_min_median_max": floor}
        print(json.dumps(cell), flush=True)
        kernel_cells.append(cell)
        for what, sec in (("deemphasis", demod.deemphasis_sections()), ("voice", demod.tone_strip_sections()),
                          ("voice+deemphasis", demod._audio_iir_sections("voice+deemphasis")), ("pass_through", None)):
            iir = demod.AudioIirBank(K)
            for k in range(K):
                iir.set_sections(k, sec)
            iir.set_stream(stream.cuda_stream)
            counts = iir._count_array([n] * K)
            ts = measure(lambda: iir.process_device(rows.data_ptr(), n, counts, out.data_ptr(), n))
            S = 0 if sec is None else int(sec.shape[0])
            cell = {"kernel": "audio_iir_kernel", "slots": K, "samples_per_slot": n, "what": what, "sections": S,
                    "plan": iir.plan(S, n), "us_per_call_min_median_max": ts,
                    "over_copy_floor": round(ts[1] / floor[1], 2)}
            print(json.dumps(cell), flush=True)
            kernel_cells.append(cell)
            iir.close()
        del rows, out
    res = {"bench": "audio_iir", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats",
           "candidates": {"none": "no audio stage behind the demodulators",
                          "iir_voice": f"audio_iir='voice' on all {K} slots (4 sections)",
                          "fir_voice": f"audio_filter='voice' on all {K} slots (1309 taps)",
                          "iir_voice_deemph": f"audio_iir='voice+deemphasis' on all {K} slots (5 sections)",
                          "iir_pass_through": f"audio_iir=[None] * {K}"},
           "cells": cells, "kernel": kernel_cells}
    if args.parent_root:
        del pool
        torch.cuda.empty_cache()
        parent_cells.append(parent_run())
        res["parent_commit_none"] = {
            "what": "the `none` candidate with the parent commit's package and library, a fresh process before and "
                    "one after this process's rounds",
            "before": parent_cells[0], "after": parent_cells[1]}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
