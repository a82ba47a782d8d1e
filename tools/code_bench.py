#!/usr/bin/env python3
"""What the code meter costs in the bank chains, by the protocol of tools/squelch_bench.py and
tools/tone_bench.py: device events around the calls of a round, the candidates alternating in one
process on one stream, --warmup untimed rounds, the median of --repeats rounds with min and max beside
it, a raw pool above the 256 MB Infinity Cache of which every call takes the next slice.

Input: u8 at 2.4 Msps, 32 NFM slots on channels of the 25 kHz raster, Gaussian noise with carriers
on the channels of 8 of the 32 slots.  Chains: ``demod.TunedReceiverBank`` and ``demod.ReceiverBank``;
calls of --samples raw samples (16 384 is the app's packet; 2^24 times the kernels).  Candidates:

  none            code=None, squelch=None: what the chain enqueued before it had a code meter;
  code            code= on all 32 slots: per call the collect of the previous call's sub-cells, the rule,
                  one upload of the call's records, the meter's launch and a copy of the sub-cell sums;
  squelch_code    the same behind a squelch whose every slot is open.

Besides the device time of a round, the host's wall time inside the code meter's collect is recorded
per call.

The kernel alone: ``CodeMeterBank`` and ``ToneMeterBank`` on the same 32 x 335 544 float rows (what a
2^24-sample call leaves), alternating, device events around each call's enqueue (record upload, launch,
copy of the results), next to the memory floor of reading the rows once at the rate a device-to-device
copy of them reaches.

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
import time

FMT, RATE, SPACING, MODE, K = "u8", 2_400_000, 25_000, "nfm", 32
CENTER = 100_000_000
RASTER = [2 + 3 * i for i in range(K)]                        # 2 .. 95: neither 0 (the u8 offset) nor 48
OFFSETS = [(c if c < 48 else c - 96) * SPACING for c in RASTER]
CARRIER_SLOTS = list(range(0, K, 4))                          # 8 of 32
CARRIER, NOISE = 0.08, 0.02
THRESHOLD_OPEN = -60.0
CODE = "023"
KERNEL_ROW = 335_544


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
    p.add_argument("--none-only", action="store_true", help="only the candidate without squelch and meter")
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
        raise SystemExit("code_bench: no GPU visible (this measurement has no CPU fallback)")
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
        candidates["code"] = {"code": [CODE] * K}
        candidates["squelch_code"] = {"squelch": [THRESHOLD_OPEN] * K, "code": [CODE] * K}

    def make(chain, kw):
        if chain == "ReceiverBank":
            rx = demod.ReceiverBank(FMT, RATE, [MODE] * K, **kw)
        else:
            rx = demod.TunedReceiverBank(FMT, RATE, SPACING, [MODE] * K, **kw)
        rx.set_frequencies(CENTER, [CENTER + o for o in OFFSETS])
        if "squelch" in kw:
            rx.squelch_debounce = 1
        rx.set_stream(stream.cuda_stream)
        return rx

    def watch_collect(rx, waits):
        """Record the host's wall time inside every collect of the chain's code meter."""
        inner = rx.code_meter._call

        def call(name, *a):
            if name != "collect":
                return inner(name, *a)
            t0 = time.perf_counter()
            inner(name, *a)
            waits.append(time.perf_counter() - t0)
        rx.code_meter._call = call

    for S in args.samples:
        calls = max(4, min(256, args.round_samples // S))
        slices = max(2, n_pool // S)
        for chain in ("TunedReceiverBank", "ReceiverBank"):
            rxs = {name: make(chain, kw) for name, kw in candidates.items()}
            pos = {name: 0 for name in rxs}
            waits = {name: [] for name, kw in candidates.items() if "code" in kw}
            for name in waits:
                watch_collect(rxs[name], waits[name])

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
            for w in waits.values():
                w.clear()
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
                    "channel_msps": round(calls * S * K / med[name] / 1e6, 1),
                    "round_s_min_median_max": [round(min(ts), 6), round(med[name], 6), round(max(ts), 6)],
                    "spread": round((max(ts) - min(ts)) / med[name], 4),
                    "over_none": round(med[name] / med["none"], 4),
                }
                if name in waits:
                    w = sorted(waits[name])
                    cell[name]["collect_host_us_median_p90_max"] = [round(w[len(w) // 2] * 1e6, 2),
                                                                   round(w[len(w) * 9 // 10] * 1e6, 2),
                                                                   round(w[-1] * 1e6, 2)]
                    assert not rxs[name].code_open.any()            # no slot carries the code
            print(json.dumps(cell), flush=True)
            cells.append(cell)
            for rx in rxs.values():
                rx.close()

    kernel = None
    if not args.none_only:
        # the kernel alone, next to the tone meter's on the same rows and the memory floor
        rows = 0.05 * torch.randn(K, KERNEL_ROW, device=dev, generator=gen, dtype=torch.float32)
        other = torch.empty_like(rows)
        counts = [KERNEL_ROW] * K
        code_meter, tone_meter = demod.CodeMeterBank(K), demod.ToneMeterBank(K)
        for k in range(K):
            tone_meter.set_probes(k, demod._tone_probes(100.0))
        code_meter.set_stream(stream.cuda_stream)
        tone_meter.set_stream(stream.cuda_stream)

        def one(enqueue, collect):
            with torch.cuda.stream(stream):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                enqueue()
                b.record()
            collect()
            b.synchronize()
            return a.elapsed_time(b) * 1e-3

        runs = {
            "code": lambda: one(lambda: code_meter.process_device(rows.data_ptr(), KERNEL_ROW, counts),
                                code_meter.collect),
            "tone": lambda: one(lambda: tone_meter.process_device(rows.data_ptr(), KERNEL_ROW, counts),
                                tone_meter.collect),
            "copy": lambda: one(lambda: other.copy_(rows), lambda: None),
        }
        per_round = 16
        for _ in range(args.warmup):
            for fn in runs.values():
                for _ in range(per_round):
                    fn()
        times = {name: [] for name in runs}
        for _ in range(args.repeats):
            for name, fn in runs.items():
                times[name].append(statistics.median(fn() for _ in range(per_round)))
        med = {name: statistics.median(ts) for name, ts in times.items()}
        nbytes = rows.numel() * 4
        copy_rate = 2 * nbytes / med["copy"]
        kernel = {"rows": f"{K} x {KERNEL_ROW} float32 ({nbytes >> 20} MiB), every slot's count the row",
                  "timing": "device events around one call's enqueue (record upload, launch(es), copy of the "
                            f"results); median of {per_round} calls per round, median of the rounds",
                  "copy_gb_s": round(copy_rate / 1e9, 1),
                  "read_once_floor_us": round(nbytes / copy_rate * 1e6, 2)}
        for name in ("code", "tone", "copy"):
            ts = times[name]
            kernel[name] = {"us_per_call": round(med[name] * 1e6, 2),
                            "us_min_median_max": [round(min(ts) * 1e6, 2), round(med[name] * 1e6, 2),
                                                  round(max(ts) * 1e6, 2)]}
        kernel["code"]["gsamples_s"] = round(rows.numel() / med["code"] / 1e9, 2)
        kernel["tone"]["gsamples_s"] = round(rows.numel() / med["tone"] / 1e9, 2)
        print(json.dumps({"kernel_alone": kernel}), flush=True)
        code_meter.close()
        tone_meter.close()
        del rows, other

    res = {"bench": "code", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats; "
                     "collect_host_us: the host's wall time inside the code meter's collect, per call",
           "candidates": {"none": "code=None, squelch=None",
                          "code": f"code={CODE} on all {K} slots",
                          "squelch_code": f"the same behind a squelch, thresholds {THRESHOLD_OPEN} dB (all {K} slots "
                                          "open), debounce 1"},
           "cells": cells}
    if kernel is not None:
        res["kernel_alone"] = kernel
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
