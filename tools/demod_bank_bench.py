#!/usr/bin/env python3
"""Rate of K demodulated channels, handles in turn against the demodulator bank, in two
comparisons that alternate their forms in one process and on one stream:

(a) "demod": K ``demod.Demodulator`` handles called in turn (4 K launches per call) against
    one ``demod.DemodulatorBank`` of K slots (4 launches and one copy of K records), on
    device-resident quadrature IQ, every slot with its own samples;
(b) "chain": a ``demod.FrontEndBank`` followed by K ``demod.Demodulator`` handles in turn
    (2 + 4 K launches per packet -- what ``demod.ReceiverBank`` enqueued before the
    demodulators were banked, built here from the public classes) against
    ``demod.ReceiverBank`` (2 + 4 launches and the record copy).

Input: u8 at 2.4 Msps, NFM slots (96 kHz quadrature rate, so a call of S raw samples is
S / 25 quadrature samples); K in --channels; calls of --samples raw samples (16 384 is the
app's packet, launch-bound; 2^24 times the kernels).  The raw samples of (b) sit in a device
pool larger than the 256 MB Infinity Cache and every call takes the next slice; the quadrature
samples of (a) come from a float pool of the same size.  Times are device events around the
calls of a round on one stream, after --warmup untimed rounds; reported is the median of
--repeats rounds with min and max beside it, in channel-samples per second (raw input samples
x channels; for (a) the raw samples its quadrature samples stand for), and bank / handles.

Prints one JSON line per cell and, with --out, writes all cells to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FMT, RATE, MODE = "u8", 2_400_000, "nfm"
CENTER = 100_000_000


def offsets(k):
    """K distinct channels spread over +-40 % of the band (none at 0)."""
    span = int(0.8 * RATE)
    return [-span // 2 + (2 * i + 1) * span // (2 * k) for i in range(k)]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, nargs="+", default=[16_384, 1 << 24], help="raw complex samples per call")
    p.add_argument("--channels", type=int, nargs="+", default=[1, 8, 32])
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MB Infinity Cache)")
    p.add_argument("--round-samples", type=int, default=1 << 26,
                   help="raw samples per timed round (calls = this / samples, between 4 and 256)")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("demod_bank_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(1)
    pool = torch.randint(0, 256, (args.pool_mb << 20,), dtype=torch.uint8, device=dev, generator=gen)
    qfloats = (args.pool_mb << 20) // 8                      # re and im pools of pool_mb / 2 each
    q_re = 0.3 * torch.randn(qfloats, device=dev, generator=gen)
    q_im = 0.3 * torch.randn(qfloats, device=dev, generator=gen)
    qrate = demod.mode_info(MODE)[0]
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

    def measure(what, S, K, calls, handles, banked, launches):
        for _ in range(args.warmup):
            timed(handles, calls)
            timed(banked, calls)
        t_h, t_b = [], []
        for _ in range(args.repeats):                        # alternating, so drift hits both alike
            t_h.append(timed(handles, calls))
            t_b.append(timed(banked, calls))
        work = calls * S * K

        def rate(ts):
            return work / statistics.median(ts) / 1e6

        def mmm(ts):
            return [round(min(ts), 6), round(statistics.median(ts), 6), round(max(ts), 6)]

        cell = {
            "comparison": what, "input": f"{FMT} {RATE} sps, {MODE} slots ({qrate} Hz quadrature rate)",
            "channels": K, "samples_per_call": S, "calls_per_round": calls, "repeats": args.repeats,
            "launches_per_call_handles": launches[0], "launches_per_call_bank": launches[1],
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

    for S in args.samples:
        calls = max(4, min(256, args.round_samples // S))
        nq = S * qrate // RATE
        for K in args.channels:
            # ---- (a) the demodulators alone, on quadrature samples
            hs = [demod.Demodulator(MODE) for _ in range(K)]
            bank = demod.DemodulatorBank([MODE] * K)
            bank.set_stream(stream.cuda_stream)
            for h in hs:
                h.set_stream(stream.cuda_stream)
            audio = torch.empty((K, nq), device=dev)
            qslices = max(1, qfloats // (K * nq))
            pos = [0]

            def q_off():
                off = 4 * (pos[0] % qslices) * K * nq
                pos[0] += 1
                return off

            def demod_handles():
                off = q_off()
                for k, h in enumerate(hs):
                    h.process_device(q_re.data_ptr() + off + 4 * k * nq, q_im.data_ptr() + off + 4 * k * nq, nq,
                                     audio[k].data_ptr(), nq)

            def demod_bank():
                off = q_off()
                bank.process_device(q_re.data_ptr() + off, q_im.data_ptr() + off, nq, nq, audio.data_ptr(), nq)

            torch.cuda.synchronize()
            measure("demod", S, K, calls, demod_handles, demod_bank, (4 * K, 4))
            bank.close()

            # ---- (b) the chain from raw bytes
            chans = [CENTER + o for o in offsets(K)]
            front = demod.FrontEndBank(FMT, RATE, qrate, K, resampler=True)
            front.set_frequencies(CENTER, chans)
            front.set_stream(stream.cuda_stream)
            rxb = demod.ReceiverBank(FMT, RATE, [MODE] * K)
            rxb.set_frequencies(CENTER, chans)
            rxb.set_stream(stream.cuda_stream)
            cap = front.max_outputs(S)
            o_re = torch.empty((K, cap), device=dev)
            o_im = torch.empty((K, cap), device=dev)
            o_au = torch.empty((K, cap), device=dev)
            slices = max(2, pool.numel() // (2 * S))
            rpos = [0]

            def raw_ptr():
                ptr = pool.data_ptr() + (rpos[0] % slices) * 2 * S
                rpos[0] += 1
                return ptr

            def chain_handles():
                got = front.process_device(raw_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)
                for k, h in enumerate(hs):
                    h.process_device(o_re[k].data_ptr(), o_im[k].data_ptr(), got, o_au[k].data_ptr(), cap)

            def chain_bank():
                rxb.process_device(raw_ptr(), S)

            torch.cuda.synchronize()
            measure("chain", S, K, calls, chain_handles, chain_bank, (2 + 4 * K, 2 + 4))
            rxb.close()
            front.close()
            for h in hs:
                h.close()
    res = {"bench": "demod_bank", "pool_mib": pool.numel() >> 20,
           "timing": "device events around the calls of a round on one stream; median of the repeats",
           "forms": {"demod/handles": "K demod.Demodulator handles in turn on one stream (4 K launches per call)",
                     "demod/bank": "one demod.DemodulatorBank of K slots (4 launches and one record copy per call)",
                     "chain/handles": "demod.FrontEndBank, then K demod.Demodulator handles in turn "
                                      "(2 + 4 K launches per packet)",
                     "chain/bank": "demod.ReceiverBank (2 + 4 launches and one record copy per packet)"},
           "cells": cells}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
