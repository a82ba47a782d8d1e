#!/usr/bin/env python3
"""Rate of the raw-IQ-to-audio chain on one GPU: u8 IQ at 2.4 Msps -> resampler to
96 kHz -> NFM -> 48 kHz audio (demod.Receiver), beside the front end alone
(demod.FrontEnd with the resampler: the path that existed before the
demodulator), in one process and alternating.

The raw samples sit in a device pool larger than the 256 MB Infinity Cache and
every call takes the next slice of it, so the input always comes from HBM.  A
call is one packet of --samples complex samples: the default (2^26, 28 s of
signal) makes a round long enough to time the kernels rather than the launches;
--samples 16384 shows the cost of feeding packets of the app's size one by one,
which is launch-bound.  Times are device events
around --calls calls on one stream, after --warmup untimed rounds; the figure
reported is the median of --repeats rounds, with the spread beside it.

Prints one JSON line and, with --out, writes the same object to a file.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAMPLE_RATE = 2_400_000


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--samples", type=int, default=1 << 26, help="complex samples per call (one packet)")
    p.add_argument("--pool-mb", type=int, default=512, help="raw pool in MiB (above the 256 MB Infinity Cache)")
    p.add_argument("--calls", type=int, default=512, help="calls per timed round")
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--mode", default="nfm")
    p.add_argument("--out", default="")
    args = p.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("demod_bench: no GPU visible (this measurement has no CPU fallback)")
    from rfanalyzer_amd import demod

    dev = torch.device("cuda", 0)
    S = args.samples
    slices = max(2, (args.pool_mb << 20) // (2 * S))
    pool = torch.randint(0, 256, (slices, 2 * S), dtype=torch.uint8, device=dev,
                         generator=torch.Generator(device=dev).manual_seed(1))
    stream = torch.cuda.Stream()
    rx = demod.Receiver("u8", SAMPLE_RATE, args.mode)
    rx.set_frequencies(100_000_000, 100_150_000)
    quad = rx.demod.quadrature_rate
    fe = demod.FrontEnd("u8", SAMPLE_RATE, quad, resampler=True)
    fe.set_frequencies(100_000_000, 100_150_000)
    cap = fe.max_outputs(S)
    o_re = torch.empty(cap, device=dev)
    o_im = torch.empty(cap, device=dev)
    rx.set_stream(stream.cuda_stream)
    fe.set_stream(stream.cuda_stream)
    torch.cuda.synchronize()
    pos = [0]
    counts = {}

    def front_alone():
        n = fe.process_device(pool[pos[0] % slices].data_ptr(), S, o_re.data_ptr(), o_im.data_ptr(), cap)
        pos[0] += 1
        counts["quadrature_samples_per_call"] = n

    def chain():
        n = rx.process_device(pool[pos[0] % slices].data_ptr(), S)
        pos[0] += 1
        counts["audio_samples_per_call"] = n

    def timed(fn):
        with torch.cuda.stream(stream):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3

    for _ in range(args.warmup):
        timed(front_alone)
        timed(chain)
    t_front, t_chain = [], []
    for _ in range(args.repeats):             # alternating, so drift hits both alike
        t_front.append(timed(front_alone))
        t_chain.append(timed(chain))
    work = args.calls * S

    def rate(ts):
        return work / statistics.median(ts) / 1e6

    res = {
        "bench": "demod_chain",
        "chain": f"u8 {SAMPLE_RATE} sps -> resampler {quad} -> {args.mode} -> {demod.AUDIO_RATE} audio",
        "samples_per_call": S, "calls_per_round": args.calls, "repeats": args.repeats,
        "pool_mib": slices * 2 * S >> 20,
        **counts,
        "front_end_msps": round(rate(t_front), 1),
        "chain_msps": round(rate(t_chain), 1),
        "chain_over_front_end": round(rate(t_chain) / rate(t_front), 4),
        "front_end_round_s_min_median_max": [round(min(t_front), 5), round(statistics.median(t_front), 5),
                                             round(max(t_front), 5)],
        "chain_round_s_min_median_max": [round(min(t_chain), 5), round(statistics.median(t_chain), 5),
                                         round(max(t_chain), 5)],
        "realtime_factor_chain": round(rate(t_chain) * 1e6 / SAMPLE_RATE, 1),
        "timing": "device events around the calls of a round on one stream",
    }
    rx.close()
    fe.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
