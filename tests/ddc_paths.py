"""The case table of the front-end FIR tile's paths (rfanalyzer_amd/csrc/ddc_fir_tile.inc),
shared by tests/test_ddc_paths_host.py (CPU: plans, packets, the oracle against the literal
loops) and tests/test_gpu_ddc_paths.py (GPU: every case bit for bit against the oracle).

A row is a filter (T taps, decimation D) that exists for one property of the tile plan
``plan_tiles`` (ddc.hip) gives it; ``plan_of`` asks the library for the plan
(``rfa_ddc_tile_plan``, host only) and asserts the property, with the mixer table length the
case really runs with, so that a change of the planning code cannot quietly move a case onto
another path.  Nothing here restates the planning rule."""
import functools
from typing import NamedTuple

import numpy as np

from oracle import demod as od
from rfanalyzer_amd import demod

SR = 2_400_000
CENTER = 100_000_000
FMT = {"s8": od.IN_S8, "u8": od.IN_U8, "s16": od.IN_S16LE, "f32": od.IN_F32_INTERLEAVED}
SB = {"s8": 2, "u8": 2, "s16": 4, "f32": 8}
# channel offset at 2.4 Msps -> mixer table length (oracle.demod.mixer_table; checked on the CPU)
OFFSET_OF_LENGTH = {1: 0, 2: 1_200_000, 3: 800_000, 4: 600_000, 5: 480_000, 443: 130_000, 499: 4801}
LENGTH_OF_OFFSET = {o: L for L, o in OFFSET_OF_LENGTH.items()}
LDS_LIMIT = 160 * 1024


class Row(NamedTuple):
    T: int
    D: int
    what: str
    holds: object          # plan dict -> bool


def _row(T, D, what, holds):
    return (T, D), Row(T, D, what, holds)


ROWS = dict([
    _row(1, 1, "T = 1, linear, first output at input 1",
         lambda p: p["pad"] == 0 and p["row"] == 1 and p["chunks"] == 1 and p["KC"] == 1),
    _row(1, 4, "T = 1, pad layout", lambda p: p["pad"] == 1 and p["row"] == 4 and p["KC"] == 1),
    _row(5, 1, "D = 1 with history", lambda p: p["pad"] == 0 and p["row"] == 1 and p["KC"] == 5),
    _row(33, 2, "smallest even D", lambda p: p["pad"] == 1 and p["row"] == 2 and p["P"] == 256 and p["chunks"] == 1),
    _row(33, 3, "smallest odd D > 1",
         lambda p: p["pad"] == 0 and p["row"] == 3 and p["P"] == 256 and p["chunks"] == 1),
    _row(8, 64, "D > T, P not a multiple of 64",
         lambda p: p["pad"] == 1 and 64 < p["P"] < 256 and p["P"] % 64 != 0 and p["threads"] == 192),
    _row(7, 65, "D > T, linear",
         lambda p: p["pad"] == 0 and p["row"] == 65 and 64 < p["P"] < 256 and p["P"] % 64 != 0),
    _row(9000, 100, "1 < P < 64, one chunk", lambda p: 1 < p["P"] < 64 and p["threads"] == 64 and p["chunks"] == 1),
    _row(9000, 101, "P = 64", lambda p: p["P"] == 64 and p["threads"] == 64 and p["chunks"] == 1 and p["pad"] == 0),
    _row(9000, 12000, "P = 1, one chunk (two outputs' window does not fit), D > T",
         lambda p: p["P"] == 1 and p["chunks"] == 1 and p["KC"] == 9000 and p["pad"] == 1),
    _row(14000, 3, "P = 1, two chunks, linear",
         lambda p: p["P"] == 1 and p["chunks"] == 2 and p["pad"] == 0 and p["KC"] < 14000),
    _row(14000, 4, "P = 1, two chunks, pad",
         lambda p: p["P"] == 1 and p["chunks"] == 2 and p["pad"] == 1 and p["KC"] < 14000),
    _row(30000, 64, "P = 1, three chunks", lambda p: p["P"] == 1 and p["chunks"] == 3 and p["pad"] == 1),
])


def table_length(fmt, offset):
    """Mixer table length of channel ``CENTER + offset`` at SR; 0 for f32 (arrives mixed)."""
    return 0 if fmt == "f32" else demod.mix_info(fmt, SR, CENTER, CENTER + offset)[1]


def plan_of(T, D, L, interpolation=1):
    """The library's plan for the filter, the row's property asserted on it."""
    plan = demod.tile_plan(T, interpolation, D, L)
    assert plan["lds_bytes"] <= LDS_LIMIT and plan["threads"] % 64 == 0 and plan["threads"] >= plan["P"], plan
    assert plan["chunks"] == -(-T // plan["KC"]), plan
    if interpolation == 1 and (T, D) in ROWS:
        row = ROWS[(T, D)]
        assert row.holds(plan), (row.what, L, plan)
    return plan


# ---------------------------------------------------------------- cases

class Case(NamedTuple):
    fmt: str
    T: int
    D: int
    byte_offset: object = None      # None: host path (aligned staging buffer); else process_device at this offset
    tune: tuple = ((0, 130_000),)   # (packet index, channel offset): set_frequencies before that packet

    @property
    def id(self):
        s = f"{self.fmt}-T{self.T}-D{self.D}"
        if self.byte_offset is not None:
            s += f"-at{self.byte_offset}"
        if self.tune != Case._field_defaults["tune"]:
            s += "-L" + "_".join(str(LENGTH_OF_OFFSET[o]) for _, o in self.tune)
        return s

    def lengths(self):
        return [table_length(self.fmt, o) for _, o in self.tune]

    def plan(self):
        """The plan under every table the case runs with (each asserted); the first one's returned."""
        return [plan_of(self.T, self.D, L) for L in self.lengths()][0]

    def sizes(self):
        return tuple(packets(self.T, self.plan()["P"], 1, self.D, retunes=len(self.tune) - 1))


PER_SAMPLE = {"s8": (2, 4, 6), "u8": (2, 4, 6), "s16": (4, 8, 12)}      # raw pointer not a multiple of 4 samples
FOUR_SAMPLE = {"s8": 8, "u8": 8, "s16": 16}                                # one group in: the four-sample loads

BASE = [Case("s8", T, D) for T, D in ROWS]
FORMATS = [Case(fmt, T, D) for fmt in ("u8", "s16", "f32") for T, D in ((33, 2), (33, 3), (8, 64), (14000, 4))]
ALIGNMENTS = [Case(fmt, T, D, off) for fmt in ("s8", "u8", "s16") for T, D in ((33, 2), (33, 3), (5, 1), (14000, 3))
              for off in (*PER_SAMPLE[fmt], FOUR_SAMPLE[fmt])]
TABLES = [Case(fmt, 33, D, off, ((0, OFFSET_OF_LENGTH[L]),))
          for fmt in ("s8", "s16") for D in (2, 3) for L in OFFSET_OF_LENGTH for off in (None, SB[fmt])]
RETUNES = [Case("s8", 33, D, off, ((0, 800_000), (6, 130_000), (8, 800_000))) for D in (2, 3) for off in (None, 2)]
ALL = BASE + FORMATS + ALIGNMENTS + TABLES + RETUNES

# rates -> (interpolation, decimation, taps per output) the oracle's RationalResampler gives
POLYPHASE = {(48_000, 44_100): (147, 160, 36), (2_400_000, 2_000_000): (5, 6, 40), (250_000, 192_000): (96, 125, 43),
             (1_000_000, 999_000): (999, 1000, 33), (10_000_000, 8_000): (1, 1250, 501)}
POLY_CASES = [("s8", sr, out, None) for sr, out in POLYPHASE] + [("s16", 250_000, 192_000, 4),
                                                                  ("f32", 2_400_000, 2_000_000, None)]


def poly_channel(sr):
    """A channel an eighth of the rate (and 1 Hz) off the centre: a long mixer table at every rate."""
    return CENTER + sr // 8 + 1


def poly_plan(fmt, sr, out):
    i, d, t = POLYPHASE[(sr, out)]
    L = 0 if fmt == "f32" else demod.mix_info(fmt, sr, CENTER, poly_channel(sr))[1]
    plan = plan_of(t, d, L, interpolation=i)
    assert plan["chunks"] == 1 and plan["row"] == max(1, d // i), plan
    if i > 1:
        assert plan["pad"] == 0 and plan["row"] == 1 and plan["P"] == 256, plan        # near unity: linear, full tile
    else:
        assert plan["pad"] == 1 and plan["row"] == 1250 and 1 < plan["P"] < 64, plan    # one phase, even row, small P
    return plan


def poly_sizes(fmt, sr, out):
    i, d, t = POLYPHASE[(sr, out)]
    return tuple(packets(t, poly_plan(fmt, sr, out)["P"], i, d))


# ---------------------------------------------------------------- packets

def outputs_after(in_total, interpolation, decimation, polyphase=False):
    """Outputs a filter has produced once it has consumed in_total inputs: FirFilter's counter
    (first output at input D - 1, at input 1 when D = 1; FirFilter.kt:46,78,101-103) or the
    RationalResampler's (output n at input n * D // I)."""
    off = 0 if polyphase else (decimation - 1 if decimation >= 2 else 1)
    lim = in_total * interpolation - off
    return -(-lim // decimation) if lim > 0 else 0


def packets(T, P, interpolation, decimation, retunes=0):
    """The ragged call sizes of one run.  In order: a first packet shorter than T - 1 (where the
    filter has a history), 1, 0, three short ones with S mod 4 = 1, 2, 3 (the running total
    still short of T - 1 for a long filter: the history kernel alone runs), exactly the inputs
    of P outputs, one packet of two full tiles and a part of a third, and a rest of a tile and a
    half (or what brings the total to 9 T / 4 where the filter is long)."""
    pd = -(-P * decimation // interpolation)
    sizes = ([(T - 1) // 2] if T >= 3 else []) + [1, 0, 5, 6, 7, pd]
    sizes.append(-(-(2 * P + max(1, P // 3)) * decimation // interpolation) + 1)
    sizes.append(max(3 * pd // 2 + 3, 9 * T // 4 - sum(sizes)))
    assert len(sizes) > 6 + retunes
    return sizes


def packet_kinds(sizes, T, P, interpolation, decimation, polyphase=False):
    """Which of the packet kinds the issue lists a sequence contains, from the plan's P."""
    kinds = set()
    done = 0
    for k, n in enumerate(sizes):
        n_out = (outputs_after(done + n, interpolation, decimation, polyphase)
                 - outputs_after(done, interpolation, decimation, polyphase))
        if k == 0 and 0 < n < T - 1:
            kinds.add("first shorter than T - 1")
        if n in (0, 1):
            kinds.add(f"{n} samples")
        if n > 4 and n % 4:
            kinds.add(f"S mod 4 = {n % 4}")
        if n == -(-P * decimation // interpolation):
            kinds.add("exactly P D inputs")
        if n_out > 2 * P and (n_out % P or P == 1):
            kinds.add("several tiles, ragged last")
        done += n
    return kinds


def required_kinds(T):
    kinds = {"0 samples", "1 samples", "S mod 4 = 1", "S mod 4 = 2", "S mod 4 = 3", "exactly P D inputs",
             "several tiles, ragged last"}
    return kinds | ({"first shorter than T - 1"} if T >= 3 else set())


# ---------------------------------------------------------------- data and the oracle's run

def fir_taps(T):
    return (np.random.default_rng(1000 + T).standard_normal(T) * 0.25).astype(np.float32)


def raw_bytes(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "s16":
        return rng.integers(-32768, 32768, 2 * n, dtype=np.int16).view(np.uint8)
    if fmt == "f32":
        return rng.standard_normal(2 * n).astype(np.float32).view(np.uint8)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8)


def case_raw(case):
    return raw_bytes(case.fmt, sum(case.sizes()), 7 * case.T + case.D + len(case.fmt))


def chunks(raw, fmt, sizes):
    pos = 0
    for n in sizes:
        yield raw[pos * SB[fmt]:(pos + n) * SB[fmt]]
        pos += n


def run_front_end(fe, case, raw, process=None):
    """Feed case's packets to a front end (oracle or device), retuning where the case says;
    the list of (re, im) per packet."""
    process = process or fe.process
    outs = []
    tune = dict(case.tune)
    for k, chunk in enumerate(chunks(raw, case.fmt, case.sizes())):
        if k in tune:
            fe.set_frequencies(CENTER, CENTER + tune[k])
        outs.append(process(chunk))
    return outs


@functools.lru_cache(maxsize=None)
def _oracle_run(fmt, T, D, tune):
    case = Case(fmt, T, D, None, tune)
    ref = od.FrontEnd(FMT[fmt], SR, max(1, SR // D), taps=fir_taps(T), decimation=D)
    outs = run_front_end(ref, case, case_raw(case))
    return outs, ref


def oracle_run(case):
    """(per-packet outputs, the oracle front end after the run), computed once per
    (format, filter, tuning) and shared by the pointer-alignment variants: do not modify."""
    return _oracle_run(case.fmt, case.T, case.D, case.tune)
