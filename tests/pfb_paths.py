"""The case table of the channelizer tile's paths (rfanalyzer_amd/csrc/channelizer.hip: pfb_kernel,
pfb_rational_kernel and their tuned siblings), shared by tests/test_pfb_paths_host.py (CPU: plans,
coverage, the float32 model against the float64 restatements) and tests/test_gpu_pfb_paths.py (GPU:
every case bit for bit against the model).

A case exists for one property of the plan the library gives it -- the radix sequence of M, the
output times per workgroup NT, what is staged in LDS.  ``Case.plan()`` asks the library
(``rfa_pfb_tile_plan``, host only, the planning code the launch runs) and asserts the property, so a
change of the planning code cannot quietly move a case onto another path; ``coverage`` is computed
from the same answers.  Nothing here restates the planning rule.

Every case is fed in two calls (``Case.sizes()``): the first fills the history and ends inside a
tile and inside a decimation period, the second holds two full tiles and a ragged one (NT = 1: 3
and 2 outputs).  Formats rotate over s8 / u8 / s16 / f32; taps are random in [-1, 1]."""
import functools
from typing import NamedTuple

import numpy as np

import pfb_model
import pfb_rational_ref as rref
import pfb_ref
from rfanalyzer_amd import demod

SB = {"s8": 2, "u8": 2, "s16": 4, "f32": 8}
FORMATS = ("s8", "u8", "s16", "f32")
LDS_MOST = 64 * 1024 + 2 * (4096 + 16) * 8          # 131 328 B: the dynamic LDS the kernels are prepared for


class Case(NamedTuple):
    M: int
    L: object               # None: rfa_pfb_create; else the interpolation of rfa_pfb_create_rational
    D: int
    T: int
    fmt: str
    why: str
    want: dict              # plan fields the case must get ("plan": the rational plan's letter)

    @property
    def id(self):
        return (f"M{self.M}-T{self.T}-D{self.D}-{self.fmt}" if self.L is None
                else f"M{self.M}-L{self.L}-D{self.D}-T{self.T}-{self.fmt}")

    def __hash__(self):     # ``want`` is a dict; a case is its id
        return hash(self.id)

    @property
    def Th(self):
        """Taps per output: T, or Tp = ceil(T / L)."""
        return self.T if self.L is None else -(-self.T // self.L)

    def plan(self) -> dict:
        """The library's plan, the case's property asserted on it."""
        p = demod.pfb_tile_plan(self.M, 0 if self.L is None else self.L, self.D, self.T)
        p["plan"] = letter(p)
        assert p["lds_bytes"] <= LDS_MOST and int(np.prod(p["radices"])) == self.M, p
        for k, v in self.want.items():
            assert p[k] == v, (self.id, self.why, k, p)
        return p

    def outputs(self):
        """(outputs of the first call, of the second)."""
        nt = self.plan()["NT"]
        if self.L is None:                                   # samples of the first call: n1 D + D // 2
            need = max(0, -(-(self.Th - 1 - self.D // 2) // self.D))
        else:                                                # floor(n1 D / L)
            need = -(-(self.Th - 1) * self.L // self.D)
        n1, n2 = (3, 2) if nt == 1 else (nt + max(1, nt // 2), 2 * nt + max(1, nt // 3))
        n1 = max(n1, need)
        if nt > 1 and n1 % nt == 0:
            n1 += 1
        return n1, n2

    def sizes(self):
        """Samples of the two calls.  Integer: the first ends half a decimation period past its last
        output, the second D - 1 samples short of another.  Rational: each ends on the last sample
        that does not yet make another output due."""
        n1, n2 = self.outputs()
        if self.L is None:
            return n1 * self.D + self.D // 2, n2 * self.D + (self.D - self.D // 2) - 1
        s1 = n1 * self.D // self.L
        return s1, (n1 + n2) * self.D // self.L - s1

    def count(self, c: int) -> int:
        """Outputs after c samples."""
        return c // self.D if self.L is None else rref.count(c, self.L, self.D)


def letter(p: dict) -> str:
    """Plan A: run and taps staged; B: the run only; C: nothing."""
    return "C" if not p["staged_run"] else ("A" if p["staged_taps"] else "B")


def _table():
    integer = [
        (8, 19, 3, "2 after 4 at the smallest M", dict(radices=[4, 2])),
        (9, 40, 4, "3 first, 3 after 3, odd M", dict(radices=[3, 3], Mp=9)),
        (10, 33, 10, "2 first, 5 after 2, D = M", dict(radices=[2, 5])),
        (12, 50, 5, "3 after 4", dict(radices=[4, 3])),
        (15, 31, 1, "5 after 3, odd M, D = 1", dict(radices=[3, 5], Mp=15)),
        (18, 100, 7, "3 after 2", dict(radices=[2, 3, 3])),
        (20, 7, 9, "T < M: residues with no tap", dict(radices=[4, 5])),
        (25, 60, 11, "5 first, 5 after 5", dict(radices=[5, 5])),
        (27, 1, 2, "T = 1: no history, no history launch", dict(radices=[3, 3, 3])),
        (32, 512, 32, "T = 16 M", dict(radices=[4, 4, 2])),
        (125, 300, 50, "three radix-5 stages", dict(radices=[5, 5, 5])),
        (256, 2901, 256, "the largest LDS request", dict(NT=16, staged_run=1, stage_points=8192, lds_bytes=LDS_MOST)),
        (256, 2902, 256, "the other side of that edge", dict(NT=16, staged_run=0)),
        (270, 800, 91, "first M past 256", dict(NT=8, staged_run=1, radices=[2, 3, 3, 3, 5])),
        (512, 3073, 512, "NT = 8 unstaged", dict(NT=8, staged_run=0)),
        (540, 1100, 200, "first M past 512", dict(NT=4, staged_run=1)),
        (1024, 2048, 300, "NT = 4 staged", dict(NT=4, staged_run=1)),
        (1024, 16384, 1024, "NT = 4 unstaged, T = 16 M", dict(NT=4, staged_run=0)),
        (1080, 2200, 401, "first M past 1024", dict(NT=2, staged_run=1)),
        (2048, 4100, 1000, "NT = 2 staged", dict(NT=2, staged_run=1, lds_bytes=122768)),
        (2048, 6000, 2048, "NT = 2 unstaged", dict(NT=2, staged_run=0)),
        (2160, 2160, 999, "first M past 2048", dict(NT=1, staged_run=1)),
        (3125, 3125, 3125, "NT = 1, five radix-5 stages, odd M, D = M", dict(NT=1, radices=[5] * 5, Mp=3125)),
        (2187, 5000, 2000, "NT = 1, seven radix-3 stages", dict(NT=1, radices=[3] * 7)),
        (4096, 5461, 4096, "NT = 1 staged at the edge", dict(NT=1, staged_run=1, stage_points=8192)),
        (4096, 5462, 4096, "NT = 1 unstaged at the edge", dict(NT=1, staged_run=0)),
    ]
    rational = [
        (16, 48, 125, 965, "the app's 48 / 125, L > NT at NT 16",
         dict(plan="A", NT=16, staged_taps=16, rows_by_time=1)),
        (16, 64, 65, 1000, "L at its limit, D = L + 1", dict(plan="A", NT=16, staged_taps=16, rows_by_time=1)),
        (32, 16, 17, 300, "L = NT", dict(plan="A", NT=16, staged_taps=16, rows_by_time=0)),
        (24, 17, 100, 500, "L = NT + 1", dict(plan="A", NT=16, staged_taps=16, rows_by_time=1)),
        (9, 2, 3, 2, "Tp = 1: no history on the rational path", dict(plan="A", radices=[3, 3])),
        (540, 7, 1000, 4000, "NT = 4, rows by time", dict(plan="A", NT=4, staged_taps=4, rows_by_time=1)),
        (1080, 2, 2159, 3000, "NT = 2, rows by phase, D = L M - 1",
         dict(plan="A", NT=2, staged_taps=2, rows_by_time=0)),
        (2048, 3, 4097, 9000, "NT = 2, rows by time", dict(plan="A", NT=2, staged_taps=2, rows_by_time=1)),
        (2048, 3, 4097, 21000, "NT = 2, nothing staged: run 8366 > 8192", dict(plan="C", NT=2, run=8366)),
        (256, 16, 255, 16000, "run staged, taps from global memory, at NT 16", dict(plan="B", NT=16)),
        (256, 1, 256, 2901, "the largest LDS request (beside the kernel's static arrays)",
         dict(plan="A", NT=16, lds_bytes=LDS_MOST)),
        (256, 1, 256, 2902, "the other side of that edge", dict(plan="B", NT=16)),
        (3125, 1, 3125, 3125, "NT = 1, five radix-5 stages", dict(plan="A", NT=1, radices=[5] * 5)),
    ]
    cases = [Case(M, None, D, T, FORMATS[i % 4], why, want) for i, (M, T, D, why, want) in enumerate(integer)]
    cases += [Case(M, L, D, T, FORMATS[(i + 1) % 4], why, want) for i, (M, L, D, T, why, want) in enumerate(rational)]
    return cases


ALL = _table()
INTEGER = [c for c in ALL if c.L is None]
RATIONAL = [c for c in ALL if c.L is not None]

# (f) the tuned store at the NT values the tuning tests never reach: step 0, +-1 and q - 1
TUNED_Q = 96
TUNED = [c for c in ALL if (c.M, c.L, c.T) in {(540, None, 1100), (1080, None, 2200), (2160, None, 2160),
                                               (1080, 2, 3000)}]


def coverage(cases) -> dict:
    """What the table runs, from the library's answers alone."""
    cov = {"first": set(), "pairs": set(), "tiles": {False: set(), True: set()}, "plans": set(), "rows": set(),
           "rows_by_time_L": set(), "one_tap": set()}
    for c in cases:
        p = c.plan()
        rad = p["radices"]
        cov["first"].add(rad[0])
        cov["pairs"] |= set(zip(rad, rad[1:]))
        if c.L is None:
            cov["tiles"][False].add((p["NT"], p["staged_run"]))
        else:
            cov["tiles"][True].add((p["NT"], p["staged_run"]))
            cov["plans"].add(p["plan"])
            if p["staged_taps"]:
                cov["rows"].add("time" if p["rows_by_time"] else "phase")
                if p["rows_by_time"]:
                    cov["rows_by_time_L"].add(c.L)
        if c.Th == 1:
            cov["one_tap"].add(c.L is not None)
    return cov


# ---------------------------------------------------------------- data

def raw_bytes(fmt, n, seed):
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return rng.uniform(-1, 1, 2 * n).astype("<f4").view(np.uint8)
    if fmt == "s16":
        return rng.integers(-32768, 32768, 2 * n, dtype=np.int16).view(np.uint8)
    return rng.integers(0, 256, 2 * n, dtype=np.uint8)


def _seed(case):
    return 7 * case.M + 3 * case.T + case.D + (0 if case.L is None else 100_003 * case.L)


@functools.lru_cache(maxsize=None)
def data(case):
    """(taps float32, raw bytes of both calls, converted samples complex128); read only."""
    taps = np.random.default_rng(_seed(case)).uniform(-1, 1, case.T).astype(np.float32)
    raw = raw_bytes(case.fmt, sum(case.sizes()), _seed(case) + 1)
    x = pfb_ref.convert(raw, case.fmt)
    for a in (taps, raw, x):
        a.setflags(write=False)
    return taps, raw, x


def selection(case):
    """(e) a selection with duplicates, ends of the range included; 23 slots where M allows, so that
    slots * NT is more than one pass of the store's 256 threads at NT = 16."""
    K = min(case.M, 23)
    sel = np.random.default_rng(_seed(case) + 2).integers(0, case.M, K)
    sel[0], sel[1], sel[2] = case.M - 1, 0, case.M - 1
    return [int(k) for k in sel]


# ---------------------------------------------------------------- references, computed once per case

def model_stream(case):
    taps, _, _ = data(case)
    return pfb_model.Stream(case.M, case.D, taps, case.L)


@functools.lru_cache(maxsize=None)
def model_run(case):
    """The model fed the case's two calls: ([M, n1], [M, n2]) complex64; read only."""
    _, _, x = data(case)
    s1, _ = case.sizes()
    m = model_stream(case)
    out = (m.process(x[:s1]), m.process(x[s1:]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def float64_run(case):
    """(the float64 restatement of every output of both calls [M, n1 + n2], the derived bound); read only."""
    taps, _, x = data(case)
    if case.L is None:
        ref, b = pfb_ref.folded(x, taps, case.M, case.D), pfb_ref.bound(taps, x, case.M)
    else:
        ref, b = rref.folded(x, taps, case.M, case.L, case.D), rref.bound(taps, x, case.M, case.L)
    ref.setflags(write=False)
    return ref, b


def ratio(y, case) -> float:
    """max |y - float64 restatement| / bound over every output of every channel."""
    ref, b = float64_run(case)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    return float(np.abs(y.astype(np.complex128) - ref).max() / b)
