"""Restatement of the slot meters' summation plan (rfanalyzer_amd/csrc/slot_sum.h)
in numpy, written from the design and not from the kernels: the order of every addition that the
level meter (rfa_squelch_*) and the frequency meter (rfa_freq_*) make, so that a device sum can be
compared bit for bit.  Also the inputs and lengths of that comparison, shared by the CPU test of the
model (test_slot_sum_plan_host.py) and the device tests (test_gpu_squelch.py, test_gpu_freq.py).

The plan: terms are cut into tiles of 16384.  256 threads sum a tile, thread t adding the terms at
t + 256 m in ascending m into a double that starts at +0.0.  A wave of 64 threads folds its
accumulators with a butterfly whose every step adds a lane's value and its partner's -- both lanes of
a pair form the same sum, the addition being commutative, so the fold is six rounds of adjacent
pairs.  The four waves are added in wave order starting from the first, the tiles in ascending order
starting from the first."""
import functools

import numpy as np

import freq_ref
import squelch_ref

TILE = 16384
THREADS = 256
WAVE = 64
LONG = [64 * TILE + 1, 65 * TILE + 5]   # 65 and 66 tiles: the tile fold fetches a second time, 1 and 2 partials
# test_gpu_squelch.LENGTHS and test_gpu_freq.LENGTHS (each module asserts that) and the long ones
POWER_LENGTHS = [1, 63, 64, 65, 255, 256, 257, 4095, 4097, TILE - 1, TILE, TILE + 1, 3 * TILE + 777] + LONG
R1_LENGTHS = [0, 1, 2, 63, 64, 65, 257, 4097, TILE, TILE + 1, 2 * TILE + 1, 40000] + LONG
K = 3


def plan_sum(terms) -> float:
    """The plan's sum of a float64 term array."""
    terms = np.asarray(terms, np.float64)
    total = 0.0
    with np.errstate(all="ignore"):
        for lo in range(0, terms.size, TILE):
            tile = terms[lo:lo + TILE]
            steps = -(-tile.size // THREADS)
            padded = np.zeros(steps * THREADS)            # +0.0 changes no accumulator: none is ever -0.0
            padded[:tile.size] = tile
            acc = np.zeros(THREADS)
            for row in padded.reshape(steps, THREADS):
                acc = acc + row
            v = acc.reshape(THREADS // WAVE, WAVE)
            for _ in range(6):
                v = v[:, 0::2] + v[:, 1::2]
            s = v[0, 0]
            for w in v[1:, 0]:
                s = s + w
            total = s if lo == 0 else total + s
    return float(total)


def sequential_sum(terms) -> float:
    """The same terms added left to right in double: what the plan must be told apart from."""
    terms = np.asarray(terms, np.float64)
    return float(np.add.accumulate(terms)[-1]) if terms.size else 0.0


@functools.lru_cache(maxsize=None)
def pin_rows(n):
    """[3, n] finite float32 rows.  Rows 0 and 2 are enveloped, 2^U(-12, 0) * U(-1, 1) per sample: their
    terms span some 48 binary orders, so the order of the additions shows in the sum's last bits.  Row
    1 is flat noise as in the other tests (its float32 power terms add exactly up to a tile)."""
    rng = np.random.Generator(np.random.PCG64(5700 + n))

    def row(k):
        x = rng.uniform(-1, 1, n)
        return ((0.3 * x) if k == 1 else 2.0 ** rng.uniform(-12, 0, n) * x).astype(np.float32)

    re = np.stack([row(k) for k in range(K)])
    im = np.stack([row(k) for k in range(K)])
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


@functools.lru_cache(maxsize=None)
def power_terms(n):
    """Per slot of pin_rows(n): the level meter's terms, float32 widened."""
    re, im = pin_rows(n)
    return tuple(squelch_ref.terms(re[k], im[k]).astype(np.float64) for k in range(K))


@functools.lru_cache(maxsize=None)
def r1_terms(n, carried):
    """Per slot of pin_rows(n): the frequency meter's (real, imaginary) terms, one per sample.  Term 0
    takes the row's own last sample as its predecessor where ``carried`` -- the same rows given twice
    -- and is +0.0 without one."""
    re, im = pin_rows(n)
    out = []
    for k in range(K):
        p1, p2, q1, q2 = freq_ref.products(re[k], im[k], (re[k, -1], im[k, -1]) if carried and n else None)
        tr, ti = p1 + p2, q1 - q2
        if not carried and n:
            tr, ti = np.concatenate([[0.0], tr]), np.concatenate([[0.0], ti])
        out.append((tr, ti))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def power_sums(n):
    return np.array([plan_sum(t) for t in power_terms(n)])


@functools.lru_cache(maxsize=None)
def r1_sums(n, carried):
    """(re[3], im[3]) of the plan."""
    t = r1_terms(n, carried)
    return np.array([plan_sum(tr) for tr, _ in t]), np.array([plan_sum(ti) for _, ti in t])
