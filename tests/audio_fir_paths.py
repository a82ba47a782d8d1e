"""The case table of the audio FIR bank's device tests (tests/test_gpu_audio_fir.py): every tap count
against every count around the filter's length and around the tile, and one call of five slots with
different tap counts and counts.  tests/test_audio_fir_host.py asserts, on the CPU, that the table
reaches every path rfa_audio_fir_plan can report."""
from rfanalyzer_amd import _lib

TILE = _lib.RFA_AUDIO_FIR_TILE
NARROW_MAX = _lib.RFA_AUDIO_FIR_NARROW_MAX
PATHS = ("none", "copy", "narrow", "wide")                  # everything rfa_audio_fir_plan can report

TAP_COUNTS = (1, 2, 3, 64, 65, 1309, 4096)


def counts_for(t: int):
    """n in {0, 1, T-2, T-1, T, TILE-1, TILE, TILE+1, 2 TILE + 17}, without repeats or negatives."""
    return sorted({n for n in (0, 1, t - 2, t - 1, t, TILE - 1, TILE, TILE + 1, 2 * TILE + 17) if n >= 0})


SINGLE = [(t, n) for t in TAP_COUNTS for n in counts_for(t)]

# five slots in one call: (tap count, count) per slot, one count 0, one slot a pass-through
MULTI = ((0, 300), (1, 0), (65, TILE + 1), (1309, 2 * TILE + 17), (4096, 77))


def shapes():
    """Every (tap count, count) a slot of the table runs."""
    return SINGLE + list(MULTI)
