"""The case table of the audio resampler bank's device tests (tests/test_gpu_audio_rs.py): every ratio with
tap counts below L, off a multiple of L and at exactly L J, the longest phase and the longest filter,
against the counts around D and around the output tile; one call of five slots; ragged call sequences.
tests/test_audio_rs_host.py asserts, on the CPU, that the table reaches every path rfa_audio_rs_plan
can report."""
from rfanalyzer_amd import demod

PATHS = ("none", "convert", "decimate", "polyphase")        # everything rfa_audio_rs_plan can report

# (L, D, T)
CASES = (
    (1, 1, 0),                                              # no filter: the conversion alone
    (1, 1, 5),
    (1, 2, 4096),                                           # J = 4096 at L = 1
    (1, 3, 65),
    (1, 6, 219),                                            # resampler_taps(48000, 8000)'s length
    (2, 3, 1),                                              # T < L: phase 1 is zero padding alone, J = 1
    (2, 3, 7),                                              # T off a multiple of L
    (2, 3, 8),                                              # T = L J
    (147, 160, 100),                                        # T < L, J = 1
    (147, 160, 1000),
    (147, 640, 1176),                                       # T = L J, J = 8
    (147, 640, 16384),                                      # the longest filter, J = 112
)


def path_of(L: int, T: int) -> str:
    return "convert" if T == 0 else "decimate" if L == 1 else "polyphase"


def tile_of(L: int, D: int, T: int) -> int:
    return demod.audio_rs_plan(L, D, T, 1)["tile"]


def tile_inputs(L: int, D: int, T: int) -> int:
    """The inputs that, from offset 0, give one full output tile and no more."""
    return tile_of(L, D, T) * D // L


def counts_for(L: int, D: int, T: int):
    """n in {0, 1, D-1, D, D+1, one tile's inputs -1 / exact / +1, a row of three tiles}, without repeats."""
    t = tile_inputs(L, D, T)
    three = (2 * tile_of(L, D, T) + 17) * D // L
    return sorted({0, 1, D - 1, D, D + 1, t - 1, t, t + 1, three})


# five slots in one call, a 0 among the counts: (L, D, T), then the counts
MULTI = (
    ((1, 6, 219), (300, 0, 6 * 1024 + 1, 2 * 6 * 1024 + 100, 5)),
    ((147, 640, 1176), (4459, 1, 0, 9000, 77)),
)

# calls of one slot that add up to a stream given whole
RAGGED = (1, 7, 0, 333, 0, 2, 14000)
RAGGED_CASES = ((1, 6, 219), (1, 2, 4096), (2, 3, 7), (147, 640, 16384), (1, 1, 0))


def shapes():
    """Every (L, D, T, n) a slot of the table runs."""
    out = [(L, D, T, n) for L, D, T in CASES for n in counts_for(L, D, T)]
    out += [(*case, n) for case, ns in MULTI for n in ns]
    out += [(*case, n) for case in RAGGED_CASES for n in RAGGED]
    return out
