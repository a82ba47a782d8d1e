"""The simulation behind demod.CodeRule's defaults: numpy in the audio domain, CPU only.

A DCS code at 600 Hz deviation under band-limited "voice" of RMS 0 / 1500 / 3000 Hz and a DC offset of
+-800 Hz, as NFM audio (deviation / 7500) at 48 kHz, through the code meter's own arithmetic (quantised
samples summed over sub-cells) into demod.dcs_score for the wanted code.  Compared: the right code, another
table code, the inverse code, voice alone and hiss.  Prints, per window length, the lowest score of the
right code and the highest of each other case.

    python tools/code_rule_sim.py [trials per cell]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from rfanalyzer_amd import demod  # noqa: E402

RATE = 48000
P = demod.CODE_SUBCELLS
SCALE = 1.0 / 7500.0                                         # NFM: audio = deviation / (0.75 * 10 kHz)


def voice(rng, n, rms):
    if rms == 0.0:
        return np.zeros(n)
    spec = np.fft.rfft(rng.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / RATE)
    spec[(f < 300.0) | (f > 3000.0)] = 0.0
    x = np.fft.irfft(spec, n)
    return x * (rms / np.sqrt(np.mean(x * x)))


def nrz(word, n, start_bit):
    bit = np.floor(start_bit + np.arange(n) * (134.4 / RATE)).astype(np.int64) % 23
    return np.where((word >> bit) & 1, 1.0, -1.0)


def subcells(audio):
    a = audio.astype(np.float32)
    q = np.rint(a.astype(np.float64) * 2.0 ** 24).astype(np.int64)
    j = 672 * P * np.arange(a.size, dtype=np.int64) // (5 * RATE)
    out = np.zeros(int(j[-1]) + 1, np.int64)
    np.add.at(out, j, q)
    return out


def main():
    trials = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    rng = np.random.Generator(np.random.PCG64(2024))
    codes = demod.DCS_CODES
    for words in (2, 4, 6):
        need = P * (23 * words + 1)
        n = int(np.ceil((need + 1) * 5 * RATE / (672 * P))) + 1
        right, wrong, inverse, speech, hiss = [], [], [], [], []
        for rms in (0.0, 1500.0, 3000.0):
            for dc in (-800.0, 800.0):
                for _ in range(trials):
                    want, other = rng.choice(len(codes), 2, replace=False)
                    w = demod.dcs_word(codes[want])
                    start = rng.uniform(0, 23)

                    def run(dev):
                        return demod.dcs_score(subcells((dev + voice(rng, n, rms) + dc) * SCALE)[:need], w, words)

                    right.append(run(600.0 * nrz(w, n, start)))
                    wrong.append(run(600.0 * nrz(demod.dcs_word(codes[other]), n, start)))
                    inverse.append(run(600.0 * nrz(w ^ 0x7FFFFF, n, start)))
                    if rms:
                        speech.append(run(np.zeros(n)))
                    hiss.append(demod.dcs_score(subcells((rng.standard_normal(n) * 3000.0 + dc) * SCALE)[:need], w,
                                                words))
        print(f"words {words} ({need} sub-cells, {need / (134.4 * P):.2f} s), {len(right)} trials per case: "
              f"right code min {min(right):.3f}; other code max {max(wrong):.3f}; inverse max {max(inverse):.3f}; "
              f"voice alone max {max(speech):.3f}; hiss max {max(hiss):.3f}")


if __name__ == "__main__":
    main()
