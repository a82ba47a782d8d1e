"""GPU: window peak / mean for every frame of a batch (rfa_set_windows, rfa_get_window_stats,
rfa_ring_window_stats) against the Kotlin-semantics restatement
(oracle/scanner.py window_stats) on the device's own rows -- the caller rows of the same call
or ring().  The bars are those of tests/test_gpu_scanner.py: peaks bit for bit, finite averages
within one float ulp (FloatArray.average() is a double sum rounded once; only the order of the
double additions differs), non-finite entries of the same kind (NaN, +inf, -inf; the sign and
payload of a NaN are not compared: host and device default NaNs differ).  Where two device
results are compared (row sources, batch splits, pipelined against serial) every bit must
agree, NaNs included."""
import numpy as np
import pytest

import signals
from oracle import scanner as osc
from rfanalyzer_amd import scanner as sc

pytestmark = pytest.mark.gpu

F0, SR = 433_000_000, 2_400_000
F32 = np.float32
TONES = ((0.21, 0.3), (0.37, 0.01), (-0.2, 0.002))


def _frames(n, count, seed):
    return signals.frames_bytes(n, count, "s8", seed=seed, tones=TONES, noise=0.01)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _same_bits(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(_bits(a), _bits(b))


def _check(pk, av, rows, lo, hi, what=""):
    """(pk, av)[f] against the restatement over rows[f]."""
    assert pk.shape == av.shape == (len(rows), len(lo)), (what, pk.shape, av.shape, len(rows), len(lo))
    for f, row in enumerate(rows):
        epk, eav = osc.window_stats(row, lo, hi)
        for name, got, exp in (("peak", pk[f], epk), ("avg", av[f], eav)):
            for kind in (np.isnan, np.isposinf, np.isneginf):
                assert np.array_equal(kind(got), kind(exp)), f"{what} frame {f}: {name} {kind.__name__} entries differ"
        ok = ~np.isnan(epk)
        bad = np.flatnonzero(_bits(pk[f])[ok] != _bits(epk)[ok])
        assert bad.size == 0, f"{what} frame {f}: {bad.size} peaks differ, first window {np.flatnonzero(ok)[bad[0]]}"
        fin = np.isfinite(eav)
        g, e = av[f][fin], eav[fin]
        near = (g == e) | (g == np.nextafter(e, F32(np.inf))) | (g == np.nextafter(e, F32(-np.inf)))
        assert near.all(), f"{what} frame {f}: {int((~near).sum())} averages beyond one ulp " \
                           f"(worst {np.abs(g.astype(np.float64) - e).max():.3e} dB)"


def _within_one_ulp(a, b):
    return np.all(np.abs(_bits(a).astype(np.int64) - _bits(b).astype(np.int64)) <= 1)


def _random_windows(n, count, wide, seed):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, n, count)
    hi = np.minimum(n - 1, lo + rng.integers(0, wide, count))
    return lo.astype(np.int32), hi.astype(np.int32)


def _grid(n, step=56):
    b = np.arange(2, n - 2, step)
    return (b - 2).astype(np.int32), (b + 2).astype(np.int32)


def _cat(*lists):
    return (np.concatenate([l[0] for l in lists]).astype(np.int32),
            np.concatenate([l[1] for l in lists]).astype(np.int32))


def _edges(n):
    return np.array([0, n - 1], np.int32), np.array([0, n - 1], np.int32)


def _whole(n):
    return np.array([0], np.int32), np.array([n - 1], np.int32)


def _batch_rows_in_ring(e, frames):
    """The rows of the last call's frames, frame order, from ring() (frames <= ring_rows)."""
    ring, ri, _ = e.ring()
    R = ring.shape[0]
    return [ring[(ri + (frames - 1 - f)) % R] for f in range(frames)]


# ------------------------------------------------------------------ 1. every ring order
@pytest.mark.parametrize("n", [4096, 32768, 65536, 262144])
def test_every_ring_order(rfa, n):
    """Natural (4096), store tiles with one and two residues (32 K, 64 K), column blocks (256 K):
    a 3-row ring that has wrapped (2 frames, then 3 read from the ring, then 4 more with caller
    rows).  Lists: the whole row, 200 overlapping random windows up to 2000 bins, one-bin windows
    at bin 0 and N - 1, and at 64 K a +-2-bin grid of 1170 windows."""
    data = _frames(n, 9, 40 + n % 97)
    fb = 2 * n
    lists = [_whole(n), _random_windows(n, 200, 2000, n), _edges(n)]
    if n == 65536:
        lists.append(_grid(n))
        assert lists[-1][0].size >= 1000
    lo, hi = _cat(*lists)
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=3) as e:
        e.set_tuning(F0, SR)
        e.set_windows(lo, hi)
        e.process(data[:2 * fb], 2, rows=False)
        e.process(data[2 * fb:5 * fb], 3, rows=False)  # ring rows, write index mid-ring
        pk, av = e.window_stats()
        _check(pk, av, _batch_rows_in_ring(e, 3), lo, hi, f"N={n} ring")
        # four more frames, more than the ring holds, with caller rows (natural order); a shorter
        # list keeps the pure-Python restatement quick
        lo2, hi2 = _cat(_random_windows(n, 60, 1000, n + 1), _edges(n), (lo[-40:], hi[-40:]))
        e.set_windows(lo2, hi2)
        rows = e.process(data[5 * fb:9 * fb], 4)
        pk, av = e.window_stats()
        _check(pk, av, rows, lo2, hi2, f"N={n} caller rows")


# ------------------------------------------------------------------ 2. every row source
_SRC = {}


def _source_case():
    if not _SRC:
        n, frames = 32768, 4
        _SRC.update(n=n, frames=frames, data=_frames(n, frames, 77),
                    win=_cat(_whole(n), _random_windows(n, 150, 1500, 9), _edges(n), _grid(n, 331)))
    return _SRC


@pytest.mark.parametrize("state", ["plain", "all_on"])
def test_every_row_source_gives_the_same_bits(rfa, state):
    """The ring (B <= ring_rows), the staging buffer (B > ring_rows, no caller rows), caller rows
    (process_host's and a torch tensor's): one set of bits, with peak-hold / EMA / channel mean
    all off and all on.  The restatement is checked once, on the caller rows."""
    import torch
    c = _source_case()
    n, frames, data = c["n"], c["frames"], c["data"]
    lo, hi = c["win"]
    kw = dict(avg="ema", ema_alpha=0.2, peak_hold=True) if state == "all_on" else {}
    dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    got = {}

    def run(name, ring_rows, how):
        with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=ring_rows, **kw) as e:
            e.set_tuning(F0, SR)
            if state == "all_on":
                e.set_channel(F0 - 100_000, F0 + 300_000)
            e.set_windows(lo, hi)
            rows = how(e)
            got[name] = e.window_stats()
            if state == "all_on":
                assert e.channel_means().shape == (frames,)
            return rows

    run("ring", frames, lambda e: e.process(data, frames, rows=False))
    run("staging", frames - 1, lambda e: e.process(data, frames, rows=False))
    rows = run("host rows", frames, lambda e: e.process(data, frames))

    def tensor(e, with_rows):
        out = torch.empty((frames, n), dtype=torch.float32, device="cuda") if with_rows else None
        e.process_tensor(dev, frames, rows=out)
        e.synchronize()
        return out

    run("tensor rows", frames - 1, lambda e: tensor(e, True))
    run("tensor ring", frames + 3, lambda e: tensor(e, False))
    if "exp_ok" not in c:
        _check(*got["host rows"], rows, lo, hi, "host rows")
        c["exp_ok"] = got["host rows"]
    for name, (pk, av) in got.items():
        _same_bits(pk, c["exp_ok"][0])
        _same_bits(av, c["exp_ok"][1])


# ------------------------------------------------------------------ 3. batching independence
def test_batching_independence_and_repeat(rfa):
    """11 frames in one call against calls of 1, 3 and 7 frames, and a repeat of the one call:
    identical bits for peak and avg (64 K: store tiles, the ring at another wrap each time)."""
    n, total = 65536, 11
    data = _frames(n, total, 5)
    fb = 2 * n
    lo, hi = _cat(_whole(n), _random_windows(n, 120, 9000, 3), _grid(n), _edges(n))

    def run(split):
        pks, avs = [], []
        with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=16) as e:
            e.set_tuning(F0, SR)
            e.set_windows(lo, hi)
            f = 0
            for b in split:
                e.process(data[f * fb:(f + b) * fb], b, rows=False)
                pk, av = e.window_stats()
                assert pk.shape == (b, lo.size)
                pks.append(pk)
                avs.append(av)
                f += b
        return np.concatenate(pks), np.concatenate(avs)

    one = run((11,))
    for split in ((1, 3, 7), (7, 3, 1), (11,)):
        got = run(split)
        _same_bits(got[0], one[0])
        _same_bits(got[1], one[1])


# ------------------------------------------------------------------ 4. non-finite rows
@pytest.mark.parametrize("window", ["none", "blackman"])
def test_non_finite_rows(rfa, window):
    """f32 input: a silent frame (-inf row), a frame with one NaN sample (NaN row), a frame
    scaled by 2^70 (+inf bins), a constant frame (window none: -inf in every bin but one)
    between plain ones; NaN wins the peak, the sums are the windows' own bins."""
    n, frames = 4096, 7
    rng = np.random.default_rng(12)
    x = (rng.standard_normal((frames, 2 * n)) * 0.1).astype(np.float32)
    x[1] = 0
    x[2, 2 * (n // 3)] = np.nan
    x[3] *= F32(2.0 ** 70)
    x[4] = 0.5
    lo, hi = _cat(_whole(n), _random_windows(n, 100, 400, 21), _edges(n), _grid(n, 97),
                  (np.array([n // 2 - 3, n // 2, n // 2 + 1], np.int32), np.array([n // 2 + 3, n // 2, n // 2 + 40], np.int32)))
    with rfa.SpectrumEngine(n, window, "f32", ring_rows=8) as e, rfa.SpectrumEngine(n, window, "f32", ring_rows=8) as r:
        for eng in (e, r):
            eng.set_tuning(F0, SR)
            eng.set_windows(lo, hi)
        rows = e.process(x.tobytes(), frames)
        pk, av = e.window_stats()
        assert np.isneginf(rows[1]).all() and np.isnan(rows[2]).all() and np.isposinf(rows[3]).any()
        if window == "none":
            assert np.isneginf(rows[4]).sum() == n - 1 and np.isfinite(rows[4]).sum() == 1
        assert np.isfinite(rows[[0, 5, 6]]).all()
        _check(pk, av, rows, lo, hi, f"window {window}")
        assert np.isnan(pk[2]).all() and np.isneginf(pk[1]).all() and np.isneginf(av[1]).all()
        # the same frames read from the ring
        r.process(x.tobytes(), frames, rows=False)
        pr, ar = r.window_stats()
        _same_bits(pr, pk)
        _same_bits(ar, av)


# ------------------------------------------------------------------ 5. the post-hoc form
def test_ring_window_stats(rfa):
    """rows_back = 1, 2 and ring_rows, newest first against ring(); rows_back = 1 against
    rfa_row_window_stats; after a retune that shifts the ring the -9999 fill is seen."""
    n, R = 65536, 4
    data = _frames(n, 6, 8)
    fb = 2 * n
    lo, hi = _cat(_whole(n), _random_windows(n, 120, 1500, 4), _edges(n), _grid(n, 613))
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=R) as e:
        e.set_tuning(F0, SR)
        e.set_windows([5], [9])  # the handle's own list is left alone
        e.process(data[:3 * fb], 3, rows=False)
        e.process(data[3 * fb:], 3, rows=False)
        own = e.window_stats()
        ring, ri, _ = e.ring()
        newest_first = [ring[(ri + r) % R] for r in range(R)]
        full_pk, full_av = e.ring_window_stats(lo, hi, R)
        _check(full_pk, full_av, newest_first, lo, hi, f"rows_back {R}")
        for back in (1, 2):
            pk, av = e.ring_window_stats(lo, hi, back)
            assert pk.shape == (back, lo.size)
            _same_bits(pk, full_pk[:back])
            _same_bits(av, full_av[:back])
        pk1, av1 = e.row_window_stats(lo, hi)
        _same_bits(full_pk[0], pk1)
        assert _within_one_ulp(full_av[0], av1)
        _same_bits(e.window_stats()[0], own[0])
        assert e.windows()[0].tolist() == [5]
        for bad in (0, R + 1):
            with pytest.raises(rfa.RfaError):
                e.ring_window_stats(lo, hi, bad)
        # retune by 300 bins: every row shifted, -9999 filled in
        e.set_tuning(F0 + 300 * SR // n, SR)
        ring, ri, _ = e.ring()
        assert (ring == F32(-9999.0)).any()
        lo2, hi2 = _cat(_edges(n), _random_windows(n, 60, 1200, 6), (np.array([0, n - 700], np.int32),
                                                                     np.array([699, n - 1], np.int32)))
        pk, av = e.ring_window_stats(lo2, hi2, R)
        _check(pk, av, [ring[(ri + r) % R] for r in range(R)], lo2, hi2, "after the retune")
        assert (pk == F32(-9999.0)).any()


# ------------------------------------------------------------------ 6. the interface
def test_bad_window_keeps_the_previous_list_and_empty_list_disables(rfa):
    n = 4096
    data = _frames(n, 5, 2)
    lo, hi = _cat(_random_windows(n, 40, 300, 1), _edges(n))
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=8) as e:
        e.set_tuning(F0, SR)
        assert e.window_stats()[0].shape == (0, 0)
        e.set_windows(lo, hi)
        assert e.window_stats()[0].shape == (0, lo.size)  # no call followed it yet
        for blo, bhi in (([5], [4]), ([0], [n]), ([-1], [3]), ([0, 7], [9, 6])):
            with pytest.raises(rfa.RfaError):
                e.set_windows(blo, bhi)
        rows = e.process(data, 5)
        pk, av = e.window_stats()
        _check(pk, av, rows, lo, hi, "after rejected lists")
        dpk, dav, fr, wn = e.window_stats_device()
        assert (fr, wn) == (5, lo.size) and dpk and dav
        e.set_windows([], [])
        e.process(data, 5, rows=False)
        assert e.window_stats()[0].shape == (0, 0)
        assert e.window_stats_device() == (0, 0, 0, 0)
        # a list alone makes the batch's rows exist: no ring, no state, no caller rows
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=0) as e:
        e.set_windows(lo, hi)
        e.process(data, 5, rows=False)
        _same_bits(e.window_stats()[0], pk)
        _same_bits(e.window_stats()[1], av)


def test_65536_windows_are_accepted(rfa):
    """One two-bin window per bin of a 64 K row: 8192 narrow pieces per block, each 4096-bin
    boundary crossed by one of them."""
    n = 65536
    lo = np.arange(n, dtype=np.int32)
    hi = np.minimum(lo + 1, n - 1).astype(np.int32)
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=2) as e:
        e.set_tuning(F0, SR)
        e.set_windows(lo, hi)
        rows = e.process(_frames(n, 2, 6), 2)
        pk, av = e.window_stats()
        _check(pk, av, rows, lo, hi, "65536 windows")


def test_set_fft_size_clears_the_list(rfa):
    n = 4096
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=4) as e:
        e.set_tuning(F0, SR)
        e.set_windows([0, 100], [n - 1, 104])
        e.set_fft_size(n)  # not a change: the list stays
        e.process(_frames(n, 2, 3), 2, rows=False)
        assert e.window_stats()[0].shape == (2, 2)
        e.set_fft_size(2 * n)
        assert e.windows() is None
        e.process(_frames(2 * n, 2, 3), 2, rows=False)
        assert e.window_stats()[0].shape == (0, 0)
        e.set_windows([2 * n - 1], [2 * n - 1])  # a bin of the new size
        e.process(_frames(2 * n, 2, 3), 2, rows=False)
        assert e.window_stats()[0].shape == (2, 1)


@pytest.mark.parametrize("packed", [True, False])
def test_process_batches_returns_the_last_batch(rfa, packed):
    import torch
    n, fpb, nb = 8192, 6, 4
    gap = 0 if packed else 2 * 2 * n
    stride_b = fpb * 2 * n + gap
    raw = np.random.default_rng(31).integers(-128, 128, size=nb * stride_b, dtype=np.int8)
    dev = torch.from_numpy(raw.view(np.uint8).copy()).cuda()
    lo, hi = _cat(_whole(n), _random_windows(n, 80, 5000, 13), _grid(n, 211))
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=40) as a, rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=40) as b:
        for e in (a, b):
            e.set_tuning(F0, SR)
            e.set_windows(lo, hi)
        a.process_batches(dev.data_ptr(), nb, stride_b, fpb, 0, None)
        for k in range(nb):
            b.process(raw[k * stride_b:k * stride_b + fpb * 2 * n].tobytes(), fpb, rows=False)
        pa, pb = a.window_stats(), b.window_stats()
        assert pa[0].shape == (fpb, lo.size)
        _same_bits(pa[0], pb[0])
        _same_bits(pa[1], pb[1])
        assert a.window_stats_device()[2:] == (fpb, lo.size)


def test_pipelined_handle_gives_the_serial_bits(rfa):
    """rfa_set_pipelined: the window pass goes where the channel mean goes (the state stream);
    both getters join first."""
    import torch
    n, R = 8192, 16
    batches = (16, 16, 8, 8, 16, 5, 16)
    data = _frames(n, sum(batches), 19)
    dev = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    lo, hi = _cat(_whole(n), _random_windows(n, 100, 3000, 17), _grid(n, 97))
    kw = dict(avg="ema", ema_alpha=0.1, peak_hold=True, ring_rows=R)
    with rfa.SpectrumEngine(n, "blackman", "s8", **kw) as a, rfa.SpectrumEngine(n, "blackman", "s8", **kw) as b:
        b.set_pipelined(16)
        for e in (a, b):
            e.set_tuning(F0, SR)
            e.set_channel(F0 - 50_000, F0 + 90_000)
            e.set_windows(lo, hi)
        f = 0
        for k, nb in enumerate(batches):
            for e in (a, b):
                e.process_device(dev.data_ptr() + f * 2 * n, nb, 0, None)
            f += nb
            if k % 2 == 0 or k == len(batches) - 1:
                sa, sb = a.window_stats(), b.window_stats()
                assert sa[0].shape == (nb, lo.size)
                _same_bits(sa[0], sb[0])
                _same_bits(sa[1], sb[1])
        np.testing.assert_array_equal(a.channel_means(), b.channel_means())
        np.testing.assert_array_equal(a.peaks(), b.peaks())


# ------------------------------------------------------------------ 7. scanner batch forms
def test_scanner_batch_functions_equal_the_single_row_ones(rfa):
    """Each batch form equals its single-row function called after one-frame process calls on
    a second engine fed the same frames (the module's 4096-point engine of test_gpu_scanner)."""
    n, R, frames = 4096, 8, 6
    data = signals.frames_bytes(n, frames, "s8", seed=33, tones=((0.21, 0.3), (0.37, 0.01), (-0.2, 0.002)), noise=0.01)
    fb = 2 * n
    scan = (F0, SR, 2_000_000, 12_500, -60.0, sc.PEAK_OR_AVERAGE, -90.0, 6.0, 0, 10 ** 12)
    chans = [F0 + k * 100_000 for k in range(-14, 15)]
    with rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=R) as e, rfa.SpectrumEngine(n, "blackman", "s8", ring_rows=R) as one:
        for eng in (e, one):
            eng.set_tuning(F0, SR)
        single = {"level": [], "scan": [], "iem": []}
        for f in range(frames):
            one.process(data[f * fb:(f + 1) * fb], 1, rows=False)
            single["level"].append(sc.average_signal_level(one))
            single["scan"].append(sc.detect_signals_in_fft(one, *scan))
            single["iem"].append(sc.detect_iem_channels(one, chans, F0, SR, -55.0))
        assert any(single["scan"]) and any(single["iem"])
        sc.watch_average_level(e)
        e.process(data, frames, rows=False)
        # (rfa_row_window_stats adds the doubles in another order: the averages agree to one ulp)
        assert _within_one_ulp(sc.average_signal_levels(e), np.array(single["level"], np.float32))
        with pytest.raises(ValueError):
            sc.detect_iem_channels_in_batch(e, chans, F0, SR, -55.0)  # another list is set
        sc.watch_scan(e, F0, SR, 2_000_000, 12_500, 0, 10 ** 12)
        e.process(data, frames, rows=False)
        got = sc.detect_signals_in_batch(e, *scan)
        assert [[s.frequency for s in fr] for fr in got] == [[s.frequency for s in fr] for fr in single["scan"]]
        assert [[s.peak_strength for s in fr] for fr in got] == [[s.peak_strength for s in fr] for fr in single["scan"]]
        sc.watch_iem_channels(e, chans, F0, SR)
        e.process(data, frames, rows=False)
        got = sc.detect_iem_channels_in_batch(e, chans, F0, SR, -55.0)
        assert [[(d.channel_frequency, d.peak_strength) for d in fr] for fr in got] == \
               [[(d.channel_frequency, d.peak_strength) for d in fr] for fr in single["iem"]]
