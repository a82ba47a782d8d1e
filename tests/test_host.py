"""CPU: host-side logic of the path -- Scheduler/FileIQSource framing, the
retune shift arithmetic of the C-ABI, frame sharding, and the chunked /
segment-combined peak-hold + EMA updates checked against the sequential
restatement (oracle/processor.py)."""
import ctypes

import numpy as np
import pytest

import oracle
from oracle import processor
from rfanalyzer_amd import sharding, source


@pytest.fixture(scope="module")
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


# ---------------------------------------------------------------- framing (Scheduler.kt:252-279)
@pytest.mark.parametrize("n_bytes,n,packet,bps", [(4_000_000, 1024, 262_144, 2), (4_000_000, 262_144, 262_144, 2),
                                                  (10_000_000, 65_536, 262_144, 4), (262_143, 1024, 262_144, 2),
                                                  (3 * 262_144, 131_072, 262_144, 2)])
def test_framing_matches_restatement(n_bytes, n, packet, bps):
    ref = processor.file_frames(n_bytes, packet, bps, n)
    assert source.file_frames(n_bytes, n, packet, bps) == len(ref)
    if len(ref) > 1:
        assert source.frame_stride(n, packet, bps) == ref[1][0] - ref[0][0]


def test_file_source_replays_full_packets_only(tmp_path):
    path = tmp_path / "cap.iq"
    data = np.random.default_rng(0).integers(0, 256, 3 * 1000 + 17, dtype=np.uint8).tobytes()
    path.write_bytes(data)
    src = source.FileIQSource()
    src.init(str(path), 2_000_000, 100_000_000, packet_size=1000)
    assert src.open()
    got = []
    while True:
        p = src.getPacket()
        if p is None:
            break
        got.append(bytes(p))
        src.returnPacket(p)
    src.close()
    assert got == [data[i * 1000:(i + 1) * 1000] for i in range(3)]  # the 17-byte tail is dropped


# ---------------------------------------------------------------- retune (FftProcessor.kt:143,173,199)
def test_retune_offset_matches_kotlin_float_semantics(lib):
    rng = np.random.default_rng(5)
    cases = [(-3, 16, 16), (7, 1024, 2_000_000), (1, 65536, 20_000_000), (-123_456_789, 65536, 1000),
             (2 ** 40, 1 << 20, 1), (-(2 ** 40), 1 << 20, 1), (999, 1000, 1000), (0, 4096, 48_000)]
    cases += [(int(d), int(1 << rng.integers(6, 21)), int(rng.integers(1, 60_000_000)))
              for d in rng.integers(-10 ** 9, 10 ** 9, 500)]
    for d, n, sr in cases:
        assert lib.rfa_retune_offset(d, n, sr) == processor.retune_shift_offset(d, n, sr), (d, n, sr)


# ---------------------------------------------------------------- sharding
@pytest.mark.parametrize("frames,world", [(256, 2), (256, 8), (7, 3), (1, 4), (1000, 7)])
def test_frame_ranges_partition(frames, world):
    seen = []
    for r in range(world):
        s, e = sharding.frame_range(frames, r, world)
        assert 0 <= s <= e <= frames
        seen.extend(range(s, e))
    assert seen == list(range(frames))


def _rows(frames, n, seed, silent=()):
    rng = np.random.default_rng(seed)
    rows = (rng.standard_normal((frames, n)) * 10 - 40).astype(np.float32)
    for f in silent:
        rows[f, rng.integers(0, n, n // 3)] = -np.inf  # some bins of the frame are exact zeros
    return rows


@pytest.mark.parametrize("cuts", [[40], [10, 25], [1, 2, 3], [0, 39]])
def test_segment_combine_equals_sequential(cuts):
    rows = _rows(41, 64, 2, silent=(5, 6, 20, 40))
    alpha = 0.25
    exp = processor.ema_batch(rows, alpha)
    bounds = [0] + sorted(set(cuts)) + [rows.shape[0]]
    segs = [sharding.ema_partial(rows[a:b], alpha) for a, b in zip(bounds, bounds[1:]) if b > a]
    got = sharding.ema_combine(None, segs)
    fin = np.isfinite(exp)
    assert np.array_equal(np.isneginf(got), np.isneginf(exp))
    np.testing.assert_allclose(got[fin], exp[fin], rtol=0, atol=1e-4)
    parts = [rows[a:b].max(0) for a, b in zip(bounds, bounds[1:]) if b > a]
    np.testing.assert_array_equal(sharding.peak_combine(parts), rows.max(0))


def _chunk_summaries(rows, alpha, chunk):
    """numpy restatement of state_partial_kernel (fft_kernels.hip), float32."""
    al, keep = np.float32(alpha), np.float32(1 - np.float32(alpha))
    out = []
    for c0 in range(0, rows.shape[0], chunk):
        pk = np.full(rows.shape[1], -np.inf, np.float32)
        emi = np.full(rows.shape[1], -np.inf, np.float32)
        am = np.ones(rows.shape[1], np.float32)
        b = np.zeros(rows.shape[1], np.float32)
        restart = np.zeros(rows.shape[1], bool)
        with np.errstate(invalid="ignore"):
            for x in rows[c0:c0 + chunk]:
                pk = np.maximum(pk, x)
                emi = np.where(np.isfinite(emi), emi + al * (x - emi), x).astype(np.float32)
                restart |= ~np.isfinite(x)
                am = (am * keep).astype(np.float32)
                b = (b + al * (x - b)).astype(np.float32)
        out.append((pk, np.where(restart, np.float32(-1), am), b, emi))
    return out


def _combine(state_pk, state_em, summaries):
    """numpy restatement of state_combine_kernel."""
    pk, em = state_pk.copy(), state_em.copy()
    for p_pk, a, b, emi in summaries:
        pk = np.maximum(pk, p_pk)
        with np.errstate(invalid="ignore"):
            em = np.where(~np.isfinite(em) | (a < 0), emi, a * em + b).astype(np.float32)
    return pk, em


@pytest.mark.parametrize("chunk", [1, 3, 8, 50])
@pytest.mark.parametrize("init", ["fresh", "warm"])
def test_chunked_state_update_equals_sequential(chunk, init):
    rows = _rows(50, 256, 3, silent=(0, 17, 18, 33))
    alpha = 0.1
    pk0 = np.full(256, -999999, np.float32)
    em0 = np.full(256, -np.inf, np.float32) if init == "fresh" else _rows(1, 256, 9)[0]
    pk, em = _combine(pk0, em0, _chunk_summaries(rows, alpha, chunk))
    np.testing.assert_array_equal(pk, np.maximum(pk0, rows.max(0)))
    exp = processor.ema_batch(rows, alpha, None if init == "fresh" else em0)
    assert np.array_equal(np.isneginf(em), np.isneginf(exp))
    fin = np.isfinite(exp)
    np.testing.assert_allclose(em[fin], exp[fin], rtol=0, atol=2e-4)


def test_device_less_calls_fail_loudly(lib):
    """No CPU fallback: creating a handle without a HIP device is an error status."""
    import rfanalyzer_amd
    if rfanalyzer_amd.device_count() > 0:
        pytest.skip("a HIP device is visible")
    with pytest.raises(rfanalyzer_amd.RfaError):
        rfanalyzer_amd.SpectrumEngine(1024, "blackman", "s8")


def test_oracle_is_not_imported_by_the_product_package():
    import pathlib
    pkg = pathlib.Path(__file__).resolve().parents[1] / "rfanalyzer_amd"
    for f in pkg.rglob("*.py"):
        text = f.read_text()
        assert "import oracle" not in text and "from oracle" not in text, f
    assert oracle.__file__  # the checker itself stays importable for tests
