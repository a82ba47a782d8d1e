"""CPU: the host side of tests/test_gpu_ddc_paths.py, so that the GPU module cannot fail for a
reason of its own -- the tile-plan query (rfa_ddc_tile_plan, no device needed) on hand-computed
plans, the plan property of every case in the table (tests/ddc_paths.py), the packet sequences,
and the vectorised oracle the GPU is held against tied to the literal per-sample loops on the
cases' own packets."""
import ctypes

import numpy as np
import pytest

import ddc_paths as dp
from oracle import demod as od
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


# ---------------------------------------------------------------- the query itself

def test_tile_plan_of_the_smallest_filter_by_hand():
    """T = 1, D = 1, no table: every P up to 256 fits; lanes per CU = P * min(LDS blocks,
    32 waves / waves per block) peaks at 2048 for P = 64, 128, 192 and 256 and the largest wins.
    LDS: span = (P - 1) * D + 1 + T = 257 samples of 8 B in rows of one, plus one 16-byte group
    of taps."""
    assert demod.tile_plan(1, 1, 1, 0) == {"P": 256, "threads": 256, "KC": 1, "chunks": 1, "pad": 0, "row": 1,
                                           "lds_bytes": 257 * 8 + 16}


def test_tile_plan_lds_bytes_by_hand():
    """T = 33, D = 2, L = 443 (pad layout): span = 255 * 2 + 1 + 33 = 544 samples = 272 rows of
    pitch 3, 8 B each; 33 taps padded to 36 floats; the table padded to 444 entries of 8 B."""
    want = 272 * 3 * 8 + 36 * 4 + 444 * 8
    assert demod.tile_plan(33, 1, 2, 443) == {"P": 256, "threads": 256, "KC": 33, "chunks": 1, "pad": 1, "row": 2,
                                              "lds_bytes": want}
    # the same filter on the linear layout (D = 3): 255 * 3 + 34 = 799 samples = 267 rows of 3
    assert demod.tile_plan(33, 1, 3, 443)["lds_bytes"] == 267 * 3 * 8 + 36 * 4 + 444 * 8
    # polyphase 5 / 6: rows of one sample, span = ceil(255 * 6 / 5) + 1 + 40 = 347
    assert demod.tile_plan(40, 5, 6, 0) == {"P": 256, "threads": 256, "KC": 40, "chunks": 1, "pad": 0, "row": 1,
                                            "lds_bytes": 347 * 8 + 40 * 4}


def test_tile_plan_argument_errors():
    L = _lib.lib()
    out = (ctypes.c_int32 * 7)()
    for args in [(0, 1, 1, 0), (1, 0, 1, 0), (1, 1, 0, 0), (1, 1, 1, -1), (-5, 1, 1, 0)]:
        assert L.rfa_ddc_tile_plan(*args, out) == _lib.RFA_ERR_INVALID, args
    assert L.rfa_ddc_tile_plan(33, 1, 2, 0, None) == _lib.RFA_ERR_INVALID
    assert L.rfa_ddc_tile_plan(33, 1, 2, 10241, out) == _lib.RFA_ERR_UNSUPPORTED   # as rfa_ddc_set_frequencies
    assert L.rfa_ddc_tile_plan(33, 1, 2, 10240, out) == _lib.RFA_OK
    with pytest.raises(_lib.RfaError):
        demod.tile_plan(0, 1, 1, 0)


def test_header_names_the_plan_fields_in_the_binding_order():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rfa.h")).read()
    fields = dict(re.findall(r"RFA_DDC_PLAN_([A-Z_]+) = (\d+)", text))
    order = ["OUTPUTS", "THREADS", "CHUNK_TAPS", "CHUNKS", "PAD", "ROW", "LDS_BYTES", "FIELDS"]
    assert [int(fields[k]) for k in order] == list(range(8))
    assert len(demod.TILE_PLAN_FIELDS) == int(fields["FIELDS"])


# ---------------------------------------------------------------- the case table

def test_channel_offsets_give_the_table_lengths():
    for L, off in dp.OFFSET_OF_LENGTH.items():
        mf = od.mix_frequency(dp.CENTER, dp.CENTER + off, dp.SR)
        for fmt in ("s8", "u8", "s16"):
            assert len(od.mixer_table(dp.FMT[fmt], dp.SR, mf)[0]) == L
            assert dp.table_length(fmt, off) == L
    assert dp.table_length("f32", 130_000) == 0


@pytest.mark.parametrize("case", dp.ALL, ids=lambda c: c.id)
def test_case_has_its_plan_property_and_packet_kinds(case):
    plan = case.plan()                                   # asserts the row's property under every table of the case
    sizes = case.sizes()
    assert dp.packet_kinds(sizes, case.T, plan["P"], 1, case.D) >= dp.required_kinds(case.T), sizes
    assert all(k < len(sizes) for k, _ in case.tune)
    if plan["chunks"] > 1:
        assert 2 * case.T <= sum(sizes) <= 3 * case.T
    else:
        assert sum(sizes) < 80_000


def test_every_row_and_axis_is_in_the_table():
    assert {(c.T, c.D) for c in dp.BASE} == set(dp.ROWS) and all(c.fmt == "s8" and c.byte_offset is None
                                                                 for c in dp.BASE)
    for fmt in ("u8", "s16", "f32"):
        rows = {(c.T, c.D) for c in dp.FORMATS if c.fmt == fmt}
        assert {(33, 2), (33, 3), (8, 64)} < rows and any(dp.plan_of(T, D, 0)["chunks"] > 1 for T, D in rows)
    for fmt, offs in (("s8", {2, 4, 6, 8}), ("u8", {2, 4, 6, 8}), ("s16", {4, 8, 12, 16})):
        for row in ((33, 2), (33, 3), (5, 1), (14000, 3)):
            assert {c.byte_offset for c in dp.ALIGNMENTS if c.fmt == fmt and (c.T, c.D) == row} == offs
        # three offsets off the four-sample grid, one on it
        assert sorted(o % (4 * dp.SB[fmt]) != 0 for o in offs) == [False, True, True, True]
    for D in (2, 3):
        for off in (None, 2):
            got = {dp.LENGTH_OF_OFFSET[c.tune[0][1]] for c in dp.TABLES
                   if c.fmt == "s8" and c.D == D and c.byte_offset == off}
            assert got == {1, 2, 3, 4, 5, 443, 499}
    assert all([dp.LENGTH_OF_OFFSET[o] for _, o in c.tune] == [3, 443, 3] for c in dp.RETUNES)


def test_the_limit_case_asks_for_the_whole_lds():
    """(14000, 3) with a 500-entry table needs exactly the 160 KiB a workgroup can have."""
    assert dp.plan_of(14000, 3, 500)["lds_bytes"] == dp.LDS_LIMIT


@pytest.mark.parametrize("fmt,sr,out,byte_offset", dp.POLY_CASES, ids=lambda v: str(v))
def test_polyphase_case_plans_and_packets(fmt, sr, out, byte_offset):
    ref = od.ResamplerFrontEnd(dp.FMT[fmt], sr, out)
    i, d, t = dp.POLYPHASE[(sr, out)]
    assert (ref.rs.I, ref.rs.D, ref.rs.nt) == (i, d, t)
    plan = dp.poly_plan(fmt, sr, out)
    sizes = dp.poly_sizes(fmt, sr, out)
    assert dp.packet_kinds(sizes, t, plan["P"], i, d, polyphase=True) >= dp.required_kinds(t), sizes
    assert sum(sizes) < 100_000
    if byte_offset is not None:
        assert byte_offset % (4 * dp.SB[fmt]) != 0


# ---------------------------------------------------------------- the oracle against the literal loops

@pytest.mark.parametrize("case", [c for c in dp.BASE + dp.FORMATS if c.T <= 33], ids=lambda c: c.id)
def test_vectorised_oracle_equals_the_literal_loops(case):
    """FirDecimator.filter (what the GPU is compared with) against FirFilter's loop as written
    (filter_literal) and against the C loop (CFrontEnd), packet by packet."""
    outs, ref = dp.oracle_run(case)
    raw = dp.case_raw(case)
    taps = dp.fir_taps(case.T)
    cfe = od.CFrontEnd(dp.FMT[case.fmt], dp.SR, max(1, dp.SR // case.D), taps=taps, decimation=case.D)
    for got, want in zip(dp.run_front_end(cfe, case, raw), outs):
        _same(got[0], want[0])
        _same(got[1], want[1])
    lit = od.FirDecimator(taps, case.D)
    mixer = od.FrontEnd(dp.FMT[case.fmt], dp.SR, max(1, dp.SR // case.D), taps=taps[:1], decimation=1)

    def literal(chunk):
        if case.fmt == "f32":
            v = chunk.view(np.float32)
            return lit.filter_literal(v[0::2], v[1::2])
        re, im = od.mix(mixer.fmt, chunk, mixer.cos_t, mixer.sin_t, mixer.cosine_index)
        mixer.cosine_index = (mixer.cosine_index + len(re)) % len(mixer.cos_t)
        return lit.filter_literal(re, im)

    for got, want in zip(dp.run_front_end(mixer, case, raw, process=literal), outs):
        _same(got[0], want[0])
        _same(got[1], want[1])
    total = sum(case.sizes())
    n_out = sum(len(o[0]) for o in outs)
    assert n_out == dp.outputs_after(total, 1, case.D)
    if case.D == 1:                                                  # first output at input 1, then one per input
        fed = np.cumsum(case.sizes())
        assert list(np.cumsum([len(o[0]) for o in outs])) == [max(0, n - 1) for n in fed]
    if case.fmt != "f32":
        assert ref.cosine_index == total % len(ref.cos_t)


@pytest.mark.parametrize("sr,out", [(2_400_000, 2_000_000), (48_000, 44_100)])
def test_resample_equals_resample_literal(sr, out):
    i, d, t = dp.POLYPHASE[(sr, out)]
    sizes = dp.poly_sizes("f32", sr, out)
    x = np.random.default_rng(sr).standard_normal((2, sum(sizes))).astype(np.float32)
    a, b = od.RationalResampler(i, d, max_taps=500), od.RationalResampler(i, d, max_taps=500)
    assert (a.I, a.D, a.nt) == (i, d, t)
    pos = n_out = 0
    for n in sizes:
        got, want = a.resample(x[0, pos:pos + n], x[1, pos:pos + n]), b.resample_literal(x[0, pos:pos + n],
                                                                                         x[1, pos:pos + n])
        _same(got[0], want[0])
        _same(got[1], want[1])
        pos += n
        n_out += len(got[0])
    assert n_out == dp.outputs_after(pos, i, d, polyphase=True)
