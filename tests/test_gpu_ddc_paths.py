"""GPU: every path of the front-end FIR tile (rfanalyzer_amd/csrc/ddc_fir_tile.inc, the body of
ddc_fir_kernel and ddc_bank_kernel), not only the ones the app's rates take.

The case table is tests/ddc_paths.py: explicit-taps filters (rfa_ddc_create_fir) chosen for the
tile plan they get -- LDS layout, tile shape, tap chunks, T = 1, D = 1, D > T -- crossed with
the input formats, the raw pointer's alignment (four-sample loads or the per-sample loop) and
mixer tables of 1 to 499 entries, plus near-unity polyphase ratios and a bank whose slots have
tables of 1, 3 and 443 entries.  Each case asserts its plan property through
rfa_ddc_tile_plan before it runs, feeds one handle a ragged packet sequence and a second one
the whole buffer, and compares bit for bit with oracle/demod.py (tied to the literal
per-sample loops in tests/test_ddc_paths_host.py)."""
import numpy as np
import pytest

import ddc_paths as dp
from oracle import demod as od
from rfanalyzer_amd import demod
from test_gpu_demod import _Dev, _same

pytestmark = pytest.mark.gpu


class _DeviceFeed:
    """process(chunk) through rfa_ddc_process on device buffers: every packet gets a raw buffer
    of exactly byte_offset + its own bytes and starts byte_offset into it."""

    def __init__(self, fe, byte_offset, sample_bytes, largest):
        self.fe, self.off, self.sb = fe, byte_offset, sample_bytes
        self.cap = fe.max_outputs(largest)
        self.re, self.im = _Dev(4 * self.cap), _Dev(4 * self.cap)

    def process(self, chunk):
        n = chunk.size // self.sb
        if n == 0:
            assert self.fe.process_device(0, 0, self.re.ptr.value, self.im.ptr.value, self.cap) == 0
            return np.zeros(0, np.float32), np.zeros(0, np.float32)
        raw = _Dev(self.off + chunk.size)
        raw.put(np.concatenate([np.full(self.off, 0x5a, np.uint8), chunk]))
        got = self.fe.process_device(raw.ptr.value + self.off, n, self.re.ptr.value, self.im.ptr.value, self.cap)
        self.fe.synchronize()
        out = self.re.get(got), self.im.get(got)
        raw.free()
        return out

    def free(self):
        self.re.free(), self.im.free()


def _feed(fe, byte_offset, sample_bytes, largest):
    """(process function, cleanup) of a front end on the host path or at a device byte offset."""
    if byte_offset is None:
        return fe.process, lambda: None
    feed = _DeviceFeed(fe, byte_offset, sample_bytes, largest)
    return feed.process, feed.free


def _same_outputs(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g[0]) == len(w[0]), (k, len(g[0]), len(w[0]))
        _same(g[0], w[0])
        _same(g[1], w[1])


def _same_mixer(fe, ref, fmt):
    c, s, mf, ci = fe.mixer()
    if fmt == "f32":
        assert len(c) == 0 and ci == 0
        return
    _same(c, ref.cos_t)
    _same(s, ref.sin_t)
    assert (mf, ci) == (ref.cos_freq, ref.cosine_index)


def _run_case(case):
    case.plan()                                       # the row's property, under every table the case runs with
    want, ref = dp.oracle_run(case)
    raw, sizes, taps = dp.case_raw(case), case.sizes(), dp.fir_taps(case.T)
    sb = dp.SB[case.fmt]
    fe = demod.FrontEnd(case.fmt, dp.SR, max(1, dp.SR // case.D), _fir=(taps, case.D))
    assert fe.ratio() == (1, case.D, case.T)
    process, done = _feed(fe, case.byte_offset, sb, max(sizes))
    got = dp.run_front_end(fe, case, raw, process=process)
    done()
    assert len(fe.mixer()[0]) == case.lengths()[-1]   # the table the plan was asserted with is the handle's own
    _same_outputs(got, want)
    _same_mixer(fe, ref, case.fmt)
    fe.close()
    if len(case.tune) == 1:                           # one call for the whole buffer: the same bits
        whole = demod.FrontEnd(case.fmt, dp.SR, max(1, dp.SR // case.D), _fir=(taps, case.D))
        whole.set_frequencies(dp.CENTER, dp.CENTER + case.tune[0][1])
        process, done = _feed(whole, case.byte_offset, sb, sum(sizes))
        g = process(raw)
        done()
        _same(g[0], np.concatenate([w[0] for w in want]))
        _same(g[1], np.concatenate([w[1] for w in want]))
        _same_mixer(whole, ref, case.fmt)
        whole.close()


@pytest.mark.parametrize("case", dp.BASE, ids=lambda c: c.id)
def test_every_plan_row_s8_aligned(rfa, case):
    _run_case(case)


@pytest.mark.parametrize("case", dp.FORMATS, ids=lambda c: c.id)
def test_formats(rfa, case):
    _run_case(case)


@pytest.mark.parametrize("case", dp.ALIGNMENTS, ids=lambda c: c.id)
def test_pointer_alignment(rfa, case):
    """Byte offsets off the four-sample grid take the per-sample loop, the one on it the
    four-sample loads with a buffer that ends at the call's last sample."""
    _run_case(case)


@pytest.mark.parametrize("case", dp.TABLES, ids=lambda c: c.id)
def test_mixer_table_lengths(rfa, case):
    """Tables of 1 to 5 entries wrap inside one group of four; 443 and 499 are the long walk."""
    _run_case(case)


@pytest.mark.parametrize("case", dp.RETUNES, ids=lambda c: c.id)
def test_retune_between_packets_restarts_the_cosine_index(rfa, case):
    _run_case(case)


# ---------------------------------------------------------------- polyphase

@pytest.mark.parametrize("fmt,sr,out,byte_offset", dp.POLY_CASES, ids=lambda v: str(v))
def test_polyphase_ratios(rfa, fmt, sr, out, byte_offset):
    """Near-unity ratios (lanes share or skip inputs unevenly, taps from the lane's phase row in
    global memory) and 1 / 1250 (a polyphase handle with one phase, even LDS row, small P)."""
    dp.poly_plan(fmt, sr, out)
    sizes = dp.poly_sizes(fmt, sr, out)
    raw = dp.raw_bytes(fmt, sum(sizes), out)
    ref = od.ResamplerFrontEnd(dp.FMT[fmt], sr, out)
    fe = demod.FrontEnd(fmt, sr, out, resampler=True)
    whole = demod.FrontEnd(fmt, sr, out, resampler=True)
    for f in (ref, fe, whole):
        f.set_frequencies(dp.CENTER, dp.poly_channel(sr))
    assert fe.ratio() == (ref.rs.I, ref.rs.D, ref.rs.nt) == dp.POLYPHASE[(sr, out)]
    _same(fe.taps, ref.rs.proto)
    process, done = _feed(fe, byte_offset, dp.SB[fmt], max(sizes))
    want, got = [], []
    for chunk in dp.chunks(raw, fmt, sizes):
        want.append(ref.process(chunk))
        got.append(process(chunk))
    done()
    _same_outputs(got, want)
    _same_mixer(fe, ref, fmt)
    process, done = _feed(whole, byte_offset, dp.SB[fmt], sum(sizes))
    g = process(raw)
    done()
    _same(g[0], np.concatenate([w[0] for w in want]))
    _same(g[1], np.concatenate([w[1] for w in want]))
    fe.close(), whole.close()


# ---------------------------------------------------------------- bank

@pytest.mark.parametrize("byte_offset", [None, 2])
def test_bank_slots_with_tables_of_1_3_and_443_entries(rfa, byte_offset):
    """One launch, three table lengths (the LDS share of the table is the longest's): every slot
    equals its single handle and the oracle."""
    offsets = [dp.OFFSET_OF_LENGTH[L] for L in (1, 3, 443)]
    sr, out = dp.SR, 96_000
    bank = demod.FrontEndBank("s8", sr, out, 3)
    bank.set_frequencies(dp.CENTER, [dp.CENTER + o for o in offsets])
    assert [bank.channel(k)[1] for k in range(3)] == [1, 3, 443]
    i, d, t = bank.ratio()
    plan = demod.tile_plan(t, i, d, 443)
    assert plan["chunks"] == 1 and plan["pad"] == 0 and plan["row"] == 25
    sizes = tuple(dp.packets(t, plan["P"], i, d))
    raw = dp.raw_bytes("s8", sum(sizes), 96)
    fes, refs = [], []
    for o in offsets:
        fes.append(demod.FrontEnd("s8", sr, out))
        refs.append(od.FrontEnd(od.IN_S8, sr, out))
        for f in (fes[-1], refs[-1]):
            f.set_frequencies(dp.CENTER, dp.CENTER + o)
    cap = bank.max_outputs(max(sizes))
    re, im = _Dev(4 * 3 * cap), _Dev(4 * 3 * cap)
    for chunk in dp.chunks(raw, "s8", sizes):
        if byte_offset is None:
            b_re, b_im = bank.process(chunk)
        elif chunk.size == 0:
            assert bank.process_device(0, 0, re.ptr.value, im.ptr.value, cap) == 0
            b_re = b_im = np.zeros((3, 0), np.float32)
        else:
            buf = _Dev(byte_offset + chunk.size)
            buf.put(np.concatenate([np.zeros(byte_offset, np.uint8), chunk]))
            n = bank.process_device(buf.ptr.value + byte_offset, chunk.size // 2, re.ptr.value, im.ptr.value, cap)
            bank.synchronize()
            b_re, b_im = (x.get(3 * cap).reshape(3, cap)[:, :n] for x in (re, im))
            buf.free()
        for k, (fe, ref) in enumerate(zip(fes, refs)):
            g, w = fe.process(chunk), ref.process(chunk)
            for a, b, c in ((b_re[k], g[0], w[0]), (b_im[k], g[1], w[1])):
                _same(np.ascontiguousarray(a), b)
                _same(b, c)
            assert bank.channel(k) == (ref.cos_freq, len(ref.cos_t), ref.cosine_index)
    re.free(), im.free()
    bank.close()
    for fe in fes:
        fe.close()
