"""GPU: every path of the channelizer tile (rfanalyzer_amd/csrc/channelizer.hip: pfb_kernel,
pfb_rational_kernel and their tuned siblings) -- every first-stage radix and every
pair of consecutive radices, every NT staged and unstaged, the rational plans A, B and C with tap
rows by phase and by time, the largest LDS request the kernels can make and the edges of the
definition (T = 1, T < M, D = 1, D = M, T = 16 M).  The cases, the plan each must get and the two
calls each is fed in are tests/pfb_paths.py; tests/test_pfb_paths_host.py checks all of that, and
the references used here, on the CPU.

Per case: (a) the plan the library reports (rfa_pfb_tile_plan) has the case's property; (b) every
output of every channel of both calls equals the float32 statement-for-statement model
(tests/pfb_model.py) bit for bit; (c) it lies within the derived worst-case bound of the float64
restatement (pfb_ref.bound / pfb_rational_ref.bound), the observed ratio going to the session
summary; (d) one call gives the bits of the two calls; (e) where M <= 256 a selection with
duplicates -- more slots * NT than one pass of the store's 256 threads where M allows -- gives the
rows of the all-channels run and leaves the padding alone; (f) at NT = 4, 2 and 1 the tuned kernel
equals the untuned twin's rows put through pfb_tuning_ref.rot, for steps 0, +-1 and q - 1."""
import functools

import numpy as np
import pytest

import golden_util as gu
import pfb_paths as pp
import pfb_tuning_ref as tref
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

SB = pp.SB
SENTINEL = 12345.0


def _make(case):
    taps = pp.data(case)[0]
    return (demod.Channelizer(case.fmt, case.M, case.D, taps) if case.L is None
            else demod.Channelizer.rational(case.fmt, case.M, case.L, case.D, taps))


def _feed(ch, case, sizes):
    """The case's stream through ``ch`` in calls of ``sizes`` samples: one [selected, n] complex64 per
    call, every call's count checked against the count rule."""
    raw = pp.data(case)[1]
    sb, parts, pos = SB[case.fmt], [], 0
    for s in sizes:
        want = case.count(pos + s) - case.count(pos)
        assert ch.max_outputs(s) == want
        out = ch.process(raw[pos * sb:(pos + s) * sb])
        assert all(o.size == want for o in out), (s, want)
        parts.append(np.stack(out))
        pos += s
    assert pos * sb == raw.size
    return parts


@functools.lru_cache(maxsize=None)
def _two_calls(case):
    """All channels of the case's two calls on the device; read only."""
    with _make(case) as ch:
        assert ch.plan()["radices"] == case.plan()["radices"]
        parts = _feed(ch, case, case.sizes())
    for a in parts:
        a.setflags(write=False)
    return tuple(parts)


def _bits(got, want, what):
    """Equal as int32 views; a mismatch names how many values differ, where the first one sits and how
    far the values are apart."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    g = np.ascontiguousarray(got).view(np.int32).reshape(got.shape + (2,))
    w = np.ascontiguousarray(want).view(np.int32).reshape(want.shape + (2,))
    bad = np.argwhere(g != w)
    if bad.size:
        k, n, part = (int(v) for v in bad[0])
        err = float(np.abs(got.astype(np.complex128) - want).max())
        raise AssertionError(f"{what}: {len(bad)} of {g.size} floats differ; first at channel {k}, output {n}, "
                             f"{'re' if part == 0 else 'im'}: {got[k, n]!r} != {want[k, n]!r}; "
                             f"channels {sorted(set(bad[:, 0].tolist()))[:8]}, outputs "
                             f"{sorted(set(bad[:, 1].tolist()))[:8]}; max |diff| {err:.3e}")


@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_every_output_equals_the_model_bit_for_bit(rfa, case):
    case.plan()                                          # (a)
    got, want = _two_calls(case), pp.model_run(case)
    assert [g.shape for g in got] == [(case.M, n) for n in case.outputs()]
    for call, (g, w) in enumerate(zip(got, want)):       # (b)
        _bits(g, w, f"{case.id} ({case.why}) call {call}")


@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_every_output_within_the_bound_of_the_float64_restatement(rfa, case):
    y = np.concatenate(_two_calls(case), axis=1)
    assert np.all(np.isfinite(y.view(np.float32)))
    r = pp.ratio(y, case)                                # (c)
    line = f"channelizer paths {case.id}: max err / bound = {r:.4f} over {y.size} outputs"
    gu.NOTES.append(line)
    print(line)
    assert r <= 1.0, (case.id, r)


@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_one_call_equals_the_two_calls(rfa, case):
    with _make(case) as ch:
        whole, = _feed(ch, case, [sum(case.sizes())])
    _bits(whole, np.concatenate(_two_calls(case), axis=1), f"{case.id} one call")       # (d)


def _device_call(ch, case, raw, n_sel, pad=3):
    """One rfa_pfb_process call on torch tensors whose rows are ``pad`` floats longer than the output
    count and prefilled with a sentinel: [n_sel, n] complex64, the padding checked."""
    import torch
    dev = torch.device("cuda", 0)
    n = ch.max_outputs(raw.size // SB[case.fmt])
    buf = torch.from_numpy(np.array(raw)).to(dev)
    re = torch.full((n_sel, n + pad), SENTINEL, dtype=torch.float32, device=dev)
    im = torch.full((n_sel, n + pad), SENTINEL, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    assert ch.process_tensor(buf, re, im) == n
    torch.cuda.synchronize(dev)
    re, im = re.cpu().numpy(), im.cpu().numpy()
    assert np.all(re[:, n:] == SENTINEL) and np.all(im[:, n:] == SENTINEL), "padding written"
    out = np.empty((n_sel, n), np.complex64)
    out.real, out.imag = re[:, :n], im[:, :n]
    return out


@pytest.mark.parametrize("case", [c for c in pp.ALL if c.M <= 256], ids=lambda c: c.id)
def test_selection_rows_equal_the_all_channels_run_and_padding_is_untouched(rfa, case):
    sel = pp.selection(case)
    raw, sb = pp.data(case)[1], SB[case.fmt]
    s1, _ = case.sizes()
    full = _two_calls(case)
    with _make(case) as ch:
        ch.set_channels(sel)
        assert ch.channels == sel
        for call, chunk in enumerate((raw[:s1 * sb], raw[s1 * sb:])):                   # (e)
            got = _device_call(ch, case, chunk, len(sel))
            _bits(got, full[call][sel], f"{case.id} selection call {call}")


@pytest.mark.parametrize("case", pp.TUNED, ids=lambda c: c.id)
def test_tuned_store_equals_the_rotated_untuned_twin(rfa, case):
    q = pp.TUNED_Q
    sel, steps = [3, case.M - 1, 0, 3], [0, 1, -1, q - 1]
    full = np.concatenate(_two_calls(case), axis=1)
    with _make(case) as ch:
        ch.set_channels(sel)
        ch.set_tuning(q, steps)
        assert ch.tuning == (q, steps)
        got = np.concatenate(_feed(ch, case, case.sizes()), axis=1)                     # (f)
    assert got.shape == (4, full.shape[1])
    for j, (k, m) in enumerate(zip(sel, steps)):
        tref.same(got[j], tref.rot(full[k], q, m))
        if m == 0:
            np.testing.assert_array_equal(got[j].view(np.int32), full[k].view(np.int32))
        else:
            assert not np.array_equal(got[j], full[k]), (case.id, j)


@pytest.mark.parametrize("case", [c for c in pp.ALL if c.Th == 1], ids=lambda c: c.id)
def test_one_tap_channel_0_is_the_product_itself(rfa, case):
    """T = 1 (rational: Tp = 1): no history is kept and no history kernel runs; u has one non-zero
    residue and every stage adds zeros to it, so channel 0 is float32(h) * x[newest] exactly."""
    taps, _, x = pp.data(case)
    y = np.concatenate(_two_calls(case), axis=1)
    n = np.arange(y.shape[1])
    if case.L is None:
        h, newest = taps[0], n * case.D + case.D - 1
    else:
        h, newest = taps[(n * case.D) % case.L], n * case.D // case.L
    xs = x[newest]
    assert np.array_equal(y[0].real, h * xs.real.astype(np.float32))
    assert np.array_equal(y[0].imag, h * xs.imag.astype(np.float32))
