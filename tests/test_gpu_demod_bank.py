"""GPU: the demodulator bank (rfa_demod_bank_*, demod.DemodulatorBank, and demod.ReceiverBank
on it).  Slot k of a bank must equal, bit for bit, a single ``demod.Demodulator`` given the same
settings and the same calls: audio is compared as int32 bit patterns (AM's silent first packet
gives NaN, which has to match too; FM is exact as well, both sides run the same device atan2),
and ``state(k)`` and ``taps(k, .)`` are compared after every call.  Every slot has its own
noise input."""
import functools

import numpy as np
import pytest

from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

F32 = np.float32
PACKETS = [1, 0, 2, 26, 27, 28, 181, 182, 363, 1000, 4097]     # tests/test_gpu_demod_chain.py's list
TOTAL = sum(PACKETS)
MIXED = ["am", "nfm", "wfm", "lsb", "usb", "cw", "off"]
RING = 8                                                       # kRecRing of csrc/demod.hip


@functools.lru_cache(maxsize=None)
def noise(seed, n=TOTAL):
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    re = (0.3 * rng.standard_normal(n)).astype(F32)
    im = (0.3 * rng.standard_normal(n)).astype(F32)
    re.setflags(write=False)
    im.setflags(write=False)
    return re, im


def inputs(k_count, n=TOTAL, seeds=None):
    seeds = list(range(k_count)) if seeds is None else seeds
    re = np.stack([noise(s, n)[0] for s in seeds])
    im = np.stack([noise(s, n)[1] for s in seeds])
    return re, im


def same(got, want, what=""):
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, (what, bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


class Pair:
    """A bank and the single handles it has to equal; ``slot_of[j]`` are the bank slots that
    handle j stands for (one each, except in the 300-slot test)."""

    def __init__(self, modes, slot_of=None, handle_modes=None):
        self.bank = demod.DemodulatorBank(modes)
        self.handles = [demod.Demodulator(m) for m in (modes if handle_modes is None else handle_modes)]
        self.slot_of = [[k] for k in range(len(modes))] if slot_of is None else slot_of

    def close(self):
        self.bank.close()
        for h in self.handles:
            h.close()

    def same_settings(self, what=""):
        for j, h in enumerate(self.handles):
            for k in self.slot_of[j]:
                assert self.bank.mode(k) == h.demodulationMode, (what, k)
                assert self.bank.channel_width(k) == h.channelWidth, (what, k)
                same(np.array(self.bank.state(k), F32), np.array(h.state(), F32), f"{what} state of slot {k}")
                for which in demod.TAPS:
                    b_re, b_im, b_dec = self.bank.taps(k, which)
                    h_re, h_im, h_dec = h.taps(which)
                    assert b_dec == h_dec, (what, k, which)
                    same(b_re, h_re, f"{what} {which} taps of slot {k}")
                    same(b_im, h_im, f"{what} {which} taps of slot {k} (im)")

    def check(self, got, h_re, h_im, ps, what=""):
        """``got``: the bank's K audio arrays of a call; the handles get row j of h_re / h_im."""
        want = []
        for j, h in enumerate(self.handles):
            w = h.process(h_re[j], h_im[j], ps)
            want.append(w)
            for k in self.slot_of[j]:
                same(got[k], w, f"{what} audio of slot {k}")
        self.same_settings(what)
        return want

    def call(self, re, im, ps=None, what=""):
        """One call on the bank and on every handle (one handle per slot)."""
        assert self.bank.max_outputs(re.shape[1]) == [h.max_outputs(re.shape[1]) for h in self.handles]
        got = self.bank.process(re, im, ps)
        assert len(got) == self.bank.n_channels
        self.check(got, re, im, ps, what)
        return got


@pytest.fixture
def pair(rfa):
    made = []

    def _pair(*a, **kw):
        p = Pair(*a, **kw)
        made.append(p)
        return p

    yield _pair
    for p in made:
        p.close()


def chunks(re, im, sizes):
    pos = 0
    for n in sizes:
        yield re[:, pos:pos + n], im[:, pos:pos + n]
        pos += n


# ------------------------------------------------------------------ 1: mixed modes, ragged calls

def test_mixed_modes_ragged_calls(pair):
    p = pair(MIXED)
    re, im = inputs(len(MIXED))
    off = MIXED.index("off")
    state0 = p.bank.state(off)
    tiles = set()
    for i, (c_re, c_im) in enumerate(chunks(re, im, PACKETS)):
        got = p.call(c_re, c_im, what=f"call {i} ({PACKETS[i]})")
        assert got[off].size == 0
        tiles.add(tuple(-(-g.size // 256) for g in got[:off]))
    assert any(len(set(t)) > 1 for t in tiles)       # slots own different numbers of audio tiles: early exit ran
    same(np.array(p.bank.state(off), F32), np.array(state0, F32), "off slot's state")
    assert p.bank.taps(off, "user")[0].size == 0     # no packet ever built its filter


# ------------------------------------------------------------------ 2: one call, many packets

@pytest.mark.parametrize("ps", [1, 27, 1000, 0])
def test_one_call_many_packets(pair, ps):
    p = pair(MIXED)
    re, im = inputs(len(MIXED))
    p.call(re, im, ps, f"ps {ps}")


@pytest.mark.parametrize("n", [255, 256, 257])
def test_single_calls_around_one_tile(pair, n):
    p = pair(MIXED)
    re, im = inputs(len(MIXED))
    p.call(re[:, :n], im[:, :n], None, f"n {n}")
    p.call(re[:, n:2 * n], im[:, n:2 * n], 100, f"n {n}, second call")


# ------------------------------------------------------------------ 3: per-slot settings mid-stream

def test_per_slot_settings_mid_stream(pair):
    modes = ["nfm", "usb", "am", "am", "lsb", "cw"]
    p = pair(modes)
    re, im = inputs(len(modes), 12 * 500)
    pos = [0]

    def step(what, n=500, ps=200):
        s = pos[0]
        pos[0] += n
        return p.call(re[:, s:s + n], im[:, s:s + n], ps, what)

    step("start")
    uf_before = [p.bank.taps(k, "user")[0] for k in range(len(modes))]
    # a width change on slot 0: its user filter is rebuilt, nobody else's
    p.bank.set_channel_width(0, 4000)
    p.handles[0].channelWidth = 4000
    step("width on slot 0")
    assert not np.array_equal(p.bank.taps(0, "user")[0], uf_before[0])
    for k in range(1, len(modes)):
        same(p.bank.taps(k, "user")[0], uf_before[k], f"user filter of slot {k}")
    # a width outside the limits is coerced as on the handle
    p.bank.set_channel_width(0, 1)
    p.handles[0].channelWidth = 1
    assert p.bank.channel_width(0) == p.handles[0].channelWidth == 3000
    step("coerced width on slot 0")
    # USB -> LSB -> CW on slot 1: the band-pass is rebuilt
    for m in ("lsb", "cw"):
        bp = np.concatenate(p.bank.taps(1, "bandpass")[:2])     # USB and LSB differ in the imaginary part
        p.bank.set_mode(1, m)
        p.handles[1].demodulationMode = m
        step(f"slot 1 to {m}")
        assert not np.array_equal(np.concatenate(p.bank.taps(1, "bandpass")[:2]), bp)
    # AM -> WFM -> AM on slot 2: the audio filters keep their delay lines
    for m in ("wfm", "am"):
        p.bank.set_mode(2, m)
        p.handles[2].demodulationMode = m
        step(f"slot 2 to {m}")
    p.bank.set_volume(4, 0.25)
    p.handles[4].audioVolumeLevel = 0.25
    step("volume on slot 4")
    p.bank.set_audio_sink(3, False)
    p.handles[3].audio_sink = False
    got = step("audio sink off on slot 3")
    assert got[3].size > got[2].size                      # AM at the packet rate against AM at 48 kHz
    p.bank.reset(5)
    p.handles[5].reset()
    p.same_settings("after reset(5)")
    assert p.bank.taps(5, "user")[0].size == 0
    step("reset on slot 5")
    # a slot switched off and on again keeps its state while off
    p.bank.set_mode(0, "off")
    p.handles[0].demodulationMode = "off"
    assert step("slot 0 off")[0].size == 0
    p.bank.set_mode(0, "nfm")
    p.handles[0].demodulationMode = "nfm"
    step("slot 0 on again")
    with pytest.raises(_lib.RfaError) as e:
        p.bank.set_mode(len(modes), "am")
    assert e.value.status == _lib.RFA_ERR_INVALID
    with pytest.raises(_lib.RfaError):
        p.bank.state(-1)


# ------------------------------------------------------------------ 4: capacity

def test_audio_stride_one_short_consumes_nothing(pair):
    import torch
    modes = ["nfm", "cw", "usb", "wfm"]           # CW (no audio decimator) writes the most
    p = pair(modes)
    n = 1000
    re, im = inputs(len(modes), 2 * n)
    p.call(re[:, :n], im[:, :n], 300, "first call")
    counts = p.bank.max_outputs(n)
    assert counts.index(max(counts)) == 1 and sorted(counts)[-2] < max(counts)
    d_re = torch.from_numpy(re[:, n:].copy()).cuda()
    d_im = torch.from_numpy(im[:, n:].copy()).cuda()
    short = torch.full((len(modes), max(counts) - 1), 7.0, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.RfaError) as e:
        p.bank.process_tensor(d_re, d_im, short, 300)
    assert e.value.status == _lib.RFA_ERR_SIZE
    p.bank.synchronize()
    assert bool((short == 7.0).all())
    assert p.bank.max_outputs(n) == counts                 # nothing was consumed in any slot
    p.same_settings("after the refused call")
    room = torch.empty((len(modes), max(counts)), dtype=torch.float32, device="cuda")
    got = p.bank.process_tensor(d_re, d_im, room, 300)
    p.bank.synchronize()
    assert got == counts
    audio = room.cpu().numpy()
    p.check([audio[k, :g] for k, g in enumerate(got)], re[:, n:], im[:, n:], 300, "with enough room")


# ------------------------------------------------------------------ 5: strides and slot count

def test_rows_of_wider_tensors(pair):
    import torch
    modes = ["am", "nfm", "usb"]
    p = pair(modes)
    n = 700
    re, im = inputs(len(modes), n)
    wide_re = torch.zeros((len(modes), n + 37), dtype=torch.float32, device="cuda")
    wide_im = torch.zeros_like(wide_re)
    wide_re[:, 5:5 + n] = torch.from_numpy(re.copy()).cuda()
    wide_im[:, 5:5 + n] = torch.from_numpy(im.copy()).cuda()
    cap = max(p.bank.max_outputs(n))
    wide_out = torch.full((len(modes), cap + 11), 7.0, dtype=torch.float32, device="cuda")
    got = p.bank.process_tensor(wide_re[:, 5:5 + n], wide_im[:, 5:5 + n], wide_out[:, 3:3 + cap], 256)
    p.bank.synchronize()
    out = wide_out.cpu().numpy()
    p.check([out[k, 3:3 + g] for k, g in enumerate(got)], re, im, 256, "strided")
    for k, g in enumerate(got):                             # nothing outside a slot's own samples
        assert (out[k, :3] == 7.0).all() and (out[k, 3 + g:] == 7.0).all(), k


def test_one_slot(pair):
    p = pair(["usb"])
    re, im = inputs(1)
    for i, (c_re, c_im) in enumerate(chunks(re, im, [1, 0, 300, 257, 1000])):
        p.call(c_re, c_im, 128, f"call {i}")


def test_300_slots(pair):
    three = ["nfm", "am", "usb"]
    k_count = 300
    p = pair([three[k % 3] for k in range(k_count)], slot_of=[list(range(j, k_count, 3)) for j in range(3)],
             handle_modes=three)
    n = 700
    h_re, h_im = inputs(3, 2 * n)
    re = np.stack([h_re[k % 3] for k in range(k_count)])
    im = np.stack([h_im[k % 3] for k in range(k_count)])
    for i, sl in enumerate([slice(0, n), slice(n, 2 * n)]):
        got = p.bank.process(re[:, sl], im[:, sl], 256)
        p.check(got, h_re[:, sl], h_im[:, sl], 256, f"call {i}")


# ------------------------------------------------------------------ 6: queued calls (the record ring)

def test_queued_calls_keep_their_records(pair):
    import torch
    modes = ["am", "nfm", "usb", "wfm", "cw", "off"]
    sizes = [[300, 1, 655, 0, 1000][i % 5] for i in range(64)]
    assert len(sizes) > RING
    warm, total = 1000, sum(sizes)
    p = pair(modes)
    re, im = inputs(len(modes), warm + total)
    # the first call builds every filter and sizes the scratch for the largest call, which
    # synchronises; the queued calls below then never wait for the device on their own
    p.call(re[:, :warm], im[:, :warm], 256, "warm-up")
    re, im = re[:, warm:], im[:, warm:]
    s = torch.cuda.Stream()
    p.bank.set_stream(s.cuda_stream)
    d_re = torch.from_numpy(re.copy()).cuda()
    d_im = torch.from_numpy(im.copy()).cuda()
    cap = max(sizes)
    out = torch.zeros((len(sizes), len(modes), cap), dtype=torch.float32, device="cuda")
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    counts = []
    with torch.cuda.stream(s):
        for _ in range(4):
            big.fill_(1)                                   # a long operation ahead of every call
        pos = 0
        for i, n in enumerate(sizes):                      # no synchronisation in between
            counts.append(p.bank.process_device(d_re.data_ptr() + 4 * pos, d_im.data_ptr() + 4 * pos, total, n,
                                                out[i].data_ptr(), cap, 256))
            pos += n
    s.synchronize()
    audio = out.cpu().numpy()
    pos = 0
    for i, n in enumerate(sizes):
        for k, h in enumerate(p.handles):
            want = h.process(re[k, pos:pos + n], im[k, pos:pos + n], 256)
            same(audio[i, k, :counts[i][k]], want, f"call {i} ({n}) slot {k}")
        pos += n
    p.same_settings("after the queue")
    p.bank.set_stream(None)


# ------------------------------------------------------------------ 7: process_tensor ordering

def test_process_tensor_is_ordered_on_torch_stream(pair):
    """process_tensor runs on torch's current stream: a torch op producing the input just
    before, and one reading the output just after, see the right data."""
    import torch
    modes = ["usb", "am", "nfm"]
    p = pair(modes)
    re, im = inputs(len(modes))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src_re = torch.from_numpy(re.copy()).to("cuda")
        src_im = torch.from_numpy(im.copy()).to("cuda")
        big = torch.empty(64 << 20, dtype=torch.uint8, device="cuda")
        big.fill_(1)                                        # keeps the stream busy ahead of the copies
        t_re, t_im = torch.empty_like(src_re), torch.empty_like(src_im)
        t_re.copy_(src_re)                                  # producers on the current (side) stream
        t_im.copy_(src_im)
        out = torch.empty((len(modes), max(p.bank.max_outputs(TOTAL))), dtype=torch.float32, device="cuda")
        got = p.bank.process_tensor(t_re, t_im, out, 1000)
        res = out.clone()                                   # consumer on the same stream
    s.synchronize()
    assert p.bank.stream == s.cuda_stream
    audio = res.cpu().numpy()
    p.check([audio[k, :g] for k, g in enumerate(got)], re, im, 1000, "process_tensor")


# ------------------------------------------------------------------ 8: ReceiverBank on the bank

def test_receiver_bank_runs_on_the_demodulator_bank(rfa):
    modes = ["nfm", "am", "usb", "lsb"]
    assert len({demod.mode_info(m)[0] for m in modes}) == 1
    center = 100_000_000
    channels = [center + o for o in (130_000, -455_000, 12_500, 300_000)]
    rng = np.random.default_rng(42)
    packets = [rng.integers(0, 256, 2 * 16_384, dtype=np.uint8) for _ in range(6)]
    with demod.ReceiverBank("u8", 2_400_000, modes) as rxb:
        assert isinstance(rxb.demods, demod.DemodulatorBank) and rxb.n_channels == 4
        rxb.set_frequencies(center, channels)
        got = []
        for j, pk in enumerate(packets):
            if j == 3:
                rxb.set_mode(1, "nfm")
                assert rxb.mode(1) == demod.MODES["nfm"]
            got.append(rxb.process(pk))
    for k, (mode, ch) in enumerate(zip(modes, channels)):
        with demod.Receiver("u8", 2_400_000, mode) as rx:
            rx.set_frequencies(center, ch)
            for j, pk in enumerate(packets):
                if j == 3 and k == 1:
                    rx.mode = "nfm"
                want = rx.process(pk)
                assert want.size > 0
                same(got[j][k], want, f"packet {j} slot {k}")
