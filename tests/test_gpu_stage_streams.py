"""GPU: the stream behaviour that csrc/stage_common.h and demod._Handle carry for all five
stages, one case per wrapper class at its smallest working shape.  A handle is moved from its
own stream to a torch stream, then by ``process_tensor`` to torch's current stream, then back;
the three calls it makes on the way give bit for bit what a second handle gives that never
leaves its own stream."""
import numpy as np
import pytest
import torch

from rfanalyzer_amd import demod

pytestmark = pytest.mark.gpu

N = 1024                                        # samples per call
FREQ, CHANNELS = 100_000_000, [100_200_000, 99_700_000]


def _front_end():
    h = demod.FrontEnd("s8", 2_400_000, 48_000)
    h.set_frequencies(FREQ, CHANNELS[0])
    return h


def _front_end_bank():
    h = demod.FrontEndBank("s8", 2_400_000, 48_000, 2)
    h.set_frequencies(FREQ, CHANNELS)
    return h


def _channelizer():
    taps = np.random.default_rng(5).uniform(-1, 1, 16).astype(np.float32)
    return demod.Channelizer("s8", 8, 8, taps)


def _raw_io(rows):
    """(inputs, outputs) of a raw-sample stage: N s8 samples -> planar float32 rows of N."""
    def make(dev):
        raw = torch.from_numpy(np.random.default_rng(11).integers(-128, 128, 2 * N, dtype=np.int8)).to(dev)
        shape = (N,) if rows is None else (rows, N)
        return (raw,), (torch.zeros(shape, device=dev), torch.zeros(shape, device=dev))
    return make


def _iq_io(rows):
    """(inputs, outputs) of a demodulator: N quadrature samples per row -> audio rows of N."""
    def make(dev):
        rng = np.random.default_rng(12)
        shape = (N,) if rows is None else (rows, N)
        re, im = (torch.from_numpy(rng.uniform(-0.5, 0.5, shape).astype(np.float32)).to(dev) for _ in range(2))
        return (re, im), (torch.zeros(shape, device=dev),)
    return make


def _ptr(t):
    return t.data_ptr()


# class name -> (make handle, make tensors, the call on device pointers)
CASES = {
    "FrontEnd": (_front_end, _raw_io(None),
                 lambda h, i, o: h.process_device(_ptr(i[0]), N, _ptr(o[0]), _ptr(o[1]), N)),
    "FrontEndBank": (_front_end_bank, _raw_io(2),
                     lambda h, i, o: h.process_device(_ptr(i[0]), N, _ptr(o[0]), _ptr(o[1]), N)),
    "Demodulator": (lambda: demod.Demodulator("am"), _iq_io(None),
                    lambda h, i, o: h.process_device(_ptr(i[0]), _ptr(i[1]), N, _ptr(o[0]), N)),
    "DemodulatorBank": (lambda: demod.DemodulatorBank(["am", "nfm"]), _iq_io(2),
                        lambda h, i, o: h.process_device(_ptr(i[0]), _ptr(i[1]), N, N, _ptr(o[0]), N)),
    "Channelizer": (_channelizer, _raw_io(8),
                    lambda h, i, o: h.process_device(_ptr(i[0]), N, _ptr(o[0]), _ptr(o[1]), N)),
}


def _result(h, count, outs):
    """What a call gave, as bits, once the handle's stream has run dry."""
    h.synchronize()
    return count, [o.cpu().numpy().view(np.int32).copy() for o in outs]


def _same(a, b, what):
    assert a[0] == b[0], f"{what}: counts {a[0]} and {b[0]}"
    assert np.any(a[1][0]), f"{what}: no output at all"
    for x, y in zip(a[1], b[1]):
        assert np.array_equal(x, y), f"{what}: outputs differ"


@pytest.mark.parametrize("name", sorted(CASES))
def test_stream_moves_keep_the_stream_of_samples(rfa, name):
    make, tensors, on_pointers = CASES[name]
    dev = torch.device("cuda", 0)
    ins, outs = tensors(dev)
    _, ref_outs = tensors(dev)
    torch.cuda.synchronize(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    with make() as h, make() as ref:
        assert isinstance(h, getattr(demod, name))
        own = h.stream
        assert own != 0 and ref.stream not in (0, own)
        want = [_result(ref, on_pointers(ref, ins, ref_outs), ref_outs) for _ in range(3)]
        assert ref.stream != 0

        _same(_result(h, on_pointers(h, ins, outs), outs), want[0], "on its own stream")
        h.set_stream(s1.cuda_stream)
        assert h.stream == s1.cuda_stream
        with torch.cuda.stream(s2):
            count = h.process_tensor(*ins, *outs)
        assert h.stream == s2.cuda_stream
        _same(_result(h, count, outs), want[1], "on torch's current stream")
        h.set_stream(None)
        assert h.stream == own
        _same(_result(h, on_pointers(h, ins, outs), outs), want[2], "back on its own stream")
        h.close()
        h.close()
        assert h._h is None
