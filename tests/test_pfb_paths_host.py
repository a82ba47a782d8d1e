"""CPU: the host side of tests/test_gpu_pfb_paths.py, so that the GPU module cannot fail for a reason
of its own -- the tile-plan query (rfa_pfb_tile_plan, no device needed) on hand-computed plans and
its argument errors against the create entries' rules, the plan property of every case of the table
(tests/pfb_paths.py) and the table's coverage computed from the query's answers, the call sizes,
and the float32 model the GPU is held against bit for bit (tests/pfb_model.py) tied to the float64
restatements within the derived bounds, to the defining sum on the small cases, and to itself over
call splits."""
import ctypes
import os
import re

import numpy as np
import pytest

import pfb_model
import pfb_paths as pp
import pfb_rational_ref as rref
import pfb_ref
from rfanalyzer_amd import _lib
from rfanalyzer_amd import demod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB64 = 8192                                            # points of 8 B in the 64 KiB staging area


@pytest.fixture(scope="module", autouse=True)
def lib():
    import rfanalyzer_amd
    rfanalyzer_amd.build()
    return rfanalyzer_amd.lib()


def _same(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


# ---------------------------------------------------------------- the query itself

def test_tile_plan_of_the_smallest_handle_by_hand():
    """M = 8, D = 3, T = 19: 16 times per workgroup (128 points), rows of 9; the run is 15 * 3 + 19 =
    64 samples, 19 taps are 10 points behind it, and both row sets are 2 * 16 * 9 points."""
    assert demod.pfb_tile_plan(8, 0, 3, 19) == {
        "NT": 16, "Mp": 9, "run": 64, "staged_run": 1, "staged_taps": 1, "rows_by_time": 0, "stage_points": 74,
        "lds_bytes": 8 * (74 + 2 * 16 * 9), "stages": 2, "radices": [4, 2]}


def test_tile_plan_at_the_largest_lds_request_by_hand():
    """M = D = 256: 16 times, rows of 257, run 15 * 256 + T.  T = 2901: 6741 samples + 1451 points of
    taps = 8192 points, the whole staging area, in front of 2 * 16 * 257 points of rows = 131 328 B,
    the most the kernels are prepared for.  T = 2902 is one point too many: nothing is staged.  The
    rational entry with L = 1 has the same run and one tap row; one tap more, and it still stages the
    run (plan B)."""
    rows = 2 * 16 * 257
    want = {"NT": 16, "Mp": 257, "run": 6741, "staged_run": 1, "staged_taps": 1, "rows_by_time": 0,
            "stage_points": KIB64, "lds_bytes": 8 * (KIB64 + rows), "stages": 4, "radices": [4, 4, 4, 4]}
    assert 8 * (KIB64 + rows) == 131_328 == pp.LDS_MOST
    assert demod.pfb_tile_plan(256, 0, 256, 2901) == want
    assert demod.pfb_tile_plan(256, 1, 256, 2901) == want
    assert demod.pfb_tile_plan(256, 0, 256, 2902) == dict(want, run=6742, staged_run=0, staged_taps=0, stage_points=0,
                                                           lds_bytes=8 * rows)
    assert demod.pfb_tile_plan(256, 1, 256, 2902) == dict(want, run=6742, staged_taps=0, stage_points=6742,
                                                           lds_bytes=8 * (6742 + rows))


def test_tile_plan_at_the_8192_point_edges_by_hand():
    """M = D = 4096: one time per workgroup, run = T.  T = 5461 and its 2731 points of taps are 8192
    points; T = 5462 needs 8193.  Rational M = 2048, L = 3, D = 4097 (NT = 2): run = ceil(4097 / 3) +
    Tp = 1366 + Tp, so Tp = 6826 (T = 20478) is the last staged run and Tp = 6827 the first plan C."""
    p = demod.pfb_tile_plan(4096, 0, 4096, 5461)
    assert (p["NT"], p["Mp"], p["run"], p["staged_run"], p["stage_points"]) == (1, 4097, 5461, 1, KIB64)
    assert p["lds_bytes"] == 8 * (KIB64 + 2 * 4097) and p["radices"] == [4] * 6
    p = demod.pfb_tile_plan(4096, 0, 4096, 5462)
    assert (p["NT"], p["run"], p["staged_run"], p["staged_taps"], p["stage_points"]) == (1, 5462, 0, 0, 0)
    assert p["lds_bytes"] == 8 * 2 * 4097
    p = demod.pfb_tile_plan(2048, 3, 4097, 20478)
    assert (p["NT"], p["run"], p["staged_run"], p["staged_taps"], p["stage_points"]) == (2, KIB64, 1, 0, KIB64)
    p = demod.pfb_tile_plan(2048, 3, 4097, 20479)
    assert (p["NT"], p["run"], p["staged_run"], p["staged_taps"], p["stage_points"]) == (2, KIB64 + 1, 0, 0, 0)


def test_tile_plan_of_the_app_ratio_by_hand():
    """M = 16, L / D = 48 / 125, T = 965: Tp = 21; 15 outputs on span ceil(15 * 125 / 48) = 40 samples, run
    61; L > NT, so 16 tap rows by time, 16 * 21 floats = 168 points."""
    assert demod.pfb_tile_plan(16, 48, 125, 965) == {
        "NT": 16, "Mp": 17, "run": 61, "staged_run": 1, "staged_taps": 16, "rows_by_time": 1, "stage_points": 229,
        "lds_bytes": 8 * (229 + 2 * 16 * 17), "stages": 2, "radices": [4, 4]}


def _create_rc(L, M, Lr, D, T):
    """The status of the matching create entry for (M, L, D, T) with a valid format and taps."""
    taps = np.zeros(max(T, 1), np.float32)
    h = ctypes.c_void_p()
    fp = taps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    rc = (L.rfa_pfb_create(0, 0, M, D, fp, T, ctypes.byref(h)) if Lr == 0
          else L.rfa_pfb_create_rational(0, 0, M, Lr, D, fp, T, ctypes.byref(h)))
    if rc == 0:
        L.rfa_pfb_destroy(h)
    return rc


def test_tile_plan_argument_errors_are_the_create_entries(lib):
    out = (ctypes.c_int32 * 21)()
    args = [(16, 0, 4, 16), (16, 0, 16, 256), (16, 0, 17, 16), (16, 0, 4, 257), (16, 0, 0, 16), (16, 0, 4, 0),
            (0, 0, 1, 16), (-16, 0, 1, 16), (7, 0, 0, 8), (7, 0, 1, 8), (14, 0, 1, 8), (4097, 0, 1, 8), (8192, 0, 1, 8),
            (4096, 0, 4096, 65536), (4096, 0, 4096, 65537),
            (16, 3, 7, 61), (16, 64, 65, 61), (16, 65, 66, 61), (16, 8, 7, 61), (16, 3, 48, 61), (16, 3, 47, 768),
            (16, 3, 49, 61), (16, 6, 14, 61), (16, 3, 7, 769), (16, 3, 0, 61), (16, 3, 7, 0), (0, 3, 7, 61),
            (7, 3, 22, 61), (7, 3, 20, 61), (22, 1, 1, 8), (16, 1, 1, 16), (16, 1, 16, 256), (16, 1, 17, 16)]
    seen = set()
    for M, Lr, D, T in args:
        rc = lib.rfa_pfb_tile_plan(M, Lr, D, T, out)
        created = _create_rc(lib, M, Lr, D, T)
        if created in (_lib.RFA_ERR_INVALID, _lib.RFA_ERR_UNSUPPORTED):
            assert rc == created, (M, Lr, D, T, rc, created)
        else:
            assert created in (_lib.RFA_OK, _lib.RFA_ERR_NODEVICE) and rc == _lib.RFA_OK, (M, Lr, D, T, rc, created)
        seen.add(rc)
    assert seen == {_lib.RFA_OK, _lib.RFA_ERR_INVALID, _lib.RFA_ERR_UNSUPPORTED}
    assert lib.rfa_pfb_tile_plan(16, 0, 4, 16, None) == _lib.RFA_ERR_INVALID
    assert lib.rfa_pfb_tile_plan(16, -1, 4, 16, out) == _lib.RFA_ERR_INVALID
    with pytest.raises(_lib.RfaError):
        demod.pfb_tile_plan(16, 0, 17, 16)


def test_header_names_the_plan_fields_in_the_binding_order():
    text = open(os.path.join(ROOT, "include", "rfa.h")).read()
    fields = dict(re.findall(r"RFA_PFB_PLAN_([A-Z_0-9]+) = (\d+)", text))
    order = ["TIMES", "PITCH", "RUN", "STAGED_RUN", "STAGED_TAPS", "ROWS_BY_TIME", "STAGE_POINTS", "LDS_BYTES",
             "STAGES", "RADIX0"]
    assert [int(fields[k]) for k in order] == list(range(10))
    assert len(demod.PFB_PLAN_FIELDS) == int(fields["RADIX0"])
    stages = int(re.search(r"#define RFA_PFB_PLAN_MAX_STAGES (\d+)", text).group(1))
    assert stages == demod.PFB_PLAN_MAX_STAGES and int(fields["FIELDS"]) == int(fields["RADIX0"]) + stages


# ---------------------------------------------------------------- the case table

@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_case_has_its_plan_property_and_call_sizes(case):
    p = case.plan()                                      # asserts the case's property
    nt = p["NT"]
    n1, n2 = case.outputs()
    s1, s2 = case.sizes()
    assert case.count(s1) == n1 and case.count(s1 + s2) - n1 == n2
    assert s1 >= case.Th - 1                             # the first call fills the history
    if nt == 1:
        assert (n1, n2) == (3, 2)
    else:
        assert n1 > nt and n1 % nt != 0                  # a full tile, and the call ends inside one
        assert n2 > 2 * nt and n2 % nt != 0              # two full tiles and a ragged one
    if case.L is None and case.D > 1:
        assert s1 % case.D != 0 and (s1 + s2) % case.D == case.D - 1
    assert s1 + s2 < 70_000
    assert pfb_model.radices(case.M) == p["radices"]
    sel = pp.selection(case)
    assert len(set(sel)) < len(sel) <= case.M and {0, case.M - 1} <= set(sel)
    if 17 <= case.M <= 256:
        assert len(sel) * nt > 256


def test_formats_rotate():
    for group in (pp.INTEGER, pp.RATIONAL):
        assert {c.fmt for c in group} == set(pp.FORMATS)
    assert len({c.id for c in pp.ALL}) == len(pp.ALL) == 39


def test_the_table_covers_every_path():
    cov = pp.coverage(pp.ALL)
    assert cov["first"] == {2, 3, 4, 5}
    # every (previous, next) pair pfb_radices' order 4.., 2, 3.., 5.. can emit
    assert cov["pairs"] == {(4, 4), (4, 2), (4, 3), (4, 5), (2, 3), (2, 5), (3, 3), (3, 5), (5, 5)}
    every = {(nt, s) for nt in (16, 8, 4, 2, 1) for s in (0, 1)}
    assert cov["tiles"][False] == every                  # the integer kernel: every NT, staged and not
    assert {nt for nt, _ in cov["tiles"][True]} >= {16, 4, 2, 1} and (2, 0) in cov["tiles"][True]
    assert cov["plans"] == {"A", "B", "C"}
    assert cov["rows"] == {"phase", "time"} and max(cov["rows_by_time_L"]) > 16
    assert cov["one_tap"] == {False, True}               # T = 1 on both kernels
    tuned = {(c.L is not None, c.plan()["NT"]) for c in pp.TUNED}
    assert tuned == {(False, 4), (False, 2), (False, 1), (True, 2)}
    most = [c for c in pp.ALL if c.plan()["lds_bytes"] == pp.LDS_MOST]
    assert {c.L for c in most} == {None, 1}              # the largest request on both kernels


# ---------------------------------------------------------------- the model

def test_model_tables_have_the_kernel_layout():
    """p * (R - 1) entries per stage, entry (k, r) = exp(-2 pi j k r / (p R)) to float32 rounding, the
    first stage's (p = 1, never read) being exp(0)."""
    for M in (8, 18, 60, 125):
        p = 1
        for R, (re, im) in zip(pfb_model.radices(M), pfb_model.twiddles(pfb_model.radices(M))):
            assert re.size == im.size == p * (R - 1) and re.dtype == np.float32
            k, r = np.divmod(np.arange(p * (R - 1)), R - 1)
            want = np.exp(-2j * np.pi * k * (r + 1) / (p * R))
            assert np.abs(re + 1j * im - want).max() <= 2.0 ** -24
            p *= R
        assert p == M


@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_model_against_the_float64_restatement(case):
    y = np.concatenate(pp.model_run(case), axis=1)
    assert y.shape == (case.M, sum(case.outputs())) and np.all(np.isfinite(y.view(np.float32)))
    r = pp.ratio(y, case)
    print(f"channelizer model {case.id}: max err / bound = {r:.4f}")
    assert r <= 1.0, (case.id, r)
    taps, _, x = pp.data(case)
    if case.M <= 32 and x.size <= 2500:                  # small enough for the defining sum itself
        ref, b = pp.float64_run(case)
        direct = (pfb_ref.direct(x, taps, case.M, case.D) if case.L is None
                  else rref.direct(x, taps, case.M, case.L, case.D))
        assert np.abs(direct - ref).max() <= 1e-11
        assert np.abs(y.astype(np.complex128) - direct).max() <= b


def test_the_defining_sum_is_reached_on_small_cases():
    small = [c for c in pp.ALL if c.M <= 32 and sum(c.sizes()) <= 2500]
    assert len(small) >= 10 and {c.L is None for c in small} == {False, True}


@pytest.mark.parametrize("case", pp.ALL, ids=lambda c: c.id)
def test_model_is_invariant_to_the_call_split(case):
    _, _, x = pp.data(case)
    two = np.concatenate(pp.model_run(case), axis=1)
    _same(pp.model_stream(case).process(x), two)
    if x.size <= 2500:                                   # calls of 1, 0 and a few samples, then the rest
        m = pp.model_stream(case)
        cuts = [1, 0, 2, 5, 1, case.D, case.M + 1]
        parts, pos = [], 0
        for n in cuts + [x.size - sum(cuts)]:
            parts.append(m.process(x[pos:pos + n]))
            pos += n
        assert pos == x.size
        _same(np.concatenate(parts, axis=1), two)


def test_one_tap_model_channel_0_is_the_product():
    """T' = 1: u has one non-zero residue and every stage adds zeros to it, so channel 0 is
    float32(h) * x[newest] itself."""
    for case in pp.ALL:
        if case.Th != 1:
            continue
        taps, _, x = pp.data(case)
        y = np.concatenate(pp.model_run(case), axis=1)
        n = np.arange(y.shape[1])
        if case.L is None:
            h, newest = taps[0], n * case.D + case.D - 1
        else:
            h, newest = taps[(n * case.D) % case.L], n * case.D // case.L
        xs = x[newest]
        assert np.array_equal(y[0].real, h * xs.real.astype(np.float32))
        assert np.array_equal(y[0].imag, h * xs.imag.astype(np.float32))
