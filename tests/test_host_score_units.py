"""The length model and the score units of the integer filters, which the library writes once (p7x_internal.hpp: tjb_of,
xw_move_of, msv_score_nats, vit_score_nats; reached through the test seam p7x_debug_score_units), against their restatement
in numpy float32 -- in both spellings that the library's callers used to have: 3 / (L + 3) with the sum taken in integers or
in floats, and the final "- 3" taken in double (upstream's `-= 3.0`) or in float.  And the names of the timing slots: enum
p7x_timing of include/p7x.h against plan7.TIMING_NAMES."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import ROOT
from pyhmmer_amd import _lib, plan7

f32 = np.float32
LENGTHS = (1, 2, 3, 61, 400, 99_999, 100_000)


def roundf(x):
    """C roundf of float32 values (half away from zero), taken exactly in double."""
    x = x.astype(np.float64)
    return np.trunc(x + np.copysign(0.5, x)).astype(f32)


def logf(x):
    return np.log(x.astype(np.float64)).astype(f32)


def pmove_spellings(L):
    """3 / (L + 3) for an int array L, float32: the sum in integers, and upstream's (2 + nj) / (L + 2 + nj) in floats."""
    return f32(3.0) / (L + 3).astype(f32), (f32(2.0) + f32(1.0)) / ((L.astype(f32) + f32(2.0)) + f32(1.0))


def tjb_np(scale_b, pmove):          # unbiased_byteify(scale_b, logf(pmove))
    s = f32(-1.0) * roundf(f32(scale_b) * logf(pmove))
    return np.where(s > 255.0, 255, s.astype(np.int32)).astype(np.int32)


def xw_move_np(scale_w, pmove):      # wordify(scale_w, logf(pmove))
    s = roundf(f32(scale_w) * logf(pmove))
    return np.clip(s, -32768.0, 32767.0).astype(np.int32)


def minus3_spellings(v):
    """v - 3 for float32 v: in double, rounded once, and in float."""
    return (v.astype(np.float64) - 3.0).astype(f32), v - f32(3.0)


def library(om, L, xJ=None, xC=None):
    L = np.ascontiguousarray(L, dtype=np.int32)
    xJ = np.zeros(0, np.int32) if xJ is None else np.ascontiguousarray(xJ, dtype=np.int32)
    xC = np.zeros(0, np.int32) if xC is None else np.ascontiguousarray(xC, dtype=np.int32)
    tjb, xwm = np.zeros(len(L), np.int32), np.zeros(len(L), np.int32)
    usc, vfsc = np.zeros((len(L), len(xJ)), f32), np.zeros((len(L), len(xC)), f32)
    st = _lib.lib().p7x_debug_score_units(om._handle, L.ctypes.data, len(L), tjb.ctypes.data, xwm.ctypes.data,
                                          xJ.ctypes.data if len(xJ) else None, len(xJ), xC.ctypes.data if len(xC) else None, len(xC),
                                          usc.ctypes.data if len(xJ) else None, vfsc.ctypes.data if len(xC) else None)
    assert st == 0, _lib.last_error()
    return tjb, xwm, usc, vfsc


@pytest.fixture(scope="module", params=["PF02826", "RREFam"])
def om(request, models):
    hmm = models[request.param][0]
    return plan7.OptimizedProfile(hmm, plan7.Background(hmm.alphabet), 400)


def test_length_model_every_length(om):
    L = np.arange(0, 100_001, dtype=np.int64)
    by_int, by_float = pmove_spellings(L)
    assert np.array_equal(by_int.view(np.uint32), by_float.view(np.uint32))
    tjb, xwm, _, _ = library(om, L)
    assert np.array_equal(tjb, tjb_np(om.scale_b, by_int)) and np.array_equal(tjb, tjb_np(om.scale_b, by_float))
    assert np.array_equal(xwm, xw_move_np(om.scale_w, by_int)) and np.array_equal(xwm, xw_move_np(om.scale_w, by_float))
    assert tjb[om.L] == om.tjb                    # the profile's own length model is the same function


def test_conversions_every_integer_score(om):
    xJ = np.arange(-1, 256, dtype=np.int32)           # -1: the MSV filter's overflow mark
    xC = np.arange(-32768, 32768, dtype=np.int32)     # the ends: no path, overflow
    tjb, xwm, usc, vfsc = library(om, LENGTHS, xJ, xC)
    scale_b, scale_w, base_b, base_w = f32(om.scale_b), f32(om.scale_w), f32(om.base), f32(om.base_w)
    for l in range(len(LENGTHS)):
        v = (xJ - tjb[l]).astype(f32) - base_b
        v = v / scale_b
        in_double, in_float = minus3_spellings(v)
        assert np.array_equal(in_double[1:].view(np.uint32), in_float[1:].view(np.uint32))
        want = in_double.copy()
        want[0] = np.inf
        assert np.array_equal(usc[l].view(np.uint32), want.view(np.uint32))
        w = (xC.astype(f32) + f32(xwm[l])) - base_w
        w = w / scale_w
        in_double, in_float = minus3_spellings(w)
        assert np.array_equal(in_double.view(np.uint32), in_float.view(np.uint32))
        want = in_double.copy()
        want[0], want[-1] = -np.inf, np.inf
        assert np.array_equal(vfsc[l].view(np.uint32), want.view(np.uint32))


def test_timing_names_are_the_header_enum():
    header = (ROOT / "include" / "p7x.h").read_text()
    body = re.search(r"enum\s+p7x_timing\s*\{(.*?)\}", header, re.S).group(1)
    names = re.findall(r"\b(P7X_MS_[A-Z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names[-1] == "P7X_MS_COUNT" and len(names) - 1 == len(plan7.TIMING_NAMES)
    assert tuple(n[len("P7X_MS_"):].lower() for n in names[:-1]) == plan7.TIMING_NAMES
    assert re.search(r"P7X_MS_MSV\s*=\s*0\s*,", body) and len(re.findall(r"=", re.sub(r"/\*.*?\*/", "", body, flags=re.S))) == 1
