"""The int8-plane cosine search's C surface without a GPU: declarations, NULL arguments, refusals before any GPU work."""
import ctypes as C

import numpy as np
import pytest

from kjarni_amd import _ffi, lib
from kjarni_amd._ffi import KjarniError

ARITY = {"kjarni_hip_cosine_codes_bytes": 2, "kjarni_hip_cosine_encode": 6, "kjarni_hip_cosine_search_coded_workspace_bytes": 4,
         "kjarni_hip_cosine_search_coded": 14, "kjarni_hip_cosine_search_coded_host": 12, "kjarni_hip_set_index_codes": 1,
         "kjarni_hip_index_codes": 0, "kjarni_hip_index_image_bytes": 0}


def test_declarations_and_switch():
    L = lib()
    for name, n in ARITY.items():
        assert hasattr(L, name) and len(_ffi.SIGNATURES[name][1]) == n
    assert L.kjarni_hip_index_codes() == 0                      # off by default
    L.kjarni_hip_set_index_codes(5)
    assert L.kjarni_hip_index_codes() == 1
    L.kjarni_hip_set_index_codes(0)
    assert L.kjarni_hip_index_codes() == 0
    # codes [n, dim] padded to 256 bytes + four floats per document; no plane for a width the route refuses
    assert L.kjarni_hip_cosine_codes_bytes(1000, 384) == 384000 + 16000
    assert L.kjarni_hip_cosine_codes_bytes(3, 64) == 256 + 48
    assert [L.kjarni_hip_cosine_codes_bytes(10, d) for d in (0, 100, 1088)] == [0, 0, 0]
    assert L.kjarni_hip_cosine_search_coded_workspace_bytes(1, 1000, 100, 10) == 256


def _host_call(q, c, dim, k, idx, sc, hits, stats, nq=1, n=4):
    p = lambda a, t: None if a is None else a.ctypes.data_as(t)
    return lib().kjarni_hip_cosine_search_coded_host(0, p(q, _ffi._f32p), nq, p(c, _ffi._f32p), n, dim, 0, k, p(idx, _ffi._i64p),
                                                     p(sc, _ffi._f32p), None if hits is None else C.byref(hits),
                                                     None if stats is None else stats)


@pytest.mark.parametrize("dim,k,nq,code", [(100, 2, 1, KjarniError.INVALID_CONFIG), (1088, 2, 1, KjarniError.INVALID_CONFIG),
                                            (64, 1025, 1, KjarniError.INVALID_CONFIG), (64, 2, 1025, KjarniError.INVALID_CONFIG),
                                            (64, 2, 1, KjarniError.NULL_POINTER)])
def test_refusals_leave_outputs_untouched(dim, k, nq, code):
    """A refused shape returns before any GPU work (this test has no GPU) with idx / score / hits / stats as they were; the last
    case is an accepted shape with a NULL corpus."""
    q, c = np.ones((1, max(dim, 1)), np.float32), np.ones((4, max(dim, 1)), np.float32)
    idx, sc = np.full((1, 4), 77, np.int64), np.full((1, 4), 7.5, np.float32)
    hits, stats = C.c_int64(99), (C.c_uint64 * 4)(9, 9, 9, 9)
    null = code == KjarniError.NULL_POINTER
    assert _host_call(q, None if null else c, dim, k, idx, sc, hits, stats, nq=nq) == code
    assert (idx == 77).all() and (sc == 7.5).all() and hits.value == 99 and list(stats) == [9, 9, 9, 9]


def test_null_and_refused_device_calls():
    L = lib()
    one = C.c_void_p(4096)   # (never dereferenced: the calls below return before any GPU work)
    assert L.kjarni_hip_cosine_encode(0, None, 4, 64, one, None) == KjarniError.NULL_POINTER
    assert L.kjarni_hip_cosine_encode(0, one, 4, 64, None, None) == KjarniError.NULL_POINTER
    assert L.kjarni_hip_cosine_encode(0, one, 4, 96, one, None) == KjarniError.INVALID_CONFIG
    args = [0, one, 1, one, 4, 64, 0, 2, one, one, one, one, None, None]
    for at in (1, 3, 8, 9, 10, 11):
        a = list(args)
        a[at] = None
        assert L.kjarni_hip_cosine_search_coded(*a) == KjarniError.NULL_POINTER
    for at, v in ((5, 100), (5, 2048), (7, 1025), (2, 1025)):
        a = list(args)
        a[at] = v
        assert L.kjarni_hip_cosine_search_coded(*a) == KjarniError.INVALID_CONFIG
