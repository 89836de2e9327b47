"""CPU-side checks of the wide index builder's seam: the argument checks gsa_build_index_opts makes before any device work and their order, its bound, the
answers of the old symbol beside it, and the batch planner (gsa_plan_index_batches, a host function) on histograms made for its edges.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from gsalign_amd import capi, hostlib

GSA_ERR_ARG, GSA_ERR_HIP, GSA_ERR_LIMIT = -1, -2, -5
LIMIT = (1 << 31) - 2


@pytest.fixture(scope="module")
def lib():
    capi.build_library(); hostlib.build()
    lib = capi.load_library()
    lib.gsa_build_index.argtypes = capi.BUILD_INDEX_ARGTYPES
    lib.gsa_build_index_opts.argtypes = capi.BUILD_INDEX_OPTS_ARGTYPES
    return lib


def _opts(lib, pac, G, flags=0, cap=0, seg=0, primary=True, L2=True, bwt=True, sa=True):
    p = C.c_uint64(); l2 = (C.c_uint64 * 5)(); b = np.zeros(64, np.uint32); s = np.zeros(64, np.uint64)
    return lib.gsa_build_index_opts(0, C.c_void_p(pac.ctypes.data) if pac is not None else None, G, flags, cap, seg, C.byref(p) if primary else None, l2 if L2 else None,
                                    C.c_void_p(b.ctypes.data) if bwt else None, C.c_void_p(s.ctypes.data) if sa else None)


def _old(lib, pac, G):
    p = C.c_uint64(); l2 = (C.c_uint64 * 5)(); b = np.zeros(64, np.uint32); s = np.zeros(64, np.uint64)
    return lib.gsa_build_index(0, C.c_void_p(pac.ctypes.data) if pac is not None else None, G, C.byref(p), l2, C.c_void_p(b.ctypes.data), C.c_void_p(s.ctypes.data))


def test_arguments_are_checked_in_order_before_any_device_work(lib):
    pac = np.zeros(16, np.uint8)
    err = lambda: lib.gsa_last_error(None)
    # NULL pointers first, whatever else is wrong
    assert _opts(lib, None, 8) == GSA_ERR_ARG and b"bad argument" in err()
    for kw in ("primary", "L2", "bwt", "sa"):
        assert _opts(lib, pac, 8, flags=2, cap=-1, **{kw: False}) == GSA_ERR_ARG and b"bad argument" in err(), kw
    assert _opts(lib, None, 1 << 40, flags=2) == GSA_ERR_ARG and b"bad argument" in err()
    # G <= 0 before the flags
    assert _opts(lib, pac, 0, flags=2) == GSA_ERR_ARG and b"bad argument" in err()
    assert _opts(lib, pac, -5, cap=-1) == GSA_ERR_ARG and b"bad argument" in err()
    # an unknown flag before the caps, the caps before the bound
    for fl in (2, 4, 1 << 20, 0x80000000):
        assert _opts(lib, pac, 8, flags=fl, cap=-1) == GSA_ERR_ARG and b"unknown flag" in err(), fl
    assert _opts(lib, pac, 8, cap=-1) == GSA_ERR_ARG and b"batch_cap" in err()
    assert _opts(lib, pac, 8, flags=1, seg=-7) == GSA_ERR_ARG and b"occ_segment" in err()
    assert _opts(lib, pac, 1 << 40, flags=2) == GSA_ERR_ARG and _opts(lib, pac, 1 << 40, cap=-1) == GSA_ERR_ARG


def test_the_new_bound(lib):
    """refused before the device is looked at and before pac is read (16 bytes here)"""
    pac = np.zeros(16, np.uint8)
    for fl in (capi.BUILD_AUTO, capi.BUILD_WIDE):
        assert _opts(lib, pac, 1 << 32, flags=fl) == GSA_ERR_LIMIT
        assert b"4 294 967 295" in lib.gsa_last_error(None)
        assert _opts(lib, pac, 1 << 40, flags=fl, cap=1024, seg=4) == GSA_ERR_LIMIT


def test_over_the_old_bound_auto_reaches_the_device_check(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    pac = np.zeros(16, np.uint8)
    assert _opts(lib, pac, 1 << 30) == GSA_ERR_HIP and b"no HIP device" in lib.gsa_last_error(None)
    assert _opts(lib, pac, (1 << 30) - 1) == GSA_ERR_HIP
    assert _opts(lib, pac, (1 << 32) - 1) == GSA_ERR_HIP
    assert _opts(lib, pac, 8) == GSA_ERR_HIP and _opts(lib, pac, 8, flags=capi.BUILD_WIDE, cap=1024, seg=4) == GSA_ERR_HIP
    with pytest.raises(capi.GsaError, match="no HIP device"):
        capi.build_index_arrays(np.zeros(16, np.uint8), 8, wide=True, batch_cap=1024)


def test_the_old_symbol_answers_as_before(lib):
    pac = np.zeros(16, np.uint8)
    assert _old(lib, None, 8) == GSA_ERR_ARG and _old(lib, pac, 0) == GSA_ERR_ARG and _old(lib, pac, -5) == GSA_ERR_ARG
    assert _old(lib, pac, 1 << 30) == GSA_ERR_LIMIT
    assert b"1 073 741 822" in lib.gsa_last_error(None)
    assert _old(lib, pac, (1 << 30) - 1) == GSA_ERR_LIMIT and _old(lib, pac, 1 << 40) == GSA_ERR_LIMIT
    assert len(capi.index_build_stats()) == 2 and len(capi.index_build_stats2()) == 3      # (index_build_stats keeps its two fields, the new ones have an accessor of their own)


def test_set_index_build_caps_refuses_negative_values(lib):
    capi.set_index_build_caps(1024, 4)
    capi.set_index_build_caps(0, 0)
    with pytest.raises(capi.GsaError):
        capi.set_index_build_caps(-1, 0)
    with pytest.raises(capi.GsaError):
        capi.set_index_build_caps(0, -1)
    with pytest.raises(capi.GsaError):
        capi.set_index_build_caps(0, 0, -1)


# ---- the batch planner ------------------------------------------------------------------------------------------------------------------------------------------
def _check_plan(hist, cap):
    hist = np.asarray(hist, dtype=np.uint64)
    first, base = capi.plan_index_batches(hist, cap)
    nb = first.size - 1
    assert nb >= 1 and first[0] == 0 and first[-1] == hist.size and np.all(np.diff(first) > 0)      # every class exactly once, in order
    cum = np.concatenate([[0], np.cumsum(hist.astype(object))])                                      # (Python integers: no overflow)
    for b in range(nb + 1):
        assert int(base[b]) == 1 + int(cum[first[b]]), b                                             # slot bases: the 64-bit prefix sums + 1
    for b in range(nb):
        n = int(cum[first[b + 1]] - cum[first[b]])
        assert n <= cap or first[b + 1] - first[b] == 1, (b, n, first[b], first[b + 1])               # over the cap: a single class
    return first, base


def test_planner_covers_every_class_once_within_the_cap(lib):
    rng = np.random.default_rng(3)
    for cap in (1, 7, 1024, 1 << 20):
        _check_plan(rng.integers(0, 50, 4096), cap)
    _check_plan(np.zeros(16), 5)                          # no suffix at all: one batch
    _check_plan([5], 1)                                   # one class
    f, _ = _check_plan(np.full(256, 4), 8)                # exact fits: two classes per batch
    assert f.size - 1 == 128
    f, _ = _check_plan(np.full(256, 4), 1 << 40)          # everything in one batch
    assert f.size - 1 == 1


def test_planner_gives_a_class_over_the_cap_a_batch_of_its_own(lib):
    f, b = _check_plan([3, 0, 0, 5000, 0, 0, 2, 2, 9000, 1], 1024)
    assert list(f) == [0, 3, 4, 8, 9, 10] and list(b) == [1, 4, 5004, 5008, 14008, 14009]
    f, b = _check_plan([0, 0, 5000, 1], 1024)            # empty classes in front of a class over the cap: a batch of no suffix
    assert list(f) == [0, 2, 3, 4] and list(b) == [1, 1, 5001, 5002]
    f, b = _check_plan([5000, 6000], 1024)
    assert list(f) == [0, 1, 2]


def test_planner_slot_bases_past_2_to_the_32_and_the_class_limit(lib):
    hist = np.array([LIMIT, 5, LIMIT, 0, LIMIT - 1, 2], np.uint64)       # sums to more than 2^32
    f, b = _check_plan(hist, 1 << 30)
    assert list(f) == [0, 1, 2, 3, 4, 5, 6] and int(b[-1]) == 1 + 3 * LIMIT - 1 + 7 and int(b[-1]) > 1 << 32
    f, b = _check_plan(hist, LIMIT)                                      # a full class and an empty one fit together
    assert list(f) == [0, 1, 2, 4, 5, 6]
    with pytest.raises(capi.GsaError, match="prefix class 2 .*2147483647") as ei:
        capi.plan_index_batches(np.array([1, 2, LIMIT + 1, 3], np.uint64), 1 << 30)
    assert ei.value.code == GSA_ERR_LIMIT
    with pytest.raises(capi.GsaError, match=r"\(AG\)") as ei:                # 16 classes: two bases, class 2 = AG
        capi.plan_index_batches(np.array([0, 0, 1 << 40] + [0] * 13, np.uint64), 1 << 30)
    assert ei.value.code == GSA_ERR_LIMIT
    with pytest.raises(capi.GsaError) as ei:
        capi.plan_index_batches(np.array([1, 2], np.uint64), 0)
    assert ei.value.code == GSA_ERR_ARG
