"""CPU-side checks of the index-builder seam: gsa_index_sizes, the argument checks gsa_build_index makes before any device work, and
gsah_build_index_with -- the host builder with its BWT/SA half supplied by a callback -- pinned by a numpy callback that sorts the
suffixes of forward + reverse complement + '$' naively.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

from gsalign_amd import capi, hostlib

GSA_ERR_ARG, GSA_ERR_HIP, GSA_ERR_LIMIT = -1, -2, -5
EXTS = ("bwt", "sa", "pac", "ann", "amb")


@pytest.fixture(scope="module")
def lib():
    capi.build_library(); hostlib.build()
    lib = capi.load_library()
    lib.gsa_build_index.argtypes = capi.BUILD_INDEX_ARGTYPES
    return lib


@pytest.mark.parametrize("name,G", [("cx", 270000), ("small", 60000)])
def test_index_sizes_match_the_golden_files(lib, golden_dir, name, G):
    assert int(open(os.path.join(golden_dir, name + ".ann")).readline().split()[0]) == G
    bwt_words, n_sa = capi.index_sizes(G)
    assert bwt_words == (os.path.getsize(os.path.join(golden_dir, name + ".bwt")) - 40) // 4
    assert n_sa - 1 == (os.path.getsize(os.path.join(golden_dir, name + ".sa")) - 56) // 8      # (sa[0] is not in the file)


def _call(lib, pac, G, primary=True, L2=True, bwt=True, sa=True):
    p = C.c_uint64(); l2 = (C.c_uint64 * 5)(); b = np.zeros(64, np.uint32); s = np.zeros(64, np.uint64)
    return lib.gsa_build_index(0, C.c_void_p(pac.ctypes.data) if pac is not None else None, G, C.byref(p) if primary else None, l2 if L2 else None,
                               C.c_void_p(b.ctypes.data) if bwt else None, C.c_void_p(s.ctypes.data) if sa else None)


def test_arguments_are_checked_before_any_device_work(lib):
    pac = np.zeros(16, np.uint8)
    assert _call(lib, None, 8) == GSA_ERR_ARG
    for kw in ("primary", "L2", "bwt", "sa"):
        assert _call(lib, pac, 8, **{kw: False}) == GSA_ERR_ARG, kw
    assert _call(lib, pac, 0) == GSA_ERR_ARG and _call(lib, pac, -5) == GSA_ERR_ARG
    # over the bound of 32-bit suffix indices: refused before the device is looked at and before pac is read (16 bytes here)
    assert _call(lib, pac, 1 << 30) == GSA_ERR_LIMIT
    assert b"1 073 741 822" in lib.gsa_last_error(None)
    assert _call(lib, pac, (1 << 30) - 1) == GSA_ERR_LIMIT and _call(lib, pac, 1 << 40) == GSA_ERR_LIMIT


def test_no_device_is_an_error_not_a_fallback(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert _call(lib, np.zeros(16, np.uint8), 8) == GSA_ERR_HIP
    with pytest.raises(capi.GsaError, match="no HIP device"):
        capi.build_index_arrays(np.zeros(16, np.uint8), 8)


def naive_bwt_sa(pac, G):
    """The BWT/SA half as index_io.cpp defines it, from a direct sort of the S + 1 suffixes of forward + reverse complement + '$'."""
    codes = ((pac[:, None] >> np.array([6, 4, 2, 0], np.uint8)[None, :]) & 3).reshape(-1)[:G].astype(np.int64)
    S = 2 * G
    T = np.concatenate([codes + 1, (3 - codes[::-1]) + 1, [0]])               # '$' = 0 sorts first
    tb = T.astype(np.uint8).tobytes()
    SA = np.array(sorted(range(S + 1), key=lambda i: tb[i:]), dtype=np.int64)   # ('$' is unique: no suffix is a prefix of another)
    assert SA[0] == S
    primary = int(np.flatnonzero(SA == 0)[0])
    sym = (T[SA[SA != 0] - 1] - 1).astype(np.uint32)                          # row i gives symbol k = i - (i > primary)
    n_words, n_blk = (S + 15) // 16, (S + 127) // 128
    padded = np.zeros(n_words * 16, np.uint32); padded[:S] = sym
    packed = (padded.reshape(-1, 16) << (2 * (15 - np.arange(16, dtype=np.uint32)))[None, :]).sum(axis=1).astype(np.uint32)
    bwt = np.zeros(n_words + (n_blk + 1) * 8, np.uint32)
    cnt = np.zeros(4, np.uint64)
    for g in range(n_blk):
        bwt[16 * g:16 * g + 8] = cnt.view(np.uint32)
        w = packed[8 * g:8 * g + 8]
        bwt[16 * g + 8:16 * g + 8 + w.size] = w
        cnt += np.bincount(sym[128 * g:128 * g + 128], minlength=4).astype(np.uint64)
    bwt[n_blk * 8 + n_words:] = cnt.view(np.uint32)
    sa = SA[::32].astype(np.uint64); sa[0] = np.uint64(0xFFFFFFFFFFFFFFFF)
    hdr = np.concatenate([[primary], np.cumsum(cnt)]).astype(np.uint64)
    return hdr, bwt, sa


@pytest.fixture(scope="module")
def seam_fasta(tmp_path_factory):
    """three short contigs, 701 bases: an N run, lower-case letters, a total that is no multiple of 4"""
    rng = np.random.default_rng(11)
    d = tmp_path_factory.mktemp("seam")
    seqs = ["".join("ACGT"[k] for k in rng.integers(0, 4, n)) for n in (300, 250, 151)]
    seqs[0] = seqs[0][:100] + "N" * 17 + seqs[0][117:]
    seqs[1] = seqs[1][:40] + seqs[1][40:90].lower() + seqs[1][90:]
    seqs[2] = seqs[2][:-9] + "AAAAAAAAA"
    assert sum(map(len, seqs)) == 701
    fa = d / "seam.fa"
    fa.write_text("".join(f">c{k} note {k}\n{s[:70]}\n{s[70:]}\n" for k, s in enumerate(seqs)))
    return str(fa)


def test_callback_seam_is_byte_identical_to_the_host_builder(lib, seam_fasta, tmp_path):
    host, seam, none = str(tmp_path / "host"), str(tmp_path / "seam"), str(tmp_path / "none")
    hostlib.build_index(seam_fasta, host)
    seen = []

    def fn(pac, G):
        seen.append((pac.size, G))
        return naive_bwt_sa(pac, G)

    hostlib.build_index_with(seam_fasta, seam, fn)
    hostlib.build_index_with(seam_fasta, none, None)      # (no callback: the host path itself)
    assert seen == [(176, 701)]
    for ext in EXTS:
        want = open(f"{host}.{ext}", "rb").read()
        assert open(f"{seam}.{ext}", "rb").read() == want, ext
        assert open(f"{none}.{ext}", "rb").read() == want, ext
    assert (os.path.getsize(host + ".bwt") - 40) // 4 == capi.index_sizes(701)[0]


def test_failing_callback_fails_the_build_and_leaves_no_bwt(lib, seam_fasta, tmp_path):
    def boom(pac, G):
        raise KeyError("boom")

    with pytest.raises(RuntimeError, match="callback failed"):
        hostlib.build_index_with(seam_fasta, str(tmp_path / "bad"), boom)
    assert not os.path.exists(tmp_path / "bad.bwt") and not os.path.exists(tmp_path / "bad.sa")
    # arrays of the wrong size are a failure too, not a buffer overrun
    with pytest.raises(RuntimeError, match="wrong size"):
        hostlib.build_index_with(seam_fasta, str(tmp_path / "bad2"), lambda pac, G: (np.zeros(5, np.uint64), np.zeros(3, np.uint32), np.zeros(3, np.uint64)))
    assert not os.path.exists(tmp_path / "bad2.bwt")
