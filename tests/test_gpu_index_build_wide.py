"""The wide device index builder (gsa_build_index_opts with GSA_BUILD_WIDE, GSA_CREATE_SORT_WIDE; k_index_wide.hip): the batched 64-bit suffix sorter and its
derivation passes, forced onto small inputs, against the index files the reference wrote (tests/golden) and against the host builder run serially (SA-IS) on the
shapes of test_gpu_index_build.py (tests/index_shapes.py) and on shapes aimed at the batch seams.  Every comparison is exact equality."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth
from index_shapes import SHAPES, _ascii, _load

pytestmark = pytest.mark.gpu
EXTS = ("bwt", "sa", "pac", "ann", "amb")
TABLES = list(capi.Aligner.TABLES)
GSA_ERR_NOMEM = -3
P = 8                                                             # bases of a prefix class (k_index_wide.hip)


def _check(prefix, **kw):
    pac, G, hdr, bwt, sa = _load(prefix)
    got_hdr, got_bwt, got_sa = capi.build_index_arrays(pac, G, wide=True, **kw)
    assert got_bwt.size == bwt.size and got_sa.size == sa.size
    assert np.array_equal(got_hdr, hdr), (got_hdr, hdr)
    assert np.array_equal(got_bwt, bwt), f"bwt words differ, first at {np.flatnonzero(got_bwt != bwt)[:5]}"
    assert np.array_equal(got_sa, sa), f"sa samples differ, first at {np.flatnonzero(got_sa != sa)[:5]}"
    return pac, G


def _host_index(tmp_path, seqs, name="r"):
    """index files of the sequences from the serial host builder; the prefix"""
    old = os.environ.get("GSA_INDEX_THREADS")
    os.environ["GSA_INDEX_THREADS"] = "1"                      # SA-IS
    try:
        fa = str(tmp_path / f"{name}.fa")
        synth.write_fasta(fa, [(f"c{k}", s) for k, s in enumerate(seqs)])
        hostlib.build_index(fa, str(tmp_path / name))
    finally:
        if old is None:
            del os.environ["GSA_INDEX_THREADS"]
        else:
            os.environ["GSA_INDEX_THREADS"] = old
    return str(tmp_path / name)


def _class_hist(pac, G):
    """(counts of the 4^P prefix classes over the 2G suffixes of forward + reverse complement, the class of suffix 0): what k_ixw_hist counts"""
    codes = ((pac[:, None] >> np.array([6, 4, 2, 0], np.uint8)[None, :]) & 3).reshape(-1)[:G].astype(np.int64)
    T = np.concatenate([codes, 3 - codes[::-1], np.zeros(P, np.int64)])      # padded with A
    cls = np.zeros(2 * G, np.int64)
    for k in range(P):
        cls = cls * 4 + T[k:k + 2 * G]
    return np.bincount(cls, minlength=4 ** P).astype(np.uint64), int(cls[0])


# ---- golden files -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cx", "small"])
def test_golden_index_files_in_one_batch(golden_dir, name):
    _check(os.path.join(golden_dir, name))
    batches, peak, active = capi.index_build_stats2()
    assert batches == 1 and peak > 0


@pytest.mark.parametrize("name", ["cx", "small"])
def test_golden_index_files_in_many_batches_and_segments(golden_dir, name):
    pac, G = _check(os.path.join(golden_dir, name), batch_cap=1024, occ_segment=4)
    batches, peak, active = capi.index_build_stats2()
    hist, _ = _class_hist(pac, G)
    first, base = capi.plan_index_batches(hist, 1024)
    n = np.diff(base.astype(np.int64))
    assert batches == int(np.count_nonzero(n)) and batches > 100
    assert (2 * G + 127) // 128 > 3 * 4                       # several Occ segments
    # (neither golden reference has a prefix class above 1024 suffixes -- their largest hold 308 and 10: a class that is a batch alone is allA4099 / AC3000 below)


# ---- the shapes of test_gpu_index_build.py, forced wide, batch_cap = 1024 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_against_the_serial_host_builder(tmp_path, shape):
    pac, G = _check(_host_index(tmp_path, SHAPES[shape]), batch_cap=1024, occ_segment=4)
    if shape in ("allA4099", "AC3000"):                      # a class above the cap is a batch alone
        first, base = capi.plan_index_batches(_class_hist(pac, G)[0], 1024)
        n = np.diff(base.astype(np.int64))
        assert np.any(n > 1024) and np.all((n <= 1024) | (np.diff(first) == 1))
        assert capi.index_build_stats2()[0] == int(np.count_nonzero(n))


# ---- the batch seams --------------------------------------------------------------------------------------------------------------------------------------------
def test_a_repeat_whose_suffixes_lie_in_different_batches(tmp_path):
    """60 kb, a 5 kb exact repeat: its suffixes begin with every kind of 8-mer, so they sit in all batches, and they tie for 5 kb: the doubling rounds of a batch
    read rank[i + h] of suffixes of other batches, refined in the same round or not yet"""
    rng = np.random.default_rng(60000)
    s = synth.random_genome(60000, rng)
    s[41000:46000] = s[7000:12000]
    _check(_host_index(tmp_path, [s]), batch_cap=8192)
    ms, rounds = capi.index_build_stats()
    batches, peak, active = capi.index_build_stats2()
    print(f"60 kb with a 5 kb repeat: {ms:.2f} ms, {rounds} rounds, {batches} batches, peak {peak / 1e6:.1f} MB")
    assert rounds >= 2 and batches >= 8


def test_a_list_of_tied_suffixes_that_does_not_fit_is_nomem(tmp_path):
    """gsa_set_index_build_caps' active_cap stands in for a device without the room: one entry too few is GSA_ERR_NOMEM with the sizes in the message -- from the
    first pass and, for a context, from gsa_create_from_pac -- nothing faults, nothing stays behind, and with exactly the room needed the build is the host's"""
    rng = np.random.default_rng(60000)
    s = synth.random_genome(60000, rng)
    s[41000:46000] = s[7000:12000]
    prefix = _host_index(tmp_path, [s])
    pac, G = _check(prefix, batch_cap=8192)
    active = capi.index_build_stats2()[2]
    assert 4 * (5000 - 29) <= active <= 4 * 5000 + 64           # the repeat's suffixes on both strands, less those unique within 29 bases; a few chance ties
    idx = indexio.load_index(prefix)
    try:
        for cap in (active - 1, 1000, 1):
            capi.set_index_build_caps(0, 0, cap)
            with pytest.raises(capi.GsaError, match=rf"still tie needs {active} entries.*room for {cap} ") as ei:
                capi.build_index_arrays(pac, G, wide=True, batch_cap=8192)
            assert ei.value.code == GSA_ERR_NOMEM
        capi.set_index_build_caps(8192, 4, active - 1)
        with pytest.raises(capi.GsaError, match="still tie") as ei:
            capi.Aligner.from_reference(pac, G, idx.chr_len, sort_wide=True, slen=12)
        assert ei.value.code == GSA_ERR_NOMEM
        capi.set_index_build_caps(0, 0, active)                  # exactly the room
        _check(prefix, batch_cap=8192)
    finally:
        capi.set_index_build_caps(0, 0, 0)
    _check(prefix, batch_cap=8192)


@pytest.mark.parametrize("where", ["first", "last"])
def test_primary_from_a_batch_relative_slot(tmp_path, where):
    """suffix 0 in the first batch (the text begins with A x 8) and in the last one (T x 8): primary = batch base + relative slot"""
    rng = np.random.default_rng(8)
    body = synth.random_genome(6000, rng)
    lead = _ascii(np.full(8, 0 if where == "first" else 3))
    s = np.concatenate([lead, _ascii([1]), body, _ascii([2])])      # (not A / T at the far end: the reverse strand does not begin the same way)
    prefix = _host_index(tmp_path, [s])
    pac, G = _check(prefix, batch_cap=1024)
    hist, cls0 = _class_hist(pac, G)
    first, base = capi.plan_index_batches(hist, 1024)
    holding = [b for b in range(first.size - 1) if base[b + 1] > base[b]]
    b0 = int(np.searchsorted(first, cls0, side="right")) - 1
    assert len(holding) >= 8 and b0 == (holding[0] if where == "first" else holding[-1])
    assert capi.index_build_stats2()[0] == len(holding)


# ---- a larger text ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big(tmp_path_factory):
    """1 000 003 bases with a 20 kb direct and a 20 kb reverse-complement repeat: the prefix of the host builder's files"""
    rng = np.random.default_rng(77)
    s = synth.random_genome(1000003, rng)
    s[700000:720000] = s[100000:120000]
    s[900000:920000] = synth.revcomp(s[300000:320000])
    return _host_index(tmp_path_factory.mktemp("wide_big"), [s], "big")


def test_large_with_planted_repeats(big):
    _check(big)
    ms, rounds = capi.index_build_stats()
    batches, peak, active = capi.index_build_stats2()
    print(f"1 000 003 bases, forced wide: {ms:.2f} ms on the device, {rounds} doubling rounds, {batches} batch, peak {peak / 1e6:.1f} MB")
    assert rounds >= 2 and ms > 0 and batches == 1


def test_narrow_and_forced_wide_return_identical_arrays(golden_dir):
    pac, G, _, _, _ = _load(os.path.join(golden_dir, "small"))
    a = capi.build_index_arrays(pac, G)
    assert capi.index_build_stats2() == (0, 0, 0)                # the narrow sorter ran
    b = capi.build_index_arrays(pac, G, wide=True, batch_cap=4096, occ_segment=16)
    assert capi.index_build_stats2()[0] > 1
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


# ---- gsa_create_from_pac ----------------------------------------------------------------------------------------------------------------------------------------
def _free_device_bytes():
    """hipMemGetInfo's free bytes, asked of the HIP runtime libgsa_hip.so itself runs on (found among the mapped files)"""
    capi.load_library()
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln and "torch" not in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert hip.hipDeviceSynchronize() == 0
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return int(fr.value)


def test_a_context_sorted_wide_has_the_tables_and_the_memory_of_a_wide_context(big):
    """GSA_CREATE_SORT_WIDE on 1 Mb with a cap of 2^16 (some thirty batches) and Occ segments of 64 blocks: every device table is the one gsa_create_opts makes with
    GSA_CREATE_WIDE from the index files, and the context holds the memory of a GSA_CREATE_WIDE context made from the same bytes without the flag -- within
    the margin of test_gpu_create_from_pac.py: 4 MB, or twice the difference between two such contexts (NOISE) when that is above 2 MB."""
    idx = indexio.load_index(big)
    G = idx.G
    pac = np.fromfile(big + ".pac", dtype=np.uint8)[:(G + 3) // 4].copy()
    k = 11
    held, tables = {}, {}

    def make(what, **kw):
        before = _free_device_bytes()
        g = capi.Aligner(idx, wide=True, kmer_k=k, slen=12) if what == "files" else capi.Aligner.from_reference(pac, G, idx.chr_len, kmer_k=k, slen=12, **kw)
        held[what] = before - _free_device_bytes()
        tables[what] = {t: g.index_table(t) for t in TABLES}
        g.close()

    capi.set_index_build_caps(1 << 16, 64)
    try:
        make("files")           # (the first context of a process also pays for what the runtime sets up once)
        make("wide1", wide=True); make("wide2", wide=True); make("sorted", sort_wide=True)
    finally:
        capi.set_index_build_caps(0, 0)
    want, got = tables["files"], tables["sorted"]
    assert want["sa_dense"].size == (2 * G + 1) * 8 and want["occ_base"].size > 0
    for t in TABLES:
        assert got[t].size == want[t].size, f"table {t}: {got[t].size} bytes, from the files {want[t].size}"
        assert np.array_equal(got[t], want[t]), f"table {t} differs, first at byte {np.flatnonzero(got[t] != want[t])[:5]}"
    w1, w2, p = held["wide1"], held["wide2"], held["sorted"]
    noise = abs(w1 - w2)
    margin = 4 << 20 if noise <= 2 << 20 else 2 * noise
    print(f"held by a wide context from the .pac bytes: {w1 / 1e6:.1f} MB and {w2 / 1e6:.1f} MB (NOISE_MB = {noise / 1e6:.1f}), sorted wide {p / 1e6:.1f} MB")
    assert min(w1, w2) - margin <= p <= max(w1, w2) + margin, (p, w1, w2)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------------------
def _golden(golden_dir, fn):
    return open(os.path.join(golden_dir, fn), "rb").read()


def _run(cwd, *args):
    env = dict(os.environ, GSA_INDEX_64BIT="1", GSA_INDEX_BATCH="4096")
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, env=env, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE).stderr.decode()


def test_cli_gpuindex_forced_wide(golden_dir, tmp_path):
    """the copy of cx.ref.fa is called `cx`, so the index prefix and the VCF's ##reference line are those of the golden run (-i cx)"""
    shutil.copy(os.path.join(golden_dir, "cx.ref.fa"), tmp_path / "cx")
    err = _run(tmp_path, "-r", "cx", "-q", os.path.join(golden_dir, "cx.qry.fa"), "-gpuindex", "-o", "out", "-t", "1")
    assert "-gpuindex:" not in err                            # no fall-back line
    for ext in EXTS:
        assert open(tmp_path / f"cx.{ext}", "rb").read() == _golden(golden_dir, f"cx.{ext}"), ext
    assert open(tmp_path / "out.maf", "rb").read() == _golden(golden_dir, "cx.maf")
    assert open(tmp_path / "out.vcf", "rb").read() == _golden(golden_dir, "cx.vcf")


def test_cli_memindex_forced_wide(golden_dir, tmp_path):
    shutil.copy(os.path.join(golden_dir, "cx.ref.fa"), tmp_path / "cx")
    err = _run(tmp_path, "-r", "cx", "-q", os.path.join(golden_dir, "cx.qry.fa"), "-memindex", "-o", "out", "-t", "1")
    assert "-memindex:" not in err
    assert sorted(os.listdir(tmp_path)) == ["cx", "out.maf", "out.vcf"]      # no index file
    assert open(tmp_path / "out.maf", "rb").read() == _golden(golden_dir, "cx.maf")
    assert open(tmp_path / "out.vcf", "rb").read() == _golden(golden_dir, "cx.vcf")
