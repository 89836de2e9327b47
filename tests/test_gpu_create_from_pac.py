"""gsa_create_from_pac (capi.Aligner.from_reference): a context whose index is built in device memory from the .pac bytes -- the suffix sort of
gsa_build_index, its SA array adopted as the dense SA -- against the context gsa_create_opts makes from the index FILES of the same sequence (written by
the serial host builder, SA-IS, which test_host_components.py pins to the reference's builder): every device table bit for bit
(gsa_export_index_table), the results of every stage, the life cycle, the memory a context keeps, the argument checks, and the CLI's -memindex.
Every comparison is exact equality."""
import ctypes as C
import os
import shutil
import subprocess
import threading

import numpy as np
import pytest

from conftest import GOLDEN, assert_stage_equal
from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu
GSA_ERR_ARG, GSA_ERR_LIMIT = -1, -5
TABLES = list(capi.Aligner.TABLES)


def _ascii(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)]


def _shapes():
    rng = np.random.default_rng(20261019)
    R = lambda n: synth.random_genome(n, rng)
    out = {}
    for G in (1, 2, 3, 5, 31, 32, 33):                       # the smallest shapes: shorter than one sort key, on its edge, every G % 4
        out[f"G{G}"] = [R(G)]
    out["G2049"] = [R(2049)]                                  # 4 099 rows: inside one 2^16-row super-block of the forced-wide layout
    out["allA4099"] = [_ascii(np.zeros(4099))]                # A...AT...T: one doubling round per power of two, a BWT of two runs
    out["unit997x64"] = [np.tile(R(997), 64)]                 # a tandem repeat: deep doubling, Occ counts that grow in lockstep
    c = R(20000)
    out["twice20k"] = [c, c.copy()]                           # two identical contigs
    h = R(2500)
    out["selfrc5k"] = [np.concatenate([h, synth.revcomp(h)])]    # equal to its own reverse complement
    out["rand70001"] = [R(70001)]                             # 140 003 rows: over two super-block boundaries of the forced-wide layout, G % 4 = 1
    return out


SHAPES = _shapes()
SMALLEST = [f"G{G}" for G in (1, 2, 3, 5, 31, 32, 33)]


class Ref:
    """A reference as both constructors take it: the index files' arrays (indexio) and the .pac bytes with the sequence lengths."""

    def __init__(self, prefix):
        self.prefix = prefix
        self.idx = indexio.load_index(prefix)
        self.G = self.idx.G
        self.pac = np.fromfile(prefix + ".pac", dtype=np.uint8)[:(self.G + 3) // 4].copy()
        self.lens = self.idx.chr_len

    def from_files(self, **kw):
        return capi.Aligner(self.idx, **kw)

    def from_pac(self, **kw):
        return capi.Aligner.from_reference(self.pac, self.G, self.lens, **kw)


@pytest.fixture(scope="module")
def refs(golden_dir, tmp_path_factory):
    """name -> Ref; the shapes' index files are written once, by the serial host builder"""
    cache = {"cx": Ref(os.path.join(golden_dir, "cx")), "small": Ref(os.path.join(golden_dir, "small"))}
    d = tmp_path_factory.mktemp("from_pac")

    def get(name):
        if name not in cache:
            fa = str(d / f"{name}.fa")
            synth.write_fasta(fa, [(f"c{k}", s) for k, s in enumerate(SHAPES[name])])
            old = os.environ.get("GSA_INDEX_THREADS")
            os.environ["GSA_INDEX_THREADS"] = "1"
            try:
                hostlib.build_index(fa, str(d / name))
            finally:
                if old is None:
                    del os.environ["GSA_INDEX_THREADS"]
                else:
                    os.environ["GSA_INDEX_THREADS"] = old
            cache[name] = Ref(str(d / name))
        return cache[name]
    return get


def _tables(a):
    return {t: a.index_table(t) for t in TABLES}


def _assert_same_tables(got, want, what):
    for t in TABLES:
        assert got[t].size == want[t].size, f"{what}: table {t}: {got[t].size} bytes, from the files {want[t].size}"
        assert np.array_equal(got[t], want[t]), f"{what}: table {t} differs, first at byte {np.flatnonzero(got[t] != want[t])[:5]}"


def _pinned_k(G):
    """the k gsa_create chooses from the text length, capped at 11 (4^11 entries: 67 / 134 MB to export): pinned, so that two contexts cannot differ by what
    the free device memory was when each was made"""
    k = 0
    while (1 << (2 * k)) < 2 * G:
        k += 1
    return min(k + 2, 11)


# ---- tables -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name,params", [("cx", dict(slen=12)), ("cx", dict(sen=1, clr=50)), ("small", dict(slen=12)), ("G2049", dict(slen=12)), ("allA4099", dict(slen=12)),
                                         ("unit997x64", dict(slen=12)), ("twice20k", dict(slen=12)), ("selfrc5k", dict(slen=12)), ("rand70001", dict(slen=12))])
def test_every_table_is_the_one_from_the_index_files(refs, name, params, wide):
    """-slen 12: a presence table of 8 MB instead of the default's 537 (the defaults: next test); -sen: the short k-mer table exists (k = 10 under the pinned 11)"""
    r = refs(name)
    k = _pinned_k(r.G)
    a = r.from_files(wide=wide, kmer_k=k, **params); want = _tables(a); a.close()
    b = r.from_pac(wide=wide, kmer_k=k, **params); got = _tables(b); b.close()
    hdr = want["header"].view(np.uint64)
    assert hdr[0] == r.idx.hdr[0] and hdr[1] == 0 and np.array_equal(hdr[2:], r.idx.hdr[1:])
    assert want["sa_dense"].size == (2 * r.G + 1) * (8 if wide else 4) and (want["occ_base"].size > 0) == wide and want["ref"].size == 2 * r.G
    assert want["kmer"].size == (32 if wide else 16) << (2 * k) and (want["kmer_lo"].size > 0) == ("sen" in params and k > 10)
    _assert_same_tables(got, want, f"{name} {'wide' if wide else 'narrow'}")


def test_every_table_with_the_defaults(refs):
    """default parameters, k chosen by the library from the text length and the free device memory -- one context at a time, so both see the same"""
    r = refs("cx")
    a = r.from_files(); want = _tables(a); a.close()
    b = r.from_pac(); got = _tables(b); b.close()
    assert want["pres"].size == 32 << 24 and want["kmer"].size > 0
    _assert_same_tables(got, want, "cx, defaults")


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("name", SMALLEST)
def test_smallest_references(refs, name, wide):
    """Whatever gsa_create_opts does with a reference of a few bases, gsa_create_from_pac does: the same tables, or the same error code."""
    r = refs(name)
    want = err_files = None
    try:
        a = r.from_files(wide=wide, slen=12); want = _tables(a); a.close()
    except capi.GsaError as e:
        err_files = e.code
    try:
        b = r.from_pac(wide=wide, slen=12); got = _tables(b); b.close()
    except capi.GsaError as e:
        assert err_files is not None and e.code == err_files, f"{name}: from the files {err_files}, from the .pac bytes {e.code}: {e}"
        return
    assert err_files is None, f"{name}: gsa_create_opts refused ({err_files}), gsa_create_from_pac did not"
    _assert_same_tables(got, want, name)


# ---- results ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_cx_stages_are_the_goldens(refs, cx_queries, wide):
    want = np.load(os.path.join(GOLDEN, "cx_stages.npz"))
    r = refs("cx")
    a = r.from_files(wide=wide); b = r.from_pac(wide=wide)
    for ci, (name, seq) in enumerate(cx_queries):
        a.set_query(seq); b.set_query(seq)
        da, db = a.dump_stages(8), b.dump_stages(8)
        assert_stage_equal(db, want, prefix=f"c{ci}_")
        assert_stage_equal(db, da)
    a.close(); b.close()


def test_small_stages(refs, golden_dir):
    """(no stage dump of `small` is committed: its golden is the MAF of the whole program, which the CLI tests compare)"""
    r = refs("small")
    a = r.from_files(); b = r.from_pac()
    for name, seq in synth.read_fasta(os.path.join(golden_dir, "small.qry.fa")):
        a.set_query(seq); b.set_query(seq)
        da = a.dump_stages(8)
        assert da["s8_b_score"].size > 0
        assert_stage_equal(b.dump_stages(8), da)
    a.close(); b.close()


@pytest.fixture(scope="module")
def fresh(tmp_path_factory):
    """600 kb in two reference contigs: a 5 kb exact repeat, a 5 kb reverse-complement repeat, an N run; the query is the reference at 1 % divergence with indels"""
    d = tmp_path_factory.mktemp("fresh")
    rng = np.random.default_rng(600)
    c1, c2 = synth.random_genome(350001, rng), synth.random_genome(250002, rng)
    c1[200000:205000] = c1[50000:55000]
    c2[100000:105000] = synth.revcomp(c1[120000:125000])
    c2[180000:180400] = ord("N")
    fa = str(d / "r.fa")
    synth.write_fasta(fa, [("r1", c1), ("r2", c2)])
    old = os.environ.get("GSA_INDEX_THREADS"); os.environ["GSA_INDEX_THREADS"] = "1"
    try:
        hostlib.build_index(fa, str(d / "r"))
    finally:
        if old is None:
            del os.environ["GSA_INDEX_THREADS"]
        else:
            os.environ["GSA_INDEX_THREADS"] = old
    r = Ref(str(d / "r"))
    # (the query is cut from the text the index holds: the N run is what the builder made of it)
    fwd = r.idx.ref[:r.G]
    qs = [synth.mutate(fwd[:350001], 0.01, rng), synth.revcomp(synth.mutate(fwd[350001:], 0.01, rng))]
    return r, qs


def test_fresh_pair_stage_8_and_the_search_leaf(fresh):
    r, qs = fresh
    assert r.lens.tolist() == [350001, 250002]
    a = r.from_files(); b = r.from_pac()
    rng = np.random.default_rng(7)
    for seq in qs:
        ra, rb = a.align_contig(seq), b.align_contig(seq)
        assert ra["blocks"].size > 0 and ra["frags"].size > ra["blocks"].size and ra["aln1"].size > 0
        for key in ("blocks", "frags", "aln1", "aln2"):
            assert np.array_equal(ra[key], rb[key]), key
    seq = qs[0]
    a.set_query(seq); b.set_query(seq)
    starts = rng.integers(0, seq.size - 1, size=2000).astype(np.int32)
    stops = np.minimum((starts // 10000 + 1) * 10000, seq.size).astype(np.int32)
    la, fa, oa = a.bwt_search_batch(starts, stops)
    lb, fb, ob = b.bwt_search_batch(starts, stops)
    assert la.max() >= 15 and fa.max() >= 2
    assert np.array_equal(la, lb) and np.array_equal(fa, fb)
    for i in range(starts.size):
        assert np.array_equal(oa[i, :fa[i]], ob[i, :fb[i]]), i
    a.close(); b.close()


# ---- life cycle ---------------------------------------------------------------------------------------------------------------------------------------------
def _assert_cx_stage_8(g, cx_queries, want, what):
    for ci, (name, seq) in enumerate(cx_queries):
        g.set_query(seq)
        assert_stage_equal(g.dump_stages(8), want, prefix=f"c{ci}_", stages=[8])


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
def test_clones_of_a_context_from_pac(refs, cx_queries, wide):
    want = np.load(os.path.join(GOLDEN, "cx_stages.npz"))
    parent = refs("cx").from_pac(wide=wide)
    child = parent.clone()
    copy = parent.clone_to_device(0)
    _assert_cx_stage_8(child, cx_queries, want, "gsa_clone")
    _assert_same_tables(_tables(copy), _tables(parent), "gsa_clone_to_device")
    child.close(); parent.close()
    _assert_cx_stage_8(copy, cx_queries, want, "gsa_clone_to_device, parent destroyed")
    copy.close()


def test_two_threads_on_one_device(refs, golden_dir):
    r = refs("small")
    a = r.from_files(kmer_k=10); want = _tables(a); a.close()
    res, errs = [None, None], []

    def work(k):
        try:
            g = r.from_pac(kmer_k=10)
            res[k] = _tables(g)
            g.close()
        except Exception as e:      # (reported by the main thread)
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        _assert_same_tables(res[k], want, f"thread {k}")


# ---- memory -------------------------------------------------------------------------------------------------------------------------------------------------
def _free_device_bytes():
    """The free bytes torch.cuda.mem_get_info() reports, i.e. hipMemGetInfo -- asked of the HIP runtime libgsa_hip.so itself runs on (found among the mapped
    files): torch brings a runtime of its own, and that one finds no GPU in a process in which the library's has opened it first."""
    capi.load_library()
    paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln and "torch" not in ln}
    assert len(paths) == 1, paths
    hip = C.CDLL(paths.pop())
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    assert hip.hipDeviceSynchronize() == 0
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return int(fr.value)


def test_a_context_from_pac_keeps_nothing_of_the_builder(tmp_path, monkeypatch):
    """1 000 003 bases: the builder's smallest per-suffix array is 8 MB, its sort scratch 24 MB -- one of them kept shows over the margin of 4 MB.
    Noise: two gsa_create_opts contexts made one after the other hold the same amount to within NOISE_MB (printed below; measured on an MI355X: 0.0 MB, and 2.1 MB more held from the .pac bytes);
    were it above 2 MB, the margin would be twice it."""
    monkeypatch.setenv("GSA_INDEX_THREADS", "1")
    rng = np.random.default_rng(1000003)
    fa = str(tmp_path / "m.fa")
    synth.write_fasta(fa, [("m", synth.random_genome(1000003, rng))])
    hostlib.build_index(fa, str(tmp_path / "m"))
    r = Ref(str(tmp_path / "m"))
    k = _pinned_k(r.G)

    def held(make):
        before = _free_device_bytes()
        g = make(kmer_k=k, slen=12)
        free = _free_device_bytes()
        g.close()
        return before - free

    held(r.from_files)      # (the first context of a process also pays for what the runtime sets up once)
    f1, f2 = held(r.from_files), held(r.from_files)
    p = held(r.from_pac)
    noise = abs(f1 - f2)
    margin = 4 << 20 if noise <= 2 << 20 else 2 * noise
    print(f"held by a context: from the files {f1 / 1e6:.1f} MB and {f2 / 1e6:.1f} MB (NOISE_MB = {noise / 1e6:.1f}), from the .pac bytes {p / 1e6:.1f} MB")
    assert p <= max(f1, f2) + margin, (p, f1, f2)


# ---- errors -------------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_checks_and_the_bound(refs):
    lib = capi.load_library()
    lib.gsa_create_from_pac.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(capi.Params), C.c_uint32, C.POINTER(C.c_void_p)]
    r = refs("small")
    lens = np.ascontiguousarray(r.lens, dtype=np.int32)

    def call(pac, G, ln, n, flags=0):
        ctx = C.c_void_p()
        rc = lib.gsa_create_from_pac(0, C.c_void_p(pac.ctypes.data) if pac is not None else None, G, C.c_void_p(ln.ctypes.data), n, None, flags, C.byref(ctx))
        assert (rc == 0) == bool(ctx.value)
        if ctx.value:
            lib.gsa_destroy(ctx)
        return rc

    def valid():
        g = r.from_pac(kmer_k=10); g.close()

    one = np.zeros(1, np.uint8)                                   # ONE byte of pac: the library must refuse before it reads 268 435 456 of them
    big = np.array([1073741823], np.int32)
    assert call(one, 1073741823, big, 1) == GSA_ERR_LIMIT and b"1 073 741 822" in lib.gsa_last_error(None)
    valid()
    bad = lens.copy(); bad[0] += 1
    assert call(r.pac, r.G, bad, lens.size) == GSA_ERR_ARG and b"sum(chr_len)" in lib.gsa_last_error(None)
    valid()
    assert call(r.pac, r.G, lens, 0) == GSA_ERR_ARG
    valid()
    assert call(None, r.G, lens, lens.size) == GSA_ERR_ARG
    valid()
    assert call(r.pac, r.G, lens, lens.size, flags=1 << 20) == GSA_ERR_ARG and b"unknown flag" in lib.gsa_last_error(None)
    valid()
    assert call(r.pac, r.G, lens, lens.size, flags=4) == 0       # GSA_CREATE_REF_PAC: implied, accepted
    # argument errors come before the bound
    assert call(None, 1073741823, big, 1) == GSA_ERR_ARG and call(one, 1073741823, big, 0) == GSA_ERR_ARG


# ---- the CLI ------------------------------------------------------------------------------------------------------------------------------------------------
def _golden(golden_dir, fn):
    return open(os.path.join(golden_dir, fn), "rb").read()


def _run(cwd, *args):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE).stderr.decode()


def test_cli_memindex_writes_no_index(golden_dir, tmp_path):
    """the copy of cx.ref.fa is called `cx`, so the VCF's ##reference line is that of the golden run (-i cx)"""
    shutil.copy(os.path.join(golden_dir, "cx.ref.fa"), tmp_path / "cx")
    err = _run(tmp_path, "-r", "cx", "-q", os.path.join(golden_dir, "cx.qry.fa"), "-memindex", "-o", "out", "-t", "1")
    assert "-memindex:" not in err
    assert sorted(os.listdir(tmp_path)) == ["cx", "out.maf", "out.vcf"]
    assert open(tmp_path / "out.maf", "rb").read() == _golden(golden_dir, "cx.maf")
    assert open(tmp_path / "out.vcf", "rb").read() == _golden(golden_dir, "cx.vcf")


def test_cli_memindex_paf_and_gpu_variants(golden_dir, tmp_path):
    a = tmp_path / "a"; a.mkdir()
    shutil.copy(os.path.join(golden_dir, "cx.ref.fa"), a / "cx")
    _run(a, "-r", "cx", "-q", os.path.join(golden_dir, "cx.qry.fa"), "-memindex", "-gpuvar", "-fmt", "3", "-o", "out", "-t", "1")
    assert sorted(os.listdir(a)) == ["cx", "out.paf", "out.vcf"]
    assert open(a / "out.vcf", "rb").read() == _golden(golden_dir, "cx.vcf")
    _run(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-gpuvar", "-fmt", "3", "-o", str(tmp_path / "b"), "-t", "1")
    paf = open(a / "out.paf", "rb").read()
    assert len(paf) > 1000 and paf == open(tmp_path / "b.paf", "rb").read()


def test_cli_memindex_with_an_existing_index_is_ignored(golden_dir, tmp_path):
    err = _run(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-memindex", "-o", str(tmp_path / "out"), "-t", "1")
    assert len([ln for ln in err.split("\n") if "-memindex" in ln]) == 1
    assert open(tmp_path / "out.maf", "rb").read() == _golden(golden_dir, "cx.maf")
    assert open(tmp_path / "out.vcf", "rb").read() == _golden(golden_dir, "cx.vcf")
