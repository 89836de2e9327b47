"""gsa_block_cs on the GPU box: the per-block cs strings (PAF's cs:Z:, short form) computed on the device from the CIGAR ops, the runs' first positions and
the two sequences must equal, byte for byte, what the host walk over the gapped strings gives (gsah_c_cs, pinned to the reference's MAF files in
test_cs_host.py) -- through the single-contig call, bundles, gsa_align_many_ex and the CLI's -fmt 3 -cs."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import cs_from_maf as cm
import paf_from_maf as pm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu


def host_cs(r):
    return hostlib.cs(None, None, r)


def same(a, b):
    return a[0].dtype == capi.BLOCK_CS_DT and a[1].dtype == np.uint8 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def aligned_cs(al, seq):
    """align one contig, take its cs strings from the device and from the host: (device answer, result dict, device CIGARs); parity and the
    lengths the ops imply asserted"""
    r = al.align_contig(seq)
    got = al.block_cs()
    want = host_cs(r)
    assert got[0].size == want[0].size == r["blocks"].size and got[1].size == want[1].size, (got[0].size, want[0].size, got[1].size, want[1].size)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:5]
    cblk, ops = al.block_cigars()
    hb, ho = hostlib.cigars(None, seq, r)
    assert np.array_equal(cblk, hb) and np.array_equal(ops, ho)               # the CIGAR pass behind the cs pass gives what it always gave
    for bi in range(cblk.size):
        assert int(got[0]["n_cs"][bi]) == capi.cs_of_ops_length(ops[cblk["cig_off"][bi]:cblk["cig_off"][bi] + cblk["n_cig"][bi]]), bi
    assert same(al.block_cs(), got)                                           # ... and leaves the cs answer alone
    return got, r, (cblk, ops)


def longest(ops, code):
    o = ops[(ops & 15) == code]
    return int((o >> 4).max()) if o.size else 0


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_cs_matches_the_host_walk(golden_dir, name, params, wide):
    px = os.path.join(golden_dir, name)
    al = capi.Aligner(indexio.load_index(px), wide=wide, **params)
    kinds, rev, n_bytes, long_x, n_letters = set(), 0, 0, 0, 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        (blk, by), r, (cblk, ops) = aligned_cs(al, seq)
        s = by.tobytes()
        kinds |= {c for c in ":*+-" if c.encode() in s}; rev += int((r["blocks"]["bdir"] == 0).sum()); n_bytes += by.size
        long_x = max(long_x, longest(ops, 8)); n_letters += s.count(b"n")
    al.close()
    if name == "cx":
        # the coverage this test stands on: all four token kinds, a reverse-strand block, an X op walked by a whole wavefront, 'n' letters
        assert kinds == set(":*+-") and rev > 0 and long_x > 64 and n_letters > 0 and n_bytes > 1000, (kinds, rev, long_x, n_letters, n_bytes)


def long_indel_pair(seed=41, n=60000):
    """A random reference of n bases and a query that carries, every 6 kb, alternately a deletion of 70-100 reference bases and an insertion of 70-100
    random bases"""
    rng = np.random.default_rng(seed)
    ref = synth.random_genome(n, rng)
    out, at = [], 0
    for k, p in enumerate(range(3000, n - 3000, 6000)):
        out.append(ref[at:p]); at = p
        m = int(rng.integers(70, 101))
        if k % 2 == 0:
            at += m
        else:
            out.append(synth.random_genome(m, rng))
    out.append(ref[at:])
    return ref, np.ascontiguousarray(np.concatenate(out))


@pytest.fixture(scope="module")
def long_indel_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lic")
    ref, qry = long_indel_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return indexio.load_index(px), qry


@pytest.mark.parametrize("strand", ["+", "-"])
def test_cs_of_long_indel_ops(long_indel_case, strand):
    """I and D ops of more than 64 columns -- written by a whole wavefront -- on either strand; they exist only because ind = 100 lets the chain cross them"""
    idx, qry = long_indel_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx, ind=100)
    (blk, by), r, (cblk, ops) = aligned_cs(al, q)
    al.close()
    assert blk.size > 0 and ((r["blocks"]["bdir"] != 0) == (strand == "+")).all()
    assert longest(ops, 1) > 64 and longest(ops, 2) > 64, (longest(ops, 1), longest(ops, 2))
    al = capi.Aligner(idx)
    _, _, (_, ops25) = aligned_cs(al, q)
    al.close()
    assert longest(ops25, 1) <= 64 and longest(ops25, 2) <= 64                # the default ind: no such op, the parameter matters


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgs")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_cs_of_large_dp_gaps(large_gap_case, dp_safe):
    """The large DP jobs' gapped strings never exist in the device's string pools: the columns come from the job's op string.  dp_safe = 1: one striped
    job per launch."""
    idx, qry = large_gap_case
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    (blk, by), r, _ = aligned_cs(al, qry)
    al.close()
    assert ((r["frags"]["bseed"] == 0) & (r["frags"]["aln_len"] > 64)).any() and {b"*"[0], b"+"[0], b"-"[0]} <= set(by.tolist())


def test_cs_of_a_bundle(cx_index, cx_queries):
    """contig k of a bundle: byte for byte the single-contig answer, asked for out of order and repeatedly"""
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [aligned_cs(al, c)[0] for c in contigs]
    assert single[2][0].size == 0 and single[2][1].size == 0 and all(single[k][1].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.block_cs(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_cs(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_cs(-1)
    al.close()


def test_cs_call_order(cx_index, cx_queries):
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    al = capi.Aligner(cx_index)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.block_cs()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.block_cs()
    al.run_to(8)
    a = al.block_cs()
    assert a[1].size > 0 and same(a, host_cs(al.blocks())) and al.cs_timing()[1] == 1      # (a refused call runs no pass)
    # the three passes keep their answers apart, in any order
    cg = al.block_cigars(); v = al.call_variants()
    assert cg[1].size > 0 and v[0].size > 0
    for order in ("scv", "vsc", "csv", "vcs"):
        for what in order:
            if what == "s":
                assert same(al.block_cs(), a), order
            elif what == "c":
                g = al.block_cigars()
                assert np.array_equal(g[0], cg[0]) and np.array_equal(g[1], cg[1]), order
            else:
                w = al.call_variants()
                assert np.array_equal(w[0], v[0]) and tuple(w[1]) == tuple(v[1]), order
    # the next contig on its way into the other query slot: the pass still reads the current one
    cur_p, nxt_p = al.pinned_copy(cur), al.pinned_copy(nxt)
    al.prefetch_contig(nxt_p)
    al.align_contig(cur_p)
    assert same(al.block_cs(), a)
    al.align_contig(nxt_p)
    assert same(al.block_cs(), host_cs(al.blocks()))
    # no block at all
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    blk, by = al.block_cs()
    assert blk.size == 0 and by.size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants", [(1, True, False), (1, False, True), (3, True, True), (3, False, False)])
def test_align_many_with_cs(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want, want_cig, want_var = [], [], []
    for c in contigs:
        cs, r, cig = aligned_cs(g0, c)
        want.append(cs); want_cig.append(cig); want_var.append(hostlib.variants(px, c, r))
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, cs):
        s = capi.cs_arrays(cs); c = capi.cigars_arrays(cig)
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (s, c, v, int(res.n_blocks))
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]) and got[ci][3] == want[ci][0].size, ci
            assert np.array_equal(got[ci][1][0], want_cig[ci][0]) and np.array_equal(got[ci][1][1], want_cig[ci][1]), ci
            if variants:
                assert np.array_equal(got[ci][2][0], want_var[ci][0]) and tuple(got[ci][2][1]) == tuple(want_var[ci][1]), ci
            else:
                assert got[ci][2] is None

    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cs=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cs=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_align_many_without_cs_keeps_its_callback(cx_index, cx_queries):
    """cigars=True alone: four arguments as before, and behind the gsa_extras there is no cs answer (GSA_ERR_STATE)"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    seen = []
    capi.align_many([al], contigs, lambda ci, res, var, cig: seen.append((ci, var, int(cig.n_blocks))) or 0, cigars=True)
    assert len(seen) == 1 and seen[0][0] == 0 and seen[0][1] is None and seen[0][2] > 0
    lib = al.lib
    lib.gsa_extras_cs.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.Cs)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        s = capi.Cs()
        rcs.append((lib.gsa_extras_cs(ex, C.byref(s)), int(s.n_blocks), int(s.n_bytes), bool(ex.contents.cig)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_VARIANTS, -4), (capi.WANT_CS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want, (want, rcs)
        if want == capi.WANT_CS:
            assert rcs[0][1] == seen[0][2] and rcs[0][2] > 0 and rcs[0][3]          # GSA_WANT_CS implies the CIGARs
        else:
            assert rcs[0][1] == 0 and rcs[0][2] == 0
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, 8, capi.RESULT_EX_FN(cb), None) == -1      # an unknown `want` bit: GSA_ERR_ARG
    al.close()


def run_cli(cwd, *args):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE).stderr


@pytest.mark.parametrize("gpuvar", [[], ["-gpuvar"]])
@pytest.mark.parametrize("name,extra,maf,vcf", [("cx", [], "cx.maf", "cx.vcf"), ("cx", ["-sen"], "cx_sen.maf", "cx_sen.vcf"), ("cx", ["-unique"], "cx_unique.maf", "cx_unique.vcf"),
                                                ("small", [], "small.maf", "small.vcf")])
def test_cli_fmt3_cs_golden(golden_dir, tmp_path, name, extra, maf, vcf, gpuvar):
    """-fmt 3 -cs: every line of out.paf is the line the reference's own MAF implies (paf_from_maf) plus a tab, "cs:Z:" and the string its two `s` lines
    imply (cs_from_maf); the VCF is the reference's"""
    err = run_cli(golden_dir, "-i", name, "-q", f"{name}.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-fmt", "3", "-cs", "-timing", *extra, *gpuvar)
    assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(os.path.join(golden_dir, maf))
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, vcf), "rb").read()
    assert not os.path.exists(tmp_path / "out.maf")
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and timing[0].rstrip().endswith(b"}") and b'"cs_s": ' in timing[0].rsplit(b",", 1)[1]      # appended at the end of the JSON line


def test_cli_cs_is_ignored_without_fmt3(golden_dir, tmp_path):
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-fmt", "1", "-cs")
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    assert not os.path.exists(tmp_path / "out.paf")
    assert sum(1 for ln in err.split(b"\n") if b"-cs" in ln) == 1            # one warning line
