"""gsa_block_segs on the GPU box: the per-block chain triples {size, dt, dq} computed on the device from the CIGAR walk's run starts must equal what the host walk
over the gapped strings gives (gsah_c_segs, pinned to the reference's MAF files in test_segs_host.py) -- through the single-contig call, bundles,
gsa_align_many_ex and the CLI's -chain."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import chain_from_maf as chm
import cs_from_maf as cm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_cs import large_gap_case, long_indel_case      # noqa: F401  (fixtures: the shapes of the cs tests)

pytestmark = pytest.mark.gpu


def host_segs(r):
    return hostlib.segs(None, None, r)


def same(a, b):
    return a[0].dtype == capi.SEG_BLOCK_DT and a[1].dtype == capi.SEG_DT and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def aligned_segs(al, seq):
    """align one contig, take its triples from the device and from the host: (device answer, result dict, device CIGARs); parity asserted"""
    r = al.align_contig(seq)
    got = al.block_segs()
    want = host_segs(r)
    assert got[0].size == want[0].size == r["blocks"].size and got[1].size == want[1].size, (got[0].size, want[0].size, got[1].size, want[1].size)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:5]
    cblk, ops = al.block_cigars()
    hb, ho = hostlib.cigars(None, seq, r)
    assert np.array_equal(cblk, hb) and np.array_equal(ops, ho)               # the CIGAR pass behind the segs pass gives what it always gave
    cols = got[1]["size"].astype(np.int64) + got[1]["dt"] + got[1]["dq"]
    for bi in range(cblk.size):
        o, n = int(got[0]["seg_off"][bi]), int(got[0]["n_seg"][bi])
        assert int(cols[o:o + n].sum()) == int(r["blocks"]["aln_len"][bi]), bi                     # every column of an untrimmed block is in a triple
    assert same(al.block_segs(), got)                                         # ... and leaves the segs answer alone
    return got, r, (cblk, ops)


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_segs_match_the_host_walk(golden_dir, name, params, wide):
    px = os.path.join(golden_dir, name)
    al = capi.Aligner(indexio.load_index(px), wide=wide, **params)
    rev, one, n_seg, dt_only, dq_only = 0, 0, 0, 0, 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        (blk, sg), r, _ = aligned_segs(al, seq)
        rev += int((r["blocks"]["bdir"] == 0).sum()); one += int((blk["n_seg"] == 1).sum()); n_seg += sg.size
        dt_only += int(((sg["dt"] > 0) & (sg["dq"] == 0)).sum()); dq_only += int(((sg["dq"] > 0) & (sg["dt"] == 0)).sum())
    al.close()
    if name == "cx":
        # the coverage this test stands on: a reverse-strand block, a one-segment block, the second workgroup of the pack pass and many of the run passes, both gap kinds
        assert rev > 0 and one > 0 and n_seg > 2000 and dt_only > 0 and dq_only > 0, (rev, one, n_seg, dt_only, dq_only)


@pytest.mark.parametrize("strand", ["+", "-"])
def test_segs_of_long_indels(long_indel_case, strand):
    """dt and dq above 64 on either strand (CIGAR runs a whole wavefront walks); they exist only because ind = 100 lets the chain cross them"""
    idx, qry = long_indel_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx, ind=100)
    (blk, sg), r, _ = aligned_segs(al, q)
    al.close()
    assert blk.size > 0 and ((r["blocks"]["bdir"] != 0) == (strand == "+")).all()
    assert int(sg["dt"].max()) > 64 and int(sg["dq"].max()) > 64, (int(sg["dt"].max()), int(sg["dq"].max()))


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_segs_of_large_dp_gaps(large_gap_case, dp_safe):
    """The large DP jobs' gapped strings never exist in the device's string pools: the columns come from the job's op string.  dp_safe = 1: one striped job per launch."""
    idx, qry = large_gap_case
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    (blk, sg), r, _ = aligned_segs(al, qry)
    al.close()
    assert ((r["frags"]["bseed"] == 0) & (r["frags"]["aln_len"] > 64)).any() and sg.size > blk.size


def test_segs_of_a_bundle(cx_index, cx_queries):
    """contig k of a bundle: the single-contig answer, asked for out of order and repeatedly"""
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [aligned_segs(al, c)[0] for c in contigs]
    assert single[2][0].size == 0 and single[2][1].size == 0 and all(single[k][1].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.block_segs(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_segs(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_segs(-1)
    al.close()


def test_segs_call_order(cx_index, cx_queries):
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    al = capi.Aligner(cx_index)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.block_segs()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.block_segs()
    al.run_to(8)
    a = al.block_segs()
    assert a[1].size > 0 and same(a, host_segs(al.blocks())) and al.seg_timing()[1] == 1      # (a refused call runs no pass and is not counted)
    # the six passes keep their answers apart, in several orders
    al.lift_set(np.arange(0, int(cx_index.G), 3, dtype=np.int64)); al.track_set(1000)
    cg = al.block_cigars(); v = al.call_variants(); s = al.block_cs(); lf = al.lift(); tk = al.track()
    assert cg[1].size > 0 and v[0].size > 0 and s[1].size > 0 and lf.size > 0 and tk.size > 0
    for order in ("gtlscv", "vgtlsc", "csgtlv", "vcsltg", "gcgsg"):
        for what in order:
            if what == "g":
                assert same(al.block_segs(), a), order
            elif what == "t":
                assert al.track().tobytes() == tk.tobytes(), order
            elif what == "l":
                assert al.lift().tobytes() == lf.tobytes(), order
            elif what == "s":
                g = al.block_cs()
                assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]), order
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
    assert same(al.block_segs(), a)
    al.align_contig(nxt_p)
    assert same(al.block_segs(), host_segs(al.blocks()))
    # no block at all
    n_calls = al.seg_timing()[1]
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    blk, sg = al.block_segs()
    assert blk.size == 0 and sg.size == 0 and al.seg_timing()[1] == n_calls + 1
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,cs", [(1, True, False), (1, False, True), (3, True, True), (3, False, False)])
def test_align_many_with_segs(cx_index, cx_queries, n_ctx, bundle, cs):
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want, want_cig, want_cs = [], [], []
    for c in contigs:
        sg, r, cig = aligned_segs(g0, c)
        want.append(sg); want_cig.append(cig); want_cs.append(hostlib.cs(None, None, r))
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, *rest):
        s = capi.cs_arrays(rest[0]) if cs else None
        g = capi.segs_arrays(rest[-1]); c = capi.cigars_arrays(cig)
        with lock:
            got[ci] = (g, c, s, int(res.n_blocks), var, len(rest))
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]) and got[ci][3] == want[ci][0].size, ci
            assert np.array_equal(got[ci][1][0], want_cig[ci][0]) and np.array_equal(got[ci][1][1], want_cig[ci][1]), ci      # GSA_WANT_SEGS delivers the CIGARs too
            assert got[ci][4] is None and got[ci][5] == (2 if cs else 1)                                                     # one trailing argument for the switch
            if cs:      # the segs pass behind the cs pass reads that pass's walk: both answers are the ones the single calls give
                assert np.array_equal(got[ci][2][0], want_cs[ci][0]) and np.array_equal(got[ci][2][1], want_cs[ci][1]), ci

    capi.align_many(ctxs, contigs, on_result, bundle=bundle, cs=cs, segs=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, cs=cs, segs=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_align_many_want_bits(cx_index, cx_queries):
    """want = GSA_WANT_SEGS alone delivers the CIGARs too; without the bit there is no segs answer behind the gsa_extras (GSA_ERR_STATE)"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    lib = al.lib
    lib.gsa_extras_segs.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.Segs)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        s = capi.Segs()
        rc = lib.gsa_extras_segs(ex, C.byref(s))
        rcs.append((rc, int(s.n_blocks), int(s.n_segs), bool(ex.contents.cig), int(ex.contents.cig.contents.n_ops) if ex.contents.cig else 0, int(res.contents.n_blocks)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_CS, -4), (capi.WANT_VARIANTS, -4), (capi.WANT_SEGS, 0), (capi.WANT_SEGS | capi.WANT_CS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want, (want, rcs)
        if want & capi.WANT_SEGS:
            assert rcs[0][1] == rcs[0][5] > 0 and rcs[0][2] > 0 and rcs[0][3] and rcs[0][4] > rcs[0][2]      # the CIGARs came along
        else:
            assert rcs[0][1] == 0 and rcs[0][2] == 0
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, 8, capi.RESULT_EX_FN(cb), None) == -1      # bit 8 stays unknown: GSA_ERR_ARG
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, 128, capi.RESULT_EX_FN(cb), None) == -1
    al.close()


def run_cli(cwd, *args):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE).stderr


@pytest.mark.parametrize("fmt", [["-fmt", "1"], ["-fmt", "3", "-cs"]])
@pytest.mark.parametrize("name,extra,maf,vcf", [("cx", [], "cx.maf", "cx.vcf"), ("cx", ["-sen"], "cx_sen.maf", "cx_sen.vcf"), ("cx", ["-unique"], "cx_unique.maf", "cx_unique.vcf"),
                                                ("small", [], "small.maf", "small.vcf")])
def test_cli_chain_golden(golden_dir, tmp_path, name, extra, maf, vcf, fmt):
    """-chain: out.chain is the chain file the reference's own MAF implies (chain_from_maf); the MAF or PAF and the VCF beside it are the files they are without it"""
    err = run_cli(golden_dir, "-i", name, "-q", f"{name}.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", *fmt, "-chain", "-timing", *extra)
    assert open(tmp_path / "out.chain", "rb").read() == chm.chain_of_maf(os.path.join(golden_dir, maf))
    if fmt[1] == "1":
        assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, maf), "rb").read()
    else:
        assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(os.path.join(golden_dir, maf))
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, vcf), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"chain_s": ' in timing[0]


def test_cli_without_chain_writes_no_chain_file(golden_dir, tmp_path):
    run_cli(golden_dir, "-i", "small", "-q", "small.qry.fa", "-o", str(tmp_path / "out"), "-t", "1")
    assert os.path.exists(tmp_path / "out.maf") and not os.path.exists(tmp_path / "out.chain")
