"""gsa_block_cigars on the GPU box: the per-block CIGARs computed on the device from records, op strings and the two sequences must equal, op
for op and count for count, what the host walk over the gapped strings gives (gsah_c_cigars, pinned to the reference's MAF files in
test_cigars_host.py) -- through the single-contig call, bundles, gsa_align_many_ex and the CLI's -fmt 3."""
import os
import subprocess
import threading

import numpy as np
import pytest

import paf_from_maf as pm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu


def host_cigars(seq, r):
    return hostlib.cigars(None, seq, r)


def same(a, b):
    return a[0].dtype == capi.BLOCK_CIGAR_DT and a[1].dtype == np.uint32 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def aligned_cigars(al, seq):
    """align one contig, take its CIGARs from the device and from the host: (device answer, result dict), parity asserted"""
    r = al.align_contig(seq)
    got = al.block_cigars()
    want = host_cigars(seq, r)
    assert got[0].size == want[0].size == r["blocks"].size and got[1].size == want[1].size, (got[0].size, want[0].size, got[1].size, want[1].size)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:5]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:5]
    return got, r


def record_runs(r, b):
    """runs per record of block b, each record taken alone: 1 for a seed, the runs of its two gapped strings for a gap"""
    F = r["frags"][b["frag_off"]:b["frag_off"] + b["n_frag"]]
    n = 0
    for f in F:
        if f["bseed"]:
            n += 1
        elif f["aln_len"]:
            o, l = int(f["aln_off"]), int(f["aln_len"])
            n += len(pm.rle(pm.column_classes(r["aln1"][o:o + l].tobytes(), r["aln2"][o:o + l].tobytes())))
    return n


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("cx", dict(sen=1, clr=50), True), ("small", {}, False)])
def test_cigars_match_the_host_walk(golden_dir, name, params, wide):
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    al = capi.Aligner(idx, wide=wide, **params)
    classes, rev, merged, n_ops = set(), 0, 0, 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        (blk, ops), r = aligned_cigars(al, seq)
        classes |= set((ops & 15).tolist()); rev += int((r["blocks"]["bdir"] == 0).sum()); n_ops += ops.size
        for bi, b in enumerate(r["blocks"]):
            assert int(blk["n_eq"][bi]) + int(blk["n_x"][bi]) + int(blk["n_ins"][bi]) + int(blk["n_del"][bi]) == int(b["aln_len"])
            merged += int(blk["n_cig"][bi] < record_runs(r, b))
    al.close()
    # the coverage this test stands on: a reverse-strand block, all four classes, and blocks in which a run spans a record boundary (fewer ops than
    # the records' own runs add up to)
    assert n_ops > 1000 and rev > 0 and classes == {1, 2, 7, 8} and merged > 0, (n_ops, rev, classes, merged)


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgc")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_cigars_of_large_dp_gaps(large_gap_case, dp_safe):
    """Gaps of more than 64 columns are walked by a whole wavefront, and they are large DP jobs: their gapped strings never exist in the device's
    string pools, the columns come from the job's op string.  dp_safe = 1: one striped job per launch."""
    px, idx, qry = large_gap_case
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    (blk, ops), r = aligned_cigars(al, qry)
    al.close()
    owners = 0
    for f in r["frags"][(r["frags"]["bseed"] == 0) & (r["frags"]["aln_len"] > 64)]:
        o, l = int(f["aln_off"]), int(f["aln_len"])
        if {8, 1, 2} <= set(pm.column_classes(r["aln1"][o:o + l].tobytes(), r["aln2"][o:o + l].tobytes()).tolist()):
            owners += 1
    assert owners >= 1, "no gap of more than 64 columns with X, I and D columns"


def test_cigars_of_a_bundle(cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer, asked for out of order and repeatedly"""
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [aligned_cigars(al, c)[0] for c in contigs]
    assert single[2][0].size == 0 and single[2][1].size == 0 and all(single[k][1].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.block_cigars(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_cigars(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.block_cigars(-1)
    al.close()


def test_cigars_call_order(cx_index, cx_queries):
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    al = capi.Aligner(cx_index)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.block_cigars()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.block_cigars()
    al.run_to(8)
    a = al.block_cigars(); b = al.block_cigars()
    assert a[1].size > 0 and same(a, b)
    assert same(a, host_cigars(cur, al.blocks()))
    # the variant pass and the CIGAR pass keep their answers apart
    v = al.call_variants()
    assert same(al.block_cigars(), a) and v[0].size > 0
    # the next contig on its way into the other query slot: the pass still reads the current one
    cur_p, nxt_p = al.pinned_copy(cur), al.pinned_copy(nxt)
    al.prefetch_contig(nxt_p)
    al.align_contig(cur_p)
    assert same(al.block_cigars(), a)
    al.align_contig(nxt_p)
    assert same(al.block_cigars(), host_cigars(nxt, al.blocks()))
    # no block at all: n_blocks = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    blk, ops = al.block_cigars()
    assert blk.size == 0 and ops.size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants", [(1, True, False), (1, False, True), (3, True, True), (3, False, False)])
def test_align_many_with_cigars(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want, want_var = [], []
    for c in contigs:
        (cg, r) = aligned_cigars(g0, c)
        want.append(cg); want_var.append(hostlib.variants(px, c, r))
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig):
        c = capi.cigars_arrays(cig)
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (c, v, int(res.n_blocks))
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]) and got[ci][2] == want[ci][0].size, ci
            if variants:
                assert np.array_equal(got[ci][1][0], want_var[ci][0]) and tuple(got[ci][1][1]) == tuple(want_var[ci][1]), ci
            else:
                assert got[ci][1] is None

    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cigars=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def run_cli(cwd, *args):
    subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.mark.parametrize("gpuvar", [[], ["-gpuvar"]])
@pytest.mark.parametrize("name,extra,maf,vcf", [("cx", [], "cx.maf", "cx.vcf"), ("cx", ["-sen"], "cx_sen.maf", "cx_sen.vcf"), ("cx", ["-unique"], "cx_unique.maf", "cx_unique.vcf"),
                                                ("small", [], "small.maf", "small.vcf")])
def test_cli_fmt3_golden(golden_dir, tmp_path, name, extra, maf, vcf, gpuvar):
    """-fmt 3: out.paf is, byte for byte, the PAF the reference's own MAF implies (paf_from_maf); the VCF is the reference's, with the variants from
    the host walk and from the device (-gpuvar)"""
    run_cli(golden_dir, "-i", name, "-q", f"{name}.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-fmt", "3", *extra, *gpuvar)
    assert open(tmp_path / "out.paf", "rb").read() == pm.paf_of_maf(os.path.join(golden_dir, maf))
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, vcf), "rb").read()
    assert not os.path.exists(tmp_path / "out.maf")


def test_cli_fmt1_still_golden(golden_dir, tmp_path):
    run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-fmt", "1")
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    assert not os.path.exists(tmp_path / "out.paf")
