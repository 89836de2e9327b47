"""gsa_call_variants on the GPU box: VariantIdentification (SeqVariant.cpp:12-119) computed on the device must give, record for record and
in the serial order, what the host walk (gsah_c_variants, pinned to the reference's VCF files in test_variants_host.py) gives on the
same result -- through the single-contig call, bundles, gsa_align_many_variants and the CLI's -gpuvar."""
import os
import subprocess
import threading

import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu


def host_variants(px, seq, r):
    return hostlib.variants(px, seq, r)


def same(a, b):
    return a[0].dtype == capi.VARIANT_DT and np.array_equal(a[0], b[0]) and tuple(a[1]) == tuple(b[1])


def aligned_variants(al, px, seq):
    """align one contig, call its variants on the device and on the host: (device answer, result dict), parity asserted"""
    r = al.align_contig(seq)
    got = al.call_variants()
    want = host_variants(px, seq, r)
    assert got[0].size == want[0].size and got[1] == want[1], (got[1], want[1])
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:5]
    return got, r


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("cx", dict(sen=1, clr=50), True), ("small", {}, False)])
def test_variants_match_the_host_walk(golden_dir, name, params, wide):
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    al = capi.Aligner(idx, wide=wide, **params)
    kinds, rev, n = set(), 0, 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        (V, cnt), _ = aligned_variants(al, px, seq)
        kinds |= set(V["kind"].tolist()); rev += int((V["rpos"] >= idx.G).sum()); n += V.size
    al.close()
    # the coverage this test stands on (checked on the CPU against the oracle's results too: test_variants_host.py): variants on the reverse
    # strand in every input, and with -sen all five kinds (the default runs of the goldens have no pure-deletion record)
    assert n > 1000 and rev > 0 and kinds >= {0, 1, 3, 4}
    if params:
        assert kinds == {0, 1, 2, 3, 4}


def large_gap_pair(seed=7, n=60000):
    """A reference of n bases and a query that differs from it in stretches of ~110 bp, one every 2 kb: a substitution every 8th base (no 15-mer
    seed fits), three bases deleted and three inserted inside.  Each stretch is ONE gap between two seeds with a query side > 64: a large DP job."""
    rng = np.random.default_rng(seed)
    ref = synth.random_genome(n, rng)
    other = {65: b"CGT", 67: b"AGT", 71: b"ACT", 84: b"ACG"}
    out, at = [], 0
    for s in range(1500, n - 1500, 2000):
        L = int(rng.integers(100, 120))
        piece = ref[s:s + L].copy()
        for p in range(3, L, 8):
            piece[p] = other[int(piece[p])][int(rng.integers(0, 3))]
        ins = np.frombuffer(bytes(other[int(ref[s + 70])][int(rng.integers(0, 3))] for _ in range(3)), np.uint8)
        piece = np.concatenate([piece[:30], piece[33:70], ins, piece[70:]])      # 3 reference bases missing, 3 query bases extra
        out += [ref[at:s], piece]; at = s + L
    out.append(ref[at:])
    return ref, np.concatenate(out)


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lg")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_variants_of_large_dp_gaps(large_gap_case, dp_safe):
    """The gapped strings of a large DP job are never in the device's string pools (they are written straight into the host's pinned copy):
    the device derives those columns from the job's op string.  dp_safe = 1: one striped job per launch."""
    px, idx, qry = large_gap_case
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    (V, cnt), r = aligned_variants(al, px, qry)
    al.close()
    F, B = r["frags"], r["blocks"]
    owners = 0
    for bi, b in enumerate(B):
        fr = F[b["frag_off"]:b["frag_off"] + b["n_frag"]]
        Vb = V[V["block"] == bi]
        for g in fr[(fr["bseed"] == 0) & (fr["qlen"] > 64) & (fr["rlen"] > 0) & (fr["qlen"] < 300) & (fr["rlen"] < 300)]:
            mine = Vb[(Vb["rpos"] >= g["rpos"] - 1) & (Vb["rpos"] < g["rpos"] + g["rlen"]) & np.isin(Vb["kind"], (0, 3, 4))]
            if set(mine["kind"].tolist()) == {0, 3, 4}:
                owners += 1
    assert owners >= 1, "no large-job gap with substitutions, an insertion and a deletion"


def test_variants_of_a_bundle(golden_dir, cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer (positions and block numbers relative to the contig)"""
    px = os.path.join(golden_dir, "cx")
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [aligned_variants(al, px, c)[0] for c in contigs]
    assert single[2][0].size == 0 and all(single[k][0].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.call_variants(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.call_variants(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.call_variants(-1)
    al.close()


def test_variants_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    al = capi.Aligner(cx_index)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.call_variants()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.call_variants()
    al.run_to(8)
    a = al.call_variants(); b = al.call_variants()
    assert a[0].size > 0 and same(a, b)
    assert same(a, host_variants(px, cur, al.blocks()))
    # the next contig on its way into the other query slot: the pass still reads the current one
    cur_p, nxt_p = al.pinned_copy(cur), al.pinned_copy(nxt)
    al.prefetch_contig(nxt_p)
    al.align_contig(cur_p)
    assert same(al.call_variants(), a)
    al.align_contig(nxt_p)
    assert same(al.call_variants(), host_variants(px, nxt, al.blocks()))
    # no block at all: n = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    V, cnt = al.call_variants()
    assert V.size == 0 and cnt == (0, 0, 0)
    al.close()


@pytest.mark.parametrize("n_ctx,bundle", [(1, True), (1, False), (3, True), (3, False)])
def test_align_many_with_variants(golden_dir, cx_index, cx_queries, n_ctx, bundle):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want = [aligned_variants(g0, px, c)[0] for c in contigs]
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var):
        v = capi.variants_array(var)
        with lock:
            got[ci] = (v, int(res.n_blocks))
        return 0

    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=True)
    assert sorted(got) == list(range(len(contigs)))
    for ci in got:
        assert same(got[ci][0], want[ci]), ci
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1 and not bundle:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=True)
        assert same(got[0][0], want[0])
    for g in ctxs[1:]:
        g.close()
    g0.close()


def run_cli(cwd, *args):
    subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)


@pytest.mark.parametrize("name,extra,maf,vcf", [("cx", [], "cx.maf", "cx.vcf"), ("cx", ["-sen"], "cx_sen.maf", "cx_sen.vcf"), ("small", [], "small.maf", "small.vcf"),
                                                ("cx", ["-no_vcf"], "cx.maf", None)])
def test_cli_gpuvar_golden(golden_dir, tmp_path, name, extra, maf, vcf):
    """-gpuvar: the VCF from the device's records is the reference's, byte for byte; the MAF does not move"""
    run_cli(golden_dir, "-i", name, "-q", f"{name}.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-gpuvar", *extra)
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, maf), "rb").read()
    if vcf:
        assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, vcf), "rb").read()
    else:
        assert not os.path.exists(tmp_path / "out.vcf")
