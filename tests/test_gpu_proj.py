"""gsa_project on the GPU box: the query projected onto the reference -- a dense word per reference base that every contig, context and device paints into with integer
maxima -- must equal, word for word, what the host walk over records and gapped strings paints (gsah_c_project, pinned to the reference's MAF files in
test_proj_host.py): through single contigs, many records, megabase seeds, large DP gaps, shared and merged accumulators in any order, gsa_align_many_ex and the CLI."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import paf_from_maf as pm
import proj_from_maf as pj
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_result_scan import TILE, dense_snv_case      # noqa: F401  (fixture)
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu


def same(a, b, what=""):
    assert a.dtype == np.uint32 and b.dtype == np.uint32 and a.size == b.size, (what, a.dtype, b.dtype, a.size, b.size)
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:5], [hex(int(v)) for v in a[bad[:5]]], [hex(int(v)) for v in b[bad[:5]]])


def trimmed_spans(idx, r):
    """sum over the result's blocks of the text positions the trimmed block covers"""
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    G, B, F, n = int(idx.G), r["blocks"], r["frags"], 0
    for b in B:
        if b["n_frag"] <= 0:
            continue
        first, last = F[int(b["frag_off"])], F[int(b["frag_off"]) + int(b["n_frag"]) - 1]
        lim = starts[int(b["chr"]) + 1] if b["bdir"] else 2 * G - starts[int(b["chr"])]
        n += max(0, min(int(last["rpos"]) + int(last["rlen"]), int(lim)) - int(first["rpos"]))
    return n


def paint(al, px, idx, seq, host):
    """align one contig, paint it on the device and into `host` on the host: the two stats are equal and n_cols is the sum of the trimmed spans; returns the result"""
    r = al.align_contig(seq)
    st = al.project()
    assert st == hostlib.project(px, seq, r, host), st
    assert st[0] == int((r["blocks"]["n_frag"] > 0).sum()) and st[1] == trimmed_spans(idx, r), (st, trimmed_spans(idx, r))
    return r


def fetched(al, host, what=""):
    """the whole accumulator: words equal to the host's, text equal to gsah_proj_text's"""
    text, words = al.proj_fetch(words=True)
    same(words, host, what)
    assert text == hostlib.proj_text(host), what
    return words


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_projection_matches_the_host_walk(golden_dir, name, params, wide):
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    G = int(idx.G)
    qs = synth.read_fasta(px + ".qry.fa")
    al = capi.Aligner(idx, wide=wide, **params)
    al.proj_open()
    assert not al.proj_fetch(words=True)[1].any()
    host = np.zeros(G, np.uint32)
    for _, seq in qs:
        paint(al, px, idx, seq, host)
    w = fetched(al, host, "all contigs")
    codes = w & 7
    assert (codes == 0).any() and (codes == 6).any() and (codes <= 6).all() and int((w != 0).sum()) > 1000
    # a sub-range, unaligned at both ends, as text and as words
    t, ww = al.proj_fetch(1237, 4099, words=True)
    assert t == hostlib.proj_text(host[1237:1237 + 4099]) and np.array_equal(ww, host[1237:1237 + 4099])
    assert al.proj_fetch(5, 0) == b""
    # every contig alone
    for _, seq in qs:
        al.proj_clear()
        one = np.zeros(G, np.uint32)
        paint(al, px, idx, seq, one)
        fetched(al, one, "one contig")
    assert al.proj_timing()[1] == 2 * len(qs)
    al.close()


@pytest.mark.parametrize("strand", ["+", "-"])
def test_projection_of_many_records(dense_snv_case, strand):
    """one block of about 150 000 records (three tiles of the second-level scan over the workgroups' sums), on either strand"""
    px, idx, qry = dense_snv_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx)
    al.proj_open()
    host = np.zeros(int(idx.G), np.uint32)
    r = paint(al, px, idx, q, host)
    fetched(al, host, strand)
    al.close()
    B = r["blocks"]
    assert ((B["bdir"] != 0) == (strand == "+")).all() and int(B["n_frag"].sum()) > 2 * TILE


@pytest.fixture(scope="module")
def identical_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("pid")
    ref = synth.random_genome(300_000, np.random.default_rng(29))
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), ref


@pytest.mark.parametrize("strand", ["+", "-"])
def test_projection_of_one_long_seed(identical_case, strand):
    """an identical 300 kb pair: nothing but seeds, every one across several column tiles, forward and reverse-complemented -- the text is the reference itself"""
    px, idx, ref = identical_case
    q = np.ascontiguousarray(ref if strand == "+" else synth.revcomp(ref))
    al = capi.Aligner(idx)
    al.proj_open()
    host = np.zeros(int(idx.G), np.uint32)
    r = paint(al, px, idx, q, host)
    text = al.proj_fetch()
    fetched(al, host, strand)
    al.close()
    # (the seed search ends a match at the end of its 10 000-base chunk: thirty seeds without a gap between them, each across five tiles of 2048 columns)
    seeds = r["frags"][r["frags"]["bseed"] == 1]
    assert int(seeds["rlen"].min()) >= 4 * 2048 and int(seeds["rlen"].sum()) == ref.size
    assert text == bytes(ref.tobytes()) and ((r["blocks"]["bdir"] != 0) == (strand == "+")).all()


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgp")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_projection_through_large_dp_gaps(large_gap_case, dp_safe):
    """gaps of more than 64 columns are walked by a whole wavefront from the op string of their (large) DP job; positions inside them carry base codes and code 6"""
    px, idx, qry = large_gap_case
    G = int(idx.G)
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    al.proj_open()
    host = np.zeros(G, np.uint32)
    r = paint(al, px, idx, qry, host)
    w = fetched(al, host, dp_safe)
    al.close()
    inside, F = set(), r["frags"]
    for i in np.flatnonzero((F["bseed"] == 0) & (F["aln_len"] > 64) & (F["rlen"] > 0) & (F["qlen"] > 0)):
        t = np.arange(int(F["rpos"][i]), int(F["rpos"][i]) + int(F["rlen"][i]))
        inside |= set((w[np.where(t < G, t, 2 * G - 1 - t)] & 7).tolist())
    assert 6 in inside and inside & {1, 2, 3, 4} and 0 not in inside, inside


def test_order_sharing_and_merging(golden_dir, cx_index, cx_queries):
    """three contexts share one accumulator through align_many with and without bundles, one contig split over the contexts, all contigs serially in reverse order on
    one context, a bundle painted contig by contig, and two accumulators painted with disjoint halves and merged: the arrays are identical"""
    px = os.path.join(golden_dir, "cx")
    G = int(cx_index.G)
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    g0 = capi.Aligner(cx_index); ctxs = [g0, g0.clone(), g0.clone()]
    g0.proj_open()
    for g in ctxs[1:]:
        g.proj_open(share=g0)
    host = np.zeros(G, np.uint32)
    for c in contigs[::-1]:
        paint(g0, px, cx_index, c, host)
    arrays = [fetched(g0, host, "serial, reverse order")]
    seen, lock = [], threading.Lock()

    def on_result(ci, res, var, cig):
        with lock:
            seen.append(ci)
        return 0

    for bundle in (True, False):
        g0.proj_clear(); seen.clear()
        capi.align_many(ctxs, contigs, on_result, bundle=bundle, proj=True)
        assert sorted(seen) == list(range(len(contigs)))
        arrays.append(fetched(ctxs[2], host, f"align_many, bundle={bundle}"))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished and painted by the first
    g0.proj_clear(); seen.clear()
    g0.set_option("split_min", 50000)
    capi.align_many(ctxs, contigs[:1], on_result, proj=True)
    capi.align_many(ctxs, contigs[1:], on_result, proj=True)
    assert len(seen) == len(contigs)
    arrays.append(fetched(g0, host, "split contig"))
    # a bundle, painted contig by contig out of order
    g0.proj_clear()
    g0.align_bundle(contigs)
    for k in (3, 0, 2, 1, 4)[:len(contigs)] + tuple(range(5, len(contigs))):
        g0.project(k)
    arrays.append(fetched(g0, host, "bundle"))
    with pytest.raises(capi.GsaError, match="error -1"):
        g0.project(len(contigs))
    # two accumulators of their own, disjoint halves of the contigs, merged through host words
    g1 = ctxs[1]
    g1.proj_close(); g1.proj_open()
    g0.proj_clear()
    for k, c in enumerate(contigs):
        g = g0 if k % 2 == 0 else g1
        g.align_contig(c); g.project()
    half = g0.proj_fetch(words=True)[1]
    assert (half != host).any()
    g0.proj_merge(g1.proj_fetch(words=True)[1])
    arrays.append(fetched(g0, host, "merged"))
    g0.proj_merge(host[1000:5000], p0=1000)      # (merging what is there already changes nothing)
    fetched(g0, host, "merged twice")
    assert len(arrays) == 6 and all(np.array_equal(a, arrays[0]) for a in arrays)
    for g in ctxs[1:]:
        g.close()
    g0.close()


@pytest.fixture(scope="module")
def tie_case(tmp_path_factory):
    """two query contigs that are the same 30 kb stretch of the reference with ten substitutions each, at different places: the two blocks score the same (the pair was
    chosen on the CPU with the oracle; the test asserts it)"""
    d = tmp_path_factory.mktemp("ptie")
    ref = synth.random_genome(60000, np.random.default_rng(41))
    n1, n2 = np.zeros(256, np.uint8), np.zeros(256, np.uint8)
    for a, b, c in zip(b"ACGT", b"CGTA", b"TACG"):
        n1[a] = b; n2[a] = c
    st = ref[10000:40000]
    A, B = st.copy(), st.copy()
    pa = np.arange(1000, 30000, 3000); pb = np.arange(2500, 30000, 3000)[:pa.size]
    A[pa] = n1[st[pa]]; B[pb] = n2[st[pb]]
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), ref, A, B, 10000 + pa, 10000 + pb


def test_tie_rule_does_not_depend_on_the_order(tie_case):
    px, idx, ref, A, B, pa, pb = tie_case
    G = int(idx.G)
    al = capi.Aligner(idx)
    al.proj_open()
    out = []
    for order in ((A, B), (B, A)):
        al.proj_clear()
        host = np.zeros(G, np.uint32)
        rs = [paint(al, px, idx, q, host) for q in order]
        assert all(r["blocks"].size == 1 and r["blocks"]["bdup"][0] == 0 for r in rs) and rs[0]["blocks"]["score"][0] == rs[1]["blocks"]["score"][0]
        out.append(fetched(al, host, "tie"))
    al.close()
    assert np.array_equal(out[0], out[1])
    w = out[0]
    code = lambda s: pm.NT4[s].astype(np.uint32) + 1
    assert np.array_equal(w[pa] & 7, np.maximum(code(A[pa - 10000]), code(ref[pa]))) and np.array_equal(w[pb] & 7, np.maximum(code(B[pb - 10000]), code(ref[pb])))
    assert (code(A[pa - 10000]) != code(ref[pa])).all() and (w[10000:40000] != 0).all() and not w[:10000].any() and not w[40000:].any()


def test_validity_and_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    G = int(cx_index.G)
    al = capi.Aligner(cx_index)
    lib = al.lib
    lib.gsa_proj_open.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    # without an accumulator
    r = al.align_contig(cur)
    for call in (al.project, al.proj_close, al.proj_clear, al.proj_fetch):
        with pytest.raises(capi.GsaError, match="error -4"):
            call()
    assert lib.gsa_proj_open(al.ctx, None, 2) == -1 and lib.gsa_proj_open(al.ctx, None, 0x80000001) == -1      # unknown flags
    cl = al.clone()
    with pytest.raises(capi.GsaError, match="error -1"):      # sharing with a context that holds no accumulator
        al.proj_open(share=cl)
    al.proj_open()
    with pytest.raises(capi.GsaError, match="error -4"):      # opening twice
        al.proj_open()
    with pytest.raises(capi.GsaError, match="error -4"):
        al.proj_open(share=al)
    # a clone starts without one
    cl.align_contig(cur)
    with pytest.raises(capi.GsaError, match="error -4"):
        cl.project()
    # before stage 8
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.project()
    assert al.proj_timing()[1] == 0      # (a refused call runs no pass)
    al.run_to(8)
    host = np.zeros(G, np.uint32)
    st = al.project()
    assert st == hostlib.project(px, cur, al.blocks(), host) and st[0] > 0
    a = fetched(al, host, "first")
    # a fetch range outside [0, G)
    for p0, n in ((-1, 10), (G - 5, 6), (0, G + 1), (G + 1, 0), (0, -1)):
        with pytest.raises(capi.GsaError, match="error -1"):
            al.proj_fetch(p0, n)
    assert al.proj_fetch(G, 0) == b"" and al.proj_fetch(G - 5, 5) == hostlib.proj_text(host[G - 5:])
    with pytest.raises(capi.GsaError, match="error -1"):
        al.proj_merge(host[:10], p0=G - 9)
    # the seven passes keep their answers apart, in several call orders (painting the same contig again changes no word)
    pos = np.arange(0, G, 3, dtype=np.int64)
    al.lift_set(pos); al.track_set(1000)
    ans = {"v": al.call_variants(), "c": al.block_cigars(), "s": al.block_cs(), "l": al.lift(), "t": al.track(), "g": al.block_segs()}
    calls = {"v": al.call_variants, "c": al.block_cigars, "s": al.block_cs, "l": al.lift, "t": al.track, "g": al.block_segs}

    def flat(x):
        return [np.asarray(y).tobytes() for y in (x if isinstance(x, tuple) else (x,))]

    for order in ("pvpcpsplptpgp", "gptlpscvp", "pcgpvtpsl"):
        for what in order:
            if what == "p":
                assert al.project() == st, order
                same(al.proj_fetch(words=True)[1], a, order)
            else:
                assert flat(calls[what]()) == flat(ans[what]), (order, what)
    # the next contig on its way into the other query slot: the pass still reads the current one
    cur_p, nxt_p = al.pinned_copy(cur), al.pinned_copy(nxt)
    al.proj_clear()
    al.prefetch_contig(nxt_p)
    al.align_contig(cur_p)
    al.project()
    fetched(al, host, "prefetch")
    al.align_contig(nxt_p)
    al.project()
    hostlib.project(px, nxt, al.blocks(), host)
    b = fetched(al, host, "second contig")
    # a contig without blocks leaves the words unchanged
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    assert al.project() == (0, 0)
    same(al.proj_fetch(words=True)[1], b, "no blocks")
    # after proj_close
    al.proj_close()
    with pytest.raises(capi.GsaError, match="error -4"):
        al.project()
    with pytest.raises(capi.GsaError, match="error -4"):
        al.proj_close()
    # the owner -- a clone -- is destroyed while a sharer lives: the sharer still paints and fetches
    cl.proj_open()
    al.proj_open(share=cl)
    cl.align_contig(cur); cl.project()
    cl.close()
    al.align_contig(nxt); al.project()
    fetched(al, host, "owner gone")
    al.close()


def test_want_bit(cx_index, cx_queries):
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries]
    g0 = capi.Aligner(cx_index); ctxs = [g0, g0.clone(), g0.clone()]
    g0.proj_open(); ctxs[1].proj_open(share=g0)
    ran = []
    with pytest.raises(capi.GsaError, match="-> -4"):      # one context of several without an accumulator: before any contig is aligned
        capi.align_many(ctxs, contigs, lambda *a: ran.append(a[0]) or 0, proj=True)
    assert not ran and not g0.proj_fetch(words=True)[1].any()
    lib = g0.lib
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    cb = capi.RESULT_EX_FN(lambda user, ci, res, ex: ran.append(ci) or 0)
    cs = (C.c_void_p * 1)(g0.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    assert lib.gsa_align_many_ex(cs, 1, qs, ql, 1, 0, capi.WANT_PROJ | 8, cb, None) == -1 and not ran      # bit 8 stays refused
    # no context with an accumulator at all: the bit is refused like an unknown one (what 128 gave before the pass existed), the callback never runs
    bare = (C.c_void_p * 1)(ctxs[2].ctx)
    assert lib.gsa_align_many_ex(bare, 1, qs, ql, 1, 0, capi.WANT_PROJ, cb, None) == -1 and not ran
    assert lib.gsa_align_many_ex(cs, 1, qs, ql, 1, 0, capi.WANT_PROJ, cb, None) == 0 and ran == [0]
    assert g0.proj_fetch(words=True)[1].any() and g0.proj_timing()[1] == 1
    for g in ctxs[1:]:
        g.close()
    g0.close()


def run_cli(cwd, *args, check=True):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=check, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


@pytest.mark.parametrize("unique", [False, True])
def test_cli_proj_golden(golden_dir, cx_index, tmp_path, unique):
    """-proj: out.proj.fa is the text the reference's own MAF implies (proj_from_maf), over all query contigs; the MAF and VCF are the golden bytes"""
    extra = ["-unique"] if unique else []
    tag = "cx_unique" if unique else "cx"
    run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-proj", *extra)
    got = open(tmp_path / "out.proj.fa", "rb").read()
    assert got == pj.proj_fasta(os.path.join(golden_dir, tag + ".maf"), cx_index.chr_names, cx_index.chr_len)
    assert got.count(b">") == len(cx_index.chr_names) and set(got) >= set(b"ACGTn-")
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, tag + ".maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, tag + ".vcf"), "rb").read()


def test_cli_proj_beside_every_other_switch(golden_dir, cx_index, tmp_path):
    """-fmt 3 -cs -gpuvar -lift -track 1000 -chain with and without -proj: the other files are the same bytes, the timing line gains proj_s"""
    pf = str(tmp_path / "pos.tsv")
    with open(pf, "w") as fh:
        for n, l in zip(cx_index.chr_names, cx_index.chr_len.tolist()):
            fh.write("".join(f"{n}\t{p}\n" for p in range(1, l + 1, 7)))
    common = ["-i", "cx", "-q", "cx.qry.fa", "-t", "1", "-fmt", "3", "-cs", "-gpuvar", "-lift", pf, "-track", "1000", "-chain", "-timing"]
    err = run_cli(golden_dir, *common, "-o", str(tmp_path / "with"), "-proj").stderr
    run_cli(golden_dir, *common, "-o", str(tmp_path / "plain"))
    for ext in ("paf", "vcf", "lift.tsv", "track.tsv", "chain"):
        a, b = open(tmp_path / f"with.{ext}", "rb").read(), open(tmp_path / f"plain.{ext}", "rb").read()
        assert a == b and len(a) > 0, ext
    assert not os.path.exists(tmp_path / "plain.proj.fa")
    assert open(tmp_path / "with.proj.fa", "rb").read() == pj.proj_fasta(os.path.join(golden_dir, "cx.maf"), cx_index.chr_names, cx_index.chr_len)
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"proj_s": ' in timing[0] and timing[0].rstrip().endswith(b"}") and b'"cs_s": ' in timing[0]
