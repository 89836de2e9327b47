"""gsa_query_track on the GPU box: the per-window track of a finished alignment over the QUERY contig, computed on the device -- record walk, window split, the trim
carried over from the reference side, wavefront reduction, integer atomics into the dense array, ownership scan, the two interval lists -- must equal, window for
window and field for field, what the host walk over the gapped strings gives (gsah_c_qtrack, pinned to the reference's MAF files in test_qtrack_host.py): through the
single-contig call, bundles, gsa_align_many_ex and the CLI's -qtrack."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import qtrack_from_maf as qm
import regions_from_maf as rm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_result_scan import dense_snv_pair
from test_gpu_variants import large_gap_pair
from test_qtrack_host import GOLDEN_MULTI, junction_pair, overruns, twice_pair

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.dtype == capi.QTRACK_WIN_DT and b.dtype == capi.QTRACK_WIN_DT and a.size == b.size and a.tobytes() == b.tobytes()


def check_qtrack(al, px, seq, r, W, k=0):
    """the device's query track of the result the context holds at window W against the host walk over `r`, field for field"""
    al.qtrack_set(W)
    got = al.qtrack(k)
    want = hostlib.qtrack(px, seq, r, W)
    assert got.size == want.size, (W, got.size, want.size)
    for f in capi.QTRACK_WIN_DT.names:
        assert np.array_equal(got[f], want[f]), (W, f, np.flatnonzero(got[f] != want[f])[:5], got[got[f] != want[f]][:3], want[got[f] != want[f]][:3])
    return got


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_qtrack_matches_the_host_walk(golden_dir, name, params, wide):
    """every contig at W in {1, 100, 1000, 2^30}; at W = 1 a 120 kb contig of cx covers more than 65 536 windows, i.e. more than 256 workgroups of EMIT, so the second
    tile of the scan over the workgroups' sums carries"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    al = capi.Aligner(idx, wide=wide, **params)
    n1, seen = 0, dict(ins=0, dele=0, x=0, multi=0, rev=0)
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        r = al.align_contig(seq)
        for W in (1, 100, 1000, 1 << 30):
            T = check_qtrack(al, px, seq, r, W)
            if W == 1:
                n1 = max(n1, T.size)
            seen["ins"] += int((T["n_ins"] > 0).sum()); seen["dele"] += int((T["n_del"] > 0).sum()); seen["x"] += int((T["n_x"] > 0).sum())
            seen["multi"] += int((T["n_multi"] > 0).sum())
        B = r["blocks"]
        seen["rev"] += int(((B["bdir"] == 0) & (B["bdup"] == 0)).sum())
    al.close()
    assert seen["ins"] > 0 and seen["dele"] > 0 and seen["x"] > 0, seen
    # (which golden cases put a base under two counted blocks is settled on the CPU: test_qtrack_host.GOLDEN_MULTI -- none does, test_qtrack_of_a_segment_present_twice below does)
    assert (seen["multi"] > 0) == (("cx_sen" if params else name) in GOLDEN_MULTI), seen
    if name == "cx":
        assert n1 > 65536 and seen["rev"] > 0, (n1, seen)


def test_qtrack_of_a_segment_present_twice(tmp_path):
    """twice_pair(): a query segment that lies twice in the reference -- two counted blocks overlap in the query, n_multi > 0, at windows that cut the overlap"""
    ref, qry = twice_pair()
    fa, px = str(tmp_path / "r.fa"), str(tmp_path / "r")
    synth.write_fasta(fa, [("chr1", ref)]); hostlib.build_index(fa, px)
    al = capi.Aligner(indexio.load_index(px))
    r = al.align_contig(qry)
    assert int((r["blocks"]["bdup"] == 0).sum()) >= 2
    for W in (1, 37, 1000, 1 << 30):
        T = check_qtrack(al, px, qry, r, W)
        assert 3500 <= int(T["n_multi"].sum()) <= 4100, (W, int(T["n_multi"].sum()))
        assert np.array_equal(T["n_eq"].astype(np.int64) + T["n_x"] + T["n_ins"] == T["n_cov"], T["n_multi"] == 0)
    al.close()


@pytest.mark.parametrize("indel,rc", [(False, False), (False, True), (True, False)])
def test_qtrack_carries_the_trim_over_on_the_device(tmp_path, indel, rc):
    """junction_pair(): the aligner's own block runs past the end of its chromosome copy inside its last seed, on either strand, alone and behind a gap record.  The host
    finds the record that holds the cut, q1 is arithmetic, COUNT splits only the kept bases of that seed (by its lane at W = 2^30, by a wavefront at W = 1 and 100), and
    the query bases behind the cut stay uncovered.  (No aligned block is cut inside a GAP record -- blocks end in seeds, and only a seed can run across a sequence end --
    so k_qtk_cut and the walkers' cut exits are not reached from here.)"""
    refs, qry = junction_pair(indel=indel)
    if rc:
        qry = np.ascontiguousarray(synth.revcomp(qry))
    fa, px = str(tmp_path / "r.fa"), str(tmp_path / "r")
    synth.write_fasta(fa, refs); hostlib.build_index(fa, px)
    idx = indexio.load_index(px)
    al = capi.Aligner(idx)
    r = al.align_contig(qry)
    B, F = r["blocks"], r["frags"]
    assert B.size == 1 and int(B["bdup"][0]) == 0 and int(B["bdir"][0]) == (0 if rc else 1) and (int(B["n_frag"][0]) > 1) == indel
    assert overruns(B, F, idx)[0] >= 2990
    for W in (1, 100, 1 << 30):
        T = check_qtrack(al, px, qry, r, W)
        assert int(T["n_cov"].sum()) == (2997 if indel else 3000) and int(T["n_del"].sum()) == (3 if indel else 0)
        assert int(T["start"][-1]) + int(T["len"][-1]) <= (3000 if W < 1000 else qry.size)
        # the reference side trims the same columns
        al.track_set(W)
        R = al.track()
        for f in ("n_eq", "n_x", "n_ins", "n_del"):
            assert int(T[f].sum()) == int(R[f].sum()), (W, f)
    al.close()


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgq")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_qtrack_through_large_dp_gaps(large_gap_case, dp_safe):
    """Gaps of more than 64 columns are walked by a whole wavefront, and they are large DP jobs: their gapped strings never exist in the device's string pools, the
    columns come from the job's op string.  dp_safe = 1: one striped job per launch.  Windows of one base inside such a gap hold inserted and mismatching bases and
    deletions charged to the base in front of them."""
    px, idx, qry = large_gap_case
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    r = al.align_contig(qry)
    T = None
    for W in (1000, 100, 1):
        T = check_qtrack(al, px, qry, r, W)
    al.close()
    B, F = r["blocks"], r["frags"]
    inside = np.zeros(qry.size, bool)
    n_big = 0
    for i in np.flatnonzero((F["bseed"] == 0) & (F["aln_len"] > 64) & (F["rlen"] > 0) & (F["qlen"] > 0)):
        bi = int(np.flatnonzero((B["frag_off"] <= i) & (i < B["frag_off"] + B["n_frag"]))[0])
        if B["bdup"][bi]:
            continue
        inside[int(F["qpos"][i]):int(F["qpos"][i]) + int(F["qlen"][i])] = True
        n_big += 1
    t = T[inside[T["start"]]]
    assert n_big > 0 and (t["n_ins"] > 0).any() and (t["n_del"] > 0).any() and (t["n_x"] > 0).any(), (n_big, t.size, int(inside.sum()))


@pytest.fixture(scope="module")
def dense_snv_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("qscan")
    ref, qry = dense_snv_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("strand", ["+", "-"])
def test_qtrack_of_many_records(dense_snv_case, strand):
    """more than 100 000 records in one block, either strand: at W = 1 every seed goes through the wavefront queue and the windows fill more than twenty tiles of the scan"""
    px, idx, qry = dense_snv_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx)
    r = al.align_contig(q)
    B = r["blocks"]
    assert ((B["bdir"] != 0) == (strand == "+")).all() and int(B["n_frag"][B["bdup"] == 0].sum()) > 100000
    T1 = check_qtrack(al, px, q, r, 1)
    Tk = check_qtrack(al, px, q, r, 1000)
    al.close()
    assert T1.size > 20 * 65536 and int(T1["n_x"].sum()) == int(Tk["n_x"].sum()) > 70000


def test_qtrack_of_a_bundle(golden_dir, cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer (positions relative to contig k), asked for out of order and repeatedly"""
    px = os.path.join(golden_dir, "cx")
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [check_qtrack(al, px, c, al.align_contig(c), 100) for c in contigs]
    assert single[2].size == 0 and all(single[k].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.qtrack(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.qtrack(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.qtrack(-1)
    al.close()


def test_qtrack_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    G = int(cx_index.G)
    al = capi.Aligner(cx_index)
    al.qtrack_set(1000)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.qtrack()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.qtrack()
    al.run_to(8)
    a = al.qtrack()
    assert a.size > 0 and same(a, hostlib.qtrack(px, cur, al.blocks(), 1000)) and al.qtrack_timing()[1] == 1      # (a refused call runs no pass)
    # without a window: GSA_ERR_STATE; a clone starts without one; a negative window is refused and changes nothing
    cl = al.clone()
    cl.align_contig(cur)
    with pytest.raises(capi.GsaError, match="error -4"):
        cl.qtrack()
    cl.close()
    al.qtrack_set(0)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.qtrack()
    al.qtrack_set(1000)
    with pytest.raises(capi.GsaError, match="error -1"):
        al.qtrack_set(-5)
    assert same(al.qtrack(), a) and al.qtrack_timing()[1] == 2
    # the reference-side window is another thing: without it gsa_ref_track is refused and gsa_query_track is not; both held together, with different lengths, both right
    with pytest.raises(capi.GsaError, match="error -4"):
        al.track()
    al.track_set(300)
    tk = al.track()
    assert tk.tobytes() == hostlib.track(px, cur, al.blocks(), 300).tobytes() and same(al.qtrack(), a)
    al.qtrack_set(0)
    assert al.track().tobytes() == tk.tobytes()
    # another window on the same result, and back
    b = check_qtrack(al, px, cur, al.blocks(), 37)
    assert b.size > a.size
    al.qtrack_set(1000)
    assert same(al.qtrack(), a)
    # the nine passes keep their answers apart, in several orders
    beg, end = rm.stride_regions(cx_index.chr_len, lengths=(1, 65, 1000), stride=11)
    al.regions_set(beg, end); al.lift_set(np.arange(0, G, 5, dtype=np.int64)); al.proj_open()
    cg = al.block_cigars(); v = al.call_variants(); s = al.block_cs(); lf = al.lift(); sg = al.block_segs(); rg = al.lift_regions(); pj = al.project(); word = al.proj_fetch(words=True)[1]
    assert cg[1].size > 0 and v[0].size > 0 and s[1].size > 0 and lf.size > 0 and tk.size > 0 and sg[1].size > 0 and rg.size > 0 and pj[0] > 0
    for order in ("qrlcvstgp", "pgtsvclrq", "cqsqlqtqr", "vqpqgqrqt"):
        for what in order:
            if what == "q":
                assert same(al.qtrack(), a), order
            elif what == "r":
                assert al.lift_regions().tobytes() == rg.tobytes(), order
            elif what == "l":
                assert al.lift().tobytes() == lf.tobytes(), order
            elif what == "s":
                g = al.block_cs()
                assert np.array_equal(g[0], s[0]) and np.array_equal(g[1], s[1]), order
            elif what == "c":
                g = al.block_cigars()
                assert np.array_equal(g[0], cg[0]) and np.array_equal(g[1], cg[1]), order
            elif what == "t":
                assert al.track().tobytes() == tk.tobytes(), order
            elif what == "g":
                g = al.block_segs()
                assert np.array_equal(g[0], sg[0]) and np.array_equal(g[1], sg[1]), order
            elif what == "p":
                assert al.project() == pj and np.array_equal(al.proj_fetch(words=True)[1], word), order
            else:
                w = al.call_variants()
                assert np.array_equal(w[0], v[0]) and tuple(w[1]) == tuple(v[1]), order
    al.proj_close()
    # the next contig on its way into the other query slot: the pass still reads the current one
    cur_p, nxt_p = al.pinned_copy(cur), al.pinned_copy(nxt)
    al.prefetch_contig(nxt_p)
    al.align_contig(cur_p)
    assert same(al.qtrack(), a)
    al.align_contig(nxt_p)
    assert same(al.qtrack(), hostlib.qtrack(px, nxt, al.blocks(), 1000))
    # no block at all: n_win = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    assert al.qtrack().size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants,cigars,lift,track", [(1, True, False, False, False, False), (1, False, True, True, True, True), (3, True, True, False, True, False), (3, False, False, True, False, True)])
def test_align_many_with_qtrack(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants, cigars, lift, track):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    pos = np.arange(0, int(cx_index.G), 2, dtype=np.int64)
    W, WR = 500, 700
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want, want_cig, want_var, want_lift, want_trk = [], [], [], [], []
    for c in contigs:
        r = g0.align_contig(c)
        want.append(check_qtrack(g0, px, c, r, W)); want_cig.append(hostlib.cigars(None, c, r)); want_var.append(hostlib.variants(px, c, r)); want_lift.append(hostlib.lift(px, c, r, pos))
        want_trk.append(hostlib.track(px, c, r, WR))
    assert sum(t.size for t in want) > 100
    for g in ctxs:
        if lift:
            g.lift_set(pos)
        if track:
            g.track_set(WR)
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, *rest):
        t = capi.qtracks_array(rest[-1])                       # (the new extra stands behind the existing ones)
        h = capi.lifts_array(rest[0]) if lift else None
        k = capi.tracks_array(rest[1 if lift else 0]) if track else None
        c = capi.cigars_arrays(cig) if cig is not None else None
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (t, c, v, h, len(rest), k)
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]), ci
            assert got[ci][4] == 1 + (1 if lift else 0) + (1 if track else 0)
            if cigars:
                assert np.array_equal(got[ci][1][0], want_cig[ci][0]) and np.array_equal(got[ci][1][1], want_cig[ci][1]), ci
            else:
                assert got[ci][1] is None
            if variants:
                assert np.array_equal(got[ci][2][0], want_var[ci][0]) and tuple(got[ci][2][1]) == tuple(want_var[ci][1]), ci
            else:
                assert got[ci][2] is None
            if lift:
                assert got[ci][3].tobytes() == want_lift[ci].tobytes(), ci
            if track:
                assert got[ci][5].tobytes() == want_trk[ci].tobytes(), ci

    if n_ctx > 1:
        # one context without a window: GSA_ERR_STATE before any contig is aligned
        for g in ctxs[1:-1]:
            g.qtrack_set(W)
        with pytest.raises(capi.GsaError, match="-> -4"):
            capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, track=track, qtrack=True)
        assert not got
        ctxs[-1].qtrack_set(W)
    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, track=track, qtrack=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cigars=cigars, lift=lift, track=track, qtrack=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_extras_qtrack_needs_the_want_bit(cx_index, cx_queries):
    """behind a gsa_extras of a call without GSA_WANT_QTRACK there is no query track (GSA_ERR_STATE); bit 8 stays refused"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    al.qtrack_set(1000)
    lib = al.lib
    lib.gsa_extras_qtrack.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.QTracks)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        t = capi.QTracks()
        rcs.append((lib.gsa_extras_qtrack(ex, C.byref(t)), int(t.n_win), bool(ex.contents.cig)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_QTRACK, 0), (capi.WANT_QTRACK | capi.WANT_CIGARS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want and (rcs[0][1] > 0) == (rc_want == 0) and rcs[0][2] == bool(want & capi.WANT_CIGARS), (want, rcs)
    rcs.clear()
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, capi.WANT_QTRACK | 8, capi.RESULT_EX_FN(cb), None) == -1 and not rcs
    al.close()


def run_cli(cwd, *args, check=True):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=check, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


@pytest.mark.parametrize("W", [1000, 1])
def test_cli_qtrack_golden(golden_dir, tmp_path, W):
    """-qtrack W: out.qtrack.tsv is the text the reference's own MAF implies (qtrack_from_maf); the other files of the run are the bytes they are without the switch"""
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-qtrack", str(W), "-timing").stderr
    assert open(tmp_path / "out.qtrack.tsv").read() == qm.qtrack_tsv(os.path.join(golden_dir, "cx.maf"), W)
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"qtrack_s": ' in timing[0]


def test_cli_qtrack_beside_paf_cs_variants_lift_and_track(golden_dir, cx_index, tmp_path):
    """-qtrack with -fmt 3 -cs -gpuvar -lift -track: the PAF, lift, track and VCF bytes are what they are without the switch"""
    import cs_from_maf as cm
    import lift_from_maf as lm
    import track_from_maf as tm
    from test_gpu_lift import position_file
    pf = str(tmp_path / "pos.tsv")
    position_file(pf, cx_index)
    maf = os.path.join(golden_dir, "cx.maf")
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-qtrack", "1000", "-fmt", "3", "-cs", "-gpuvar", "-lift", pf, "-track", "700", "-timing").stderr
    assert open(tmp_path / "out.qtrack.tsv").read() == qm.qtrack_tsv(maf, 1000)
    assert open(tmp_path / "out.track.tsv").read() == tm.track_tsv(maf, cx_index.chr_names, cx_index.chr_len, 700)
    assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(maf)
    assert open(tmp_path / "out.lift.tsv").read() == lm.lift_tsv(maf, cx_index.chr_names, cx_index.chr_len)
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"qtrack_s": ' in timing[0] and b'"track_s": ' in timing[0] and b'"lift_s": ' in timing[0]


@pytest.mark.parametrize("arg", ["0", "x", "-3", "12k"])
def test_cli_qtrack_refuses_what_is_no_window(golden_dir, tmp_path, arg):
    r = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "o"), "-t", "1", "-qtrack", arg, check=False)
    assert r.returncode == 1 and sum(1 for ln in r.stderr.split(b"\n") if b"-qtrack" in ln) == 1
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]
