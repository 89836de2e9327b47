"""gsa_ref_track on the GPU box: the per-window track of a finished alignment over the reference sequences, computed on the device -- record walk, window split,
wavefront reduction, integer atomics into the dense array, ownership scan -- must equal, window for window and field for field, what the host walk over the gapped
strings gives (gsah_c_track, pinned to the reference's MAF files in test_track_host.py): through the single-contig call, bundles, gsa_align_many_ex and the CLI's -track."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import track_from_maf as tm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_result_scan import dense_snv_pair
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.dtype == capi.TRACK_WIN_DT and b.dtype == capi.TRACK_WIN_DT and a.size == b.size and a.tobytes() == b.tobytes()


def check_track(al, px, seq, r, W, k=0):
    """the device's track of the result the context holds at window W against the host walk over `r`, field for field"""
    al.track_set(W)
    got = al.track(k)
    want = hostlib.track(px, seq, r, W)
    assert got.size == want.size, (W, got.size, want.size)
    for f in capi.TRACK_WIN_DT.names:
        assert np.array_equal(got[f], want[f]), (W, f, np.flatnonzero(got[f] != want[f])[:5], got[got[f] != want[f]][:3], want[got[f] != want[f]][:3])
    return got


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_track_matches_the_host_walk(golden_dir, name, params, wide):
    """every contig at W in {1, 100, 1000, 2^30}; at W = 1 a contig of cx covers more than 65 536 windows (the reference has more than 3 x 65 536), i.e. more than 256
    workgroups of EMIT, so the second tile of the scan over the workgroups' sums carries"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    al = capi.Aligner(idx, wide=wide, **params)
    n1, seen = 0, dict(ins=0, dele=0, x=0, deep=0, rev=0)
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        r = al.align_contig(seq)
        for W in (1, 100, 1000, 1 << 30):
            T = check_track(al, px, seq, r, W)
            if W == 1:
                n1 = max(n1, T.size)
            seen["ins"] += int((T["n_ins"] > 0).sum()); seen["dele"] += int((T["n_del"] > 0).sum()); seen["x"] += int((T["n_x"] > 0).sum())
            seen["deep"] += int((T["n_eq"].astype(np.int64) + T["n_x"] + T["n_del"] > T["n_cov"]).sum())
        B = r["blocks"]
        seen["rev"] += int(((B["bdir"] == 0) & (B["bdup"] == 0)).sum())
    al.close()
    assert seen["ins"] > 0 and seen["dele"] > 0 and seen["x"] > 0, seen
    if name == "cx":
        assert int(idx.G) > 3 * 65536 and n1 > 65536 and seen["deep"] > 0 and seen["rev"] > 0, (n1, seen)


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgt")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_track_through_large_dp_gaps(large_gap_case, dp_safe):
    """Gaps of more than 64 columns are walked by a whole wavefront, and they are large DP jobs: their gapped strings never exist in the device's string pools,
    the columns come from the job's op string.  dp_safe = 1: one striped job per launch.  Windows of one base that only such a gap covers hold inserted, deleted
    and mismatching bases."""
    px, idx, qry = large_gap_case
    G = int(idx.G)
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    r = al.align_contig(qry)
    T = None
    for W in (1000, 100, 1):
        T = check_track(al, px, qry, r, W)
    al.close()
    assert (T["chr"] == 0).all()
    B, F = r["blocks"], r["frags"]
    inside = np.zeros(G, bool)
    for i in np.flatnonzero((F["bseed"] == 0) & (F["aln_len"] > 64) & (F["rlen"] > 0) & (F["qlen"] > 0)):
        bi = int(np.flatnonzero((B["frag_off"] <= i) & (i < B["frag_off"] + B["n_frag"]))[0])
        if B["bdup"][bi]:
            continue
        t = np.arange(int(F["rpos"][i]) + 1, int(F["rpos"][i]) + int(F["rlen"][i]))      # (not the gap's first base: an insertion in front of it belongs to the seed)
        inside[np.where(t < G, t, 2 * G - 1 - t)] = True
    t = T[inside[T["start"]] & (T["n_eq"].astype(np.int64) + T["n_x"] + T["n_del"] == 1)]
    assert (t["n_ins"] > 0).any() and (t["n_del"] > 0).any() and (t["n_x"] > 0).any(), (t.size, int(inside.sum()))


@pytest.fixture(scope="module")
def dense_snv_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("tscan")
    ref, qry = dense_snv_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("strand", ["+", "-"])
def test_track_of_many_records(dense_snv_case, strand):
    """149 997 records in one block, either strand: at W = 1 every seed goes through the wavefront queue and the windows fill more than twenty tiles of the scan"""
    px, idx, qry = dense_snv_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx)
    r = al.align_contig(q)
    B = r["blocks"]
    assert ((B["bdir"] != 0) == (strand == "+")).all() and int(B["n_frag"][B["bdup"] == 0].sum()) > 100000
    T1 = check_track(al, px, q, r, 1)
    Tk = check_track(al, px, q, r, 1000)
    al.close()
    assert T1.size > 20 * 65536 and int(T1["n_x"].sum()) == int(Tk["n_x"].sum()) > 70000


def test_track_of_a_bundle(golden_dir, cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer, asked for out of order and repeatedly"""
    px = os.path.join(golden_dir, "cx")
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    al = capi.Aligner(cx_index)
    single = [check_track(al, px, c, al.align_contig(c), 100) for c in contigs]
    assert single[2].size == 0 and all(single[k].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.track(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.track(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.track(-1)
    al.close()


def test_track_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    al = capi.Aligner(cx_index)
    al.track_set(1000)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.track()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.track()
    al.run_to(8)
    a = al.track()
    assert a.size > 0 and same(a, hostlib.track(px, cur, al.blocks(), 1000)) and al.track_timing()[1] == 1      # (a refused call runs no pass)
    # without a window: GSA_ERR_STATE; a clone starts without one; a negative window is refused and changes nothing
    cl = al.clone()
    cl.align_contig(cur)
    with pytest.raises(capi.GsaError, match="error -4"):
        cl.track()
    cl.close()
    al.track_set(0)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.track()
    al.track_set(1000)
    with pytest.raises(capi.GsaError, match="error -1"):
        al.track_set(-5)
    assert same(al.track(), a) and al.track_timing()[1] == 2
    # another window on the same result, and back
    b = check_track(al, px, cur, al.blocks(), 37)
    assert b.size > a.size
    al.track_set(1000)
    assert same(al.track(), a)
    # the five passes keep their answers apart, in any order
    al.lift_set(np.arange(0, int(cx_index.G), 3, dtype=np.int64))
    cg = al.block_cigars(); v = al.call_variants(); s = al.block_cs(); lf = al.lift()
    assert cg[1].size > 0 and v[0].size > 0 and s[1].size > 0 and lf.size > 0
    for order in ("tlscv", "vtlsc", "cstlv", "vcslt"):
        for what in order:
            if what == "t":
                assert same(al.track(), a), order
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
    assert same(al.track(), a)
    al.align_contig(nxt_p)
    assert same(al.track(), hostlib.track(px, nxt, al.blocks(), 1000))
    # no block at all: n_win = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    assert al.track().size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants,cigars,lift", [(1, True, False, False, False), (1, False, True, True, True), (3, True, True, False, True), (3, False, False, True, False)])
def test_align_many_with_track(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants, cigars, lift):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    pos = np.arange(0, int(cx_index.G), 2, dtype=np.int64)
    W = 500
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    want, want_cig, want_var, want_lift = [], [], [], []
    for c in contigs:
        r = g0.align_contig(c)
        want.append(check_track(g0, px, c, r, W)); want_cig.append(hostlib.cigars(None, c, r)); want_var.append(hostlib.variants(px, c, r)); want_lift.append(hostlib.lift(px, c, r, pos))
    assert sum(t.size for t in want) > 100
    if lift:
        for g in ctxs:
            g.lift_set(pos)
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, *rest):
        t = capi.tracks_array(rest[-1])
        h = capi.lifts_array(rest[0]) if lift else None
        c = capi.cigars_arrays(cig) if cig is not None else None
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (t, c, v, h, len(rest))
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]), ci
            assert got[ci][4] == (2 if lift else 1)
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

    if n_ctx > 1:
        # one context without a window: GSA_ERR_STATE before any contig is aligned
        for g in ctxs[1:-1]:
            g.track_set(W)
        with pytest.raises(capi.GsaError, match="-> -4"):
            capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, track=True)
        assert not got
        ctxs[-1].track_set(W)
    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, track=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cigars=cigars, lift=lift, track=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_extras_track_needs_the_want_bit(cx_index, cx_queries):
    """behind a gsa_extras of a call without GSA_WANT_TRACK there is no track (GSA_ERR_STATE); bit 8 stays refused"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    al.track_set(1000)
    lib = al.lib
    lib.gsa_extras_track.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.Tracks)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        t = capi.Tracks()
        rcs.append((lib.gsa_extras_track(ex, C.byref(t)), int(t.n_win), bool(ex.contents.cig)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_TRACK, 0), (capi.WANT_TRACK | capi.WANT_CIGARS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want and (rcs[0][1] > 0) == (rc_want == 0) and rcs[0][2] == bool(want & capi.WANT_CIGARS), (want, rcs)
    rcs.clear()
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, capi.WANT_TRACK | 8, capi.RESULT_EX_FN(cb), None) == -1 and not rcs
    al.close()


def run_cli(cwd, *args, check=True):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=check, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


@pytest.mark.parametrize("W", [1000, 1])
def test_cli_track_golden(golden_dir, cx_index, tmp_path, W):
    """-track W: out.track.tsv is the text the reference's own MAF implies (track_from_maf); the other files of the run are the bytes they are without the switch"""
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-track", str(W), "-timing").stderr
    assert open(tmp_path / "out.track.tsv").read() == tm.track_tsv(os.path.join(golden_dir, "cx.maf"), cx_index.chr_names, cx_index.chr_len, W)
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"track_s": ' in timing[0]


def test_cli_track_beside_paf_cs_variants_and_lift(golden_dir, cx_index, tmp_path):
    """-track with -fmt 3 -cs -gpuvar -lift: the PAF, lift and VCF bytes are what they are without the switch"""
    import cs_from_maf as cm
    import lift_from_maf as lm
    from test_gpu_lift import position_file
    pf = str(tmp_path / "pos.tsv")
    position_file(pf, cx_index)
    maf = os.path.join(golden_dir, "cx.maf")
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-track", "1000", "-fmt", "3", "-cs", "-gpuvar", "-lift", pf, "-timing").stderr
    assert open(tmp_path / "out.track.tsv").read() == tm.track_tsv(maf, cx_index.chr_names, cx_index.chr_len, 1000)
    assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(maf)
    assert open(tmp_path / "out.lift.tsv").read() == lm.lift_tsv(maf, cx_index.chr_names, cx_index.chr_len)
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"track_s": ' in timing[0] and b'"lift_s": ' in timing[0]


@pytest.mark.parametrize("arg", ["0", "x", "-3", "12k"])
def test_cli_track_refuses_what_is_no_window(golden_dir, tmp_path, arg):
    r = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "o"), "-t", "1", "-track", arg, check=False)
    assert r.returncode == 1 and sum(1 for ln in r.stderr.split(b"\n") if b"-track" in ln) == 1
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o.")]
