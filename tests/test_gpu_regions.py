"""gsa_lift_regions on the GPU box: reference intervals carried through a finished alignment on the device -- per-record class prefix, block search, two record
searches and two gap walks per region -- must equal, hit for hit and field for field, what the host walk over the gapped strings gives (gsah_c_lift_regions, pinned
to the reference's MAF files in test_regions_host.py): through the single-contig call, bundles, gsa_align_many_ex and the CLI's -liftbed."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import regions_from_maf as rm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_variants import large_gap_pair
from test_regions_host import KINDS, assert_kinds, kinds_of, region_set

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.dtype == capi.REGION_HIT_DT and b.dtype == capi.REGION_HIT_DT and a.size == b.size and a.tobytes() == b.tobytes()


def parity(got, want):
    assert got.dtype == capi.REGION_HIT_DT and got.size == want.size, (got.size, want.size)
    for f in capi.REGION_HIT_DT.names:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:5], got[got[f] != want[f]][:3], want[got[f] != want[f]][:3])


def aligned_regions(al, px, seq, beg, end):
    """align one contig and lift the context's regions (beg, end: the same lists, for the host): (device hits, result dict), parity asserted"""
    r = al.align_contig(seq)
    got = al.lift_regions()
    parity(got, hostlib.lift_regions(px, seq, r, beg, end))
    return got, r


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_regions_match_the_host_walk(golden_dir, name, params, wide):
    """the region sets of test_regions_host.py (cx: well above 3 x 65 536 of them, so the second tile of the scan over the workgroups' sums carries), then the same
    regions shuffled, and a list in which regions repeat: the answers are per idx"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    G = int(idx.G)
    rng = np.random.default_rng(17)
    al = capi.Aligner(idx, wide=wide, **params)
    seen = {k: 0 for k in KINDS}
    for ci, (_, seq) in enumerate(synth.read_fasta(px + ".qry.fa")):
        r = al.align_contig(seq)
        d = capi.result_as_dump(r, True)
        beg, end = region_set(idx, d)
        if name == "cx":
            assert beg.size > 3 * 65536
        al.regions_set(beg, end)
        H = al.lift_regions()
        W = hostlib.lift_regions(px, seq, r, beg, end)
        parity(H, W)
        assert (np.diff(H["idx"]) > 0).all()
        want = by_overlap(d, G, H, beg, end)      # (which choices went against the score: from the result's own blocks)
        for k, v in kinds_of(d, G, H, beg, end, want).items():
            seen[k] += v
        if ci == 0:
            # the same contig's result, other region lists: each hit is the hit of its region
            n = beg.size
            by_reg = np.full(n, -1, np.int64); by_reg[H["idx"]] = np.arange(H.size)
            perm = rng.permutation(n)
            rep = rng.integers(0, n, 5000); rep[1::2] = rep[0::2]
            for lst in (perm, rep):
                al.regions_set(beg[lst], end[lst])
                P = al.lift_regions()
                assert same(P, hostlib.lift_regions(px, seq, r, beg[lst], end[lst]))
                assert (np.diff(P["idx"]) > 0).all() and np.array_equal(P["idx"], np.flatnonzero(by_reg[lst] >= 0))
                src = H[by_reg[lst[P["idx"]]]]
                for f in capi.REGION_HIT_DT.names[1:]:
                    assert np.array_equal(P[f], src[f]), f
            assert al.region_timing()[1] == 3
    al.close()
    assert_kinds(name, seen)


def by_overlap(d, G, H, beg, end):
    """per hit: some other block that is no duplicate overlaps the region less than the chosen one and scores higher -- the choice went against the score"""
    f_at = np.concatenate([[0], np.cumsum(d["b_nfrag"])]).astype(np.int64)
    full = np.zeros(H.size, bool)
    sub = np.flatnonzero(H["n_cover"] > 1)      # (a lone block has no rival)
    if sub.size == 0:
        return full
    H = H[sub]
    out = np.zeros(H.size, bool)
    b = beg[H["idx"]]; e = end[H["idx"]]
    span = []
    for bi in range(d["b_score"].size):
        t0 = int(d["f_rpos"][f_at[bi]]); t1 = int(d["f_rpos"][f_at[bi + 1] - 1]) + int(d["f_rlen"][f_at[bi + 1] - 1])
        span.append((t0, t1) if d["b_bdir"][bi] else (2 * G - t1, 2 * G - t0))      # (the golden results need no trim)
    ov = np.stack([np.minimum(e, s1) - np.maximum(b, s0) for s0, s1 in span])
    mine = ov[H["block"], np.arange(H.size)]
    for bi in range(d["b_score"].size):
        out |= (H["block"] != bi) & (d["b_bdup"][H["block"]] == 0) & (d["b_bdup"][bi] == 0) & (ov[bi] > 0) & (ov[bi] < mine) & (d["b_score"][bi] > d["b_score"][H["block"]])
    full[sub] = out
    return full


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgr")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_regions_through_large_dp_gaps(large_gap_case, dp_safe):
    """Gaps of more than 64 columns are walked by a whole wavefront in CLASS and in EMIT, and they are large DP jobs: their gapped strings never exist in the device's
    string pools, the columns come from the job's op string.  dp_safe = 1: one striped job per launch.  Regions start and end at every column of every such gap."""
    px, idx, qry = large_gap_case
    G = int(idx.G)
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    r = al.align_contig(qry)
    d = capi.result_as_dump(r, True)
    big = np.flatnonzero((d["f_bseed"] == 0) & (d["f_alnlen"] > 64) & (d["f_rlen"] > 0) & (d["f_qlen"] > 0))
    assert big.size >= 10 and (d["b_bdir"] != 0).all()
    r0 = d["f_rpos"][big].astype(np.int64); r1 = r0 + d["f_rlen"][big]
    b, e = [], []
    for k in range(big.size):
        a = np.arange(r0[k], r1[k], dtype=np.int64)
        b += [a, np.full(a.size, r0[k] - 5)]; e += [np.full(a.size, r1[k] + 5), a + 1]      # a start at every column, an end at every column
        ia, ib = np.triu_indices(a.size)
        b.append(a[ia]); e.append(a[ib] + 1)                                                # both ends inside the gap
        if k + 1 < big.size:                                                                # the two ends in two such gaps: the prefix covers what lies between
            m = int(min(a.size, r1[k + 1] - r0[k + 1]))
            b.append(a[:m]); e.append(r0[k + 1] + np.arange(m) + 1)
    b.append(np.array([0, r0[0], r0[0] + 3], np.int64)); e.append(np.array([G, r1[-1], r1[-1] - 2], np.int64))      # and across all of them
    beg, end = np.concatenate(b), np.concatenate(e)
    al.regions_set(beg, end)
    H = al.lift_regions()
    parity(H, hostlib.lift_regions(px, qry, r, beg, end))
    al.close()
    assert H.size == beg.size
    iA, iB, gA, gB, _, _ = rm.end_records(d, G, H, beg, end)
    isbig = np.zeros(d["f_rpos"].size, bool); isbig[big] = True
    assert ((iA == iB) & isbig[iA]).sum() > 1000 and ((iA != iB) & isbig[iA] & isbig[iB]).sum() > 100
    assert (H["n_ins"] > 0).any() and (H["n_del"] > 0).any() and (H["n_x"] > 0).any()


def test_regions_of_a_bundle(golden_dir, cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer (q_lo / q_hi relative to contig k), asked for out of order and repeatedly"""
    px = os.path.join(golden_dir, "cx")
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    beg, end = rm.stride_regions(cx_index.chr_len)
    al = capi.Aligner(cx_index)
    al.regions_set(beg, end)
    single = [aligned_regions(al, px, c, beg, end)[0] for c in contigs]
    assert single[2].size == 0 and all(single[k].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.lift_regions(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.lift_regions(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.lift_regions(-1)
    al.close()


def test_regions_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    G = int(cx_index.G)
    beg, end = rm.stride_regions(cx_index.chr_len, lengths=(1, 65, 1000), stride=11)
    al = capi.Aligner(cx_index)
    al.regions_set(beg, end)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.lift_regions()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.lift_regions()
    al.run_to(8)
    a = al.lift_regions()
    assert a.size > 0 and same(a, hostlib.lift_regions(px, cur, al.blocks(), beg, end)) and al.region_timing()[1] == 1      # (a refused call runs no pass)
    # without regions: GSA_ERR_STATE; a clone starts without them
    cl = al.clone()
    cl.align_contig(cur)
    with pytest.raises(capi.GsaError, match="error -4"):
        cl.lift_regions()
    cl.close()
    al.regions_set(np.zeros(0, np.int64), np.zeros(0, np.int64))
    with pytest.raises(capi.GsaError, match="error -4"):
        al.lift_regions()
    al.regions_set(beg, end)
    assert same(al.lift_regions(), a)
    # a bad region: refused, the first offender and its entry named, nothing changed
    s1 = int(cx_index.chr_len[0])
    for (b0, e0), why in (((G - 5, G + 1), "outside"), ((-1, 4), "outside"), ((G, G + 3), "outside"), ((50, 50), "empty"), ((60, 50), "reversed"), ((s1 - 3, s1 + 3), "crosses a sequence boundary")):
        b2, e2 = beg[:100].copy(), end[:100].copy(); b2[57], e2[57] = b0, e0; b2[80], e2[80] = 9, 9
        with pytest.raises(capi.GsaError, match=r"error -1: .*region \[%d, %d\) \(entry 57\).*%s" % (b0, e0, why)):
            al.regions_set(b2, e2)
        assert same(al.lift_regions(), a)
    # replacing the regions
    al.regions_set(beg[::-1].copy(), end[::-1].copy())
    b = al.lift_regions()
    assert same(b, hostlib.lift_regions(px, cur, al.blocks(), beg[::-1], end[::-1])) and b.size == a.size and not same(a, b)
    al.regions_set(beg, end)
    # the eight passes keep their answers apart, in several orders
    al.lift_set(np.arange(0, G, 5, dtype=np.int64)); al.track_set(1000); al.proj_open()
    cg = al.block_cigars(); v = al.call_variants(); s = al.block_cs(); lf = al.lift(); tk = al.track(); sg = al.block_segs(); pj = al.project(); word = al.proj_fetch(words=True)[1]
    assert cg[1].size > 0 and v[0].size > 0 and s[1].size > 0 and lf.size > 0 and tk.size > 0 and sg[1].size > 0 and pj[0] > 0
    for order in ("rlcvstgp", "pgtsvclr", "crsrlrtr", "vrprgrlr"):
        for what in order:
            if what == "r":
                assert same(al.lift_regions(), a), order
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
    assert same(al.lift_regions(), a)
    al.align_contig(nxt_p)
    assert same(al.lift_regions(), hostlib.lift_regions(px, nxt, al.blocks(), beg, end))
    # no block at all: n_hits = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    assert al.lift_regions().size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants,cigars,lift", [(1, True, False, False, False), (1, False, True, True, True), (3, True, True, False, True), (3, False, False, True, False)])
def test_align_many_with_regions(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants, cigars, lift):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    beg, end = rm.stride_regions(cx_index.chr_len, lengths=(1, 64, 1000), stride=13)
    pos = np.arange(0, int(cx_index.G), 3, dtype=np.int64)
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    g0.regions_set(beg, end)
    for g in ctxs:
        g.lift_set(pos)
    want, want_cig, want_var, want_lift = [], [], [], []
    for c in contigs:
        h, r = aligned_regions(g0, px, c, beg, end)
        want.append(h); want_cig.append(hostlib.cigars(None, c, r)); want_var.append(hostlib.variants(px, c, r)); want_lift.append(hostlib.lift(px, c, r, pos))
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, *more):
        h = capi.regions_array(more[-1])
        l = capi.lifts_array(more[0]) if lift else None
        c = capi.cigars_arrays(cig) if cig is not None else None
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (h, c, v, l)
        return 0

    def check(n):
        assert sorted(got) == list(range(n))
        for ci in got:
            assert same(got[ci][0], want[ci]), ci
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
        # one context without regions: GSA_ERR_STATE before any contig is aligned
        for g in ctxs[1:-1]:
            g.regions_set(beg, end)
        with pytest.raises(capi.GsaError, match="-> -4"):
            capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, regions=True)
        assert not got
        ctxs[-1].regions_set(beg, end)
    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=lift, regions=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cigars=cigars, lift=lift, regions=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_extras_regions_needs_the_want_bit(cx_index, cx_queries):
    """behind a gsa_extras of a call without GSA_WANT_REGIONS there is no region answer (GSA_ERR_STATE); bit 8 stays refused"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    al.regions_set(np.arange(0, 1000, dtype=np.int64), np.arange(0, 1000, dtype=np.int64) + 50)
    lib = al.lib
    lib.gsa_extras_regions.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.RegionLifts)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        l = capi.RegionLifts()
        rcs.append((lib.gsa_extras_regions(ex, C.byref(l)), int(l.n_hits), bool(ex.contents.cig)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_REGIONS, 0), (capi.WANT_REGIONS | capi.WANT_CIGARS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want and (rcs[0][1] > 0) == (rc_want == 0) and rcs[0][2] == bool(want & capi.WANT_CIGARS), (want, rcs)
    rcs.clear()
    assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, capi.WANT_REGIONS | 8, capi.RESULT_EX_FN(cb), None) == -1 and not rcs      # bit 8 stays refused
    al.close()


def run_cli(cwd, *args, check=True):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=check, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


@pytest.mark.parametrize("extra", [[], ["-fmt", "3", "-cs", "-gpuvar", "-lift"]])
def test_cli_liftbed_golden(golden_dir, cx_index, tmp_path, extra):
    """-liftbed with every reference sequence and the stride sets: out.regions.tsv is the text the reference's own MAF implies (regions_from_maf); the other files
    of the run are the bytes they are without the switch"""
    b1, e1 = rm.stride_regions(cx_index.chr_len, lengths=(), stride=7)      # every whole sequence, in front
    b2, e2 = rm.stride_regions(cx_index.chr_len)
    beg, end = np.concatenate([b1, b2[:-b1.size]]), np.concatenate([e1, e2[:-e1.size]])
    names = [f"r{i}" if i % 3 else "." for i in range(beg.size)]
    bed = str(tmp_path / "in.bed")
    with open(bed, "w") as fh:
        fh.write("track name=test\n#comment\n\nbrowser position chrA:1-10\n")
        fh.write(rm.bed_text(cx_index.chr_names, cx_index.chr_len, beg, end, [n + "\t0\t+" if n != "." else None for n in names]))
    args = list(extra)
    if "-lift" in args:
        pf = str(tmp_path / "pos.tsv")
        open(pf, "w").write("".join(f"{cx_index.chr_names[0]}\t{p}\n" for p in range(1, 2000, 7)))
        args.insert(args.index("-lift") + 1, pf)
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-liftbed", bed, "-timing", *args).stderr
    assert open(tmp_path / "out.regions.tsv").read() == rm.regions_tsv(os.path.join(golden_dir, "cx.maf"), cx_index.chr_names, cx_index.chr_len, beg, end, names)
    if extra:
        import cs_from_maf as cm
        assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(os.path.join(golden_dir, "cx.maf"))
        assert os.path.getsize(tmp_path / "out.lift.tsv") > 1000
    else:
        assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"regions_s": ' in timing[0]


def test_cli_liftbed_refuses_what_the_reference_does_not_hold(golden_dir, cx_index, tmp_path):
    """an unknown name, start >= end, an end beyond the sequence, a malformed line: status 1, one -liftbed line, no output file"""
    n0, l0 = cx_index.chr_names[0], int(cx_index.chr_len[0])
    for k, line in enumerate(("nosuchseq\t5\t9\n", f"{n0}\t9\t9\n", f"{n0}\t10\t{l0 + 1}\n", f"{n0}\t10\n", f"{n0}\t10\tx20\n", f"{n0}\t12\t5\n")):
        pf = str(tmp_path / f"bad{k}.bed")
        open(pf, "w").write(f"#c\n{n0}\t0\t10\tgene\n" + line)
        r = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / f"o{k}"), "-t", "1", "-liftbed", pf, check=False)
        assert r.returncode == 1 and sum(1 for ln in r.stderr.split(b"\n") if b"-liftbed" in ln) == 1, r.stderr
        assert not [f for f in os.listdir(tmp_path) if f.startswith(f"o{k}.")]
