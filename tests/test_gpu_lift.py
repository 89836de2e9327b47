"""gsa_lift on the GPU box: reference positions carried through a finished alignment on the device -- block search, record search and gap walk over records, op
strings and the two sequences -- must equal, hit for hit and field for field, what the host walk over the gapped strings gives (gsah_c_lift, pinned to the
reference's MAF files in test_lift_host.py): through the single-contig call, bundles, gsa_align_many_ex and the CLI's -lift."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import lift_from_maf as lm
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.dtype == capi.LIFT_HIT_DT and b.dtype == capi.LIFT_HIT_DT and a.size == b.size and a.tobytes() == b.tobytes()


def aligned_lift(al, px, seq, pos):
    """align one contig and lift the context's positions (pos: the same list, for the host): (device hits, result dict), parity asserted"""
    r = al.align_contig(seq)
    got = al.lift()
    want = hostlib.lift(px, seq, r, pos)
    assert got.size == want.size, (got.size, want.size)
    for f in capi.LIFT_HIT_DT.names:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:5], got[got[f] != want[f]][:3], want[got[f] != want[f]][:3])
    return got, r


@pytest.mark.parametrize("name,params,wide", [("cx", {}, False), ("cx", {}, True), ("cx", dict(sen=1, clr=50), False), ("small", {}, False)])
def test_lift_matches_the_host_walk(golden_dir, name, params, wide):
    """ALL reference positions (cx: well above 3 x 65 536 of them, so the second tile of the scan over the workgroups' sums carries), then the same positions
    shuffled, and a list in which positions repeat: the answers are per idx"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    G = int(idx.G)
    if name == "cx":
        assert G > 3 * 65536
    allpos = np.arange(G, dtype=np.int64)
    rng = np.random.default_rng(17)
    perm = rng.permutation(G).astype(np.int64)
    rep = rng.integers(0, G, 5000).astype(np.int64); rep[1::2] = rep[0::2]
    al = capi.Aligner(idx, wide=wide, **params)
    classes, rev, multi, none, n = set(), 0, 0, 0, 0
    for ci, (_, seq) in enumerate(synth.read_fasta(px + ".qry.fa")):
        al.lift_set(allpos)
        H, r = aligned_lift(al, px, seq, allpos)
        classes |= set(H["cls"].tolist()); rev += int(H["rev"].sum()); multi += int((H["n_cover"] > 1).sum()); none += G - H.size; n += H.size
        assert (np.diff(H["idx"]) > 0).all()
        if ci == 0:
            # the same contig's result, other position lists: each hit is the hit of its position
            by_pos = np.full(G, -1, np.int64); by_pos[H["idx"]] = np.arange(H.size)
            for lst in (perm, rep):
                al.lift_set(lst)
                P = al.lift()
                assert same(P, hostlib.lift(px, seq, r, lst))
                assert (np.diff(P["idx"]) > 0).all() and np.array_equal(P["idx"], np.flatnonzero(by_pos[lst] >= 0))
                src = H[by_pos[lst[P["idx"]]]]
                for f in ("qpos", "block", "cls", "rev", "n_cover"):
                    assert np.array_equal(P[f], src[f]), f
            assert al.lift_timing()[1] == 3
    al.close()
    assert n > 1000 and rev > 0 and none > 0 and classes == {2, 7, 8}, (n, rev, none, classes)
    if name == "cx":
        assert multi > 0


@pytest.fixture(scope="module")
def large_gap_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("lgl")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("dp_safe", [0, 1])
def test_lift_through_large_dp_gaps(large_gap_case, dp_safe):
    """Gaps of more than 64 columns are walked by a whole wavefront, and they are large DP jobs: their gapped strings never exist in the device's string pools,
    the columns come from the job's op string.  dp_safe = 1: one striped job per launch.  At least one hit of each class lies inside such a gap."""
    px, idx, qry = large_gap_case
    G = int(idx.G)
    allpos = np.arange(G, dtype=np.int64)
    al = capi.Aligner(idx)
    if dp_safe:
        al.set_option("dp_safe", 1)
    al.lift_set(allpos)
    H, r = aligned_lift(al, px, qry, allpos)
    al.close()
    inside = set()
    B, F = r["blocks"], r["frags"]
    for i in np.flatnonzero((F["bseed"] == 0) & (F["aln_len"] > 64) & (F["rlen"] > 0) & (F["qlen"] > 0)):
        bi = int(np.flatnonzero((B["frag_off"] <= i) & (i < B["frag_off"] + B["n_frag"]))[0])
        t = np.arange(int(F["rpos"][i]), int(F["rpos"][i]) + int(F["rlen"][i]))
        p = np.where(t < G, t, 2 * G - 1 - t)
        inside |= set(H["cls"][np.isin(H["idx"], p) & (H["block"] == bi)].tolist())      # (hits whose chosen block is the gap's own block lie inside this gap)
    assert inside == {2, 7, 8}, inside


def test_lift_of_a_bundle(golden_dir, cx_index, cx_queries):
    """contig k of a bundle: field for field the single-contig answer (qpos relative to contig k), asked for out of order and repeatedly"""
    px = os.path.join(golden_dir, "cx")
    rng = np.random.default_rng(3)
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][:41234]),
               synth.random_genome(12345, rng), np.ascontiguousarray(cx_queries[2][1][1000:28001])]
    allpos = np.arange(int(cx_index.G), dtype=np.int64)
    al = capi.Aligner(cx_index)
    al.lift_set(allpos)
    single = [aligned_lift(al, px, c, allpos)[0] for c in contigs]
    assert single[2].size == 0 and all(single[k].size > 0 for k in (0, 1, 3))
    res = al.align_bundle(contigs)
    assert [r["blocks"].size > 0 for r in res] == [True, True, False, True]
    for k in (3, 0, 2, 1, 0):
        assert same(al.lift(k), single[k]), k
    with pytest.raises(capi.GsaError, match="error -1"):
        al.lift(len(contigs))
    with pytest.raises(capi.GsaError, match="error -1"):
        al.lift(-1)
    al.close()


def test_lift_call_order(golden_dir, cx_index, cx_queries):
    px = os.path.join(golden_dir, "cx")
    cur, nxt = cx_queries[0][1], cx_queries[1][1]
    G = int(cx_index.G)
    pos = np.arange(0, G, 3, dtype=np.int64)
    al = capi.Aligner(cx_index)
    al.lift_set(pos)
    with pytest.raises(capi.GsaError, match="error -4"):      # GSA_ERR_STATE: nothing aligned yet
        al.lift()
    al.set_query(cur); al.run_to(7)
    with pytest.raises(capi.GsaError, match="error -4"):
        al.lift()
    al.run_to(8)
    a = al.lift()
    assert a.size > 0 and same(a, hostlib.lift(px, cur, al.blocks(), pos)) and al.lift_timing()[1] == 1      # (a refused call runs no pass)
    # without positions: GSA_ERR_STATE; a clone starts without them
    cl = al.clone()
    cl.align_contig(cur)
    with pytest.raises(capi.GsaError, match="error -4"):
        cl.lift()
    cl.close()
    al.lift_set(np.zeros(0, np.int64))
    with pytest.raises(capi.GsaError, match="error -4"):
        al.lift()
    al.lift_set(pos)
    assert same(al.lift(), a)
    # a position outside [0, G): refused, the first offender named, nothing changed
    for bad in (G, -1):
        p2 = pos[:100].copy(); p2[57] = bad
        with pytest.raises(capi.GsaError, match=r"error -1: .*position %d \(entry 57\)" % bad):
            al.lift_set(p2)
        assert same(al.lift(), a)
    # replacing the positions
    al.lift_set(pos[::-1].copy())
    b = al.lift()
    assert same(b, hostlib.lift(px, cur, al.blocks(), pos[::-1])) and b.size == a.size and not same(a, b)
    al.lift_set(pos)
    # the four passes keep their answers apart, in any order
    cg = al.block_cigars(); v = al.call_variants(); s = al.block_cs()
    assert cg[1].size > 0 and v[0].size > 0 and s[1].size > 0
    for order in ("lscv", "vlsc", "cslv", "vcsl"):
        for what in order:
            if what == "l":
                assert same(al.lift(), a), order
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
    assert same(al.lift(), a)
    al.align_contig(nxt_p)
    assert same(al.lift(), hostlib.lift(px, nxt, al.blocks(), pos))
    # no block at all: n_hits = 0
    al.align_contig(synth.random_genome(20000, np.random.default_rng(5)))
    assert al.lift().size == 0
    al.close()


@pytest.mark.parametrize("n_ctx,bundle,variants,cigars", [(1, True, False, False), (1, False, True, True), (3, True, True, False), (3, False, False, True)])
def test_align_many_with_lift(golden_dir, cx_index, cx_queries, n_ctx, bundle, variants, cigars):
    px = os.path.join(golden_dir, "cx")
    contigs = [np.ascontiguousarray(q) for _, q in cx_queries] + [np.ascontiguousarray(cx_queries[0][1][:33333]), np.ascontiguousarray(cx_queries[1][1][500:41234])]
    pos = np.arange(0, int(cx_index.G), 2, dtype=np.int64)
    g0 = capi.Aligner(cx_index); ctxs = [g0] + [g0.clone() for _ in range(n_ctx - 1)]
    g0.lift_set(pos)
    want, want_cig, want_var = [], [], []
    for c in contigs:
        h, r = aligned_lift(g0, px, c, pos)
        want.append(h); want_cig.append(hostlib.cigars(None, c, r)); want_var.append(hostlib.variants(px, c, r))
    got, lock = {}, threading.Lock()

    def on_result(ci, res, var, cig, lf):
        h = capi.lifts_array(lf)
        c = capi.cigars_arrays(cig) if cig is not None else None
        v = capi.variants_array(var) if var is not None else None
        with lock:
            got[ci] = (h, c, v, int(res.n_blocks))
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

    if n_ctx > 1:
        # one context without positions: GSA_ERR_STATE before any contig is aligned
        for g in ctxs[1:-1]:
            g.lift_set(pos)
        with pytest.raises(capi.GsaError, match="-> -4"):
            capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=True)
        assert not got
        ctxs[-1].lift_set(pos)
    capi.align_many(ctxs, contigs, on_result, bundle=bundle, variants=variants, cigars=cigars, lift=True)
    check(len(contigs))
    # ONE contig and several contexts: seeded by chunk range on all of them (split_min lowered: the contig is 120 kb), finished by the first
    if n_ctx > 1:
        ctxs[0].set_option("split_min", 50000)
        got.clear()
        capi.align_many(ctxs, contigs[:1], on_result, variants=variants, cigars=cigars, lift=True)
        check(1)
    for g in ctxs[1:]:
        g.close()
    g0.close()


def test_extras_lift_needs_the_want_bit(cx_index, cx_queries):
    """behind a gsa_extras of a call without GSA_WANT_LIFT there is no lift answer (GSA_ERR_STATE)"""
    contigs = [np.ascontiguousarray(cx_queries[0][1][:33333])]
    al = capi.Aligner(cx_index)
    al.lift_set(np.arange(1000, dtype=np.int64))
    lib = al.lib
    lib.gsa_extras_lift.argtypes = [C.POINTER(capi.Extras), C.POINTER(capi.Lifts)]
    lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, capi.RESULT_EX_FN, C.c_void_p]
    rcs = []

    def cb(user, ci, res, ex):
        l = capi.Lifts()
        rcs.append((lib.gsa_extras_lift(ex, C.byref(l)), int(l.n_hits), bool(ex.contents.cig)))
        return 0

    ctxs = (C.c_void_p * 1)(al.ctx)
    qs = (C.c_char_p * 1)(C.cast(contigs[0].ctypes.data, C.c_char_p)); ql = (C.c_int32 * 1)(int(contigs[0].size))
    for want, rc_want in ((capi.WANT_CIGARS, -4), (capi.WANT_LIFT, 0), (capi.WANT_LIFT | capi.WANT_CIGARS, 0)):
        rcs.clear()
        assert lib.gsa_align_many_ex(ctxs, 1, qs, ql, 1, 0, want, capi.RESULT_EX_FN(cb), None) == 0
        assert len(rcs) == 1 and rcs[0][0] == rc_want and rcs[0][2] == bool(want & capi.WANT_CIGARS), (want, rcs)
    al.close()


def run_cli(cwd, *args, check=True):
    return subprocess.run([hostlib.CLI_PATH, *args], cwd=cwd, check=check, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)


def position_file(path, idx, vcf_like=False):
    """every reference position, in order: name <tab> 1-based position (vcf_like: a header line and further columns, which are ignored)"""
    with open(path, "w") as fh:
        if vcf_like:
            fh.write("##fileformat=VCFv4.1\n#CHROM\tPOS\tID\n")
        for n, l in zip(idx.chr_names, idx.chr_len.tolist()):
            fh.write("".join(f"{n}\t{p}\t.\tA\n" if vcf_like else f"{n}\t{p}\n" for p in range(1, l + 1)))


@pytest.mark.parametrize("extra", [[], ["-fmt", "3", "-cs", "-gpuvar"]])
def test_cli_lift_golden(golden_dir, cx_index, tmp_path, extra):
    """-lift with every reference position: out.lift.tsv is the text the reference's own MAF implies (lift_from_maf); the other files of the run are the bytes they
    are without the switch"""
    pf = str(tmp_path / "pos.tsv")
    position_file(pf, cx_index, vcf_like=bool(extra))
    err = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / "out"), "-t", "1", "-lift", pf, "-timing", *extra).stderr
    assert open(tmp_path / "out.lift.tsv").read() == lm.lift_tsv(os.path.join(golden_dir, "cx.maf"), cx_index.chr_names, cx_index.chr_len)
    if extra:
        import cs_from_maf as cm
        assert open(tmp_path / "out.paf", "rb").read() == cm.paf_cs_of_maf(os.path.join(golden_dir, "cx.maf"))
    else:
        assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
    timing = [ln for ln in err.split(b"\n") if ln.startswith(b"GSA_TIMING ")]
    assert len(timing) == 1 and b'"lift_s": ' in timing[0]


def test_cli_lift_refuses_what_the_reference_does_not_hold(golden_dir, cx_index, tmp_path):
    for k, line in enumerate((f"nosuchseq\t5\n", f"{cx_index.chr_names[0]}\t{int(cx_index.chr_len[0]) + 1}\n", f"{cx_index.chr_names[0]}\t0\n")):
        pf = str(tmp_path / f"bad{k}.tsv")
        open(pf, "w").write(f"#c\n{cx_index.chr_names[0]}\t1\n" + line)
        r = run_cli(golden_dir, "-i", "cx", "-q", "cx.qry.fa", "-o", str(tmp_path / f"o{k}"), "-t", "1", "-lift", pf, check=False)
        assert r.returncode == 1 and sum(1 for ln in r.stderr.split(b"\n") if b"-lift" in ln) == 1
        assert not [f for f in os.listdir(tmp_path) if f.startswith(f"o{k}.")]
