"""CPU tests of the per-window query track (gsa_qtrack_win / gsa_qtracks, include/gsa_hip.h): the record layout, and the host walk gsah_c_qtrack -- the comparator of
the GPU pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, to the reference-side track (the same columns, seen from the other
sequence), to itself across window lengths, and to the trim, the depth-two count and the short last window on hand-made results (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import qtrack_from_maf as qm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import gapped, overrun_case      # noqa: F401  (fixture)
from test_track_host import golden_results             # noqa: F401  (fixture)

FIELDS = ("n_cov", "n_multi", "n_eq", "n_x", "n_ins", "n_del")
WINDOWS = (1, 64, 1000, 1 << 30)


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_qtrack_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_qtrack_win); }\nint sz2(void) { return (int)sizeof(gsa_qtracks); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'int o1(void) { return (int)offsetof(gsa_qtrack_win, len); }\nint o2(void) { return (int)offsetof(gsa_qtrack_win, n_multi); }\nint o3(void) { return (int)offsetof(gsa_qtrack_win, n_del); }\n'
                   'int o4(void) { return (int)offsetof(gsa_qtracks, win); }\nunsigned w(void) { return GSA_WANT_QTRACK; }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 32 == capi.QTRACK_WIN_DT.itemsize == C.sizeof(capi.QTrackWin) == qm.QTRACK_DT.itemsize
    assert x.sz2() == 16 == C.sizeof(capi.QTracks) and x.sz3() == 16
    assert x.o1() == 4 == capi.QTRACK_WIN_DT.fields["len"][1] and x.o2() == 12 == capi.QTRACK_WIN_DT.fields["n_multi"][1] and x.o3() == 28 == capi.QTRACK_WIN_DT.fields["n_del"][1]
    assert x.o4() == 8
    assert x.w() == 512 == capi.WANT_QTRACK
    assert capi.QTRACK_WIN_DT == qm.QTRACK_DT


def well_formed(T, qlen, W):
    assert T.dtype == capi.QTRACK_WIN_DT
    assert (np.diff(T["start"].astype(np.int64)) > 0).all() and (T["n_cov"] > 0).all()
    assert (T["start"] % W == 0).all() and (T["start"] >= 0).all() and np.array_equal(T["len"], np.minimum(T["start"].astype(np.int64) + W, qlen) - T["start"])
    assert (T["n_multi"] <= T["n_cov"]).all() and (T["n_cov"] <= T["len"]).all()
    depth = T["n_eq"].astype(np.int64) + T["n_x"] + T["n_ins"]
    # (every covered base lies in a kept column of every block that covers it: the depth sum is n_cov where no base is covered twice, and greater exactly elsewhere)
    assert (depth >= T["n_cov"]).all() and np.array_equal(depth == T["n_cov"], T["n_multi"] == 0)


def same(a, b, what=""):
    assert a.size == b.size, (what, a.size, b.size)
    for f in capi.QTRACK_WIN_DT.names:
        assert np.array_equal(a[f], b[f]), (what, f, np.flatnonzero(a[f] != b[f])[:5], a[a[f] != b[f]][:3], b[a[f] != b[f]][:3])


def regroup(T1, W, qlen):
    """the answer at W = 1 summed into windows of W bases"""
    j, inv = np.unique(T1["start"] // W, return_inverse=True)
    T = np.zeros(j.size, capi.QTRACK_WIN_DT)
    T["start"] = j * W; T["len"] = np.minimum((j.astype(np.int64) + 1) * W, qlen) - j.astype(np.int64) * W
    for f in FIELDS:
        T[f] = np.bincount(inv, weights=T1[f].astype(np.float64), minlength=j.size).astype(np.int64)
    return T


@pytest.mark.parametrize("key", ["cx", "cx_sen", "small"])
def test_host_qtrack_gives_what_the_reference_maf_implies(golden_results, key):
    """every contig, every field, W in {1, 64, 1000, 2^30}: hostlib.qtrack == the columns of the reference's MAF; the totals of the four classes == those of the
    reference-side track (no golden result is trimmed); the answer at W = 1 regrouped == the answer at every W"""
    px, idx, res = golden_results[key]
    seen = dict(ins=0, dele=0, x=0, multi=0, rev=0, holes=0, dup=0)
    for qn, seq, d, mine in res:
        qlen = len(seq)
        T1 = hostlib.qtrack(px, seq, d, 1)
        for W in WINDOWS:
            T = hostlib.qtrack(px, seq, d, W)
            well_formed(T, qlen, W)
            assert [b[0] == 1 for b in mine] == [bool(x) for x in d["b_bdup"]]
            same(T, qm.contig_qtrack(mine, qlen, W), (key, qn, W))
            same(T, regroup(T1, W, qlen), (key, qn, W, "regrouped"))
            R = hostlib.track(px, seq, d, W)
            for f in ("n_eq", "n_x", "n_ins", "n_del"):
                assert int(T[f].sum()) == int(R[f].sum()), (key, qn, W, f)
            seen["ins"] += int((T["n_ins"] > 0).sum()); seen["dele"] += int((T["n_del"] > 0).sum()); seen["x"] += int((T["n_x"] > 0).sum())
            seen["multi"] += int((T["n_multi"] > 0).sum()); seen["holes"] += (qlen + W - 1) // W - T.size
            seen["rev"] += sum(1 for b in mine if b[0] != 1 and b[2][3] == "-")
            # the reference's golden runs hold no duplicate block: the contig's first block marked as one leaves the track
            if len(mine) > 0:
                d2 = dict(d); d2["b_bdup"] = d["b_bdup"].copy(); d2["b_bdup"][0] = 1
                T2 = hostlib.qtrack(px, seq, d2, W)
                same(T2, qm.contig_qtrack(mine, qlen, W, score=[1] + [b[0] for b in mine[1:]]), (key, qn, W, "dup"))
                assert int(T2["n_eq"].sum()) < int(T["n_eq"].sum())
                seen["dup"] += 1
    # the ground this test stands on (GOLDEN_MULTI: the cases in which some query base lies under two counted blocks; tests/test_gpu_qtrack.py relies on it)
    assert seen["ins"] > 0 and seen["dele"] > 0 and seen["x"] > 0 and seen["holes"] > 0 and seen["dup"] > 0, seen
    assert (seen["multi"] > 0) == (key in GOLDEN_MULTI), seen
    if key != "small":
        assert seen["rev"] > 0, seen


# No golden case puts a query base under two counted blocks (checked here, on every run); twice_pair() below does, and tests/test_gpu_qtrack.py names it.
GOLDEN_MULTI = ()


def twice_pair(seed=1, seglen=4000, flank=6000, d=0.03):
    """(reference, query): a query segment that is present twice in the reference, each copy 3 % diverged from it -- collapsed sequence as an assembly shows it.  The
    two blocks that hold it are both counted (neither is a duplicate) and overlap in the query over about seglen bases."""
    rng = np.random.default_rng(seed)
    seg = synth.random_genome(seglen, rng)
    a, b, c = (synth.random_genome(flank, rng) for _ in range(3))
    ref = np.concatenate([a, synth.mutate(seg, d, rng), b, synth.mutate(seg, d, rng), c])
    qry = np.concatenate([synth.mutate(a, 0.01, rng), seg, synth.mutate(c, 0.01, rng)])
    return ref, qry


def test_qtrack_of_a_segment_present_twice_in_the_reference(oracle_built, tmp_path):
    """the oracle's finished blocks of twice_pair(): two counted blocks, no duplicate, and the segment's bases are under both"""
    ref, qry = twice_pair()
    fa, px = str(tmp_path / "r.fa"), str(tmp_path / "r")
    synth.write_fasta(fa, [("chr1", ref)]); hostlib.build_index(fa, px)
    o = oracle_built.Oracle(indexio.load_index(px), {})
    o.set_query(qry); o.run_to(8)
    d = o.blocks(with_aln=True)
    o.close()
    assert d["b_score"].size >= 2 and not d["b_bdup"].any()
    for W in (1, 1000):
        T = hostlib.qtrack(px, qry, d, W)
        well_formed(T, len(qry), W)
        assert 3500 <= int(T["n_multi"].sum()) <= 4100 and int(T["n_cov"].sum()) > 15000, (W, int(T["n_multi"].sum()))
        R = hostlib.track(px, qry, d, W)
        for f in ("n_eq", "n_x", "n_ins", "n_del"):
            assert int(T[f].sum()) == int(R[f].sum()), (W, f)


def junction_pair(seed=3, n=6000, indel=False):
    """([(name, reference sequence)] x 2, query): the query joins the last 3000 bases of chrA to the first 3000 of chrB, so a seed runs across the junction and the
    block that holds it runs past the end of its chromosome copy: it is cut there, inside that seed.  indel: three bases deleted and one changed shortly in front of
    the junction, so that the trimmed block also holds a gap record."""
    rng = np.random.default_rng(seed)
    A, B = synth.random_genome(n, rng), synth.random_genome(n, rng)
    tail, head = A[n - 3000:].copy(), B[:3000].copy()
    if indel:
        tail = np.concatenate([tail[:-12], tail[-9:]])
        tail[-5] = ord("A") if tail[-5] != ord("A") else ord("C")
    return [("chrA", A), ("chrB", B)], np.concatenate([tail, head])


def overruns(blocks, frags, idx):
    """per block: the reference bases by which its last record runs past the end of its chromosome copy (gsa_frag fields by name)"""
    G = int(idx.G)
    fwd = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    out = []
    for b in blocks:
        last = frags[int(b["frag_off"]) + int(b["n_frag"]) - 1]
        c = int(b["chr"])
        lim = fwd[c] + int(idx.chr_len[c]) if b["bdir"] else 2 * G - fwd[c]
        out.append(max(int(last["rpos"]) + int(last["rlen"]) - int(lim), 0))
    return out


@pytest.mark.parametrize("indel,rc", [(False, False), (False, True), (True, False)])
def test_qtrack_of_a_block_that_the_aligner_runs_over_a_sequence_end(oracle_built, tmp_path, indel, rc):
    """junction_pair() through the oracle: the block is trimmed inside its last seed, on either strand, and the query bases behind the cut are uncovered"""
    refs, qry = junction_pair(indel=indel)
    if rc:
        qry = np.ascontiguousarray(synth.revcomp(qry))
    fa, px = str(tmp_path / "r.fa"), str(tmp_path / "r")
    synth.write_fasta(fa, refs); hostlib.build_index(fa, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx, {})
    o.set_query(qry); o.run_to(8)
    d = o.blocks(with_aln=True)
    o.close()
    assert d["b_score"].size == 1 and int(d["b_bdir"][0]) == (0 if rc else 1)
    l = int(d["b_nfrag"][0]) - 1
    assert d["f_bseed"][l] == 1 and (int(d["b_nfrag"][0]) > 1) == indel
    for W in (1, 100, 1 << 30):
        T = hostlib.qtrack(px, qry, d, W)
        well_formed(T, len(qry), W)
        assert int(T["n_cov"].sum()) == (2997 if indel else 3000) == int(T["n_eq"].sum()) + int(T["n_x"].sum()) and int(T["n_del"].sum()) == (3 if indel else 0)
        assert int(T["start"][-1]) + int(T["len"][-1]) <= (3000 if W < 1000 else len(qry)) and int(T["start"][0]) == 0
        R = hostlib.track(px, qry, d, W)
        for f in ("n_eq", "n_x", "n_ins", "n_del"):
            assert int(T[f].sum()) == int(R[f].sum()), (W, f)


def hand_made(px, blocks):
    """a result dict in the oracle's dump layout over the index at px: blocks = [(bdir, chr, bdup, [('s', qpos, rpos, len) | ('g', ops, ref, qry) behind a seed])]"""
    B, F, A1, A2 = [], [], [], []
    for bdir, chrom, bdup, recs in blocks:
        cols, nf = 0, 0
        for r in recs:
            if r[0] == "s":
                F.append((1, r[1], r[3], r[3], r[2], 0)); cols += r[3]
            else:
                _, qp, ql, rl, rp, _ = F[-1]
                a1, a2, rn, qn = gapped(r[2], r[3], rp + rl, qp + ql, r[1])
                F.append((0, qp + ql, qn, rn, rp + rl, len(a1))); A1.append(a1); A2.append(a2); cols += len(a1)
            nf += 1
        B.append((cols - 3, cols, bdup, nf, bdir, 1, chrom))
    return {"b_score": np.array([b[0] for b in B], np.int32), "b_aln_len": np.array([b[1] for b in B], np.int32), "b_bdup": np.array([b[2] for b in B], np.int32),
            "b_nfrag": np.array([b[3] for b in B], np.int32), "b_bdir": np.array([b[4] for b in B], np.int32), "b_gpos": np.array([b[5] for b in B], np.int32),
            "b_chr": np.array([b[6] for b in B], np.int32),
            "f_bseed": np.array([f[0] for f in F], np.int32), "f_qpos": np.array([f[1] for f in F], np.int32), "f_qlen": np.array([f[2] for f in F], np.int32),
            "f_rlen": np.array([f[3] for f in F], np.int32), "f_rpos": np.array([f[4] for f in F], np.int64), "f_alnlen": np.array([f[5] for f in F], np.int32),
            "aln1": np.frombuffer(b"".join(A1), np.uint8), "aln2": np.frombuffer(b"".join(A2), np.uint8)}


def test_qtrack_carries_the_trim_over_from_the_reference(overrun_case):
    """the hand-made result whose blocks run past the end of their reference sequences: query bases behind the cut are uncovered, the duplicate contributes nothing.
    Blocks 0 and 2 are cut inside their last SEED (arithmetic), blocks 1 and 3 inside their last GAP (the columns decide)."""
    px, qfa, qry, dump = overrun_case
    qlen = len(qry)
    # block 0: seed q[10, 60), gap MMDDMIM q[60, 66), seed q[66, 116) r[355, 405) cut at 400 -> q[10, 111)
    # block 1: seed q[200, 240), gap of 16 M q[240, 256) then D M M I M | I ...: the reference base 400 is the second I -> q[200, 260)
    # block 2 (reverse strand of chrB, text [900, 1000)): seed q[400, 460), gap MDMMIIM q[460, 465), seed q[465, 503) r[966, 1004) cut at 1000 -> q[400, 499)
    # block 3 (reverse strand): seed q[600, 645), gap of 23 M q[645, 668) then I I | M ...: r 998 and 999 face '-', the M on r 1000 is cut -> q[600, 668)
    # block 4 (a duplicate): not counted.  block 5: seed q[900, 930), gap IIMM, seed q[932, 952): nothing to trim
    spans = [(10, 111), (200, 260), (400, 499), (600, 668), (900, 952)]
    T1 = hostlib.qtrack(px, qry, dump, 1)
    well_formed(T1, qlen, 1)
    assert T1["start"].tolist() == [q for a, b in spans for q in range(a, b)]
    assert (T1["n_cov"] == 1).all() and (T1["n_multi"] == 0).all() and ((T1["n_eq"] + T1["n_x"] + T1["n_ins"]) == 1).all()
    at = {int(s): t for s, t in zip(T1["start"], T1)}
    assert [int(at[q]["n_ins"]) for q in (62, 63, 256, 461)] == [1, 1, 1, 1] and int(T1["n_ins"].sum()) == 4
    # deletions are charged to the query base in front of them: r 353 -> q 64; r 398 -> q 258; r 963, 964 -> q 463; r 998, 999 -> q 667; r 40, 41 -> q 929
    assert {int(t["start"]): int(t["n_del"]) for t in T1 if t["n_del"]} == {64: 1, 258: 1, 463: 2, 667: 2, 929: 2}
    for W in (7, 100, 1000):
        T = hostlib.qtrack(px, qry, dump, W)
        well_formed(T, qlen, W)
        same(T, regroup(T1, W, qlen), W)
        assert int(T["n_cov"].sum()) == sum(b - a for a, b in spans)
    # the duplicate alone, and no block at all: n_win = 0
    nf = np.concatenate([[0], np.cumsum(dump["b_nfrag"])])
    only = {k: v[4:5] for k, v in dump.items() if k.startswith("b_")}
    only.update({k: v[int(nf[4]):int(nf[5])] for k, v in dump.items() if k.startswith("f_")})
    only["aln1"] = dump["aln1"][:0]; only["aln2"] = dump["aln2"][:0]
    assert hostlib.qtrack(px, qry, only, 10).size == 0
    assert hostlib.qtrack(px, qry, {k: v[:0] for k, v in dump.items()}, 10).size == 0


def test_qtrack_cut_inside_a_gap_keeps_the_insertion_behind_the_last_kept_base(overrun_case):
    """a sibling of the overrun result: one forward block on chrA (ends at 400) whose cut falls inside a gap record that is NOT the last record -- an inserted base right
    behind the last kept reference base is kept (the base in front of it is), the columns behind it and the whole seed that follows are not"""
    px, qfa, qry, _ = overrun_case
    ref = np.ascontiguousarray(indexio.load_index(px).ref)
    # seed q[1200, 1230) r[360, 390); gap at r 390 / q 1230: 8 M (r 390..397, q 1230..1237), D D (q 1238, 1239), M (r 398, q 1240), I (r 399, charged to q 1240),
    # D (q 1241: behind r 399, the last kept base -> kept), M on r 400: cut.  Then M M and a seed of 20: all behind the cut
    dump = hand_made(px, [(1, 0, 0, [("s", 1200, 360, 30), ("g", b"M" * 8 + b"DDMIDMMM", ref, qry), ("s", 1245, 403, 20)])])
    assert int(dump["f_qpos"][2]) == 1245 and int(dump["f_rpos"][2]) == 403
    T1 = hostlib.qtrack(px, qry, dump, 1)
    well_formed(T1, len(qry), 1)
    assert T1["start"].tolist() == list(range(1200, 1242))
    assert T1["start"][T1["n_ins"] > 0].tolist() == [1238, 1239, 1241] and T1["start"][T1["n_del"] > 0].tolist() == [1240]
    assert int(T1["n_eq"].sum()) + int(T1["n_x"].sum()) == 30 + 8 + 1
    T = hostlib.qtrack(px, qry, dump, 40)
    assert T["start"].tolist() == [1200, 1240] and T["n_cov"].tolist() == [40, 2] and T["n_ins"].tolist() == [2, 1] and T["n_del"].tolist() == [0, 1]
    # the reference side trims the same columns: the totals agree class by class
    R = hostlib.track(px, qry, dump, 40)
    for f in ("n_eq", "n_x", "n_ins", "n_del"):
        assert int(T[f].sum()) == int(R[f].sum()), f


def test_qtrack_counts_bases_under_two_blocks_and_a_short_last_window(overrun_case):
    """two counted blocks whose query intervals overlap in q[150, 180), a third that merely touches the second, a duplicate over all of it, and a contig of 215 bases
    at W = 50: the last window is 15 bases long"""
    px, qfa, qry, _ = overrun_case
    ref = np.ascontiguousarray(indexio.load_index(px).ref)
    dump = hand_made(px, [(1, 0, 0, [("s", 100, 10, 80)]),                                              # q[100, 180)
                          (1, 1, 0, [("s", 150, 450, 30), ("g", b"MIMDM", ref, qry), ("s", 184, 484, 21)]),   # q[150, 205): M I M D M = q 180, -, 181, 182, 183
                          (1, 0, 0, [("s", 205, 200, 5)]),                                               # q[205, 210): touches, no overlap
                          (1, 0, 1, [("s", 90, 250, 120)])])                                             # a duplicate: not counted
    T = hostlib.qtrack(px, 215, dump, 50)
    well_formed(T, 215, 50)
    assert T["start"].tolist() == [100, 150, 200] and T["len"].tolist() == [50, 50, 15]
    assert T["n_cov"].tolist() == [50, 50, 10] and T["n_multi"].tolist() == [0, 30, 0]
    assert (T["n_eq"] + T["n_x"] + T["n_ins"]).tolist() == [50, 80, 10] and T["n_ins"].tolist() == [0, 1, 0] and T["n_del"].tolist() == [0, 1, 0]
    T1 = hostlib.qtrack(px, 215, dump, 1)
    well_formed(T1, 215, 1)
    assert T1["start"][T1["n_multi"] > 0].tolist() == list(range(150, 180))
    same(T, regroup(T1, 50, 215))
    # one window over the whole contig
    Tw = hostlib.qtrack(px, 215, dump, 1 << 30)
    assert Tw["start"].tolist() == [0] and Tw["len"].tolist() == [215] and Tw["n_cov"].tolist() == [110] and Tw["n_multi"].tolist() == [30]


def test_qtrack_tsv_of_the_golden_maf_is_the_host_walk_as_text(golden_results, golden_dir):
    """qtrack_from_maf.qtrack_tsv (what the CLI test compares with) against hostlib.qtrack formatted the way Emitter::qtrack_text does: one line per query contig and
    covered window, BED-style coordinates inside the contigs"""
    px, idx, res = golden_results["small"]
    txt = qm.qtrack_tsv(os.path.join(golden_dir, "small.maf"), 100)
    want = [qm.HEADER]
    for qn, seq, d, _ in res:
        for t in hostlib.qtrack(px, seq, d, 100):
            want.append("\t".join([qn.split()[0]] + [str(int(x)) for x in (t["start"], int(t["start"]) + int(t["len"]), t["n_cov"], t["n_multi"], t["n_eq"], t["n_x"], t["n_ins"], t["n_del"])]) + "\n")
    assert txt == "".join(want) and len(want) > 10
