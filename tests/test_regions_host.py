"""CPU tests of lifting reference intervals through an alignment (gsa_region_hit / gsa_region_lifts, include/gsa_hip.h): the record layout, and the host walk
gsah_c_lift_regions -- the comparator of the GPU pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, to the host CIGARs of the same
blocks, to the point lift of the same result, and to the iExtension trim and the choice rule on a hand-made result that runs past the end of its reference sequences
(no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import paf_from_maf as pm
import regions_from_maf as rm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import overrun_case      # noqa: F401  (fixture)

FIXTURES = [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")]
KINDS = ("reverse", "multi", "clip_lo", "clip_hi", "one_gap", "two_gaps", "empty_query", "ins", "one_record", "by_overlap")


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_region_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_region_hit); }\nint sz2(void) { return (int)sizeof(gsa_region_lifts); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   + "".join(f"int o_{f}(void) {{ return (int)offsetof(gsa_region_hit, {f}); }}\n" for f in capi.REGION_HIT_DT.names) + "unsigned w(void) { return GSA_WANT_REGIONS; }\n")
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 48 == capi.REGION_HIT_DT.itemsize == C.sizeof(capi.RegionHit)
    assert x.sz2() == 16 == C.sizeof(capi.RegionLifts) and x.sz3() == 16 == C.sizeof(capi.Extras)
    want = dict(idx=0, block=4, off_lo=8, off_hi=12, q_lo=16, q_hi=20, n_eq=24, n_x=28, n_del=32, n_ins=36, rev=40, _pad0=41, n_cover=42, _pad1=44)
    for f, o in want.items():
        assert getattr(x, "o_" + f)() == o == capi.REGION_HIT_DT.fields[f][1] == getattr(capi.RegionHit, f).offset, f
    assert x.w() == 256 == capi.WANT_REGIONS
    assert {"gsa_regions_set", "gsa_lift_regions", "gsa_get_region_timing", "gsa_extras_regions"} <= set(capi.EXPORTS)


def region_set(idx, d):
    """the regions of one contig: the stride sets, every whole sequence, and every interval inside one gap record of the contig's result"""
    b1, e1 = rm.stride_regions(idx.chr_len)
    b2, e2 = rm.gap_record_regions(d, idx.chr_len)
    return np.concatenate([b1, b2]), np.concatenate([e1, e2])


def kinds_of(d, G, H, beg, end, by_overlap=None):
    """which of the kinds the tests stand on the hits H show (a dict of counts)"""
    n = {k: 0 for k in KINDS}
    if H.size == 0:
        return n
    iA, iB, gA, gB, t_lo, t_hi = rm.end_records(d, G, H, beg, end)
    ln = (end - beg)[H["idx"]]
    n["reverse"] = int((H["rev"] != 0).sum()); n["multi"] = int((H["n_cover"] > 1).sum())
    n["clip_lo"] = int((H["off_lo"] > 0).sum()); n["clip_hi"] = int((H["off_hi"] < ln).sum())
    n["one_gap"] = int(((iA == iB) & gA).sum()); n["two_gaps"] = int(((iA != iB) & gA & gB).sum())
    n["empty_query"] = int((H["q_lo"] == H["q_hi"]).sum()); n["ins"] = int((H["n_ins"] > 0).sum())
    n["one_record"] = int(((iA == iB) & (t_lo == d["f_rpos"][iA]) & (t_hi == d["f_rpos"][iA] + d["f_rlen"][iA])).sum())
    if by_overlap is not None:
        n["by_overlap"] = int(by_overlap.sum())
    return n


def assert_kinds(name, seen):
    """cx (narrow and -sen) shows every kind; small has one block per contig that starts with its sequence: no second covering block, no clip in front"""
    need = KINDS if name == "cx" else [k for k in KINDS if k not in ("multi", "clip_lo", "by_overlap")]
    assert all(seen[k] > 0 for k in need), (name, seen)


def cigar_regions(d, ops_blk, ops, bi, starts, G, beg, end):
    """Second derivation, no MAF: from the host CIGAR ops of block bi (output order: reference-forward) and its end records, what a result that holds this block
    ALONE gives for the regions (beg, end): dict of arrays over the regions that overlap the block's trimmed coverage, and their indices."""
    f0 = int(np.concatenate([[0], np.cumsum(d["b_nfrag"])])[bi]); nf = int(d["b_nfrag"][bi])
    o = ops[int(ops_blk["cig_off"][bi]):int(ops_blk["cig_off"][bi]) + int(ops_blk["n_cig"][bi])]
    cls = np.repeat((o & 15).astype(np.uint8), (o >> 4).astype(np.int64))
    rc = cls != 1; qc = cls != 2
    cols = np.flatnonzero(rc)
    z = np.zeros(1, np.int64)
    nq = np.concatenate([z, np.cumsum(qc)])
    pre = {c: np.concatenate([z, np.cumsum(cls == c)]) for c in (7, 8, 2, 1)}
    first_r, first_q = int(d["f_rpos"][f0]), int(d["f_qpos"][f0])
    last_r = int(d["f_rpos"][f0 + nf - 1]) + int(d["f_rlen"][f0 + nf - 1]); last_q = int(d["f_qpos"][f0 + nf - 1]) + int(d["f_qlen"][f0 + nf - 1])
    assert cols.size == last_r - first_r
    fwd = bool(d["b_bdir"][bi]); c = int(d["b_chr"][bi])
    g0, g1 = (first_r, last_r) if fwd else (2 * G - last_r, 2 * G - first_r)      # the untrimmed block in forward coordinates; output column j of a reference base holds g0 + j
    c0, c1 = max(g0, int(starts[c])), min(g1, int(starts[c + 1]))                  # the trim
    lo = np.maximum(beg, c0); hi = np.minimum(end, c1)
    w = np.flatnonzero(hi > lo)
    lo, hi = lo[w], hi[w]
    cs = cols[lo - g0]; ce = cols[hi - 1 - g0]
    r = {k: pre[k2][ce + 1] - pre[k2][cs] for k, k2 in (("n_eq", 7), ("n_x", 8), ("n_del", 2), ("n_ins", 1))}
    r["q_lo"] = first_q + nq[cs] if fwd else last_q - nq[ce + 1]
    r["q_hi"] = r["q_lo"] + nq[ce + 1] - nq[cs]
    r["off_lo"] = lo - beg[w]; r["off_hi"] = hi - beg[w]
    return w, r


@pytest.mark.parametrize("name,params,maf", FIXTURES)
def test_host_regions_give_what_the_reference_maf_implies(oracle_built, golden_dir, name, params, maf):
    """every region of the set, every contig: hostlib.lift_regions == the columns of the reference's MAF under the choice rule; block by block == the host CIGARs;
    and == the point lift of the same result at the span's two ends"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    G = int(idx.G)
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    chr_start = {n: int(s) for n, s in zip(idx.chr_names, starts)}
    blocks = pm.maf_blocks(os.path.join(golden_dir, maf))
    o = oracle_built.Oracle(idx, params)
    at = 0
    seen = {k: 0 for k in KINDS}
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True)
        nb = int(d["b_score"].size)
        mine = blocks[at:at + nb]; at += nb
        beg, end = region_set(idx, d)
        H = hostlib.lift_regions(px, seq, d, beg, end)
        assert H.dtype == capi.REGION_HIT_DT
        got = rm.dense(H, beg.size)
        want = rm.contig_regions(mine, chr_start, d["b_bdup"], d["b_score"], beg, end)
        for k in rm.FIELDS:
            g, w = got[k], want[k]
            assert np.array_equal(g, w), (k, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])
        for k, v in kinds_of(d, G, H, beg, end, want["by_overlap"][H["idx"]]).items():
            seen[k] += v
        if nb == 0:
            assert H.size == 0
            continue
        # the sums the contract states
        assert np.array_equal(H["n_eq"].astype(np.int64) + H["n_x"] + H["n_del"], H["off_hi"].astype(np.int64) - H["off_lo"])
        assert np.array_equal(H["n_eq"].astype(np.int64) + H["n_x"] + H["n_ins"], H["q_hi"].astype(np.int64) - H["q_lo"])
        # consistency with the point lift: regions of length 1 are gsa_lift's hits
        one = np.flatnonzero(end - beg == 1)
        L = hostlib.lift(px, seq, d, beg[one])
        H1 = H[np.isin(H["idx"], one)]
        assert np.array_equal(one[L["idx"]], H1["idx"]) and np.array_equal(L["block"], H1["block"]) and np.array_equal(L["n_cover"], H1["n_cover"]) and np.array_equal(L["rev"], H1["rev"])
        # ... and the two end columns of every span, lifted within the chosen block (a result that holds that block alone), give q_lo and q_hi
        f_at = np.concatenate([[0], np.cumsum(d["b_nfrag"])]); a_at = np.concatenate([[0], np.cumsum(d["f_alnlen"])])
        cblk, cops = hostlib.cigars(px, seq, d)
        for bi in range(nb):
            fs = slice(int(f_at[bi]), int(f_at[bi + 1]))
            alone = {k: v[bi:bi + 1] for k, v in d.items() if k.startswith("b_")}
            alone.update({k: v[fs] for k, v in d.items() if k.startswith("f_")})
            alone["aln1"] = d["aln1"][int(a_at[fs.start]):int(a_at[fs.stop])]; alone["aln2"] = d["aln2"][int(a_at[fs.start]):int(a_at[fs.stop])]
            Hb = H[H["block"] == bi]
            if Hb.size:
                p_lo = beg[Hb["idx"]] + Hb["off_lo"]; p_hi = beg[Hb["idx"]] + Hb["off_hi"]
                first, last = (p_lo, p_hi - 1) if d["b_bdir"][bi] else (p_hi - 1, p_lo)      # the span's first and last column in WALK order
                La = hostlib.lift(px, seq, alone, first); Lz = hostlib.lift(px, seq, alone, last)
                assert La.size == Hb.size == Lz.size
                assert np.array_equal(Hb["q_lo"], La["qpos"] + (La["cls"] == 2))
                assert np.array_equal(Hb["q_hi"], Lz["qpos"] + 1)      # (= / X: behind the base it faces; D: behind the base consumed last in front)
            # the second derivation, without the MAF: the block's own CIGAR
            w, r = cigar_regions(d, cblk, cops, bi, starts, G, beg, end)
            Ha = hostlib.lift_regions(px, seq, alone, beg, end)
            assert np.array_equal(Ha["idx"], w) and (Ha["block"] == 0).all() and (Ha["n_cover"] == 1).all() and (Ha["rev"] == (0 if d["b_bdir"][bi] else 1)).all(), bi
            for k, v in r.items():
                assert np.array_equal(Ha[k].astype(np.int64), v), (bi, k)
    o.close()
    assert at == len(blocks)
    # the coverage this test (and the GPU test, on the same sets) stands on
    assert_kinds(name, seen)


def test_regions_stop_at_the_end_of_the_reference_sequence(overrun_case):
    """the hand-made result whose blocks run past the end of their reference sequences (G = 700): regions across the trimmed ends, the choice between overlapping
    blocks (overlap before score), the reverse pair, the duplicate, the neighbours of an inserted pair, and regions the call refuses"""
    px, qfa, qry, dump = overrun_case
    idx = indexio.load_index(px)
    G = int(idx.G)
    assert G == 700

    def lift(d, regs):
        b = np.array([r[0] for r in regs], np.int64); e = np.array([r[1] for r in regs], np.int64)
        return hostlib.lift_regions(px, qry, d, b, e)

    # block 0: forward on chrA [300, 405) untrimmed -> [300, 400); block 1: [340, 406) -> [340, 400); block 5: [10, 64)
    # blocks 2 and 3: reverse strand of chrB -> forward positions [400, 500) / [400, 470); block 4 (a duplicate): forward on chrB [650, 702) -> [650, 700)
    sc = dump["b_score"]
    assert sc[0] > sc[1]
    H = lift(dump, [(390, 400), (250, 400), (0, 400), (330, 360), (340, 400), (360, 400)])
    assert H["idx"].tolist() == [0, 1, 2, 3, 4, 5]
    # across the trimmed end of chrA: block 0's seed [355, 405) answers up to 400 and no further
    assert (H["block"][:2] == 0).all() and H["off_lo"].tolist()[:3] == [0, 50, 300] and H["off_hi"].tolist()[:3] == [10, 150, 400] and H["n_cover"].tolist()[:3] == [2, 2, 3]
    assert H["q_lo"][0] == 66 + 35 and H["q_hi"][0] == 66 + 45 and H["n_eq"][0] == 10
    assert H["n_eq"][1] + H["n_x"][1] + H["n_del"][1] == 100 and H["q_lo"][1] == 10
    # [330, 360): block 0 covers all 30 bases, block 1 only 20 -- and [340, 400), [360, 400): equal overlap, the score decides
    assert H["block"][3] == 0 and H["block"][4] == 0 and H["block"][5] == 0 and (H["n_cover"][3:] == 2).all()
    # the same with the scores swapped: [330, 360) still goes to block 0, AGAINST the score; the equal overlaps now go to block 1
    swapped = {k: v.copy() for k, v in dump.items()}
    swapped["b_score"][0], swapped["b_score"][1] = sc[1], sc[0]
    S = lift(swapped, [(330, 360), (340, 400), (360, 400), (339, 400)])
    assert S["block"].tolist() == [0, 1, 1, 0] and S["off_lo"].tolist() == [0, 0, 0, 0] and S["off_hi"].tolist() == [30, 60, 40, 61]
    assert S["q_lo"][1] == 200 and S["q_lo"][0] == 10 + 30
    # the reverse pair: forward [400, 500) is block 2's text [G + 200, G + 300); [400, 470) block 3's too.  A region over both, one over block 2 alone, one across
    # the sequence start 400 is refused by the device call and split here by hand
    R = lift(dump, [(400, 500), (470, 500), (400, 401), (499, 500), (440, 480)])
    assert (R["block"] == 2).all() and (R["rev"] == 1).all() and R["n_cover"].tolist() == [2, 1, 2, 1, 2]
    assert R["off_lo"].tolist() == [0, 0, 0, 0, 0] and R["off_hi"].tolist() == [100, 30, 1, 1, 40]
    assert R["q_lo"][3] == 400 and R["q_hi"][3] == 401 and R["n_eq"][3] == 1      # text G + 200: the first base of block 2's first seed
    assert R["q_lo"][0] == 400 and R["q_lo"][1] == 400 and R["q_hi"][1] == 430
    for h in R:
        assert int(h["n_eq"]) + int(h["n_x"]) + int(h["n_del"]) == h["off_hi"] - h["off_lo"] and int(h["n_eq"]) + int(h["n_x"]) + int(h["n_ins"]) == h["q_hi"] - h["q_lo"]
    # the duplicate answers where it is alone, trimmed at 700, and loses to any block that is not one
    D = lift(dump, [(640, 700), (690, 700)])
    assert (D["block"] == 4).all() and D["off_lo"].tolist() == [10, 0] and D["off_hi"].tolist() == [60, 10] and (D["n_cover"] == 1).all() and D["q_lo"].tolist() == [800, 840]
    dup0 = {k: v.copy() for k, v in dump.items()}
    dup0["b_bdup"][:] = [1, 0, 0, 0, 1, 0]
    assert lift(dup0, [(330, 360)])["block"].tolist() == [1]      # (20 bases of a block that is no duplicate before 30 of one that is)
    # block 5: seed [10, 40) at query 900, gap "IIMM": reference 40 and 41 face '-', 42 and 43 face query 930 and 931, then the seed [44, 64) at 932
    I = lift(dump, [(40, 42), (40, 41), (41, 42), (39, 42), (41, 43), (38, 46), (42, 44), (0, 100)])
    assert (I["block"] == 5).all()
    assert I["n_del"].tolist() == [2, 1, 1, 2, 1, 2, 0, 2] and I["n_ins"].tolist() == [0] * 8
    assert I["q_lo"].tolist() == [930, 930, 930, 929, 930, 928, 930, 900] and I["q_hi"].tolist() == [930, 930, 930, 930, 931, 934, 932, 952]
    assert I["off_lo"][7] == 10 and I["off_hi"][7] == 64
    # block 0's gap "MMDDMIM" behind the seed [300, 350) at query 10: columns 350 351 - - 352 353(D) 354; the inserted pair 62, 63 lies strictly inside [351, 353) only
    J = lift(dump, [(351, 352), (351, 353), (352, 353), (350, 355), (353, 354), (300, 305)])
    assert (J["block"] == 0).all() and J["n_ins"].tolist() == [0, 2, 0, 2, 0, 0] and J["n_del"].tolist() == [0, 0, 0, 1, 1, 0]
    assert J["q_lo"].tolist() == [61, 61, 64, 60, 65, 10] and J["q_hi"].tolist() == [62, 65, 65, 66, 65, 15]
    # regions no block overlaps, and what the host comparator leaves out (the device call refuses them): empty, reversed, outside [0, G), across a sequence boundary
    N = lift(dump, [(100, 200), (64, 300), (300, 300), (305, 300), (-5, 10), (690, 701), (390, 410), (399, 401), (10, 11)])
    assert N["idx"].tolist() == [8]      # ((390, 410) and (399, 401) cross the boundary between chrA and chrB at 400)
    assert lift(dump, []).size == 0
    assert hostlib.lift_regions(px, qry, {k: v[:0] for k, v in dump.items()}, np.array([0], np.int64), np.array([700], np.int64)).size == 0


def test_regions_tsv_of_the_golden_maf_is_well_formed(golden_dir):
    """regions_from_maf.regions_tsv (what the CLI test compares with): one line per overlapped region and contig, intervals inside their sequences"""
    idx = indexio.load_index(os.path.join(golden_dir, "small"))
    beg, end = rm.stride_regions(idx.chr_len, lengths=(1, 65, 1000), stride=97)
    txt = rm.regions_tsv(os.path.join(golden_dir, "small.maf"), idx.chr_names, idx.chr_len, beg, end)
    lines = txt.split("\n")
    assert lines[0] + "\n" == rm.HEADER and lines[-1] == "" and len(lines) > 500
    qlen = {n: s.size for n, s in synth.read_fasta(os.path.join(golden_dir, "small.qry.fa"))}
    clen = dict(zip(idx.chr_names, idx.chr_len.tolist()))
    for ln in lines[1:-1]:
        f = ln.split("\t")
        v = [int(x) for x in f[1:3] + f[4:6] + f[7:9] + f[10:]]
        assert len(f) == 16 and 0 <= v[0] <= v[2] < v[3] <= v[1] <= clen[f[0]] and 0 <= v[4] <= v[5] <= qlen[f[6]] and f[9] in "+-"
        assert v[6] + v[7] + v[8] == v[3] - v[2] and v[6] + v[7] + v[9] == v[5] - v[4] and v[11] >= 1
