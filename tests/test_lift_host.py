"""CPU tests of lifting reference positions through an alignment (gsa_lift_hit / gsa_lifts, include/gsa_hip.h): the record layout, and the host walk gsah_c_lift
-- the comparator of the GPU pass -- pinned, for EVERY reference position, to the REFERENCE's own MAF files through the oracle's finished blocks, to the host CIGARs of
the same blocks, and to the iExtension trim on a hand-made result that runs past the end of its reference sequences (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lift_from_maf as lm
import paf_from_maf as pm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import overrun_case      # noqa: F401  (fixture)


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_lift_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_lift_hit); }\nint sz2(void) { return (int)sizeof(gsa_lifts); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'int o1(void) { return (int)offsetof(gsa_lift_hit, cls); }\nint o2(void) { return (int)offsetof(gsa_lift_hit, n_cover); }\nunsigned w(void) { return GSA_WANT_LIFT; }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 16 == capi.LIFT_HIT_DT.itemsize == C.sizeof(capi.LiftHit)
    assert x.sz2() == 16 == C.sizeof(capi.Lifts) and x.sz3() == 16
    assert x.o1() == 12 == capi.LIFT_HIT_DT.fields["cls"][1] and x.o2() == 14 == capi.LIFT_HIT_DT.fields["n_cover"][1]
    assert x.w() == 16 == capi.WANT_LIFT


def dense(H, n):
    """hits -> arrays over the n input positions (cls 0: no hit)"""
    assert H.dtype == capi.LIFT_HIT_DT
    assert (np.diff(H["idx"]) > 0).all() and (H.size == 0 or (H["idx"][0] >= 0 and H["idx"][-1] < n)) and (H["cls"] != 0).all()
    qpos = np.full(n, -1, np.int32); cls = np.zeros(n, np.uint8); rev = np.zeros(n, np.uint8); blk = np.full(n, -1, np.int32); ncov = np.zeros(n, np.uint16)
    i = H["idx"]
    qpos[i] = H["qpos"]; cls[i] = H["cls"]; rev[i] = H["rev"]; blk[i] = H["block"]; ncov[i] = H["n_cover"]
    return qpos, cls, rev, blk, ncov


def cigar_lift(d, ops_blk, ops, bi, G):
    """Second oracle, no MAF: from the host CIGAR ops of block bi (output order: reference-forward) prefix sums give every reference base's class and query position.
    Returns (text positions covered by the UNTRIMMED block, ascending in reference-forward order; qpos; cls)."""
    f0 = int(np.concatenate([[0], np.cumsum(d["b_nfrag"])])[bi]); nf = int(d["b_nfrag"][bi])
    o = ops[int(ops_blk["cig_off"][bi]):int(ops_blk["cig_off"][bi]) + int(ops_blk["n_cig"][bi])]
    cls = np.repeat((o & 15).astype(np.uint8), (o >> 4).astype(np.int64))
    rc = cls != 1; qc = cls != 2
    cols = np.flatnonzero(rc)
    nq = np.cumsum(qc) - qc
    first_r, first_q = int(d["f_rpos"][f0]), int(d["f_qpos"][f0])
    last_r = int(d["f_rpos"][f0 + nf - 1]) + int(d["f_rlen"][f0 + nf - 1]); last_q = int(d["f_qpos"][f0 + nf - 1]) + int(d["f_qlen"][f0 + nf - 1])
    if d["b_bdir"][bi]:
        t = first_r + np.arange(cols.size, dtype=np.int64)
        q = first_q + nq[cols] - (~qc[cols]).astype(np.int64)
    else:      # the ops run against the walk: the first column is the walk's last
        t = last_r - 1 - np.arange(cols.size, dtype=np.int64)
        q = last_q - 1 - nq[cols]      # (a D column too: the base printed next behind it is the one the walk consumed last)
    assert t.size == last_r - first_r
    return t, q.astype(np.int32), cls[cols]


@pytest.mark.parametrize("name,params,maf", [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")])
def test_host_lift_gives_what_the_reference_maf_implies(oracle_built, golden_dir, name, params, maf):
    """every reference position, every contig: hostlib.lift == the columns of the reference's MAF under the choice rule; and, block by block, == the host CIGARs"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    G = int(idx.G)
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    chr_start = {n: int(s) for n, s in zip(idx.chr_names, starts)}
    blocks = pm.maf_blocks(os.path.join(golden_dir, maf))
    allpos = np.arange(G, dtype=np.int64)
    o = oracle_built.Oracle(idx, params)
    at = 0
    seen_cls, n_rev, n_multi, n_none, n_hits = set(), 0, 0, 0, 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True)
        nb = int(d["b_score"].size)
        mine = blocks[at:at + nb]; at += nb
        H = hostlib.lift(px, seq, d, allpos)
        got = dense(H, G)
        want = lm.contig_lifts(mine, chr_start, G, d["b_bdup"], d["b_score"])
        for g, w, what in zip(got, want, ("qpos", "cls", "rev", "block", "n_cover")):
            assert np.array_equal(g, w), (what, np.flatnonzero(g != w)[:5], g[g != w][:5], w[g != w][:5])
        seen_cls |= set(H["cls"].tolist()); n_rev += int(H["rev"].sum()); n_multi += int((H["n_cover"] > 1).sum()); n_none += G - H.size; n_hits += H.size
        # the second oracle: the block's own CIGAR.  hostlib.lift restricted to block bi (a result that holds this block alone) must agree with it
        cblk, cops = hostlib.cigars(px, seq, d)
        f_at = np.concatenate([[0], np.cumsum(d["b_nfrag"])])
        a_at = np.concatenate([[0], np.cumsum(d["f_alnlen"])])
        for bi in range(nb):
            fs = slice(int(f_at[bi]), int(f_at[bi + 1]))
            one = {k: v[bi:bi + 1] for k, v in d.items() if k.startswith("b_")}
            one.update({k: v[fs] for k, v in d.items() if k.startswith("f_")})
            one["aln1"] = d["aln1"][int(a_at[fs.start]):int(a_at[fs.stop])]; one["aln2"] = d["aln2"][int(a_at[fs.start]):int(a_at[fs.stop])]
            t, q, c = cigar_lift(d, cblk, cops, bi, G)
            p = t if d["b_bdir"][bi] else 2 * G - 1 - t
            lim = starts[int(d["b_chr"][bi]) + 1]      # (a block that runs over the end of its sequence: the trim)
            keep = (p < lim) if d["b_bdir"][bi] else (p >= starts[int(d["b_chr"][bi])])
            Hb = hostlib.lift(px, seq, one, p[keep])
            assert Hb.size == int(keep.sum()) and np.array_equal(Hb["idx"], np.arange(Hb.size)), bi
            assert np.array_equal(Hb["qpos"], q[keep]) and np.array_equal(Hb["cls"], c[keep]) and (Hb["rev"] == (0 if d["b_bdir"][bi] else 1)).all() and (Hb["n_cover"] == 1).all(), bi
    o.close()
    assert at == len(blocks)
    # the coverage this test stands on
    assert n_hits > 1000 and n_rev > 0 and n_none > 0 and seen_cls == {2, 7, 8}, (n_hits, n_rev, n_none, seen_cls)
    if name == "cx":
        assert n_multi > 0


def test_lift_stops_at_the_end_of_the_reference_sequence(overrun_case):
    """the hand-made result whose blocks run past the end of their reference sequences: no hit beyond that end, the choice rule between overlapping blocks, and
    positions outside the reference"""
    px, qfa, qry, dump = overrun_case
    idx = indexio.load_index(px)
    G = int(idx.G)
    assert G == 700
    allpos = np.arange(G, dtype=np.int64)
    H = hostlib.lift(px, qry, dump, allpos)
    qpos, cls, rev, blk, ncov = dense(H, G)
    # block 0: forward on chrA [300, 405) untrimmed -> [300, 400); block 1: [340, 406) -> [340, 400); block 5: [10, 64)
    # blocks 2 and 3: reverse strand of chrB, text [G + 200, G + 304) and [G + 230, G + 307) -> trimmed at G + 300, i.e. forward positions 2G - 1 - t in [400, 500) / [400, 470)
    # block 4 (a duplicate): forward on chrB [650, 702) -> [650, 700)
    assert set(np.flatnonzero(cls).tolist()) == set(range(10, 64)) | set(range(300, 500)) | set(range(650, 700))
    assert (blk[300:340] == 0).all() and (ncov[300:340] == 1).all() and (ncov[340:400] == 2).all()
    sc = dump["b_score"]
    assert (blk[340:400] == (0 if sc[0] >= sc[1] else 1)).all()
    assert (blk[400:500] == 2).all() and (ncov[400:470] == 2).all() and (ncov[470:500] == 1).all() and (rev[400:500] == 1).all() and (rev[:400] == 0).all()
    assert (blk[650:700] == 4).all() and (blk[10:64] == 5).all()
    # a seed column: the position's own offset into the seed
    assert cls[300] == 7 and qpos[300] == 10 and cls[349] == 7 and qpos[349] == 59
    assert qpos[399] == 66 + (399 - 355) and cls[399] == 7
    # block 5's gap is "IIMM" behind the seed [10, 40): reference bases 40 and 41 face '-' (the last query base in front: 929), 42 and 43 face query 930 and 931
    assert cls[40] == 2 and cls[41] == 2 and qpos[40] == 929 and qpos[41] == 929 and qpos[42] == 930 and qpos[43] == 931 and qpos[44] == 932
    # reverse strand: text position G + 200 is forward position 2G - 1 - (G + 200) = 499 and faces query 400, as stored
    assert qpos[499] == 400 and cls[499] == 7 and qpos[440] == 400 + 59
    # positions outside [0, G) have no hit on the host (the device call refuses them), repeated positions answer per idx
    H2 = hostlib.lift(px, qry, dump, np.array([-1, 300, G, 300, 5, 2 * G], np.int64))
    assert H2["idx"].tolist() == [1, 3] and H2["qpos"].tolist() == [10, 10]
    # no positions, no blocks
    assert hostlib.lift(px, qry, dump, np.zeros(0, np.int64)).size == 0
    empty = {k: v[:0] for k, v in dump.items()}
    assert hostlib.lift(px, qry, empty, allpos).size == 0


def test_lift_tsv_of_the_golden_maf_is_well_formed(golden_dir):
    """lift_from_maf.lift_tsv (what the CLI test compares with): one line per covered position and contig, 1-based columns inside their sequences"""
    idx = indexio.load_index(os.path.join(golden_dir, "small"))
    txt = lm.lift_tsv(os.path.join(golden_dir, "small.maf"), idx.chr_names, idx.chr_len)
    lines = txt.split("\n")
    assert lines[0].startswith("#") and lines[-1] == "" and len(lines) > 1000
    qlen = {n: s.size for n, s in synth.read_fasta(os.path.join(golden_dir, "small.qry.fa"))}
    clen = dict(zip(idx.chr_names, idx.chr_len.tolist()))
    for ln in lines[1:-1]:
        f = ln.split("\t")
        assert len(f) == 8 and 1 <= int(f[1]) <= clen[f[0]] and 1 <= int(f[3]) <= qlen[f[2]] and f[4] in "+-" and f[5] in "=XD" and int(f[7]) >= 1
