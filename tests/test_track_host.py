"""CPU tests of the per-window reference track (gsa_track_win / gsa_tracks, include/gsa_hip.h): the record layout, and the host walk gsah_c_track -- the comparator of
the GPU pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, to the host lift of every position at W = 1, to itself across window
lengths, and to the trim on a hand-made result that runs past the end of its reference sequences (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import track_from_maf as tm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import overrun_case      # noqa: F401  (fixture)

FIELDS = ("n_cov", "n_eq", "n_x", "n_del", "n_ins")


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_track_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_track_win); }\nint sz2(void) { return (int)sizeof(gsa_tracks); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'int o1(void) { return (int)offsetof(gsa_track_win, len); }\nint o2(void) { return (int)offsetof(gsa_track_win, n_cov); }\nint o3(void) { return (int)offsetof(gsa_track_win, n_ins); }\n'
                   'int o4(void) { return (int)offsetof(gsa_tracks, win); }\nunsigned w(void) { return GSA_WANT_TRACK; }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 32 == capi.TRACK_WIN_DT.itemsize == C.sizeof(capi.TrackWin) == tm.TRACK_DT.itemsize
    assert x.sz2() == 16 == C.sizeof(capi.Tracks) and x.sz3() == 16
    assert x.o1() == 8 == capi.TRACK_WIN_DT.fields["len"][1] and x.o2() == 12 == capi.TRACK_WIN_DT.fields["n_cov"][1] and x.o3() == 28 == capi.TRACK_WIN_DT.fields["n_ins"][1]
    assert x.o4() == 8
    assert x.w() == 32 == capi.WANT_TRACK
    assert capi.TRACK_WIN_DT == tm.TRACK_DT


def well_formed(T, idx, W):
    assert T.dtype == capi.TRACK_WIN_DT
    key = T["chr"].astype(np.int64) << 32 | T["start"]
    assert (np.diff(key) > 0).all() and (T["n_cov"] > 0).all() and (T["n_cov"] <= T["len"]).all()
    L = np.asarray(idx.chr_len, np.int64)[T["chr"]]
    assert (T["start"] % W == 0).all() and (T["start"] >= 0).all() and np.array_equal(T["len"], np.minimum(T["start"].astype(np.int64) + W, L) - T["start"])
    assert (T["n_eq"].astype(np.int64) + T["n_x"] + T["n_del"] >= T["n_cov"]).all()      # (every covered base lies in a column of some counted block)


def same(a, b, what=""):
    assert a.size == b.size, (what, a.size, b.size)
    for f in capi.TRACK_WIN_DT.names:
        assert np.array_equal(a[f], b[f]), (what, f, np.flatnonzero(a[f] != b[f])[:5], a[a[f] != b[f]][:3], b[a[f] != b[f]][:3])


@pytest.fixture(scope="module")
def golden_results(oracle_built, golden_dir):
    """(prefix, index, [(query name, sequence, finished blocks of the oracle, the MAF's blocks of that contig)]) per golden case, computed once"""
    import paf_from_maf as pm
    out = {}
    for key, name, params, maf in (("cx", "cx", {}, "cx.maf"), ("cx_sen", "cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", "small", {}, "small.maf")):
        px = os.path.join(golden_dir, name)
        idx = indexio.load_index(px)
        blocks = pm.maf_blocks(os.path.join(golden_dir, maf))
        o = oracle_built.Oracle(idx, params)
        at, res = 0, []
        for qn, seq in synth.read_fasta(px + ".qry.fa"):
            o.set_query(seq); o.run_to(8)
            d = o.blocks(with_aln=True)
            nb = int(d["b_score"].size)
            res.append((qn, seq, d, blocks[at:at + nb])); at += nb
        o.close()
        assert at == len(blocks)
        out[key] = (px, idx, res)
    return out


@pytest.mark.parametrize("key", ["cx", "cx_sen", "small"])
def test_host_track_gives_what_the_reference_maf_implies(golden_results, key):
    """every contig, every field, W in {1, 64, 1000, 2^30}: hostlib.track == the columns of the reference's MAF"""
    px, idx, res = golden_results[key]
    seen = dict(ins=0, dele=0, x=0, deep=0, rev=0, holes=0, dup=0)
    for W in (1, 64, 1000, 1 << 30):
        total = sum((int(L) + W - 1) // W for L in idx.chr_len)
        for qn, seq, d, mine in res:
            T = hostlib.track(px, seq, d, W)
            well_formed(T, idx, W)
            # (the MAF prints a duplicate with score 1: the same set as bdup != 0)
            assert [b[0] == 1 for b in mine] == [bool(x) for x in d["b_bdup"]]
            same(T, tm.contig_track(mine, idx.chr_names, idx.chr_len, W), (key, qn, W))
            depth = T["n_eq"].astype(np.int64) + T["n_x"] + T["n_del"]
            seen["ins"] += int((T["n_ins"] > 0).sum()); seen["dele"] += int((T["n_del"] > 0).sum()); seen["x"] += int((T["n_x"] > 0).sum())
            seen["deep"] += int((depth > T["n_cov"]).sum()); seen["holes"] += total - T.size
            seen["rev"] += sum(1 for b in mine if b[0] != 1 and b[2][3] == "-")
            # the reference's golden runs hold no duplicate block: the contig's first block marked as one (what OutputMAF would print with score 1) leaves the track
            if len(mine) > 0:
                d2 = dict(d); d2["b_bdup"] = d["b_bdup"].copy(); d2["b_bdup"][0] = 1
                T2 = hostlib.track(px, seq, d2, W)
                same(T2, tm.contig_track(mine, idx.chr_names, idx.chr_len, W, score=[1] + [b[0] for b in mine[1:]]), (key, qn, W, "dup"))
                assert int(T2["n_eq"].sum()) < int(T["n_eq"].sum())
                seen["dup"] += 1
    # the ground this test stands on
    assert seen["ins"] > 0 and seen["dele"] > 0 and seen["x"] > 0 and seen["holes"] > 0, seen
    assert seen["dup"] > 0, seen
    if key != "small":
        assert seen["deep"] > 0 and seen["rev"] > 0, seen


def test_track_at_one_base_is_the_lift_of_every_position(golden_results):
    """W = 1 against hostlib.lift: n_cov == 1 exactly at the positions whose chosen block is no duplicate (a counted block that covers a position beats every duplicate);
    where exactly one counted block covers the position, the one-hot of (n_eq, n_x, n_del) is the hit's class"""
    px, idx, res = golden_results["cx"]
    G = int(idx.G)
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    allpos = np.arange(G, dtype=np.int64)
    n_single = 0
    for qn, seq, d, _ in res:
        T = hostlib.track(px, seq, d, 1)
        H = hostlib.lift(px, seq, d, allpos)
        assert (T["len"] == 1).all() and (T["n_cov"] == 1).all()
        p = starts[T["chr"]] + T["start"]
        counted = H[d["b_bdup"][H["block"]] == 0]
        assert np.array_equal(p, counted["idx"])
        depth = T["n_eq"].astype(np.int64) + T["n_x"] + T["n_del"]
        one = depth == 1
        cls = np.where(T["n_eq"] == 1, 7, np.where(T["n_x"] == 1, 8, 2))
        assert np.array_equal(cls[one], counted["cls"][one])
        n_single += int(one.sum())
    assert n_single > 1000


@pytest.mark.parametrize("W", [1, 50, 1000])
def test_track_nests(golden_results, W):
    """windows restart per sequence, so window j at 2W is windows 2j and 2j + 1 at W: all five fields add up"""
    for key in ("cx", "small"):
        px, idx, res = golden_results[key]
        for qn, seq, d, _ in res:
            A, B = hostlib.track(px, seq, d, W), hostlib.track(px, seq, d, 2 * W)
            k = (A["chr"].astype(np.int64) << 32) | (A["start"] // (2 * W) * (2 * W))
            u, inv = np.unique(k, return_inverse=True)
            assert np.array_equal(u, (B["chr"].astype(np.int64) << 32) | B["start"]), (key, qn)
            for f in FIELDS:
                assert np.array_equal(np.bincount(inv, weights=A[f].astype(np.float64), minlength=u.size).astype(np.int64), B[f].astype(np.int64)), (key, qn, f)


def test_track_stops_at_the_end_of_the_reference_sequence(overrun_case):
    """the hand-made result whose blocks run past the end of their reference sequences: no window beyond a sequence's end, the duplicate contributes nothing"""
    px, qfa, qry, dump = overrun_case
    idx = indexio.load_index(px)
    assert int(idx.G) == 700 and idx.chr_len.tolist() == [400, 300]
    # block 0: forward on chrA [300, 405) untrimmed -> [300, 400); block 1: [340, 406) -> [340, 400); block 5: [10, 64)
    # blocks 2 and 3: reverse strand of chrB, trimmed to the forward positions [400, 500) / [400, 470), i.e. [0, 100) / [0, 70) inside chrB
    # block 4 (a duplicate): forward on chrB [250, 302) inside the sequence: not counted
    T1 = hostlib.track(px, qry, dump, 1)
    well_formed(T1, idx, 1)
    a, b = T1[T1["chr"] == 0], T1[T1["chr"] == 1]
    assert a["start"].tolist() == list(range(10, 64)) + list(range(300, 400)) and b["start"].tolist() == list(range(100))
    depth = T1["n_eq"].astype(np.int64) + T1["n_x"] + T1["n_del"]
    da, db = depth[T1["chr"] == 0], depth[T1["chr"] == 1]
    assert (da[:54 + 40] == 1).all() and (da[54 + 40:] == 2).all() and (db[:70] == 2).all() and (db[70:] == 1).all()
    # block 5's gap is "IIMM" behind the seed [10, 40): reference bases 40 and 41 face '-'
    assert a["n_del"][30:32].tolist() == [1, 1] and a["n_del"][:30].sum() == 0
    for W in (7, 100, 1000):
        T = hostlib.track(px, qry, dump, W)
        well_formed(T, idx, W)
        assert (T["start"].astype(np.int64) + T["len"] <= np.asarray(idx.chr_len)[T["chr"]]).all()
        for c, cov, dep in ((0, 54 + 100, 54 + 100 + 60), (1, 100, 100 + 70)):
            t = T[T["chr"] == c]
            assert int(t["n_cov"].sum()) == cov and int(t["n_eq"].sum()) + int(t["n_x"].sum()) + int(t["n_del"].sum()) == dep, (W, c)
        for f in FIELDS[1:]:
            assert int(T[f].sum()) == int(T1[f].sum()), (W, f)
    # the duplicate alone, and no block at all: n_win = 0
    nf = np.concatenate([[0], np.cumsum(dump["b_nfrag"])])
    only = {k: v[4:5] for k, v in dump.items() if k.startswith("b_")}
    only.update({k: v[int(nf[4]):int(nf[5])] for k, v in dump.items() if k.startswith("f_")})
    only["aln1"] = dump["aln1"][:0]; only["aln2"] = dump["aln2"][:0]
    assert hostlib.track(px, qry, only, 10).size == 0
    assert hostlib.track(px, qry, {k: v[:0] for k, v in dump.items()}, 10).size == 0


def test_track_tsv_of_the_golden_maf_is_well_formed(golden_dir):
    """track_from_maf.track_tsv (what the CLI test compares with): one line per query contig and covered window, BED-style coordinates inside the sequences"""
    idx = indexio.load_index(os.path.join(golden_dir, "small"))
    txt = tm.track_tsv(os.path.join(golden_dir, "small.maf"), idx.chr_names, idx.chr_len, 100)
    lines = txt.split("\n")
    assert lines[0] == "#ref\tstart\tend\tquery\tcovered\tmatch\tmismatch\tdeleted\tinserted" and lines[-1] == "" and len(lines) > 10
    clen = dict(zip(idx.chr_names, idx.chr_len.tolist()))
    qnames = {n for n, _ in synth.read_fasta(os.path.join(golden_dir, "small.qry.fa"))}
    for ln in lines[1:-1]:
        f = ln.split("\t")
        assert len(f) == 9 and f[3] in qnames and int(f[1]) % 100 == 0 and int(f[1]) < int(f[2]) == min(int(f[1]) + 100, clen[f[0]])
        assert 1 <= int(f[4]) <= int(f[2]) - int(f[1]) and int(f[5]) + int(f[6]) + int(f[7]) >= int(f[4])
