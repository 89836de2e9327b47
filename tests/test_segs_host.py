"""CPU tests of the per-block chain segments (gsa_seg / gsa_seg_block / gsa_segs, include/gsa_hip.h): the record layout, the host walk gsah_c_segs -- the comparator
of the GPU pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, the iExtension trim on triples, the chain emitter, and the agreement
of the triples with the lifted positions of hostlib.lift (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_from_maf as chm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import gapped


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_segs_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_seg); }\nint sz1(void) { return (int)sizeof(gsa_seg_block); }\nint sz2(void) { return (int)sizeof(gsa_segs); }\n'
                   'int sz3(void) { return (int)sizeof(gsa_extras); }\nint want(void) { return (int)GSA_WANT_SEGS; }\n'
                   'int fn(void) { return (int)sizeof(gsa_block_segs((gsa_ctx *)0, 0, (gsa_segs *)0)) + (int)sizeof(gsa_extras_segs((const gsa_extras *)0, (gsa_segs *)0))'
                   ' + (int)sizeof(gsa_get_seg_timing((gsa_ctx *)0, (double *)0, (int64_t *)0)); }\n')      # (unevaluated: the functions' C declarations)
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 12 == capi.SEG_DT.itemsize == C.sizeof(capi.Seg)
    assert x.sz1() == 16 == capi.SEG_BLOCK_DT.itemsize == C.sizeof(capi.SegBlock)
    assert x.sz2() == C.sizeof(capi.Segs) == 32 and x.sz3() == C.sizeof(capi.Extras) == 16
    assert x.want() == capi.WANT_SEGS == 64 and x.fn() == 12
    assert {"gsa_block_segs", "gsa_get_seg_timing", "gsa_extras_segs"} <= set(capi.EXPORTS)


# blocks, reverse-strand blocks, segments, gaps with only dt, gaps with only dq, longest segment, one-segment blocks of the golden MAF files (derived from the
# files with chain_from_maf)
GOLDEN_SEG_SHAPE = {"cx.maf": (22, 1, 2834, 1379, 1433, 2480, 1), "small.maf": (2, 1, 372, 180, 190, 986)}


def golden_seg_shape(golden_dir, maf):
    blocks = chm.maf_blocks(os.path.join(golden_dir, maf))
    tr = [chm.block_triples(b[1], b[2])[0] for b in blocks]
    gaps = [(dt, dq) for t in tr for _, dt, dq in t[:-1]]
    return (len(blocks), sum(1 for b in blocks if b[2][3] == "-"), sum(len(t) for t in tr), sum(1 for dt, dq in gaps if dt and not dq), sum(1 for dt, dq in gaps if dq and not dt),
            max(s for t in tr for s, _, _ in t), sum(1 for t in tr if len(t) == 1))


def test_golden_coverage(golden_dir):
    """what the parity tests stand on -- and what they do not hold: no golden block has a gap with both sides, none starts or ends in a gap column (the hand-made
    inputs below bring those)"""
    for maf, want in GOLDEN_SEG_SHAPE.items():
        assert golden_seg_shape(golden_dir, maf)[:len(want)] == want, maf
        for _, ref, qry in chm.maf_blocks(os.path.join(golden_dir, maf)):
            tr, ld, li, td, ti = chm.triples_of_kinds(chm.column_kinds(ref[5], qry[5]))
            assert (ld, li, td, ti) == (0, 0, 0, 0)
            assert all((dt == 0) != (dq == 0) for _, dt, dq in tr[:-1]) and tr[-1][1:] == (0, 0)


def block_cols(sg):
    return int(sg["size"].sum()) + int(sg["dt"].sum()) + int(sg["dq"].sum())


def as_tuples(sg):
    return [(int(s), int(a), int(b)) for s, a, b in zip(sg["size"], sg["dt"], sg["dq"])]


@pytest.mark.parametrize("name,params,maf", [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")])
def test_host_segs_give_the_reference_maf_columns(oracle_built, golden_dir, tmp_path, name, params, maf):
    """comparator triples -> trimmed == the triples derived here from the two `s` lines of every block of the reference's MAF; and the whole chain file the emitter
    writes == the chain those MAF lines imply, byte for byte"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    blocks = chm.maf_blocks(os.path.join(golden_dir, maf))
    want = [(chm.block_triples(b[1], b[2])[0], len(b[1][5])) for b in blocks]
    o = oracle_built.Oracle(idx, params)
    at, dumps = 0, []
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True); dumps.append(d)
        blk, sg = hostlib.segs(None, None, d)
        assert blk.dtype == capi.SEG_BLOCK_DT and sg.dtype == capi.SEG_DT
        assert blk.size == d["b_score"].size and blk["n_seg"].sum() == sg.size and (blk["seg_off"] == np.concatenate([[0], np.cumsum(blk["n_seg"])[:-1]])).all()
        for bi in range(blk.size):
            tr, cols = want[at]; at += 1
            mine = sg[blk["seg_off"][bi]:blk["seg_off"][bi] + blk["n_seg"][bi]]
            assert block_cols(mine) == int(d["b_aln_len"][bi])                         # untrimmed: starts and ends with a seed, every column is in a triple
            ext = block_cols(mine) - cols                                                # iExtension: the MAF text is shorter by what ran over the chromosome's end
            assert ext >= 0
            assert as_tuples(hostlib.segs_trim(mine, bool(d["b_bdir"][bi]), ext)) == tr, (bi, ext)
    assert at == len(want)
    it = iter(dumps)
    out_maf, out_vcf, out_chain = str(tmp_path / "o.maf"), str(tmp_path / "o.vcf"), str(tmp_path / "o.chain")
    hostlib.emit(px, px + ".qry.fa", out_maf, out_vcf, name, lambda ci, seq: next(it), chain=out_chain)
    o.close()
    assert open(out_chain, "rb").read() == chm.chain_of_maf(os.path.join(golden_dir, maf))
    assert open(out_maf, "rb").read() == open(os.path.join(golden_dir, maf), "rb").read()      # the chain in front trims nothing: the MAF is trimmed once
    assert open(out_vcf, "rb").read() == open(os.path.join(golden_dir, maf.replace(".maf", ".vcf")), "rb").read()


KIND_OF_CODE = {7: 0, 8: 0, 2: 1, 1: 2}


def test_segs_trim_is_cutting_the_text():
    """gsah_segs_trim against cutting the column list itself and stripping the gap columns the cut left at the edge (the scheme of test_cs_trim_is_cutting_the_text):
    forward blocks lose their last columns, reverse-strand blocks (triples in output order) their first; cuts inside a segment, at a segment's edge, inside a gap,
    through a gap with I and D columns, of everything and of more than there is.  The lists start and end with aligned columns, as untrimmed blocks do."""
    rng = np.random.default_rng(14)
    seen = set()
    for trial in range(200):
        n = int(rng.integers(1, 12))
        codes = rng.choice([1, 2, 7, 8], n)
        codes = np.concatenate([[7], codes, [8 if trial % 2 else 7]])
        codes = codes[np.concatenate([[True], codes[1:] != codes[:-1]])]
        lens = rng.integers(1, 9, codes.size)
        kinds = np.repeat(np.array([KIND_OF_CODE[int(c)] for c in codes], np.uint8), lens)
        full = chm.triples_of_kinds(kinds)[0]
        assert sum(s + a + b for s, a, b in full) == kinds.size
        t = np.array(full, capi.SEG_DT)
        inner = np.flatnonzero(kinds != 0)
        for bdir in (True, False):
            exts = {0, 1, int(lens[-1]), int(lens[0]), int(rng.integers(0, kinds.size + 1)), kinds.size, kinds.size + 3}
            if inner.size:      # a cut that ends on a gap column, and one that ends right behind it
                g = int(inner[int(rng.integers(0, inner.size))])
                exts |= {kinds.size - g, kinds.size - g - 1} if bdir else {g, g + 1}
            for ext in sorted(exts):
                keep = kinds[:max(kinds.size - ext, 0)] if bdir else kinds[min(ext, kinds.size):]
                got = as_tuples(hostlib.segs_trim(t, bdir, ext))
                assert got == chm.triples_of_kinds(keep)[0], (trial, bdir, ext)
                if 0 < ext < kinds.size:
                    c, e = (kinds.size - ext, kinds.size - ext - 1) if bdir else (ext - 1, ext)      # the cut's innermost column, the first column that stays
                    if kinds[e] == 0:
                        seen.add("seg" if kinds[c] == 0 else "seg-edge")
                    else:
                        seen.add("gap" if kinds[c] != 0 else "gap-edge")
                        lo = e
                        while kinds[lo - 1] != 0:
                            lo -= 1
                        hi = e
                        while kinds[hi + 1] != 0:
                            hi += 1
                        if kinds[c] != 0 and {1, 2} <= set(kinds[lo:hi + 1].tolist()):
                            seen.add("both")
                elif ext >= kinds.size:
                    assert got == []
    assert {"seg", "seg-edge", "gap", "gap-edge", "both"} <= seen


@pytest.fixture(scope="module")
def gap_edge_case(tmp_path_factory):
    """A sibling of test_cigars_host.overrun_case, built the same way: two reference sequences (400 and 300 bp) and one hand-made result of five blocks --
    (op strings: 'I' = a reference base facing '-', a chain's dt; 'D' = a query base facing '-', dq)
    A  forward on chrA, its last record a gap that runs 6 over: the cut ends inside an 'IIII' gap, which goes whole; in front a 'DD' run touches an 'III' run
    B  reverse strand of chrB, a seed as last record, 4 over; its gap holds 'DD' next to 'I'
    C  reverse strand of chrB, its last record a gap, 3 over: the cut ends inside an 'IIDDD' gap (one 'D' cut), so the block's start moves by what is left of it on both sides
    D  forward on chrB, one seed, 2 over, a duplicate: a one-segment block that -unique skips
    E  nothing to trim"""
    d = tmp_path_factory.mktemp("ge")
    rng = np.random.default_rng(29)
    chrA, chrB = synth.random_genome(400, rng), synth.random_genome(300, rng)
    qry = synth.random_genome(2000, rng)
    fa = str(d / "r.fa"); px = str(d / "r"); qfa = str(d / "q.fa")
    synth.write_fasta(fa, [("chrA", chrA), ("chrB", chrB)]); synth.write_fasta(qfa, [("q1", qry)])
    hostlib.build_index(fa, px)
    idx = indexio.load_index(px)
    G = idx.G
    assert G == 700
    ref = np.ascontiguousarray(idx.ref)
    B, F, A1, A2 = [], [], [], []

    def block(bdir, chrom, gpos, recs):
        """recs: ('s', qpos, rpos, len) | ('g', ops) behind a seed"""
        cols, nf = 0, 0
        for r in recs:
            if r[0] == "s":
                F.append((1, r[1], r[3], r[3], r[2], 0)); cols += r[3]
            else:
                _, qp, ql, rl, rp, _ = F[-1]
                a1, a2, rn, qn = gapped(ref, qry, rp + rl, qp + ql, r[1])
                F.append((0, qp + ql, qn, rn, rp + rl, len(a1))); A1.append(a1); A2.append(a2); cols += len(a1)
            nf += 1
        B.append((cols - 3, cols, 0, nf, bdir, gpos, chrom))

    block(1, 0, 341, [("s", 200, 340, 40), ("g", b"M" * 10 + b"DD" + b"III" + b"M" * 5 + b"IIII" + b"M" * 4)])      # 26 reference bases from 380: 6 over
    block(0, 1, 0, [("s", 400, G + 200, 60), ("g", b"MIMMDDIM"), ("s", 466, G + 266, 38)])                          # ends at G + 304: 4 over
    block(0, 1, 0, [("s", 600, G + 230, 45), ("g", b"M" * 20 + b"DDI" + b"MMM" + b"IIDDD" + b"MM")])               # 28 reference bases from G + 275: 3 over
    block(1, 1, 251, [("s", 800, 650, 52)])
    block(1, 0, 11, [("s", 900, 10, 30), ("g", b"IIMM"), ("s", 932, 44, 20)])
    dump = {"b_score": np.array([b[0] for b in B], np.int32), "b_aln_len": np.array([b[1] for b in B], np.int32), "b_bdup": np.array([0, 0, 0, 1, 0], np.int32),
            "b_nfrag": np.array([b[3] for b in B], np.int32), "b_bdir": np.array([b[4] for b in B], np.int32), "b_gpos": np.array([b[5] for b in B], np.int32),
            "b_chr": np.array([b[6] for b in B], np.int32),
            "f_bseed": np.array([f[0] for f in F], np.int32), "f_qpos": np.array([f[1] for f in F], np.int32), "f_qlen": np.array([f[2] for f in F], np.int32),
            "f_rlen": np.array([f[3] for f in F], np.int32), "f_rpos": np.array([f[4] for f in F], np.int64), "f_alnlen": np.array([f[5] for f in F], np.int32),
            "aln1": np.frombuffer(b"".join(A1), np.uint8), "aln2": np.frombuffer(b"".join(A2), np.uint8)}
    return px, qfa, qry, dump


def parse_chain(data: bytes):
    """[(header fields, [(size, dt, dq)])] of a chain file"""
    out = []
    for para in data.decode().split("\n\n"):
        if not para.strip():
            continue
        lines = para.strip("\n").split("\n")
        h = lines[0].split(" ")
        assert h[0] == "chain" and len(h) == 13
        tr = [tuple(int(x) for x in ln.split("\t")) for ln in lines[1:-1]] + [(int(lines[-1]), 0, 0)]
        assert all(len(t) == 3 for t in tr)
        out.append((h, tr))
    return out


@pytest.mark.parametrize("allow_dup", [True, False])
def test_chain_trims_like_the_maf_text(gap_edge_case, tmp_path, allow_dup):
    """the emitter cuts the triples the way maf_block cuts text and drops the gap the cut left at the edge: the chain it writes == the chain implied by the MAF the same
    library writes; the header's invariants hold"""
    px, qfa, qry, dump = gap_edge_case
    cp = lambda: {k: v.copy() for k, v in dump.items()}
    blk, sg = hostlib.segs(None, None, cp())
    un = [as_tuples(sg[b["seg_off"]:b["seg_off"] + b["n_seg"]]) for b in blk]
    assert un[0] == [(50, 3, 2), (5, 4, 0), (4, 0, 0)]                         # a gap with both sides: 'DD' touches 'III'
    assert un[1] == [(39, 1, 2), (2, 1, 0), (61, 0, 0)]                        # reverse strand, output order: 'MIMMDDIM' back to front, the gap in front comes behind
    assert un[2] == [(2, 2, 3), (3, 1, 2), (65, 0, 0)] and un[3] == [(52, 0, 0)] and un[4] == [(30, 2, 0), (22, 0, 0)]
    hostlib.emit(px, qfa, str(tmp_path / "o.maf"), str(tmp_path / "m.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=1, chain=str(tmp_path / "o.chain"))
    hostlib.emit(px, qfa, str(tmp_path / "p.maf"), str(tmp_path / "p.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=1)
    assert open(tmp_path / "o.maf", "rb").read() == open(tmp_path / "p.maf", "rb").read() and open(tmp_path / "m.vcf", "rb").read() == open(tmp_path / "p.vcf", "rb").read()
    got = open(tmp_path / "o.chain", "rb").read()
    assert got == chm.chain_of_maf(str(tmp_path / "o.maf"))
    chains = parse_chain(got)
    assert len(chains) == (5 if allow_dup else 4) and [int(h[12]) for h, _ in chains] == list(range(1, len(chains) + 1))
    for h, tr in chains:
        assert int(h[6]) - int(h[5]) == sum(s + dt for s, dt, _ in tr) and int(h[11]) - int(h[10]) == sum(s + dq for s, _, dq in tr)
        assert all(s > 0 and dt >= 0 and dq >= 0 and dt + dq > 0 for s, dt, dq in tr[:-1]) and tr[-1][0] > 0
    assert chains[0][1] == [(50, 3, 2), (5, 0, 0)]                             # A: the cut ended inside 'IIII', the whole gap went
    assert chains[0][0][1:7] == ["59", "chrA", "400", "+", "340", "398"] and chains[0][0][7:12] == ["q1", "2000", "+", "200", "257"]
    assert chains[2][1][0][0] == 3 and chains[2][0][9] == "-"                  # C: 'MM' and one 'D' cut, 'IIDD' dropped, the chain starts with 'MMM'
    assert any(dt > 0 and dq > 0 for _, tr in chains for _, dt, dq in tr)
    if allow_dup:
        assert chains[3][0][1] == "1" and len(chains[3][1]) == 1               # the duplicate prints score 1; one segment, no data line with three fields
    # the same chain beside a PAF with cs, whose emitter trims the result after the chain has read it
    hostlib.emit(px, qfa, str(tmp_path / "q.paf"), str(tmp_path / "q.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3, cs=True, chain=str(tmp_path / "q.chain"))
    assert open(tmp_path / "q.chain", "rb").read() == got


def map_through(tr_walk, r0, q0, t):
    """text position t through a block's triples in WALK order from (r0, q0): ('M', query position) | ('D', None) | None"""
    r, q = r0, q0
    for size, dt, dq in tr_walk:
        if r <= t < r + size:
            return "M", q + (t - r)
        if r + size <= t < r + size + dt:
            return "D", None
        r += size + dt; q += size + dq
    return None


def test_segs_agree_with_lift(oracle_built, golden_dir):
    """every lifted position of class '=' / 'X' is mapped to the hit's query position by the chosen block's triples; a position of class 'D' lies in a dt gap"""
    px = os.path.join(golden_dir, "cx")
    idx = indexio.load_index(px)
    G = int(idx.G)
    o = oracle_built.Oracle(idx, {})
    rng = np.random.default_rng(5)
    pos = np.sort(rng.choice(G, 20000, replace=False)).astype(np.int64)
    seen = {7: 0, 8: 0, 2: 0}; rev = 0
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True)
        blk, sg = hostlib.segs(None, None, d)
        hits = hostlib.lift(px, None, d, pos)
        f0 = np.concatenate([[0], np.cumsum(d["b_nfrag"])[:-1]])
        for h in hits:
            bi = int(h["block"]); fwd = bool(d["b_bdir"][bi])
            tr = as_tuples(sg[blk["seg_off"][bi]:blk["seg_off"][bi] + blk["n_seg"][bi]])
            if not fwd:      # output order -> walk order: back to front, a triple's gap is the one IN FRONT of its segment
                tr = [(tr[k][0],) + (tr[k - 1][1:] if k > 0 else (0, 0)) for k in range(len(tr) - 1, -1, -1)]
                rev += 1
            p = int(pos[h["idx"]]); t = p if fwd else 2 * G - 1 - p
            m = map_through(tr, int(d["f_rpos"][f0[bi]]), int(d["f_qpos"][f0[bi]]), t)
            assert m is not None, (bi, p)
            if int(h["cls"]) == 2:
                assert m[0] == "D", (bi, p)
            else:
                assert m == ("M", int(h["qpos"])), (bi, p, m, int(h["qpos"]))
            seen[int(h["cls"])] += 1
    o.close()
    assert seen[7] > 10000 and seen[8] > 50 and seen[2] > 20 and rev > 0
