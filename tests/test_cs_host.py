"""CPU tests of the per-block cs strings (gsa_cs_block / gsa_cs, include/gsa_hip.h): the record layout, the host walk gsah_c_cs -- the comparator of the GPU
pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, the iExtension trim, and the PAF emitter's cs:Z: field (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cs_from_maf as cm
import paf_from_maf as pm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth
from test_cigars_host import overrun_case      # noqa: F401  (the hand-made result whose blocks run past the end of their reference sequence)


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_cs_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_cs_block); }\nint sz2(void) { return (int)sizeof(gsa_cs); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'int want(void) { return (int)GSA_WANT_CS; }\nint fn(void) { return (int)sizeof(gsa_block_cs((gsa_ctx *)0, 0, (gsa_cs *)0)); }\n')      # (unevaluated: the function's C declaration)
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 16 == capi.BLOCK_CS_DT.itemsize == C.sizeof(capi.CsBlock)
    assert x.sz2() == C.sizeof(capi.Cs) == 32 and x.sz3() == C.sizeof(capi.Extras) == 16
    assert x.want() == capi.WANT_CS == 4 and x.fn() == 4
    assert {"gsa_block_cs", "gsa_get_cs_timing", "gsa_extras_cs"} <= set(capi.EXPORTS)


# blocks, reverse-strand blocks, cs bytes, longest X run, longest I / D run and 'n' letters of the golden MAF files under the rule of include/gsa_hip.h (derived from
# the files with cs_from_maf)
GOLDEN_CS_SHAPE = {"cx.maf": (22, 1, 91181, 146, 60, 30, 283), "small.maf": (2, 1, 11924)}


def golden_cs_shape(golden_dir, maf):
    blocks = pm.maf_blocks(os.path.join(golden_dir, maf))
    runs = [pm.paf_line(*b)[1] for b in blocks]
    cs = cm.maf_cs(os.path.join(golden_dir, maf))
    longest = lambda code: max([n for r in runs for c, n in r if c == code], default=0)
    n_letters = sum(s.count("n") for s in cs)
    return (len(blocks), sum(1 for b in blocks if b[2][3] == "-"), sum(len(s) for s in cs), longest(8), longest(1), longest(2), n_letters)


def test_golden_coverage(golden_dir):
    """what the parity tests stand on: all four token kinds, a reverse-strand block, X runs of more than 64 columns and of more than one, 'n' letters"""
    for maf, want in GOLDEN_CS_SHAPE.items():
        assert golden_cs_shape(golden_dir, maf)[:len(want)] == want, maf
    runs = [pm.paf_line(*b)[1] for b in pm.maf_blocks(os.path.join(golden_dir, "cx.maf"))]
    assert sum(1 for r in runs for c, n in r if c == 8 and n > 1) == 1091
    rows = b"".join(b[1][5] + b[2][5] for b in pm.maf_blocks(os.path.join(golden_dir, "cx.maf")))
    assert {ord("R"), ord("Y"), ord("N")} <= set(rows) and any(chr(c).islower() for c in set(rows))


@pytest.mark.parametrize("name,params,maf", [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")])
def test_host_cs_gives_the_reference_maf_columns(oracle_built, golden_dir, tmp_path, name, params, maf):
    """comparator strings -> trimmed == the strings derived here from the two `s` lines of every block of the reference's MAF; and the whole PAF file
    the emitter writes with cs=True == the PAF those MAF lines imply, byte for byte"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    blocks = pm.maf_blocks(os.path.join(golden_dir, maf))
    want = [(pm.paf_line(*b)[1], cm.cs_of_rows(b[1][5], b[2][5])) for b in blocks]
    o = oracle_built.Oracle(idx, params)
    at, dumps = 0, []
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True); dumps.append(d)
        cblk, ops = hostlib.cigars(None, seq, d)
        blk, by = hostlib.cs(None, None, d)
        assert blk.dtype == capi.BLOCK_CS_DT and by.dtype == np.uint8
        assert blk.size == d["b_score"].size and blk["n_cs"].sum() == by.size and (blk["cs_off"] == np.concatenate([[0], np.cumsum(blk["n_cs"])[:-1]])).all()
        for bi in range(blk.size):
            runs, cs = want[at]; at += 1
            mine_ops = ops[cblk["cig_off"][bi]:cblk["cig_off"][bi] + cblk["n_cig"][bi]]
            mine = by[blk["cs_off"][bi]:blk["cs_off"][bi] + blk["n_cs"][bi]].tobytes()
            assert len(mine) == capi.cs_of_ops_length(mine_ops)
            ext = int((mine_ops >> 4).sum()) - sum(l for _, l in runs)                     # iExtension: the MAF text is shorter by what ran over the chromosome's end
            assert ext >= 0
            got = hostlib.cs_trim(mine, mine_ops, bool(d["b_bdir"][bi]), ext)
            assert got.decode() == cs, (bi, ext)
    assert at == len(want)
    it = iter(dumps)
    out_paf, out_vcf = str(tmp_path / "o.paf"), str(tmp_path / "o.vcf")
    hostlib.emit(px, px + ".qry.fa", out_paf, out_vcf, name, lambda ci, seq: next(it), fmt=3, cs=True)
    o.close()
    assert open(out_paf, "rb").read() == cm.paf_cs_of_maf(os.path.join(golden_dir, maf))
    assert open(out_vcf, "rb").read() == open(os.path.join(golden_dir, maf.replace(".maf", ".vcf")), "rb").read()


def test_cs_trim_is_cutting_the_text():
    """gsah_cs_trim against cutting the column list itself (the scheme of test_cigar_trim_is_cutting_the_text): forward blocks lose their last columns,
    reverse-strand blocks (string in output order) their first; cuts inside a run, at run edges, over several runs, of everything and of more than there is"""
    rng = np.random.default_rng(12)
    for trial in range(200):
        n = int(rng.integers(1, 12))
        codes = rng.choice([1, 2, 7, 8], n)
        codes = codes[np.concatenate([[True], codes[1:] != codes[:-1]])]
        lens = rng.integers(1, 9, codes.size)
        if trial % 7 == 0:
            lens[int(rng.integers(0, lens.size))] = int(rng.choice([9, 10, 11, 99, 100, 101, 1000]))      # a ':n' whose number of digits changes under the cut
        cols = np.repeat(codes, lens).astype(np.uint8)
        r = bytes(rng.choice(list(b"acgtn"), cols.size).astype(np.uint8)); q = bytes(rng.choice(list(b"acgtn"), cols.size).astype(np.uint8))
        ops = pm.ops_of(list(zip(codes.tolist(), lens.tolist())))
        full = cm.cs_of_cols(cols, r, q)
        assert len(full) == capi.cs_of_ops_length(ops)
        for bdir in (True, False):
            for ext in sorted({0, 1, int(lens[-1]), int(lens[0]), int(rng.integers(0, cols.size + 1)), cols.size, cols.size + 3}):
                sl = slice(0, max(cols.size - ext, 0)) if bdir else slice(min(ext, cols.size), None)
                got = hostlib.cs_trim(full, ops, bdir, ext)
                assert got.decode() == cm.cs_of_cols(cols[sl], r[sl], q[sl]), (trial, bdir, ext)


@pytest.mark.parametrize("allow_dup", [True, False])
def test_paf_cs_trim_like_the_maf_text(overrun_case, tmp_path, allow_dup):
    """the emitter trims the strings the way maf_block trims text: the PAF with cs it writes == the PAF with cs implied by the MAF the same library writes"""
    px, qfa, qry, dump = overrun_case
    cp = lambda: {k: v.copy() for k, v in dump.items()}
    hostlib.emit(px, qfa, str(tmp_path / "o.maf"), str(tmp_path / "m.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=1)
    hostlib.emit(px, qfa, str(tmp_path / "o.paf"), str(tmp_path / "p.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3, cs=True)
    blocks = pm.maf_blocks(str(tmp_path / "o.maf"))
    assert len(blocks) == (6 if allow_dup else 5)
    got = open(tmp_path / "o.paf", "rb").read()
    assert got == cm.paf_cs_of_maf(str(tmp_path / "o.maf"))
    assert all(ln.split(b"\t")[-1].startswith(b"cs:Z:") and ln.split(b"\t")[-2].startswith(b"cg:Z:") for ln in got.split(b"\n")[:-1])
    assert b"*" in got and b"+" in got.split(b"cs:Z:")[1] and b"n" in b"".join(ln.split(b"cs:Z:")[1] for ln in got.split(b"\n")[:-1])      # the lower-case base and the N of the first gap
    assert open(tmp_path / "p.vcf", "rb").read() == open(tmp_path / "m.vcf", "rb").read()
    # without cs=True the file is the plain PAF
    hostlib.emit(px, qfa, str(tmp_path / "q.paf"), str(tmp_path / "q.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3)
    assert open(tmp_path / "q.paf", "rb").read() == pm.paf_of_maf(str(tmp_path / "o.maf"))
