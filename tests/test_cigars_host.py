"""CPU tests of the per-block CIGARs (gsa_block_cigar / gsa_cigars, include/gsa_hip.h): the record layout and the header's cg helper, the host
walk gsah_c_cigars -- the comparator of the GPU pass -- pinned to the REFERENCE's own MAF files through the oracle's finished blocks, the
iExtension trim, and the PAF emitter (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import paf_from_maf as pm
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_cigar_record_layout_and_cg_helper(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_block_cigar); }\nint sz2(void) { return (int)sizeof(gsa_cigars); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'size_t cg(const uint32_t *ops, int64_t n, char *buf, size_t cap) { return gsa_cigar_string(ops, n, buf, cap); }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 32 == capi.BLOCK_CIGAR_DT.itemsize == C.sizeof(capi.BlockCigar)
    assert x.sz2() == C.sizeof(capi.Cigars) == 32 and x.sz3() == C.sizeof(capi.Extras) == 16
    x.cg.restype = C.c_size_t
    x.cg.argtypes = [C.c_void_p, C.c_int64, C.c_char_p, C.c_size_t]
    ops = np.array([(1 << 4) | 7, (10 << 4) | 8, (123456 << 4) | 1, (((1 << 28) - 1) << 4) | 2, (60 << 4) | 7, (9 << 4) | 8], np.uint32)
    want = capi.cigar_string(ops)
    assert want == "1=10X123456I268435455D60=9X"
    buf = C.create_string_buffer(128)
    assert x.cg(C.c_void_p(ops.ctypes.data), ops.size, buf, 128) == len(want) and buf.value.decode() == want
    assert x.cg(C.c_void_p(ops.ctypes.data), 0, buf, 128) == 0 and buf.value == b""
    small = C.create_string_buffer(b"#" * 16, 16)                      # a buffer that is too short: cut, terminated, the full length reported
    assert x.cg(C.c_void_p(ops.ctypes.data), ops.size, small, 8) == len(want) and small.value.decode() == want[:7] and small.raw[8:] == b"#" * 8


def golden_paf_runs(golden_dir, maf):
    return [pm.paf_line(*b) for b in pm.maf_blocks(os.path.join(golden_dir, maf))]


# blocks and total ops of the three MAF files under the column rule of include/gsa_hip.h (derived from the files with paf_from_maf).  Comparing the two rows
# byte for byte instead -- case-sensitive, N equal to N -- gives 27 303 / 27 344 / 3 640 ops: cx holds 3 430 columns that differ only in case and 255 with an N
# against a base, so the totals tell the two rules apart
GOLDEN_SHAPE = {"cx.maf": (22, 27493), "cx_sen.maf": (22, 27479), "small.maf": (2, 3640)}


@pytest.mark.parametrize("name,params,maf", [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")])
def test_host_cigars_give_the_reference_maf_columns(oracle_built, golden_dir, tmp_path, name, params, maf):
    """comparator ops -> trimmed -> cg strings == the strings derived here from the two `s` lines of every block of the reference's MAF; and the
    whole PAF file the emitter writes from them == the PAF those MAF lines imply, byte for byte"""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    want = golden_paf_runs(golden_dir, maf)
    n_ops = sum(len(r) for _, r in want)
    assert (len(want), n_ops) == GOLDEN_SHAPE[maf]
    assert sum(1 for ln, _ in want if ln.split("\t")[4] == "-") >= 1                      # a reverse-strand block in every file
    if maf == "cx.maf":
        assert max(len(r) for _, r in want) == 9650 and max(l for _, r in want for c, l in r if c in (1, 2)) == 60
        assert {c for _, r in want for c, _ in r} == {1, 2, 7, 8}
    o = oracle_built.Oracle(idx, params)
    at, dumps = 0, []
    for _, seq in synth.read_fasta(px + ".qry.fa"):
        o.set_query(seq); o.run_to(8)
        d = o.blocks(with_aln=True); dumps.append(d)
        blk, ops = hostlib.cigars(px, seq, d)
        blk2, ops2 = hostlib.cigars(None, None, d)                                        # without the query text a seed is '=' by definition: the same answer
        assert np.array_equal(blk, blk2) and np.array_equal(ops, ops2)
        assert blk.size == d["b_score"].size and (blk["n_cig"].sum() == ops.size) and (blk["cig_off"] == np.concatenate([[0], np.cumsum(blk["n_cig"])[:-1]])).all()
        for bi in range(blk.size):
            line, runs = want[at]; at += 1
            b = blk[bi]; mine = ops[b["cig_off"]:b["cig_off"] + b["n_cig"]]
            cols = int(b["n_eq"]) + int(b["n_x"]) + int(b["n_ins"]) + int(b["n_del"])
            assert cols == int((mine >> 4).sum()) == int(d["b_aln_len"][bi])
            ext = cols - sum(l for _, l in runs)                                         # iExtension: the MAF text is shorter by what ran over the chromosome's end
            assert ext >= 0
            got, cnt = hostlib.cigar_trim(mine, bool(d["b_bdir"][bi]), ext, (b["n_eq"], b["n_x"], b["n_ins"], b["n_del"]))
            assert capi.cigar_string(got) == pm.cg_of(runs), (bi, ext)
            assert cnt == tuple(sum(l for c, l in runs if c == k) for k in (7, 8, 1, 2))
    assert at == len(want)
    it = iter(dumps)
    out_paf, out_vcf = str(tmp_path / "o.paf"), str(tmp_path / "o.vcf")
    hostlib.emit(px, px + ".qry.fa", out_paf, out_vcf, name, lambda ci, seq: next(it), fmt=3)
    o.close()
    assert open(out_paf, "rb").read() == "".join(ln + "\n" for ln, _ in want).encode()
    assert open(out_vcf, "rb").read() == open(os.path.join(golden_dir, maf.replace(".maf", ".vcf")), "rb").read()


def test_host_paf_unique(oracle_built, golden_dir, tmp_path):
    """-unique: duplicate blocks are skipped, as in OutputMAF"""
    px = os.path.join(golden_dir, "cx")
    o = oracle_built.Oracle(indexio.load_index(px), {})

    def per_contig(ci, seq):
        o.set_query(seq); o.run_to(8)
        return o.blocks(with_aln=True)

    hostlib.emit(px, px + ".qry.fa", str(tmp_path / "o.paf"), str(tmp_path / "o.vcf"), "cx", per_contig, allow_dup=False, fmt=3)
    o.close()
    assert open(tmp_path / "o.paf", "rb").read() == pm.paf_of_maf(os.path.join(golden_dir, "cx_unique.maf"))


def test_cigar_trim_is_cutting_the_text():
    """gsah_cigar_trim against cutting the column list itself: forward blocks lose their last columns, reverse-strand blocks (ops in output
    order) their first; cuts inside a run, at run edges, over several runs, of everything and of more than there is"""
    rng = np.random.default_rng(11)
    for trial in range(200):
        n = int(rng.integers(1, 12))
        codes = rng.choice([1, 2, 7, 8], n)
        codes = codes[np.concatenate([[True], codes[1:] != codes[:-1]])]
        lens = rng.integers(1, 9, codes.size)
        cols = np.repeat(codes, lens).astype(np.uint8)
        ops = pm.ops_of(list(zip(codes.tolist(), lens.tolist())))
        cnt = tuple(int((cols == k).sum()) for k in (7, 8, 1, 2))
        for bdir in (True, False):
            for ext in sorted({0, 1, int(lens[-1]), int(lens[0]), int(rng.integers(0, cols.size + 1)), cols.size, cols.size + 3}):
                keep = cols[:max(cols.size - ext, 0)] if bdir else cols[min(ext, cols.size):]
                got, c2 = hostlib.cigar_trim(ops, bdir, ext, cnt)
                assert np.array_equal(got, pm.ops_of(pm.rle(keep))), (trial, bdir, ext)
                assert c2 == tuple(int((keep == k).sum()) for k in (7, 8, 1, 2))


def gapped(ref, qry, rpos, qpos, ops):
    """the two gapped strings of an M/D/I op string ('D': '-' in the reference row, 'I': '-' in the query row) and the bases they use"""
    a1, a2 = capi.apply_ops(ref[rpos:].tobytes(), qry[qpos:].tobytes(), ops)
    return a1, a2, len(ops) - ops.count(b"D"), len(ops) - ops.count(b"I")


@pytest.fixture(scope="module")
def overrun_case(tmp_path_factory):
    """Two reference sequences (400 and 300 bp) and one hand-made result of six blocks whose last record runs past the end of the block's
    reference sequence by a few bases (the sixth does not): forward and reverse strand, a seed and a gap as the last record, a cut inside a run
    and a cut over several runs."""
    d = tmp_path_factory.mktemp("ov")
    rng = np.random.default_rng(23)
    chrA, chrB = synth.random_genome(400, rng), synth.random_genome(300, rng)
    qry = synth.random_genome(2000, rng)
    qry[62] |= 0x20; qry[63] = ord("N")                # inside the first block's gap: a lower-case base and an ambiguous one
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

    # forward on chrA (ends at 400): last record a seed that runs 5 over; a cut inside the last '=' run
    block(1, 0, 301, [("s", 10, 300, 50), ("g", b"MMDDMIM"), ("s", 66, 355, 50)])
    # forward on chrA: last record a GAP that runs 6 over, the cut crosses several runs (... M I I M D M: 6 columns hold 5 reference bases -> more)
    block(1, 0, 341, [("s", 200, 340, 40), ("g", b"M" * 16 + b"DMMIMIMDMMMM")])
    # reverse strand of chrB: positions [G, G + 300); last record a seed that runs 4 over (into chrA's reverse copy)
    block(0, 1, 0, [("s", 400, G + 200, 60), ("g", b"MDMMIIM"), ("s", 465, G + 266, 38)])
    # reverse strand of chrB: last record a gap, 7 over
    block(0, 1, 0, [("s", 600, G + 230, 45), ("g", b"M" * 23 + b"IIMMDMMMDMM")])
    # forward on chrB (fwd positions [400, 700)): a seed as last record, 2 over, and a duplicate block
    block(1, 1, 251, [("s", 800, 650, 52)])
    # nothing to trim
    block(1, 0, 11, [("s", 900, 10, 30), ("g", b"IIMM"), ("s", 932, 44, 20)])
    dump = {"b_score": np.array([b[0] for b in B], np.int32), "b_aln_len": np.array([b[1] for b in B], np.int32), "b_bdup": np.array([0, 0, 0, 0, 1, 0], np.int32),
            "b_nfrag": np.array([b[3] for b in B], np.int32), "b_bdir": np.array([b[4] for b in B], np.int32), "b_gpos": np.array([b[5] for b in B], np.int32),
            "b_chr": np.array([b[6] for b in B], np.int32),
            "f_bseed": np.array([f[0] for f in F], np.int32), "f_qpos": np.array([f[1] for f in F], np.int32), "f_qlen": np.array([f[2] for f in F], np.int32),
            "f_rlen": np.array([f[3] for f in F], np.int32), "f_rpos": np.array([f[4] for f in F], np.int64), "f_alnlen": np.array([f[5] for f in F], np.int32),
            "aln1": np.frombuffer(b"".join(A1), np.uint8), "aln2": np.frombuffer(b"".join(A2), np.uint8)}
    return px, qfa, qry, dump


@pytest.mark.parametrize("allow_dup", [True, False])
def test_paf_trim_like_the_maf_text(overrun_case, tmp_path, allow_dup):
    """the emitter trims ops the way maf_block trims text: the PAF it writes == the PAF implied by the MAF the same library writes for the same result"""
    px, qfa, qry, dump = overrun_case
    cp = lambda: {k: v.copy() for k, v in dump.items()}
    hostlib.emit(px, qfa, str(tmp_path / "o.maf"), str(tmp_path / "m.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=1)
    hostlib.emit(px, qfa, str(tmp_path / "o.paf"), str(tmp_path / "p.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3)
    blocks = pm.maf_blocks(str(tmp_path / "o.maf"))
    assert len(blocks) == (6 if allow_dup else 5)
    # the cut happened: the printed text is shorter than the records by 5, 6, 4, 7, 2, 0 columns
    full = dump["b_aln_len"].tolist(); over = [5, 6, 4, 7, 2, 0]
    if not allow_dup:
        full.pop(4); over.pop(4)
    assert [len(b[1][5]) for b in blocks] == [f - e for f, e in zip(full, over)]
    assert [b[2][3] for b in blocks] == (["+", "+", "-", "-", "+", "+"] if allow_dup else ["+", "+", "-", "-", "+"])
    got = open(tmp_path / "o.paf", "rb").read()
    assert got == pm.paf_of_maf(str(tmp_path / "o.maf"))
    if allow_dup:
        assert got.split(b"\n")[4].split(b"\t")[13:15] == [b"AS:i:1", b"tp:A:S"]
    # the variant walk sees the same shortened records either way
    assert open(tmp_path / "p.vcf", "rb").read() == open(tmp_path / "m.vcf", "rb").read()
    # untrimmed comparator: the last block's ops are the text's
    blk, ops = hostlib.cigars(px, qry, dump)
    assert capi.cigar_string(ops[blk["cig_off"][5]:blk["cig_off"][5] + blk["n_cig"][5]]) == pm.cg_of(pm.paf_line(*blocks[-1])[1])
