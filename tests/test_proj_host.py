"""CPU tests of the query projected onto the reference (gsa_project / gsa_proj_stat, include/gsa_hip.h): the layout, and the host walk gsah_c_project -- the comparator of
the GPU pass -- pinned word for word to the REFERENCE's own MAF files through the oracle's finished blocks, per contig and accumulated in either order; to the host lift of
every position wherever the two best covering blocks differ; to the duplicate flag, to the trim on a hand-made result that runs past the end of its reference
sequences, and the FASTA text of the emitter (no GPU needed)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import paf_from_maf as pm
import proj_from_maf as pj
from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio
from test_cigars_host import overrun_case      # noqa: F401  (fixture)
from test_track_host import golden_results     # noqa: F401  (fixture)


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_proj_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stddef.h>\n#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_proj_stat); }\nint o1(void) { return (int)offsetof(gsa_proj_stat, n_cols); }\nint sz3(void) { return (int)sizeof(gsa_extras); }\n'
                   'unsigned w(void) { return GSA_WANT_PROJ; }\nunsigned f(void) { return GSA_PROJ_NO_DUP; }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 16 == C.sizeof(capi.ProjStat) and x.o1() == 8 == capi.ProjStat.n_cols.offset and x.sz3() == 16
    assert x.w() == 128 == capi.WANT_PROJ and x.f() == 1 == capi.PROJ_NO_DUP


def chr_starts(idx):
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    return starts, {n: int(s) for n, s in zip(idx.chr_names, starts)}


def same(a, b, what=""):
    assert a.dtype == np.uint32 and b.dtype == np.uint32 and a.size == b.size
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (what, bad.size, bad[:5], [hex(int(v)) for v in a[bad[:5]]], [hex(int(v)) for v in b[bad[:5]]])


@pytest.mark.parametrize("key", ["cx", "cx_sen", "small"])
def test_host_projection_gives_what_the_reference_maf_implies(golden_results, key):
    """hostlib.project == the columns of the reference's MAF, word for word: every contig alone, all contigs accumulated in file order and in reverse order; the alphabet"""
    px, idx, res = golden_results[key]
    G = int(idx.G)
    _, chr_start = chr_starts(idx)
    want_all = np.zeros(G, np.uint32)
    fwd, n_rev_cols, spans = np.zeros(G, np.uint32), 0, 0
    for qn, seq, d, mine in res:
        assert [b[0] == 1 for b in mine] == [bool(x) for x in d["b_bdup"]]
        got = np.zeros(G, np.uint32)
        nb, ncols = hostlib.project(px, seq, d, got)
        want = pj.contig_words(mine, chr_start, np.zeros(G, np.uint32), d["b_bdup"], d["b_score"])
        same(got, want, (key, qn))
        assert nb == len(mine) and ncols == sum(b[1][2] for b in mine)      # (words offered: the MAF lines' own reference sizes)
        spans += ncols
        pj.contig_words(mine, chr_start, want_all, d["b_bdup"], d["b_score"])
        hostlib.project(px, seq, d, fwd)
        n_rev_cols += sum(b[1][2] for b in mine if b[2][3] == "-")
    same(fwd, want_all, (key, "file order"))
    back = np.zeros(G, np.uint32)
    for qn, seq, d, mine in reversed(res):
        hostlib.project(px, seq, d, back)
    same(back, want_all, (key, "reverse order"))
    assert hostlib.proj_text(fwd) == pj.text_of(want_all)
    # the ground this test stands on: covered and uncovered positions, deleted bases, and N or mismatching bases (a mismatch shows as a base that is not the reference's)
    codes = fwd & 7
    ref_code = pm.NT4[np.asarray(idx.ref[:G], np.uint8)].astype(np.uint32) + 1
    assert (codes == 0).any() and (codes == 6).any() and ((codes >= 1) & (codes <= 5) & (codes != ref_code)).any() and (codes <= 6).all(), np.bincount(codes, minlength=8)
    assert ((fwd != 0) == (fwd >> 31 == 1)).all()      # (the golden runs hold no duplicate block)
    assert spans >= int((fwd != 0).sum()) > 1000
    if key != "small":
        assert n_rev_cols > 0


def one_block(d, bi):
    """the result that holds block bi alone"""
    f_at = np.concatenate([[0], np.cumsum(d["b_nfrag"])]); a_at = np.concatenate([[0], np.cumsum(d["f_alnlen"])])
    fs = slice(int(f_at[bi]), int(f_at[bi + 1]))
    one = {k: v[bi:bi + 1] for k, v in d.items() if k.startswith("b_")}
    one.update({k: v[fs] for k, v in d.items() if k.startswith("f_")})
    one["aln1"] = d["aln1"][int(a_at[fs.start]):int(a_at[fs.stop])]; one["aln2"] = d["aln2"][int(a_at[fs.start]):int(a_at[fs.stop])]
    return one


def test_projection_is_the_lift_of_every_position_where_the_best_blocks_differ(golden_results):
    """against hostlib.lift of every position: wherever the two best covering blocks differ in (dup, clamped score) the character is the one the hit implies"""
    px, idx, res = golden_results["cx"]
    G = int(idx.G)
    allpos = np.arange(G, dtype=np.int64)
    n_hits = n_decided = n_multi = 0
    for qn, seq, d, _ in res:
        words = np.zeros(G, np.uint32)
        hostlib.project(px, seq, d, words)
        text = np.frombuffer(hostlib.proj_text(words), np.uint8)
        H = hostlib.lift(px, seq, d, allpos)
        assert np.array_equal(np.flatnonzero(words), H["idx"])      # (the same trimmed coverage)
        # the two greatest (dup, clamped score) keys among the blocks that cover each position
        top = np.zeros((2, G), np.int64)
        for bi in range(int(d["b_score"].size)):
            w = np.zeros(G, np.uint32)
            hostlib.project(px, seq, one_block(d, bi), w)
            k = np.where(w != 0, (w >> 3).astype(np.int64) + 1, 0)
            lo = np.minimum(top[0], k); top[0] = np.maximum(top[0], k); top[1] = np.maximum(top[1], lo)
        p = H["idx"]
        decided = top[0][p] != top[1][p]
        assert ((H["n_cover"] == 1) <= decided).all()
        q = np.asarray(seq, np.uint8)[np.maximum(H["qpos"], 0)]
        code = pm.NT4[q].astype(np.int64) + 1
        code = np.where((H["rev"] == 1) & (code <= 4), 5 - code, code)
        code = np.where(H["cls"] == 2, 6, code)
        assert np.array_equal(text[p][decided], pj.LETTERS[code][decided])
        assert np.array_equal((words[p] >> 3)[decided].astype(np.int64) + 1, top[0][p][decided])
        n_hits += int(p.size); n_decided += int(decided.sum()); n_multi += int((H["n_cover"] > 1).sum())
    assert n_multi > 0 and n_decided >= 0.9 * n_hits > 1000, (n_hits, n_decided, n_multi)


def test_no_dup_leaves_duplicate_blocks_out(golden_results):
    """a result whose first block is marked a duplicate: without the flag its bases stand with bit 31 clear, with GSA_PROJ_NO_DUP they are absent"""
    px, idx, res = golden_results["small"]
    G = int(idx.G)
    qn, seq, d, mine = next(r for r in res if len(r[3]) > 0)
    d2 = dict(d); d2["b_bdup"] = d["b_bdup"].copy(); d2["b_bdup"][0] = 1
    first = np.zeros(G, np.uint32); hostlib.project(px, seq, one_block(d, 0), first)
    rest = np.zeros(G, np.uint32)
    for bi in range(1, len(mine)):
        hostlib.project(px, seq, one_block(d, bi), rest)
    only_first = (first != 0) & (rest == 0)
    assert only_first.sum() > 0
    a = np.zeros(G, np.uint32); na = hostlib.project(px, seq, d2, a)
    b = np.zeros(G, np.uint32); nb = hostlib.project(px, seq, d2, b, flags=capi.PROJ_NO_DUP)
    assert na[0] == len(mine) and nb[0] == len(mine) - 1
    assert (a[only_first] != 0).all() and (a[only_first] >> 31 == 0).all() and np.array_equal(a[only_first] & 0x7FFFFFFF, first[only_first] & 0x7FFFFFFF)
    assert (b[only_first] == 0).all() and np.array_equal(b, rest)
    _, chr_start = chr_starts(idx)
    same(b, pj.contig_words(mine, chr_start, np.zeros(G, np.uint32), d2["b_bdup"], d2["b_score"], no_dup=True), "no_dup")


def test_projection_stops_at_the_end_of_the_reference_sequence(overrun_case):
    """the hand-made result whose blocks run past the end of their reference sequences paints nothing beyond its sequence's end"""
    px, qfa, qry, dump = overrun_case
    idx = indexio.load_index(px)
    G = int(idx.G)
    assert G == 700
    w = np.zeros(G, np.uint32)
    nb, ncols = hostlib.project(px, qry, dump, w)
    # block 0: forward on chrA [300, 405) -> [300, 400); block 1: [340, 406) -> [340, 400); blocks 2 and 3: reverse strand of chrB -> forward [400, 500) / [400, 470);
    # block 4 (a duplicate): [650, 702) -> [650, 700); block 5: [10, 64)
    assert set(np.flatnonzero(w).tolist()) == set(range(10, 64)) | set(range(300, 500)) | set(range(650, 700))
    assert nb == 6 and ncols == 54 + 100 + 60 + 100 + 70 + 50
    assert (w[650:700] >> 31 == 0).all() and (w[300:500] >> 31 == 1).all()
    q = np.asarray(qry, np.uint8)
    code = lambda c: int(pm.NT4[c]) + 1
    # a seed column: the query base itself; block 5's gap is "IIMM" behind the seed [10, 40): reference bases 40 and 41 face '-', 42 faces query 930
    assert int(w[10] & 7) == code(q[900]) and int(w[40] & 7) == 6 and int(w[41] & 7) == 6 and int(w[42] & 7) == code(q[930])
    # reverse strand: forward position 499 faces query 400 as stored, complemented
    assert int(w[499] & 7) == 5 - code(q[400])
    # each block alone stays inside its sequence too, and a result without blocks paints nothing
    for bi in range(6):
        o = np.zeros(G, np.uint32); hostlib.project(px, qry, one_block(dump, bi), o)
        c = int(dump["b_chr"][bi]); lo = 0 if c == 0 else 400; hi = 400 if c == 0 else 700
        assert o[:lo].sum() == 0 and o[hi:].sum() == 0 and (o != 0).any()
    e = np.zeros(G, np.uint32)
    assert hostlib.project(px, qry, {k: v[:0] for k, v in dump.items()}, e) == (0, 0) and not e.any()
    with pytest.raises(RuntimeError):
        hostlib.project(px, qry, dump, np.zeros(G - 1, np.uint32))


def test_proj_fasta_text(golden_dir, golden_results):
    """Emitter::proj_text: one record per reference sequence, names as the .ann round trip delivers them, 60 columns, a short last line"""
    px, idx, res = golden_results["small"]
    G = int(idx.G)
    w = np.zeros(G, np.uint32)
    for qn, seq, d, _ in res:
        hostlib.project(px, seq, d, w)
    txt = hostlib.emit_proj(px, w)
    assert txt == pj.fasta_of(w, idx.chr_names, idx.chr_len)
    assert txt == pj.proj_fasta(os.path.join(golden_dir, "small.maf"), idx.chr_names, idx.chr_len)
    recs = txt.split(b">")[1:]
    assert [r.split(b"\n", 1)[0].decode() for r in recs] == list(idx.chr_names)
    for r, L in zip(recs, idx.chr_len.tolist()):
        lines = r.split(b"\n")[1:]
        assert lines[-1] == b"" and all(len(x) == 60 for x in lines[:-2]) and len(lines[-2]) == (L - 1) % 60 + 1 and sum(len(x) for x in lines) == L
    assert set(txt.replace(b"\n", b"")) - set(b">") >= set(b"ACGT")
