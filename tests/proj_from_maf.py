"""Helpers of the projection tests (no tests in here): the accumulator words of gsa_project (include/gsa_hip.h) derived from nothing but a MAF file's own `s` lines.

A column of a block that holds a reference base offers key | code to that base's word: the code of the character the query row prints there (A C G T in either case
1..4, '-' 6, anything else 5 -- the MAF prints a reverse-strand block reverse-complemented, so its query row is already the complemented one and its reference row counts
forward), the key from the block's (bdup, score); the word keeps the maximum.  The MAF text is trimmed (iExtension), and so is the coverage derived from it."""
import numpy as np

import paf_from_maf as pm

LETTERS = np.frombuffer(b"nACGTN-?", np.uint8)


def key_of(bdup, score) -> int:
    return ((0 if bdup else 1) << 31) | (min(max(int(score), 0), (1 << 28) - 1) << 3)


def block_words(ref, qry, chr_start, key):
    """One MAF block (the two `s` records of paf_from_maf.maf_blocks) -> (pos int64[], words uint32[]): the 0-based forward global reference positions the block covers
    (chr_start: name without "ref." -> first global position of that sequence) and what it offers to each."""
    rname, rstart, rsize, rstrand, _, t1 = ref
    t2 = qry[5]
    assert rname.startswith("ref.") and rstrand == "+"
    a = np.frombuffer(t1, np.uint8); b = np.frombuffer(t2, np.uint8)
    cols = np.flatnonzero(a != 0x2D)
    assert cols.size == rsize
    pos = chr_start[rname[4:]] + rstart + np.arange(cols.size, dtype=np.int64)
    code = np.where(b[cols] == 0x2D, 6, pm.NT4[b[cols]].astype(np.uint32) + 1).astype(np.uint32)
    return pos, (np.uint32(key) | code).astype(np.uint32)


def contig_words(blocks, chr_start, words, bdup, score, no_dup=False):
    """The blocks of ONE query contig (maf_blocks entries in result order; bdup / score: the result's own values per block) painted into words (uint32[G], in place)."""
    for bi, (_, ref, qry) in enumerate(blocks):
        if no_dup and bdup[bi]:
            continue
        p, w = block_words(ref, qry, chr_start, key_of(bdup[bi], score[bi]))
        np.maximum.at(words, p, w)
    return words


def text_of(words) -> bytes:
    return LETTERS[np.asarray(words, np.uint32) & 7].tobytes()


def fasta_of(words, chr_names, chr_len) -> bytes:
    """<prefix>.proj.fa of an accumulator: one record per reference sequence, 60 characters per line"""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    out = []
    for c, name in enumerate(chr_names):
        t = text_of(words[int(starts[c]):int(starts[c + 1])])
        out.append(b">" + name.encode() + b"\n" + b"".join(t[i:i + 60] + b"\n" for i in range(0, len(t), 60)))
    return b"".join(out)


def proj_fasta(path, chr_names, chr_len) -> bytes:
    """The text of <prefix>.proj.fa derived from the MAF at `path` alone, all query contigs together.  The keys are the MAF's own: score = 1 marks a duplicate, and the
    score is the printed (trimmed) one -- the same order as the result's wherever overlapping blocks do not differ by less than a trim."""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    chr_start = {n: int(s) for n, s in zip(chr_names, starts)}
    words = np.zeros(int(starts[-1]), np.uint32)
    bl = pm.maf_blocks(path)
    contig_words(bl, chr_start, words, [b[0] == 1 for b in bl], [b[0] for b in bl])
    return fasta_of(words, chr_names, chr_len)
