"""Helpers of the lift tests (no tests in here): where a MAF file says every reference position lies on the query, derived from nothing but the MAF's own `s` lines.

A column of a block that holds a reference base lifts that base: to the query base it faces (class = or X, the rule of paf_from_maf.column_classes), or -- where
the query row holds '-' (class D) -- to the query base consumed last in front of the column in WALK order.  The MAF prints a reverse-strand block reverse-complemented:
its columns run against the walk, its query coordinates count on the '-' strand, so the position in the contig as stored is size - 1 - coordinate, and the base consumed
last in front of a column in walk order is the one printed next behind it.  The MAF text is trimmed (iExtension), and so is the coverage derived from it."""
import numpy as np

import paf_from_maf as pm

CLASS_LETTER = {7: "=", 8: "X", 2: "D"}


def block_lift(ref, qry, chr_start):
    """One MAF block (the two `s` records of paf_from_maf.maf_blocks) -> (pos int64[], qpos int32[], cls uint8[], rev): the 0-based forward global reference positions
    the block covers (chr_start: name without "ref." -> first global position of that sequence), ascending, and for each the query position in the contig as stored
    and the class of its column."""
    rname, rstart, rsize, rstrand, _, t1 = ref
    _, qstart, qsize, qstrand, qsrc, t2 = qry
    assert rname.startswith("ref.") and rstrand == "+"
    cls = pm.column_classes(t1, t2)
    a = np.frombuffer(t1, np.uint8); b = np.frombuffer(t2, np.uint8)
    rc, qc = a != 0x2D, b != 0x2D
    assert int(rc.sum()) == rsize and int(qc.sum()) == qsize
    nq = np.cumsum(qc) - qc                                   # query bases printed in front of every column
    cols = np.flatnonzero(rc)
    pos = chr_start[rname[4:]] + rstart + np.arange(cols.size, dtype=np.int64)
    if qstrand == "+":
        q = qstart + nq[cols] - (~qc[cols]).astype(np.int64)      # a D column: the base in front of it
    else:
        q = qsrc - 1 - (qstart + nq[cols])                        # a D column: the base printed next, which the walk consumed last
    return pos, q.astype(np.int32), cls[cols], qstrand == "-"


def contig_lifts(blocks, chr_start, G, bdup, score):
    """What the blocks of ONE query contig (maf_blocks entries in result order; bdup / score: the result's own values per block, the keys of the choice) imply for every
    reference position [0, G) under the choice rule of gsa_lift: arrays qpos, cls (0: not covered), rev, block, n_cover."""
    qpos = np.full(G, -1, np.int32); cls = np.zeros(G, np.uint8); rev = np.zeros(G, np.uint8); blk = np.full(G, -1, np.int32); ncov = np.zeros(G, np.int64)
    cur_dup = np.zeros(G, np.int64); cur_score = np.zeros(G, np.int64)
    for bi, (_, ref, qry) in enumerate(blocks):
        p, q, c, r = block_lift(ref, qry, chr_start)
        ncov[p] += 1
        dup, sc = int(bdup[bi] != 0), int(score[bi])
        better = (blk[p] < 0) | (dup < cur_dup[p]) | ((dup == cur_dup[p]) & (sc > cur_score[p]))      # (ties: the smaller index, which came first)
        w = p[better]
        qpos[w] = q[better]; cls[w] = c[better]; rev[w] = r; blk[w] = bi; cur_dup[w] = dup; cur_score[w] = sc
    return qpos, cls, rev, blk, np.minimum(ncov, 65535).astype(np.uint16)


def lift_tsv(path, chr_names, chr_len, allow_dup=True):
    """The text of <prefix>.lift.tsv for a run whose position file lists EVERY reference position in order, derived from the MAF at `path`: per query contig in file order,
    per position in input order, the hit the MAF's blocks of that contig imply.  The choice keys are the MAF's own: score = 1 marks a duplicate."""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    chr_start = {n: int(s) for n, s in zip(chr_names, starts)}
    G = int(starts[-1])
    by_q, order = {}, []
    for b in pm.maf_blocks(path):
        qn = b[2][0][4:].rstrip(" ")
        if qn not in by_q:
            by_q[qn] = []; order.append(qn)
        by_q[qn].append(b)
    chr_of = np.repeat(np.arange(len(chr_names)), chr_len)
    out = ["#ref\tpos\tquery\tqpos\tstrand\tclass\tscore\tn_cover\n"]
    for qn in order:
        bl = by_q[qn]
        sc = [b[0] for b in bl]
        qpos, cls, rev, blk, ncov = contig_lifts(bl, chr_start, G, [s == 1 for s in sc], sc)
        for p in np.flatnonzero(cls):
            c = int(chr_of[p])
            out.append(f"{chr_names[c]}\t{p - starts[c] + 1}\t{qn}\t{int(qpos[p]) + 1}\t{'-' if rev[p] else '+'}\t{CLASS_LETTER[int(cls[p])]}\t{sc[int(blk[p])]}\t{int(ncov[p])}\n")
    return "".join(out)
