"""Helpers of the query-track tests (no tests in here): the per-window track over the QUERY contig that a MAF file implies, derived from nothing but the MAF's own `s` lines.

A block counts unless its score is 1 (OutputMAF prints a duplicate that way).  Positions are 0-based in the contig as stored: the MAF prints a '-' strand query line
reverse-complemented, with its start counted from the other end, so its k-th printed base is stored base srcSize - 1 - (start + k).  Every column that holds a query
base counts, by its class (the rule of paf_from_maf.column_classes: = / X / I), in the window of that base; a column whose query row holds '-' (class D) counts as
one deleted base in the window of the query base consumed last in front of it in WALK order.  The walk runs forward in the stored contig, so on a '-' strand block it
runs against the printed columns and that base is the one printed next behind the column.  A block covers the stored interval of its query line."""
import numpy as np

import paf_from_maf as pm

QTRACK_DT = np.dtype([("start", "<i4"), ("len", "<i4"), ("n_cov", "<u4"), ("n_multi", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4")])
FIELDS = ("n_eq", "n_x", "n_ins", "n_del")
CODE_FIELD = {7: 0, 8: 1, 1: 2}
HEADER = "#query\tstart\tend\tcovered\tmulti\tmatch\tmismatch\tinserted\tdeleted\n"


def block_columns(ref, qry):
    """One MAF block -> (stored contig position int64[], field int8[]) per column: field 0 '=', 1 'X', 2 'I' at the column's own query base, 3 'D' at the query base
    consumed last in front of it in walk order; and the stored interval [lo, hi) of the block's query bases"""
    t1 = ref[5]
    _, qstart, qsize, qstrand, qsrc, t2 = qry
    cls = pm.column_classes(t1, t2)
    qc = np.frombuffer(t2, np.uint8) != 0x2D
    assert int(qc.sum()) == qsize
    nq = np.cumsum(qc) - qc                                  # query bases printed in front of every column
    k = np.where(qc, nq, nq - 1 if qstrand == "+" else nq).astype(np.int64)      # the printed index of the base a column is charged to
    at = qstart + k if qstrand == "+" else qsrc - 1 - (qstart + k)
    lo, hi = (qstart, qstart + qsize) if qstrand == "+" else (qsrc - qstart - qsize, qsrc - qstart)
    fld = np.full(cls.size, 3, np.int8)
    for code, f in CODE_FIELD.items():
        fld[cls == code] = f
    assert ((fld == 3) == ~qc).all()
    assert ((at >= lo) & (at < hi)).all()                    # (a block starts and ends with a seed: a deletion has a query base on either side)
    return at, fld, lo, hi


def contig_qtrack(blocks, qlen, W, score=None):
    """What the blocks of ONE query contig (maf_blocks entries) imply: a QTRACK_DT array, one record per window with n_cov > 0, ascending by start.
    score: the blocks' scores if not the MAF's own (1 marks a duplicate)."""
    qlen = int(qlen)
    nwin = (qlen + W - 1) // W
    depth = np.zeros(qlen, np.int64)
    cnt = np.zeros((4, nwin), np.int64)
    for bi, (sc, ref, qry) in enumerate(blocks):
        if (sc if score is None else score[bi]) == 1:
            continue
        assert qry[4] == qlen
        at, fld, lo, hi = block_columns(ref, qry)
        depth[lo:hi] += 1
        for f in range(4):
            cnt[f] += np.bincount(at[fld == f] // W, minlength=nwin)
    ncov = np.bincount(np.flatnonzero(depth >= 1) // W, minlength=nwin)
    nmul = np.bincount(np.flatnonzero(depth >= 2) // W, minlength=nwin)
    j = np.flatnonzero(ncov)
    T = np.zeros(j.size, QTRACK_DT)
    T["start"] = j * W; T["len"] = np.minimum((j + 1) * W, qlen) - j * W; T["n_cov"] = ncov[j]; T["n_multi"] = nmul[j]
    for f, name in enumerate(FIELDS):
        T[name] = cnt[f][j]
        assert int(cnt[f].sum()) == int(cnt[f][j].sum())     # (nothing counted in a window without coverage)
    return T


def by_query(path):
    """the blocks of a MAF file per query contig, contigs in file order: [(query name, contig length, [maf_blocks entries])]"""
    by_q, order = {}, []
    for b in pm.maf_blocks(path):
        qn = b[2][0][4:].rstrip(" ")
        if qn not in by_q:
            by_q[qn] = (b[2][4], []); order.append(qn)
        by_q[qn][1].append(b)
    return [(qn, by_q[qn][0], by_q[qn][1]) for qn in order]


def qtrack_tsv(path, W):
    """The text of <prefix>.qtrack.tsv the MAF at `path` implies: per query contig in file order, per window ascending."""
    out = [HEADER]
    for qn, qlen, bl in by_query(path):
        for t in contig_qtrack(bl, qlen, W):
            out.append(f"{qn}\t{int(t['start'])}\t{int(t['start']) + int(t['len'])}\t{int(t['n_cov'])}\t{int(t['n_multi'])}\t{int(t['n_eq'])}\t{int(t['n_x'])}\t{int(t['n_ins'])}\t{int(t['n_del'])}\n")
    return "".join(out)
