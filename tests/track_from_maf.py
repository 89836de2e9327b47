"""Helpers of the track tests (no tests in here): the per-window reference track a MAF file implies, derived from nothing but the MAF's own `s` lines.

A block counts unless its score is 1 (OutputMAF prints a duplicate that way).  Every column that holds a reference base counts, by its class (the rule of
paf_from_maf.column_classes: = / X / D), in the window of that base; a column whose reference row holds '-' (class I) counts as one inserted base in the window of
the reference base consumed last in front of it in WALK order.  The MAF prints a reverse-strand block reverse-complemented: its columns run against the walk, so that
base is the one printed next behind the column (the rule of lift_from_maf.block_lift).  The MAF text is trimmed (iExtension), and so is the coverage derived from it.
Windows restart at every reference sequence."""
import numpy as np

import paf_from_maf as pm

TRACK_DT = np.dtype([("chr", "<i4"), ("start", "<i4"), ("len", "<i4"), ("n_cov", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_del", "<u4"), ("n_ins", "<u4")])
FIELDS = ("n_eq", "n_x", "n_del", "n_ins")
CODE_FIELD = {7: 0, 8: 1, 2: 2}


def block_columns(ref, qry):
    """One MAF block -> (local reference position int64[], field int8[]) per counted column: field 0 '=', 1 'X', 2 'D' at the column's own base, 3 'I' at the base
    consumed last in front of it in walk order"""
    _, rstart, rsize, rstrand, _, t1 = ref
    qstrand, t2 = qry[3], qry[5]
    assert rstrand == "+"
    cls = pm.column_classes(t1, t2)
    rc = np.frombuffer(t1, np.uint8) != 0x2D
    assert int(rc.sum()) == rsize
    nr = np.cumsum(rc) - rc                                  # reference bases printed in front of every column
    at = rstart + np.where(rc, nr, nr - 1 if qstrand == "+" else nr).astype(np.int64)
    fld = np.full(cls.size, 3, np.int8)
    for code, f in CODE_FIELD.items():
        fld[cls == code] = f
    assert ((fld == 3) == ~rc).all()
    keep = (at >= rstart) & (at < rstart + rsize)            # (an insertion at the block's edge has no base in front of it: none in a block that starts with a seed)
    return at[keep], fld[keep]


def contig_track(blocks, chr_names, chr_len, W, score=None):
    """What the blocks of ONE query contig (maf_blocks entries) imply: a TRACK_DT array, one record per window with n_cov > 0, ascending by (chr, start).
    score: the blocks' scores if not the MAF's own (1 marks a duplicate)."""
    ci = {n: i for i, n in enumerate(chr_names)}
    chr_len = [int(x) for x in chr_len]
    nwin = [(L + W - 1) // W for L in chr_len]
    cov = [np.zeros(L, bool) for L in chr_len]
    cnt = [np.zeros((4, n), np.int64) for n in nwin]
    for bi, (sc, ref, qry) in enumerate(blocks):
        if (sc if score is None else score[bi]) == 1:
            continue
        c = ci[ref[0][4:]]
        cov[c][ref[1]:ref[1] + ref[2]] = True
        at, fld = block_columns(ref, qry)
        for f in range(4):
            cnt[c][f] += np.bincount(at[fld == f] // W, minlength=nwin[c])
    out = []
    for c, L in enumerate(chr_len):
        ncov = np.bincount(np.flatnonzero(cov[c]) // W, minlength=nwin[c])
        j = np.flatnonzero(ncov)
        T = np.zeros(j.size, TRACK_DT)
        T["chr"] = c; T["start"] = j * W; T["len"] = np.minimum((j + 1) * W, L) - j * W; T["n_cov"] = ncov[j]
        for f, name in enumerate(FIELDS):
            T[name] = cnt[c][f][j]
            assert int(cnt[c][f].sum()) == int(cnt[c][f][j].sum())      # (nothing counted in a window without coverage)
        out.append(T)
    return np.concatenate(out) if out else np.zeros(0, TRACK_DT)


def by_query(path):
    """the blocks of a MAF file per query contig, contigs in file order: [(query name, [maf_blocks entries])]"""
    by_q, order = {}, []
    for b in pm.maf_blocks(path):
        qn = b[2][0][4:].rstrip(" ")
        if qn not in by_q:
            by_q[qn] = []; order.append(qn)
        by_q[qn].append(b)
    return [(qn, by_q[qn]) for qn in order]


def track_tsv(path, chr_names, chr_len, W):
    """The text of <prefix>.track.tsv the MAF at `path` implies: per query contig in file order, per window ascending."""
    out = ["#ref\tstart\tend\tquery\tcovered\tmatch\tmismatch\tdeleted\tinserted\n"]
    for qn, bl in by_query(path):
        for t in contig_track(bl, chr_names, chr_len, W):
            out.append(f"{chr_names[int(t['chr'])]}\t{int(t['start'])}\t{int(t['start']) + int(t['len'])}\t{qn}\t{int(t['n_cov'])}\t{int(t['n_eq'])}\t{int(t['n_x'])}\t{int(t['n_del'])}\t{int(t['n_ins'])}\n")
    return "".join(out)
