"""Helpers of the region-lift tests (no tests in here): where a MAF file says every reference INTERVAL lies on the query and how its columns are classed, derived from
nothing but the MAF's own `s` lines.

A block covers the forward reference positions its reference line names (the MAF text is trimmed by iExtension, and so is the coverage derived from it).  The span of
a region under a block is one interval of those positions; its columns are the block's columns from the one that holds the span's first base through the one that holds
its last, both included -- the same set whichever way the block is printed, so the four class counts (paf_from_maf.column_classes) do not depend on the strand.  The
query interval does: the MAF prints a reverse-strand block reverse-complemented, its columns run against the walk and its query coordinates count on the '-' strand, so a
base printed at coordinate c lies at size - 1 - c in the contig as stored, and the span's first column in WALK order is the one printed last (lift_from_maf's rule)."""
import numpy as np

import paf_from_maf as pm

HEADER = "#ref\tstart\tend\tname\tcstart\tcend\tquery\tqstart\tqend\tstrand\tmatch\tmismatch\tdeleted\tinserted\tscore\tn_cover\n"


class BlockColumns:
    """One MAF block (the two `s` records of paf_from_maf.maf_blocks): its forward global reference interval [g0, g1), the column of every reference base, and prefix
    counts over its printed columns."""

    def __init__(self, ref, qry, chr_start):
        rname, rstart, rsize, rstrand, _, t1 = ref
        _, qstart, qsize, qstrand, qsrc, t2 = qry
        assert rname.startswith("ref.") and rstrand == "+"
        cls = pm.column_classes(t1, t2)
        a = np.frombuffer(t1, np.uint8); b = np.frombuffer(t2, np.uint8)
        rc, qc = a != 0x2D, b != 0x2D
        assert int(rc.sum()) == rsize and int(qc.sum()) == qsize
        self.g0 = chr_start[rname[4:]] + rstart; self.g1 = self.g0 + rsize
        self.rev = qstrand == "-"
        self.qstart, self.qsrc = qstart, qsrc
        self.cols = np.flatnonzero(rc)
        z = np.zeros(1, np.int64)
        self.pre = {c: np.concatenate([z, np.cumsum(cls == c)]) for c in (7, 8, 2, 1)}      # columns of class c in front of column j
        self.nq = np.concatenate([z, np.cumsum(qc)])                                        # query bases printed in front of column j

    def spans(self, lo, hi):
        """forward global spans [lo, hi) inside [g0, g1) (int64 arrays) -> dict of arrays n_eq, n_x, n_del, n_ins, q_lo, q_hi"""
        cs = self.cols[lo - self.g0]; ce = self.cols[hi - 1 - self.g0]
        out = {k: (self.pre[c][ce + 1] - self.pre[c][cs]) for k, c in (("n_eq", 7), ("n_x", 8), ("n_del", 2), ("n_ins", 1))}
        q0 = self.qstart + self.nq[cs]; q1 = self.qstart + self.nq[ce + 1]      # the span's query bases in printed coordinates [q0, q1)
        assert np.array_equal(q1 - q0, out["n_eq"] + out["n_x"] + out["n_ins"])
        out["q_lo"] = self.qsrc - q1 if self.rev else q0
        out["q_hi"] = out["q_lo"] + (q1 - q0)
        return out


FIELDS = ("block", "off_lo", "off_hi", "q_lo", "q_hi", "n_eq", "n_x", "n_del", "n_ins", "rev", "n_cover")


def contig_regions(blocks, chr_start, bdup, score, beg, end):
    """What the blocks of ONE query contig (maf_blocks entries in result order; bdup / score: the result's own values per block, the keys of the choice) imply for the
    regions [beg[i], end[i]) under the choice rule of gsa_lift_regions: a dict of int64 arrays over the regions (block -1: no block overlaps), plus `by_overlap`: the
    choice went AGAINST the score -- some overlapping block that is no duplicate scores higher than the chosen one and overlaps less."""
    beg = np.asarray(beg, np.int64); end = np.asarray(end, np.int64)
    n = beg.size
    r = {k: np.zeros(n, np.int64) for k in FIELDS}
    r["block"][:] = -1; r["q_lo"][:] = -1; r["q_hi"][:] = -1
    cur_dup = np.zeros(n, np.int64); cur_ov = np.zeros(n, np.int64); cur_sc = np.zeros(n, np.int64)
    cols = [BlockColumns(ref, qry, chr_start) for _, ref, qry in blocks]
    for bi, bc in enumerate(cols):
        lo = np.maximum(beg, bc.g0); hi = np.minimum(end, bc.g1)
        ov = hi - lo
        m = ov > 0
        r["n_cover"][m] += 1
        dup, sc = int(bdup[bi] != 0), int(score[bi])
        better = m & ((r["block"] < 0) | (dup < cur_dup) | ((dup == cur_dup) & ((ov > cur_ov) | ((ov == cur_ov) & (sc > cur_sc)))))      # (ties: the smaller index, which came first)
        w = np.flatnonzero(better)
        if w.size == 0:
            continue
        s = bc.spans(lo[w], hi[w])
        for k, v in s.items():
            r[k][w] = v
        r["block"][w] = bi; r["rev"][w] = int(bc.rev); r["off_lo"][w] = lo[w] - beg[w]; r["off_hi"][w] = hi[w] - beg[w]
        cur_dup[w] = dup; cur_ov[w] = ov[w]; cur_sc[w] = sc
    r["n_cover"] = np.minimum(r["n_cover"], 65535)
    by_ov = np.zeros(n, bool)
    for bi, bc in enumerate(cols):
        ov = np.minimum(end, bc.g1) - np.maximum(beg, bc.g0)
        by_ov |= (r["block"] >= 0) & (r["block"] != bi) & (cur_dup == 0) & (int(bdup[bi] != 0) == 0) & (ov > 0) & (ov < cur_ov) & (int(score[bi]) > cur_sc)
    r["by_overlap"] = by_ov
    return r


def dense(H, n):
    """REGION_HIT_DT hits -> the dict contig_regions gives (without by_overlap), over the n input regions"""
    assert (np.diff(H["idx"]) > 0).all() and (H.size == 0 or (H["idx"][0] >= 0 and H["idx"][-1] < n))
    assert (H["_pad0"] == 0).all() and (H["_pad1"] == 0).all() and (H["block"] >= 0).all()
    r = {k: np.zeros(n, np.int64) for k in FIELDS}
    r["block"][:] = -1; r["q_lo"][:] = -1; r["q_hi"][:] = -1
    for k in FIELDS:
        r[k][H["idx"]] = H[k]
    return r


def stride_regions(chr_len, lengths=(1, 2, 63, 64, 65, 1000), stride=7):
    """all regions of the given lengths at the given stride inside every reference sequence, then every whole sequence: (beg, end) in forward global coordinates"""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    b, e = [], []
    for L in lengths:
        for c, n in enumerate(np.asarray(chr_len).tolist()):
            s = np.arange(0, n - L + 1, stride, dtype=np.int64)
            b.append(starts[c] + s); e.append(starts[c] + s + L)
    b.append(starts[:-1]); e.append(starts[1:])
    return np.concatenate(b), np.concatenate(e)


def gap_record_regions(d, chr_len):
    """from a result dump (oracle layout): every [a, b) with both ends inside one gap record's reference bases, for every gap record, in forward global coordinates and
    cut to the record's reference sequence"""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    G = int(starts[-1])
    blk_of = np.repeat(np.arange(d["b_nfrag"].size), d["b_nfrag"])
    b, e = [], []
    for i in np.flatnonzero((d["f_bseed"] == 0) & (d["f_rlen"] > 0)):
        bi = int(blk_of[i]); c = int(d["b_chr"][bi])
        t0 = int(d["f_rpos"][i]); t1 = t0 + int(d["f_rlen"][i])
        p0, p1 = (t0, t1) if d["b_bdir"][bi] else (2 * G - t1, 2 * G - t0)
        p0 = max(p0, int(starts[c])); p1 = min(p1, int(starts[c + 1]))
        if p1 <= p0:
            continue
        a = np.arange(p0, p1, dtype=np.int64)
        ia, ib = np.triu_indices(a.size)
        b.append(a[ia]); e.append(a[ib] + 1)
    if not b:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(b), np.concatenate(e)


def end_records(d, G, H, beg, end):
    """for the hits H of the regions (beg, end) on the result dump d: the indices (into the dump's records) of the records that hold the span's first and last
    reference base, and whether each is a gap record"""
    f_at = np.concatenate([[0], np.cumsum(d["b_nfrag"])]).astype(np.int64)
    iA = np.zeros(H.size, np.int64); iB = np.zeros(H.size, np.int64)
    p_lo = beg[H["idx"]] + H["off_lo"]; p_hi = beg[H["idx"]] + H["off_hi"]
    t_lo = np.where(H["rev"] != 0, 2 * G - p_hi, p_lo); t_hi = np.where(H["rev"] != 0, 2 * G - p_lo, p_hi)
    for bi in np.unique(H["block"]):
        m = H["block"] == bi
        rp = d["f_rpos"][f_at[bi]:f_at[bi + 1]].astype(np.int64)
        iA[m] = f_at[bi] + np.searchsorted(rp, t_lo[m], side="right") - 1
        iB[m] = f_at[bi] + np.searchsorted(rp, t_hi[m] - 1, side="right") - 1
    gap = d["f_bseed"] == 0
    return iA, iB, gap[iA], gap[iB], t_lo, t_hi


def regions_tsv(path, chr_names, chr_len, beg, end, names=None):
    """The text of <prefix>.regions.tsv for a run whose BED file lists the regions (beg, end) (forward global coordinates) in order, derived from the MAF at `path`: per
    query contig in file order, per region in input order, the hit the MAF's blocks of that contig imply.  The choice keys are the MAF's own: score = 1 marks a duplicate."""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    chr_start = {n: int(s) for n, s in zip(chr_names, starts)}
    beg = np.asarray(beg, np.int64); end = np.asarray(end, np.int64)
    chr_of = np.searchsorted(starts, beg, side="right") - 1
    by_q, order = {}, []
    for b in pm.maf_blocks(path):
        qn = b[2][0][4:].rstrip(" ")
        if qn not in by_q:
            by_q[qn] = []; order.append(qn)
        by_q[qn].append(b)
    out = [HEADER]
    for qn in order:
        bl = by_q[qn]
        sc = [b[0] for b in bl]
        r = contig_regions(bl, chr_start, [s == 1 for s in sc], sc, beg, end)
        for i in np.flatnonzero(r["block"] >= 0):
            c = int(chr_of[i]); s0 = int(beg[i] - starts[c])
            out.append(f"{chr_names[c]}\t{s0}\t{int(end[i] - starts[c])}\t{names[i] if names is not None else '.'}\t{s0 + int(r['off_lo'][i])}\t{s0 + int(r['off_hi'][i])}\t{qn}\t"
                       f"{int(r['q_lo'][i])}\t{int(r['q_hi'][i])}\t{'-' if r['rev'][i] else '+'}\t{int(r['n_eq'][i])}\t{int(r['n_x'][i])}\t{int(r['n_del'][i])}\t{int(r['n_ins'][i])}\t"
                       f"{sc[int(r['block'][i])]}\t{int(r['n_cover'][i])}\n")
    return "".join(out)


def bed_text(chr_names, chr_len, beg, end, names=None):
    """the BED lines of the regions (beg, end) given in forward global coordinates; names[i]: what follows the end (None: nothing)"""
    starts = np.concatenate([[0], np.cumsum(chr_len)]).astype(np.int64)
    c = np.searchsorted(starts, np.asarray(beg, np.int64), side="right") - 1
    return "".join(f"{chr_names[int(k)]}\t{int(b - starts[k])}\t{int(e - starts[k])}" + (f"\t{names[i]}" if names is not None and names[i] is not None else "") + "\n" for i, (k, b, e) in enumerate(zip(c, beg, end)))
