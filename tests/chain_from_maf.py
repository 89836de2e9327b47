"""Helper of the chain tests (no tests in here): the UCSC chain file a MAF file implies, derived from nothing but the MAF's own lines.

A block's columns are those of its two `s` lines: a column is ALIGNED where both rows hold a base, a gap column where one row holds '-' ('D' where the
query row does: a reference base faces the gap; 'I' where the reference row does).  A chain neither starts nor ends with a gap: gap columns at either edge
are stripped and the `s` line's coordinates shrink by the bases they held.  What is left is cut into maximal runs of aligned columns, {size, dt, dq} with the
gap BEHIND the run, the last one bare.  Header fields are the `s` lines' own (names without their "ref." / "qry." prefix, starts, source sizes, the query's
strand; for '-' the MAF start already counts on the reverse strand, as a chain's does), the score is the `a` line's, ids count from 1 over the file."""
import numpy as np


def maf_blocks(path):
    """[(score, (name, start, size, strand, src_size, text) of the reference line, the same of the query line)]"""
    out, cur = [], None
    for ln in open(path, "rb").read().split(b"\n"):
        if ln.startswith(b"a score="):
            cur = [int(ln[8:]), None, None]
        elif ln.startswith(b"s ") and cur is not None:
            f = ln.split()
            rec = (f[1].decode(), int(f[2]), int(f[3]), f[4].decode(), int(f[5]), f[6] if len(f) > 6 else b"")
            if cur[1] is None:
                cur[1] = rec
            else:
                cur[2] = rec; out.append(tuple(cur)); cur = None
    return out


def column_kinds(t1: bytes, t2: bytes) -> np.ndarray:
    """0 = aligned, 1 = D (reference base faces '-'), 2 = I (query base faces '-'), per column of the reference row t1 / the query row t2"""
    a = np.frombuffer(t1, np.uint8); b = np.frombuffer(t2, np.uint8)
    assert a.size == b.size
    k = np.zeros(a.size, np.uint8)
    k[b == 0x2D] = 1
    k[a == 0x2D] = 2
    return k


def triples_of_kinds(k: np.ndarray):
    """(triples [(size, dt, dq)], leading D, leading I, trailing D, trailing I) of a column list; no aligned column: ([], ...) with everything counted as leading"""
    al = np.flatnonzero(k == 0)
    if al.size == 0:
        return [], int((k == 1).sum()), int((k == 2).sum()), 0, 0
    lo, hi = int(al[0]), int(al[-1]) + 1
    lead, trail, core = k[:lo], k[hi:], k[lo:hi]
    out, size, dt, dq = [], 0, 0, 0
    for c in core.tolist():
        if c == 0:
            if dt or dq:
                out.append((size, dt, dq)); size, dt, dq = 0, 0, 0
            size += 1
        elif c == 1:
            dt += 1
        else:
            dq += 1
    out.append((size, 0, 0))
    return out, int((lead == 1).sum()), int((lead == 2).sum()), int((trail == 1).sum()), int((trail == 2).sum())


def block_triples(ref, qry):
    """the triples of one MAF block and its chain coordinates (tStart, tEnd, qStart, qEnd)"""
    tr, ld, li, td, ti = triples_of_kinds(column_kinds(ref[5], qry[5]))
    ts, te = ref[1] + ld, ref[1] + ref[2] - td
    qs, qe = qry[1] + li, qry[1] + qry[2] - ti
    return tr, (ts, te, qs, qe)


def chain_text(tr, score, ref, qry, coords, cid) -> str:
    assert ref[0].startswith("ref.") and qry[0].startswith("qry.") and ref[3] == "+"
    ts, te, qs, qe = coords
    assert te - ts == sum(s + dt for s, dt, _ in tr) and qe - qs == sum(s + dq for s, _, dq in tr)
    lines = [f"chain {score} {ref[0][4:]} {ref[4]} + {ts} {te} {qry[0][4:]} {qry[4]} {qry[3]} {qs} {qe} {cid}"]
    lines += [f"{s}\t{dt}\t{dq}" for s, dt, dq in tr[:-1]] + [str(tr[-1][0]), ""]
    return "\n".join(lines) + "\n"


def chain_of_maf(path) -> bytes:
    out, cid = [], 0
    for score, ref, qry in maf_blocks(path):
        tr, coords = block_triples(ref, qry)
        if not tr:
            continue      # a block left without an aligned column prints nothing and takes no id
        cid += 1
        out.append(chain_text(tr, score, ref, qry, coords, cid))
    return "".join(out).encode()
