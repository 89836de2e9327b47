"""Helpers of the CIGAR / PAF tests (no tests in here): the PAF a MAF file implies, derived from nothing but the MAF's own lines.

The CIGAR of a block is the run-length encoding of the columns of its two `s` lines (include/gsa_hip.h): I where the reference row holds '-',
D where the query row does, = where both hold the same one of A/C/G/T in any case, X for every other pair.  The PAF line carries the MAF
line's own coordinates, the query's turned onto its forward strand."""
import numpy as np

NT4 = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    NT4[ord(_c)] = _i; NT4[ord(_c.lower())] = _i
CODE = {"I": 1, "D": 2, "=": 7, "X": 8}
LETTER = {v: k for k, v in CODE.items()}


def column_classes(t1: bytes, t2: bytes) -> np.ndarray:
    """BAM op code per column of the reference row t1 / the query row t2"""
    a = np.frombuffer(t1, np.uint8); b = np.frombuffer(t2, np.uint8)
    assert a.size == b.size
    x, y = NT4[a], NT4[b]
    cls = np.where((x == y) & (x < 4), 7, 8).astype(np.uint8)
    cls[b == 0x2D] = 2
    cls[a == 0x2D] = 1
    return cls


def rle(cls: np.ndarray):
    """[(code, length)] of a class-per-column array"""
    if cls.size == 0:
        return []
    cut = np.flatnonzero(np.diff(cls)) + 1
    starts = np.concatenate([[0], cut]); ends = np.concatenate([cut, [cls.size]])
    return [(int(cls[s]), int(e - s)) for s, e in zip(starts, ends)]


def ops_of(runs) -> np.ndarray:
    return np.array([(n << 4) | c for c, n in runs], np.uint32)


def cg_of(runs) -> str:
    return "".join(f"{n}{LETTER[c]}" for c, n in runs)


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


def paf_line(score, ref, qry):
    """One PAF line (no newline) and its runs.  A duplicate block is printed with score=1 by OutputMAF (no real block scores that low): tp:A:S."""
    rname, rstart, rsize, rstrand, rsrc, t1 = ref
    qname, qstart, qsize, qstrand, qsrc, t2 = qry
    assert rname.startswith("ref.") and qname.startswith("qry.") and rstrand == "+"
    runs = rle(column_classes(t1, t2))
    n = {c: sum(l for k, l in runs if k == c) for c in (1, 2, 7, 8)}
    assert n[7] + n[8] + n[2] == rsize and n[7] + n[8] + n[1] == qsize
    qs, qe = (qstart, qstart + qsize) if qstrand == "+" else (qsrc - qstart - qsize, qsrc - qstart)
    f = [qname[4:], qsrc, qs, qe, qstrand, rname[4:], rsrc, rstart, rstart + rsize, n[7], len(t1), 255,
         f"NM:i:{n[8] + n[1] + n[2]}", f"AS:i:{score}", "tp:A:S" if score == 1 else "tp:A:P", "cg:Z:" + cg_of(runs)]
    return "\t".join(str(x) for x in f), runs


def paf_of_maf(path) -> bytes:
    return "".join(paf_line(*b)[0] + "\n" for b in maf_blocks(path)).encode()
