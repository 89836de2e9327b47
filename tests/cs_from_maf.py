"""Helper of the cs tests (no tests in here): the cs string (PAF's cs:Z:, short form; include/gsa_hip.h) a MAF block implies, derived from nothing but its
two `s` lines.

The columns are classified and run-length encoded by paf_from_maf (the CIGAR's rule); an '=' run of n columns prints ":n", an 'X' run "*rq" per column,
an 'I' run "+" and its query letters, a 'D' run "-" and its reference letters.  The letter of a byte is the byte lower-cased when that is one of acgt and
'n' for everything else, NUL included (the reference prints NUL for the complement of an IUPAC code on a reverse-strand block)."""
import numpy as np

import paf_from_maf as pm

LETTER = np.full(256, ord("n"), np.uint8)
for _c in "acgt":
    LETTER[ord(_c)] = ord(_c); LETTER[ord(_c.upper())] = ord(_c)


def letters(t: bytes) -> bytes:
    return LETTER[np.frombuffer(t, np.uint8)].tobytes()


def cs_of_rows(t1: bytes, t2: bytes, runs=None) -> str:
    """the cs of the reference row t1 / the query row t2"""
    if runs is None:
        runs = pm.rle(pm.column_classes(t1, t2))
    r, q = letters(t1).decode(), letters(t2).decode()
    out, at = [], 0
    for code, n in runs:
        if code == 7:
            out.append(f":{n}")
        elif code == 8:
            out.append("".join(f"*{r[i]}{q[i]}" for i in range(at, at + n)))
        elif code == 1:
            out.append("+" + q[at:at + n])
        else:
            out.append("-" + r[at:at + n])
        at += n
    assert at == len(t1) == len(t2)
    return "".join(out)


def cs_of_cols(cls, r: bytes, q: bytes) -> str:
    """the cs of a class-per-column array and the two rows' LETTERS (already lower case / 'n'; what lies under a '-' is not looked at)"""
    out, at = [], 0
    r, q = r.decode(), q.decode()
    for code, n in pm.rle(np.asarray(cls, np.uint8)):
        out.append(f":{n}" if code == 7 else "".join(f"*{r[i]}{q[i]}" for i in range(at, at + n)) if code == 8 else ("+" + q[at:at + n]) if code == 1 else ("-" + r[at:at + n]))
        at += n
    return "".join(out)


def cs_length_of_runs(runs) -> int:
    return sum(1 + len(str(n)) if c == 7 else 3 * n if c == 8 else 1 + n for c, n in runs)


def maf_cs(path):
    """[cs string] of every block of a MAF file, in file order"""
    return [cs_of_rows(b[1][5], b[2][5]) for b in pm.maf_blocks(path)]


def paf_cs_of_maf(path) -> bytes:
    """the PAF with cs:Z: a MAF file implies: paf_from_maf's line, a tab, "cs:Z:" and the block's cs"""
    return "".join(pm.paf_line(*b)[0] + "\tcs:Z:" + cs_of_rows(b[1][5], b[2][5]) + "\n" for b in pm.maf_blocks(path)).encode()
