"""The band class of the gap DP (gsalign_amd/csrc/k_dp_band.hip) restated for the tests, from the REFERENCE's alignments only: which jobs the layout
admits, and which of them the certificate keeps.  A job is certified exactly when the full-matrix optimum -- the score of the reference's own gapped
strings -- exceeds UB = min(m, n) - |n - m| - 3 (B + 1) - 4: a path that leaves the band scores at most UB, so an optimum above UB is found inside
the band, and an optimum at or below UB bounds the band score too."""
import numpy as np

DIAGS = 128
MAX_LEN = 5000


def fits(m, n, B):
    """the layout admits an m x n job: its band, from an even diagonal at or below min(0, n - m) - B up to max(0, n - m) + B, has at most 128 diagonals"""
    lo = min(0, n - m) - B
    base = lo - (lo & 1)
    return 1 <= m <= MAX_LEN and 1 <= n <= MAX_LEN and max(0, n - m) + B - base + 1 <= DIAGS


def ub(m, n, B):
    return min(m, n) - abs(n - m) - 3 * (B + 1) - 4


def is_striped(m, n):
    """the job belongs to the striped kernel's class (k_dp.hip: not n <= 64 and m + n - 1 <= 128)"""
    return not (n <= 64 and m + n - 1 <= 128)


def score_of(g1, g2):
    """score of two gapped strings: match 1, mismatch -1, a column with an N 0, a gap of k columns 2 + k"""
    a = np.frombuffer(g1, np.uint8); b = np.frombuffer(g2, np.uint8)
    ga, gb = a == 45, b == 45
    both = ~(ga | gb)
    ua, ubb = a | 0x20, b | 0x20
    acgt = lambda x: (x == 97) | (x == 99) | (x == 103) | (x == 116)
    real = both & acgt(ua) & acgt(ubb)
    sc = int((real & (ua == ubb)).sum()) - int((real & (ua != ubb)).sum())
    for g in (ga, gb):
        x = np.diff(np.concatenate([[0], g.astype(np.int8), [0]]))
        sc -= 2 * int((x == 1).sum()) + int(g.sum())
    return sc


def certified(m, n, B, gapped):
    """what the band kernel must decide for an admitted job whose reference alignment is `gapped`"""
    return score_of(*gapped) > ub(m, n, B)


def ops_of(g1, g2):
    """M / D / I string of two gapped strings ('D': '-' in the first row)"""
    a = np.frombuffer(g1, np.uint8); b = np.frombuffer(g2, np.uint8)
    o = np.full(a.size, ord("M"), np.uint8)
    o[a == 45] = ord("D"); o[b == 45] = ord("I")
    return o.tobytes()
