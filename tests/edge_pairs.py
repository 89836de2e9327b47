"""Constructed query/reference pairs that sit ON the thresholds of stages 1-8 (a helper module, not a conftest).

Every case is a SEQUENCE built from pieces of one fixed reference, so every seed is one the reference program itself finds: the real
reference, the CPU restatement and the GPU are compared on the same input.  Between planted events a query differs from the reference by
substitutions at CHOSEN positions only (no small indels: they would fill the PosDiff gaps the cases are about), so seed positions, seed
lengths, PosDiff values, group counts and gap lengths follow from the construction; `predicted_seeds` restates them and the CPU tests hold
the restatement's stage output against them and against `expect`.

    refs, cases = build_cases()      # refs: [(name, uint8 array)], cases: [Case(name, params, query, expect, family)]
    q, rows, notes = leaf_query()    # the query and the windows of the gap-similarity leaf test

How a query is kept exact: positions are either COPIED reference bases or FIX positions (substituted bases, inserted / unrelated bases).  After
assembly every 15-mer of the query that contains a fix position and occurs anywhere in the text (both strands) gets one of its fix bases
changed, until none is left.  A seed is at least MinSeedLength = 15 long, so no seed contains a fix position: the seeds are exactly the runs of
copied bases between fix positions (cut at the 10 000-base chunk edges of the seed search) that are >= MinSeedLength long.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

CHUNK = 10000                     # seed-search chunk (GSAlign.cpp:5)
SLEN = 15                         # default MinSeedLength
REF_LENS = (360000, 60000, 60000)
TANDEM_AT, TANDEM_UNIT, TANDEM_N = 30000, 20, 3          # ref1: a 20-base unit three times (a seed over two units has two hits 20 apart)
KUNIT, KUNIT_AT, KUNIT_N = b"ACGTT", 20000, 60           # ref2: a 5-base unit 60 times (5-mer counts known by construction)

Case = namedtuple("Case", "name params query expect family")

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i; _CODE[_c + 32] = _i
_COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTNacgtn", b"TGCANtgcan"):
    _COMP[_a] = _b


def revcomp(s):
    return _COMP[s[::-1]]


def make_refs():
    rng = np.random.default_rng(20261)
    refs = [_ACGT[rng.integers(0, 4, size=n)] for n in REF_LENS]
    u = refs[1][TANDEM_AT:TANDEM_AT + TANDEM_UNIT].copy()
    for k in range(1, TANDEM_N):
        refs[1][TANDEM_AT + k * TANDEM_UNIT:TANDEM_AT + (k + 1) * TANDEM_UNIT] = u
    refs[2][KUNIT_AT:KUNIT_AT + len(KUNIT) * KUNIT_N] = np.frombuffer(KUNIT * KUNIT_N, np.uint8)
    return [(f"edge_ref{i}", r) for i, r in enumerate(refs)]


def _kmer_codes(seq, k=15):
    c = _CODE[seq].astype(np.int64)
    n = c.size - k + 1
    if n <= 0:
        return np.zeros(0, np.int64)
    out = np.zeros(n, np.int64)
    for j in range(k):
        out = (out << 2) | c[j:j + n]
    return out


class World:
    """The text (forward strands, then their reverse complement: 2G bases) and its sorted 15-mers."""

    def __init__(self, refs):
        self.refs = refs
        self.fwd = np.concatenate([r for _, r in refs])
        self.G = int(self.fwd.size)
        self.text = np.concatenate([self.fwd, revcomp(self.fwd)])
        self.off = np.concatenate([[0], np.cumsum([r.size for _, r in refs])]).astype(np.int64)
        self.k15 = np.unique(_kmer_codes(self.text))


class Builder:
    """A query as pieces.  src[i] = text position of a copied base, -1 at a fix position; forbid[i] = the base a fix position must not hold."""

    def __init__(self, world, seed):
        self.w = world
        self.rng = np.random.default_rng(seed)
        self.seq, self.src, self.forbid = [], [], []

    def __len__(self):
        return sum(s.size for s in self.seq)

    def copy(self, r, n, subs=(), endsub=True):
        """text[r:r+n] of the forward strand with substitutions at the offsets `subs` (and at the last base unless endsub=False)."""
        s = self.w.fwd[r:r + n].copy(); assert s.size == n
        src = np.arange(r, r + n, dtype=np.int64); fb = np.zeros(n, np.uint8)
        pos = sorted(set(int(p) for p in subs if 0 <= p < n) | ({n - 1} if endsub and n else set()))
        for p in pos:
            fb[p] = s[p]; src[p] = -1
            s[p] = _ACGT[(int(_CODE[s[p]]) + int(self.rng.integers(1, 4))) & 3]
        self.seq.append(s); self.src.append(src); self.forbid.append(fb)
        return self

    def copy_every(self, r, n, step, endsub=True):
        return self.copy(r, n, range(step - 1, n, step), endsub)

    def free(self, n):
        """n unrelated bases (an insertion, or a replaced stretch)."""
        self.seq.append(_ACGT[self.rng.integers(0, 4, size=n)]); self.src.append(np.full(n, -1, np.int64)); self.forbid.append(np.zeros(n, np.uint8))
        return self

    def lit(self, b):
        """literal bytes, kept as written (fix positions that the clean-up leaves alone: forbid = 255)."""
        a = np.frombuffer(b, np.uint8).copy()
        self.seq.append(a); self.src.append(np.full(a.size, -1, np.int64)); self.forbid.append(np.full(a.size, 255, np.uint8))
        return self

    def build(self, rev=False, clean=True):
        q = np.concatenate(self.seq); src = np.concatenate(self.src); fb = np.concatenate(self.forbid)
        if rev:
            q = revcomp(q); fb = np.where((fb == 0) | (fb == 255), fb, _COMP[fb])[::-1].copy()
            src = np.where(src >= 0, 2 * self.w.G - 1 - src, -1)[::-1].copy()
        if clean:
            self._clean(q, src, fb)
        return np.ascontiguousarray(q), src

    def _clean(self, q, src, fb):
        fix = (src < 0) & (fb != 255)
        nfix = np.concatenate([[0], np.cumsum(fix)])
        for _ in range(200):
            codes = _kmer_codes(q)
            if codes.size == 0:
                return
            at = np.searchsorted(self.w.k15, codes)
            hit = (at < self.w.k15.size) & (self.w.k15[np.minimum(at, self.w.k15.size - 1)] == codes) & (nfix[15:15 + codes.size] - nfix[:codes.size] > 0)
            idx = np.flatnonzero(hit)
            if idx.size == 0:
                return
            for i in idx:
                cand = i + np.flatnonzero(fix[i:i + 15])
                p = int(cand[int(self.rng.integers(0, cand.size))])
                while True:
                    b = _ACGT[int(self.rng.integers(0, 4))]
                    if b != q[p] and b != fb[p]:
                        q[p] = b; break
        raise AssertionError("edge_pairs: the clean-up of chance 15-mers did not converge")


def predicted_seeds(src, slen=SLEN):
    """(qpos, len, rpos) of every seed, in the reference's order (PosDiff, then qpos): runs of copied bases cut at chunk edges."""
    n = src.size
    ok = src >= 0
    brk = np.ones(n + 1, bool)
    brk[1:n] = ~(ok[1:] & ok[:-1] & (src[1:] == src[:-1] + 1)) | (np.arange(1, n) % CHUNK == 0)
    b = np.flatnonzero(brk[:-1] & ok); e = np.flatnonzero(brk[1:] & ok) + 1
    keep = e - b >= slen
    q, l = b[keep], (e - b)[keep]; r = src[q]
    o = np.lexsort((q, r - q))
    return q[o].astype(np.int32), l[o].astype(np.int32), r[o].astype(np.int64)


def groups_of(pd_sorted, ind):
    """group sizes of sorted PosDiff values: a jump of more than `ind` starts a group (SeedGrouping)."""
    if pd_sorted.size == 0:
        return []
    cut = np.flatnonzero(np.diff(pd_sorted) > ind) + 1
    return np.diff(np.concatenate([[0], cut, [pd_sorted.size]])).tolist()


def pd_jumps(qpos, rpos):
    return np.diff(np.unique(rpos.astype(np.int64) - qpos)).tolist()


# ---------------------------------------------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------------------------------------------
A_INDS = (0, 1, 2, 16, 25, 31, 32, 33, 40)


def _family_a(w, cases):
    """Group splits: consecutive PosDiff jumps of ind-1, ind, ind+1, ind+2 (then 1), by insertion and by deletion, on both strands."""
    k = 0
    for ind in A_INDS:
        sizes = [s for s in (ind - 1, ind, ind + 1, ind + 2, 1) if s > 0]
        for kind in ("ins", "del"):
            for rev in (False, True):
                b = Builder(w, 1000 + k); r = 20000 + 9000 * (k % 30); k += 1
                for s in sizes + [0]:
                    b.copy_every(r, 1500, 100); r += 1500
                    if kind == "ins":
                        b.free(s)
                    else:
                        r += s
                q, src = b.build(rev)
                up = (kind == "del") != rev           # PosDiff grows along the sorted order in the order the events were planted
                jumps = sizes if up else sizes[::-1]
                gs, cur = [], 15
                for s in jumps:
                    if s > ind:
                        gs.append(cur); cur = 0
                    cur += 15
                gs.append(cur)
                cases.append(Case(f"A_ind{ind}_{kind}_{'rev' if rev else 'fwd'}", dict(ind=ind), q,
                                  dict(src=src, pd_jumps=jumps, n_groups=len(gs), group_seeds=gs), "A"))


def bitmap_index(pd, qlen):
    """bit of a PosDiff value in the bitmap of occupied values of a single contig: key = rPos - qPos + (contig length)."""
    return pd + qlen


def _family_b(w, cases):
    """Bitmap geometry: the lower side of a jump of ind / ind+1 on the last value before a 32 / 1024 / 32768 boundary of the bitmap, and the
    upper side on the first value after it; then 33 consecutive offsets of one short contig (no formula involved)."""
    k = 0
    for ind in (25, 31):
        for J in (ind, ind + 1):
            for M in (32, 1024, 32768):
                for side in ("lo", "hi"):
                    qlen = 3000 + J
                    # first segment at r0 (PosDiff r0, the upper side), second after an insertion of J (PosDiff r0 - J, the lower side)
                    want = (M - 1 + J - qlen) % M if side == "lo" else (-qlen) % M
                    base = 40000 + 4000 * k; r0 = base + ((want - base) % M); k += 1
                    b = Builder(w, 2000 + k).copy_every(r0, 1500, 100).free(J).copy_every(r0 + 1500, 1500, 100)
                    q, src = b.build()
                    assert q.size == qlen
                    lo, hi = bitmap_index(r0 - J, qlen), bitmap_index(r0, qlen)
                    assert (lo % M == M - 1) if side == "lo" else (hi % M == 0)
                    cases.append(Case(f"B_ind{ind}_j{J}_m{M}_{side}", dict(ind=ind), q,
                                      dict(src=src, pd_jumps=[J], n_groups=1 if J <= ind else 2, group_seeds=[30] if J <= ind else [15, 15],
                                           bm_mod=M, bm_lower=lo % M, bm_upper=hi % M), "B"))
    for ind in (25, 31):
        for t in range(33):
            r = 100000 + t
            b = Builder(w, 2500 + 40 * ind + t).copy_every(r, 400, 50).free(ind).copy_every(r + 400, 400, 50).free(ind + 1).copy_every(r + 800, 400, 50)
            q, src = b.build()
            cases.append(Case(f"B_sweep_ind{ind}_o{t}", dict(ind=ind), q, dict(src=src, pd_jumps=[ind + 1, ind], n_groups=2, group_seeds=[8, 16]), "B"))


def _window_query(w, seed, r, parts, rev=False):
    """parts: (n_seeds, stride, insertion in front).  Seeds of stride-1 bases; PosDiff falls by the insertion."""
    b = Builder(w, seed)
    for n, stride, ins in parts:
        b.free(ins)
        strides = stride if isinstance(stride, (list, tuple)) else [stride] * n
        for s in strides:
            b.copy(r, s); r += s
    return b.build(rev)


def _family_c(w, cases):
    """Outlier windows: a window closes at the first unique seed whose PosDiff differs from its predecessor's once 30 unique seeds are counted AND
    the window spans MORE than 3000 query bases (GSAlign.cpp:326-337).  A: k seeds at PosDiff p; B: two at p-20; C: two at p-40; D: 35 at p-60.
    If the window closes AT B, B joins the window of D and is an outlier there (38 > MaxIndelSize from its mean, fewer than 3 in its bucket); if
    it closes only at C, B stays with A and survives.  So the seeds of stage 2 tell on which side of 30 / 3000 the count fell."""
    r = 150000
    for k in (28, 29, 30):         # the count at B's first seed is k + 1 = 29, 30, 31
        q, src = _window_query(w, 3000 + k, r, [(k, 110, 0), (2, 110, 20), (2, 110, 20), (35, 110, 20)])
        total = k + 39
        cases.append(Case(f"C_count{k + 1}", {}, q, dict(src=src, n_groups=1, group_seeds=[total], window_count=k + 1, s2_seeds=total - (2 if k + 1 >= 30 else 0)), "C"))
    for span in (2999, 3000, 3001):   # 30 seeds in A (count 31 at B), first seed of A to first seed of B exactly `span` bases
        last = span - 20 - 29 * 99
        q, src = _window_query(w, 3100 + span, r + 20000, [(30, [99] * 29 + [last], 0), (2, 110, 20), (2, 110, 20), (35, 110, 20)])
        cases.append(Case(f"C_span{span}", {}, q, dict(src=src, n_groups=1, group_seeds=[69], window_span=span, s2_seeds=69 - (2 if span > 3000 else 0)), "C"))
    for k2 in (25, 26, 27):        # the SECOND window: closed at B (29 seeds in A), then B B C C D*k2 count 4 + k2 = 29, 30, 31 at E's first seed
        parts = [(29, 110, 0), (2, 105, 20), (2, 105, 20), (k2, 105, 20), (2, 60, 20), (2, 60, 20), (35, 60, 20)]
        q, src = _window_query(w, 3200 + k2, r + 40000, parts)
        total = 29 + 4 + k2 + 4 + 35
        # window 2 closed at E: B dies in it, E dies in window 3 (40 from H's mean); closed only at F: B dies, E stays with D
        cases.append(Case(f"C_second_count{4 + k2}", {}, q, dict(src=src, n_groups=1, group_seeds=[total], window_count=4 + k2, s2_seeds=total - 2 - (2 if 4 + k2 >= 30 else 0)), "C"))
    # a multi-hit query position (a seed over two units of ref1's tandem array: hits 20 apart, one group) as the last seed before the window edge
    t0 = int(w.off[1]) + TANDEM_AT
    b = Builder(w, 3300)
    a0 = t0 - 29 * 110
    for i in range(29):
        b.copy(a0 + 110 * i, 110)
    b.copy(t0, 2 * TANDEM_UNIT + 1)                       # 40 copied bases + the substituted 41st
    rr = t0 + 2 * TANDEM_UNIT + 1
    for n, ins in ((2, 20), (2, 20), (35, 20)):
        b.free(ins)
        for _ in range(n):
            b.copy(rr, 110); rr += 110
    q, src = b.build()
    # the window closes at B (29 unique seeds + the multi-hit position in A), B dies as an outlier, and the mean of the five live unique neighbours on either
    # side (5 at p; 2 at p-40 and 3 at p-60) is p-26: one more than MaxIndelSize from the nearer hit, so NEITHER hit survives (RemoveRedundantSeeds' strict <)
    cases.append(Case("C_multihit_at_window_edge", {}, q, dict(src=src, n_groups=1, extra_hits=[(29 * 110, 2 * TANDEM_UNIT, t0 + TANDEM_UNIT)], multi_qpos=29 * 110, multi_kept=0,
                                                               neighbour_mean_off=26), "C"))


def _family_d(w, cases):
    """Block filters (AddAlnBlock, GSAlign.cpp:29-49): seed-length sum clr-1 / clr / clr+1, aligned length alen-1 / alen / alen+1."""
    r = 230000
    for clr in (200, 50):
        for d in (-1, 0, 1):
            b = Builder(w, 4000 + clr + d)
            if clr == 200:       # three seeds 60 + 60 + (80 + d), one substitution between them: 202 + d query bases
                b.copy(r, 61).copy(r + 61, 61).copy(r + 122, 80 + d, endsub=False)
            else:                # 16 + 16 + (18 + d) with stretches of 9-base runs (no seeds) between them: more than 200 query bases
                b.copy(r, 17).copy_every(r + 17, 100, 10).copy(r + 117, 17).copy_every(r + 134, 100, 10).copy(r + 234, 18 + d, endsub=False)
            q, src = b.build()
            cases.append(Case(f"D_score_clr{clr}_{clr + d}", dict(clr=clr), q, dict(src=src, n_groups=1, seed_sum=clr + d, s2_blocks=1 if d >= 0 else 0), "D"))
            r += 1000
    for d in (-1, 0, 1):         # two seeds 99 + (100 + d) and one substitution: 199 + d + 1 query bases from first to last seed base
        b = Builder(w, 4100 + d).copy(r, 100).copy(r + 100, 100 + d, endsub=False)
        q, src = b.build()
        cases.append(Case(f"D_alen_{200 + d}", dict(clr=50), q, dict(src=src, n_groups=1, region=200 + d, s2_blocks=1 if d >= 0 else 0), "D"))
        r += 1000


def _family_e(w, cases):
    """Gaps (CheckGapsBetweenSeeds, ProcessCandidateAlignment.cpp:120-156): a stretch between two seeds of one block replaced by unrelated bases,
    of 299 .. 5001 bases, on one diagonal and 10 bases off it; same-diagonal gaps with a chosen number of agreeing positions; overlaps."""
    r = 250000; k = 0
    for n in (299, 300, 301, 4999, 5000, 5001):
        for d in (0, 10):
            b = Builder(w, 5000 + k); k += 1
            b.copy_every(r, 1000, 100).free(n - 1).copy_every(r + 1000 + n - 1 - d, 1000, 100)     # the substituted last base of a seed run belongs to the gap
            q, src = b.build()
            cases.append(Case(f"E_gap{n}_{'diag' if d == 0 else 'off'}", {}, q, dict(src=src, n_groups=1, gap=(n, n - d), s2_blocks=2 if n > 5000 else 1), "E"))      # (> 5000: cut in stage 2 already)
            r += 8000
    r = 10000 + int(w.off[1])
    for L in (400, 401):
        half = (L + 1) // 2
        for m in (half - 1, half, half + 1):
            b = Builder(w, 5100 + k); k += 1
            # the gap: L bases of which exactly m agree -- the seed's substituted end base, L - 2 bases that agree at the even and disagree at the odd
            # offsets until the count is reached (agreeing runs stay below a seed's length), and a substituted last base in front of the next seed
            dis = L - m
            pos = list(range(1, 2 * (dis - 2), 2)) + [L - 2]
            assert len(pos) == dis - 1 and pos[-2] < L - 2 and L - 2 - pos[-2] < 15
            b.copy_every(r, 1000, 100).copy(r + 1000, L - 1, pos, endsub=False).copy_every(r + 1000 + L - 1, 1000, 100)
            q, src = b.build()
            cases.append(Case(f"E_agree_len{L}_{m}", {}, q, dict(src=src, n_groups=1, gap=(L, L), agree=m, s2_blocks=1), "E"))
            r += 4000
    r = 40000 + int(w.off[1])
    b = Builder(w, 5200).copy_every(r, 500, 100).copy(r + 500, 100, endsub=False).free(1).copy_every(r + 599, 501, 100)
    q, src = b.build()
    cases.append(Case("E_ref_overlap_1", {}, q, dict(src=src, n_groups=1, ref_overlap=1), "E"))
    b = Builder(w, 5201).copy_every(r + 3000, 500, 100).copy(r + 3500, 20, endsub=False).free(1).copy_every(r + 3500, 500, 100)
    q, src = b.build()
    cases.append(Case("E_ref_overlap_seed", {}, q, dict(src=src, n_groups=1, ref_overlap=20), "E"))


def _family_f(w, cases):
    """Tile edges of the fused passes: one contig of more than 6200 seeds in 210 groups of 29 / 30 / 31 seeds (an insertion of 30 between groups)."""
    b = Builder(w, 6000); r = 12000; n = 0
    for g in range(210):
        k = 29 + g % 3
        b.copy_every(r, 50 * k, 50).free(30); r += 50 * k; n += k
    q, src = b.build()
    cases.append(Case("F_tile_edges", {}, q, dict(src=src, n_groups=210, min_seeds=6200), "F"))


def bundle_contigs(w):
    """Family G: three short contigs for one bundle.  The first has its seeds at the highest PosDiff the text allows (query start against the end of the
    reverse-strand half), the second at the lowest (query end against the start of the text): a merge across the per-contig key stride would join them."""
    c0 = Builder(w, 7000).copy_every(0, 1200, 100)
    q0, s0 = c0.build(rev=True)        # revcomp(ref0[0:1200]): text positions 2G-1200 .. 2G-1, query positions from 0
    # (the first base of the reverse query is the substituted one: the seeds start at query position 1, text position 2G - 1199)
    q1, s1 = Builder(w, 7001).free(6000).copy_every(0, 1200, 100, endsub=False).build()
    q2, s2 = Builder(w, 7002).copy_every(int(w.off[2]) + 100, 3000, 100).build()
    return [("G_high", q0, s0), ("G_low", q1, s1), ("G_mid", q2, s2)]


_cache = {}


def world():
    if "w" not in _cache:
        _cache["w"] = World(make_refs())
    return _cache["w"]


def build_cases():
    """(refs, cases); deterministic, built once per process."""
    if "cases" not in _cache:
        w = world(); cases = []
        for fam in (_family_a, _family_b, _family_c, _family_d, _family_e, _family_f):
            fam(w, cases)
        assert len({c.name for c in cases}) == len(cases)
        _cache["cases"] = cases
    return world().refs, _cache["cases"]


# ---------------------------------------------------------------------------------------------------------------------------------
# the gap-similarity leaf (CalGapSimilarity, KmerAnalysis.cpp:78-121)
# ---------------------------------------------------------------------------------------------------------------------------------
def count_agree(q, text, q1, q2, r1):
    a = _CODE[q[q1:q2]]; b = _CODE[text[r1:r1 + (q2 - q1)]]
    return int(((a == b) | (a == 4) | (b == 4)).sum())


def kmer_common(a, b):
    """multiset intersection of the 5-mers of two windows WITHOUT N / n / IUPAC letters (plain definition)."""
    from collections import Counter
    ca = Counter(bytes(a[i:i + 5]) for i in range(len(a) - 4)); cb = Counter(bytes(b[i:i + 5]) for i in range(len(b) - 4))
    return sum(min(v, cb[k]) for k, v in ca.items())


def leaf_query():
    """(query, rows, notes): rows = (case id, q1, q2, r1, r2) per window, notes[case id] says what the window is built to hit."""
    if "leaf" in _cache:
        return _cache["leaf"]
    w = world(); G2 = 2 * w.G
    b = Builder(w, 8000)
    rows, notes = [], []

    def add(note, q1, q2, r1, r2):
        rows.append((len(notes), q1, q2, r1, r2)); notes.append(note)

    # (1) an ordinary copy with 5 % substitutions: short windows, long windows
    base_r = 60000
    b.copy_every(base_r, 12000, 20)
    for L in range(0, 13):
        add(f"len{L}_diag", 1000, 1000 + L, base_r + 1000, base_r + 1000 + L)
        add(f"len{L}_off", 1000, 1000 + L, 200000, 200000 + L + 3)
        add(f"qlen7_rlen{L}", 2000, 2007, 210000, 210000 + L)
    for ql, rl in ((4999, 5000), (5000, 4999), (5000, 5001), (5001, 5000), (5001, 4990), (4990, 5001), (5000, 5000), (5001, 5001), (4999, 4999)):
        add(f"unrelated_{ql}x{rl}", 500, 500 + ql, 220000, 220000 + rl)
        add(f"related_off_{ql}x{rl}", 500, 500 + ql, base_r + 497, base_r + 497 + rl)
    # (2) same-diagonal windows with a chosen number of agreeing positions; 5002 / 5003 bases (no 5-mer rescue above 5000) and 400 / 401
    spots = []
    for L in (5002, 5003, 400, 401):
        half = (L + 1) // 2
        for m in (half - 1, half, half + 1):
            r = 100000 + 6000 * len(spots)
            q1 = len(b)
            dis = list(range(0, L, 2))[:L - m]; dis += list(range(1, L, 2))[:L - m - len(dis)]      # disagree at the even offsets first
            b.copy(r, L, dis, endsub=False)
            spots.append((f"agree_len{L}_{m}", q1, q1 + L, r, m))
    # (3) 5-mer intersection of floor((q_len + r_len) * 0.1) and one more: shared tandem units (ref2) against unit copies + poly-A in the query
    k0 = int(w.off[2]) + KUNIT_AT
    rwin = (k0, k0 + 100)
    found = {}
    rtxt = w.fwd[rwin[0]:rwin[1]]
    for t in (40, 41, 42):
        for f in range(180, 260):
            qtxt = np.frombuffer(KUNIT * 40, np.uint8)[:t].tolist() + [65] * f
            c = kmer_common(np.array(qtxt, np.uint8), rtxt); lim = int((t + f + 100) * 0.1)
            for name, want in (("kmer_at_limit", lim), ("kmer_limit_plus_1", lim + 1)):
                if c == want and name not in found and t + f != 100:
                    found[name] = (t, f, c)
        if len(found) == 2:
            break
    assert len(found) == 2, found
    kspots = []
    for name, (t, f, c) in sorted(found.items()):
        q1 = len(b) + 1
        b.lit(b"C" + (KUNIT * 40)[:t] + b"A" * f + b"C")
        kspots.append((name, q1, q1 + t + f, c))
    # (4) letters: N, n, IUPAC, N in the first / last five, fewer than five bases between two Ns -- a copy with the letters written in
    lr = 300000
    q_let = len(b)
    b.copy_every(lr, 3000, 25)
    # (5) the last bases of the query: a copy that ends the query
    q_tail = len(b)
    b.copy_every(330000, 700, 20)
    q, src = b.build()
    for pos, ch in ((100, "N"), (300, "n"), (500, "R"), (700, "N"), (996, "N"), (1200, "N"), (1203, "N"), (1400, "N"), (1405, "N"), (1600, "N"), (1601, "N")):
        q[q_let + pos] = ord(ch)
    for nm, a, e in (("N_mid", 50, 250), ("n_mid", 250, 450), ("iupac", 450, 650), ("N_first5", 698, 900), ("N_last5", 900, 1000), ("N_gap3", 1150, 1350), ("N_gap5", 1350, 1550),
                     ("N_pair", 1550, 1750), ("N_only_short", 1198, 1206), ("N_at_0", 700, 720), ("N_window_6", 1199, 1205)):
        add(nm + "_diag", q_let + a, q_let + e, lr + a, lr + e)
        add(nm + "_off", q_let + a, q_let + e, lr + a + 1, lr + e + 3)
        add(nm + "_unrelated", q_let + a, q_let + e, 5000 + a, 5000 + e + 7)
    for name, q1, q2, r, m in spots:
        assert count_agree(q, w.text, q1, q2, r) == m
        add(name, q1, q2, r, r + (q2 - q1))
    for name, q1, q2, c in kspots:
        assert kmer_common(q[q1:q2], rtxt) == c
        add(name, q1, q2, rwin[0], rwin[1])
    n = q.size
    add("query_end_diag", n - 300, n, 330000 + 400, 330000 + 700)
    add("query_end_off", n - 333, n, 5000, 5400)
    add("query_end_len3", n - 3, n, 5000, 5009)
    add("text_end_diag", q_tail, q_tail + 300, G2 - 300, G2)
    add("text_end_off", 100, 433, G2 - 401, G2)
    add("text_end_len4", 100, 104, G2 - 4, G2)
    add("both_ends", n - 9, n, G2 - 9, G2)
    _cache["leaf"] = (q, np.asarray(rows, np.int64), notes)
    return _cache["leaf"]
