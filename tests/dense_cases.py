"""Constructed chunks for the dense seed search (csrc/k_seed_dense.hip: k_dense_search, k_dense_sweep, k_dense_resolve) -- a helper module, not a conftest.

    ref, cases = build_cases(slen)            # the default MinSeedLength
    ref, cases = build_cases(SEN_SLEN, sen=True)
    ref, cases = build_cases(slen, sen, kmer_k=K)    # a row of the (kmer_k, MinSeedLength) grid, GRID below

`ref` is a 200 kb random reference with copies of its own stretches planted in its far end (150 000 ...); it does NOT depend on slen / sen, so one index serves
both.  `cases` is an ordered dict  name -> (query, must_be_seed_starts, must_not_be_seed_starts, [(start, expected_len, expected_freq)]):  the longest match
from `start` inside its chunk (what BWT_Search computes) has expected_len bases and occurs expected_freq times in the forward text + its reverse complement.
A query is colinear with a stretch of the reference and differs from it by substitutions at CHOSEN positions only: every 100 bases (70, 170, ...) where nothing is
constructed, and the case's own ones inside a stretch that is cleared of the regular ones.  Where a match has to end at an exact base, the substituted base is the
one of the three for which the match does not go on anywhere else in the text (`stop`); where a short match has to be unique, its place is the first one at which
it is (`_unique_start`): both are searches in the text, no index involved.

How a start gets onto the reference's chain (only those starts reach the seeds that the GPU is compared on): by default a match of the chain ends at the
substitution in front of it and the hop is its length + 1; under -sen the hop behind a seed is 5 whatever its length, so there a run of five N stands in front of
the start: a walk cannot jump it and leaves it base by base.

Families: seg_edge_*  back_*  freq_*  text_*  len_* / n_at_* / start_at_*  resolve_*  handover_last_chunk  cand_cap_sen.

The grid: which rungs of the search ladder exist depends on how MinSeedLength compares with the jump table's kmer_k, so build_cases takes the
kmer_k that the context will be forced to (None: the text's own, 12) and GRID lists the rows.  What follows the row: text_* (kmer_k + n bases), len_k-1 / len_k,
len_klo (whenever an N can stand behind MinSeedLength bases and inside the first kmer_k), the run of seg_edge_* (25 bases, MinSeedLength where that is more: the
planted second copy has 26, so above 25 the listed matches are unique), and the families
    len_between_*        exact lengths MinSeedLength + 1 and kmer_k - 1 where they lie strictly between the two: the kmer_k-entry is absent, the seed is accepted
    len_pres_16 / _17    (MinSeedLength >= 18) the presence table answers for 16 bases: the bit is set, no seed results
    pres_look_{1..4}     j starts in a row whose first pres_k = min(MinSeedLength, 16) bases occur nowhere (one substitution at the last of them, chosen so), then
                         a seed of 40 bases: the look-ahead of the speculative kernel (three starts per presence line) and its fall-through on the fourth;
                         pres_look_2_p16 (MinSeedLength > 16): the start behind the absent run matches exactly 16 bases -- present, and no seed
    start_at_clen-k/-k+1 (kmer_k > MinSeedLength) a seed of kmer_k / kmer_k - 1 bases into the chunk's last base: s + kmer_k = clen and clen + 1
    n_word_32_{29..32}   (MinSeedLength 30) an N at that offset from a start on the chain: the mask of the first min(MinSeedLength, 32) bases at the 32-bit edge
MER (30) is the longest MinSeedLength there is and the resolver's hops are matches of 38 - 40 bases, so freq_* and resolve_hop_* hold on every row as they are.
A construction that has no place on a row (a 7-mer that occurs once in 400 kb) is named in DROPPED; nothing is left out silently.
"""
from __future__ import annotations

import numpy as np

from gsalign_amd import synth

CHUNK = 10000                   # GSA_CHUNK
REF_LEN = 200_000
DEFAULT_SLEN = 15
SEN_SLEN = 10                   # MinSeedLength under -sen whatever -slen says (gsa_set_params; main.cpp:323 of the reference)
MAX_FREQ = 100                  # GSA_MAX_SEED_FREQ
RS_B = 40                       # k_dense_resolve: positions per thread
SEGS = (40, 160)                # k_dense_sweep: starts per segment of its two launch shapes
MER = 30                        # the planted repeat of the freq_* family
FREQ_S = 5000                   # its start in the query

_ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.zeros(256, np.uint8); _CODE[_ACGT] = np.arange(4, dtype=np.uint8)

# where the queries come from (reference offsets); the plants lie at PLANT_AT ...
A_SEG = {40: 10_000, 160: 20_000}
A_FREQ = {"freq_100": 30_000, "freq_101": 40_000, "freq_cross_down": 50_000, "freq_cross_up": 60_000}
A_HAND = 70_000                 # chunks 0 and 1 of handover_last_chunk
A_FREE = 100_000                # every case without a plant
PLANT_AT = 150_000
TANDEM_AT, TANDEM_UNIT, TANDEM_N = 170_000, 40, 200      # 8 kb: a unit 200 times
SEG_E = {40: 2040, 160: 2080}   # the segment edge of seg_edge_*: 2040 is one of the 40-start segments only


def kmer_k_for(text_len: int) -> int:
    """Length of the k-mer jump table the library builds for a text (forward + reverse) of text_len bases: ceil(log4) + 2, at most 15 (build_kmer_table)."""
    k = 0
    while (1 << (2 * k)) < text_len:
        k += 1
    return min(k + 2, 15)


def rot(b, r=1):
    """the base(s) b rotated by r within ACGT: never b itself for r = 1, 2, 3"""
    return _ACGT[(_CODE[b] + r) & 3]


def text_of(ref) -> bytes:
    """what the index holds: the forward bases, then their reverse complement"""
    return ref.tobytes() + synth.revcomp(ref).tobytes()


def count_in(text: bytes, pat: bytes, cap: int = MAX_FREQ + 2) -> int:
    """occurrences of pat in text, overlapping ones too, counted up to cap"""
    n, i = 0, text.find(pat)
    while i >= 0 and n < cap:
        n += 1; i = text.find(pat, i + 1)
    return n


def make_ref():
    """The reference with its plants; the same for every slen."""
    ref = synth.random_genome(REF_LEN, np.random.default_rng(20262))
    at = PLANT_AT
    # seg_edge_*_dup: the 25 bases right of the edge once more, between the reference's own next base (the query has a substitution there) and a base that
    # differs from the one in front of the edge
    for seg in SEGS:
        a, E = A_SEG[seg], SEG_E[seg]
        ref[at] = rot(ref[a + E - 1]); ref[at + 1:at + 27] = ref[a + E:a + E + 26]
        at += 100
    # freq_*: copies of ref[a + s - 1 : a + s + 31) = the base in front of the 30-mer, the 30-mer, the base behind it.  The query has a substitution behind the
    # 30-mer, so its match ends there at every copy.  With the colinear occurrence: 100 / 101 / 101 / 101 occurrences of the 30-mer; of the 31-mer that starts one
    # base earlier: cross_down 100 (one copy has another base in front), cross_up 100 (all 100 copies have the QUERY's substituted base in front, the colinear one not)
    for name, copies in (("freq_100", MAX_FREQ - 1), ("freq_101", MAX_FREQ), ("freq_cross_down", MAX_FREQ), ("freq_cross_up", MAX_FREQ)):
        a = A_FREQ[name]
        unit = ref[a + FREQ_S - 1:a + FREQ_S + MER + 1].copy()
        for k in range(copies):
            ref[at:at + unit.size] = unit
            if name == "freq_cross_up" or (name == "freq_cross_down" and k == 0):
                ref[at] = rot(unit[0], 1 if name == "freq_cross_up" else 2)
            at += unit.size
        at += 100
    assert at < TANDEM_AT - 2000
    # handover_last_chunk: a tandem array
    ref[TANDEM_AT:TANDEM_AT + TANDEM_UNIT * TANDEM_N] = np.tile(ref[TANDEM_AT:TANDEM_AT + TANDEM_UNIT].copy(), TANDEM_N)
    return ref


class _Q:
    """One query: colinear with ref[a : a + n), regular substitutions outside the cleared stretches."""

    def __init__(self, ref, a, n, sen, clear=()):
        self.ref, self.a, self.sen = ref, a, sen
        self.q = ref[a:a + n].copy()
        pos = np.arange(70, n, 100)
        for lo, hi in clear:
            pos = pos[(pos < lo) | (pos >= hi)]
        self.q[pos] = rot(self.q[pos])
        self.stops = []

    def sub(self, p, r=1):
        self.q[p] = rot(self.ref[self.a + p], r)

    def enter(self, e):
        """start e is on the chain and the base in front of it does not continue any match"""
        if self.sen:
            self.q[e - 5:e] = ord("N")
        else:
            self.sub(e - 1)

    def stop(self, s, p):
        """the match from s ends in front of p: a substitution there, chosen in finish()"""
        self.stops.append((s, p))

    def finish(self, text):
        for s, p in self.stops:
            for r in (1, 2, 3):
                self.sub(p, r)
                if self.q[s:p + 1].tobytes() not in text:
                    break
            else:
                raise AssertionError(f"dense_cases: every base at {p} continues a match from {s} somewhere")
        return np.ascontiguousarray(self.q)


class NoPlace(AssertionError):
    """a construction has no place in this text"""


def _unique_start(ref, text, a, s0, n, step=1):
    """the first start s >= s0 (s0, s0 + step, ...) at which ref[a + s : a + s + n) occurs once in the text"""
    for s in range(s0, s0 + 4000 * step, step):
        if count_in(text, ref[a + s:a + s + n].tobytes(), 2) == 1:
            return s
    raise NoPlace("dense_cases: no unique stretch")


def longest_in(text: bytes, qb: bytes, s: int, end: int):
    """(length, occurrences) of the longest match of qb[s : end) in the text, base by base"""
    L = 0
    while s + L < end and qb[s + L] in b"ACGT" and text.find(qb[s:s + L + 1]) >= 0:
        L += 1
    return L, (count_in(text, qb[s:s + L]) if L else 0)


# the rows: kmer_k -> (MinSeedLength, -sen) ...; -sen forces MinSeedLength 10
GRID = {
    12: ((10, False), (11, False), (12, False), (13, False), (14, False), (16, False), (17, False), (30, False), (SEN_SLEN, True)),
    15: ((10, False), (13, False), (14, False), (15, False), (16, False), (30, False), (SEN_SLEN, True)),
    8: ((10, False), (15, False), (30, False), (SEN_SLEN, True)),
}
# (kmer_k, MinSeedLength, sen) -> the constructions that have no place on that row: a match of exactly 7 bases that occurs once does not exist in 400 kb
# (a 7-mer is expected 24 times).  build_cases fails if a name listed here CAN be placed, and if one not listed cannot.
DROPPED = {(8, slen, sen): ("len_k-1",) for slen, sen in GRID[8]}
NEW_FAMILIES = ("len_between_", "len_pres_", "pres_look_", "start_at_clen-k", "n_word_32_")


def cases_digest(ref, cases) -> str:
    """sha256 over the reference and every case: name, query bytes, both start lists, the triples"""
    import hashlib
    h = hashlib.sha256(np.ascontiguousarray(ref).tobytes())
    for name, (q, on, off, trip) in cases.items():
        h.update(repr((name, [int(x) for x in on], [int(x) for x in off], [tuple(int(x) for x in t) for t in trip])).encode()); h.update(q.tobytes())
    return h.hexdigest()


_cache = {}


def build_cases(slen: int = DEFAULT_SLEN, sen: bool = False, kmer_k: int | None = None):
    """(ref, cases) for MinSeedLength slen; sen: the chain hops 5 behind a seed (pass SEN_SLEN with it); kmer_k: the jump table's k-mer length when the
    context is forced to one (None: the one the library picks for this text)."""
    key = (slen, sen, kmer_k)
    if key in _cache:
        return _cache[key]
    if "ref" not in _cache:
        _cache["ref"] = make_ref(); _cache["text"] = text_of(_cache["ref"])
    ref, text = _cache["ref"], _cache["text"]
    S, K = slen, kmer_k or kmer_k_for(2 * REF_LEN)
    PK = min(S, 16)                                # build_presence: pres_k
    drop = DROPPED.get((kmer_k, slen, sen), ()) if kmer_k else ()
    cases = {}

    def add(name, Q, on, off, trip):
        assert name not in cases
        cases[name] = (Q.finish(text), sorted(on), sorted(off), trip)

    def both(dflt, always=()):
        """starts that are on the chain by the default hop only"""
        return list(always) + ([] if sen else list(dflt))

    # ---- sweep segments: a match that starts 3 bases left of a segment's first start E and runs 25 bases into it ----
    R = max(25, S)                                 # (the plant holds 26 bases: a longer run meets the second copy on its way and ends unique)
    for seg in SEGS:
        E = SEG_E[seg]
        for dup in (False, True):
            a = A_SEG[seg] if dup else A_FREE
            f = 2 if dup and R == 25 else 1
            sfx = "_dup" if dup else ""
            Q = _Q(ref, a, CHUNK, sen, [(E - 60, E + 90)]); Q.enter(E - 3); Q.stop(E - 3, E + R)
            add(f"seg_edge_{seg}{sfx}", Q, [E - 3], both([E]), [(E - 3, R + 3, 1), (E - 1, R + 1, 1), (E, R, f), (E + 1, R - 1, f)])
            # the left neighbour does not extend: the left lane's search from scratch at its last start E - 1 meets a substituted base, E is on the chain
            Q = _Q(ref, a, CHUNK, sen, [(E - 60, E + 90)]); Q.enter(E); Q.stop(E, E + R)
            add(f"seg_edge_{seg}{sfx}_noext", Q, [E], [], [(E, R, f), (E + 1, R - 1, f)])

    # ---- M_BACK: the start of the text, the forward / reverse seam, a word edge of the query words ----
    Q = _Q(ref, 0, CHUNK, sen)
    add("back_text_start", Q, [0], [], [(0, 70, 1), (1, 69, 1)])
    for u in range(1000, 1400):                    # (the first seven from which no match reaches MinSeedLength, so that start 7 is on the chain: at 15 those of 1000)
        Q = _Q(ref, 0, CHUNK - 7, sen); Q.q = np.concatenate([rot(ref[u:u + 7]), Q.q])      # seven unrelated bases in front: the 32 starts of a backward step reach past text position 0
        if sen or all(longest_in(text, Q.q[:40].tobytes(), i, 40)[0] < S for i in range(7)):
            break
    else:
        raise NoPlace("back_text_start_off")
    add("back_text_start_off", Q, both([7]), [], [(7, 70, 1), (8, 69, 1)])
    G = REF_LEN
    tx =np.frombuffer(text, np.uint8)
    q = tx[2 * G - 300:2 * G].copy(); q[[100, 200]] = rot(q[[100, 200]])          # the reverse complement of ref[0 : 300): ends at the last base of the doubled text
    Q = _Q(ref, 0, 0, sen); Q.q = q
    add("back_seam", Q, both([101, 201], [0]), [], [(0, 100, 1), (201, 99, 1)])
    q = tx[G - 300:G + 100].copy(); q[[100, 250]] = rot(q[[100, 250]])            # the last 300 forward bases and the 100 behind the seam
    Q = _Q(ref, 0, 0, sen); Q.q = q
    add("back_seam_fwd", Q, both([101, 251], [0]), [], [(0, 100, 1), (101, 149, 1), (251, 149, 1)])
    for p in (31, 32, 33):
        Q = _Q(ref, A_FREE, CHUNK, sen, [(0, 70)]); Q.sub(70); Q.enter(p)
        add(f"back_word_edge_{p}", Q, [p], [], [(p, 70 - p, 1)])

    # ---- M_BFM: MaxSeedFreq crossed in one step ----
    s = FREQ_S
    for name, e, on, off, trip in (("freq_100", s, [s], [], [(s, MER, 100)]), ("freq_101", s, [], [s], [(s, MER, 101)]),
                                   ("freq_cross_down", s - 1, [s - 1], [], [(s - 1, MER + 1, 100), (s, MER, 101)]),
                                   ("freq_cross_up", s, [], [s], [(s, MER, 101)] + ([] if sen else [(s - 1, MER + 1, 100)]))):
        Q = _Q(ref, A_FREQ[name], CHUNK, sen, [(s - 60, s + 100)]); Q.enter(e); Q.stop(e, s + MER)
        add(name, Q, on, off, trip)

    # ---- M_TEXT: 64-base windows behind the k-mer jump; the start is the last one of a segment, so the sweep searches it from scratch as well ----
    s = 159 + 160 * 12
    for n in (63, 64, 65, 127, 128, 129):
        Q = _Q(ref, A_FREE, CHUNK, sen, [(s - 60, s + K + n + 60)]); Q.enter(s); Q.stop(s, s + K + n)
        add(f"text_{n}", Q, [s], [], [(s, K + n, 1)])
    s = 159 + 160 * 61
    Q = _Q(ref, A_FREE, 2 * CHUNK, sen, [(s - 60, CHUNK + 60)]); Q.enter(s)        # the text goes on matching behind the chunk's last base
    add("text_chunk_end", Q, [s], [], [(s, CHUNK - s, 1)])

    add("cand_cap_sen", _Q(ref, A_FREE + 20_000, CHUNK, sen, [(0, CHUNK)]), [0], [], [(0, CHUNK, 1), (5, CHUNK - 5, 1)])

    # ---- the search ladder's switches ----
    def short(name, n, nbase=None, klo=False):
        """a match of exactly n bases, unique, at a start that is on the chain; nbase: an N ends it instead of a substitution"""
        try:
            s0 = 2999
            while True:                            # (the first unique place; the next one where no base ends the match there -- short k-mers: all three go on somewhere)
                s0 = _unique_start(ref, text, A_FREE, s0 + 1, n)
                if nbase is not None or any((ref[A_FREE + s0:A_FREE + s0 + n].tobytes() + bytes(rot(ref[A_FREE + s0 + n:A_FREE + s0 + n + 1], r))) not in text for r in (1, 2, 3)):
                    break
        except NoPlace:
            assert name in drop, (name, "has no place on row", (kmer_k, slen, sen), "and is not in DROPPED")
            return
        assert name not in drop, (name, "is in DROPPED and can be placed on row", (kmer_k, slen, sen))
        Q = _Q(ref, A_FREE, CHUNK, sen, [(s0 - 60, s0 + 90)]); Q.enter(s0)
        if nbase is None:
            Q.stop(s0, s0 + n)
        else:
            Q.q[s0 + n] = ord("N")
        add(name, Q, [s0] if n >= S else [], [] if n >= S else [s0], [(s0, n, 1)])

    short("len_min-1", S - 1); short("len_min", S)
    short("len_k-1", K - 1); short("len_k", K)
    if (sen or kmer_k) and S + 1 < K:
        short("len_klo", S + 1, nbase=True)        # an N inside the first kmer_k bases: the long table is out of reach, the short one (kmer_lo_k = MinSeedLength) is not
    if kmer_k:
        for name, n in (("len_between_min+1", S + 1), ("len_between_k-1", K - 1)):
            if S < n < K:                          # the presence bit is set, the kmer_k-entry says "absent", the walk from the first base finds a seed
                short(name, n)
        if S >= 18:
            short("len_pres_16", 16); short("len_pres_17", 17)      # present by their 16 bases and no seeds
        if S == 30:
            for o in (29, 30, 31, 32):
                short(f"n_word_32_{o}", o, nbase=True)
    short("n_at_L-1", S - 1, nbase=True); short("n_at_L", S, nbase=True)
    ends = [("start_at_clen-min", S), ("start_at_clen-min+1", S - 1)]
    if kmer_k and K > S:
        ends += [("start_at_clen-k", K), ("start_at_clen-k+1", K - 1)]      # s + kmer_k = clen: the last start with a table entry; clen + 1: the first without
    for name, n in ends:
        s = CHUNK - n
        a = A_FREE + _unique_start(ref, text, A_FREE + s, 0, n)
        Q = _Q(ref, a, 2 * CHUNK, sen, [(s - 60, CHUNK + 60)]); Q.enter(s)
        add(name, Q, [s] if n >= S else [], [] if n >= S else [s], [(s, n, 1)])

    # ---- the presence table ahead of a walk: j starts whose first pres_k bases occur nowhere, then one that is a seed (p16: present by 16 bases, 16 < MinSeedLength) ----
    def pres_look(name, j, p16=False):
        for e in range(4000, 8000, 7):
            for r in (1, 2, 3):
                Q = _Q(ref, A_FREE, CHUNK, sen, [(e - 60, e + j + 120)]); Q.enter(e); Q.sub(e + j - 1, r)
                if all(Q.q[e + i:e + i + PK].tobytes() not in text for i in range(j)):
                    break
            else:
                continue
            n = 16 if p16 else 40
            Q.stop(e + j, e + j + n)
            qb = Q.finish(text).tobytes()
            if count_in(text, qb[e + j:e + j + n], 2) != 1:
                continue
            trip = [(e + i,) + longest_in(text, qb, e + i, CHUNK) for i in range(j)] + [(e + j, n, 1)]
            assert all(t[1] < PK for t in trip[:j])
            add(name, Q, [] if p16 else [e + j], list(range(e, e + j)) + ([e + j] if p16 else []), trip)
            return
        raise NoPlace(name)

    if kmer_k:
        for j in (1, 2, 3, 4):
            pres_look(f"pres_look_{j}", j)
        if S > 16:
            pres_look("pres_look_2_p16", 2, p16=True)

    # ---- k_dense_resolve: blocks of RS_B positions ----
    p = RS_B * 50
    for h in (39, 40, 41):                         # the hop from a block's first position
        Q = _Q(ref, A_FREE, CHUNK, sen, [(p - 60, p + h + 30)]); Q.enter(p); Q.stop(p, p + h - 1)
        add(f"resolve_hop_{h}", Q, both([p + h], [p]), [], [(p, h - 1, 1)])
    s = RS_B * 50 + 1
    Q = _Q(ref, A_FREE, CHUNK, sen, [(s - 60, s + 260)]); Q.enter(s); Q.stop(s, s + 200)
    add("resolve_skip_blocks", Q, both([s + 201], [s]), [], [(s, 200, 1)])
    for n, last in ((9999, 9997), (10001, 9999)):  # the last hop lands on clen - 1 (the last block has 39 positions) / on clen
        Q = _Q(ref, A_FREE, n, sen, [(9790, n)]); Q.enter(9850); Q.stop(9850, last)
        add(f"resolve_tail_{n}", Q, [9850], [], [(9850, last - 9850, 1)])
    s1, s2 = RS_B * 50 + 38, RS_B * 80 + 35        # -sen: 2038 -> 2043 across a block edge, 3235 -> 3240 onto one
    Q = _Q(ref, A_FREE, CHUNK, sen, [(s1 - 60, s1 + 60), (s2 - 60, s2 + 60)]); Q.enter(s1); Q.enter(s2); Q.sub(s1 + 60); Q.sub(s2 + 60)
    add("resolve_sen_edge", Q, [s1, s2] + ([s1 + 5, s2 + 5] if sen else []), [], [(s1, 60, 1), (s2, 60, 1)])

    # ---- slot != chunk: only the third chunk is heavy (a tandem array with more than MaxSeedFreq copies, a substitution every 100 bases) ----
    if not sen:
        Q = _Q(ref, A_HAND, 3 * CHUNK, sen)
        q3 = _Q(ref, TANDEM_AT - 1000, CHUNK, sen)
        Q.q[2 * CHUNK:] = q3.q
        s = 2 * CHUNK + 1000 + 71                  # behind a substitution inside the array: 99 bases that occur in ~197 units
        add("handover_last_chunk", Q, [71, CHUNK + 71], [s], [(s, 99, MAX_FREQ + 2)])

    _cache[key] = (ref, cases)
    return _cache[key]
