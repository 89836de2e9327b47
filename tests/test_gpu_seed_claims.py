"""The seed kernel's walks across sub-range ends (csrc/k_seed.hip, seed_chunk): a walk ends where the start it arrives at is memoised, claimed by
a search in flight or behind the chunk's end, and the resolver behind the pass follows the memo in LDS.  The shapes at which that can go wrong, built
from a 200 kb random reference with short copies of the QUERY's bases planted in it (far from the region the queries are colinear with):

(a) hop_over    a left-edge search finds a planted 20-mer across a mismatch 3 bases behind the edge and hops over the true entry (the base behind
                the mismatch): whoever completes the match in front of the mismatch has to search from the true entry.
(b) two_exits   the left-edge match (a planted copy of S + 5 bases) spans its whole sub-range and ends at E1; from the true entry the colinear match runs on to
                E2 > E1, in another sub-range: the resolver has to replace the exit, and the sub-range that E1 lies in is not on the chain.
(c) six_in_a_row  six consecutive sub-ranges, each entered 3 bases behind its left edge by a match that ends there, each left edge with a planted
                20-mer that hops over that entry: every true entry is known only when the predecessor's match is complete.
(d) same_start  two sub-ranges without a mismatch, and one behind them: the first matches of both left edges end at that one mismatch, both walks
                arrive at the start behind it.  (Which of them gets there first is the kernel's timing; the claim bit or the memo stops the other.)
(e) edges       chunks of 9 999 and 10 001 bases and a three-chunk contig, the last stretch of every chunk without a mismatch: the chain's last hop
                passes the chunk's end.
(f) n_at_claim  a run of N across a sub-range edge five bases behind a start of the true chain.

Every case: accepted seeds (qPos, len, rPos of every located hit) and seed groups of stage 1 and the finished blocks of gsa_align_contig against
the oracle -- exact, in both index layouts -- and no chunk handed to the dense kernels, so that it is the speculative kernel that is under test.
(a)-(d): one memory-bound pass (seed_stats()[0] == 1): the claims covered the chain, not the fallback pass.  What each construction is meant to
do is checked on the oracle's side (next start per start from its BWT search) when the module's fixture builds it."""
import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu

CHUNK = 10000          # GSA_CHUNK
NSUB = 64              # sub-ranges per chunk
S = -(-CHUNK // NSUB)  # their length in a full chunk
MIN_SEED = 15          # -slen
REF_LEN = 200_000
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _subst(q, pos):
    """A guaranteed mismatch at every position of `pos`: the base rotated within ACGT."""
    code = np.zeros(256, np.uint8); code[ACGT] = np.arange(4, dtype=np.uint8)
    q[pos] = ACGT[(code[q[pos]] + 1) & 3]


def _query(ref, a, n, keep_clear=()):
    """n bases colinear with ref[a:], a substitution every 100 bases (at 70, 170, ...) except inside the [lo, hi) stretches of keep_clear."""
    q = ref[a:a + n].copy()
    pos = np.arange(70, n, 100)
    for lo, hi in keep_clear:
        pos = pos[(pos < lo) | (pos >= hi)]
    _subst(q, pos)
    return q


class _Planter:
    """Copies of query bases into the reference's far end, each followed by a base that ends the match there."""
    def __init__(self, ref):
        self.ref, self.at = ref, 150_000

    def plant(self, q, lo, hi):
        n = hi - lo
        self.ref[self.at:self.at + n] = q[lo:hi]
        if hi < q.size:                                   # the base behind the copy differs from the query's next one
            self.ref[self.at + n] = q[hi]; _subst(self.ref, np.array([self.at + n]))
        self.at += n + 200


def _build(ref):
    """The queries (and, as a side effect, the planted copies in ref) + what each case is checked for on the oracle's side:
    name -> (query, starts that must be seeds, starts that must not be, [(start, lowest next start)] of searches, one pass expected).
    Every construction clears the regular substitutions around it and sets its own, so it holds for any sub-range length S."""
    pl = _Planter(ref)
    cases = {}

    def at(q, *pos):
        _subst(q, np.array(pos))

    # (a) sub-range 11, left edge L: the chain starts at L - 29, meets a mismatch at L + 3 and goes on from L + 4 (to a mismatch at L + 45); a copy of q[L : L + 20) elsewhere
    L = 11 * S
    q = _query(ref, 10_000, CHUNK, keep_clear=[(L - 40, L + 60)]); at(q, L - 30, L + 3, L + 45); pl.plant(q, L, L + 20)
    cases["hop_over"] = (q, [L - 29, L + 4], [L], [(L, L + 21)], True)
    # (b) sub-range 20: mismatch at L + 3, true entry L + 4; q[L : L + S + 5) elsewhere -> E1 = L + S + 6, in sub-range 21; no mismatch in front of X in sub-range 22,
    #     so the match from L + 4 ends there -> E2 = X + 1
    L = 20 * S; X = 22 * S + 20; E1 = L + S + 6
    q = _query(ref, 25_000, CHUNK, keep_clear=[(L - 40, 22 * S + 60)]); at(q, L - 30, L + 3, X); pl.plant(q, L, L + S + 5)
    cases["two_exits"] = (q, [L + 4, X + 1], [L, E1], [(L, E1), (L + 4, X + 1)], True)
    # (c) sub-ranges 30 .. 35: the only mismatches are at left edge + 2 (and one in front, one behind); q[edge : edge + 20) elsewhere for each of the six
    edges = [v * S for v in range(30, 36)]
    q = _query(ref, 40_000, CHUNK, keep_clear=[(edges[0] - 40, edges[5] + S + 60)]); at(q, edges[0] - 30, *[e + 2 for e in edges], edges[5] + S + 2)
    for e in edges:
        pl.plant(q, e, e + 20)
    cases["six_in_a_row"] = (q, [e + 3 for e in edges], edges, [(e, e + 21) for e in edges], True)
    # (d) sub-ranges 50 and 51: no mismatch from L50 - 29 to X = L51 + 40: both left edges' first matches end at X, both walks arrive at X + 1
    L50, L51 = 50 * S, 51 * S; X = L51 + 40
    q = _query(ref, 55_000, CHUNK, keep_clear=[(L50 - 40, L51 + S + 60)]); at(q, L50 - 30, X)
    cases["same_start"] = (q, [L50 - 29, X + 1], [L50, L51], [(L50, X + 1), (L51, X + 1)], True)
    # (e) the last stretch of every chunk clear: the last match of a chunk runs into the chunk's end
    for n in (9999, 10001, 29999):
        clear = [(c * CHUNK + 9871, (c + 1) * CHUNK) for c in range(3)]
        cases[f"edges_{n}"] = (_query(ref, 70_000, n, keep_clear=clear), [9871], [], [(9871, min(n, CHUNK) + 1)], False)
    # (f) start E - 10 of the true chain (mismatch at E - 11), N over [E - 5, E + 6): across the edge E of sub-range 41
    E = 41 * S
    q = _query(ref, 105_000, CHUNK, keep_clear=[(E - 60, E + 60)]); at(q, E - 50, E - 11, E + 40); q[E - 5:E + 6] = ord("N")
    cases["n_at_claim"] = (q, [E - 49, E + 6], [E - 10], [(E - 10, E - 9)], False)
    return cases


def _next_start(o, q, s):
    """next(s) of the reference's walk inside s's chunk, from the oracle's BWT search (the query is set)."""
    end = min(q.size, (s // CHUNK + 1) * CHUNK)
    ln, locs = o.bwt_search(s, end)
    return s + ln + 1 if ln >= MIN_SEED and locs.size > 0 else s + 1


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_claims")
    ref = synth.random_genome(REF_LEN, np.random.default_rng(20261))
    cases = _build(ref)
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx)
    want = {}
    for name, (q, on, off, nexts, one_pass) in cases.items():
        o.set_query(q)
        for s, lowest in nexts:                            # the constructions do what they are meant to
            assert _next_start(o, q, s) >= lowest, (name, s, _next_start(o, q, s), lowest)
        o.run_to(1)
        s1 = o.seeds() + o.groups()
        starts = set(np.unique(s1[0]).tolist())
        assert all(s in starts for s in on) and not any(s in starts for s in off), (name, sorted(starts & set(on + off)))
        for c in range((q.size + CHUNK - 1) // CHUNK):     # seeds in every chunk that is long enough to hold one
            if min(q.size, (c + 1) * CHUNK) - c * CHUNK >= MIN_SEED:
                assert any(c * CHUNK <= s < (c + 1) * CHUNK for s in starts), (name, c)
        o.run_to(8)
        want[name] = (q, s1, o.blocks(with_aln=True), one_pass)
    o.close()
    return idx, want


@pytest.fixture(scope="module", params=["narrow", "wide"])
def gpu(request, world):
    a = capi.Aligner(world[0], wide=(request.param == "wide"))
    yield a
    a.close()


@pytest.mark.parametrize("name", ["hop_over", "two_exits", "six_in_a_row", "same_start", "edges_9999", "edges_10001", "edges_29999", "n_at_claim"])
def test_claimed_walks(gpu, world, name):
    q, s1, blocks, one_pass = world[1][name]
    gpu.set_query(q); gpu.run_to(1)
    got = gpu.seeds() + gpu.groups()
    st = gpu.seed_stats()
    print(f"{name}: passes {int(st[0])}, chunks handed over {int(st[1])}, wave iterations max {int(st[2])}")
    assert int(st[1]) == 0, (name, int(st[1]))
    for k, (a, b) in enumerate(zip(got, s1)):
        assert a.shape == b.shape and np.array_equal(a, b), (name, ("qpos", "len", "rpos", "gbeg", "gend")[k])
    if one_pass:
        assert int(st[0]) == 1, (name, int(st[0]))
    gpu.align_contig(q); full = gpu.blocks_as_dump(with_aln=True)
    for k, v in blocks.items():
        assert np.array_equal(full[k], v), (name, k)
