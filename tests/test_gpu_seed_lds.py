"""The seed kernel's per-chunk LDS state at its edges (csrc/k_seed.hip, SeedLds): independent one-chunk waves share a workgroup, the
N bitmap lies behind the long-hop table, and the on-path bits reuse the query's words once the walks are over.  The table is
held to 512 entries here (gsa_set_option "seed_lhop"): the size of the SEED_LDS_DIET build, which these shapes were written for
(there a chunk with ambiguous bases has 256, and one without keeps no N bitmap), and one that a chunk can actually fill.

Every case: accepted seeds (qPos, len, rPos of every located hit, so the frequency as well) and seed groups of stage 1, and the
finished blocks of gsa_align_contig, against the oracle -- exact, in both index layouts.  Inputs are synthetic with fixed seeds;
the oracle's side is computed once per module."""
import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu

CHUNK = 10000          # GSA_CHUNK
NSUB = 96              # sub-ranges per chunk: their length is ceil(10000 / 96) = 105
LHOP_N = 512           # long-hop entries the tests let a chunk use
REF_LEN = 200_000


def _subst(q, pos):
    """A guaranteed mismatch at every position of `pos`: the base rotated within ACGT."""
    code = np.zeros(256, np.uint8); code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    q[pos] = np.frombuffer(b"ACGT", np.uint8)[(code[q[pos]] + 1) & 3]


def _diverged(ref, a, n, rng):
    """n bases: ref[a:] with the usual 1 % event mix (substitutions and short indels)."""
    return np.ascontiguousarray(synth.mutate(ref[a:a + n + 1000], 0.01, rng)[:n])


def _long_hop_query(ref):
    """30 kb, colinear with ref[50000:80000].  Chunks 0 and 2: a substitution every 100 bases.  Chunk 1 is the caller's: a substitution every p
    bases makes every stretch between two of them an accepted match of p - 1 >= MinSeedLength bases, i.e. one long hop of p."""
    q = ref[50000:80000].copy()
    _subst(q, np.arange(50, 10000, 100)); _subst(q, np.arange(20050, 30000, 100))
    return q


def _cases(ref):
    rng = np.random.default_rng(20260)
    cases = {}
    # chunk-edge shapes: the last sub-range is short; one- and three-chunk contigs leave most of a workgroup's twelve waves without a chunk
    for n in (9999, 10000, 10001, 20000, 29999):
        cases[f"edge_{n}"] = _diverged(ref, 1000 + n, n, rng)
    # long hops: half of chunk 1 in exact runs, the other half with a mismatch every 18 bases (5000 / 18 = 277 hops + the two runs: more than
    # half of the 512 entries on the true chain alone; the speculative walks add up to one per sub-range)
    q = _long_hop_query(ref)
    _subst(q, np.array([10000 + 2000, 10000 + 7500 - 1])); _subst(q, 10000 + np.arange(2018, 4500, 18)); _subst(q, 10000 + np.arange(7500, 10000, 18))
    cases["hops_half"] = q
    # ... and one that cannot fit: a mismatch every 17 bases over the whole of chunk 1 = 588 accepted 16-base matches
    q = _long_hop_query(ref)
    _subst(q, 10000 + np.arange(16, 10000, 17))
    cases["hops_overflow"] = q
    # N and case: runs of N at position 0, across a 32-base word edge, across a sub-range edge (10 x 105 = 1050) and at the chunk's last base;
    # IUPAC letters and a lower-case n; chunk 1 has no ambiguous base but a soft-masked block; chunk 2 starts with an N
    q = _diverged(ref, 100000, 30000, rng)
    q[0:5] = ord("N"); q[60:70] = ord("N"); q[1045:1056] = ord("N"); q[9999] = ord("N"); q[4000] = ord("n")
    for k, c in enumerate(b"RYKMSWBDHV"):
        q[3000 + 37 * k] = c
    q[5000:5600] |= 0x20; q[12000:13000] |= 0x20          # (lower case)
    q[20000:20003] = ord("N")
    cases["n_and_case"] = q
    # thirteen chunks: one more than a workgroup's waves -- two workgroups, whose 24 waves race for 13 tickets; eleven draw none
    cases["thirteen_chunks"] = _diverged(ref, 20000, 130000, rng)
    return cases


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("seed_lds")
    ref = synth.random_genome(REF_LEN, np.random.default_rng(20251))
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx)
    want = {}
    for name, q in _cases(ref).items():
        o.set_query(q); o.run_to(1)
        s1 = o.seeds() + o.groups()
        o.run_to(8)
        want[name] = (q, s1, o.blocks(with_aln=True))
    o.close()
    return idx, want


@pytest.fixture(scope="module", params=["narrow", "wide"])
def gpu(request, world):
    a = capi.Aligner(world[0], wide=(request.param == "wide"))
    a.set_option("seed_lhop", LHOP_N)
    yield a
    a.close()


def _stage1(g, q):
    g.set_query(q); g.run_to(1)
    return g.seeds() + g.groups()


def _check(g, world, name, stays=True):
    """stays: no chunk of the case may be handed to the dense kernels -- those stage the query themselves, and a chunk that goes to them says
    nothing about the speculative kernel's LDS layout.  (1 % divergence: ~100 accepted matches per chunk + at most one hop per speculative
    sub-range, under 256 entries; a few tens of wave-iterations of the budget of 256.)"""
    q, s1, blocks = world[1][name]
    got = _stage1(g, q)
    handed = int(g.seed_stats()[1])
    print(f"{name}: {handed} chunks handed over")
    assert not stays or handed == 0, (name, handed)
    for k, (a, b) in enumerate(zip(got, s1)):
        assert a.shape == b.shape and np.array_equal(a, b), (name, ("qpos", "len", "rpos", "gbeg", "gend")[k])
    assert s1[0].size > 0, name
    g.align_contig(q); full = g.blocks_as_dump(with_aln=True)
    for k, v in blocks.items():
        assert np.array_equal(full[k], v), (name, k)
    return got, handed


@pytest.mark.parametrize("n", [9999, 10000, 10001, 20000, 29999])
def test_chunk_edge_lengths(gpu, world, n):
    _check(gpu, world, f"edge_{n}")


def _chain_hops(s1, chunk):
    """Accepted matches of the true chain that start in `chunk`: each is one long hop (len + 1 >= 16) in that chunk's table."""
    qpos = np.unique(s1[0])
    return int(((qpos >= chunk * CHUNK) & (qpos < (chunk + 1) * CHUNK)).sum())


def test_long_hops_fill_half_the_table(gpu, world):
    q, s1, _ = world[1]["hops_half"]
    n = _chain_hops(s1, 1)
    assert LHOP_N // 2 <= n <= LHOP_N - 2 * NSUB, n      # (the input is what it is meant to be: half the table from the chain, room for the speculative walks' hops)
    assert np.diff(np.unique(s1[0])).max() > 2000        # hops far beyond the 2-bit codes
    _, handed = _check(gpu, world, "hops_half")
    print(f"hops_half: {n} chain hops in chunk 1, {handed} chunks handed over")


def test_long_hop_table_overflow_hands_the_chunk_over(gpu, world):
    q, s1, _ = world[1]["hops_overflow"]
    n = _chain_hops(s1, 1)
    assert n > LHOP_N, n                                  # more hops on the true chain than the table has entries
    _, handed = _check(gpu, world, "hops_overflow", stays=False)
    assert handed >= 1, handed                            # the chunk went to the dense kernels -- and the seeds are still the oracle's
    print(f"hops_overflow: {n} chain hops in chunk 1, {handed} chunks handed over")


def test_ambiguous_bases_and_case(gpu, world):
    _check(gpu, world, "n_and_case")


def test_thirteen_chunks_twice_on_one_context(gpu, world):
    a, _ = _check(gpu, world, "thirteen_chunks")
    b, _ = _check(gpu, world, "thirteen_chunks")          # (which wave gets which chunk differs from run to run: the result may not)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
