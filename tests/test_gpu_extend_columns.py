"""The extend stage's string writer and gap classifier work a lane per string column (csrc/k_extend.hip: k_gap_class, k_materialize;
tile_scan / tile_find / seg_mask): the records of a tile of 256 are laid out column by column and wavefronts take the columns in
chunks of 64, so a record may begin and end anywhere in a chunk, run over several chunks, wavefront shares and -- its neighbours --
tile edges, and a DP record's consumed-base counts are carried from chunk to chunk.

Every case: the finished blocks of gsa_align_contig with both gapped strings against the oracle's stage 8 -- exact, in both index
layouts.  Inputs are synthetic with fixed seeds; the oracle's side is computed once per module, and every case first asserts ON THE
ORACLE'S RESULT that the record shapes it is there for occur (string lengths <= 32, 33-64, > 64; DP and other gaps; large DP jobs, which
k_materialize must pass over), so a change of a generator cannot empty it silently."""
import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu

REF_LEN = 200_000
FLANK = 200            # exact bases between two planted runs
MAX_MISMATCH = 5       # GSA_MAX_MISMATCH: an equal-length gap with more mismatches goes to DP

# a run of k rotated bases between exact flanks is one equal-length gap (k, k).  Up to 5 it stays an equal-length record of k columns; from 6
# on it is a DP record whose string is the DP's op string (k columns or a few more: that depends on the bases); 31-34 and 63-66 lie around
# the chunk length and its half; from k = 65 on the job is a large (striped) one -- more than 64 query bases, or more than 128 anti-diagonals
# -- which k_materialize must pass over.
RUN_KS = tuple(range(1, 10)) + (31, 32, 33, 34, 63, 64, 65, 66, 70, 129, 200)
RUN_LARGE_FROM = 65
# the string length the oracle gives every run on this reference (fixed seeds), per case: a change of a generator shows here first
RUN_ALNLEN = {"runs": {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 11, 31: 33, 32: 34, 33: 36, 34: 37, 63: 68, 64: 73, 65: 69, 66: 69, 70: 74, 129: 136, 200: 217},
              "few": {3: 3, 8: 9, 33: 37, 65: 70, 129: 136}}


def _rot(q, pos):
    """A guaranteed mismatch at every position of `pos`: the base rotated within ACGT."""
    code = np.zeros(256, np.uint8); code[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4, dtype=np.uint8)
    q[pos] = np.frombuffer(b"ACGT", np.uint8)[(code[q[pos]] + 1) & 3]


def _diverged(ref, a, n, rng):
    """n bases: ref[a:] with the usual 1 % event mix (substitutions and short indels): the mass of short records."""
    return np.ascontiguousarray(synth.mutate(ref[a:a + n + 2000], 0.01, rng)[:n])


def _runs_query(ref, a, n, ks):
    """n bases, a clean colinear copy of ref[a:a + n] with a run of k rotated bases for every k of `ks`, FLANK exact bases apart.
    Returns the query, {k: query position of the run} and the position behind the last run."""
    q = ref[a:a + n].copy()
    pos, at = 1000, {}
    for k in ks:
        _rot(q, np.arange(pos, pos + k)); at[k] = pos
        pos += k + FLANK
    return q, at, pos


def _cases(ref):
    rng = np.random.default_rng(20270)
    cases, planted = {}, {}
    # substitution runs of every length at which the writer changes its way: 1-5 stay equal-length records, 6-9 the first DP records,
    # 31-34 / 63-66 around the chunk length and its half, three large jobs
    q, at, pos = _runs_query(ref, 20000, 30000, RUN_KS)
    extra = {}
    _rot(q, pos + np.array([0, 5, 10, 15, 20])); extra["eq21"] = pos; pos += 21 + FLANK           # five mismatches over 21 bases: still FT_EQ, (21, 21, 21)
    _rot(q, pos + np.array([0, 5, 10, 15, 20, 25])); extra["dp26"] = pos; pos += 26 + FLANK       # six over 26 bases: DP
    _rot(q, pos + np.array([0, 4])); q[pos + 2] = ord("N"); extra["eqN"] = pos; pos += 5 + FLANK      # a query N inside an equal-length gap: skipped by the count
    _rot(q, pos + np.array([0, 6])); q[pos + 3] = ord("n"); extra["eqn"] = pos; pos += 7 + FLANK      # ... and a lower-case n
    cases["runs"] = q; planted["runs"] = (at, extra)
    # fewer than 64 records: less than one chunk of records, a tile with three idle wavefronts
    q, at, _ = _runs_query(ref, 60000, 30000, (3, 8, 33, 65, 129))
    cases["few"] = q; planted["few"] = (at, {})
    # the 1 % background: about a thousand records, whose gaps meet chunk, wavefront-share and tile edges wherever they fall
    cases["background"] = _diverged(ref, 90000, 60000, rng)
    # two blocks in one contig (the second piece on the reverse strand): a tile straddles the block edge and adds per record
    cases["two_blocks"] = np.concatenate([_diverged(ref, 30000, 40000, rng), synth.revcomp(_diverged(ref, 120000, 40000, rng))])
    # the pool-consistency pair and the bundle: a larger contig first, three short ones
    cases["larger"] = _diverged(ref, 5000, 120000, rng)
    for k in range(3):
        cases[f"short{k}"] = _diverged(ref, 10000 + 50000 * k, 30000 + 1500 * k, rng)
    return cases, planted


def _shapes(d):
    """What the oracle's stage-8 dump holds: record counts by string length, DP and other gaps, large DP jobs."""
    gap = d["f_bseed"] == 0
    ql, rl, al = d["f_qlen"][gap].astype(np.int64), d["f_rlen"][gap].astype(np.int64), d["f_alnlen"][gap].astype(np.int64)
    # mismatches of every gap's strings (positions where the query is not ACGT do not count): an equal-length gap with at most MAX_MISMATCH is no DP gap
    code = np.full(256, 4, np.uint8)
    for k, c in enumerate(b"ACGT"):
        code[c] = k; code[c | 0x20] = k
    a1, a2 = code[d["aln1"]], code[d["aln2"]]
    bad = ((a2 != 4) & (a1 != a2)).astype(np.int64)
    csum = np.concatenate([[0], np.cumsum(bad)]); off = np.concatenate([[0], np.cumsum(al)])
    mism = csum[off[1:]] - csum[off[:-1]]
    dp = (ql > 0) & (rl > 0) & ~((ql == rl) & (al == ql) & (mism <= MAX_MISMATCH))
    large = dp & ~((ql <= 64) & (ql + rl - 1 <= 128))
    # where the columns of the small DP records fall, as k_materialize lays them out: tiles of 256 records in the dump's order (the device's order
    # for a contig of one block), seeds and large jobs without columns, chunks of 64 columns, a contiguous share of ceil(chunks / 4) chunks for each of
    # the four wavefronts.  dp_chunk: small DP records that run over a chunk edge (the carry); dp_share: ... over the first column of a share
    # (the count of the ops in front of the share)
    L = np.zeros(d["f_bseed"].size, np.int64); L[gap] = np.where(large, 0, al)
    small = np.zeros(L.size, bool); small[gap] = dp & ~large
    dp_chunk = dp_share = 0
    for t0 in range(0, L.size, 256):
        Lt = L[t0:t0 + 256]; first = np.cumsum(Lt) - Lt; last = first + Lt - 1
        T = int(Lt.sum()); cw = ((T + 63) // 64 + 3) // 4
        sm = small[t0:t0 + 256]
        dp_chunk += int((sm & (first // 64 != last // 64)).sum())
        for w in (1, 2, 3):
            m = 64 * cw * w
            if m < T:
                dp_share += int((sm & (first < m) & (m <= last)).sum())
    return dict(dp_chunk=dp_chunk, dp_share=dp_share, nrec=int(d["f_bseed"].size), nblk=int(d["b_nfrag"].size), le32=int(((al > 0) & (al <= 32)).sum()), le64=int(((al > 32) & (al <= 64)).sum()),
                gt64=int((al > 64).sum()), dp=int(dp.sum()), other=int((~dp).sum()), large=int(large.sum()), nfrag=[int(x) for x in d["b_nfrag"]])


def _gap_at(d, qpos):
    """(qlen, rlen, aln_len) of the gap record that starts at query position qpos."""
    k = np.flatnonzero((d["f_bseed"] == 0) & (d["f_qpos"] == qpos))
    assert k.size == 1, (qpos, k)
    return int(d["f_qlen"][k[0]]), int(d["f_rlen"][k[0]]), int(d["f_alnlen"][k[0]])


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("extend_columns")
    ref = synth.random_genome(REF_LEN, np.random.default_rng(20271))
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    cases, planted = _cases(ref)
    o = oracle_built.Oracle(idx)
    want = {}
    for name, q in cases.items():
        assert 30000 <= q.size <= 120000, (name, q.size)
        o.set_query(q); o.run_to(8)
        dump = o.blocks(with_aln=True)
        want[name] = (q, dump, _shapes(dump))
        print(name, want[name][2])
    o.close()
    return idx, want, planted


@pytest.fixture(scope="module", params=["narrow", "wide"])
def gpu(request, world):
    """(aligner, wide): a context per index layout."""
    a = capi.Aligner(world[0], wide=(request.param == "wide"))
    yield a, request.param == "wide"
    a.close()


def _check(g, world, name):
    q, want, _ = world[1][name]
    res = g.align_contig(q)
    got = capi.result_as_dump(res, with_aln=True)
    for k, v in want.items():
        assert np.array_equal(got[k], v), (name, k)
    return res


def _planted_runs_are_there(world, name):
    """The planted runs came out as the gap records they were planted for (on the oracle's result)."""
    _, dump, sh = world[1][name]
    at, extra = world[2][name]
    for k, pos in at.items():
        ql, rl, al = _gap_at(dump, pos)
        assert (ql, rl, al) == (k, k, RUN_ALNLEN[name][k]), (name, k, ql, rl, al)
    assert sh["large"] == sum(1 for k in at if k >= RUN_LARGE_FROM), (name, sh)
    return dump, sh, extra


def test_substitution_runs_of_every_length(gpu, world):
    dump, sh, extra = _planted_runs_are_there(world, "runs")
    assert _gap_at(dump, extra["eq21"]) == (21, 21, 21)              # five mismatches: no DP
    ql, rl, al = _gap_at(dump, extra["dp26"]); assert (ql, rl) == (26, 26)
    assert _gap_at(dump, extra["eqN"]) == (5, 5, 5) and _gap_at(dump, extra["eqn"]) == (7, 7, 7)
    # 1-5, eq21, eqN, eqn: 8 other gaps; 6-9, 31-34, 63-66, 70, 129, 200 and dp26: 16 DP gaps, five of them large jobs
    assert sh["other"] == 8 and sh["dp"] == 16 and sh["large"] == 5, sh
    assert sh["le32"] == 13 and sh["le64"] == 4 and sh["gt64"] == 7, sh
    assert sh["nblk"] == 1 and sh["dp_chunk"] >= 2 and sh["dp_share"] >= 2, sh      # small DP records over chunk edges and over the first column of a wavefront's share
    _check(gpu[0], world, "runs")


def test_fewer_records_than_a_chunk(gpu, world):
    _, sh, _ = _planted_runs_are_there(world, "few")
    assert sh["nrec"] < 64 and sh["dp"] == 4 and sh["other"] == 1 and sh["large"] == 2, sh
    assert sh["le32"] == 2 and sh["le64"] == 1 and sh["gt64"] == 2, sh
    _check(gpu[0], world, "few")


def test_background_of_short_records(gpu, world):
    sh = world[1]["background"][2]
    # 60 kb at 1 %: ~600 events, so several tiles of records and a last tile that is not full; insertions, deletions, equal-length and DP gaps
    assert sh["nrec"] > 512 and sh["nrec"] % 256 != 0, sh
    assert sh["le32"] >= 300 and sh["dp"] >= 50 and sh["other"] >= 200 and sh["le64"] >= 2 and sh["gt64"] >= 2 and sh["large"] >= 2, sh
    assert sh["nblk"] == 1 and sh["dp_chunk"] >= 3 and sh["dp_share"] >= 1, sh
    _check(gpu[0], world, "background")


def test_tile_straddles_a_block_edge(gpu, world):
    sh = world[1]["two_blocks"][2]
    assert sh["nblk"] >= 2 and sh["nfrag"][0] % 256 != 0 and sh["nfrag"][0] > 256 and sh["nfrag"][1] > 256, sh      # the block edge lies inside a tile
    assert sh["le32"] >= 300 and sh["dp"] >= 50 and sh["other"] >= 200 and sh["le64"] >= 1 and sh["gt64"] >= 2 and sh["large"] >= 2, sh
    _check(gpu[0], world, "two_blocks")


def _same_result(a, b, what):
    for k in ("blocks", "frags", "aln1", "aln2"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


def test_pools_do_not_depend_on_the_previous_contig(gpu, world):
    """A larger contig, then a smaller one on the same context: the smaller one's raw string pools -- the bytes no record owns included --
    are those of a fresh context."""
    sh = world[1]["larger"][2]
    assert sh["nrec"] > world[1]["runs"][2]["nrec"] and sh["le32"] >= 600 and sh["dp"] >= 100 and sh["le64"] >= 2 and sh["gt64"] >= 5 and sh["large"] >= 5, sh
    assert sh["nblk"] == 1 and sh["dp_chunk"] >= 10 and sh["dp_share"] >= 2, sh
    _check(gpu[0], world, "larger")
    second = _check(gpu[0], world, "runs")
    fresh = capi.Aligner(world[0], wide=gpu[1])
    try:
        first = fresh.align_contig(world[1]["runs"][0])
    finally:
        fresh.close()
    assert second["aln1"].size > int(second["frags"]["aln_len"].sum())       # (there IS slack: a DP gap's room is m + n)
    _same_result(second, first, "runs after larger")


def test_bundle_of_three_short_contigs(gpu, world):
    """gsa_align_many puts the three into one pass (one record list, one pair of pools, block edges inside tiles): every contig's result is
    what it gets alone, and the oracle's."""
    names = [f"short{k}" for k in range(3)]
    for n in names:
        sh = world[1][n][2]
        assert sh["le32"] >= 150 and sh["dp"] >= 25 and sh["other"] >= 100 and sh["le64"] >= 1, (n, sh)
    alone = [_check(gpu[0], world, n) for n in names]
    out = {}

    def on_result(ci, res):
        out[ci] = gpu[0]._result(res)
        return 0
    capi.align_many([gpu[0]], [world[1][n][0] for n in names], on_result)
    assert sorted(out) == [0, 1, 2]
    for k, n in enumerate(names):
        got = capi.result_as_dump(out[k], with_aln=True)
        for key, v in world[1][n][1].items():
            assert np.array_equal(got[key], v), (n, key)
        _same_result(out[k], alone[k], n)
