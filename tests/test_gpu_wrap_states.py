"""The counters a context never resets, at the launch where each comes round (DESIGN, "Counters that are never reset"): the 16-bit epoch of the striped DP's
boundary granules, the tag of the band class's certificate flags, the 30-bit epoch of the look-back status words, the fused passes' 32-bit ticket, and the
epoch and ticket of the sliced window-chain walk.  The test hooks "dbg_*" (gsa_set_option) put a counter just below its wrap; an epoch only moves forward,
so the hook itself makes no stale word valid.  Every test first runs the context in its young state, so that the buffers hold words tagged with the very
epochs the counter restarts at, at the offsets the wrapped launch reads; asserts through Aligner.launch_counters() that the wrap happened and that the
buffer was not replaced in between (a fresh buffer is cleared anyway, which would hide the wrap path); and compares bit-exactly with the committed
goldens or the oracle, never with another run of the library."""
import os

import numpy as np
import pytest

import dp_band_ref as br
from conftest import GOLDEN, assert_stage_equal
from gsalign_amd import capi, synth
from test_gpu_dp_pairs import _pair

pytestmark = pytest.mark.gpu

LB_EPOCH, LB_TICKET, DP_EPOCH, BAND_EPOCH, WALK_EPOCH, WALK_TICKET, WALK_SLICES, BND_BYTES = range(8)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _counters(a):
    return [int(v) for v in a.launch_counters()]


def _ops_equal(a, s1, s2, want, what):
    ops = a.ksw2_batch(s1, s2)
    for i in range(len(s1)):
        assert capi.apply_ops(s1[i], s2[i], ops[i]) == want[i], f"{what}: job {i} m={len(s1[i])} n={len(s2[i])}"


def test_hooks_move_counters_forward_only(cx_index):
    """An epoch hook refuses a value below the counter's and one outside its width, and changes nothing then; the chain-walk hooks refuse a context that
    has not walked a chain in slices yet; a ticket hook moves the host's value and the device word together (no drift afterwards)."""
    a = capi.Aligner(cx_index)
    try:
        v = _counters(a)
        assert v[DP_EPOCH] == v[BAND_EPOCH] == v[WALK_EPOCH] == v[WALK_TICKET] == v[WALK_SLICES] == v[BND_BYTES] == 0, v
        for name, top, at in (("dbg_dp_epoch", 0xffff, DP_EPOCH), ("dbg_band_epoch", 0xffffffff, BAND_EPOCH), ("dbg_lb_epoch", 0x3fffffff, LB_EPOCH)):
            cur = _counters(a)[at]
            a.set_option(name, cur + 7)
            for bad in (cur + 6, -1, top + 1):
                with pytest.raises(capi.GsaError):
                    a.set_option(name, bad)
            assert _counters(a)[at] == cur + 7
            a.set_option(name, top)
            assert _counters(a)[at] == top
        for name in ("dbg_walk_epoch", "dbg_walk_ticket"):
            with pytest.raises(capi.GsaError):
                a.set_option(name, 1)
        for bad in (-1, 1 << 32):
            with pytest.raises(capi.GsaError):
                a.set_option("dbg_lb_ticket", bad)
        a.set_option("dbg_lb_ticket", 0xfffffff0)
        assert _counters(a)[LB_TICKET] == 0xfffffff0      # (launch_counters raises on drift)
    finally:
        a.close()


# ---- (a) dp_epoch: 16 bits, tags the boundary granules that stripes hand over through HBM ----
# (m, n): two workgroups side by side; the lagged form with more than eight stripes (more than one workgroup); the one-wave class, where every hand-off
# goes through HBM; a neighbour
DP_SHAPES = [(130, 257), (130, 321), (200, 600), (300, 1100), (4000, 200), (4100, 129), (150, 129)]


@pytest.fixture(scope="module")
def dp_batches(oracle_built):
    """batches A and B: the same shapes in the same order, different sequences"""
    out = []
    for seed in (70, 71):
        rng = np.random.default_rng(seed)
        s1, s2 = (list(x) for x in zip(*[_pair(rng, m, n) for m, n in DP_SHAPES]))
        out.append((s1, s2, [oracle_built.oracle_ksw2(x, y) for x, y in zip(s1, s2)]))
    return out


@pytest.mark.parametrize("dp_pair", [0, 2])
def test_dp_epoch_wraps(cx_index, dp_batches, dp_pair):
    """A at the context's first epoch, the counter put to 0xffff, B: the launch wraps, and every offset B reads still holds A's granules, tagged 1 -- the
    epoch B restarts at.  Then, on a new context: A, the counter put to 0xfffe, B (tag 0xffff is a legal tag), A (wraps), B."""
    A, B = dp_batches
    for first, seq, expect in ((0xffff, (B,), (1,)), (0xfffe, (B, A, B), (0xffff, 1, 2))):
        a = capi.Aligner(cx_index)
        try:
            a.set_option("dp_pair", dp_pair); a.set_option("dp_band", 0)
            _ops_equal(a, *A, "A, young context")
            v = _counters(a)
            assert v[DP_EPOCH] == 1 and v[BND_BYTES] > 0, v
            held = v[BND_BYTES]
            a.set_option("dbg_dp_epoch", first)
            for k, (batch, e) in enumerate(zip(seq, expect)):
                _ops_equal(a, *batch, f"dp_pair {dp_pair}, from {first:#x}, launch {k}")
                v = _counters(a)
                print(f"dp_epoch: dp_pair {dp_pair} set {first:#x} launch {k}: epoch {v[DP_EPOCH]} bytes {v[BND_BYTES]}")
                assert v[DP_EPOCH] == e, v
                assert v[BND_BYTES] == held, "the boundary buffer was replaced: its clearing hides the wrap"
        finally:
            a.close()


# ---- (b) band_epoch: 32 bits, tags the certificate flags that let k_dp_stripe leave early ----
def test_band_epoch_wraps(cx_index, oracle_built):
    """A: six admitted jobs that certify (their flags carry tag 1).  The counter put to 2^32 - 1.  B: the same shapes, unrelated sequences: every job falls
    back -- with A's flags of tag 1 still in place the striped kernel would leave early and B's op strings would be the band's.  Then A again."""
    rng = np.random.default_rng(72)
    A, B = [], []
    for m in (150, 300, 700):
        x = rng.integers(0, 4, m).astype(np.uint8)
        y = x.copy(); hit = rng.random(m) < 0.03; y[hit] = (y[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
        A += [(ACGT[x].tobytes(), ACGT[x].tobytes()), (ACGT[x].tobytes(), ACGT[y].tobytes())]
        B += [(ACGT[rng.integers(0, 4, m)].tobytes(), ACGT[rng.integers(0, 4, m)].tobytes()) for _ in range(2)]
    wantA = [oracle_built.oracle_ksw2(x, y) for x, y in A]; wantB = [oracle_built.oracle_ksw2(x, y) for x, y in B]
    for P, want, cert in ((A, wantA, True), (B, wantB, False)):      # the batches are what they claim, by the restated certificate
        assert all(br.is_striped(len(x), len(y)) and br.fits(len(x), len(y), 32) and br.certified(len(x), len(y), 32, w) == cert for (x, y), w in zip(P, want))
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_band", 2)

        def call(P, want, moved, what):
            before = [int(v) for v in a.dp_band_stats()]
            _ops_equal(a, [p[0] for p in P], [p[1] for p in P], want, what)
            got = [int(y) - x for x, y in zip(before, a.dp_band_stats())]
            assert got == moved, (what, got)

        call(A, wantA, [6, 6, 0], "A, young context")
        assert _counters(a)[BAND_EPOCH] == 1
        a.set_option("dbg_band_epoch", 0xffffffff)
        call(B, wantB, [6, 0, 6], "B, the launch that wraps")
        assert _counters(a)[BAND_EPOCH] == 1
        call(B, wantB, [6, 0, 6], "B again")
        call(A, wantA, [6, 6, 0], "A again")
        assert _counters(a)[BAND_EPOCH] == 3
    finally:
        a.close()


# ---- (c) lb_epoch: 30 bits, tags the look-back status words of every fused pass ----
@pytest.mark.parametrize("golden,params", [("cx_stages.npz", {}), ("cx_sen_stages.npz", dict(sen=1, clr=50))])
def test_lb_epoch_wraps(cx_index, cx_queries, golden, params):
    """All eight contigs once: the early status words carry epochs 1 .. E.  Then the counter put to 2^30 - k and contig 0 again, k = 3, 17, 40 -- the wrap
    lands in a different stage each time, and the epochs behind it (at most E) are ones that this context has used on the same words before.  Contig 0
    makes 26 fused passes (measured; not the 50 of a contig with large gaps), so for k = 40 it runs twice and the second run's launch 14 comes round.  The
    -sen contigs have 8 000 - 23 000 seeds: many tiles per pass."""
    want = np.load(os.path.join(GOLDEN, golden))
    a = capi.Aligner(cx_index, **params)
    try:
        for ci, (name, seq) in enumerate(cx_queries):
            a.set_query(seq)
            assert_stage_equal(a.dump_stages(8), want, prefix=f"c{ci}_")
        E = _counters(a)[LB_EPOCH]
        a.set_query(cx_queries[0][1])
        assert_stage_equal(a.dump_stages(8), want, prefix="c0_")
        n0 = _counters(a)[LB_EPOCH] - E      # fused passes of contig 0
        for k in (3, 17, 40):
            a.set_option("dbg_lb_epoch", (1 << 30) - k)
            for run in range(-(-k // n0)):      # (as many runs of the contig as it takes to make k launches)
                a.set_query(cx_queries[0][1])
                assert_stage_equal(a.dump_stages(8), want, prefix="c0_")
            v = _counters(a)
            print(f"lb_epoch: {golden} set 2^30 - {k}: {v[LB_EPOCH]} after the contig's {n0} passes (E = {E})")
            assert 1 <= v[LB_EPOCH] <= E, (k, v, n0, E)      # launch k of the contig came round and took epoch 1: only epochs that this context has used on the same words before
    finally:
        a.close()


# ---- (d) the fused passes' ticket: 32 bits, modular; nothing to do at 2^32, `ticket - base` has to stay right ----
def test_lb_ticket_across_2_32(cx_index, cx_queries):
    """-sen contig 0: 23 269 seeds, about 23 tiles per pass.  The ticket put to 2^32 - k: k = 1, 2, 5 put 2^32 inside the tile numbers of one launch, 300
    between two launches.  Host and device still agree afterwards (launch_counters raises on drift)."""
    want = np.load(os.path.join(GOLDEN, "cx_sen_stages.npz"))
    assert want["c0_s1_qpos"].size == 23269
    a = capi.Aligner(cx_index, sen=1, clr=50)
    try:
        for k in (1, 2, 5, 300):
            a.set_option("dbg_lb_ticket", (1 << 32) - k)
            assert _counters(a)[LB_TICKET] == (1 << 32) - k
            a.set_query(cx_queries[0][1])
            assert_stage_equal(a.dump_stages(8), want, prefix="c0_")
            v = _counters(a)
            print(f"lb_ticket: set 2^32 - {k}: {v[LB_TICKET]} after the contig")
            assert v[LB_TICKET] < (1 << 20) and v[LB_TICKET] + k > 300, (k, v)      # came round: more than 300 draws per contig, far fewer than 2^20
    finally:
        a.close()


def test_ticket_holds_behind_the_contig_retry(cx_index, cx_queries):
    """gsa_align_contig's retry after a stripe hand-off time-out (test hook dp_fake_timeout, as tests/test_gpu_parity.py forces it): the first pass ends in
    an error behind all its fused passes, the second runs them again.  The device ticket and the host's value agree behind it, and the next contig is right."""
    want = np.load(os.path.join(GOLDEN, "cx_stages.npz"))
    a = capi.Aligner(cx_index)
    try:
        for rep, hook in enumerate((1, 0)):
            a.set_option("dp_fake_timeout", hook); a.set_profiling(False)
            before = _counters(a)[LB_TICKET]
            got = capi.result_as_dump(a.align_contig(cx_queries[0][1]), with_aln=True)
            for key, val in got.items():
                assert np.array_equal(want[f"c0_s8_{key}"], val), (rep, key)
            ms = (capi.C.c_double * 10)(); n = capi.C.c_int64()
            assert a.lib.gsa_get_wall_sums(a.ctx, ms, capi.C.byref(n)) == 0 and n.value == 1 + hook      # (gsa_run_to(8) ran twice where the hook was set)
            assert _counters(a)[LB_TICKET] > before      # no drift (launch_counters raises), and tickets were drawn
    finally:
        a.close()


# ---- (e) walk_epoch / walk_ticket: the sliced window-chain walk (k_walk_chain), entry words {epoch, rank} per slice ----
WALK_SCALE = 6          # synth.make_complex(2024, scale): the smallest scale at which a contig's candidate list fills more than one slice of 16 384
WALK_BIG, WALK_SMALL = 6, 4      # q7_gaps: 92 103 seeds, 22 706 candidates under -sen -- two slices; q5_rev: 9 053 seeds, 107 candidates -- one slice


@pytest.fixture(scope="module")
def walk_case(oracle_built, tmp_path_factory):
    from gsalign_amd import hostlib, indexio
    d = tmp_path_factory.mktemp("walk")
    refs, qrys = synth.make_complex(2024, scale=WALK_SCALE)
    fa, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(fa, refs); hostlib.build_index(fa, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx, dict(sen=1, clr=50))
    o.set_query(qrys[WALK_BIG][1]); want = o.dump_stages(8); o.close()
    return idx, qrys[WALK_SMALL][1], qrys[WALK_BIG][1], want


def test_walk_epoch_and_ticket_wrap(walk_case):
    """Input: synth.make_complex(2024, scale=6) under sen=1, clr=50, contig q7_gaps (the -sen golden's contig 0 has 459 candidates, one slice; q7_gaps has
    8 385 at scale 5 and 22 706 at scale 6, counted from the oracle's stage-1 seeds: two slices, and launch_counters()[6] == 2 on the device; 92 103 seeds: a grid of 6).  A one-slice contig first: it allocates the entry words with room to
    spare, and they stay zero.  Then the epoch put to 2^32 - 1 and the ticket to 2^32 - 1: the two-slice contig's launch is the one that comes round -- its
    epoch must not be 0, the tag of a word never written -- and its tickets straddle 2^32.  Then once more."""
    idx, small, big, want = walk_case
    grid = (want["s1_qpos"].size + 16383) // 16384
    a = capi.Aligner(idx, sen=1, clr=50)
    try:
        a.set_option("walk_chain_min", 0)
        a.set_query(small); a.run_to(8)
        v = _counters(a)
        assert v[WALK_EPOCH] == 1 and v[WALK_SLICES] == 1 and v[WALK_TICKET] == 1, v
        a.set_option("dbg_walk_epoch", 0xffffffff); a.set_option("dbg_walk_ticket", 0xffffffff)
        for rep in range(2):
            a.set_query(big)
            assert_stage_equal(a.dump_stages(8), want)
            v = _counters(a)      # (no drift: it raises)
            print(f"walk: rep {rep}: epoch {v[WALK_EPOCH]} ticket {v[WALK_TICKET]} slices {v[WALK_SLICES]} (grid {grid})")
            assert v[WALK_SLICES] >= 2, "the contig's chain stayed inside one slice: no entry word was read"
            assert v[WALK_EPOCH] == 1 + rep
            # (a replaced buffer restarts both counters at zero: the ticket would be (1 + rep) * grid)
            assert v[WALK_TICKET] == (1 + rep) * grid - 1 and grid >= 2, (v, grid)
    finally:
        a.close()
