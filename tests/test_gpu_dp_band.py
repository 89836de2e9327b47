"""The band class of the striped gap DP (k_dp_band.hip: two near-diagonal jobs per wavefront inside a window of 128 diagonals, an exactness
certificate per job, fall-back to k_dp_stripe) against the oracle's ksw2, job by job, through Aligner.ksw2_batch; every batch is called twice, so
that buffers and tags are reused.  dp_band = 2 sends every job the layout admits through the band, small margins (B = 4, 8) put the band's edges
within reach of small jobs.  What the library must report (gsa_get_dp_band_stats: evaluated, certified, fallen back) is restated in dp_band_ref.py
from the REFERENCE's alignments: a job is certified exactly when the reference's score exceeds UB."""
import numpy as np
import pytest

import dp_band_ref as br
from gsalign_amd import capi, synth

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


def _rand(rng, n):
    return rng.integers(0, 4, n).astype(np.uint8)


def _subst(rng, a, rate):
    b = a.copy()
    hit = rng.random(b.size) < rate
    b[hit] = (b[hit] + rng.integers(1, 4, int(hit.sum()))) & 3
    return b


def _with_delta(rng, m, delta, rate=0.03):
    """reference side of m bases; query side = the same with substitutions and ONE indel of |delta| bases in the middle (n = m + delta)"""
    a = _rand(rng, m)
    b = _subst(rng, a, rate)
    k = m // 2
    b = np.concatenate([b[:k], _rand(rng, delta), b[k:]]) if delta >= 0 else np.concatenate([b[:k + delta // 2], b[k + delta // 2 - delta:]])
    return ACGT[a].tobytes(), ACGT[b].tobytes()


def _excursion(rng, m, B, over):
    """identical sides but for B + over bases inserted at m / 4 and B + over bases deleted 60 columns on: the optimal path runs on diagonal
    B + over in between -- the band's last diagonal (over = 0), or the first one outside (over = 1)"""
    a = _rand(rng, m); g = B + over; k = m // 4
    b = np.concatenate([a[:k], (a[k:k + g] + 2) & 3, a[k:k + 60], a[k + 60 + g:]])      # (inserted bases differ from the ones they stand in front of)
    return ACGT[a].tobytes(), ACGT[b].tobytes()


def _limits(minlen, B):
    """largest n - m >= 0 and smallest n - m <= 0 the layout admits at this size, restated"""
    up = max(d for d in range(0, 140) if br.fits(minlen, minlen + d, B))
    dn = min(d for d in range(-140, 1) if br.fits(minlen - d, minlen, B))
    assert not br.fits(minlen, minlen + up + 1, B) and not br.fits(minlen - dn + 1, minlen, B)
    return up, dn


def _cases(B, seed):
    rng = np.random.default_rng(seed)
    P = []
    for minlen in (65, 66, 128, 129, 200):
        up, dn = _limits(minlen, B)
        for d in (0, 1, -1, B, -B, up, dn, up + 1, dn - 1):
            P.append(_with_delta(rng, minlen if d >= 0 else minlen - d, d))
    for m in (130, 201):
        P.append(_excursion(rng, m, B, 0)); P.append(_excursion(rng, m, B, 1))
        s1, s2 = _excursion(rng, m, B, 0); P.append((s2, s1))                      # ... and on the other side of the band
        s1, s2 = _excursion(rng, m, B, 1); P.append((s2, s1))
    a = _rand(rng, 150)
    P.append((ACGT[a].tobytes(), ACGT[a].tobytes()))                               # identical: certified (score m)
    P.append((ACGT[a].tobytes(), ACGT[_rand(rng, 152)].tobytes()))                 # unrelated
    P.append((ACGT[a].tobytes(), ACGT[_subst(rng, a, 0.3)].tobytes()))             # 30 % diverged
    for k in range(3):                                                             # N on both sides
        s1, s2 = _with_delta(rng, 140 + k, (0, 3, -2)[k])
        s1 = bytearray(s1); s2 = bytearray(s2)
        for q in rng.integers(0, len(s1), 6): s1[q] = ord("N")
        for q in rng.integers(0, len(s2), 6): s2[q] = ord("n")
        s1[70] = s2[70] = ord("N")
        P.append((bytes(s1), bytes(s2)))
    unit = _rand(rng, 4)
    while len(set(unit.tolist())) < 3: unit = _rand(rng, 4)
    t = np.resize(unit, 160)
    P.append((ACGT[t].tobytes(), ACGT[t[:156]].tobytes()))                         # a tandem of a 4-base unit, one unit deleted: ties everywhere
    P.append((ACGT[t[:156]].tobytes(), ACGT[t].tobytes()))
    P.append((b"A" * 100, b"A" * 97)); P.append((b"A" * 97, b"A" * 100)); P.append((b"C" * 80 + b"G" * 40, b"C" * 76 + b"G" * 44))      # homopolymers
    return P


@pytest.fixture(scope="module")
def want_of(oracle_built):
    memo = {}

    def f(s1, s2):
        if (s1, s2) not in memo: memo[(s1, s2)] = oracle_built.oracle_ksw2(s1, s2)
        return memo[(s1, s2)]
    return f


def _run(a, P, want_of, B, what, admitted=None):
    """both calls give the oracle's strings, and the counters move by what the restated certificate says"""
    s1 = [p[0] for p in P]; s2 = [p[1] for p in P]
    want = [want_of(x, y) for x, y in P]
    adm = [br.is_striped(len(x), len(y)) and br.fits(len(x), len(y), B) for x, y in P] if admitted is None else admitted
    n_adm = sum(adm); n_cert = sum(1 for k in range(len(P)) if adm[k] and br.certified(len(s1[k]), len(s2[k]), B, want[k]))
    before = [int(v) for v in a.dp_band_stats()]
    for rep in range(2):
        ops = a.ksw2_batch(s1, s2)
        for i in range(len(P)):
            assert capi.apply_ops(s1[i], s2[i], ops[i]) == want[i], f"{what}: rep {rep} job {i} m={len(s1[i])} n={len(s2[i])}"
    after = [int(v) for v in a.dp_band_stats()]
    got = [y - x for x, y in zip(before, after)]
    print(f"{what}: B={B} jobs={len(P)} admitted={n_adm} certified={n_cert} counters={got}")
    assert got == [2 * n_adm, 2 * n_cert, 2 * (n_adm - n_cert)], (what, got, n_adm, n_cert)
    return n_adm, n_cert


@pytest.mark.parametrize("B", [4, 8])
def test_constructed_jobs(cx_index, want_of, B):
    """n - m in {0, +-1, +-B, the layout's limit either way, one past it}, shorter sides 65, 66, 128, 129, 200; a path on the band's last diagonal and one
    on the first diagonal outside (either side); identical, unrelated, 30 % diverged; N on both sides; a tandem with a unit deleted, homopolymers.  First
    each job with a partner of another kind (two jobs per wavefront), then all in one batch."""
    P = _cases(B, 40 + B)
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_band", 2); a.set_option("dp_band_margin", B)
        n_adm = n_cert = 0
        for k in range(0, len(P), 7):
            x, y = _run(a, P[k:k + 7], want_of, B, f"jobs {k}..")
            n_adm += x; n_cert += y
        x, y = _run(a, P, want_of, B, "all jobs")
        assert (x, y) == (n_adm, n_cert)
        assert 0 < n_cert < n_adm < len(P)      # certified, fallen back and refused by the layout: all three occur
        # the edge cases are what they claim: the reference's path reaches diagonal B (kept) / B + 1 (falls back)
        for m in (130, 201):
            for over, keep in ((0, True), (1, False)):
                s1, s2 = _excursion(np.random.default_rng(1), m, B, over)
                w = want_of(s1, s2)
                d = np.cumsum((np.frombuffer(w[0], np.uint8) == 45).astype(int) - (np.frombuffer(w[1], np.uint8) == 45).astype(int))
                assert int(d.max()) == B + over and int(d.min()) >= 0 and br.certified(len(s1), len(s2), B, w) == keep
    finally:
        a.close()


def test_mixed_batch_and_half_certified_pair(cx_index, want_of):
    """One batch of certified, uncertified, refused (100 x 170, 180 x 100: n - m past the layout), small-class (40 x 40) and one-wave-class (4000 x 65) jobs at the
    default margin; then, at dp_pair = 2, two striped jobs that share a wavefront of k_dp_stripe<4, 1> with exactly one of them certified: the pair
    runs and rewrites the certified partner's bytes."""
    rng = np.random.default_rng(50)
    P = [_with_delta(rng, 150, 0), _with_delta(rng, 300, 5), _with_delta(rng, 90, -20), (ACGT[_rand(rng, 150)].tobytes(), ACGT[_rand(rng, 150)].tobytes()),
         _with_delta(rng, 100, 70), _with_delta(rng, 40, 0), _with_delta(rng, 100, -80), _with_delta(rng, 4000, 65 - 4000), _with_delta(rng, 700, 10), _with_delta(rng, 1400, -33)]
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_band", 2)
        n_adm, n_cert = _run(a, P, want_of, 32, "mixed batch")
        assert (n_adm, n_cert) == (6, 5)         # (150 x 150, 300 x 305, 110 x 90, 700 x 710, 1433 x 1400 certified; the unrelated 150 x 150 falls back)
        a.set_option("dp_pair", 2)
        n_adm, n_cert = _run(a, [P[0], P[3]], want_of, 32, "one certified partner")
        assert (n_adm, n_cert) == (2, 1)
        jobs, paired = (int(v) for v in a.dp_stats()[:2])
        assert paired >= 4                       # (the two calls of the last batch ran their jobs side by side)
    finally:
        a.close()


def _long_related(rng, m, n):
    """m x n near DP_BAND_MAX_LEN: 2 % substitutions, one 20-base insertion and one 20-base deletion (and the indel that n - m asks for, in the middle)"""
    a = _rand(rng, m)
    b = _subst(rng, a, 0.02)
    b = np.concatenate([b[:m // 4], _rand(rng, 20), b[m // 4:3 * m // 4], b[3 * m // 4 + 20:]])
    k = m // 2
    b = np.concatenate([b[:k], _rand(rng, n - m), b[k:]]) if n >= m else np.concatenate([b[:k], b[k + m - n:]])
    assert b.size == n
    return ACGT[a].tobytes(), ACGT[b].tobytes()


def _with_six_n(rng, pair):
    s1, s2 = bytearray(pair[0]), bytearray(pair[1])
    for q in rng.choice(len(s1), 3, replace=False): s1[q] = ord("N")
    for q in rng.choice(len(s2), 3, replace=False): s2[q] = ord("N")
    return bytes(s1), bytes(s2)


def test_single_jobs_at_the_stated_limit(cx_index, want_of):
    """The band's absolute 16-bit scores are argued for sides up to DP_BAND_MAX_LEN = 5000 (gsa_dp.h): 5000 x 5000 identical (certified); with 2 %
    substitutions and two 20-base indels (at this length that optimum is already below UB), unrelated, and A...A against C...C -- every column a mismatch,
    the lowest scores a window can hold --, which fall back; n - m at the largest value either way that the layout and the length limit admit at this
    size, 2 % diverged and 0.5 % diverged (certified: walked back inside the band); one base past the length limit either way: refused, not counted.  One
    job per batch: its partner half of the wavefront is empty."""
    rng = np.random.default_rng(60)
    B = 32
    a = _rand(rng, 5000)
    up, dn = _limits(4940, B)
    assert (up, dn) == (60, -60)                  # (here the length limit binds first: 4940 + 60 = 5000 ...)
    up2, _ = _limits(4937, B); _, dn2 = _limits(4938, B)
    assert (up2, dn2) == (63, -62)                # (... and here the 128 diagonals do, with the longer side at 5000)
    singles = [("identical", (ACGT[a].tobytes(), ACGT[a].tobytes()), True), ("related", _long_related(rng, 5000, 5000), True),
               ("unrelated", (ACGT[a].tobytes(), ACGT[_rand(rng, 5000)].tobytes()), True), ("A against C", (b"A" * 5000, b"C" * 5000), True),
               ("4940 x 5000", _long_related(rng, 4940, 4940 + up), True), ("5000 x 4940", _long_related(rng, 4940 - dn, 4940), True),
               ("4937 x 5000", _long_related(rng, 4937, 4937 + up2), True), ("5000 x 4938", _long_related(rng, 4938 - dn2, 4938), True),
               ("4940 x 5000, close", _with_delta(rng, 4940, up, rate=0.005), True), ("5000 x 4940, close", _with_delta(rng, 4940 - dn, dn, rate=0.005), True),
               ("5001 x 5000", _long_related(rng, 5001, 5000), False), ("5000 x 5001", _long_related(rng, 5000, 5001), False)]
    g = capi.Aligner(cx_index)
    try:
        g.set_option("dp_band", 2)
        cert = {}
        for what, pair, admitted in singles:
            assert br.fits(len(pair[0]), len(pair[1]), B) == admitted, what
            n_adm, n_cert = _run(g, [pair], want_of, B, what)
            assert n_adm == int(admitted), what
            cert[what] = n_cert
        assert cert["identical"] == cert["4940 x 5000, close"] == cert["5000 x 4940, close"] == 1 and cert["unrelated"] == cert["A against C"] == 0, cert
    finally:
        g.close()


def test_long_and_short_job_share_a_wavefront(cx_index, want_of):
    """The band list pairs neighbours in (m + n) order: a batch of two jobs puts them into the two halves of ONE wavefront.  5000 x 5000 beside 65 x 66: the
    short job's half goes on computing for thousands of steps past its end.  The same with six N in the long job only and in the short job only (the
    kernel's "has an N" form is chosen per pair, not per job), and a 4999 x 5000 unrelated job that falls back beside a 66 x 65 identical one that is
    certified."""
    rng = np.random.default_rng(61)
    B = 32
    long_, short = _with_delta(rng, 5000, 0, rate=0.005), _with_delta(rng, 65, 1)      # (0.5 % substitutions: the long job is certified -- it walks back inside the band)
    x = _rand(rng, 66)
    batches = [("long + short", [long_, short]), ("N in the long job", [_with_six_n(rng, long_), short]), ("N in the short job", [long_, _with_six_n(rng, short)]),
               ("one certified partner", [(ACGT[_rand(rng, 4999)].tobytes(), ACGT[_rand(rng, 5000)].tobytes()), (ACGT[x].tobytes(), ACGT[x[:65]].tobytes())])]
    g = capi.Aligner(cx_index)
    try:
        g.set_option("dp_band", 2)
        for what, P in batches:
            assert [(len(p[0]), len(p[1])) for p in P] in ([(5000, 5000), (65, 66)], [(4999, 5000), (66, 65)])
            n_adm, n_cert = _run(g, P, want_of, B, what)
            assert n_adm == 2 and n_cert == (1 if what == "one certified partner" else 2), (what, n_adm, n_cert)
    finally:
        g.close()


def test_default_rule_on_a_contig(oracle_built, tmp_path):
    """The benchmark's generator at 4 Mb, -alen 5000, default options: every stage-8 array equals the oracle's, jobs are certified, and as many fall
    back as the restated certificate says of the reference's gap alignments -- at B = 32 none."""
    from gsalign_amd import hostlib, indexio
    refs, qrys = synth.make_pair_fast(4_000_000, 1, 0.01, seed=11, repeats=True)
    fa, px = str(tmp_path / "r.fa"), str(tmp_path / "r")
    synth.write_fasta(fa, refs); hostlib.build_index(fa, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx, dict(alen=5000))
    o.set_query(qrys[0][1]); o.run_to(8); want = o.blocks(with_aln=True); o.close()
    al = want["f_alnlen"].astype(np.int64); off = np.concatenate([[0], np.cumsum(al)])
    fail = 0
    for i in np.flatnonzero((want["f_bseed"] == 0) & (al > 0)):
        m, n = int(want["f_rlen"][i]), int(want["f_qlen"][i])
        if m > 0 and n > 0 and br.is_striped(m, n) and br.fits(m, n, 32):
            fail += not br.certified(m, n, 32, (want["aln1"][off[i]:off[i] + al[i]].tobytes(), want["aln2"][off[i]:off[i] + al[i]].tobytes()))
    g = capi.Aligner(idx, alen=5000)
    try:
        for rep in range(2):
            d = capi.result_as_dump(g.align_contig(qrys[0][1]), with_aln=True)
            for key, v in want.items():
                assert np.array_equal(d[key], v), (rep, key)
        ev, cert, fell = (int(v) for v in g.dp_band_stats())
        print(f"contig: evaluated={ev} certified={cert} fallen back={fell} predicted to fall back={2 * fail}")
        assert cert > 0 and ev == cert + fell and fell == 2 * fail == 0
    finally:
        g.close()
