"""The striped gap DP's side-by-side form (k_dp_stripe<4, 1>: two jobs in the two 16-bit halves of a wavefront, option dp_pair) against the oracle's
ksw2 (ksw2_alignment.cpp:74-95), pair by pair, through Aligner.ksw2_batch.  Every batch is called twice, so that buffers, tickets and the boundary
epoch are reused.  Shapes are the smallest at which the form can go wrong: the hand-off block is 8 rows, a direction dword 8 steps, a stripe's ramp 63
steps, a workgroup 4 stripes of each job."""
import os
import sys

import numpy as np
import pytest

from gsalign_amd import capi

pytestmark = pytest.mark.gpu

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")


def _pair(rng, m, n, kind="related", with_n=False):
    """A reference side of m and a query side of n bases: the query is the reference with substitutions and indels (cut / padded to n), the
    reference itself, or unrelated."""
    a = rng.integers(0, 4, m).astype(np.uint8)
    if kind == "unrelated":
        b = rng.integers(0, 4, n).astype(np.uint8)
    else:
        d = 0.0 if kind == "identical" else 0.12
        out = []; j = 0
        while j < m and len(out) < n:
            r = rng.random()
            if r < d * 0.6: out.append((int(a[j]) + 1 + int(rng.integers(0, 3))) & 3); j += 1
            elif r < d * 0.8: out.extend(rng.integers(0, 4, int(rng.integers(1, 12))).tolist())
            elif r < d: j += int(rng.integers(1, 12))
            else: out.append(int(a[j])); j += 1
        out = out[:n]
        while len(out) < n: out.append(int(a[len(out)]) if kind == "identical" and len(out) < m else int(rng.integers(0, 4)))
        b = np.array(out, dtype=np.uint8)
    A = np.frombuffer(b"ACGT", dtype=np.uint8)[a].copy(); B = np.frombuffer(b"ACGT", dtype=np.uint8)[b].copy()
    if with_n:
        A[rng.integers(0, m, max(1, m // 20))] = ord("N")
        B[rng.integers(0, n, max(1, n // 20))] = ord("N")
    return A.tobytes(), B.tobytes()


def _steps_lagged(m, n):
    P = (n + 63) // 64
    return sum(64 + m + min(n - pp * 128 - 64, 64) - 1 if 2 * pp + 1 < P else m + min(n - pp * 128, 64) - 1 for pp in range((P + 1) // 2))


def _steps_pair(mx, nx, my, ny):
    PX, PY = (nx + 63) // 64, (ny + 63) // 64
    return sum(max(mx + min(nx - p * 64, 64) - 1 if p < PX else 0, my + min(ny - p * 64, 64) - 1 if p < PY else 0) for p in range(max(PX, PY)))


def _rule_pairs(shapes):
    """Jobs that launch_stripes' rule puts side by side in ONE size class of (m, n) jobs, restated: (stripe count, m) order, largest first, ties in list
    order; neighbours pair where the pair's wave-steps are fewer than the two lagged forms' together."""
    cl = sorted(range(len(shapes)), key=lambda i: (-((shapes[i][1] + 63) // 64), -shapes[i][0], i))
    k = paired = 0
    while k < len(cl):
        if k + 1 < len(cl) and _steps_pair(*shapes[cl[k]], *shapes[cl[k + 1]]) < _steps_lagged(*shapes[cl[k]]) + _steps_lagged(*shapes[cl[k + 1]]):
            paired += 2; k += 2
        else:
            k += 1
    return paired


def _check(al, oracle, s1, s2, want, what):
    for rep in range(2):
        ops = al.ksw2_batch(s1, s2)
        for i in range(len(s1)):
            assert capi.apply_ops(s1[i], s2[i], ops[i]) == want[i], f"{what}: rep {rep} job {i} m={len(s1[i])} n={len(s2[i])}"


# (mX, nX, mY, nY): the two partners of one launch.  Query sides 65 ... 321 give 2 ... 6 stripes: 257 and 321 put the virtual job into two workgroups
# (hand-off through HBM), unequal counts leave a half empty in the last waves of the longer job
QS = [65, 127, 128, 129, 192, 193, 256, 257, 321]
PARTNERS = []
for k, d in enumerate([0, 1, 7, 8, 9, 63, 64, 65]):
    PARTNERS.append((130, QS[k % 9], 130 + d, QS[k % 9]))                    # equal stripe counts
    PARTNERS.append((130 + d, QS[(k + 4) % 9], 130, QS[(2 * k + 1) % 9]))      # unequal ones, either partner the longer
    PARTNERS.append((130, 321, 130 + d, 257))                                # two workgroups
for msmall in range(1, 9):
    PARTNERS.append((msmall, QS[msmall % 9], 131, QS[(msmall + 3) % 9]))
    PARTNERS.append((129 + msmall, 257, msmall, 65 + msmall))
PARTNERS += [(200, 321, 200, 321), (137, 70, 139, 321), (72, 321, 260, 129)]


@pytest.fixture(scope="module")
def partner_cases(oracle_built):
    rng = np.random.default_rng(20)
    cases = []
    for k, (mx, nx, my, ny) in enumerate(PARTNERS):
        s1x, s2x = _pair(rng, mx, nx, with_n=(k % 5 == 2))
        s1y, s2y = _pair(rng, my, ny, "identical" if k == 3 else ("unrelated" if k == 4 else "related"))
        s1, s2 = [s1x, s1y], [s2x, s2y]
        cases.append((s1, s2, [oracle_built.oracle_ksw2(a, b) for a, b in zip(s1, s2)]))
    return cases


def test_constructed_partners(oracle_built, cx_index, partner_cases):
    """Two striped jobs per launch at dp_pair = 2: they run side by side whatever their shapes.  Reference sides equal and 1, 7, 8, 9, 63, 64, 65 rows
    apart, and 1 - 8 rows beside ~130; query sides with equal and unequal stripe counts, in one and in two workgroups; N bases on both sides of a
    partner, an identical and an unrelated pair.  Then all of them in one launch (neighbours in (stripe count, m) order are partners)."""
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_pair", 2)
        for k, (s1, s2, want) in enumerate(partner_cases):
            _check(a, oracle_built, s1, s2, want, f"partners {PARTNERS[k]}")
        s1 = [s for c in partner_cases for s in c[0]]; s2 = [s for c in partner_cases for s in c[1]]; want = [w for c in partner_cases for w in c[2]]
        _check(a, oracle_built, s1, s2, want, "all partners in one launch")
    finally:
        a.close()


@pytest.mark.parametrize("dp_pair", [1, 3])
def test_odd_count_and_mixed_forms(oracle_built, cx_index, dp_pair):
    """2k + 1 striped jobs at dp_pair = 1 (the default: a list this short stays unpaired) and 3 (the step-count rule alone: paired and lagged workgroups
    in one call): equal and near-equal jobs pair (four stripes of m rows: 4 (m + 63) steps against 2 x 2 (m + 127)), a
    ten-stripe job of 150 rows beside a nine-stripe job of 900 does not (9 x 963 + 213 steps against 5 x 277 + 5 x 1027), one job is left over, and
    the 4000 x 65 job belongs to the one-wave class, which never pairs."""
    rng = np.random.default_rng(21)
    shapes = [(200, 200), (200, 200), (300, 257), (301, 250), (150, 129), (151, 129), (200, 40), (230, 40), (150, 640), (900, 576), (700, 65), (4000, 65), (180, 130)]
    assert len(shapes) % 2 == 1
    s1, s2 = zip(*[_pair(rng, m, n) for m, n in shapes])
    s1, s2 = list(s1), list(s2)
    want = [oracle_built.oracle_ksw2(x, y) for x, y in zip(s1, s2)]
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_pair", dp_pair)
        _check(a, oracle_built, s1, s2, want, f"mixed forms, dp_pair {dp_pair}")
        # what the library launched in those two calls (gsa_get_dp_stats: jobs, of them side by side, lagged launches, side-by-side launches)
        jobs, paired, n_lag, n_sbs = (int(v) for v in a.dp_stats())
        in_lds = [s for s in shapes if s[0] <= 3968]      # (the one-wave class above is a launch of its own)
        expect = _rule_pairs(in_lds) if dp_pair == 3 else 0
        assert jobs == 2 * len(shapes) and paired == 2 * expect, (jobs, paired, expect)
        if dp_pair == 3:
            assert 0 < expect < len(in_lds) - 1 and n_sbs == 2 and n_lag == 4      # pairs, more than one job left over; per call: the one-wave class, the class's unpaired jobs, its pairs
        else:
            assert n_sbs == 0 and n_lag == 4
    finally:
        a.close()


def test_default_rule_in_a_long_class(oracle_built, cx_index):
    """The default path at the size where it pairs: 4 301 striped jobs with reference sides up to 768 bases make a size class of more than
    DP_PAIR_MIN_JOBS = 4096 jobs, which is put in order, paired by the step-count rule and launched as pairs, with its unpaired jobs beside them on the
    second stream; 60 jobs in the classes above (769 - 1 000 and 1 600 - 1 700 rows, 4 000 rows) are too few to pair.  Queries are the references with
    8 % substitutions, cut or padded to 65 - 192 columns (one to three stripes)."""
    rng = np.random.default_rng(22)
    shapes = [(int(rng.integers(60, 200)), int(rng.integers(65, 193))) for _ in range(4301)]
    shapes += [(int(rng.integers(769, 1001)), int(rng.integers(65, 130))) for _ in range(40)] + [(int(rng.integers(1600, 1701)), 70) for _ in range(19)] + [(4000, 65)]
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    s1, s2 = [], []
    for m, n in shapes:
        a = rng.integers(0, 4, m).astype(np.uint8)
        b = np.resize(a, n); b[m:] = rng.integers(0, 4, max(n - m, 0))
        sub = rng.random(n) < 0.08
        b[sub] = (b[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
        s1.append(acgt[a].tobytes()); s2.append(acgt[b].tobytes())
    want = [oracle_built.oracle_ksw2(x, y) for x, y in zip(s1, s2)]
    a = capi.Aligner(cx_index)      # (dp_pair stays at its default)
    try:
        _check(a, oracle_built, s1, s2, want, "default rule")
        jobs, paired, n_lag, n_sbs = (int(v) for v in a.dp_stats())
        expect = _rule_pairs(shapes[:4301])
        assert jobs == 2 * len(shapes) and paired == 2 * expect and expect >= 4200, (jobs, paired, expect)
        assert n_sbs == 2 and n_lag == 8, (n_lag, n_sbs)      # per call: the one-wave class, the two short classes, the long class's odd job beside its pairs
    finally:
        a.close()


@pytest.fixture(scope="module")
def fuzz_case(oracle_built):
    sys.path.insert(0, TOOLS)
    import dp_fuzz
    s1, s2 = dp_fuzz.make_pairs(1200, 3)
    return s1, s2, [oracle_built.oracle_ksw2(x, y) for x, y in zip(s1, s2)]


@pytest.mark.parametrize("dp_pair", [0, 1, 2, 3])
def test_same_answers_either_way(oracle_built, cx_index, fuzz_case, dp_pair):
    """1200 random pairs around the striped kernel's edges, never paired, the default, always paired and paired where the step count says so (3: the default's rule without its
    list-length condition): each run equals the oracle, so
    they equal each other."""
    s1, s2, want = fuzz_case
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_pair", dp_pair)
        _check(a, oracle_built, s1, s2, want, f"dp_pair {dp_pair}")
    finally:
        a.close()


def test_retry_path_never_pairs(oracle_built, cx_index, partner_cases):
    """dp_safe = 1 (the retry after a hand-off time-out: one striped job per launch) with dp_pair = 2: nothing pairs, same ops."""
    s1 = [s for c in partner_cases[:6] for s in c[0]]; s2 = [s for c in partner_cases[:6] for s in c[1]]; want = [w for c in partner_cases[:6] for w in c[2]]
    a = capi.Aligner(cx_index)
    try:
        a.set_option("dp_pair", 2)
        ref = a.ksw2_batch(s1, s2)
        a.set_option("dp_safe", 1)
        _check(a, oracle_built, s1, s2, want, "dp_safe")
        got = a.ksw2_batch(s1, s2)
        assert got == ref
    finally:
        a.close()
