"""The side-by-side form of the striped gap DP hands a job's (x, v) of a stripe's last column to the next wave as two nibbles (k_dp_stripe.hip,
dp_pack4), which needs 0 <= x, v <= 15 in every cell INSIDE a matrix.  The proof is the algebra in the kernel's comment: inside a matrix z <= 7 without
the cap (scores differ by at most one match between neighbours), u >= 0 and a <= z, so v = z - u <= 7 and x = a - (z - 2) <= 2.  This file does not
replace that argument; it guards it: a Python restatement of gsa_dp.h's dp_cell with the kernel's boundary values -- not the kernel itself -- over pairs
chosen to push the differences to their ends (identical, unrelated, all-N, one-base repeats against each other, long gaps on either side) asserts the
bounds the argument claims, x <= 2 and v <= 7, so that a drift in either shows.  The kernel's own hand-off is checked on the GPU (test_gpu_dp_pairs.py)."""
import numpy as np


def _xv_range(s1, s2):
    """(max x, max v, min x, min v) over the cells of the m x n matrix; s1 = reference side (rows), s2 = query side (columns), codes 0-4."""
    m, n = len(s1), len(s2)
    u = [0 if t == 0 else 2 for t in range(n)]      # u, y of the row above, per column
    y = [0] * n
    hi_x = hi_v = 0; lo_x = lo_v = 0
    for j in range(m):
        x1, v1 = 0, (0 if j == 0 else 2)            # the column in front of the matrix
        for t in range(n):
            a_, b_ = s2[t], s1[j]
            z = (0 if (a_ == 4 or b_ == 4) else (1 if a_ == b_ else -1)) + 6
            a = x1 + v1; b = y[t] + u[t]
            z = max(z, a, b)
            assert z <= 7, "the kernel's cap at 7 binds inside a matrix"
            un, vn = z - v1, z - u[t]
            xn, yn = max(a - (z - 2), 0), max(b - (z - 2), 0)
            u[t], y[t] = un, yn
            x1, v1 = xn, vn
            hi_x = max(hi_x, xn); hi_v = max(hi_v, vn); lo_x = min(lo_x, xn); lo_v = min(lo_v, vn)
    return hi_x, hi_v, lo_x, lo_v


def test_boundary_values_stay_within_the_claimed_bounds():
    rng = np.random.default_rng(7)
    r = rng.integers(0, 4, 150).tolist()
    cases = [(r, r), (r, rng.integers(0, 4, 140).tolist()), ([4] * 90, [4] * 70), ([0] * 120, [1] * 100), ([0] * 100, [0] * 9), ([0] * 3, [0] * 130),
             (r, r[:40] + r[110:]), (r[:30] + r[120:], r), ([0] * 70 + r[:60], [1] * 5 + r[:60]), (r[:1], r), (r, r[:1])]
    for s1, s2 in cases:
        hx, hv, lx, lv = _xv_range(s1, s2)
        assert 0 <= lx and 0 <= lv and hx <= 2 and hv <= 7, (len(s1), len(s2), hx, hv, lx, lv)
