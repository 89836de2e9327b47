"""What "the same result" means wherever two runs of the library are compared (bundle against alone, retry against the plain run)."""
import numpy as np

from gsalign_amd import capi


def same_result(a, b, what):
    """blocks and records byte for byte (offsets included), the strings the records address, and the whole pools: they give a DP gap
    the room it can need at most -- m + n -- and the bytes no record owns are zero since late round 3 (they used to be whatever the
    buffer held: tools/stress_consistency.py saw bundles differ from call to call in exactly those bytes)"""
    for k in ("blocks", "frags"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k)
    assert a["aln1"].size == b["aln1"].size and a["aln2"].size == b["aln2"].size, (what, "pool size")
    assert np.array_equal(a["aln1"], b["aln1"]) and np.array_equal(a["aln2"], b["aln2"]), (what, "pool bytes outside the records' strings")
    da, db = capi.result_as_dump(a, with_aln=True), capi.result_as_dump(b, with_aln=True)
    for k in ("aln1", "aln2"):
        assert np.array_equal(da[k], db[k]), (what, k)
