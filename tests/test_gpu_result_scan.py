"""The result passes (gsa_call_variants, gsa_block_cigars, gsa_block_cs) at a size at which their second-level scans -- one workgroup over tiles of
256 workgroup sums, with a carry from tile to tile -- run more than one tile.  The goldens' contigs have a few thousand records, far below the 65 536
work items of one tile; here ONE block holds about 150 000 records, 150 000 ops and 75 000 variants, on either strand."""
import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_cigars import aligned_cigars
from test_gpu_cs import aligned_cs
from test_gpu_variants import aligned_variants

pytestmark = pytest.mark.gpu

TILE = 256 * 256      # work items of one tile of a second-level scan: 256 workgroups of 256


def dense_snv_pair(seed=17, n=1_500_000, step=20):
    """A random reference of n bases and a query that differs from it by one substitution at every position step, 2 step, ... < n - step: seeds of
    step - 1 bases with one-base gaps between them, all in one block"""
    ref = synth.random_genome(n, np.random.default_rng(seed))
    nxt = np.zeros(256, np.uint8)
    for a, b in zip(b"ACGT", b"CGTA"):
        nxt[a] = b
    qry = ref.copy()
    at = np.arange(step, n - step, step)
    qry[at] = nxt[ref[at]]
    return ref, qry


@pytest.fixture(scope="module")
def dense_snv_case(tmp_path_factory):
    d = tmp_path_factory.mktemp("rscan")
    ref, qry = dense_snv_pair()
    fa = str(d / "r.fa"); px = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, px)
    return px, indexio.load_index(px), qry


@pytest.mark.parametrize("strand", ["+", "-"])
def test_result_passes_beyond_one_scan_tile(dense_snv_case, strand):
    """parity with the host walks where the workgroups' sums of all three passes fill more than two tiles (three tiles, two carries); "-": a
    reverse-strand block, so the mirrored store of the ops and the mirrored slot of the cs pass run at this size too"""
    px, idx, qry = dense_snv_case
    q = qry if strand == "+" else np.ascontiguousarray(synth.revcomp(qry))
    al = capi.Aligner(idx)
    (V, cnt), r = aligned_variants(al, px, q)
    (cblk, ops), _ = aligned_cigars(al, q)
    (sblk, by), _, _ = aligned_cs(al, q)
    al.close()
    B = r["blocks"]
    # the coverage this test stands on
    assert ((B["bdir"] != 0) == (strand == "+")).all(), B["bdir"]
    assert int(B["n_frag"][B["bdup"] == 0].sum()) > 2 * TILE and int(B["n_frag"].sum()) > 2 * TILE      # work items of the variant pass / of the CIGAR pass
    assert ops.size > 2 * TILE                                                                          # work items of the cs pass
    assert V.size > TILE and cnt[0] > TILE, (V.size, cnt)
    assert int(cblk["n_cig"].sum()) == ops.size and int(sblk["n_cs"].sum()) == by.size
