"""gsa_lift and gsa_lift_regions read ONE span table (csrc/gsa_walk.h: SpanBlk, span_build) and keep it in ONE pair of buffers; gsa_ref_track and gsa_project build
theirs with the same builder.  Each call rebuilds its table and has consumed it when it returns, so the passes may follow each other in any order on one context:
every answer must equal the host walk's (hostlib), a repeated call must repeat its answer, and a region of one base must be the lift of that base."""
import os

import numpy as np
import pytest

from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_variants import large_gap_pair

pytestmark = pytest.mark.gpu

W = 1000
EQ, X, DEL = 7, 8, 2      # GSA_CIGAR_EQ / _X / _DEL


@pytest.fixture(scope="module")
def cases(golden_dir, tmp_path_factory):
    """name -> (index prefix, index, contigs): the golden cx pair (blocks on both strands) and one block whose gaps are all above 64 columns (the wave path)"""
    px = os.path.join(golden_dir, "cx")
    d = tmp_path_factory.mktemp("span")
    ref, qry = large_gap_pair()
    fa = str(d / "r.fa"); lg = str(d / "r")
    synth.write_fasta(fa, [("r1", ref)])
    hostlib.build_index(fa, lg)
    return {"cx": (px, indexio.load_index(px), [np.ascontiguousarray(q) for _, q in synth.read_fasta(px + ".qry.fa")]),
            "large_gap": (lg, indexio.load_index(lg), [qry])}


def same(a, b, dt):
    assert a.dtype == dt and b.dtype == dt and a.size == b.size, (a.size, b.size)
    for f in dt.names:
        assert np.array_equal(a[f], b[f]), (f, np.flatnonzero(a[f] != b[f])[:5])


@pytest.mark.parametrize("name", ["cx", "large_gap"])
def test_lift_and_regions_share_their_table(cases, name):
    px, idx, contigs = cases[name]
    G = int(idx.G)
    seq_end = np.cumsum(idx.chr_len).astype(np.int64)
    pos = np.arange(0, G, 1 if name == "large_gap" else 3, dtype=np.int64)
    al = capi.Aligner(idx)
    al.lift_set(pos); al.track_set(W); al.proj_open()
    want_words = np.zeros(G, np.uint32)
    strands, wide, n_blocks = set(), 0, 0
    for seq in contigs:
        r = al.align_contig(seq)
        d = capi.result_as_dump(r, True)
        n_blocks = max(n_blocks, int(d["b_score"].size))
        wide += int(((d["f_bseed"] == 0) & (d["f_alnlen"] > 64) & (d["f_rlen"] > 0) & (d["f_qlen"] > 0)).sum())
        want_lift = hostlib.lift(px, seq, r, pos)
        if want_lift.size == 0:      # (a contig without blocks: there is no lifted position to put a region at)
            assert d["b_score"].size == 0 and al.lift().size == 0
            continue
        # every region of one base at a lifted position, then regions of several lengths that start there
        p = pos[want_lift["idx"]]
        beg = np.concatenate([p, p[::7]]); end = np.concatenate([p + 1, p[::7] + 150])
        end = np.minimum(end, seq_end[np.searchsorted(seq_end, beg, side="right")])      # (a region stays inside its sequence)
        al.regions_set(beg, end)
        l1 = al.lift(); g1 = al.lift_regions(); l2 = al.lift()
        tk = al.track(); pj = al.project()
        g2 = al.lift_regions()
        same(l1, want_lift, capi.LIFT_HIT_DT)
        same(g1, hostlib.lift_regions(px, seq, r, beg, end), capi.REGION_HIT_DT)
        same(tk, hostlib.track(px, seq, r, W), capi.TRACK_WIN_DT)
        assert pj == hostlib.project(px, seq, r, want_words) and np.array_equal(al.proj_fetch(words=True)[1], want_words)
        assert l1.tobytes() == l2.tobytes() and g1.tobytes() == g2.tobytes()
        # a region of one base is the lift of that base
        one = g1[:p.size]
        assert p.size > 0 and np.array_equal(one["idx"], np.arange(p.size))
        for f in ("block", "rev", "n_cover"):
            assert np.array_equal(one[f], l1[f]), f
        gone = (l1["cls"] == DEL).astype(np.int32)
        assert np.array_equal(one["q_lo"], l1["qpos"] + gone) and np.array_equal(one["q_hi"], l1["qpos"] + 1)
        assert np.array_equal(one["n_eq"], l1["cls"] == EQ) and np.array_equal(one["n_x"], l1["cls"] == X) and np.array_equal(one["n_del"], gone) and not one["n_ins"].any()
        strands |= set(np.unique(l1["rev"]).tolist())
    al.proj_close()
    al.close()
    if name == "cx":
        assert strands == {0, 1}
    else:
        assert n_blocks == 1 and wide >= 10
