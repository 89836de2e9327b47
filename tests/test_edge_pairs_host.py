"""The constructed threshold cases of tests/edge_pairs.py on the CPU: (1) every case hits the edge it is built for, read off the restatement's own
stage output; (2) the restatement equals the real reference at all eight stages on every case (skipped where oracle/_ref is absent); (3) the
restatement reproduces the real reference's gap-similarity verdicts on the leaf windows (tests/golden/gapsim_edges.npz).  No GPU."""
import os

import numpy as np
import pytest

import edge_pairs as ep
from conftest import GOLDEN, assert_stage_equal
from gsalign_amd import hostlib, indexio, synth

REFS, CASES = ep.build_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def edge_index(tmp_path_factory):
    d = tmp_path_factory.mktemp("edge")
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, REFS); hostlib.build_index(rf, px)
    return indexio.load_index(px)


@pytest.fixture(scope="module")
def ora(oracle_built, edge_index):
    o = oracle_built.Oracle(edge_index)
    yield o
    o.close()


def test_text_is_what_the_generator_assumes(edge_index):
    w = ep.world()
    assert edge_index.G == w.G and np.array_equal(np.frombuffer(bytes(edge_index.ref), np.uint8) if not isinstance(edge_index.ref, np.ndarray) else edge_index.ref, w.text)


def _blocks_of(d, st):
    """[(qpos, qlen, rpos, rlen) arrays] per block of stage st."""
    out, off = [], 0
    for n in d[f"s{st}_b_nfrag"]:
        out.append(tuple(d[f"s{st}_f_{k}"][off:off + n] for k in ("qpos", "qlen", "rpos", "rlen"))); off += n
    return out


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_case_hits_its_edge(ora, name):
    c = BY_NAME[name]; x = c.expect
    ora.set_params(**c.params); ora.set_query(c.query)
    d = ora.dump_stages(4)
    q, l, r = d["s1_qpos"], d["s1_qlen"], d["s1_rpos"]
    assert q.size > 0
    # every seed is the one the construction places (and nothing else was found)
    pq, pl, pr = ep.predicted_seeds(x["src"], 15)
    if "extra_hits" in x:
        e = np.asarray(x["extra_hits"], np.int64)
        pq = np.concatenate([pq, e[:, 0]]).astype(np.int32); pl = np.concatenate([pl, e[:, 1]]).astype(np.int32); pr = np.concatenate([pr, e[:, 2]])
        o = np.lexsort((pq, pr - pq)); pq, pl, pr = pq[o], pl[o], pr[o]
    assert np.array_equal(q, pq) and np.array_equal(l, pl) and np.array_equal(r, pr), "seeds differ from the construction"
    pd = r - q
    ind = c.params.get("ind", 25)
    sizes = (d["s1_gend"] - d["s1_gbeg"]).tolist()
    assert sizes == ep.groups_of(pd, ind)
    assert len(sizes) == x["n_groups"]
    if "pd_jumps" in x:
        assert ep.pd_jumps(q, r) == x["pd_jumps"]
    if "group_seeds" in x:
        assert sizes == x["group_seeds"]
    if "bm_mod" in x:
        M = x["bm_mod"]
        assert ep.bitmap_index(int(pd.min()), c.query.size) % M == x["bm_lower"] and ep.bitmap_index(int(pd.max()), c.query.size) % M == x["bm_upper"]
        assert x["bm_lower"] == M - 1 or x["bm_upper"] == 0
    if "min_seeds" in x:
        assert q.size >= x["min_seeds"] and set(sizes) >= {29, 30, 31}
    if "window_count" in x or "window_span" in x:
        # replay of the window rule on the restatement's seeds (all unique here): count at the first seed of the PosDiff step that closes / does not close the window
        o = np.argsort(q, kind="stable"); qq, pp = q[o], pd[o]
        n, i, closes = 1, 0, []
        for j in range(1, qq.size):
            if pp[j] == pp[j - 1]:
                n += 1
            else:
                n += 1
                closes.append((n, int(qq[j] - qq[i])))
                if n >= 30 and qq[j] - qq[i] > 3000:
                    i, n = j, 0
        if "window_span" in x:
            assert closes[0] == (31, x["window_span"])
        elif name.startswith("C_second"):
            assert closes[0][0] == 30 and closes[0][1] > 3000 and closes[3][0] == x["window_count"] and closes[3][1] > 3000
        else:
            assert closes[0][0] == x["window_count"] and closes[0][1] > 3000
    if "s2_seeds" in x:
        assert d["s2_f_qpos"].size == x["s2_seeds"]
    if "multi_qpos" in x:
        assert int((q == x["multi_qpos"]).sum()) == 2 and int((d["s2_f_qpos"] == x["multi_qpos"]).sum()) == x["multi_kept"]
        o = np.argsort(q, kind="stable"); qq, pp = q[o], pd[o]; at = int(np.flatnonzero(qq == x["multi_qpos"])[0])
        alive = np.isin(qq, d["s2_f_qpos"]) | (qq == x["multi_qpos"])
        near = np.concatenate([np.flatnonzero(alive[:at])[-5:], (at + 2 + np.flatnonzero(alive[at + 2:]))[:5]])
        assert int(pp[at]) - int(pp[near].sum()) // 10 == x["neighbour_mean_off"] == ind + 1
    if "seed_sum" in x:
        assert int(l.sum()) == x["seed_sum"] and d["s2_b_score"].size == x["s2_blocks"]
        if x["s2_blocks"]:
            assert d["s2_b_score"].tolist() == [x["seed_sum"]]
    if "region" in x:
        assert int(q.max() + l[np.argmax(q)] - q.min()) == x["region"] and d["s2_b_score"].size == x["s2_blocks"]
    if "gap" in x:
        assert d["s2_b_score"].size == x["s2_blocks"]
        blocks = _blocks_of(d, 3) if x["s2_blocks"] == 1 else [tuple(a[np.argsort(q, kind="stable")] for a in (q, l, r, l))]      # (a gap over 5000 never reaches stage 3 as one block)
        gaps = [(int(bq[i + 1] - bq[i] - bl[i]), int(br[i + 1] - br[i] - brl[i])) for bq, bl, br, brl in blocks for i in range(bq.size - 1)]
        assert tuple(x["gap"]) in gaps and max(g[0] for g in gaps) == x["gap"][0]
        if "agree" in x:
            bq, bl, br, brl = _blocks_of(d, 3)[0]
            i = [g[0] for g in gaps].index(x["gap"][0])
            assert ep.count_agree(c.query, ep.world().text, int(bq[i] + bl[i]), int(bq[i + 1]), int(br[i] + brl[i])) == x["agree"]
    if "ref_overlap" in x:
        bq, bl, br, brl = _blocks_of(d, 2)[0]
        ov = (br[:-1] + brl[:-1] - br[1:]).max()
        assert int(ov) == x["ref_overlap"]


def test_bundle_contigs_sit_at_both_ends_of_the_text(ora):
    w = ep.world()
    (_, q0, s0), (_, q1, s1), _ = ep.bundle_contigs(w)
    ora.set_params()
    ora.set_query(q0); d = ora.dump_stages(1)
    assert int((d["s1_rpos"] + d["s1_qlen"]).max()) == 2 * w.G and np.array_equal(d["s1_qpos"], ep.predicted_seeds(s0)[0])
    ora.set_query(q1); d = ora.dump_stages(1)
    assert int(d["s1_rpos"].min()) == 0 and int(d["s1_qpos"].min()) == 6000 and np.array_equal(d["s1_qpos"], ep.predicted_seeds(s1)[0])


def _param_sets():
    sets = []
    for c in CASES:
        if c.params not in sets:
            sets.append(c.params)
    return sets


@pytest.mark.parametrize("params", _param_sets(), ids=lambda p: "-".join(f"{k}{v}" for k, v in p.items()) or "defaults")
def test_restatement_equals_the_real_reference(oracle_built, tmp_path, params):
    op = oracle_built
    if not op.have_ref():
        pytest.skip("oracle/_ref not built")
    mine = [c for c in CASES if c.params == params]
    if params == {}:
        mine = mine + [Case_(n, q) for n, q, _ in ep.bundle_contigs(ep.world())]
    rf, qf, px = str(tmp_path / "r.fa"), str(tmp_path / "q.fa"), str(tmp_path / "r")
    synth.write_fasta(rf, REFS); op.ref_build_index(rf, px)
    synth.write_fasta(qf, [(c.name, c.query) for c in mine])
    op.ref_dump_subprocess(px, qf, str(tmp_path / "ref.npz"), params)
    want = np.load(str(tmp_path / "ref.npz"))
    o = op.Oracle(indexio.load_index(px), params)
    for ci, c in enumerate(mine):
        o.set_query(c.query)
        assert_stage_equal(o.dump_stages(8), want, prefix=f"c{ci}_")
    o.close()


class Case_:
    def __init__(self, name, query):
        self.name, self.query = name, query


def test_gap_similarity_edge_windows_known_answers(ora):
    q, rows, notes = ep.leaf_query()
    gold = np.load(os.path.join(GOLDEN, "gapsim_edges.npz"))["rows"]
    assert np.array_equal(gold[:, [6, 1, 2, 3, 4]], rows), "tests/golden/gapsim_edges.npz is not of this generator: rerun tests/golden/make_golden.py --gapsim-edges"
    ora.set_query(q)
    for (ci, q1, q2, r1, r2, want, cid) in gold:
        assert ora.gap_similarity(int(q1), int(q2), int(r1), int(r2)) == want, notes[int(cid)]
    # both verdicts occur on each side of the lines the windows are built around
    v = {notes[int(r[6])]: int(r[5]) for r in gold}
    for L in (5002, 5003):
        h = (L + 1) // 2
        assert (v[f"agree_len{L}_{h - 1}"], v[f"agree_len{L}_{h}"], v[f"agree_len{L}_{h + 1}"]) == (0, 1, 1)
    assert (v["kmer_at_limit"], v["kmer_limit_plus_1"]) == (0, 1)
    assert v["unrelated_5001x5000"] == 0 and v["unrelated_5000x4999"] == 1
