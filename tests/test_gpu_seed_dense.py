"""The dense seed search at its edges (csrc/k_seed_dense.hip): k_dense_sweep in both launch shapes, k_dense_search with and without a chunk list, and
k_dense_resolve behind each, on the constructed chunks of tests/dense_cases.py -- one construction per boundary the kernels name (sweep segments, M_BACK
at the text's start / the seam / a word edge, MaxSeedFreq crossed in one M_BFM step, the 64-base windows of M_TEXT, the switches of the search ladder,
the 40-position blocks of the resolver, a chunk list whose slot is not its chunk, a chunk at the candidate cap).  tests/test_dense_cases_host.py holds
the constructions themselves to a brute force on the CPU.

    id             options                        params          kernel under test
    sweep160       seed_mode 0, sweep_shape 0     defaults        k_dense_sweep<., 4, 128>
    sweep40        seed_mode 0, sweep_shape 1     defaults        k_dense_sweep<., 1, 256>
    sweep160_sen   seed_mode 0, sweep_shape 0     sen=1, clr=50   the sweep under -sen
    sweep40_sen    seed_mode 0, sweep_shape 1     sen=1, clr=50
    search_sen     (default seed_mode)            sen=1, clr=50   k_dense_search<., 512>
    handover       (default) / seed_mode 2        defaults        k_dense_search<., 256> with a chunk list

Every context in the narrow and the wide index layout (both E16 instances).  All cases of a setting run one after another on ONE context, so the
per-slot records and the candidate buffers of one case meet the next; cand_cap_sen (a chunk identical to the reference) is in the middle of the list.
Per case: the accepted seeds (qPos, len, rPos of every located hit, so the frequencies as well) and the seed groups of stage 1 and the finished blocks
of gsa_align_contig with their strings, against the oracle -- exact; every chunk went through the dense kernels (handover: exactly one, the others
through the speculative kernel).  One index per module; the oracle's side is computed once per setting.

Not here: the sweep WITH a chunk list needs 1024 handed-over chunks, a contig of 10 Mb -- that stays with the large pairs of test_gpu_parity.py."""
import ctypes as C

import numpy as np
import pytest

import dense_cases as dc
from gsalign_amd import capi, hostlib, indexio, synth

pytestmark = pytest.mark.gpu

SETTINGS = {"default": (dc.DEFAULT_SLEN, False, {}), "sen": (dc.SEN_SLEN, True, dict(sen=1, clr=50))}
# id -> (options, setting, only these cases (None: all of the setting), every chunk dense)
CONTEXTS = {
    "sweep160": (dict(seed_mode=0, sweep_shape=0), "default", None, True),
    "sweep40": (dict(seed_mode=0, sweep_shape=1), "default", None, True),
    "sweep160_sen": (dict(seed_mode=0, sweep_shape=0), "sen", None, True),
    "sweep40_sen": (dict(seed_mode=0, sweep_shape=1), "sen", None, True),
    "search_sen": ({}, "sen", None, True),
    "handover": ({}, "default", ["handover_last_chunk"], False),
    "handover_search": (dict(seed_mode=2), "default", ["handover_last_chunk"], False),
}
S1 = ("qpos", "len", "rpos", "gbeg", "gend")


def build_world(oracle_py, d):
    """(index, (setting, case) -> (query, the oracle's stage-1 seeds + groups, its finished blocks)); d: a scratch directory for the index"""
    ref, _ = dc.build_cases()
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    o = oracle_py.Oracle(idx)
    want = {}
    for setting, (slen, sen, params) in SETTINGS.items():
        ref2, cases = dc.build_cases(slen, sen)
        assert np.array_equal(ref, ref2), setting
        o.set_params(**params)
        for name, (q, on, off, _) in cases.items():
            o.set_query(q); o.run_to(1)
            s1 = o.seeds() + o.groups()
            starts = set(np.unique(s1[0]).tolist())
            assert all(s in starts for s in on) and not any(s in starts for s in off), (setting, name, sorted(starts & set(on + off)))
            o.run_to(8)
            want[setting, name] = (q, s1, o.blocks(with_aln=True))
    o.close()
    return idx, want


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    return build_world(oracle_built, tmp_path_factory.mktemp("seed_dense"))


def _kmer_k(a, wide):
    """kmer_k of a context, from the size of its jump table"""
    n = C.c_uint64(0)
    a.lib.gsa_export_index_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    a._ck(a.lib.gsa_export_index_table(a.ctx, a.TABLES["kmer"], None, 0, C.byref(n)))
    entries = int(n.value) // (32 if wide else 16)
    assert entries > 0 and entries & (entries - 1) == 0, entries
    return (entries.bit_length() - 1) // 2


def check_case(g, want, setting, name, dense_all):
    q, s1, blocks = want[setting, name]
    n_chunks = (q.size + dc.CHUNK - 1) // dc.CHUNK
    g.set_query(q); g.run_to(1)
    got = g.seeds() + g.groups()
    st = g.seed_stats()
    if dense_all is None:                                # (test_gpu_seed_grid.py: the caller holds the returned figures to its own rule)
        pass
    elif dense_all:
        assert int(st[1]) == n_chunks, (name, "dense chunks", int(st[1]), n_chunks)
    else:
        assert int(st[1]) == 1, (name, "chunks handed over", int(st[1]))
        assert int(st[0]) >= 1, (name, "passes of the speculative kernel", int(st[0]))
    for k, (a, b) in enumerate(zip(got, s1)):
        assert a.shape == b.shape, (name, S1[k], "count", a.shape, b.shape)
        assert np.array_equal(a, b), (name, S1[k], "first difference at", int(np.flatnonzero(a != b)[0]))
    assert s1[0].size > 0, (name, "no seeds")
    g.align_contig(q); full = g.blocks_as_dump(with_aln=True)
    for k, v in blocks.items():
        assert full[k].shape == v.shape and np.array_equal(full[k], v), (name, "block field", k)
    return st


@pytest.mark.parametrize("layout", ["narrow", "wide"])
@pytest.mark.parametrize("ctx", list(CONTEXTS))
def test_dense_cases(world, ctx, layout):
    idx, want = world
    options, setting, only, dense_all = CONTEXTS[ctx]
    slen, sen, params = SETTINGS[setting]
    names = only or list(dc.build_cases(slen, sen)[1])
    g = capi.Aligner(idx, wide=(layout == "wide"), **params)
    try:
        for k, v in options.items():
            g.set_option(k, v)
        assert _kmer_k(g, layout == "wide") == dc.kmer_k_for(2 * idx.G), (ctx, "kmer_k the constructions assume")
        for name in names:
            check_case(g, want, setting, name, dense_all)
        if only:                                         # the handed-over chunk once more: its slot's records and the list are the previous run's
            check_case(g, want, setting, only[0], dense_all)
    finally:
        g.close()
