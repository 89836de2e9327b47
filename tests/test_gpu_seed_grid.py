"""The seed search over the (kmer_k, MinSeedLength) grid.  Which rungs of the ladder exist -- the presence table and what it is built
from, the short k-mer table, the jump table's reach -- depends on how MinSeedLength compares with kmer_k (csrc/k_tables.hip: build_kmer_lo,
build_presence, build_kmer_table), and the mode a start is searched in depends on both (k_seed.hip, k_seed_dense.hip).  tests/test_gpu_seed_dense.py
holds (12, 15) and (12, -sen); here every row of dense_cases.GRID runs the constructed chunks of tests/dense_cases.py, built for that row:

    kmer_k 12 (this text's own)   -slen 10 11 12 13 14 16 17 30, -sen
    kmer_k 15 (a human index's)   -slen 10 13 14 15 16 30, -sen
    kmer_k  8 (a crowded card's)  -slen 10 15 30, -sen

    id             options                        rows            kernel under test
    spec           (default seed_mode)            -slen rows      k_seed_wg; a chunk it hands over goes to k_dense_search (kmer_k 8: SPEC_BUDGET)
    sweep160       seed_mode 0, sweep_shape 0     -slen rows      k_dense_sweep<., 4, 128>
    sweep40        seed_mode 0, sweep_shape 1     -slen, k = 15   k_dense_sweep<., 1, 256>
    search_sen     (default seed_mode)            -sen            k_dense_search<., 512>
    sweep160_sen   seed_mode 0, sweep_shape 0     -sen            the sweep under -sen

One owner of the index per (kmer_k, layout), made once for the module (kmer_k 15: a jump table of 16 GiB narrow, 32 GiB wide); every test function is
one (kmer_k, context, layout): a gsa_clone of the owner with the context's options, which borrows the jump table and goes through its rows with
gsa_set_params -- that rebuilds the presence table and the short k-mer table and nothing else.  Per case, exact against the oracle (check_case of
test_gpu_seed_dense.py): the stage-1 seeds with every located hit, the groups, the finished blocks with their strings.  Under `spec` the families
that test a switch of the speculative kernel itself must not be handed over to the dense kernels (seed_stats()[1] == 0): handed over, they would test
k_dense_search a second time and k_seed_wg not at all.  The other families' figure is printed.  The (15, 15) row runs a second time with the presence
table built from a scan of the text instead of from the jump table.  A last test alternates an owner at (15, 15) with a clone of it at -slen 10.

The oracle does not know about kmer_k: its side is computed once per (MinSeedLength, -sen, query) and shared between the rows."""
import ctypes as C
import time

import numpy as np
import pytest

import dense_cases as dc
from gsalign_amd import capi, hostlib, indexio, synth
from test_gpu_seed_dense import _kmer_k, check_case

pytestmark = pytest.mark.gpu

# id -> (options, the -sen rows (else the -slen rows), kmer_k values, every chunk dense (None: the rule of QUIET))
CONTEXTS = {
    "spec": ({}, False, (12, 15, 8), None),
    "sweep160": (dict(seed_mode=0, sweep_shape=0), False, (12, 15, 8), True),
    "sweep40": (dict(seed_mode=0, sweep_shape=1), False, (15,), True),
    "search_sen": ({}, True, (12, 15, 8), True),
    "sweep160_sen": (dict(seed_mode=0, sweep_shape=0), True, (12, 15, 8), True),
}
RUNS = [(K, ctx) for ctx, (_, _, ks, _) in CONTEXTS.items() for K in ks]
# under `spec` no chunk of these may be handed over
QUIET = ("len_", "n_at_", "start_at_", "text_", "pres_look_", "n_word_")
SEN = dict(sen=1, clr=50)
# kmer_k -> seed_budget of its `spec` context.  An 8-mer of this text has six occurrences: behind the table entry a search takes two or three Occ steps
# more before its row is unique, a chunk of a hundred searches crosses the default budget of 256 wave-iterations (measured: text_63, text_64 and three
# of freq_* go to the dense kernels, equal to the oracle there), and the quiet families would test k_dense_search.  Four times the default keeps them
# in k_seed_wg; kmer_k 12 and 15 run at the default.
SPEC_BUDGET = {8: 1024}


def build_world(oracle_py, d):
    """(index, (row, case) -> (query, the oracle's stage-1 seeds + groups, its finished blocks)), row = (kmer_k, MinSeedLength, -sen)"""
    ref, _ = dc.build_cases()
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    o = oracle_py.Oracle(idx)
    want, memo = {}, {}
    for slen, sen in sorted({(slen, sen) for rows in dc.GRID.values() for slen, sen in rows}):
        o.set_params(**(SEN if sen else dict(slen=slen)))
        for K, rows in dc.GRID.items():
            if (slen, sen) not in rows:
                continue
            ref2, cases = dc.build_cases(slen, sen, kmer_k=K)
            assert np.array_equal(ref, ref2), (K, slen, sen)
            for name, (q, on, off, _) in cases.items():
                key = (slen, sen, q.tobytes())
                if key not in memo:
                    o.set_query(q); o.run_to(1)
                    s1 = o.seeds() + o.groups()
                    o.run_to(8)
                    memo[key] = (q, s1, o.blocks(with_aln=True))
                s1 = memo[key][1]
                starts = set(np.unique(s1[0]).tolist())
                assert all(s in starts for s in on) and not any(s in starts for s in off), (K, slen, sen, name, sorted(starts & set(on + off)))
                want[(K, slen, sen), name] = memo[key]
    o.close()
    return idx, want


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    return build_world(oracle_built, tmp_path_factory.mktemp("seed_grid"))


@pytest.fixture(scope="module")
def owners(world):
    """(kmer_k, layout) -> the context that owns that index, made at its first use and kept; default parameters, default options, never changed"""
    idx, _ = world
    made = {}

    def get(K, layout):
        if (K, layout) not in made:
            t0 = time.perf_counter()
            g = capi.Aligner(idx, wide=(layout == "wide"), kmer_k=K)
            made[K, layout] = g
            print(f"seed grid: owner kmer_k {K} {layout}: created in {time.perf_counter() - t0:.2f} s")
            assert _kmer_k(g, layout == "wide") == K, (K, layout, "the forced kmer_k was not taken: is a quarter of the device memory free?")
        return made[K, layout]

    yield get
    for g in made.values():
        g.close()


def table_bytes(g, which):
    """the defined size of one device table of a context (gsa_export_index_table without a buffer: nothing is copied); 0: the table is absent"""
    n = C.c_uint64(0)
    g.lib.gsa_export_index_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    g._ck(g.lib.gsa_export_index_table(g.ctx, g.TABLES[which], None, 0, C.byref(n)))
    return int(n.value)


def run_row(g, want, row, dense_all, label, failures, names=None):
    """all cases of a row on g, which is set to the row's parameters; -> {case: chunks handed over} of the cases that are not QUIET"""
    K, slen, sen = row
    handed = {}
    for name in names or list(dc.build_cases(slen, sen, kmer_k=K)[1]):
        try:
            st = check_case(g, want, row, name, dense_all)
            if dense_all is None:
                if name.startswith(QUIET):
                    assert int(st[1]) == 0, (name, "chunks handed over to the dense kernels", int(st[1]))
                    assert int(st[0]) >= 1, (name, "passes of the speculative kernel", int(st[0]))
                elif int(st[1]):
                    handed[name] = int(st[1])
        except AssertionError as e:
            failures.append((label, row, name) + tuple(e.args))
    return handed


def set_row(g, row, layout, failures):
    """g at the row's parameters; the tables gsa_set_params has to leave behind, by their sizes"""
    K, slen, sen = row
    g.set_params(**(SEN if sen else dict(slen=slen)))
    lo = table_bytes(g, "kmer_lo") // (32 if layout == "wide" else 16)
    for what, got, exp in (("kmer_k", _kmer_k(g, layout == "wide"), K), ("entries of the short k-mer table", lo, (1 << (2 * slen)) if 8 <= slen <= 13 and slen < K else 0),
                           ("bytes of the presence table", table_bytes(g, "pres"), 32 << (2 * (min(slen, 16) - 3)))):
        if got != exp:
            failures.append(("set_params", row, layout, what, got, exp))


@pytest.mark.parametrize("layout", ["narrow", "wide"])
@pytest.mark.parametrize("K,ctx", RUNS, ids=[f"k{K}-{ctx}" for K, ctx in RUNS])
def test_grid(world, owners, K, ctx, layout):
    _, want = world
    options, sen_rows, _, dense_all = CONTEXTS[ctx]
    g = owners(K, layout).clone()
    failures = []
    try:
        for k, v in options.items():
            g.set_option(k, v)
        if ctx == "spec" and K in SPEC_BUDGET:
            g.set_option("seed_budget", SPEC_BUDGET[K])
        for slen, sen in dc.GRID[K]:
            if sen != sen_rows:
                continue
            row = (K, slen, sen)
            set_row(g, row, layout, failures)
            handed = run_row(g, want, row, dense_all, ctx, failures)
            if dense_all is None:
                print(f"seed grid: {ctx} {layout} {row}: chunks handed over outside the quiet families: {handed}")
        if ctx == "spec" and K == 15:                    # (15, 15) once more, its presence table from the scan of the text
            g.set_option("pres_from_kmer", 0)
            set_row(g, (15, 14, False), layout, failures); set_row(g, (15, 15, False), layout, failures)      # (a table of the same k is kept: away and back)
            run_row(g, want, (15, 15, False), dense_all, ctx + ", pres_from_kmer 0", failures)
    finally:
        g.close()
    for f in failures:
        print("seed grid: differs:", layout, f[:6])
    assert not failures, (len(failures), failures[:20])


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_owner_and_clone_at_two_rows(world, owners, layout):
    """The owner at (15, 15) and a clone of it at -slen 10, case by case in turn: the clone borrows the jump table and reads a presence table and a
    short k-mer table of its own, the owner's stay what they were."""
    _, want = world
    rows = ((15, 15, False), (15, 10, False))
    owner = owners(15, layout)
    g = owner.clone()
    failures = []
    try:
        g.set_params(slen=10)
        assert _kmer_k(g, layout == "wide") == 15 and table_bytes(g, "kmer_lo") and not table_bytes(owner, "kmer_lo")
        assert table_bytes(owner, "pres") == 32 << 24 and table_bytes(g, "pres") == 32 << 14
        names = [[n for n in dc.build_cases(slen, sen, kmer_k=K)[1] if n.startswith("len_")] for K, slen, sen in rows]
        assert any(n.startswith("len_between_") for n in names[1]) and "len_klo" in names[1] and len(names[0]) >= 4
        for i in range(max(map(len, names))):
            for ctx, row, mine in ((owner, rows[0], names[0]), (g, rows[1], names[1])):
                if i < len(mine):
                    run_row(ctx, want, row, None, "owner" if ctx is owner else "clone", failures, [mine[i]])
    finally:
        g.close()
    for f in failures:
        print("seed grid: differs:", layout, f[:6])
    assert not failures, (len(failures), failures[:20])
