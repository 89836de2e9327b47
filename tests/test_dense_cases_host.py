"""The constructed chunks of tests/dense_cases.py on the CPU, held to a plain reference that is neither the oracle nor a kernel: for every listed
(start, expected_len, expected_freq) the longest match from `start` inside its chunk is found by bytes.find over the forward text + its reverse
complement (extended base by base while the next base is unambiguous, inside the chunk and the longer string still occurs), and its occurrences are
counted by overlapping finds, up to 102.  That has to equal the expectation, and the oracle's BWT_Search(start, chunk end) has to give the same length
and -- where the match is a seed (MinSeedLength bases, at most MaxSeedFreq occurrences) -- as many locations, else none.

The seam cases (back_seam, back_seam_fwd) are held to the oracle ONLY: whether a match may run across the end of the forward strand into the reverse
one, or end at the text's last base, is the reference's decision and not the brute force's; their listed lengths and counts are compared with
BWT_Search alone.

Then the chain: from the oracle's stage-1 seeds, every must_be start is a seed's start and no must_not_be start is.  No listed start may be skipped:
the number of starts checked is held against the number listed.  Both settings: the default MinSeedLength and -sen (the library forces 10).  No GPU.

The grid: the same two judges for every row of dense_cases.GRID -- (kmer_k, MinSeedLength) with kmer_k 8, 12 and 15 -- and, for the
pres_look_* family, bytes.find for what the presence table has to say about each start.  build_cases(15) and build_cases(10, sen=True) are held to the
digest they had before build_cases took a kmer_k."""
import numpy as np
import pytest

import dense_cases as dc
from gsalign_amd import hostlib, indexio, synth

SETTINGS = {"default": (dc.DEFAULT_SLEN, False, {}), "sen": (dc.SEN_SLEN, True, dict(sen=1, clr=50))}
SEAM = ("back_seam", "back_seam_fwd")
ACGT = set(b"ACGT")


@pytest.fixture(scope="module")
def world(oracle_built, tmp_path_factory):
    d = tmp_path_factory.mktemp("dense_host")
    ref, _ = dc.build_cases()
    rf, px = str(d / "r.fa"), str(d / "r")
    synth.write_fasta(rf, [("ref", ref)]); hostlib.build_index(rf, px)
    idx = indexio.load_index(px)
    o = oracle_built.Oracle(idx)
    yield ref, idx, o, {}
    o.close()


def _brute(text, q, s, end):
    """(length, occurrences up to 102) of the longest match of q[s:] inside [s, end)"""
    L = 0
    while s + L < end and q[s + L] in ACGT and text.find(q[s:s + L + 1]) >= 0:
        L += 1
    return L, (dc.count_in(text, q[s:s + L]) if L else 0)


def test_one_reference_for_both_settings(world):
    ref, idx, *_ = world
    ref2, _ = dc.build_cases(dc.SEN_SLEN, sen=True)
    assert np.array_equal(ref, ref2)
    assert idx.G == dc.REF_LEN and bytes(np.asarray(idx.ref).tobytes()[:2 * idx.G]) == dc.text_of(ref)


def test_families_are_all_there():
    for setting, (slen, sen, _) in SETTINGS.items():
        names = list(dc.build_cases(slen, sen)[1])
        for fam in ("seg_edge_40", "seg_edge_160", "seg_edge_40_dup", "seg_edge_160_dup_noext", "back_text_start", "back_text_start_off", "back_seam", "back_seam_fwd", "back_word_edge_31", "back_word_edge_32",
                    "back_word_edge_33", "freq_100", "freq_101", "freq_cross_up", "freq_cross_down", "text_63", "text_64", "text_65", "text_127", "text_128", "text_129", "text_chunk_end",
                    "len_min-1", "len_min", "len_k-1", "len_k", "n_at_L-1", "n_at_L", "start_at_clen-min", "start_at_clen-min+1", "resolve_hop_39", "resolve_hop_40", "resolve_hop_41",
                    "resolve_skip_blocks", "resolve_tail_9999", "resolve_tail_10001", "resolve_sen_edge", "cand_cap_sen"):
            assert fam in names, (setting, fam)
        assert ("len_klo" in names) == sen and ("handover_last_chunk" in names) == (not sen), setting
        assert names.index("cand_cap_sen") not in (0, len(names) - 1), setting          # in the middle: the cases behind it meet its buffers
        for name, (q, *_rest) in dc.build_cases(slen, sen)[1].items():
            assert q.size <= 3 * dc.CHUNK, (setting, name, q.size)


def _hold(world, label, slen, sen, params, cases):
    """every listed triple against the brute force and BWT_Search, the must / must-not starts against the oracle's stage-1 seeds.  The oracle's side
    depends on the parameters and the query alone (not on kmer_k): it is computed once per (MinSeedLength, -sen, query) and shared between the rows"""
    ref, idx, o, memo = world
    text = dc.text_of(ref)
    o.set_params(**params)
    listed = checked = 0
    for name, (q, on, off, trip) in cases.items():
        qb = q.tobytes()
        ends = {s: min(q.size, (s // dc.CHUNK + 1) * dc.CHUNK) for s, _, _ in trip}
        key = (slen, sen, qb, tuple(sorted(ends)))
        if key not in memo:
            o.set_query(q)
            found = {}
            for s, end in ends.items():
                ln, locs = o.bwt_search(s, end)
                found[s] = (ln, int(locs.size))
            o.run_to(1)
            qpos, qlen, rpos = o.seeds()
            memo[key] = (found, qpos.copy(), qlen.copy())
        found, qpos, qlen = memo[key]
        listed += len(trip)
        for s, want_len, want_freq in trip:
            ln, nlocs = found[s]
            seed = want_len >= slen and want_freq <= dc.MAX_FREQ
            if name not in SEAM:
                bkey = (qb, s, ends[s])
                if bkey not in memo:
                    memo[bkey] = _brute(text, qb, s, ends[s])      # (does not depend on the row either)
                got = memo[bkey]
                assert got == (want_len, want_freq), (label, name, s, "brute force (len, freq)", got, (want_len, want_freq))
            assert ln == want_len, (label, name, s, "oracle len", ln, want_len)
            assert nlocs == (want_freq if seed else 0), (label, name, s, "oracle freq", nlocs, want_freq)
            checked += 1
        starts = set(np.unique(qpos).tolist())
        missing = [s for s in on if s not in starts]; extra = [s for s in off if s in starts]
        assert not missing and not extra, (label, name, "must_be missing", missing, "must_not_be present", extra)
        for s, want_len, want_freq in trip:                   # a listed start that is a seed's start carries the listed length and count
            if s in starts:
                assert set(qlen[qpos == s].tolist()) == {want_len} and int((qpos == s).sum()) == want_freq, (label, name, s, "seed len / hits")
    assert checked == listed and listed > 0, (label, checked, listed)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_constructions_hold(world, setting):
    slen, sen, params = SETTINGS[setting]
    _hold(world, setting, slen, sen, params, dc.build_cases(slen, sen)[1])


# ---- the (kmer_k, MinSeedLength) grid ----
ROWS = [(K, slen, sen) for K, rows in dc.GRID.items() for slen, sen in rows]
# sha256 (dense_cases.cases_digest) of what build_cases(15) and build_cases(10, sen=True) gave before the module took a kmer_k
DIGEST_BEFORE_GRID = {(dc.DEFAULT_SLEN, False): "f0d8e26bbe15524fb27cbc964c1240208896be938ccfef22a53ff45fcf465ea4",
                      (dc.SEN_SLEN, True): "a052179efea524bd175fab80eefc59442c69560cedb713e741c66813b9a69281"}


def _row_id(row):
    return f"k{row[0]}-" + ("sen" if row[2] else f"slen{row[1]}")


def test_existing_calls_unchanged():
    for (slen, sen), want in DIGEST_BEFORE_GRID.items():
        ref, cases = dc.build_cases(slen, sen)
        assert len(cases) == 43 and dc.cases_digest(ref, cases) == want, (slen, sen)
        assert dc.build_cases(slen, sen, kmer_k=None)[1] is cases


def test_grid_rows_and_families():
    assert set(dc.GRID) == {8, 12, 15}
    seen = {}
    for K, slen, sen in ROWS:
        assert 10 <= slen <= 30 and (not sen or slen == dc.SEN_SLEN)
        ref, cases = dc.build_cases(slen, sen, kmer_k=K)
        assert np.array_equal(ref, dc.build_cases()[0])
        names = list(cases)
        assert len(names) >= 40, (K, slen, sen, len(names))
        for name in dc.DROPPED.get((K, slen, sen), ()):
            assert name not in names
        for fam in dc.NEW_FAMILIES:
            if any(n.startswith(fam) for n in names):
                seen.setdefault(fam, set()).add(K)
        # what each row must hold, from the orderings alone
        assert ("len_klo" in names) == (slen + 1 < K), (K, slen, sen)
        assert ("len_between_min+1" in names) == (slen + 1 < K) and ("len_between_k-1" in names) == (slen + 1 < K), (K, slen, sen)
        assert ("start_at_clen-k" in names) == (K > slen) and ("start_at_clen-k+1" in names) == (K > slen), (K, slen, sen)
        assert ("len_pres_16" in names) == (slen >= 18) and ("len_pres_17" in names) == (slen >= 18), (K, slen, sen)
        assert ("pres_look_2_p16" in names) == (slen > 16) and all(f"pres_look_{j}" in names for j in (1, 2, 3, 4)), (K, slen, sen)
        assert all((f"n_word_32_{o}" in names) == (slen == 30) for o in (29, 30, 31, 32)), (K, slen, sen)
        assert ("handover_last_chunk" in names) == (not sen)
        for name, (q, *_rest) in cases.items():
            assert q.size <= 3 * dc.CHUNK, (K, slen, sen, name, q.size)
    for fam in dc.NEW_FAMILIES:
        assert {12, 15} <= seen.get(fam, set()), (fam, seen.get(fam))
    for key, names in dc.DROPPED.items():
        assert key in ROWS and names, key


def test_grid_text_and_len_follow_kmer_k():
    for K in dc.GRID:
        _, cases = dc.build_cases(15, False, kmer_k=K)
        for n in (63, 64, 65, 127, 128, 129):
            assert cases[f"text_{n}"][3][0][1] == K + n
        if "len_k" in cases:
            assert cases["len_k"][3][0][1] == K
        if "len_k-1" in cases:
            assert cases["len_k-1"][3][0][1] == K - 1
    # MinSeedLength 15 under the text's own kmer_k: the constructions of before the grid, and the new families behind them
    _, c15 = dc.build_cases(15, False, kmer_k=dc.kmer_k_for(2 * dc.REF_LEN))
    for name, (q, on, off, trip) in dc.build_cases()[1].items():
        q2, on2, off2, trip2 = c15[name]
        assert np.array_equal(q, q2) and (on, off, trip) == (on2, off2, trip2), name


@pytest.mark.parametrize("row", ROWS, ids=_row_id)
def test_grid_row_holds(world, row):
    K, slen, sen = row
    ref = world[0]
    text = dc.text_of(ref)
    _, cases = dc.build_cases(slen, sen, kmer_k=K)
    pk = min(slen, 16)
    for name, (q, on, off, trip) in cases.items():            # the presence table's side of pres_look_*: absent by pres_k bases, then present by MinSeedLength
        if name.startswith("pres_look_"):
            j = 2 if name.endswith("p16") else int(name[-1])
            e = off[0]
            assert off[:j] == list(range(e, e + j)), (row, name)
            for s in off[:j]:
                assert bytes(q[s:s + pk]) not in text and set(q[s:s + pk].tolist()) <= ACGT, (row, name, s, "present")
            s = e + j
            assert bytes(q[s:s + pk]) in text, (row, name, s, "absent")
            if name.endswith("p16"):
                assert off == list(range(e, e + j + 1)) and not on and trip[-1][:2] == (s, 16) and 16 < slen
            else:
                assert on == [s] and bytes(q[s:s + slen]) in text and trip[-1][1] >= slen
        if name.startswith("n_word_32_"):
            o = int(name.rsplit("_", 1)[1]); s = (on or off)[0]
            assert q[s + o] == ord("N") and (on == [s]) == (o >= slen), (row, name)
        if name.startswith("start_at_clen-k"):
            s = on[0]
            assert s + K == dc.CHUNK + (1 if name.endswith("+1") else 0) and dc.CHUNK - s >= slen, (row, name)
    _hold(world, _row_id(row), slen, sen, dict(sen=1, clr=50) if sen else dict(slen=slen), cases)
