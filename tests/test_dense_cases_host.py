"""The constructed chunks of tests/dense_cases.py on the CPU, held to a plain reference that is neither the oracle nor a kernel: for every listed
(start, expected_len, expected_freq) the longest match from `start` inside its chunk is found by bytes.find over the forward text + its reverse
complement (extended base by base while the next base is unambiguous, inside the chunk and the longer string still occurs), and its occurrences are
counted by overlapping finds, up to 102.  That has to equal the expectation, and the oracle's BWT_Search(start, chunk end) has to give the same length
and -- where the match is a seed (MinSeedLength bases, at most MaxSeedFreq occurrences) -- as many locations, else none.

The seam cases (back_seam, back_seam_fwd) are held to the oracle ONLY: whether a match may run across the end of the forward strand into the reverse
one, or end at the text's last base, is the reference's decision and not the brute force's; their listed lengths and counts are compared with
BWT_Search alone.

Then the chain: from the oracle's stage-1 seeds, every must_be start is a seed's start and no must_not_be start is.  No listed start may be skipped:
the number of starts checked is held against the number listed.  Both settings: the default MinSeedLength and -sen (the library forces 10).  No GPU."""
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
    yield ref, idx, o
    o.close()


def _brute(text, q, s, end):
    """(length, occurrences up to 102) of the longest match of q[s:] inside [s, end)"""
    L = 0
    while s + L < end and q[s + L] in ACGT and text.find(q[s:s + L + 1]) >= 0:
        L += 1
    return L, (dc.count_in(text, q[s:s + L]) if L else 0)


def test_one_reference_for_both_settings(world):
    ref, idx, _ = world
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


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_constructions_hold(world, setting):
    ref, idx, o = world
    slen, sen, params = SETTINGS[setting]
    text = dc.text_of(ref)
    _, cases = dc.build_cases(slen, sen)
    o.set_params(**params)
    listed = checked = 0
    for name, (q, on, off, trip) in cases.items():
        qb = q.tobytes()
        o.set_query(q)
        listed += len(trip)
        for s, want_len, want_freq in trip:
            end = min(q.size, (s // dc.CHUNK + 1) * dc.CHUNK)
            ln, locs = o.bwt_search(s, end)
            seed = want_len >= slen and want_freq <= dc.MAX_FREQ
            if name not in SEAM:
                got = _brute(text, qb, s, end)
                assert got == (want_len, want_freq), (setting, name, s, "brute force (len, freq)", got, (want_len, want_freq))
            assert ln == want_len, (setting, name, s, "oracle len", ln, want_len)
            assert locs.size == (want_freq if seed else 0), (setting, name, s, "oracle freq", locs.size, want_freq)
            checked += 1
        o.run_to(1)
        qpos, qlen, rpos = o.seeds()
        starts = set(np.unique(qpos).tolist())
        missing = [s for s in on if s not in starts]; extra = [s for s in off if s in starts]
        assert not missing and not extra, (setting, name, "must_be missing", missing, "must_not_be present", extra)
        for s, want_len, want_freq in trip:                   # a listed start that is a seed's start carries the listed length and count
            if s in starts:
                assert set(qlen[qpos == s].tolist()) == {want_len} and int((qpos == s).sum()) == want_freq, (setting, name, s, "seed len / hits")
    assert checked == listed and listed > 0, (setting, checked, listed)
