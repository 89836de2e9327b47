"""gsa_build_index on the GPU: the suffix sorter and the BWT / Occ / SA-sample passes of k_index.hip against the index files the reference
wrote (tests/golden) and against the host builder run serially (SA-IS, which test_host_components.py pins to the reference's builder) on the
shapes where a prefix-doubling sorter can go wrong.  Every comparison is exact equality."""
import os
import subprocess
import threading

import numpy as np
import pytest

from gsalign_amd import capi, hostlib, synth
from index_shapes import SHAPES, _load

pytestmark = pytest.mark.gpu
EXTS = ("bwt", "sa", "pac", "ann", "amb")


def _check(prefix):
    pac, G, hdr, bwt, sa = _load(prefix)
    got_hdr, got_bwt, got_sa = capi.build_index_arrays(pac, G)
    assert got_bwt.size == bwt.size and got_sa.size == sa.size
    assert np.array_equal(got_hdr, hdr), (got_hdr, hdr)
    assert np.array_equal(got_bwt, bwt), f"bwt words differ, first at {np.flatnonzero(got_bwt != bwt)[:5]}"
    assert np.array_equal(got_sa, sa), f"sa samples differ, first at {np.flatnonzero(got_sa != sa)[:5]}"


@pytest.mark.parametrize("name", ["cx", "small"])
def test_golden_index_files(golden_dir, name):
    _check(os.path.join(golden_dir, name))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes_against_the_serial_host_builder(tmp_path, monkeypatch, shape):
    monkeypatch.setenv("GSA_INDEX_THREADS", "1")             # SA-IS
    fa = str(tmp_path / "r.fa")
    synth.write_fasta(fa, [(f"c{k}", s) for k, s in enumerate(SHAPES[shape])])
    hostlib.build_index(fa, str(tmp_path / "r"))
    _check(str(tmp_path / "r"))


def test_seam_end_to_end_with_n_runs(tmp_path, monkeypatch):
    """hostlib.build_index_gpu: FASTA parsing, N -> lrand48 and the five writers around the device builder"""
    monkeypatch.setenv("GSA_INDEX_THREADS", "1")
    rng = np.random.default_rng(5)
    s = synth.random_genome(30001, rng)
    s[1000:1300] = ord("N"); s[20000:20007] = ord("n")
    fa = str(tmp_path / "n.fa")
    synth.write_fasta(fa, [("withN", s)])
    hostlib.build_index(fa, str(tmp_path / "host"))
    hostlib.build_index_gpu(fa, str(tmp_path / "gpu"))
    for ext in EXTS:
        assert open(tmp_path / f"gpu.{ext}", "rb").read() == open(tmp_path / f"host.{ext}", "rb").read(), ext


def test_large_with_planted_repeats(tmp_path, monkeypatch):
    monkeypatch.setenv("GSA_INDEX_THREADS", "1")
    rng = np.random.default_rng(77)
    s = synth.random_genome(1000003, rng)
    s[700000:720000] = s[100000:120000]                                  # a 20 kb exact repeat
    s[900000:920000] = synth.revcomp(s[300000:320000])                   # a 20 kb reverse-complement repeat
    fa = str(tmp_path / "big.fa")
    synth.write_fasta(fa, [("big", s)])
    hostlib.build_index(fa, str(tmp_path / "big"))
    _check(str(tmp_path / "big"))
    ms, rounds = capi.index_build_stats()
    print(f"1 000 003 bases: {ms:.2f} ms on the device, {rounds} doubling rounds")
    assert rounds >= 2 and ms > 0                                         # the doubling path ran


def test_two_threads_on_one_device(golden_dir):
    pac, G, hdr, bwt, sa = _load(os.path.join(golden_dir, "small"))
    res, errs = [None, None], []

    def work(k):
        try:
            res[k] = capi.build_index_arrays(pac, G)
        except Exception as e:      # (reported by the main thread)
            errs.append(e)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for k in range(2):
        assert np.array_equal(res[k][0], hdr) and np.array_equal(res[k][1], bwt) and np.array_equal(res[k][2], sa), k


def test_cli_index_subcommand(golden_dir, tmp_path):
    subprocess.run([hostlib.CLI_PATH, "index", "-gpuindex", os.path.join(golden_dir, "cx.ref.fa"), str(tmp_path / "cx")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for ext in EXTS:
        assert open(tmp_path / f"cx.{ext}", "rb").read() == open(os.path.join(golden_dir, f"cx.{ext}"), "rb").read(), ext


def test_cli_builds_its_index_on_the_gpu_and_aligns(golden_dir, tmp_path):
    """-r with -gpuindex: the copy of cx.ref.fa is called `cx`, so the index prefix and the VCF's ##reference line are those of the golden run (-i cx)"""
    import shutil
    shutil.copy(os.path.join(golden_dir, "cx.ref.fa"), tmp_path / "cx")
    subprocess.run([hostlib.CLI_PATH, "-r", "cx", "-q", os.path.join(golden_dir, "cx.qry.fa"), "-gpuindex", "-o", "out", "-t", "1"], cwd=tmp_path, check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for ext in EXTS:
        assert open(tmp_path / f"cx.{ext}", "rb").read() == open(os.path.join(golden_dir, f"cx.{ext}"), "rb").read(), ext
    assert open(tmp_path / "out.maf", "rb").read() == open(os.path.join(golden_dir, "cx.maf"), "rb").read()
    assert open(tmp_path / "out.vcf", "rb").read() == open(os.path.join(golden_dir, "cx.vcf"), "rb").read()
