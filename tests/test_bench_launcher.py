"""bench.py --gpus N must really become N ranks (round-1 finding: the flag was parsed and ignored).  CPU check with the
--dry stub: `python bench.py --gpus 2 --dry` re-executes itself under torch.distributed.run, rank 0 prints one JSON line
with n_gpus = 2, and the staged result gather (shard.ResultStage / gather_staged: ONE genome's contigs dealt to the ranks by LPT,
every finished contig to rank 0, checked byte for byte inside the run) has left all contigs of the genome on rank 0."""
import json
import os
import subprocess
import sys

from conftest import ROOT


def run(*args):
    env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_gpus_2_relaunches_as_two_ranks():
    d = run("--gpus", "2", "--dry", "--steps", "3", "--warmup", "1")
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1 and d["config"]["contigs_on_rank0_after_gather"] == 5 and d["config"]["world_size"] == 2
    assert d["scaling"] == "strong" and d["higher_is_better"] is True and d["value"] > 0


def test_gpus_1_runs_in_process():
    d = run("--dry", "--steps", "2", "--warmup", "0")
    assert d["n_gpus"] == 1


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--dry"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


CONTRACT_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}


def test_dry_line_is_compact_and_complete():
    """Round 5's driver record had `parsed: null`: the line was 32 KB and the driver keeps less of stdout than that.  The LAST stdout
    line must be one small strict-JSON object with the contract's keys."""
    env = dict(os.environ); env.pop("WORLD_SIZE", None); env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--steps", "2", "--warmup", "1"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    last = r.stdout.rstrip("\n").splitlines()[-1]
    assert len(last) < 4096
    d = json.loads(last, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))      # NaN / Infinity refused
    assert CONTRACT_KEYS <= set(d) and isinstance(d["config"]["workload"], str) and len(d["config"]["workload"]) <= 120


def test_compact_line_of_a_full_measurement():
    """The whole object of a real run (round 5's 32 KB line, kept under profiles/) through bench.compact_line: < 4 KB, strict JSON, the
    contract's keys + roofline + cpu_baseline + end_to_end, one entry per further workload."""
    sys.path.insert(0, ROOT)
    import bench
    full = json.loads(open(os.path.join(ROOT, "profiles", "r05_bench_default.json")).read().strip().splitlines()[-1])
    full["roofline"]["physical_frac"] = float("nan"); full["kernels"][0]["achieved"] = float("inf")           # what a zero-duration timer would produce
    line = bench.compact_line(bench._clean(full))
    assert len(line) < 4096 and "\n" not in line
    d = json.loads(line, parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    assert CONTRACT_KEYS <= set(d)
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic", "physical_frac", "algorithmic_bytes_per_step"} <= set(d["roofline"])
    assert {"value", "unit", "cores", "kind", "sample", "parity_sample"} <= set(d["cpu_baseline"])
    assert {"total_s", "align_many_s"} <= set(d["end_to_end"])
    assert d["roofline"]["physical_frac"] is None and abs(d["roofline"]["frac"] - full["roofline"]["frac"]) < 1e-3
    assert [e["workload"] for e in d["extra_workloads"]] == [e["workload"] for e in full["extra_workloads"]]
    assert len(d["config"]["workload"]) <= 120 and abs(d["value"] - full["value"]) < 1e-3
    json.dumps(bench._clean(full), allow_nan=False)                  # the detail file is strict JSON as well


def test_dump_outputs_is_refused_without_a_timed_path():
    """--dump-outputs writes what the timed GPU path returned: the --dry stub has no such result, and the option says so."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--dump-outputs", "x"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr


def test_output_dump_arrays(tmp_path):
    """bench.OutputDump on a made-up gsa_result: every contig's sizes, all rows of a small array, a seeded sample (with row numbers)
    of a large one, float64 throughout, the same files from the same input, and far below the 64 MB a dump may take."""
    import ctypes as C

    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from gsalign_amd import capi
    B = np.zeros(3, capi.BLOCK_DT); B["score"] = [5, 6, 7]; B["frag_off"] = [0, 10, 2 ** 40]; B["chr"] = [1, 2, 3]
    R = np.zeros(500_000, capi.REC_DT); R["w0"] = np.arange(R.size); R["w3"] = 2 ** 32 - 1
    a1 = (np.arange(1_000_000) % 251).astype(np.uint8); a2 = a1[::-1].copy()
    r = capi.Result(); r.n_blocks = 3; r.n_frags = R.size; r.n_aln = a1.size
    r.blocks = C.cast(B.ctypes.data, C.POINTER(capi.Block)); r.recs = C.cast(R.ctypes.data, C.POINTER(capi.Rec))
    r.aln1 = C.cast(a1.ctypes.data, C.POINTER(C.c_char)); r.aln2 = C.cast(a2.ctypes.data, C.POINTER(C.c_char))
    out = []
    for rep in range(2):
        d = bench.OutputDump(str(tmp_path / f"d{rep}"), 2)
        d.take(1, 123, r); d.take(0, 77, r)                      # (contexts finish in any order)
        d.write()
        out.append({fn[:-4]: np.load(tmp_path / f"d{rep}" / fn) for fn in sorted(os.listdir(tmp_path / f"d{rep}"))})
    x, y = out
    assert sorted(x) == ["blocks", "records", "sizes", "strings"]
    assert all(v.dtype == np.float64 and np.array_equal(v, y[k]) for k, v in x.items()) and sum(v.nbytes for v in x.values()) < 64e6
    assert x["sizes"].tolist() == [[0, 77, 3, 500000, 1000000], [1, 123, 3, 500000, 1000000]]
    assert x["blocks"].shape == (6, 10) and x["blocks"][2].tolist() == [0, 2, 7, 0, 0, 0, 2 ** 40, 0, 0, 3]
    per = bench.DUMP_ROWS // 2
    assert x["records"].shape == (2 * per, 6) and x["strings"].shape == (2 * per, 4)
    rows = x["records"][:, 1].astype(np.int64)
    assert np.array_equal(x["records"][:, 2], R["w0"][rows]) and (x["records"][:, 5] == 2 ** 32 - 1).all() and (np.diff(rows[:per]) >= 0).all()
    off = x["strings"][:, 1].astype(np.int64)
    assert np.array_equal(x["strings"][:, 2], a1[off]) and np.array_equal(x["strings"][:, 3], a2[off])
    d = bench.OutputDump(str(tmp_path / "short"), 2); d.take(0, 77, r)
    try:
        d.write(); raise AssertionError("a dump that misses a contig of the step must not be written")
    except RuntimeError:
        pass


def test_set_up_on_threads_gives_the_serial_genomes():
    """The benchmark generates its contigs on a pool of threads: same seeds, same bytes as the plain loop."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from gsalign_amd import synth
    wl = dict(bench.WORKLOADS["yeast"], lengths=[40_000, 30_000, 20_000], repeats=True, n_query=2)
    refs = bench.synth_reference(wl)
    for i, (name, r) in enumerate(refs):
        want = synth.fast_genome(wl["lengths"][i], 11000 + i); synth.inject_repeats(want, 11000 + i)
        assert name == f"chr{i + 1}" and np.array_equal(r, want)

    class Args:
        fasta_query = ""
    for k, gq in enumerate(bench.make_queries(wl, refs, Args)):
        for i, (_, r) in enumerate(refs):
            assert np.array_equal(gq[i], synth.fast_mutate(r, wl["div"], 7000 + 10 * k + i))


def test_cached_index_is_used_only_when_current(tmp_path, monkeypatch):
    """prepare_inputs() leaves `<workload>_<bases>.done` holding the key of the checkout that built the index; a missing marker,
    another key or an empty GSA_BENCH_CACHE mean: no cached index, the run builds its own."""
    sys.path.insert(0, ROOT)
    import bench
    wl = bench.WORKLOADS["ecoli"]
    monkeypatch.setenv("GSA_BENCH_CACHE", str(tmp_path))
    assert bench.cache_dir() == str(tmp_path) and bench.cached_prefix("ecoli", wl) is None
    px = tmp_path / "ecoli_5000000"
    (tmp_path / "ecoli_5000000.done").write_text("0123456789abcdef")
    assert bench.cached_prefix("ecoli", wl) is None
    (tmp_path / "ecoli_5000000.done").write_text(bench.cache_key("ecoli", wl))
    assert bench.cached_prefix("ecoli", wl) == str(px)
    assert bench.cache_key("ecoli", wl) != bench.cache_key("ecoli", dict(wl, lengths=[5_000_001]))
    monkeypatch.setenv("GSA_BENCH_CACHE", "")
    assert bench.cache_dir() is None and bench.cached_prefix("ecoli", wl) is None
