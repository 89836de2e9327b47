"""bench.py on the GPU (the 5 Mb workload, seconds per run): a plain run measures the headline figure and nothing else and, asked
to, dumps what its last timed step returned -- the same arrays from run to run; --full adds the figures that take passes of
their own."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CONTRACT_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}
FULL_ONLY = {"roofline", "kernels", "stage_ms_one_context_alone", "one_contig_latency", "counters_per_step", "resident", "no_prefetch", "bundled", "extra_workloads", "end_to_end", "cpu_baseline"}


def bench(tmp_path, *args):
    """(result line, detail object) of `bench.py --workload ecoli ...` with its scratch files under tmp_path."""
    env = dict(os.environ, GSA_BENCH_TMP=str(tmp_path / "scratch"), GSA_BENCH_DETAIL=str(tmp_path / "detail.json"))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "ecoli", *args], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    with open(tmp_path / "detail.json") as f:
        return json.loads(lines[0]), json.load(f)


def test_plain_run_measures_the_headline_only_and_dumps_its_last_step(tmp_path):
    dumps = []
    for rep in ("a", "b"):
        line, detail = bench(tmp_path, "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / rep))
        assert CONTRACT_KEYS <= set(line) and line["steps"] == 3 and line["warmup"] == 1 and line["dtype"] == "u8" and line["unit"] == "Gbp/s"
        assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
        assert abs(line["value"] - line["config"]["query_bp_per_step"] / (line["ms_per_step"] * 1e-3) / 1e9) < 0.01 * line["value"]
        assert not (FULL_ONLY & set(line)) and not (FULL_ONLY & set(detail))
        dumps.append({fn[:-4]: np.load(tmp_path / rep / fn) for fn in sorted(os.listdir(tmp_path / rep))})
    a, b = dumps
    assert sorted(a) == ["blocks", "records", "sizes", "strings"] and sum(v.nbytes for v in a.values()) <= 64e6
    for k, v in a.items():
        assert v.dtype == np.float64 and v.shape == b[k].shape and np.array_equal(v, b[k]), k
    contig, length, n_blocks, n_frags, n_aln = a["sizes"][0]
    # (the step's genome is one of the rotating mutated copies of the 5 Mb reference: at 2 % divergence a tenth of the events insert and a
    #  tenth delete up to 10 bases, so its length is within 2 % of the reference's)
    assert a["sizes"].shape == (1, 5) and abs(length - 5_000_000) < 100_000 and n_blocks >= 1 and n_frags > 1000 and n_aln > 0
    assert a["blocks"].shape == (n_blocks, 10) and a["blocks"][:, 5].sum() == n_frags            # every record belongs to a block
    assert a["records"].shape[0] == min(n_frags, 200_000) and a["strings"].shape[0] == min(n_aln, 200_000)
    # (bases and gap signs; 0 = the pools' padding between strings, which the library clears before it writes them)
    assert set(np.unique(a["strings"][:, 2:]).astype(np.uint8).tobytes()) <= set(b"ACGTNacgtn-\0")


def test_full_run_adds_the_figures_that_take_passes_of_their_own(tmp_path):
    line, detail = bench(tmp_path, "--full", "--steps", "3", "--warmup", "1", "--extra", "", "--no-cpu-baseline", "--no-e2e")
    assert CONTRACT_KEYS <= set(line) and line["steps"] == 3 and line["roofline"]["frac"] is not None
    assert {"roofline", "kernels", "stage_ms_one_context_alone", "one_contig_latency", "counters_per_step", "resident", "no_prefetch", "bundled"} <= set(detail)
    assert detail["counters_per_step"]["seeds"] > 0 and detail["stage_ms_one_context_alone"]["seed_search"] > 0
