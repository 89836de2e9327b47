#!/usr/bin/env python3
"""Index build: the host builder (all threads, as it stands) against the GPU builder (hostlib.build_index_gpu -> gsa_build_index), same process, same box.

  python tools/index_build_time.py [--mb 5,50,250] [--out profiles/index_build.json] [--device 0]

Per size: a synthetic reference from gsalign_amd.synth (four sequences, human-like repeats: what the host sorter's depth costs come from), its FASTA written once;
wall seconds of hostlib.build_index and of hostlib.build_index_gpu on it (both include FASTA parsing and writing the five files -- what a user waits for),
the device ms and doubling rounds gsa_get_index_build_stats reports for the GPU build, and a byte comparison of the two sets of files.  One process, one GPU
context at a time; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
import argparse
import filecmp
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsalign_amd import capi, hostlib, synth      # noqa: E402

EXTS = ("bwt", "sa", "pac", "ann", "amb")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", default="5,50,250")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build.json"))
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="gsa_ixtime_")
    rows = []
    try:
        for mb in [int(x) for x in a.mb.split(",") if x]:
            refs = []
            for k in range(4):
                r = synth.fast_genome(mb * 250000, (31 + mb) * 1000 + k)
                synth.inject_human_like(r, (31 + mb) * 1000 + k)
                refs.append((f"chr{k + 1}", r))
            fa = os.path.join(tmp, f"r{mb}.fa")
            synth.write_fasta(fa, refs)
            G = sum(int(s.size) for _, s in refs)
            del refs
            t0 = time.perf_counter(); hostlib.build_index(fa, os.path.join(tmp, "host")); t_host = time.perf_counter() - t0
            t0 = time.perf_counter(); hostlib.build_index_gpu(fa, os.path.join(tmp, "gpu"), a.device); t_gpu = time.perf_counter() - t0
            dev_ms, rounds = capi.index_build_stats()
            same = all(filecmp.cmp(os.path.join(tmp, f"host.{e}"), os.path.join(tmp, f"gpu.{e}"), shallow=False) for e in EXTS)
            row = {"reference_bp": G, "host_build_s": round(t_host, 3), "gpu_build_s": round(t_gpu, 3), "gpu_device_ms": round(dev_ms, 2), "doubling_rounds": rounds,
                   "files_identical": same, "host_threads": int(os.environ.get("GSA_INDEX_THREADS", 0)) or min(os.cpu_count() or 1, 128), "usable_cpus": len(os.sched_getaffinity(0))}
            print(json.dumps(row), flush=True)
            rows.append(row)
            for e in EXTS:
                for p in ("host", "gpu"):
                    os.remove(os.path.join(tmp, f"{p}.{e}"))
            os.remove(fa)
            if not same:
                raise SystemExit("the two builders wrote different files")
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/index_build_time.py", "rows": rows}, fh, indent=1)
            fh.write("\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
