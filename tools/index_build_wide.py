#!/usr/bin/env python3
"""The wide device index builder (gsa_build_index_opts, k_index_wide.hip) at scale: device ms, doubling rounds, batches, peak device bytes and wall seconds.

  python tools/index_build_wide.py [--runs 250,1200,3080] [--append] [--out profiles/index_build_wide.json] [--device 0] [--host-threads 16]

Runs, each once, each a child process under a `timeout` of its own (one GPU context at a time; a run that fails or times out is recorded as such and ends the tool):
  250    a 250 Mb reference (tools/index_build_time.py's: four sequences, human-like repeats): the narrow sorter against the forced wide one (default batch cap,
         and a cap of 2^26 for several batches), index files compared byte for byte with each other
  1200   1.2 Gbp (five sequences, human-like repeats), the first size that takes the AUTO-wide path: hostlib.build_index_gpu against the host builder on
         --host-threads threads, files compared byte for byte; then the program with -memindex on that reference against the program on the index files (MAF bytes)
  3080   bench.py's default workload (24 sequences with GRCh38 lengths, 3.08 Gbp): build_index_gpu against bench.py's cached index files where they exist,
         else against a host build
Wall seconds include FASTA parsing and writing the five files on both sides -- what a user waits for.  The GPU side of a run is measured and written first."""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXTS = ("bwt", "sa", "pac", "ann", "amb")
NOTE = ("each run once; wall seconds are whole builds; peak_device_bytes includes the list of tied suffixes, which is given the free device memory up to 24 bytes "
        "per suffix, so it says that the build fits, not what it needs; tied_after_first_pass is that list's real length at its longest")
LIMITS = {"250": 300, "1200": 840, "3080": 1150}      # seconds of a run's `timeout`


def _same(a, b):
    return all(filecmp.cmp(f"{a}.{e}", f"{b}.{e}", shallow=False) for e in EXTS)


def _gpu_build(hostlib, capi, fa, prefix, device, **kw):
    t0 = time.perf_counter(); hostlib.build_index_gpu(fa, prefix, device, **kw); wall = time.perf_counter() - t0
    ms, rounds = capi.index_build_stats(); batches, peak, active = capi.index_build_stats2()
    return {"gpu_build_s": round(wall, 3), "gpu_device_ms": round(ms, 2), "doubling_rounds": rounds, "batches": batches, "peak_device_bytes": peak,
            "tied_after_first_pass": active}


def _synth(synth, lengths, seed0):
    refs = []
    for k, n in enumerate(lengths):
        r = synth.fast_genome(int(n), seed0 + k)
        synth.inject_human_like(r, seed0 + k)
        refs.append((f"chr{k + 1}", r))
    return refs


def _memindex(hostlib, synth, fa, px, prefix):
    """GSAlign_hip -r ref.fa -memindex (gsa_create_from_pac with the wide sorter above the old bound) against -i <index files>: a 2 Mb query, 1 % diverged from the
    start of the first sequence; whole-program wall seconds and whether the two MAF files are the same bytes"""
    with open(fa, "rb") as fh:
        fh.readline()
        head = fh.read(2_100_000)
    q = synth.fast_mutate(synth.np.frombuffer(head.replace(b"\n", b""), dtype=synth.np.uint8)[:2_000_000].copy(), 0.01, 4711)
    synth.write_fasta(px("q.fa"), [("q", q)])
    out = {}
    for name, args in (("files", ["-i", prefix]), ("memindex", ["-r", fa, "-memindex"])):
        t0 = time.perf_counter()
        p = subprocess.run(["timeout", "-k", "10", "240", hostlib.CLI_PATH, *args, "-q", px("q.fa"), "-o", px("out_" + name), "-t", "16"], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        out[name + "_s"] = round(time.perf_counter() - t0, 3)
        out[name + "_status"] = p.returncode
        if p.returncode != 0:
            out[name + "_stderr"] = p.stderr.decode(errors="replace")[-400:]
            out["maf_identical"] = False
            return out
    out["maf_bytes"] = os.path.getsize(px("out_files.maf"))
    out["maf_identical"] = out["maf_bytes"] > 0 and filecmp.cmp(px("out_files.maf"), px("out_memindex.maf"), shallow=False)
    return out


def one(kind, device, host_threads, row_path):
    from gsalign_amd import capi, hostlib, synth
    tmp = tempfile.mkdtemp(prefix="gsa_ixwide_")
    row = {"run": kind}

    def save():
        with open(row_path, "w") as fh:
            json.dump(row, fh)

    try:
        fa = os.path.join(tmp, "r.fa")
        px = lambda n: os.path.join(tmp, n)
        if kind == "250":
            refs = _synth(synth, [62_500_000] * 4, 281000)
        elif kind == "1200":
            refs = _synth(synth, [240_000_000] * 5, 1231000)
        else:
            import bench
            refs = bench.synth_reference(bench.WORKLOADS["human_full"])
        row["reference_bp"] = sum(int(s.size) for _, s in refs)
        synth.write_fasta(fa, refs)
        del refs
        if kind == "250":
            row["narrow"] = _gpu_build(hostlib, capi, fa, px("narrow"), device); save()
            row["wide"] = _gpu_build(hostlib, capi, fa, px("wide"), device, wide=True); save()
            row["wide_cap_2_26"] = _gpu_build(hostlib, capi, fa, px("wide26"), device, wide=True, batch_cap=1 << 26); save()
            row["files_identical"] = _same(px("narrow"), px("wide")) and _same(px("narrow"), px("wide26"))
        else:
            row.update(_gpu_build(hostlib, capi, fa, px("gpu"), device)); save()
            other, row["compared_with"] = None, "host build"
            if kind == "3080":
                import bench
                other = bench.cached_prefix("human_full", bench.WORKLOADS["human_full"])
                if other:
                    row["compared_with"] = "bench.py's cached index files"
            if not other and kind == "3080" and bench.host_mem_gb() < 256:      # (bench.py's own threshold for building this index on the host)
                row["compared_with"] = "nothing: the host has too little memory for the host build; the files' bytes are UNVERIFIED"
                row["files_identical"] = None
                save()
                return 0
            if not other:
                os.environ["GSA_INDEX_THREADS"] = str(host_threads)
                t0 = time.perf_counter(); hostlib.build_index(fa, px("host")); row["host_build_s"] = round(time.perf_counter() - t0, 3)
                row["host_threads"] = host_threads
                other = px("host")
            row["files_identical"] = _same(px("gpu"), other)
            if kind == "1200" and row["files_identical"]:
                save()
                row["memindex"] = _memindex(hostlib, synth, fa, px, other)
                if not row["memindex"]["maf_identical"]:
                    row["files_identical"] = False
        save()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return 0 if row.get("files_identical") else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="250,1200,3080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build_wide.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--append", action="store_true", help="keep the rows of other runs that --out already holds")
    ap.add_argument("--one", default="", help=argparse.SUPPRESS)
    ap.add_argument("--row", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        raise SystemExit(one(a.one, a.device, a.host_threads, a.row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    kinds = [k for k in a.runs.split(",") if k]
    rows = [r for r in json.load(open(a.out)).get("rows", []) if r.get("run") not in kinds] if a.append and os.path.exists(a.out) else []
    for kind in kinds:
        row_path = a.out + f".{kind}.tmp"
        child = subprocess.Popen(["timeout", "-k", "10", str(LIMITS[kind]), sys.executable, os.path.abspath(__file__), "--one", kind, "--row", row_path,
                                  "--device", str(a.device), "--host-threads", str(a.host_threads)])
        t0 = time.perf_counter()
        while True:
            try:
                rc = child.wait(timeout=60)
                break
            except subprocess.TimeoutExpired:
                print(f"[run {kind}: {time.perf_counter() - t0:.0f} s]", flush=True)
        row = json.load(open(row_path)) if os.path.exists(row_path) else {"run": kind}
        if os.path.exists(row_path):
            os.remove(row_path)
        row["exit_status"] = rc
        print(json.dumps(row), flush=True)
        rows.append(row)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/index_build_wide.py", "note": NOTE, "rows": rows}, fh, indent=1)
            fh.write("\n")
        if rc != 0:
            raise SystemExit(f"run {kind} ended with status {rc}")      # (nothing more is started on the device)


if __name__ == "__main__":
    main()
