#!/usr/bin/env python3
"""GSAlign_hip end to end with and without -gpuvar (the variant pass on the GPU, gsa_call_variants): -timing figures of both, the device
time of the variant pass, and a byte comparison of the two paths' VCF and MAF files.

  python tools/variants_e2e.py [--runs 3] [--mb 250] [--commit HASH] [--parent-cli PATH] [--out profiles/variants_gpuvar.txt]

Input: the pair bench.py's `end_to_end` leg uses (default workload, BASELINE configs[4]: cached index, query genome 0) when the index cache
holds a current index; else a synthetic pair of --mb Mb (one reference sequence, a 1 %-diverged copy as the query: one chromosome-sized
contig), index built here.  Everything this writes besides --out lives in a scratch directory that is removed at the end."""
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
from gsalign_amd import hostlib, synth      # noqa: E402

KEYS = ("variants_s", "align_many_s", "result_copy_s_sum", "vcf_s", "output_drain_after_align_s", "total_s")


def run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} -> {r.returncode}\n{r.stderr[-800:]}")
    t = [ln for ln in r.stderr.splitlines() if ln.startswith("GSA_TIMING ")]
    v = [ln for ln in r.stderr.splitlines() if ln.startswith("GSA_VARIANT_PASS ")]
    return json.loads(t[-1][len("GSA_TIMING "):]), (json.loads(v[-1][len("GSA_VARIANT_PASS "):]) if v else None)


def inputs(tmp, mb):
    """(index prefix, query FASTA, extra CLI flags, description of the input)"""
    import bench
    name, _ = bench.default_workload()
    wl = bench.WORKLOADS[name]
    px = bench.cached_prefix(name, wl)
    qfa = os.path.join(tmp, "q.fa")
    t = time.time()
    if px:
        refs = bench.synth_reference(wl)
        genome = bench.per_contig(lambda i, nr: synth.fast_mutate(nr[1], wl["div"], 7000 + i), refs)      # query genome 0 of bench.make_queries
        synth.write_fasta(qfa, [(f"q{i + 1}", c) for i, c in enumerate(genome)])
        flags = []
        for k, v in (wl.get("params") or {}).items():
            flags += ["-" + k, str(v)]
        return px, qfa, flags, f"bench.py workload {name}: {wl['label']} (cached index, query genome 0; FASTA written in {time.time() - t:.0f} s)"
    refs, qrys = synth.make_pair_fast(mb * 1000000, 1, 0.01, seed=23)
    rfa, px = os.path.join(tmp, "r.fa"), os.path.join(tmp, "r")
    synth.write_fasta(rfa, refs); synth.write_fasta(qfa, qrys)
    hostlib.build_index(rfa, px)
    return px, qfa, [], (f"no cached index of bench.py's default workload on this host: synthetic pair, one sequence of {mb} Mb against its 1 %-diverged copy "
                         f"(synth.make_pair_fast seed 23; inputs + index built in {time.time() - t:.0f} s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--mb", type=int, default=250)
    ap.add_argument("--ctx", type=int, default=2)
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--parent-cli", default="", help="a GSAlign_hip built from the parent commit: its default path is run beside the two (row `parent`)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_var_")
    try:
        px, qfa, flags, what = inputs(tmp, a.mb)
        lines = [f"# GSAlign_hip -timing with and without -gpuvar (opt-in: VariantIdentification on the GPU); commit: {commit}",
                 f"# input: {what}", f"# -ctx {a.ctx}; {a.runs} runs each, alternating, same box, same process environment; seconds (the CLI's own clock)"]
        legs = ([("parent", a.parent_cli, [])] if a.parent_cli else []) + [("default", hostlib.CLI_PATH, []), ("gpuvar", hostlib.CLI_PATH, ["-gpuvar"])]
        rows = {tag: [] for tag, _, _ in legs}
        dev = []
        for i in range(a.runs):
            for tag, cli, flag in legs:
                out = os.path.join(tmp, f"o_{tag}")
                T, V = run([cli, "-i", px, "-q", qfa, "-o", out, "-ctx", str(a.ctx), "-timing", *flags, *flag])
                rows[tag].append(T)
                s = f"{tag:8s} run {i + 1}: " + "  ".join(f"{k}={T[k]:.3f}" for k in KEYS)
                if V:
                    per = V["device_ms_sum"] / max(V["query_bp"], 1) * 250e6
                    dev.append(per)
                    s += f"  variant_pass_device_ms_sum={V['device_ms_sum']:.3f} passes={V['passes']} ({per:.3f} ms per 250 Mb of query)"
                print(s, flush=True); lines.append(s)
        same = all(filecmp.cmp(os.path.join(tmp, "o_default" + e), os.path.join(tmp, f"o_{tag}" + e), shallow=False) for e in (".vcf", ".maf") for tag in rows)
        lines.append(f"VCF and MAF of all legs byte-identical: {same} (VCF {os.path.getsize(os.path.join(tmp, 'o_default.vcf'))} bytes, {T['query_bp']} query bases, {T['contigs']} contigs)")
        for tag, rr in rows.items():
            tot = [r["total_s"] for r in rr]; am = [r["align_many_s"] for r in rr]
            lines.append(f"{tag:8s} median: " + "  ".join(f"{k}={sorted(r[k] for r in rr)[len(rr) // 2]:.3f}" for k in KEYS)
                         + f"  run-to-run spread: total_s {(max(tot) - min(tot)) / min(tot) * 100:.1f} %, align_many_s {(max(am) - min(am)) / min(am) * 100:.1f} %")
        if dev:
            lines.append(f"variant pass, device time (hipEvents around count + scan + emit + the copy home): median {sorted(dev)[len(dev) // 2]:.3f} ms per 250 Mb of query")
        print("\n".join(lines[-4:]))
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
        if not same:
            raise SystemExit("outputs differ")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
