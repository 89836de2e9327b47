#!/usr/bin/env python3
"""GSAlign_hip from two FASTA files, three ways: plain (-r: the host builds the index files), -gpuindex (the GPU builds them) and -memindex (the index is
built in device memory, gsa_create_from_pac: no file) -- whole-program wall times, what -timing says about the build / create terms, the bytes each way
leaves beside the reference, and a byte comparison of the three ways' MAF and VCF files.

  python tools/memindex_e2e.py [--mb 5,50,250] [--rounds 3] [--commit HASH] [--out profiles/memindex_e2e.txt]

Per size: a reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as the query.  Every run gets a
fresh directory with a copy of the reference FASTA in it (so nothing of an earlier run's index is found); the modes alternate, --rounds times over.
One process on the GPU at a time; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
import argparse
import filecmp
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsalign_amd import hostlib, synth      # noqa: E402

MODES = (("plain", []), ("gpuindex", ["-gpuindex"]), ("memindex", ["-memindex"]))
KEYS = ("total_s", "align_starts_at_s", "index_build_s", "index_load_s", "ref_parse_s", "gsa_create_s", "create_from_pac_s", "align_many_s")


def run_mode(tmp, rfa, qfa, flags, keep, threads):
    """one run in a fresh directory -> (-timing dict, bytes left beside the reference); its MAF / VCF are moved to `keep`"""
    d = tempfile.mkdtemp(prefix="run_", dir=tmp)
    try:
        shutil.copy(rfa, os.path.join(d, "ref.fa"))
        r = subprocess.run([hostlib.CLI_PATH, "-r", "ref.fa", "-q", qfa, "-o", "out", "-t", str(threads), "-timing", *flags], cwd=d, capture_output=True, text=True, timeout=1500)
        if r.returncode != 0:
            raise SystemExit(f"GSAlign_hip {' '.join(flags)} -> {r.returncode}\n{r.stderr[-800:]}")
        t = [ln for ln in r.stderr.splitlines() if ln.startswith("GSA_TIMING ")]
        T = json.loads(t[-1][len("GSA_TIMING "):])
        beside = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f not in ("ref.fa", "out.maf", "out.vcf"))
        for e in (".maf", ".vcf"):
            shutil.move(os.path.join(d, "out" + e), keep + e)
        return T, beside
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", default="5,50,250")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="-t of the CLI (host side)")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_memix_")
    lines = [f"# GSAlign_hip -r ref.fa -q qry.fa -timing: plain / -gpuindex / -memindex; commit: {commit}",
             f"# whole-program wall times (the CLI's own clock, seconds); every run in a fresh directory; the modes alternate over {a.rounds} rounds; -t {a.threads}; "
             f"host threads: {os.environ.get('GSA_INDEX_THREADS', 'all')} (index builder), usable CPUs {len(os.sched_getaffinity(0))}"]
    ok = True
    try:
        for mb in [int(x) for x in a.mb.split(",") if x]:
            refs, qrys = synth.make_pair_fast(mb * 1000000, 4, 0.01, seed=4100 + mb)
            rfa, qfa = os.path.join(tmp, f"r{mb}.fa"), os.path.join(tmp, f"q{mb}.fa")
            synth.write_fasta(rfa, refs); synth.write_fasta(qfa, qrys)
            del refs, qrys
            lines.append(f"## reference {mb} Mb in four sequences (synth.make_pair_fast seed {4100 + mb}), query: its copy at 1 % divergence")
            rows = {tag: [] for tag, _ in MODES}; beside = {}
            for i in range(a.rounds):
                for tag, flags in MODES:
                    T, b = run_mode(tmp, rfa, qfa, flags, os.path.join(tmp, f"o{mb}_{tag}"), a.threads)
                    rows[tag].append(T); beside[tag] = b
                    s = f"{mb:4d} Mb {tag:9s} round {i + 1}: " + "  ".join(f"{k}={T.get(k, 0.0):.3f}" for k in KEYS) + f"  bytes_beside_reference={b}"
                    print(s, flush=True); lines.append(s)
                    for e in (".maf", ".vcf"):
                        if tag != "plain" and not filecmp.cmp(os.path.join(tmp, f"o{mb}_plain{e}"), os.path.join(tmp, f"o{mb}_{tag}{e}"), shallow=False):
                            ok = False; lines.append(f"!! {mb} Mb round {i + 1}: {tag}{e} differs from plain{e}")
            for tag, rr in rows.items():
                med = lambda k: sorted(r.get(k, 0.0) for r in rr)[len(rr) // 2]
                lines.append(f"{mb:4d} Mb {tag:9s} median: " + "  ".join(f"{k}={med(k):.3f}" for k in KEYS) + f"  bytes_beside_reference={beside[tag]}")
            lines.append(f"{mb:4d} Mb MAF and VCF of the three modes byte-identical in every round: {ok} "
                         f"(MAF {os.path.getsize(os.path.join(tmp, f'o{mb}_plain.maf'))} bytes, VCF {os.path.getsize(os.path.join(tmp, f'o{mb}_plain.vcf'))} bytes)")
            for f in os.listdir(tmp):
                os.remove(os.path.join(tmp, f))
            if a.out:      # (written size by size: a run that is cut short keeps what it has)
                with open(a.out, "w") as fh:
                    fh.write("\n".join(lines) + "\n")
            if not ok:
                raise SystemExit("outputs differ")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
