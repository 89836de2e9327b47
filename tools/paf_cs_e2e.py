#!/usr/bin/env python3
"""What -cs costs: GSAlign_hip -i ... -q ... -fmt 3 -timing with and without -cs -- whole-program wall times, what -timing says about the CIGAR and cs passes
(cigar_s, cs_s), the PAF bytes and the cs bytes per query base, and a check that the PAF with -cs is the plain PAF plus one cs:Z: field per line.

  python tools/paf_cs_e2e.py [--mb 50] [--rounds 3] [--commit HASH] [--out profiles/paf_cs_e2e.txt]

A repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as the query; the index files are built once
(on the host, outside every timed run); the two modes alternate, --rounds times over, medians reported.  One process on the GPU at a time; run it once, under one
`timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gsalign_amd import hostlib, synth      # noqa: E402

MODES = (("plain", []), ("cs", ["-cs"]))
KEYS = ("total_s", "align_many_s", "cigar_s", "cs_s", "result_copy_s_sum", "maf_format_s", "output_drain_after_align_s", "maf_write_s")


def run_mode(tmp, qfa, flags, threads):
    r = subprocess.run([hostlib.CLI_PATH, "-i", "ref", "-q", qfa, "-o", "out", "-t", str(threads), "-fmt", "3", "-timing", *flags], cwd=tmp, capture_output=True, text=True, timeout=1500)
    if r.returncode != 0:
        raise SystemExit(f"GSAlign_hip {' '.join(flags)} -> {r.returncode}\n{r.stderr[-800:]}")
    t = [ln for ln in r.stderr.splitlines() if ln.startswith("GSA_TIMING ")]
    return json.loads(t[-1][len("GSA_TIMING "):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="-t of the CLI (host side)")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_pafcs_")
    lines = [f"# GSAlign_hip -i ref -q qry.fa -fmt 3 -timing, without / with -cs; commit: {commit}",
             f"# whole-program wall times (the CLI's own clock, seconds); the modes alternate over {a.rounds} rounds; -t {a.threads}; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, qfa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "qry.fa")
        synth.write_fasta(rfa, refs); synth.write_fasta(qfa, qrys)
        qbp = sum(int(q.size) for _, q in qrys)
        del refs, qrys
        hostlib.build_index(rfa, os.path.join(tmp, "ref"))
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {qbp} bases")
        rows = {tag: [] for tag, _ in MODES}; size = {}
        for i in range(a.rounds):
            for tag, flags in MODES:
                T = run_mode(tmp, qfa, flags, a.threads)
                rows[tag].append(T); size[tag] = os.path.getsize(os.path.join(tmp, "out.paf"))
                s = f"{a.mb:4d} Mb {tag:5s} round {i + 1}: " + "  ".join(f"{k}={T.get(k, 0.0):.3f}" for k in KEYS) + f"  paf_bytes={size[tag]}"
                print(s, flush=True); lines.append(s)
                shutil.move(os.path.join(tmp, "out.paf"), os.path.join(tmp, f"{tag}.paf"))
        # the PAF with -cs is the plain PAF plus one field per line
        n_lines, cs_bytes, same = 0, 0, True
        with open(os.path.join(tmp, "plain.paf"), "rb") as fa, open(os.path.join(tmp, "cs.paf"), "rb") as fb:
            for la, lb in zip(fa, fb):
                head, sep, cs = lb.rstrip(b"\n").rpartition(b"\tcs:Z:")
                same = same and sep != b"" and head == la.rstrip(b"\n")
                n_lines += 1; cs_bytes += len(cs)
            same = same and fa.read(1) == b"" and fb.read(1) == b""
        for tag, rr in rows.items():
            med = lambda k: sorted(r.get(k, 0.0) for r in rr)[len(rr) // 2]
            lines.append(f"{a.mb:4d} Mb {tag:5s} median: " + "  ".join(f"{k}={med(k):.3f}" for k in KEYS) + f"  paf_bytes={size[tag]}")
        lines.append(f"{a.mb:4d} Mb {n_lines} PAF lines; with -cs every line is the plain line plus its cs:Z: field: {same}; cs bytes {cs_bytes} = {cs_bytes / max(qbp, 1):.4f} per query base")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
        if not same:
            raise SystemExit("the PAF with -cs is not the plain PAF plus a field")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
