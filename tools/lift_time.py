#!/usr/bin/env python3
"""What lifting costs: uniformly random reference positions carried through the alignment of a 50 Mb pair, on the GPU (gsa_lift: the wall time gsa_get_lift_timing
reports, launches, the one read-back and the copy home included) and on the host (hostlib.lift: the wall time of gsah_c_lift on --threads threads, the index already
loaded and the result already in its C form), per query contig.

  python tools/lift_time.py [--mb 50] [--n 10000000] [--rounds 3] [--threads 16] [--commit HASH] [--out profiles/lift_time.txt]

The pair is the one of tools/paf_cs_e2e.py: a repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as
the query; the index files are built once, on the host, outside every timed call.  Every contig is aligned, lifted on the GPU, lifted on the host and the two answers
compared; the two sides alternate, --rounds times over, medians reported.  One process on the GPU; run it once, under one `timeout`.  Everything besides --out lives in
a scratch directory that is removed at the end."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=50)
    ap.add_argument("--n", type=int, default=10000000, help="positions")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="threads of the host comparator's pool")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GSA_HOST_THREADS"] = str(a.threads)      # (read once, when the host library's pool comes up)
    from gsalign_amd import capi, hostlib, indexio, synth
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_lift_")
    lines = [f"# gsa_lift against hostlib.lift: {a.n} uniformly random reference positions per query contig; commit: {commit}",
             f"# gpu_ms: gsa_get_lift_timing around one gsa_lift (host wall time inside the call); host_ms: wall time of gsah_c_lift on {a.threads} threads; the two alternate over "
             f"{a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref")
        synth.write_fasta(rfa, refs)
        del refs
        hostlib.build_index(rfa, px)
        idx = indexio.load_index(px)
        G = int(idx.G)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        pos = np.random.default_rng(99).integers(0, G, a.n).astype(np.int64)
        al = capi.Aligner(idx)
        al.lift_set(pos)
        gpu = [[] for _ in qrys]; host = [[] for _ in qrys]; hits = [0] * len(qrys); recs = [0] * len(qrys)
        for rnd in range(a.rounds):
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                ms0, _ = al.lift_timing()
                H = al.lift()
                gpu[ci].append(al.lift_timing()[0] - ms0)
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                if rnd == 0 and ci == 0:
                    hostlib.lift(px, None, res, pos[:1])      # (the host library loads the index on its first call)
                t0 = time.perf_counter()
                Hh = hostlib.lift(px, None, res, pos)
                host[ci].append((time.perf_counter() - t0) * 1e3)
                if H.tobytes() != Hh.tobytes():
                    raise SystemExit(f"contig {ci}: the device's hits are not the host's")
                hits[ci] = int(H.size); recs[ci] = int(r["frags"].size)
                s = f"{a.mb:4d} Mb contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {recs[ci]} records) round {rnd + 1}: gpu_ms={gpu[ci][-1]:.3f}  host_ms={host[ci][-1]:.3f}  hits={hits[ci]}"
                print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2]
        for ci in range(len(qrys)):
            g, h = med(gpu[ci]), med(host[ci])
            lines.append(f"{a.mb:4d} Mb contig {ci} median: gpu_ms={g:.3f} ({a.n / max(g, 1e-9) / 1e6:.2f} G positions/s)  host_ms={h:.3f} ({a.n / max(h, 1e-9) / 1e6:.3f} G positions/s)  hits={hits[ci]}")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
