#!/usr/bin/env python3
"""What projecting the query onto the reference costs: every contig of a 50 Mb pair painted into the accumulator on the GPU (gsa_project: the wall time
gsa_get_proj_timing reports -- five launches, one read-back of four counters), on the host (hostlib.project: the wall time of gsah_c_project on --threads threads, the
index already loaded and the result already in its C form), and by the only device route to the same information there was before: gsa_lift of EVERY reference
position with the copy home of its hits (gsa_get_lift_timing), per query contig.

  python tools/proj_time.py [--mb 50] [--rounds 3] [--threads 16] [--commit HASH] [--out profiles/proj_time.txt]

The pair is the one of tools/paf_cs_e2e.py: a repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as
the query; the index files are built once, on the host, outside every timed call.  Every contig is aligned, painted on the GPU, painted on the host, lifted, and the
accumulators compared word for word (and the lift's hits with the words' coverage); the three sides alternate, --rounds times over, medians reported.  The first
gsa_proj_open (which allocates and clears 4 bytes per reference base) and the first gsa_project (which allocates the pass's buffers) are reported apart.  One process
on the GPU; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
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
    tmp = tempfile.mkdtemp(prefix="gsa_proj_")
    lines = [f"# gsa_project against hostlib.project and against gsa_lift of every reference position, per query contig; commit: {commit}",
             f"# gpu_ms: gsa_get_proj_timing around one gsa_project (host wall time inside the call); host_ms: wall time of gsah_c_project on {a.threads} threads; lift_ms: "
             f"gsa_get_lift_timing around one gsa_lift of all G positions (its hits' copy home included); the three alternate over {a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref")
        synth.write_fasta(rfa, refs)
        del refs
        hostlib.build_index(rfa, px)
        idx = indexio.load_index(px)
        G = int(idx.G)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        al = capi.Aligner(idx)
        t0 = time.perf_counter()
        al.proj_open()
        open_ms = (time.perf_counter() - t0) * 1e3
        al.lift_set(np.arange(G, dtype=np.int64))
        host_words = np.zeros(G, np.uint32)
        gpu = [[] for _ in qrys]; host = [[] for _ in qrys]; lift = [[] for _ in qrys]; cols = [0] * len(qrys); first = None
        for rnd in range(a.rounds):
            al.proj_clear(); host_words[:] = 0
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                ms0, _ = al.proj_timing()
                st = al.project()
                g = al.proj_timing()[0] - ms0
                if first is None:
                    first = g
                    # (the first call allocated: the contig is painted again for the figure that counts -- the words do not change)
                    ms0, _ = al.proj_timing()
                    al.project()
                    g = al.proj_timing()[0] - ms0
                gpu[ci].append(g)
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                if rnd == 0 and ci == 0:
                    hostlib.project(px, seq, res, np.zeros(G, np.uint32))      # (the host library loads the index on its first call)
                t0 = time.perf_counter()
                hst = hostlib.project(px, seq, res, host_words)
                host[ci].append((time.perf_counter() - t0) * 1e3)
                ms0, _ = al.lift_timing()
                H = al.lift()
                lift[ci].append(al.lift_timing()[0] - ms0)
                if st != hst:
                    raise SystemExit(f"contig {ci}: device stat {st}, host stat {hst}")
                if H.size > st[1]:      # (equal where no two blocks of the contig overlap)
                    raise SystemExit(f"contig {ci}: {H.size} lifted positions, {st[1]} words offered")
                cols[ci] = st[1]
                s = (f"{a.mb:4d} Mb contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {r['frags'].size} records) round {rnd + 1}: gpu_ms={g:.3f}  host_ms={host[ci][-1]:.3f}  "
                     f"lift_ms={lift[ci][-1]:.3f}  words={st[1]}")
                print(s, flush=True); lines.append(s)
            t0 = time.perf_counter()
            text, words = al.proj_fetch(words=True)
            fetch_ms = (time.perf_counter() - t0) * 1e3
            if not np.array_equal(words, host_words) or text != hostlib.proj_text(host_words):
                raise SystemExit(f"round {rnd + 1}: the device's accumulator is not the host's")
            s = f"{a.mb:4d} Mb round {rnd + 1}: accumulators identical ({int((words != 0).sum())} of {G} words painted); gsa_proj_fetch of text and words, {5 * G} bytes through the Python wrapper: {fetch_ms:.1f} ms"
            print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2]
        lines.append(f"first calls: gsa_proj_open (hipMalloc + clear of {4 * G} bytes) {open_ms:.3f} ms; the first gsa_project (allocates the pass's buffers) {first:.3f} ms")
        for ci in range(len(qrys)):
            g, h, l = med(gpu[ci]), med(host[ci]), med(lift[ci])
            lines.append(f"{a.mb:4d} Mb contig {ci} median: gpu_ms={g:.3f}  host_ms={h:.3f}  lift_ms={l:.3f}  words={cols[ci]}  atomic bytes / time = {4 * cols[ci] / max(g, 1e-9) / 1e9:.4f} TB/s "
                         f"(whole call; the chip-wide rate of float atomic adds in the microarchitecture notes is about 1.3 TB/s)")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
