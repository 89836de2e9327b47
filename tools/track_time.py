#!/usr/bin/env python3
"""What the per-window reference track costs: the alignment of a 50 Mb pair turned into windows of W reference bases, on the GPU (gsa_ref_track: the wall time
gsa_get_track_timing reports, launches, the one read-back and the copy home included) and on the host (hostlib.track: the wall time of gsah_c_track on --threads
threads, the index already loaded and the result already in its C form), per query contig and window length.

  python tools/track_time.py [--mb 50] [--windows 1000,100000] [--rounds 3] [--threads 16] [--commit HASH] [--out profiles/track_time.txt]

The pair is the one of tools/paf_cs_e2e.py: a repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as
the query; the index files are built once, on the host, outside every timed call.  Every contig is aligned, tracked on the GPU, tracked on the host and the two answers
compared; the two sides alternate, --rounds times over, medians reported.  The context's first call, which allocates and clears the dense array, is reported apart
(a call of its own before the rounds).  One process on the GPU; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is
removed at the end."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=50)
    ap.add_argument("--windows", default="1000,100000")
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
    windows = [int(w) for w in a.windows.split(",")]
    tmp = tempfile.mkdtemp(prefix="gsa_track_")
    lines = [f"# gsa_ref_track against hostlib.track at W in {windows}; commit: {commit}",
             f"# gpu_ms: gsa_get_track_timing around one gsa_ref_track (host wall time inside the call); host_ms: wall time of gsah_c_track on {a.threads} threads; the two alternate over "
             f"{a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref")
        synth.write_fasta(rfa, refs)
        del refs
        hostlib.build_index(rfa, px)
        idx = indexio.load_index(px)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        al = capi.Aligner(idx)
        # the first call of the context: it allocates and clears the dense array (16 bytes per window of the reference), the tables and the output
        r = al.align_contig(qrys[0][1])
        for W in windows:
            al.track_set(W)
            ms0, _ = al.track_timing()
            T = al.track()
            s = f"{a.mb:4d} Mb W={W} first call after gsa_track_set (contig 0, {T.size} windows; the smallest W comes first and allocates): gpu_ms={al.track_timing()[0] - ms0:.3f}"
            print(s, flush=True); lines.append(s)
        gpu = {(W, ci): [] for W in windows for ci in range(len(qrys))}; host = {k: [] for k in gpu}; nwin = {}
        warmed = False
        for rnd in range(a.rounds):
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                if not warmed:
                    hostlib.track(px, None, res, windows[0]); warmed = True      # (the host library loads the index on its first call)
                for W in windows:
                    al.track_set(W)
                    ms0, _ = al.track_timing()
                    T = al.track()
                    gpu[W, ci].append(al.track_timing()[0] - ms0)
                    t0 = time.perf_counter()
                    Th = hostlib.track(px, None, res, W)
                    host[W, ci].append((time.perf_counter() - t0) * 1e3)
                    if T.tobytes() != Th.tobytes():
                        raise SystemExit(f"contig {ci} W={W}: the device's windows are not the host's")
                    nwin[W, ci] = int(T.size)
                    s = (f"{a.mb:4d} Mb contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {r['frags'].size} records) W={W} round {rnd + 1}: gpu_ms={gpu[W, ci][-1]:.3f}  "
                         f"host_ms={host[W, ci][-1]:.3f}  windows={nwin[W, ci]}  identical=True")
                    print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2]
        for W in windows:
            for ci in range(len(qrys)):
                lines.append(f"{a.mb:4d} Mb contig {ci} W={W} median: gpu_ms={med(gpu[W, ci]):.3f}  host_ms={med(host[W, ci]):.3f}  windows={nwin[W, ci]}")
        lines.append("# UNMEASURED: a result of many overlapping blocks (this pair gives one block per contig), W = 1, a whole human reference")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
