#!/usr/bin/env python3
"""What the per-window query track costs: the alignment of a 50 Mb pair turned into windows of W query bases on the GPU (gsa_query_track: the wall time
gsa_get_qtrack_timing reports, launches, the one read-back and the copy home included), against its yardstick gsa_ref_track on the same context and result (the same
records, the same columns, existing code; gsa_get_track_timing) and against the host (hostlib.qtrack: the wall time of gsah_c_qtrack on --threads threads, the index
already loaded and the result already in its C form), per query contig and window length.

  python tools/qtrack_time.py [--mb 50] [--windows 1000,100000] [--rounds 3] [--threads 16] [--commit HASH] [--out profiles/qtrack_time.txt]

The pair is the one of tools/paf_cs_e2e.py: a repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as
the query; the index files are built once, on the host, outside every timed call.  Every contig is aligned, tracked on the GPU on both sides, tracked on the host and
the answers compared; the three alternate, --rounds times over, medians reported, with gsa_ref_track's own spread (max - min over its rounds) beside them: the new pass
is judged against gsa_ref_track's median plus that spread.  The context's first call allocates the dense array and the pass's other buffers, and no API gives them
back: it is measured in a process of its own (--first-call, started ONCE from here, never in a loop).  One process on the GPU at a time; run it once, under one
`timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def first_call(px, qfa, windows):
    """the child process: a fresh context, contig 0 aligned, one gsa_query_track per window -- the smallest first, which allocates"""
    from gsalign_amd import capi, indexio, synth
    al = capi.Aligner(indexio.load_index(px))
    seq = synth.read_fasta(qfa)[0][1]
    al.align_contig(seq)
    for W in windows:
        al.qtrack_set(W)
        ms0, _ = al.qtrack_timing()
        T = al.qtrack()
        print(f"FIRST W={W} windows={T.size} gpu_ms={al.qtrack_timing()[0] - ms0:.3f}", flush=True)
    al.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=50)
    ap.add_argument("--windows", default="1000,100000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="threads of the host comparator's pool")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--first-call", nargs=2, metavar=("INDEX_PREFIX", "QUERY_FA"), default=None, help="(internal) the child process that measures a context's first call")
    a = ap.parse_args()
    windows = [int(w) for w in a.windows.split(",")]
    if a.first_call:
        return first_call(a.first_call[0], a.first_call[1], windows)
    os.environ["GSA_HOST_THREADS"] = str(a.threads)      # (read once, when the host library's pool comes up)
    from gsalign_amd import capi, hostlib, indexio, synth
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_qtrack_")
    lines = [f"# gsa_query_track against gsa_ref_track (the yardstick: same context, same result) and hostlib.qtrack at W in {windows}; commit: {commit}",
             f"# q_ms: gsa_get_qtrack_timing around one gsa_query_track (host wall time inside the call); r_ms: gsa_get_track_timing around one gsa_ref_track; host_ms: wall time of "
             f"gsah_c_qtrack on {a.threads} threads; the three alternate over {a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px, qfa = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref"), os.path.join(tmp, "q0.fa")
        synth.write_fasta(rfa, refs)
        synth.write_fasta(qfa, qrys[:1])
        del refs
        hostlib.build_index(rfa, px)
        idx = indexio.load_index(px)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        # the first call of a context, in a process of its own, once, before this process opens the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--first-call", px, qfa, "--windows", a.windows], capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            raise SystemExit(f"the first-call process failed ({r.returncode}): {r.stderr[-2000:]}")
        for ln in r.stdout.split("\n"):
            if ln.startswith("FIRST "):
                s = f"{a.mb:4d} Mb first call of a fresh context (contig 0; the smallest W comes first and allocates): {ln[6:]}"
                print(s, flush=True); lines.append(s)
        al = capi.Aligner(idx)
        keys = [(W, ci) for W in windows for ci in range(len(qrys))]
        q_ms = {k: [] for k in keys}; r_ms = {k: [] for k in keys}; host = {k: [] for k in keys}; nwin = {}
        warmed = False
        for rnd in range(a.rounds):
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                if not warmed:
                    hostlib.qtrack(px, int(seq.size), res, windows[0]); al.track_set(windows[0]); al.track(); warmed = True      # (the host library loads the index on its first call; gsa_ref_track allocates on its first)
                for W in windows:
                    al.qtrack_set(W); al.track_set(W)
                    # (alternating: the query side first in odd rounds, the reference side first in even ones)
                    for side in ("qr" if rnd % 2 == 0 else "rq"):
                        if side == "q":
                            ms0, _ = al.qtrack_timing()
                            T = al.qtrack()
                            q_ms[W, ci].append(al.qtrack_timing()[0] - ms0)
                        else:
                            ms0, _ = al.track_timing()
                            R = al.track()
                            r_ms[W, ci].append(al.track_timing()[0] - ms0)
                    t0 = time.perf_counter()
                    Th = hostlib.qtrack(px, int(seq.size), res, W)
                    host[W, ci].append((time.perf_counter() - t0) * 1e3)
                    if T.tobytes() != Th.tobytes():
                        raise SystemExit(f"contig {ci} W={W}: the device's windows are not the host's")
                    pinned = all(int(T[f].sum()) == int(R[f].sum()) for f in ("n_eq", "n_x", "n_ins", "n_del"))
                    nwin[W, ci] = int(T.size)
                    s = (f"{a.mb:4d} Mb contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {r['frags'].size} records) W={W} round {rnd + 1}: q_ms={q_ms[W, ci][-1]:.3f}  "
                         f"r_ms={r_ms[W, ci][-1]:.3f}  host_ms={host[W, ci][-1]:.3f}  windows={nwin[W, ci]}  identical=True  class totals equal gsa_ref_track's={pinned}")
                    print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2]
        for W in windows:
            for ci in range(len(qrys)):
                rm, spread = med(r_ms[W, ci]), max(r_ms[W, ci]) - min(r_ms[W, ci])
                verdict = "within" if med(q_ms[W, ci]) <= rm + spread else "ABOVE"
                lines.append(f"{a.mb:4d} Mb contig {ci} W={W} median: q_ms={med(q_ms[W, ci]):.3f}  r_ms={rm:.3f} (spread {spread:.3f})  host_ms={med(host[W, ci]):.3f}  windows={nwin[W, ci]}  "
                             f"-> {verdict} gsa_ref_track's median + spread")
        lines.append("# UNMEASURED: a result of many overlapping blocks (this pair gives one block per contig, so the depth >= 2 list is empty), W = 1 at scale, a whole human pair")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
