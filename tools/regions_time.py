#!/usr/bin/env python3
"""What lifting intervals costs: random reference regions carried through the alignment of a 50 Mb pair, per query contig,
  regions  on the GPU (gsa_lift_regions: the wall time gsa_get_region_timing reports -- launches, the one read-back and the copy home included), for the regions sorted
           by start and for the same regions shuffled; and for ONE region, which leaves CLASS + PREFIX (they do not depend on the regions) and the call's fixed cost
  host     hostlib.lift_regions (gsah_c_lift_regions on --threads threads, the index already loaded and the result already in its C form)
  perbase  the only device route there was before the pass: gsa_lift of EVERY base of the regions (gsa_get_lift_timing, the positions already on the device -- their
           upload is not counted) plus the reduction of the per-base hits to per-region counts and query ends on the host (numpy), in chunks of --chunk positions

  python tools/regions_time.py [--mb 50] [--rounds 3] [--threads 16] [--commit HASH] [--out profiles/regions_time.txt]

Two region sets: (a) 10^5 regions of 2 kb, (b) 10^7 regions of 100 b, each inside one reference sequence.  The pair is the one of tools/lift_time.py: a repeat-free
reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its 1 %-diverged copy as the query; the index files are built once, on the host,
outside every timed call.  Every contig is aligned; the device's hits are compared with the host's in every round; the legs alternate, --rounds times over, medians
reported.  One process on the GPU; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
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


def make_regions(idx, n, length, rng):
    """n regions of `length` bases, each inside one sequence (sequences drawn by their share of the starts), sorted by start"""
    room = np.maximum(np.asarray(idx.chr_len, np.int64) - length + 1, 0)
    starts = np.concatenate([[0], np.cumsum(idx.chr_len)]).astype(np.int64)
    c = rng.choice(room.size, n, p=room / room.sum())
    beg = np.sort(starts[c] + (rng.random(n) * room[c]).astype(np.int64))
    return beg, beg + length


def per_base(al, beg, length, chunk):
    """the per-base route: (ms inside gsa_lift, ms of the host reduction, regions with a hit)"""
    per = max(chunk // length, 1)
    ms_lift = ms_red = 0.0
    n_hit = 0
    off = np.arange(length, dtype=np.int64)
    for a in range(0, beg.size, per):
        pos = (beg[a:a + per, None] + off[None, :]).ravel()
        al.lift_set(pos)
        m0, _ = al.lift_timing()
        H = al.lift()
        ms_lift += al.lift_timing()[0] - m0
        t0 = time.perf_counter()
        if H.size:
            rid = H["idx"] // length                                   # (positions are region-major, hits ascend in idx: rid is sorted)
            first = np.concatenate([[0], np.flatnonzero(np.diff(rid)) + 1])
            cls = H["cls"]
            n_eq = np.add.reduceat((cls == 7).astype(np.int32), first); n_x = np.add.reduceat((cls == 8).astype(np.int32), first); n_del = np.add.reduceat((cls == 2).astype(np.int32), first)
            q_lo = np.minimum.reduceat(H["qpos"], first); q_hi = np.maximum.reduceat(H["qpos"], first)
            assert n_eq.size == n_x.size == n_del.size == q_lo.size == q_hi.size == first.size
            n_hit += int(first.size)
        ms_red += (time.perf_counter() - t0) * 1e3
    return ms_lift, ms_red, n_hit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16, help="threads of the host comparator's pool")
    ap.add_argument("--chunk", type=int, default=100000000, help="positions per gsa_lift call of the per-base route")
    ap.add_argument("--sets", default="100000x2000,10000000x100", help="region sets: COUNTxLENGTH, comma-separated")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GSA_HOST_THREADS"] = str(a.threads)      # (read once, when the host library's pool comes up)
    from gsalign_amd import capi, hostlib, indexio, synth
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    sets = [tuple(int(v) for v in s.split("x")) for s in a.sets.split(",")]
    tmp = tempfile.mkdtemp(prefix="gsa_regions_")
    lines = [f"# gsa_lift_regions against hostlib.lift_regions and against gsa_lift of every base + a host reduction, per query contig; commit: {commit}",
             f"# sorted_ms / shuffled_ms / one_ms: gsa_get_region_timing around one gsa_lift_regions (host wall time inside the call) for the regions sorted by start, the same shuffled, and ONE region "
             f"(CLASS + PREFIX + the call's fixed cost); host_ms: wall time of gsah_c_lift_regions on {a.threads} threads; perbase_ms: gsa_get_lift_timing of gsa_lift over every base of the sorted regions "
             f"(chunks of {a.chunk} positions, uploads not counted) + the numpy reduction to per-region counts; the legs alternate over {a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref")
        synth.write_fasta(rfa, refs)
        del refs
        hostlib.build_index(rfa, px)
        idx = indexio.load_index(px)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        rng = np.random.default_rng(99)
        regs = []
        for n, L in sets:
            beg, end = make_regions(idx, n, L, rng)
            perm = rng.permutation(n)
            regs.append((n, L, beg, end, perm))
        al = capi.Aligner(idx)
        keys = ("sorted", "shuffled", "one", "host", "perbase_lift", "perbase_reduce")
        T = {(si, ci, k): [] for si in range(len(sets)) for ci in range(len(qrys)) for k in keys}
        hits = {}
        for rnd in range(a.rounds):
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                for si, (n, L, beg, end, perm) in enumerate(regs):
                    if rnd == 0 and ci == 0 and si == 0:      # (the first call loads code objects and sizes buffers; the host library loads the index on its first call)
                        al.regions_set(beg[:1000], end[:1000]); al.lift_regions()
                        hostlib.lift_regions(px, None, res, beg[:1], end[:1])

                    def timed():
                        m0, _ = al.region_timing()
                        H = al.lift_regions()
                        return al.region_timing()[0] - m0, H

                    al.regions_set(beg, end)
                    ms, H = timed(); T[si, ci, "sorted"].append(ms)
                    t0 = time.perf_counter()
                    Hh = hostlib.lift_regions(px, None, res, beg, end)
                    T[si, ci, "host"].append((time.perf_counter() - t0) * 1e3)
                    if H.tobytes() != Hh.tobytes():
                        raise SystemExit(f"set {si} contig {ci}: the device's hits are not the host's")
                    al.regions_set(beg[perm], end[perm])
                    ms, P = timed(); T[si, ci, "shuffled"].append(ms)
                    if P.size != H.size:
                        raise SystemExit(f"set {si} contig {ci}: the shuffled regions give {P.size} hits, the sorted ones {H.size}")
                    al.regions_set(beg[:1], end[:1])
                    ms, _ = timed(); T[si, ci, "one"].append(ms)
                    pl, pr, ph = per_base(al, beg, L, a.chunk)
                    T[si, ci, "perbase_lift"].append(pl); T[si, ci, "perbase_reduce"].append(pr)
                    if ph != H.size:
                        raise SystemExit(f"set {si} contig {ci}: the per-base route finds {ph} regions with a hit, the pass {H.size}")
                    hits[si, ci] = int(H.size)
                    s = (f"{n} x {L} b, contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {r['frags'].size} records) round {rnd + 1}: sorted_ms={T[si, ci, 'sorted'][-1]:.3f}  shuffled_ms={T[si, ci, 'shuffled'][-1]:.3f}  "
                         f"one_ms={T[si, ci, 'one'][-1]:.3f}  host_ms={T[si, ci, 'host'][-1]:.3f}  perbase_ms={pl + pr:.3f} (gsa_lift {pl:.3f} + reduction {pr:.3f})  hits={hits[si, ci]}")
                    print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2]
        for si, (n, L, _, _, _) in enumerate(regs):
            for ci in range(len(qrys)):
                m = {k: med(T[si, ci, k]) for k in keys}
                lines.append(f"{n} x {L} b, contig {ci} median: sorted_ms={m['sorted']:.3f} ({n / max(m['sorted'], 1e-9) / 1e3:.1f} M regions/s)  shuffled_ms={m['shuffled']:.3f}  one_ms={m['one']:.3f}  "
                             f"host_ms={m['host']:.3f}  perbase_ms={m['perbase_lift'] + m['perbase_reduce']:.3f} (gsa_lift {m['perbase_lift']:.3f} + reduction {m['perbase_reduce']:.3f})  hits={hits[si, ci]}")
        lines.append("## UNMEASURED: a whole human reference, results with many overlapping blocks per region, several GPUs.  The default path is untouched: bench.py never reaches the pass.")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
