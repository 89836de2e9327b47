#!/usr/bin/env python3
"""What the chain triples cost: gsa_block_segs on the alignment of a 50 Mb pair, on the GPU (the wall time gsa_get_seg_timing reports: the CIGAR walk with positions,
the four launches behind it, two read-backs and the copies home) and on the host (hostlib.segs: the wall time of gsah_c_segs, the result already in its C form), per
query contig -- and how much of the GPU call is the CIGAR pass in front of it (gsa_block_cigars alone, the same walk without positions, by gsa_get_cigar_timing).

  python tools/chain_time.py [--mb 50] [--rounds 3] [--threads 16] [--gpuindex] [--commit HASH] [--out profiles/chain_time.txt]

The pair is the one of tools/paf_cs_e2e.py and tools/lift_time.py: a repeat-free reference of that many Mb in four sequences (synth.make_pair_fast, fixed seed) and its
1 %-diverged copy as the query; the index files are built once (--gpuindex: on the GPU), outside every timed call.  Every contig is aligned, its triples taken on the GPU and on
the host and the two answers compared; the two sides alternate, --rounds times over, medians reported; the context's first (allocating) call is listed apart.  One
process on the GPU; run it once, under one `timeout`.  Everything besides --out lives in a scratch directory that is removed at the end."""
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
    ap.add_argument("--threads", type=int, default=16, help="threads of the host library's pool")
    ap.add_argument("--gpuindex", action="store_true", help="build the index files with the GPU builder (the same bytes, seconds instead of minutes at 50 Mb)")
    ap.add_argument("--commit", default="", help="what was measured (written into the file)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ["GSA_HOST_THREADS"] = str(a.threads)      # (read once, when the host library's pool comes up)
    from gsalign_amd import capi, hostlib, indexio, synth
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True)
        commit = r.stdout.strip() if r.returncode == 0 else "unknown"
    tmp = tempfile.mkdtemp(prefix="gsa_chain_")
    lines = [f"# gsa_block_segs against hostlib.segs; commit: {commit}",
             f"# gpu_ms: gsa_get_seg_timing around one gsa_block_segs (host wall time inside the call, its CIGAR walk included); cigar_ms: gsa_get_cigar_timing around one "
             f"gsa_block_cigars (that walk without positions); host_ms: wall time of gsah_c_segs (host pool of {a.threads} threads; the walk itself is serial); the sides alternate over "
             f"{a.rounds} rounds; usable CPUs {len(os.sched_getaffinity(0))}"]
    try:
        refs, qrys = synth.make_pair_fast(a.mb * 1000000, 4, 0.01, seed=4100 + a.mb)
        rfa, px = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "ref")
        synth.write_fasta(rfa, refs)
        del refs
        (hostlib.build_index_gpu if a.gpuindex else hostlib.build_index)(rfa, px)
        idx = indexio.load_index(px)
        lines.append(f"## reference {a.mb} Mb in four sequences (synth.make_pair_fast seed {4100 + a.mb}), query: its copy at 1 % divergence, {sum(int(q.size) for _, q in qrys)} bases in {len(qrys)} contigs")
        al = capi.Aligner(idx)
        gpu = [[] for _ in qrys]; cig = [[] for _ in qrys]; host = [[] for _ in qrys]
        first = None
        for rnd in range(a.rounds):
            for ci, (name, seq) in enumerate(qrys):
                r = al.align_contig(seq)
                ms0, _ = al.seg_timing()
                blk, sg = al.block_segs()
                g_ms = al.seg_timing()[0] - ms0
                c0, _ = al.cigar_timing()
                _, ops = al.block_cigars()
                c_ms = al.cigar_timing()[0] - c0
                keep = []
                res = hostlib.result_from_arrays(r, keep)
                t0 = time.perf_counter()
                hblk, hsg = hostlib.segs(None, None, res)
                h_ms = (time.perf_counter() - t0) * 1e3
                if blk.tobytes() != hblk.tobytes() or sg.tobytes() != hsg.tobytes():
                    raise SystemExit(f"contig {ci}: the device's triples are not the host's")
                if first is None:
                    first = g_ms      # (the context's first call allocates: listed, not part of the medians)
                    tag = " (first call: allocates)"
                else:
                    gpu[ci].append(g_ms); tag = ""
                cig[ci].append(c_ms); host[ci].append(h_ms)
                s = (f"{a.mb:4d} Mb contig {ci} ({seq.size} bases, {r['blocks'].size} blocks, {int(r['frags'].size)} records, {int(ops.size)} ops, {int(sg.size)} segments) round {rnd + 1}: "
                     f"gpu_ms={g_ms:.3f}{tag}  cigar_ms={c_ms:.3f}  host_ms={h_ms:.3f}")
                print(s, flush=True); lines.append(s)
        al.close()
        med = lambda v: sorted(v)[len(v) // 2] if v else float("nan")
        for ci in range(len(qrys)):
            g, c, h = med(gpu[ci]), med(cig[ci]), med(host[ci])
            lines.append(f"{a.mb:4d} Mb contig {ci} median: gpu_ms={g:.3f}  of it the CIGAR walk about cigar_ms={c:.3f}  host_ms={h:.3f}  (host / gpu = {h / max(g, 1e-9):.1f})")
        lines.append(f"first call on the context: gpu_ms={first:.3f}")
        if a.out:
            with open(a.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
