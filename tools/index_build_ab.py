#!/usr/bin/env python3
"""The narrow device index builder (gsa_build_index) at 250 Mb, another build of the library against this tree's: device ms per child process, the two alternating,
three pairs, on one input (tools/index_build_wide.py's 250 Mb reference).

  python tools/index_build_ab.py --parent-lib /path/to/parent/libgsa_hip.so [--out profiles/index_build_narrow_ab.json]

Each child runs under a `timeout` of its own with GSA_LIB_PATH naming its library; a child that fails ends the tool."""
import json, os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) == 3 and not sys.argv[1].startswith("--"):      # child: pac file, G
    import numpy as np
    from gsalign_amd import capi
    pac = np.fromfile(sys.argv[1], dtype=np.uint8); G = int(sys.argv[2])
    lib = capi.load_library(); lib.gsa_build_index.argtypes = capi.BUILD_INDEX_ARGTYPES
    import ctypes as C
    bw, ns = capi.index_sizes(G)
    bwt = np.zeros(bw, np.uint32); sa = np.zeros(ns, np.uint64); p = C.c_uint64(); L2 = (C.c_uint64 * 5)()
    rc = lib.gsa_build_index(0, C.c_void_p(pac.ctypes.data), G, C.byref(p), L2, C.c_void_p(bwt.ctypes.data), C.c_void_p(sa.ctypes.data))
    assert rc == 0, rc
    ms, rounds = capi.index_build_stats()
    import zlib
    print(json.dumps({"ms": round(ms, 2), "rounds": rounds, "crc": zlib.crc32(bwt.tobytes()) ^ zlib.crc32(sa.tobytes())}))
    raise SystemExit(0)
import argparse
from gsalign_amd import hostlib, synth
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build_narrow_ab.json"))
a = ap.parse_args()
tmp = tempfile.mkdtemp(prefix="gsa_ab_")
refs = []
for k in range(4):
    r = synth.fast_genome(62_500_000, 281000 + k); synth.inject_human_like(r, 281000 + k); refs.append((f"chr{k + 1}", r))
fa = os.path.join(tmp, "r.fa"); synth.write_fasta(fa, refs); del refs
ref = hostlib.reference_from_fasta(fa)
pac, G = (ref["pac"], ref["G"]) if isinstance(ref, dict) else (ref[0], ref[1])
pf = os.path.join(tmp, "r.pac"); pac.tofile(pf)
out = {"parent": [], "tree": []}
libs = {"parent": os.path.abspath(a.parent_lib), "tree": os.path.join(ROOT, "gsalign_amd", "lib", "libgsa_hip.so")}
for pair in range(3):
    for who in ("parent", "tree"):
        p = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.abspath(__file__), pf, str(G)], env=dict(os.environ, GSA_LIB_PATH=libs[who]), capture_output=True, text=True)
        if p.returncode != 0:
            print(who, pair, "status", p.returncode, p.stderr[-500:]); raise SystemExit(1)
        row = json.loads(p.stdout.strip().splitlines()[-1]); out[who].append(row); print(who, pair, row, flush=True)
import shutil; shutil.rmtree(tmp, ignore_errors=True)
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump({"tool": "tools/index_build_ab.py", "what": "narrow device builder (gsa_build_index) at 250 Mb, human-like repeats: device ms per child process, the parent commit's library and this tree's alternating, three pairs; crc: the arrays' checksum", "rows": out}, fh, indent=1)
    fh.write("\n")
