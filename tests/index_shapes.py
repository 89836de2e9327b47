"""The shapes test_gpu_index_build.py and test_gpu_index_build_wide.py put through the device index builder, and their readers -- a helper module, not a conftest."""
import numpy as np

from gsalign_amd import indexio, synth


def _load(prefix):
    """(pac bytes, G, hdr, bwt, sa) of index files"""
    G = int(open(prefix + ".ann").readline().split()[0])
    idx = indexio.load_index(prefix)
    return np.fromfile(prefix + ".pac", dtype=np.uint8)[:(G + 3) // 4], G, idx.hdr, idx.bwt, idx.sa


def _ascii(codes):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.asarray(codes, dtype=np.int64)]


def _shapes():
    rng = np.random.default_rng(20261018)
    R = lambda n: synth.random_genome(n, rng)
    out = {}
    for G in (1, 2, 3, 5, 31, 32, 33):                      # shorter than one key, on the key's edge, every G % 4
        out[f"G{G}"] = [R(G)]
    out["G2049"] = [R(2049)]                                 # S + 1 just over one 4096-key sort tile
    out["allA4099"] = [_ascii(np.zeros(4099))]               # A...AT...T: LCPs of about G, the end-of-text rule on a run of the smallest letter; wide: one prefix class far over the cap
    out["AC3000"] = [_ascii(np.tile([0, 1], 3000))]
    out["unit997x64"] = [np.tile(R(997), 64)]
    out["tails"] = [np.concatenate([_ascii(np.full(40, 3)), R(3000), _ascii(np.zeros(40))])]      # padded tail keys tie on both strands
    c = R(20000)
    out["twice20k"] = [c, c.copy()]                          # two identical contigs
    h = R(2500)
    out["selfrc5k"] = [np.concatenate([h, synth.revcomp(h)])]   # equal to its own reverse complement
    return out


SHAPES = _shapes()
