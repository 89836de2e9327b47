"""ctypes binding of libgsa_hip.so (include/gsa_hip.h) for tests and bench.py.

This is plumbing only: it fills `gsa_index_view` from numpy arrays and calls the
C ABI.  There is no CPU path: if the library or a GPU is missing, loading /
`Aligner()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libgsa_hip.so")

EXPORTS = [
    "gsa_default_params", "gsa_create", "gsa_create_opts", "gsa_reserve_index", "gsa_release_reserved", "gsa_clone", "gsa_clone_to_device", "gsa_host_alloc", "gsa_host_free", "gsa_destroy", "gsa_set_params", "gsa_last_error", "gsa_align_contig", "gsa_align_many", "gsa_align_bundle",
    "gsa_align_contig_device", "gsa_set_query_device", "gsa_device_alloc", "gsa_device_free", "gsa_device_upload", "gsa_get_seed_stats", "gsa_get_dp_stats", "gsa_get_dp_band_stats", "gsa_get_launch_counters", "gsa_hit_buffers", "gsa_seed_chunks", "gsa_hit_count", "gsa_export_hits", "gsa_import_hits", "gsa_finish_contig",
    "gsa_set_query", "gsa_rewind", "gsa_run_to", "gsa_seed_count", "gsa_get_seeds", "gsa_group_count", "gsa_get_groups", "gsa_get_blocks",
    "gsa_bwt_search_batch", "gsa_ksw2_batch", "gsa_gap_similarity_batch", "gsa_get_counters", "gsa_get_timings", "gsa_set_profiling", "gsa_bind_host_thread",
    "gsa_prefetch_contig", "gsa_prefetch_bundle", "gsa_cancel_prefetch", "gsa_get_wall_sums", "gsa_get_alloc_stats", "gsa_debug_buffers", "gsa_set_option", "gsa_host_register", "gsa_host_unregister",
    "gsa_call_variants", "gsa_align_many_variants", "gsa_get_variant_timing",
    "gsa_block_cigars", "gsa_get_cigar_timing", "gsa_align_many_ex",
    "gsa_block_cs", "gsa_get_cs_timing", "gsa_extras_cs",
    "gsa_lift_set", "gsa_lift", "gsa_get_lift_timing", "gsa_extras_lift",
    "gsa_track_set", "gsa_ref_track", "gsa_get_track_timing", "gsa_extras_track",
    "gsa_block_segs", "gsa_get_seg_timing", "gsa_extras_segs",
    "gsa_proj_open", "gsa_proj_close", "gsa_proj_clear", "gsa_project", "gsa_proj_fetch", "gsa_proj_merge", "gsa_get_proj_timing",
    "gsa_regions_set", "gsa_lift_regions", "gsa_get_region_timing", "gsa_extras_regions",
    "gsa_qtrack_set", "gsa_query_track", "gsa_get_qtrack_timing", "gsa_extras_qtrack",
    "gsa_index_sizes", "gsa_build_index", "gsa_get_index_build_stats",
    "gsa_create_from_pac", "gsa_export_index_table",
    "gsa_build_index_opts", "gsa_get_index_build_stats2", "gsa_set_index_build_caps", "gsa_plan_index_batches",
]


class IndexView(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("bwt", C.POINTER(C.c_uint32)), ("bwt_words", C.c_uint64),
                ("sa", C.POINTER(C.c_uint64)), ("n_sa", C.c_uint64), ("ref", C.c_char_p), ("G", C.c_int64),
                ("chr_len", C.POINTER(C.c_int32)), ("n_chr", C.c_int32)]


class Params(C.Structure):
    _fields_ = [("min_seed_len", C.c_int32), ("max_indel", C.c_int32), ("min_block_score", C.c_int32), ("min_aln_len", C.c_int32),
                ("min_identity", C.c_int32), ("sensitive", C.c_int32), ("one_on_one", C.c_int32)]


class Seed(C.Structure):
    _fields_ = [("qpos", C.c_int32), ("len", C.c_int32), ("rpos", C.c_int64)]


class Frag(C.Structure):
    _fields_ = [("bseed", C.c_int32), ("qpos", C.c_int32), ("qlen", C.c_int32), ("rlen", C.c_int32), ("rpos", C.c_int64),
                ("aln_off", C.c_int64), ("aln_len", C.c_int32), ("_pad", C.c_int32)]


class Block(C.Structure):
    _fields_ = [("score", C.c_int32), ("aln_len", C.c_int32), ("bdup", C.c_int32), ("n_frag", C.c_int32), ("frag_off", C.c_int64),
                ("bdir", C.c_int32), ("gpos", C.c_int32), ("chr", C.c_int32), ("_pad", C.c_int32)]


class Rec(C.Structure):
    """gsa_rec, 16 bytes: seed {qpos >= 0, len, rpos} or gap {-1 - qlen, rlen, aln_len, aln_off} (include/gsa_hip.h)."""
    _fields_ = [("w0", C.c_int32), ("w1", C.c_int32), ("w2", C.c_int32), ("w3", C.c_uint32)]


class Result(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_frags", C.c_int64), ("n_aln", C.c_int64), ("blocks", C.POINTER(Block)),
                ("recs", C.POINTER(Rec)), ("aln1", C.POINTER(C.c_char)), ("aln2", C.POINTER(C.c_char))]


class Variant(C.Structure):
    """gsa_variant, 32 bytes (include/gsa_hip.h): kind 0 substitution, 1 / 2 insertion / deletion record, 3 / 4 insertion / deletion inside an aligned gap."""
    _fields_ = [("rpos", C.c_int64), ("qpos", C.c_int32), ("len", C.c_int32), ("chr", C.c_int32), ("pos", C.c_int32), ("kind", C.c_int32), ("block", C.c_int32)]


class Variants(C.Structure):
    _fields_ = [("n", C.c_int64), ("v", C.POINTER(Variant)), ("n_snv", C.c_int64), ("n_ins", C.c_int64), ("n_del", C.c_int64)]


VARIANT_DT = np.dtype([("rpos", "<i8"), ("qpos", "<i4"), ("len", "<i4"), ("chr", "<i4"), ("pos", "<i4"), ("kind", "<i4"), ("block", "<i4")])
VCF_TYPE = ("SUBSTITUTE", "INSERT", "DELETE", "INSERT", "DELETE")      # by gsa_variant::kind


def variants_array(var: "Variants"):
    """gsa_variants -> (VARIANT_DT array (a copy), (n_snv, n_ins, n_del))."""
    n = int(var.n)
    V = np.ctypeslib.as_array(C.cast(var.v, C.POINTER(C.c_uint8)), shape=(n * VARIANT_DT.itemsize,)).view(VARIANT_DT).copy() if n else np.zeros(0, VARIANT_DT)
    return V, (int(var.n_snv), int(var.n_ins), int(var.n_del))


def variant_alleles(V: np.ndarray, ref, query) -> list:
    """[(REF, ALT)] as bytes for the records V: the numpy form of gsa_variant_alleles (include/gsa_hip.h).  ref = RefSequence (2G bytes), query = the contig."""
    ref = ref.tobytes() if isinstance(ref, np.ndarray) else bytes(ref)
    query = query.tobytes() if isinstance(query, np.ndarray) else bytes(query)
    out = []
    for v in V:
        r, q, n, k = int(v["rpos"]), int(v["qpos"]), int(v["len"]) + 1, int(v["kind"])
        if k == 1:
            out.append((ref[r:r + 1], query[q:q + n]))
        elif k == 2:
            out.append((ref[r:r + n], query[q:q + 1]))
        elif k == 3:
            out.append((query[q:q + 1], query[q:q + n]))
        elif k == 4:
            out.append((ref[r:r + n], ref[r:r + 1]))
        else:
            out.append((ref[r:r + 1], query[q:q + 1]))
    return out


class BlockCigar(C.Structure):
    """gsa_block_cigar, 32 bytes (include/gsa_hip.h): where a block's ops lie and its columns per class."""
    _fields_ = [("cig_off", C.c_int64), ("n_cig", C.c_int32), ("n_eq", C.c_int32), ("n_x", C.c_int32), ("n_ins", C.c_int32), ("n_del", C.c_int32), ("_pad", C.c_int32)]


class Cigars(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_ops", C.c_int64), ("blk", C.POINTER(BlockCigar)), ("ops", C.POINTER(C.c_uint32))]


class Extras(C.Structure):
    _fields_ = [("var", C.POINTER(Variants)), ("cig", C.POINTER(Cigars))]


class CsBlock(C.Structure):
    """gsa_cs_block, 16 bytes (include/gsa_hip.h): where a block's cs string lies and its length."""
    _fields_ = [("cs_off", C.c_int64), ("n_cs", C.c_int32), ("_pad", C.c_int32)]


class Cs(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_bytes", C.c_int64), ("blk", C.POINTER(CsBlock)), ("cs", C.POINTER(C.c_char))]


class LiftHit(C.Structure):
    """gsa_lift_hit, 16 bytes (include/gsa_hip.h): where input position idx lies on the query contig."""
    _fields_ = [("idx", C.c_int32), ("qpos", C.c_int32), ("block", C.c_int32), ("cls", C.c_uint8), ("rev", C.c_uint8), ("n_cover", C.c_uint16)]


class Lifts(C.Structure):
    _fields_ = [("n_hits", C.c_int64), ("hits", C.POINTER(LiftHit))]


class RegionHit(C.Structure):
    """gsa_region_hit, 48 bytes (include/gsa_hip.h): where input region idx lies on the query contig and how its columns are classed."""
    _fields_ = [("idx", C.c_int32), ("block", C.c_int32), ("off_lo", C.c_int32), ("off_hi", C.c_int32), ("q_lo", C.c_int32), ("q_hi", C.c_int32),
                ("n_eq", C.c_uint32), ("n_x", C.c_uint32), ("n_del", C.c_uint32), ("n_ins", C.c_uint32),
                ("rev", C.c_uint8), ("_pad0", C.c_uint8), ("n_cover", C.c_uint16), ("_pad1", C.c_int32)]


class RegionLifts(C.Structure):
    _fields_ = [("n_hits", C.c_int64), ("hits", C.POINTER(RegionHit))]


class TrackWin(C.Structure):
    """gsa_track_win, 32 bytes (include/gsa_hip.h): one window of a reference sequence and what the counted blocks put into it."""
    _fields_ = [("chr", C.c_int32), ("start", C.c_int32), ("len", C.c_int32), ("n_cov", C.c_uint32), ("n_eq", C.c_uint32), ("n_x", C.c_uint32), ("n_del", C.c_uint32), ("n_ins", C.c_uint32)]


class Tracks(C.Structure):
    _fields_ = [("n_win", C.c_int64), ("win", C.POINTER(TrackWin))]


class QTrackWin(C.Structure):
    """gsa_qtrack_win, 32 bytes (include/gsa_hip.h): one window of the query contig and what the counted blocks put into it."""
    _fields_ = [("start", C.c_int32), ("len", C.c_int32), ("n_cov", C.c_uint32), ("n_multi", C.c_uint32), ("n_eq", C.c_uint32), ("n_x", C.c_uint32), ("n_ins", C.c_uint32), ("n_del", C.c_uint32)]


class QTracks(C.Structure):
    _fields_ = [("n_win", C.c_int64), ("win", C.POINTER(QTrackWin))]


class Seg(C.Structure):
    """gsa_seg, 12 bytes (include/gsa_hip.h): one data line of a chain -- an aligned segment and the gap behind it in output order."""
    _fields_ = [("size", C.c_int32), ("dt", C.c_int32), ("dq", C.c_int32)]


class SegBlock(C.Structure):
    """gsa_seg_block, 16 bytes: where a block's triples lie and how many there are."""
    _fields_ = [("seg_off", C.c_int64), ("n_seg", C.c_int32), ("_pad", C.c_int32)]


class Segs(C.Structure):
    _fields_ = [("n_blocks", C.c_int32), ("n_segs", C.c_int64), ("blk", C.POINTER(SegBlock)), ("seg", C.POINTER(Seg))]


SEG_DT = np.dtype([("size", "<i4"), ("dt", "<i4"), ("dq", "<i4")])
SEG_BLOCK_DT = np.dtype([("seg_off", "<i8"), ("n_seg", "<i4"), ("_pad", "<i4")])
TRACK_WIN_DT = np.dtype([("chr", "<i4"), ("start", "<i4"), ("len", "<i4"), ("n_cov", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_del", "<u4"), ("n_ins", "<u4")])
QTRACK_WIN_DT = np.dtype([("start", "<i4"), ("len", "<i4"), ("n_cov", "<u4"), ("n_multi", "<u4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_ins", "<u4"), ("n_del", "<u4")])
LIFT_HIT_DT = np.dtype([("idx", "<i4"), ("qpos", "<i4"), ("block", "<i4"), ("cls", "u1"), ("rev", "u1"), ("n_cover", "<u2")])
REGION_HIT_DT = np.dtype([("idx", "<i4"), ("block", "<i4"), ("off_lo", "<i4"), ("off_hi", "<i4"), ("q_lo", "<i4"), ("q_hi", "<i4"), ("n_eq", "<u4"), ("n_x", "<u4"), ("n_del", "<u4"), ("n_ins", "<u4"),
                          ("rev", "u1"), ("_pad0", "u1"), ("n_cover", "<u2"), ("_pad1", "<i4")])
BLOCK_CS_DT = np.dtype([("cs_off", "<i8"), ("n_cs", "<i4"), ("_pad", "<i4")])
BLOCK_CIGAR_DT = np.dtype([("cig_off", "<i8"), ("n_cig", "<i4"), ("n_eq", "<i4"), ("n_x", "<i4"), ("n_ins", "<i4"), ("n_del", "<i4"), ("_pad", "<i4")])
CIGAR_LETTERS = "MIDNSHP=X"      # by BAM op code; the library writes I (1), D (2), = (7) and X (8)
WANT_VARIANTS, WANT_CIGARS, WANT_CS, WANT_LIFT, WANT_TRACK, WANT_SEGS, WANT_PROJ = 1, 2, 4, 16, 32, 64, 128
WANT_REGIONS = 256
WANT_QTRACK = 512
PROJ_NO_DUP = 1
PROJ_LETTERS = "nACGTN-"         # by the low three bits of an accumulator word (0: uncovered)


class ProjStat(C.Structure):
    """gsa_proj_stat, 16 bytes (include/gsa_hip.h): blocks painted, words offered."""
    _fields_ = [("n_blocks", C.c_int32), ("_pad", C.c_int32), ("n_cols", C.c_int64)]


def lifts_array(l: "Lifts"):
    """gsa_lifts -> LIFT_HIT_DT array (a copy)."""
    n = int(l.n_hits)
    return np.ctypeslib.as_array(C.cast(l.hits, C.POINTER(C.c_uint8)), shape=(n * LIFT_HIT_DT.itemsize,)).view(LIFT_HIT_DT).copy() if n else np.zeros(0, LIFT_HIT_DT)


def regions_array(l: "RegionLifts"):
    """gsa_region_lifts -> REGION_HIT_DT array (a copy)."""
    n = int(l.n_hits)
    return np.ctypeslib.as_array(C.cast(l.hits, C.POINTER(C.c_uint8)), shape=(n * REGION_HIT_DT.itemsize,)).view(REGION_HIT_DT).copy() if n else np.zeros(0, REGION_HIT_DT)


def tracks_array(t: "Tracks"):
    """gsa_tracks -> TRACK_WIN_DT array (a copy)."""
    n = int(t.n_win)
    return np.ctypeslib.as_array(C.cast(t.win, C.POINTER(C.c_uint8)), shape=(n * TRACK_WIN_DT.itemsize,)).view(TRACK_WIN_DT).copy() if n else np.zeros(0, TRACK_WIN_DT)


def qtracks_array(t: "QTracks"):
    """gsa_qtracks -> QTRACK_WIN_DT array (a copy)."""
    n = int(t.n_win)
    return np.ctypeslib.as_array(C.cast(t.win, C.POINTER(C.c_uint8)), shape=(n * QTRACK_WIN_DT.itemsize,)).view(QTRACK_WIN_DT).copy() if n else np.zeros(0, QTRACK_WIN_DT)


def segs_arrays(sg: "Segs"):
    """gsa_segs -> (SEG_BLOCK_DT array, SEG_DT array), both copies; block b's triples are seg[seg_off : seg_off + n_seg]."""
    nb, n = int(sg.n_blocks), int(sg.n_segs)
    blk = np.ctypeslib.as_array(C.cast(sg.blk, C.POINTER(C.c_uint8)), shape=(nb * SEG_BLOCK_DT.itemsize,)).view(SEG_BLOCK_DT).copy() if nb else np.zeros(0, SEG_BLOCK_DT)
    seg = np.ctypeslib.as_array(C.cast(sg.seg, C.POINTER(C.c_uint8)), shape=(n * SEG_DT.itemsize,)).view(SEG_DT).copy() if n else np.zeros(0, SEG_DT)
    return blk, seg


def cigars_arrays(cig: "Cigars"):
    """gsa_cigars -> (BLOCK_CIGAR_DT array, uint32 ops), both copies."""
    nb, no = int(cig.n_blocks), int(cig.n_ops)
    blk = np.ctypeslib.as_array(C.cast(cig.blk, C.POINTER(C.c_uint8)), shape=(nb * BLOCK_CIGAR_DT.itemsize,)).view(BLOCK_CIGAR_DT).copy() if nb else np.zeros(0, BLOCK_CIGAR_DT)
    ops = np.ctypeslib.as_array(cig.ops, shape=(no,)).copy() if no else np.zeros(0, np.uint32)
    return blk, ops


def cs_arrays(cs: "Cs"):
    """gsa_cs -> (BLOCK_CS_DT array, uint8 bytes), both copies; block b's string is bytes[cs_off : cs_off + n_cs]."""
    nb, n = int(cs.n_blocks), int(cs.n_bytes)
    blk = np.ctypeslib.as_array(C.cast(cs.blk, C.POINTER(C.c_uint8)), shape=(nb * BLOCK_CS_DT.itemsize,)).view(BLOCK_CS_DT).copy() if nb else np.zeros(0, BLOCK_CS_DT)
    by = np.ctypeslib.as_array(C.cast(cs.cs, C.POINTER(C.c_uint8)), shape=(n,)).copy() if n else np.zeros(0, np.uint8)
    return blk, by


def cs_of_ops_length(ops) -> int:
    """bytes of the cs string the ops imply: ':' and the decimal length for '=', 3 per 'X' column, 1 + the columns for 'I' / 'D'"""
    ops = np.asarray(ops, dtype=np.uint32)
    return int(sum((1 + len(str(int(o) >> 4))) if int(o) & 15 == 7 else (3 * (int(o) >> 4) if int(o) & 15 == 8 else 1 + (int(o) >> 4)) for o in ops))


def cigar_string(ops) -> str:
    """ops (len << 4 | code) as PAF's cg string: the numpy form of gsa_cigar_string (include/gsa_hip.h)."""
    ops = np.asarray(ops, dtype=np.uint32)
    return "".join(f"{int(o) >> 4}{CIGAR_LETTERS[int(o) & 15] if int(o) & 15 < len(CIGAR_LETTERS) else '?'}" for o in ops)


FRAG_DT = np.dtype([("bseed", "<i4"), ("qpos", "<i4"), ("qlen", "<i4"), ("rlen", "<i4"), ("rpos", "<i8"), ("aln_off", "<i8"), ("aln_len", "<i4"), ("_pad", "<i4")])
BLOCK_DT = np.dtype([("score", "<i4"), ("aln_len", "<i4"), ("bdup", "<i4"), ("n_frag", "<i4"), ("frag_off", "<i8"), ("bdir", "<i4"), ("gpos", "<i4"), ("chr", "<i4"), ("_pad", "<i4")])
SEED_DT = np.dtype([("qpos", "<i4"), ("len", "<i4"), ("rpos", "<i8")])
REC_DT = np.dtype([("w0", "<i4"), ("w1", "<i4"), ("w2", "<i4"), ("w3", "<u4")])


def expand_recs(recs: np.ndarray) -> np.ndarray:
    """gsa_rec[n] -> gsa_frag[n] (FRAG_DT): numpy form of gsa_expand_frags (include/gsa_hip.h)."""
    n = recs.size
    F = np.zeros(n, FRAG_DT)
    if not n:
        return F
    seed = recs["w0"] >= 0
    rpos = recs.view(np.int64).reshape(-1, 2)[:, 1]
    F["bseed"] = seed
    F["qpos"][seed] = recs["w0"][seed]; F["qlen"][seed] = recs["w1"][seed]; F["rlen"][seed] = recs["w1"][seed]; F["rpos"][seed] = rpos[seed]
    g = np.flatnonzero(~seed)
    if g.size:
        assert g[0] > 0 and seed[g - 1].all(), "a gap record follows a seed record"
        F["qpos"][g] = recs["w0"][g - 1] + recs["w1"][g - 1]; F["rpos"][g] = rpos[g - 1] + recs["w1"][g - 1]
        F["qlen"][g] = -1 - recs["w0"][g]; F["rlen"][g] = recs["w1"][g]; F["aln_len"][g] = recs["w2"][g]; F["aln_off"][g] = recs["w3"][g]
    return F


def pack_recs(F: np.ndarray) -> np.ndarray:
    """gsa_frag[n] -> gsa_rec[n]: the inverse (what the library's last pass does on the device)."""
    R = np.zeros(F.size, REC_DT)
    seed = F["bseed"] != 0
    rpos = R.view(np.int64).reshape(-1, 2)[:, 1]
    R["w0"][seed] = F["qpos"][seed]; R["w1"][seed] = F["qlen"][seed]; rpos[seed] = F["rpos"][seed]
    g = ~seed
    R["w0"][g] = -1 - F["qlen"][g]; R["w1"][g] = F["rlen"][g]; R["w2"][g] = F["aln_len"][g]; R["w3"][g] = F["aln_off"][g].astype(np.uint32)
    return R


def build_library() -> None:
    """hipcc cross-compiles for gfx950 without a GPU (seconds per file once warm)."""
    subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j8", "lib"], check=True, stdout=subprocess.DEVNULL)


def load_library() -> C.CDLL:
    path = os.environ.get("GSA_LIB_PATH") or LIB_PATH          # (GSA_LIB_PATH: an experiment variant of the library, tools only)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` (there is no CPU fallback)")
    lib = C.CDLL(path)
    lib.gsa_create.argtypes = [C.c_int, C.POINTER(IndexView), C.POINTER(Params), C.POINTER(C.c_void_p)]
    lib.gsa_create_opts.argtypes = [C.c_int, C.POINTER(IndexView), C.POINTER(Params), C.c_uint32, C.POINTER(C.c_void_p)]
    lib.gsa_clone.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    lib.gsa_clone_to_device.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.gsa_host_alloc.restype = C.c_void_p
    lib.gsa_host_alloc.argtypes = [C.c_size_t]
    lib.gsa_host_free.argtypes = [C.c_void_p]
    lib.gsa_device_alloc.restype = C.c_void_p
    lib.gsa_device_alloc.argtypes = [C.c_int, C.c_size_t]
    lib.gsa_device_free.argtypes = [C.c_int, C.c_void_p]
    lib.gsa_device_upload.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    lib.gsa_align_contig_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(Result)]
    lib.gsa_set_query_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.gsa_prefetch_contig.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    lib.gsa_cancel_prefetch.argtypes = [C.c_void_p]
    lib.gsa_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.gsa_last_error.restype = C.c_char_p
    lib.gsa_last_error.argtypes = [C.c_void_p]
    lib.gsa_seed_count.restype = C.c_int64
    lib.gsa_hit_count.restype = C.c_int64
    lib.gsa_hit_count.argtypes = [C.c_void_p]
    lib.gsa_export_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.gsa_import_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    for name in ("gsa_destroy", "gsa_set_params", "gsa_align_contig", "gsa_set_query", "gsa_run_to", "gsa_seed_count", "gsa_get_seeds",
                 "gsa_group_count", "gsa_get_groups", "gsa_get_blocks", "gsa_bwt_search_batch", "gsa_ksw2_batch", "gsa_gap_similarity_batch",
                 "gsa_get_counters", "gsa_get_timings", "gsa_set_profiling"):
        fn = getattr(lib, name)
        if fn.argtypes is None:
            fn.argtypes = None
    return lib


def index_sizes(G: int):
    """gsa_index_sizes: (bwt_words, n_sa) of the index of a reference of G forward bases -- arithmetic, no device."""
    lib = load_library()
    lib.gsa_index_sizes.argtypes = [C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    bw, ns = C.c_uint64(), C.c_uint64()
    rc = lib.gsa_index_sizes(int(G), C.byref(bw), C.byref(ns))
    if rc != 0:
        raise GsaError(f"gsa_index_sizes -> {rc}: {lib.gsa_last_error(None).decode()}")
    return int(bw.value), int(ns.value)


BUILD_INDEX_ARGTYPES = [C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]


BUILD_INDEX_OPTS_ARGTYPES = [C.c_int, C.c_void_p, C.c_int64, C.c_uint32, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p]
BUILD_AUTO, BUILD_WIDE = 0, 1      # GSA_BUILD_* (include/gsa_hip.h)
CREATE_SORT_WIDE = 2               # GSA_CREATE_SORT_WIDE


def build_index_arrays(pac, G: int, device: int = 0, wide: bool = False, batch_cap: int = 0, occ_segment: int = 0):
    """gsa_build_index_opts: the .pac bytes of G forward bases -> (hdr uint64[5] = [primary, L2[1..4]], bwt uint32[], sa uint64[]), the arrays of
    indexio.BwaIndex, suffix-sorted on the GPU.  wide: the batched 64-bit sorter at any size (GSA_BUILD_WIDE; otherwise it runs over 1 073 741 822 bases only),
    batch_cap / occ_segment: its batch size and Occ scan segment (0: the defaults).  Raises GsaError (.code = the library's error code) when the library refuses."""
    lib = load_library()
    lib.gsa_build_index_opts.argtypes = BUILD_INDEX_OPTS_ARGTYPES
    pac = np.ascontiguousarray(pac, dtype=np.uint8)
    if G <= 0 or pac.size < (G + 3) // 4:
        raise ValueError("pac holds fewer than G bases")
    bw, ns = index_sizes(G)
    bwt = np.zeros(bw, np.uint32); sa = np.zeros(ns, np.uint64)
    primary = C.c_uint64(); L2 = (C.c_uint64 * 5)()
    rc = lib.gsa_build_index_opts(int(device), C.c_void_p(pac.ctypes.data), int(G), BUILD_WIDE if wide else BUILD_AUTO, int(batch_cap), int(occ_segment),
                                  C.byref(primary), L2, C.c_void_p(bwt.ctypes.data), C.c_void_p(sa.ctypes.data))
    if rc != 0:
        e = GsaError(f"gsa_build_index -> {rc}: {lib.gsa_last_error(None).decode()}"); e.code = rc
        raise e
    return np.array([primary.value, L2[1], L2[2], L2[3], L2[4]], dtype=np.uint64), bwt, sa


def index_build_stats():
    """gsa_get_index_build_stats: (device ms, doubling rounds) of the calling thread's last gsa_build_index."""
    lib = load_library()
    ms, rounds = C.c_double(), C.c_int32()
    lib.gsa_get_index_build_stats.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int32)]
    lib.gsa_get_index_build_stats(C.byref(ms), C.byref(rounds))
    return float(ms.value), int(rounds.value)


def index_build_stats2():
    """gsa_get_index_build_stats2: (batches that held a suffix, peak device bytes, suffixes still tied after the first pass) of the calling thread's last build;
    (0, 0, 0) after the narrow sorter."""
    lib = load_library()
    batches, peak, active = C.c_int64(), C.c_uint64(), C.c_int64()
    lib.gsa_get_index_build_stats2.argtypes = [C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)]
    lib.gsa_get_index_build_stats2(C.byref(batches), C.byref(peak), C.byref(active))
    return int(batches.value), int(peak.value), int(active.value)


def set_index_build_caps(batch_cap: int = 0, occ_segment: int = 0, active_cap: int = 0) -> None:
    """gsa_set_index_build_caps (test support, process-wide; 0: the defaults): the wide builder's batch cap and Occ segment inside
    Aligner.from_reference(sort_wide=True), and a limit on the entries of its list of tied suffixes in every wide build."""
    lib = load_library()
    lib.gsa_set_index_build_caps.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    if lib.gsa_set_index_build_caps(int(batch_cap), int(occ_segment), int(active_cap)) != 0:
        raise GsaError(f"gsa_set_index_build_caps: {lib.gsa_last_error(None).decode()}")


def plan_index_batches(hist, batch_cap: int):
    """gsa_plan_index_batches: (first[n_batches + 1], base[n_batches + 1]) of the wide builder's batches for the class counts `hist`; GsaError (.code) when refused."""
    lib = load_library()
    lib.gsa_plan_index_batches.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    first = np.zeros(hist.size + 1, np.int64); base = np.zeros(hist.size + 1, np.uint64); nb = C.c_int64()
    rc = lib.gsa_plan_index_batches(C.c_void_p(hist.ctypes.data), hist.size, int(batch_cap), hist.size, C.c_void_p(first.ctypes.data), C.c_void_p(base.ctypes.data), C.byref(nb))
    if rc != 0:
        e = GsaError(f"gsa_plan_index_batches -> {rc}: {lib.gsa_last_error(None).decode()}"); e.code = rc
        raise e
    return first[:nb.value + 1].copy(), base[:nb.value + 1].copy()


def bind_host_thread(device: int = 0) -> None:
    """gsa_bind_host_thread: the calling thread moves to the CPUs next to `device` (threads started later inherit that)."""
    lib = load_library()
    lib.gsa_bind_host_thread.argtypes = [C.c_int]
    lib.gsa_bind_host_thread(int(device))


RESULT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(Result))
RESULT_VAR_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(Result), C.POINTER(Variants))
RESULT_EX_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(Result), C.POINTER(Extras))


class DeviceContig:
    """A query contig resident in device memory (gsa_device_alloc + gsa_device_upload): what gsa_align_contig_device takes."""

    def __init__(self, lib, device: int, seq: np.ndarray):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self.lib, self.device, self.size = lib, int(device), int(seq.size)
        self.ptr = lib.gsa_device_alloc(self.device, self.size)
        if not self.ptr:
            raise GsaError("gsa_device_alloc failed")
        if lib.gsa_device_upload(self.device, C.c_void_p(self.ptr), C.c_void_p(seq.ctypes.data), self.size) != 0:
            raise GsaError("gsa_device_upload failed")

    def free(self):
        if self.ptr:
            self.lib.gsa_device_free(self.device, C.c_void_p(self.ptr)); self.ptr = None


def align_many(aligners, contigs, on_result=None, in_order: bool = False, bundle: bool = True, prefetch: bool = True, variants: bool = False, cigars: bool = False, cs: bool = False, lift: bool = False, track: bool = False, segs: bool = False, proj: bool = False, regions: bool = False, qtrack: bool = False) -> None:
    """gsa_align_many: `contigs` (uint8 arrays, or DeviceContig objects -- all of one kind) on the given contexts, one host
    thread per context inside the library.  on_result(contig_index, Result) runs on the worker threads (the Result is valid
    during the call only).  in_order: hand the contigs out as listed (GSA_MANY_IN_ORDER) instead of longest first.
    bundle=False: GSA_MANY_NO_BUNDLE (every contig in a pass of its own; by default short contigs share passes).
    prefetch=False: GSA_MANY_NO_PREFETCH (a contig is uploaded when its turn comes; by default a context uploads its next contig
    while it aligns the current one).
    variants=True: gsa_align_many_variants -- the worker runs the variant pass first and on_result(contig_index, Result, Variants) gets its records too
    (variants_array copies them out).
    cigars=True: gsa_align_many_ex with GSA_WANT_CIGARS (and GSA_WANT_VARIANTS when variants=True) -- on_result(contig_index, Result, Variants or None, Cigars)
    (cigars_arrays copies them out).
    cs=True: GSA_WANT_CS as well (it implies the CIGARs) -- on_result gets a fifth argument, the contig's Cs (gsa_extras_cs; cs_arrays copies it out).
    lift=True: gsa_align_many_ex with GSA_WANT_LIFT (every aligner holds positions: lift_set) -- on_result(contig_index, Result, Variants or None, Cigars or None[, Cs]) gets
    one more argument, the contig's Lifts (gsa_extras_lift; lifts_array copies it out).
    track=True: gsa_align_many_ex with GSA_WANT_TRACK (every aligner holds a window: track_set) -- on_result gets one more argument behind all of those, the contig's
    Tracks (gsa_extras_track; tracks_array copies it out).
    segs=True: gsa_align_many_ex with GSA_WANT_SEGS (it implies the CIGARs) -- on_result gets one more argument behind all of those, the contig's Segs (gsa_extras_segs;
    segs_arrays copies it out).
    proj=True: gsa_align_many_ex with GSA_WANT_PROJ (every aligner holds an accumulator: proj_open) -- the worker paints every contig behind the other passes; on_result
    gets nothing more.  Some aligners without an accumulator: -4; none with one: -1, like an unknown bit.
    regions=True: gsa_align_many_ex with GSA_WANT_REGIONS (every aligner holds regions: regions_set) -- on_result gets one more argument behind all of those, the contig's
    RegionLifts (gsa_extras_regions; regions_array copies it out).
    qtrack=True: gsa_align_many_ex with GSA_WANT_QTRACK (every aligner holds a query-side window: qtrack_set) -- on_result gets one more argument behind all of those,
    the contig's QTracks (gsa_extras_qtrack; qtracks_array copies it out)."""
    lib = aligners[0].lib
    n = len(contigs)
    ctxs = (C.c_void_p * len(aligners))(*[a.ctx for a in aligners])
    on_dev = n > 0 and isinstance(contigs[0], DeviceContig)
    qs = (C.c_char_p * n)(*[C.cast(c.ptr if on_dev else c.ctypes.data, C.c_char_p) for c in contigs])
    ql = (C.c_int32 * n)(*[int(c.size) for c in contigs])
    flags = (1 if in_order else 0) | (2 if on_dev else 0) | (0 if bundle else 8) | (0 if prefetch else 16)
    if cigars or cs or lift or track or segs or proj or regions or qtrack:
        lib.gsa_extras_cs.argtypes = [C.POINTER(Extras), C.POINTER(Cs)]
        lib.gsa_extras_lift.argtypes = [C.POINTER(Extras), C.POINTER(Lifts)]
        lib.gsa_extras_track.argtypes = [C.POINTER(Extras), C.POINTER(Tracks)]
        lib.gsa_extras_segs.argtypes = [C.POINTER(Extras), C.POINTER(Segs)]
        lib.gsa_extras_regions.argtypes = [C.POINTER(Extras), C.POINTER(RegionLifts)]
        lib.gsa_extras_qtrack.argtypes = [C.POINTER(Extras), C.POINTER(QTracks)]

        def ex_cb(user, ci, res, ex):
            e = ex.contents
            args = (ci, res.contents, e.var.contents if e.var else None, e.cig.contents if e.cig else None)
            if cs:
                s = Cs()
                rc_cs = lib.gsa_extras_cs(ex, C.byref(s))
                if rc_cs != 0:
                    return int(rc_cs)
                args += (s,)
            if lift:
                lf = Lifts()
                rc_l = lib.gsa_extras_lift(ex, C.byref(lf))
                if rc_l != 0:
                    return int(rc_l)
                args += (lf,)
            if track:
                tk = Tracks()
                rc_t = lib.gsa_extras_track(ex, C.byref(tk))
                if rc_t != 0:
                    return int(rc_t)
                args += (tk,)
            if segs:
                sg = Segs()
                rc_g = lib.gsa_extras_segs(ex, C.byref(sg))
                if rc_g != 0:
                    return int(rc_g)
                args += (sg,)
            if regions:
                rg = RegionLifts()
                rc_r = lib.gsa_extras_regions(ex, C.byref(rg))
                if rc_r != 0:
                    return int(rc_r)
                args += (rg,)
            if qtrack:
                qt = QTracks()
                rc_q = lib.gsa_extras_qtrack(ex, C.byref(qt))
                if rc_q != 0:
                    return int(rc_q)
                args += (qt,)
            return int((on_result(*args) if on_result else 0) or 0)
        cbx = RESULT_EX_FN(ex_cb)
        lib.gsa_align_many_ex.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.c_uint32, RESULT_EX_FN, C.c_void_p]
        rc = lib.gsa_align_many_ex(ctxs, len(aligners), qs, ql, n, flags, (WANT_CIGARS if cigars or cs else 0) | (WANT_CS if cs else 0) | (WANT_VARIANTS if variants else 0) | (WANT_LIFT if lift else 0) | (WANT_TRACK if track else 0) | (WANT_SEGS if segs else 0) | (WANT_PROJ if proj else 0) | (WANT_REGIONS if regions else 0) | (WANT_QTRACK if qtrack else 0), cbx, None)
    elif variants:
        cbv = RESULT_VAR_FN(lambda user, ci, res, var: int((on_result(ci, res.contents, var.contents) if on_result else 0) or 0))
        lib.gsa_align_many_variants.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, RESULT_VAR_FN, C.c_void_p]
        rc = lib.gsa_align_many_variants(ctxs, len(aligners), qs, ql, n, flags, cbv, None)
    else:
        cb = RESULT_FN((lambda user, ci, res: int(on_result(ci, res.contents) or 0)) if on_result else 0)
        lib.gsa_align_many.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, RESULT_FN, C.c_void_p]
        rc = lib.gsa_align_many(ctxs, len(aligners), qs, ql, n, flags, cb, None)
    if rc != 0:
        msgs = [lib.gsa_last_error(a.ctx).decode() for a in aligners]
        raise GsaError(f"gsa_align_many{'_ex' if cigars or cs or lift or track or segs or proj or regions or qtrack else '_variants' if variants else ''} -> {rc}: {'; '.join(m for m in msgs if m)}")


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def result_as_dump(r: dict, with_aln: bool = False) -> dict:
    """A result dict (Aligner._result: blocks / frags / aln1 / aln2) in the shape of oracle_py._StageReader.blocks(): records
    gathered in block order."""
    B, F = r["blocks"], r["frags"]
    idx = np.concatenate([np.arange(o, o + n) for o, n in zip(B["frag_off"], B["n_frag"])]) if B.size else np.zeros(0, np.int64)
    Fo = F[idx] if idx.size else np.zeros(0, FRAG_DT)
    out = {"b_score": B["score"].copy(), "b_aln_len": B["aln_len"].copy(), "b_bdup": B["bdup"].copy(), "b_nfrag": B["n_frag"].copy(),
           "b_bdir": B["bdir"].copy(), "b_gpos": B["gpos"].copy(), "b_chr": B["chr"].copy(),
           "f_bseed": Fo["bseed"].copy(), "f_qpos": Fo["qpos"].copy(), "f_qlen": Fo["qlen"].copy(), "f_rlen": Fo["rlen"].copy(),
           "f_alnlen": Fo["aln_len"].copy(), "f_rpos": Fo["rpos"].copy()}
    if with_aln:
        segs1 = [r["aln1"][o:o + n] for o, n in zip(Fo["aln_off"], Fo["aln_len"]) if n]
        segs2 = [r["aln2"][o:o + n] for o, n in zip(Fo["aln_off"], Fo["aln_len"]) if n]
        out["aln1"] = np.concatenate(segs1) if segs1 else np.zeros(0, np.uint8)
        out["aln2"] = np.concatenate(segs2) if segs2 else np.zeros(0, np.uint8)
    return out


class GsaError(RuntimeError):
    pass


class Aligner:
    """One gsa_ctx on one GPU."""

    # gsa_set_option names a test / tool may also give through the environment (GSA_<NAME>): the LIBRARY reads no environment variable,
    # this Python layer does and passes the values on
    ENV_OPTIONS = ("split_min", "bundle_contig", "bundle_cap", "seed_budget", "dp_lane", "seed_mode", "pd_bitmap", "walk_chain_min", "pd_two_level_min", "pres_from_kmer", "pd_bytes", "sweep_shape", "dp_side", "dp_pair", "dp_band", "dp_band_margin", "dp_safe", "dp_fake_timeout")

    def _options_from_env(self):
        for name in self.ENV_OPTIONS:
            v = os.environ.get("GSA_" + name.upper())
            if v is not None and v != "":
                self.set_option(name, {"sweep": 0, "spec": 1, "search": 2}.get(v, v) if name == "seed_mode" else v)
        if os.environ.get("GSA_NO_PDBITMAP"):
            self.set_option("pd_bitmap", 0)

    def set_option(self, name: str, value) -> None:
        self._ck(self.lib.gsa_set_option(self.ctx, name.encode(), C.c_int64(int(value))))

    def __init__(self, idx, device: int = 0, wide: bool = False, kmer_k: int = 0, pac=None, _clone_of=None, _copy_to=None, **params):
        self.lib = load_library()
        self.idx = idx
        self._pinned = []
        self._devbufs = []
        if _clone_of is not None and _copy_to is not None:
            self.ctx = C.c_void_p()
            rc = self.lib.gsa_clone_to_device(_clone_of.ctx, int(_copy_to), C.byref(self.ctx))
            if rc != 0:
                raise GsaError(f"gsa_clone_to_device -> {rc}: {self.lib.gsa_last_error(None).decode()}")
            self._options_from_env()          # (independent of its parent: owns its copy of the index)
            return
        if _clone_of is not None:
            self.ctx = C.c_void_p()
            rc = self.lib.gsa_clone(_clone_of.ctx, C.byref(self.ctx))
            if rc != 0:
                raise GsaError(f"gsa_clone -> {rc}: {self.lib.gsa_last_error(None).decode()}")
            self._parent = _clone_of        # keeps the index owner alive
            self._options_from_env()
            return
        self._ref = np.ascontiguousarray(idx.ref)
        v = IndexView()
        v.primary = int(idx.hdr[0])
        v.L2[0] = 0
        for i in range(1, 5):
            v.L2[i] = int(idx.hdr[i])
        v.bwt = _p(idx.bwt, C.c_uint32); v.bwt_words = idx.bwt.size
        v.sa = _p(idx.sa, C.c_uint64); v.n_sa = idx.sa.size
        v.ref = self._ref.ctypes.data_as(C.c_char_p); v.G = idx.G
        if pac is not None:      # GSA_CREATE_REF_PAC: the bytes of the .pac file instead of RefSequence -- the device unpacks the text itself
            self._pac = np.ascontiguousarray(pac, dtype=np.uint8)
            assert self._pac.size >= (idx.G + 3) // 4
            v.ref = self._pac.ctypes.data_as(C.c_char_p)
        v.chr_len = _p(idx.chr_len, C.c_int32); v.n_chr = len(idx.chr_len)
        self.ctx = C.c_void_p()
        p = self._params(**params)
        # wide=True (or GSA_FORCE_WIDE=1 in the environment of the test run): GSA_CREATE_WIDE, the >= 2^32-row device layout on any index;
        # kmer_k (or GSA_KMER_K): GSA_CREATE_KMER_K
        wide = wide or os.environ.get("GSA_FORCE_WIDE", "0") not in ("", "0")
        kmer_k = kmer_k or int(os.environ.get("GSA_KMER_K", "0") or 0)
        prio = int(os.environ.get("GSA_PRIO", "0") or 0)          # GSA_CREATE_PRIO (experiments / bench: stream priorities)
        flags = (1 if wide else 0) | ((kmer_k & 15) << 8) | ((prio & 3) << 16) | (4 if pac is not None else 0)
        rc = self.lib.gsa_create_opts(device, C.byref(v), C.byref(p), flags, C.byref(self.ctx))
        if rc != 0:
            e = GsaError(f"gsa_create -> {rc}: {self.lib.gsa_last_error(None).decode()}"); e.code = rc
            raise e
        self._options_from_env()

    @classmethod
    def from_reference(cls, pac, G: int, chr_len, device: int = 0, wide: bool = False, kmer_k: int = 0, sort_wide: bool = False, **params) -> "Aligner":
        """gsa_create_from_pac: a context from the .pac bytes of the G forward bases and the sequence lengths (hostlib.reference_from_fasta gives them) -- the index is
        built in device memory, no index file and no host index array exists (self.idx is None).  Raises GsaError (.code = the library's error code)."""
        self = cls.__new__(cls)
        self.lib = load_library()
        self.idx = None
        self._pinned = []
        self._devbufs = []
        self.lib.gsa_create_from_pac.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.POINTER(Params), C.c_uint32, C.POINTER(C.c_void_p)]
        pac = np.ascontiguousarray(pac, dtype=np.uint8); chr_len = np.ascontiguousarray(chr_len, dtype=np.int32)
        wide = wide or os.environ.get("GSA_FORCE_WIDE", "0") not in ("", "0")
        kmer_k = kmer_k or int(os.environ.get("GSA_KMER_K", "0") or 0)
        prio = int(os.environ.get("GSA_PRIO", "0") or 0)
        flags = (1 if wide else 0) | ((kmer_k & 15) << 8) | ((prio & 3) << 16) | (CREATE_SORT_WIDE if sort_wide else 0)      # (sort_wide: GSA_CREATE_SORT_WIDE, the batched 64-bit sorter; implies wide)
        self.ctx = C.c_void_p()
        p = self._params(**params)
        rc = self.lib.gsa_create_from_pac(int(device), C.c_void_p(pac.ctypes.data), int(G), C.c_void_p(chr_len.ctypes.data), int(chr_len.size), C.byref(p), flags, C.byref(self.ctx))
        if rc != 0:
            e = GsaError(f"gsa_create_from_pac -> {rc}: {self.lib.gsa_last_error(None).decode()}"); e.code = rc
            raise e
        self._options_from_env()
        return self

    TABLES = {"header": 0, "occ": 1, "occ_base": 2, "sa_dense": 3, "sa": 4, "kmer": 5, "kmer_lo": 6, "pres": 7, "ref": 8, "ref2": 9}      # GSA_TABLE_* (include/gsa_hip.h)

    def index_table(self, which) -> np.ndarray:
        """gsa_export_index_table: the raw bytes of one device table of this context (a name of TABLES or its number); an absent table is empty."""
        w = self.TABLES[which] if isinstance(which, str) else int(which)
        self.lib.gsa_export_index_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
        n = C.c_uint64(0)
        self._ck(self.lib.gsa_export_index_table(self.ctx, w, None, 0, C.byref(n)))
        out = np.zeros(int(n.value), np.uint8)
        if out.size:
            self._ck(self.lib.gsa_export_index_table(self.ctx, w, C.c_void_p(out.ctypes.data), out.size, C.byref(n)))
        return out

    def clone(self) -> "Aligner":
        """A further context on the same GPU sharing this one's device index (gsa_clone)."""
        return Aligner(self.idx, _clone_of=self)

    def clone_to_device(self, device: int) -> "Aligner":
        """A context on GPU `device` whose device index is a device-to-device COPY of this one's (gsa_clone_to_device): no upload, no table builds."""
        return Aligner(self.idx, _clone_of=self, _copy_to=device)

    def pinned_copy(self, seq: np.ndarray) -> np.ndarray:
        """seq copied into pinned host memory from gsa_host_alloc (what a FASTA loader of an integrated host reads into)."""
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        p = self.lib.gsa_host_alloc(seq.size + 64)
        if not p:
            raise GsaError("gsa_host_alloc failed")
        self._pinned.append(p)
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(seq.size,))
        buf[:] = seq
        return buf

    def device_copy(self, seq: np.ndarray, device: int = 0) -> DeviceContig:
        """seq uploaded once into device memory (gsa_device_alloc / gsa_device_upload); freed by close()."""
        d = DeviceContig(self.lib, device, seq)
        self._devbufs.append(d)
        return d

    def prefetch_contig(self, seq: np.ndarray):
        """gsa_prefetch_contig: start the upload of the NEXT contig; the following align_contig(seq) -- same buffer -- finds it on the device."""
        self._ck(self.lib.gsa_prefetch_contig(self.ctx, seq.ctypes.data_as(C.c_char_p), C.c_int32(seq.size)))

    def cancel_prefetch(self):
        self._ck(self.lib.gsa_cancel_prefetch(self.ctx))

    def align_contig_device(self, d: DeviceContig) -> dict:
        res = Result()
        self._ck(self.lib.gsa_align_contig_device(self.ctx, C.c_void_p(d.ptr), C.c_int32(d.size), C.byref(res)))
        return self._result(res)

    def seed_stats(self) -> np.ndarray:
        st = np.zeros(8, np.uint64)
        self._ck(self.lib.gsa_get_seed_stats(self.ctx, _p(st, C.c_uint64)))
        return st

    def dp_stats(self) -> np.ndarray:
        """Sums since the context was made: striped DP jobs, of them side by side, lagged launches, side-by-side launches."""
        st = np.zeros(4, np.uint64)
        self._ck(self.lib.gsa_get_dp_stats(self.ctx, _p(st, C.c_uint64)))
        return st

    def dp_band_stats(self) -> np.ndarray:
        """Sums since the context was made: striped DP jobs evaluated inside the diagonal band, of them certified, fallen back to the striped kernel."""
        st = np.zeros(3, np.uint64)
        self._ck(self.lib.gsa_get_dp_band_stats(self.ctx, _p(st, C.c_uint64)))
        return st

    def launch_counters(self) -> np.ndarray:
        """The counters a context never resets: [0] look-back epoch, [1] fused-pass ticket, [2] DP granule epoch, [3] band tag, [4] chain-walk epoch, [5] chain-walk
        ticket, [6] slices of the last sliced chain walk, [7] bytes of the boundary-granule buffer.  Raises GsaError ("ticket drift") if a device ticket word
        differs from the host's value."""
        st = np.zeros(8, np.uint64)
        self._ck(self.lib.gsa_get_launch_counters(self.ctx, _p(st, C.c_uint64)))
        return st

    def _params(self, slen=15, ind=25, clr=200, alen=200, idy=70, sen=0, one=0) -> Params:
        return Params(slen, ind, clr, alen, idy, sen, one)

    def _ck(self, rc):
        if rc != 0:
            raise GsaError(f"libgsa_hip error {rc}: {self.lib.gsa_last_error(self.ctx).decode()}")

    def set_params(self, **params):
        p = self._params(**params)
        self._ck(self.lib.gsa_set_params(self.ctx, C.byref(p)))

    def set_profiling(self, on: bool, count_blocks: bool = False, seed_only: bool = False, variants: bool = False):
        self._ck(self.lib.gsa_set_profiling(self.ctx, (1 if on else 0) | (2 if count_blocks else 0) | (4 if seed_only else 0) | (8 if variants else 0)))

    def set_query(self, seq: np.ndarray):
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self._q = seq
        self._ck(self.lib.gsa_set_query(self.ctx, seq.ctypes.data_as(C.c_char_p), C.c_int32(seq.size)))

    def rewind(self):
        """Stage 0 again with the uploaded contig (no new copy)."""
        self._ck(self.lib.gsa_rewind(self.ctx))

    def run_to(self, stage: int):
        self._ck(self.lib.gsa_run_to(self.ctx, stage))

    def align_contig(self, seq: np.ndarray) -> dict:
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self._q = seq
        res = Result()
        self._ck(self.lib.gsa_align_contig(self.ctx, seq.ctypes.data_as(C.c_char_p), C.c_int32(seq.size), C.byref(res)))
        return self._result(res)

    # ---- one contig seeded by several GPUs (gsa_seed_chunks ... gsa_finish_contig) ----
    def seed_chunks(self, seq: np.ndarray, chunk_beg: int, chunk_end: int) -> int:
        seq = np.ascontiguousarray(seq, dtype=np.uint8)
        self._q = seq
        self._ck(self.lib.gsa_seed_chunks(self.ctx, seq.ctypes.data_as(C.c_char_p), C.c_int32(seq.size), C.c_int32(chunk_beg), C.c_int32(chunk_end)))
        return int(self.lib.gsa_hit_count(self.ctx))

    def hit_count(self) -> int:
        return int(self.lib.gsa_hit_count(self.ctx))

    def export_hits(self, keys_ptr=None, vals_ptr=None):
        """Hits of this context's chunk range.  Without arguments: two numpy arrays; with pointers (host or device memory of
        gsa_hit_count entries): copied there."""
        n = int(self.lib.gsa_hit_count(self.ctx))
        if keys_ptr is not None:
            self._ck(self.lib.gsa_export_hits(self.ctx, C.c_void_p(keys_ptr), C.c_void_p(vals_ptr)))
            return n
        k = np.zeros(n, np.uint64); v = np.zeros(n, np.uint32)
        if n:
            self._ck(self.lib.gsa_export_hits(self.ctx, C.c_void_p(k.ctypes.data), C.c_void_p(v.ctypes.data)))
        return k, v

    def import_hits(self, keys, vals, n=None):
        """keys / vals: numpy arrays, or raw pointers (host or device memory) with n."""
        if n is None:
            keys = np.ascontiguousarray(keys, np.uint64); vals = np.ascontiguousarray(vals, np.uint32)
            n = int(keys.size); kp, vp = keys.ctypes.data, vals.ctypes.data
        else:
            kp, vp = keys, vals
        self._ck(self.lib.gsa_import_hits(self.ctx, C.c_void_p(kp), C.c_void_p(vp), C.c_int64(n)))

    def finish_contig(self) -> dict:
        res = Result()
        self._ck(self.lib.gsa_finish_contig(self.ctx, C.byref(res)))
        return self._result(res)

    def seeds(self):
        n = self.lib.gsa_seed_count(self.ctx)
        out = np.zeros(n, dtype=SEED_DT)
        if n:
            self._ck(self.lib.gsa_get_seeds(self.ctx, out.ctypes.data_as(C.c_void_p)))
        return out["qpos"].copy(), out["len"].copy(), out["rpos"].copy()

    def groups(self):
        n = self.lib.gsa_group_count(self.ctx)
        b = np.zeros(n, np.int32); e = np.zeros(n, np.int32)
        if n:
            self._ck(self.lib.gsa_get_groups(self.ctx, _p(b, C.c_int32), _p(e, C.c_int32)))
        return b, e

    def _result(self, res: Result) -> dict:
        nb, nf, na = res.n_blocks, res.n_frags, res.n_aln
        blocks = np.ctypeslib.as_array(C.cast(res.blocks, C.POINTER(C.c_uint8)), shape=(nb * BLOCK_DT.itemsize,)).view(BLOCK_DT).copy() if nb else np.zeros(0, BLOCK_DT)
        recs = np.ctypeslib.as_array(C.cast(res.recs, C.POINTER(C.c_uint8)), shape=(nf * REC_DT.itemsize,)).view(REC_DT).copy() if nf else np.zeros(0, REC_DT)
        frags = expand_recs(recs)
        a1 = np.ctypeslib.as_array(C.cast(res.aln1, C.POINTER(C.c_uint8)), shape=(na,)).copy() if na else np.zeros(0, np.uint8)
        a2 = np.ctypeslib.as_array(C.cast(res.aln2, C.POINTER(C.c_uint8)), shape=(na,)).copy() if na else np.zeros(0, np.uint8)
        return dict(blocks=blocks, frags=frags, aln1=a1, aln2=a2)

    def call_variants(self, k: int = 0):
        """gsa_call_variants on the stage-8 result this context holds (contig k of a bundle): (VARIANT_DT array, (n_snv, n_ins, n_del))."""
        var = Variants()
        self.lib.gsa_call_variants.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Variants)]
        self._ck(self.lib.gsa_call_variants(self.ctx, C.c_int32(k), C.byref(var)))
        return variants_array(var)

    def block_cigars(self, k: int = 0):
        """gsa_block_cigars on the stage-8 result this context holds (contig k of a bundle): (BLOCK_CIGAR_DT array, one entry per block; uint32 ops)."""
        cig = Cigars()
        self.lib.gsa_block_cigars.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Cigars)]
        self._ck(self.lib.gsa_block_cigars(self.ctx, C.c_int32(k), C.byref(cig)))
        return cigars_arrays(cig)

    def block_cs(self, k: int = 0):
        """gsa_block_cs on the stage-8 result this context holds (contig k of a bundle): (BLOCK_CS_DT array, one entry per block; uint8 bytes of all strings)."""
        cs = Cs()
        self.lib.gsa_block_cs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Cs)]
        self._ck(self.lib.gsa_block_cs(self.ctx, C.c_int32(k), C.byref(cs)))
        return cs_arrays(cs)

    def lift_set(self, pos) -> None:
        """gsa_lift_set: the reference positions (0-based forward global coordinates) this context lifts from now on; an empty list clears them."""
        pos = np.ascontiguousarray(pos, dtype=np.int64)
        self.lib.gsa_lift_set.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self._ck(self.lib.gsa_lift_set(self.ctx, C.c_void_p(pos.ctypes.data) if pos.size else None, C.c_int64(pos.size)))

    def lift(self, k: int = 0):
        """gsa_lift on the stage-8 result this context holds (contig k of a bundle): LIFT_HIT_DT array, ascending in idx."""
        l = Lifts()
        self.lib.gsa_lift.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Lifts)]
        self._ck(self.lib.gsa_lift(self.ctx, C.c_int32(k), C.byref(l)))
        return lifts_array(l)

    def regions_set(self, beg, end) -> None:
        """gsa_regions_set: the reference regions [beg[i], end[i]) (0-based forward global coordinates, half-open, each inside one sequence) this context lifts from now
        on; empty lists clear them."""
        beg = np.ascontiguousarray(beg, np.int64); end = np.ascontiguousarray(end, np.int64)
        if beg.shape != end.shape or beg.ndim != 1:
            raise ValueError("regions_set: beg and end must be one-dimensional and of one length")
        self.lib.gsa_regions_set.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
        self._ck(self.lib.gsa_regions_set(self.ctx, C.c_void_p(beg.ctypes.data) if beg.size else None, C.c_void_p(end.ctypes.data) if end.size else None, C.c_int64(beg.size)))

    def lift_regions(self, k: int = 0):
        """gsa_lift_regions on the stage-8 result this context holds (contig k of a bundle): REGION_HIT_DT array, ascending in idx."""
        l = RegionLifts()
        self.lib.gsa_lift_regions.argtypes = [C.c_void_p, C.c_int32, C.POINTER(RegionLifts)]
        self._ck(self.lib.gsa_lift_regions(self.ctx, C.c_int32(k), C.byref(l)))
        return regions_array(l)

    def region_timing(self):
        """(host wall ms inside gsa_lift_regions on this context since it was created, number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_region_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_region_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def lift_timing(self):
        """(host wall ms inside gsa_lift on this context since it was created, number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_lift_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_lift_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def track_set(self, window: int) -> None:
        """gsa_track_set: the window length W of this context's per-window reference track from now on; 0 clears it."""
        self.lib.gsa_track_set.argtypes = [C.c_void_p, C.c_int32]
        self._ck(self.lib.gsa_track_set(self.ctx, C.c_int32(int(window))))

    def track(self, k: int = 0):
        """gsa_ref_track on the stage-8 result this context holds (contig k of a bundle): TRACK_WIN_DT array, ascending by (chr, start)."""
        t = Tracks()
        self.lib.gsa_ref_track.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Tracks)]
        self._ck(self.lib.gsa_ref_track(self.ctx, C.c_int32(k), C.byref(t)))
        return tracks_array(t)

    def qtrack_set(self, window: int) -> None:
        """gsa_qtrack_set: the window length W of this context's per-window query track from now on; 0 clears it.  Independent of track_set."""
        self.lib.gsa_qtrack_set.argtypes = [C.c_void_p, C.c_int32]
        self._ck(self.lib.gsa_qtrack_set(self.ctx, C.c_int32(int(window))))

    def qtrack(self, k: int = 0):
        """gsa_query_track on the stage-8 result this context holds (contig k of a bundle): QTRACK_WIN_DT array, ascending by start."""
        t = QTracks()
        self.lib.gsa_query_track.argtypes = [C.c_void_p, C.c_int32, C.POINTER(QTracks)]
        self._ck(self.lib.gsa_query_track(self.ctx, C.c_int32(k), C.byref(t)))
        return qtracks_array(t)

    def qtrack_timing(self):
        """(host wall ms inside gsa_query_track on this context since it was created, number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_qtrack_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_qtrack_timing(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, int(n.value)

    def track_timing(self):
        """(host wall ms inside gsa_ref_track on this context since it was created, number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_track_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_track_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def block_segs(self, k: int = 0):
        """gsa_block_segs on the stage-8 result this context holds (contig k of a bundle): (SEG_BLOCK_DT array, one entry per block; SEG_DT array of all triples)."""
        sg = Segs()
        self.lib.gsa_block_segs.argtypes = [C.c_void_p, C.c_int32, C.POINTER(Segs)]
        self._ck(self.lib.gsa_block_segs(self.ctx, C.c_int32(k), C.byref(sg)))
        return segs_arrays(sg)

    def seg_timing(self):
        """(host wall ms inside gsa_block_segs on this context since it was created, its CIGAR pass included; number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_seg_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_seg_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def proj_open(self, share: "Aligner" = None, no_dup: bool = False) -> None:
        """gsa_proj_open: an accumulator of G words on this context's device (share=None), or the one `share` holds on the same device.  no_dup: GSA_PROJ_NO_DUP."""
        self.lib.gsa_proj_open.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
        self._ck(self.lib.gsa_proj_open(self.ctx, share.ctx if share is not None else None, C.c_uint32(PROJ_NO_DUP if no_dup else 0)))

    def proj_close(self) -> None:
        """gsa_proj_close: this context lets go of its accumulator (the last holder frees it)."""
        self.lib.gsa_proj_close.argtypes = [C.c_void_p]
        self._ck(self.lib.gsa_proj_close(self.ctx))

    def proj_clear(self) -> None:
        """gsa_proj_clear: every word back to 0."""
        self.lib.gsa_proj_clear.argtypes = [C.c_void_p]
        self._ck(self.lib.gsa_proj_clear(self.ctx))

    def project(self, k: int = 0):
        """gsa_project: the stage-8 result this context holds (contig k of a bundle) painted into its accumulator.  Returns (blocks painted, words offered)."""
        st = ProjStat()
        self.lib.gsa_project.argtypes = [C.c_void_p, C.c_int32, C.POINTER(ProjStat)]
        self._ck(self.lib.gsa_project(self.ctx, C.c_int32(k), C.byref(st)))
        return int(st.n_blocks), int(st.n_cols)

    def proj_fetch(self, p0: int = 0, n: int = None, words: bool = False):
        """gsa_proj_fetch of positions [p0, p0 + n) (n=None: to the end of the reference): the characters as bytes, or with words=True (bytes, uint32 array)."""
        n = int(self.idx.G) - int(p0) if n is None else int(n)
        text = np.zeros(max(n, 1), np.uint8)
        w = np.zeros(max(n, 1), np.uint32) if words else None
        self.lib.gsa_proj_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        self._ck(self.lib.gsa_proj_fetch(self.ctx, C.c_int64(p0), C.c_int64(n), C.c_void_p(text.ctypes.data), C.c_void_p(w.ctypes.data) if words else None))
        t = text[:max(n, 0)].tobytes()
        return (t, w[:max(n, 0)]) if words else t

    def proj_merge(self, words, p0: int = 0) -> None:
        """gsa_proj_merge: host words (another device's accumulator, as proj_fetch(words=True) returns them) into positions [p0, p0 + len(words)): the maximum stays."""
        w = np.ascontiguousarray(words, dtype=np.uint32)
        self.lib.gsa_proj_merge.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]
        self._ck(self.lib.gsa_proj_merge(self.ctx, C.c_int64(p0), C.c_int64(w.size), C.c_void_p(w.ctypes.data) if w.size else None))

    def proj_timing(self):
        """(host wall ms inside gsa_project on this context since it was created, number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_proj_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_proj_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def cs_timing(self):
        """(host wall ms inside gsa_block_cs on this context since it was created, its CIGAR pass included; number of calls)."""
        ms, n = C.c_double(0), C.c_int64(0)
        self.lib.gsa_get_cs_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_cs_timing(self.ctx, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def cigar_timing(self):
        """(host wall ms inside gsa_block_cigars on this context since it was created, number of calls)."""
        ms = C.c_double(0); n = C.c_int64(0)
        self.lib.gsa_get_cigar_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_cigar_timing(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def variant_timing(self):
        """(device ms summed over the variant passes since set_profiling(..., variants=True), number of passes)."""
        ms = C.c_double(0); n = C.c_int64(0)
        self.lib.gsa_get_variant_timing.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        self._ck(self.lib.gsa_get_variant_timing(self.ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def raw_result(self) -> Result:
        """The gsa_result view (pointers into library-owned memory, no copies)."""
        res = Result()
        self._ck(self.lib.gsa_get_blocks(self.ctx, C.byref(res)))
        return res

    def block_records(self) -> np.ndarray:
        """uint8 [n_blocks, 40]: the finished gsa_block records (copied; small)."""
        res = self.raw_result()
        if not res.n_blocks:
            return np.zeros((0, 40), np.uint8)
        return np.ctypeslib.as_array(C.cast(res.blocks, C.POINTER(C.c_uint8)), shape=(res.n_blocks * 40,)).reshape(-1, 40).copy()

    def blocks(self) -> dict:
        res = Result()
        self._ck(self.lib.gsa_get_blocks(self.ctx, C.byref(res)))
        return self._result(res)

    def blocks_as_dump(self, with_aln: bool = False) -> dict:
        """Same keys/shapes as oracle_py._StageReader.blocks(): records gathered in block order."""
        return result_as_dump(self.blocks(), with_aln)

    def dump_stages(self, upto: int = 8) -> dict:
        d = {}
        for st in range(1, upto + 1):
            self.run_to(st)
            if st == 1:
                q, l, r = self.seeds(); b, e = self.groups()
                d.update(s1_qpos=q, s1_qlen=l, s1_rpos=r, s1_gbeg=b, s1_gend=e)
            else:
                for k, v in self.blocks_as_dump(with_aln=(st == 8)).items():
                    d[f"s{st}_{k}"] = v
        return d

    def counters(self) -> np.ndarray:
        c = np.zeros(8, np.uint64)
        self._ck(self.lib.gsa_get_counters(self.ctx, _p(c, C.c_uint64)))
        return c

    def timings(self) -> np.ndarray:
        t = np.zeros(8, np.float32)
        self._ck(self.lib.gsa_get_timings(self.ctx, _p(t, C.c_float)))
        return t

    # ---- leaf operators ----
    def bwt_search_batch(self, start, stop):
        start = np.ascontiguousarray(start, np.int32); stop = np.ascontiguousarray(stop, np.int32)
        n = start.size
        ln = np.zeros(n, np.int32); fr = np.zeros(n, np.int32); loc = np.zeros(n * 100, np.int64)
        self._ck(self.lib.gsa_bwt_search_batch(self.ctx, C.c_int32(n), _p(start, C.c_int32), _p(stop, C.c_int32), _p(ln, C.c_int32), _p(fr, C.c_int32), _p(loc, C.c_int64)))
        return ln, fr, loc.reshape(n, 100)

    def ksw2_batch(self, s1_list, s2_list):
        """list of bytes pairs -> list of forward op strings (bytes)."""
        n = len(s1_list)
        l1 = np.array([len(x) for x in s1_list], np.int32); l2 = np.array([len(x) for x in s2_list], np.int32)
        o1 = np.concatenate([[0], np.cumsum(l1[:-1], dtype=np.int64)]).astype(np.int64) if n else np.zeros(0, np.int64)
        o2 = np.concatenate([[0], np.cumsum(l2[:-1], dtype=np.int64)]).astype(np.int64) if n else np.zeros(0, np.int64)
        mn = (l1 + l2).astype(np.int64)
        oo = np.concatenate([[0], np.cumsum(mn[:-1])]).astype(np.int64) if n else np.zeros(0, np.int64)
        p1 = b"".join(s1_list) + b"\0"; p2 = b"".join(s2_list) + b"\0"
        ops = np.zeros(int(mn.sum()) + 1, np.uint8); ol = np.zeros(n, np.int32)
        self._ck(self.lib.gsa_ksw2_batch(self.ctx, C.c_int32(n), p1, _p(o1, C.c_int64), _p(l1, C.c_int32), p2, _p(o2, C.c_int64), _p(l2, C.c_int32),
                                         ops.ctypes.data_as(C.c_char_p), _p(oo, C.c_int64), _p(ol, C.c_int32)))
        return [ops[oo[i]:oo[i] + ol[i]].tobytes() for i in range(n)]

    def gap_similarity_batch(self, q1, q2, r1, r2):
        q1 = np.ascontiguousarray(q1, np.int32); q2 = np.ascontiguousarray(q2, np.int32)
        r1 = np.ascontiguousarray(r1, np.int64); r2 = np.ascontiguousarray(r2, np.int64)
        res = np.zeros(q1.size, np.int32)
        self._ck(self.lib.gsa_gap_similarity_batch(self.ctx, C.c_int32(q1.size), _p(q1, C.c_int32), _p(q2, C.c_int32), _p(r1, C.c_int64), _p(r2, C.c_int64), _p(res, C.c_int32)))
        return res

    def align_bundle(self, contigs) -> list:
        """gsa_align_bundle: several contigs (uint8 arrays, or DeviceContig objects -- all of one kind) in ONE pass; one result dict
        per contig, each what align_contig of that contig alone gives."""
        n = len(contigs)
        on_dev = n > 0 and isinstance(contigs[0], DeviceContig)
        self._q = contigs
        qs = (C.c_char_p * n)(*[C.cast(c.ptr if on_dev else c.ctypes.data, C.c_char_p) for c in contigs])
        ql = (C.c_int32 * n)(*[int(c.size) for c in contigs])
        res = (Result * n)()
        self.lib.gsa_align_bundle.argtypes = [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.POINTER(Result)]
        self._ck(self.lib.gsa_align_bundle(self.ctx, qs, ql, n, 2 if on_dev else 0, res))
        return [self._result(res[k]) for k in range(n)]

    def align_contig_raw(self, seq: np.ndarray) -> Result:
        """gsa_align_contig without copying the result out (views into library-owned memory)."""
        self._q = seq
        res = Result()
        self._ck(self.lib.gsa_align_contig(self.ctx, seq.ctypes.data_as(C.c_char_p), C.c_int32(seq.size), C.byref(res)))
        return res

    def close(self):
        if self.ctx:
            self.lib.gsa_destroy(self.ctx); self.ctx = C.c_void_p()
        for p in self._pinned:
            self.lib.gsa_host_free(p)
        self._pinned = []
        for d in self._devbufs:
            d.free()
        self._devbufs = []


def apply_ops(s1: bytes, s2: bytes, ops: bytes):
    """Forward M/D/I string -> the two gapped strings (what ksw2_alignment leaves in s1/s2)."""
    a, b, i, j = bytearray(), bytearray(), 0, 0
    for o in ops:
        if o == 0x44:      # 'D': gap in s1
            a.append(0x2D); b.append(s2[j]); j += 1
        elif o == 0x49:    # 'I': gap in s2
            a.append(s1[i]); b.append(0x2D); i += 1
        else:
            a.append(s1[i]); b.append(s2[j]); i += 1; j += 1
    return bytes(a), bytes(b)
