"""ctypes binding of libgsa_host.so: the CPU-side components (index builder, MAF/VCF
emitters) behind a small C API, so the CPU test-suite can check them without a GPU."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

from . import capi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libgsa_host.so")
CLI_PATH = os.path.join(HERE, "bin", "GSAlign_hip")

RESULT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_char), C.c_int, C.POINTER(capi.Result))


def build() -> None:
    subprocess.run(["make", "-C", os.path.join(HERE, "csrc"), "-j8", "all"], check=True, stdout=subprocess.DEVNULL)


def load() -> C.CDLL:
    path = os.environ.get("GSA_HOST_LIB_PATH") or LIB_PATH      # (an instrumented build of the same sources: tools/host_tsan.sh)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build()")
    return C.CDLL(path)


def build_index(fasta: str, prefix: str) -> None:
    err = C.create_string_buffer(256)
    if load().gsah_c_build_index(fasta.encode(), prefix.encode(), err) != 0:
        raise RuntimeError(err.value.decode())


BWT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint8), C.c_int64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64))


def build_index_with(fasta: str, prefix: str, fn) -> None:
    """gsah_build_index_with: the index builder with its BWT/SA half supplied by `fn`.  fn(pac uint8[ceil(G/4)], G) returns
    (hdr uint64[5] = [primary, L2[1..4]], bwt uint32[], sa uint64[]) -- the arrays of indexio.BwaIndex, sized as capi.index_sizes(G) says;
    an exception (or arrays of another size) fails the build before .bwt / .sa are written.  fn = None: the host builder (build_index)."""
    failure: list = []

    def cb(user, pac, G, primary, L2, bwt, sa):
        try:
            G = int(G)
            hdr, b, s = fn(np.ctypeslib.as_array(pac, shape=((G + 3) // 4,)).copy(), G)
            hdr = np.asarray(hdr, dtype=np.uint64); b = np.ascontiguousarray(b, dtype=np.uint32); s = np.ascontiguousarray(s, dtype=np.uint64)
            S = 2 * G
            if hdr.size != 5 or b.size != (S + 15) // 16 + ((S + 127) // 128 + 1) * 8 or s.size != (S + 32) // 32:
                raise ValueError("the callback's arrays have the wrong size")
            primary[0] = int(hdr[0]); L2[0] = 0
            for k in range(1, 5):
                L2[k] = int(hdr[k])
            C.memmove(bwt, b.ctypes.data, b.nbytes); C.memmove(sa, s.ctypes.data, s.nbytes)
            return 0
        except Exception as e:      # (an exception must not unwind through the C frames)
            failure.append(e)
            return 1

    err = C.create_string_buffer(256)
    lib = load()
    lib.gsah_c_build_index_with.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_char_p]
    keep = BWT_FN(cb) if fn is not None else None
    rc = lib.gsah_c_build_index_with(fasta.encode(), prefix.encode(), C.cast(keep, C.c_void_p) if keep is not None else None, None, err)
    if rc != 0:
        e = RuntimeError(err.value.decode() + (f": {failure[0]!r}" if failure else ""))
        if failure:
            e.__cause__ = failure[0]
        raise e


def build_index_gpu(fasta: str, prefix: str, device: int = 0, wide: bool = False, batch_cap: int = 0, occ_segment: int = 0) -> None:
    """The index files of `fasta` with the BWT/SA half built on the GPU (capi.build_index_arrays): the same five files as build_index.  wide: the batched
    64-bit sorter whatever the length (it runs by itself over 1 073 741 822 bases)."""
    build_index_with(fasta, prefix, lambda pac, G: capi.build_index_arrays(pac, G, device, wide=wide, batch_cap=batch_cap, occ_segment=occ_segment))


def reference_from_fasta(fasta: str):
    """gsah_reference_from_fasta: (pac uint8[ceil(G / 4)], G, names, lens int32[]) of a reference FASTA -- what the index builder would put into .pac and .ann, with
    no file written: the arguments of capi.Aligner.from_reference."""
    lib = load()
    lib.gsah_c_reference_from_fasta.argtypes = [C.c_char_p, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong), C.c_char_p]
    lib.gsah_c_reference_pac.restype = C.POINTER(C.c_uint8)
    lib.gsah_c_reference_name.restype = C.c_char_p
    G, nb = C.c_longlong(), C.c_longlong()
    err = C.create_string_buffer(256)
    n = lib.gsah_c_reference_from_fasta(fasta.encode(), C.byref(G), C.byref(nb), err)
    if n < 0:
        raise RuntimeError(err.value.decode())
    pac = np.ctypeslib.as_array(lib.gsah_c_reference_pac(), shape=(int(nb.value),)).copy()
    names = [lib.gsah_c_reference_name(i).decode() for i in range(n)]
    lens = np.array([lib.gsah_c_reference_len(i) for i in range(n)], dtype=np.int32)
    return pac, int(G.value), names, lens


def result_from_dump(d: dict, keep: list):
    """dict in the oracle/capi 'blocks_as_dump' layout -> a populated capi.Result (arrays appended to `keep`)."""
    nb = d["b_score"].size; nf = d["f_qpos"].size
    B = np.zeros(nb, capi.BLOCK_DT); F = np.zeros(nf, capi.FRAG_DT)
    B["score"] = d["b_score"]; B["aln_len"] = d["b_aln_len"]; B["bdup"] = d["b_bdup"]; B["n_frag"] = d["b_nfrag"]
    B["frag_off"] = np.concatenate([[0], np.cumsum(d["b_nfrag"][:-1], dtype=np.int64)]) if nb else 0
    B["bdir"] = d["b_bdir"]; B["gpos"] = d["b_gpos"]; B["chr"] = d["b_chr"]
    F["bseed"] = d["f_bseed"]; F["qpos"] = d["f_qpos"]; F["qlen"] = d["f_qlen"]; F["rlen"] = d["f_rlen"]; F["rpos"] = d["f_rpos"]
    F["aln_len"] = d["f_alnlen"]
    F["aln_off"] = np.concatenate([[0], np.cumsum(d["f_alnlen"][:-1], dtype=np.int64)]) if nf else 0
    a1 = np.ascontiguousarray(d["aln1"]); a2 = np.ascontiguousarray(d["aln2"])
    keep.extend([B, F, a1, a2])
    r = capi.Result()
    r.n_blocks = nb; r.n_frags = nf; r.n_aln = a1.size
    R = capi.pack_recs(F); keep.append(R)
    r.blocks = C.cast(B.ctypes.data, C.POINTER(capi.Block)); r.recs = C.cast(R.ctypes.data, C.POINTER(capi.Rec))
    r.aln1 = C.cast(a1.ctypes.data, C.POINTER(C.c_char)); r.aln2 = C.cast(a2.ctypes.data, C.POINTER(C.c_char))
    return r


def emit(index_prefix: str, query_fa: str, maf_path: str, vcf_path: str, reference_label: str, per_contig, allow_dup: bool = True, fmt: int = 1, summary: bool = False, cs: bool = False, chain: str = None) -> None:
    """per_contig(ci, seq_uint8) -> dump dict of the finished contig (stage 8 layout).  fmt 1 = MAF, 2 = ALN, 3 = PAF with the host comparator's CIGARs (written to maf_path).
    summary=True (fmt 3 only; gsah_c_emit_summary): the PAF is formatted from a summary result -- blocks and block ends, taken out of the full dump, with the
    comparator's CIGARs -- and no VCF is written (vcf_path is not opened).
    cs=True (fmt 3 only; gsah_c_emit_paf_cs): every line also gets the cs:Z: field, from the host comparator gsah_block_cs.
    chain=path (not with summary=True; gsah_c_emit_chain): a UCSC chain file is written there beside the other files, its triples from the host comparator gsah_block_segs."""
    keep: list = []
    if cs and (fmt != 3 or summary):
        raise ValueError("cs=True goes with fmt=3 (and not with summary=True)")
    if summary and fmt != 3:
        raise ValueError("summary=True formats PAF only (fmt=3)")
    if chain is not None and summary:
        raise ValueError("chain= needs the records and strings a summary result does not hold")

    def cb(user, ci, seq, ln, out):
        s = np.frombuffer(C.string_at(seq, ln), dtype=np.uint8)
        r = result_from_dump(per_contig(ci, s), keep)
        C.memmove(out, C.byref(r), C.sizeof(capi.Result))
        return 0

    err = C.create_string_buffer(256)
    if summary:
        rc = load().gsah_c_emit_summary(index_prefix.encode(), query_fa.encode(), maf_path.encode(), 1 if allow_dup else 0, RESULT_CB(cb), None, err)
        if rc != 0:
            raise RuntimeError(f"gsah_c_emit_summary -> {rc}: {err.value.decode()}")
        return
    if chain is not None:
        rc = load().gsah_c_emit_chain(index_prefix.encode(), query_fa.encode(), maf_path.encode(), vcf_path.encode(), reference_label.encode(), 1 if allow_dup else 0, int(fmt), 1 if cs else 0,
                                      chain.encode(), RESULT_CB(cb), None, err)
        if rc != 0:
            raise RuntimeError(f"gsah_c_emit_chain -> {rc}: {err.value.decode()}")
        return
    if cs:
        rc = load().gsah_c_emit_paf_cs(index_prefix.encode(), query_fa.encode(), maf_path.encode(), vcf_path.encode(), reference_label.encode(), 1 if allow_dup else 0, RESULT_CB(cb), None, err)
        if rc != 0:
            raise RuntimeError(f"gsah_c_emit_paf_cs -> {rc}: {err.value.decode()}")
        return
    rc = load().gsah_c_emit_fmt(index_prefix.encode(), query_fa.encode(), maf_path.encode(), vcf_path.encode(), reference_label.encode(),
                                1 if allow_dup else 0, fmt, RESULT_CB(cb), None, err)
    if rc != 0:
        raise RuntimeError(f"gsah_c_emit -> {rc}: {err.value.decode()}")


def dotplot(index_prefix: str, query_fa: str, contig: int, gp_path: str, out_prefix: str, per_contig) -> bool:
    """OutputDotplot (DotPloting.cpp:10-71) for one contig: gnuplot script + data files, gnuplot itself is not run."""
    keep: list = []

    def cb(user, ci, seq, ln, out):
        s = np.frombuffer(C.string_at(seq, ln), dtype=np.uint8)
        r = result_from_dump(per_contig(ci, s), keep)
        C.memmove(out, C.byref(r), C.sizeof(capi.Result))
        return 0

    err = C.create_string_buffer(256)
    rc = load().gsah_c_dotplot(index_prefix.encode(), query_fa.encode(), contig, gp_path.encode(), out_prefix.encode(), RESULT_CB(cb), None, err)
    if rc < 0:
        raise RuntimeError(f"gsah_c_dotplot -> {rc}: {err.value.decode()}")
    return rc == 1


def result_from_arrays(r: dict, keep: list):
    """A result dict of capi.Aligner (blocks / frags / aln1 / aln2, records where the blocks' frag_off says) -> a populated capi.Result."""
    B = np.ascontiguousarray(r["blocks"]); R = capi.pack_recs(r["frags"])
    a1 = np.ascontiguousarray(r["aln1"]); a2 = np.ascontiguousarray(r["aln2"])
    keep.extend([B, R, a1, a2])
    res = capi.Result()
    res.n_blocks = B.size; res.n_frags = R.size; res.n_aln = a1.size
    res.blocks = C.cast(B.ctypes.data, C.POINTER(capi.Block)); res.recs = C.cast(R.ctypes.data, C.POINTER(capi.Rec))
    res.aln1 = C.cast(a1.ctypes.data, C.POINTER(C.c_char)); res.aln2 = C.cast(a2.ctypes.data, C.POINTER(C.c_char))
    return res


def variants(index_prefix: str, seq: np.ndarray, result):
    """gsah_c_variants: VariantIdentification of one finished contig on the host, as gsa_variant records in the serial order -- what
    Aligner.call_variants computes on the GPU.  result: a capi.Result, a dump dict (oracle layout) or a result dict of capi.Aligner.
    Returns (VARIANT_DT array, (n_snv, n_ins, n_del))."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    lib = load()
    lib.gsah_c_variants.restype = C.c_longlong
    lib.gsah_c_variants.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.POINTER(capi.Result), C.c_void_p, C.c_longlong, C.POINTER(C.c_longlong)]
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    cnt = (C.c_longlong * 3)()
    n = lib.gsah_c_variants(index_prefix.encode(), C.c_void_p(seq.ctypes.data), int(seq.size), C.byref(result), None, 0, cnt)
    if n < 0:
        raise RuntimeError(f"gsah_c_variants -> {n}")
    V = np.zeros(int(n), capi.VARIANT_DT)
    if n:
        n2 = lib.gsah_c_variants(index_prefix.encode(), C.c_void_p(seq.ctypes.data), int(seq.size), C.byref(result), C.c_void_p(V.ctypes.data), n, cnt)
        assert n2 == n
    return V, (int(cnt[0]), int(cnt[1]), int(cnt[2]))


def cigars(index_prefix, seq, result):
    """gsah_c_cigars: the CIGAR of every block of one finished contig on the host, from the gapped strings and seed records, untrimmed -- what
    Aligner.block_cigars computes on the GPU.  result: a capi.Result, a dump dict (oracle layout) or a result dict of capi.Aligner.  seq: the query
    contig (seed columns are classified from its text) or None.  index_prefix is not needed by the walk and may be None (kept for symmetry with variants()).
    Returns (BLOCK_CIGAR_DT array, uint32 ops)."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    lib = load()
    lib.gsah_c_cigars.restype = C.c_longlong
    lib.gsah_c_cigars.argtypes = [C.c_void_p, C.c_int, C.POINTER(capi.Result), C.c_void_p, C.c_void_p, C.c_longlong]
    sp, sn = None, 0
    if seq is not None:
        seq = np.ascontiguousarray(seq, dtype=np.uint8); sp, sn = C.c_void_p(seq.ctypes.data), int(seq.size)
    blk = np.zeros(int(result.n_blocks), capi.BLOCK_CIGAR_DT)
    n = lib.gsah_c_cigars(sp, sn, C.byref(result), C.c_void_p(blk.ctypes.data), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_cigars -> {n}")
    ops = np.zeros(int(n), np.uint32)
    if n:
        n2 = lib.gsah_c_cigars(sp, sn, C.byref(result), C.c_void_p(blk.ctypes.data), C.c_void_p(ops.ctypes.data), n)
        assert n2 == n
    return blk, ops


def cigar_trim(ops, bdir: bool, ext: int, counts):
    """gsah_c_cigar_trim: iExtension's trim on ONE block's ops (output order) -- the last `ext` columns in walk order go.  counts = (n_eq, n_x, n_ins, n_del).
    Returns (ops that stay, reduced counts)."""
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    bc = np.zeros(1, capi.BLOCK_CIGAR_DT)
    bc["n_cig"] = ops.size; bc["n_eq"], bc["n_x"], bc["n_ins"], bc["n_del"] = counts
    out = np.zeros(max(ops.size, 1), np.uint32)
    lib = load()
    lib.gsah_c_cigar_trim.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_void_p, C.c_void_p]
    n = lib.gsah_c_cigar_trim(C.c_void_p(ops.ctypes.data), 1 if bdir else 0, int(ext), C.c_void_p(out.ctypes.data), C.c_void_p(bc.ctypes.data))
    if n < 0:
        raise RuntimeError(f"gsah_c_cigar_trim -> {n}")
    assert n == int(bc["n_cig"][0])
    return out[:n].copy(), (int(bc["n_eq"][0]), int(bc["n_x"][0]), int(bc["n_ins"][0]), int(bc["n_del"][0]))


def cs(index_prefix, seq, result):
    """gsah_c_cs: the cs string (PAF's cs:Z:, short form) of every block of one finished contig on the host, from the gapped strings and seed records, untrimmed -- what
    Aligner.block_cs computes on the GPU.  result: a capi.Result, a dump dict (oracle layout) or a result dict of capi.Aligner.  index_prefix and seq are not needed by the
    walk and may be None (kept for symmetry with cigars()).  Returns (BLOCK_CS_DT array, uint8 bytes); block b's string is bytes[cs_off : cs_off + n_cs]."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    lib = load()
    lib.gsah_c_cs.restype = C.c_longlong
    lib.gsah_c_cs.argtypes = [C.POINTER(capi.Result), C.c_void_p, C.c_void_p, C.c_longlong]
    blk = np.zeros(int(result.n_blocks), capi.BLOCK_CS_DT)
    n = lib.gsah_c_cs(C.byref(result), C.c_void_p(blk.ctypes.data), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_cs -> {n}")
    by = np.zeros(int(n), np.uint8)
    if n:
        n2 = lib.gsah_c_cs(C.byref(result), C.c_void_p(blk.ctypes.data), C.c_void_p(by.ctypes.data), n)
        assert n2 == n
    return blk, by


def lift(index_prefix, seq, result, positions):
    """gsah_c_lift: the reference positions (0-based forward global coordinates) lifted through one finished contig on the host, from the records and the gapped
    strings -- what Aligner.lift computes on the GPU, by the contract of gsa_lift (include/gsa_hip.h).  result: a capi.Result, a dump dict (oracle layout) or a result
    dict of capi.Aligner.  The index under index_prefix supplies the reference sequences' lengths (the trim); seq is not needed by the walk and may be None.
    Returns a LIFT_HIT_DT array, ascending in idx; positions no block covers are absent."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    pos = np.ascontiguousarray(positions, dtype=np.int64)
    lib = load()
    lib.gsah_c_lift.restype = C.c_longlong
    lib.gsah_c_lift.argtypes = [C.c_char_p, C.POINTER(capi.Result), C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    H = np.zeros(int(pos.size), capi.LIFT_HIT_DT)
    n = lib.gsah_c_lift(index_prefix.encode(), C.byref(result), C.c_void_p(pos.ctypes.data), int(pos.size), C.c_void_p(H.ctypes.data), int(H.size))
    if n < 0:
        raise RuntimeError(f"gsah_c_lift -> {n}")
    return H[:int(n)].copy()


def lift_regions(index_prefix, seq, result, beg, end):
    """gsah_c_lift_regions: the reference regions [beg[i], end[i]) (0-based forward global coordinates, half-open) lifted through one finished contig on the host, from
    the records and the gapped strings -- what Aligner.lift_regions computes on the GPU, by the contract of gsa_lift_regions (include/gsa_hip.h).  result: a capi.Result,
    a dump dict (oracle layout) or a result dict of capi.Aligner.  The index under index_prefix supplies the reference sequences' lengths (the trim); seq is not needed
    by the walk and may be None.  Returns a REGION_HIT_DT array, ascending in idx; regions no block overlaps are absent."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    b = np.ascontiguousarray(beg, dtype=np.int64); e = np.ascontiguousarray(end, dtype=np.int64)
    if b.shape != e.shape or b.ndim != 1:
        raise ValueError("lift_regions: beg and end must be one-dimensional and of one length")
    lib = load()
    lib.gsah_c_lift_regions.restype = C.c_longlong
    lib.gsah_c_lift_regions.argtypes = [C.c_char_p, C.POINTER(capi.Result), C.c_void_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    H = np.zeros(int(b.size), capi.REGION_HIT_DT)
    n = lib.gsah_c_lift_regions(index_prefix.encode(), C.byref(result), C.c_void_p(b.ctypes.data), C.c_void_p(e.ctypes.data), int(b.size), C.c_void_p(H.ctypes.data), int(H.size))
    if n < 0:
        raise RuntimeError(f"gsah_c_lift_regions -> {n}")
    return H[:int(n)].copy()


def track(index_prefix, seq, result, W: int):
    """gsah_c_track: the per-window track of one finished contig over the reference sequences at window length W, on the host, from the records and the gapped
    strings -- what Aligner.track computes on the GPU, by the contract of gsa_ref_track (include/gsa_hip.h).  result: a capi.Result, a dump dict (oracle layout) or a
    result dict of capi.Aligner.  The index under index_prefix supplies the reference sequences' lengths; seq is not needed by the walk and may be None.
    Returns a TRACK_WIN_DT array: one record per window with n_cov > 0, ascending by (chr, start)."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    lib = load()
    lib.gsah_c_track.restype = C.c_longlong
    lib.gsah_c_track.argtypes = [C.c_char_p, C.POINTER(capi.Result), C.c_int32, C.c_void_p, C.c_longlong]
    n = lib.gsah_c_track(index_prefix.encode(), C.byref(result), int(W), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_track -> {n}")
    T = np.zeros(int(n), capi.TRACK_WIN_DT)
    if n:
        n2 = lib.gsah_c_track(index_prefix.encode(), C.byref(result), int(W), C.c_void_p(T.ctypes.data), int(T.size))
        if n2 != n:
            raise RuntimeError(f"gsah_c_track -> {n2} after {n}")
    return T


def qtrack(index_prefix, seq, result, W: int):
    """gsah_c_qtrack: the per-window track of one finished contig over the QUERY contig at window length W, on the host, from the records and the gapped strings -- what
    Aligner.qtrack computes on the GPU, by the contract of gsa_query_track (include/gsa_hip.h).  result: a capi.Result, a dump dict (oracle layout) or a result dict of
    capi.Aligner.  seq: the contig (uint8 array or bytes; only its length is read -- or the length itself); the index under index_prefix supplies the reference
    sequences' lengths (the trim).  Returns a QTRACK_WIN_DT array: one record per window with n_cov > 0, ascending by start."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    qlen = int(seq) if isinstance(seq, (int, np.integer)) else len(seq)
    lib = load()
    lib.gsah_c_qtrack.restype = C.c_longlong
    lib.gsah_c_qtrack.argtypes = [C.c_char_p, C.POINTER(capi.Result), C.c_int32, C.c_int32, C.c_void_p, C.c_longlong]
    n = lib.gsah_c_qtrack(index_prefix.encode(), C.byref(result), qlen, int(W), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_qtrack -> {n}")
    T = np.zeros(int(n), capi.QTRACK_WIN_DT)
    if n:
        n2 = lib.gsah_c_qtrack(index_prefix.encode(), C.byref(result), qlen, int(W), C.c_void_p(T.ctypes.data), int(T.size))
        if n2 != n:
            raise RuntimeError(f"gsah_c_qtrack -> {n2} after {n}")
    return T


def project(index_prefix, seq, result, words, flags: int = 0):
    """gsah_c_project: one finished contig painted into the caller's accumulator `words` (a C-contiguous uint32 array of G entries, changed in place: the maximum stays)
    on the host, from the records, the gapped strings and the query contig seq (uint8 array or bytes: its bases stand in the seeds' columns) -- what Aligner.project
    paints on the GPU, by the contract of gsa_project (include/gsa_hip.h).  result: a capi.Result, a dump dict (oracle layout) or a result dict of capi.Aligner.
    flags: capi.PROJ_NO_DUP.  Returns (blocks painted, words offered)."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    if not (isinstance(words, np.ndarray) and words.dtype == np.uint32 and words.flags.c_contiguous and words.flags.writeable):
        raise TypeError("words: a writeable C-contiguous uint32 array")
    q = np.ascontiguousarray(np.frombuffer(seq, np.uint8) if isinstance(seq, (bytes, bytearray)) else seq, dtype=np.uint8)
    st = capi.ProjStat()
    lib = load()
    lib.gsah_c_project.restype = C.c_int
    lib.gsah_c_project.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(capi.Result), C.c_uint32, C.c_void_p, C.c_longlong, C.POINTER(capi.ProjStat)]
    rc = lib.gsah_c_project(index_prefix.encode(), C.c_void_p(q.ctypes.data), C.byref(result), int(flags), C.c_void_p(words.ctypes.data), int(words.size), C.byref(st))
    if rc < 0:
        raise RuntimeError(f"gsah_c_project -> {rc}")
    return int(st.n_blocks), int(st.n_cols)


def proj_text(words) -> bytes:
    """gsah_c_proj_text: accumulator words -> characters (codes 1..6: A C G T N -, word 0: n)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(max(int(w.size), 1), np.uint8)
    lib = load()
    lib.gsah_c_proj_text.restype = C.c_int
    lib.gsah_c_proj_text.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p]
    rc = lib.gsah_c_proj_text(C.c_void_p(w.ctypes.data), int(w.size), C.c_void_p(out.ctypes.data))
    if rc < 0:
        raise RuntimeError(f"gsah_c_proj_text -> {rc}")
    return out[:int(w.size)].tobytes()


def emit_proj(index_prefix, words) -> bytes:
    """gsah_c_emit_proj: the FASTA text -proj writes for the accumulator `words` (G entries): one record per reference sequence, 60 characters per line."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    lib = load()
    lib.gsah_c_emit_proj.restype = C.c_longlong
    lib.gsah_c_emit_proj.argtypes = [C.c_char_p, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong]
    n = lib.gsah_c_emit_proj(index_prefix.encode(), C.c_void_p(w.ctypes.data), int(w.size), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_emit_proj -> {n}")
    out = np.zeros(max(int(n), 1), np.uint8)
    n2 = lib.gsah_c_emit_proj(index_prefix.encode(), C.c_void_p(w.ctypes.data), int(w.size), C.c_void_p(out.ctypes.data), int(n))
    if n2 != n:
        raise RuntimeError(f"gsah_c_emit_proj -> {n2} after {n}")
    return out[:int(n)].tobytes()


def segs(index_prefix, seq, result):
    """gsah_c_segs: the chain triples of every block of one finished contig on the host, from the gapped strings and seed records, untrimmed -- what Aligner.block_segs
    computes on the GPU.  result: a capi.Result, a dump dict (oracle layout) or a result dict of capi.Aligner.  index_prefix and seq are not needed by the walk and may be
    None (kept for symmetry with cigars()).  Returns (SEG_BLOCK_DT array, SEG_DT array); block b's triples are seg[seg_off : seg_off + n_seg]."""
    keep: list = []
    if isinstance(result, dict):
        result = result_from_dump(result, keep) if "b_score" in result else result_from_arrays(result, keep)
    lib = load()
    lib.gsah_c_segs.restype = C.c_longlong
    lib.gsah_c_segs.argtypes = [C.POINTER(capi.Result), C.c_void_p, C.c_void_p, C.c_longlong]
    blk = np.zeros(int(result.n_blocks), capi.SEG_BLOCK_DT)
    n = lib.gsah_c_segs(C.byref(result), C.c_void_p(blk.ctypes.data), None, 0)
    if n < 0:
        raise RuntimeError(f"gsah_c_segs -> {n}")
    sg = np.zeros(int(n), capi.SEG_DT)
    if n:
        n2 = lib.gsah_c_segs(C.byref(result), C.c_void_p(blk.ctypes.data), C.c_void_p(sg.ctypes.data), n)
        assert n2 == n
    return blk, sg


def segs_trim(triples, bdir: bool, ext: int):
    """gsah_c_segs_trim: iExtension's trim on ONE block's triples (output order) -- the last `ext` columns in walk order go, and a gap the cut falls into or ends at goes
    whole.  Returns the SEG_DT array that stays (its last triple with dt = dq = 0)."""
    t = np.ascontiguousarray(triples, dtype=capi.SEG_DT)
    out = np.zeros(max(t.size, 1), capi.SEG_DT)
    lib = load()
    lib.gsah_c_segs_trim.restype = C.c_longlong
    lib.gsah_c_segs_trim.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p]
    n = lib.gsah_c_segs_trim(C.c_void_p(t.ctypes.data), int(t.size), 1 if bdir else 0, int(ext), C.c_void_p(out.ctypes.data))
    if n < 0:
        raise RuntimeError(f"gsah_c_segs_trim -> {n}")
    return out[:n].copy()


def cs_trim(cs_bytes, ops, bdir: bool, ext: int) -> bytes:
    """gsah_c_cs_trim: iExtension's trim on ONE block's cs string (of its untrimmed ops, output order) -- the last `ext` columns in walk order go, a cut ':n' is
    printed again.  Returns the string that stays: the cs of the trimmed ops."""
    b = np.frombuffer(cs_bytes.encode() if isinstance(cs_bytes, str) else bytes(cs_bytes), np.uint8)
    ops = np.ascontiguousarray(ops, dtype=np.uint32)
    out = np.zeros(max(b.size, 1), np.uint8)
    lib = load()
    lib.gsah_c_cs_trim.restype = C.c_longlong
    lib.gsah_c_cs_trim.argtypes = [C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong, C.c_int, C.c_longlong, C.c_void_p]
    n = lib.gsah_c_cs_trim(C.c_void_p(b.ctypes.data), int(b.size), C.c_void_p(ops.ctypes.data), int(ops.size), 1 if bdir else 0, int(ext), C.c_void_p(out.ctypes.data))
    if n < 0:
        raise RuntimeError(f"gsah_c_cs_trim -> {n}")
    return out[:n].tobytes()
