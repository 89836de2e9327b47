"""CPU tests of the variant records (gsa_variant, include/gsa_hip.h): the header's allele helper against its numpy form, the record
layout, and the host walk gsah_c_variants -- the comparator of the GPU pass -- pinned to the REFERENCE's own VCF files through the
oracle's finished blocks (no GPU needed)."""
import ctypes as C
import os
import subprocess
from collections import Counter

import numpy as np
import pytest

from conftest import ROOT
from gsalign_amd import capi, hostlib, indexio, synth


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def test_variant_record_layout(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include "gsa_hip.h"\nint sz(void) { return (int)sizeof(gsa_variant); }\nint sz2(void) { return (int)sizeof(gsa_variants); }\n')
    so = tmp_path / "s.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    assert x.sz() == 32 == capi.VARIANT_DT.itemsize == C.sizeof(capi.Variant)
    assert x.sz2() == C.sizeof(capi.Variants) == 40


def test_variant_alleles_like_the_header(tmp_path):
    """gsa_variant_alleles compiled from the header as plain C99 against capi.variant_alleles, on hand-made records of all five kinds."""
    src = tmp_path / "x.c"
    src.write_text('#include <string.h>\n#include "gsa_hip.h"\n'
                   'void alleles(const gsa_variant *v, const char *ref, const char *query, char *r_out, char *a_out, uint32_t *n)\n'
                   '{ const char *rp, *ap; gsa_variant_alleles(v, ref, query, &rp, &n[0], &ap, &n[1]); memcpy(r_out, rp, n[0]); memcpy(a_out, ap, n[1]); }\n')
    so = tmp_path / "x.so"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(so)], check=True)
    x = C.CDLL(str(so))
    ref = np.frombuffer(b"ACGTTGCAAGGCTTAACCGGTTAACCGGATATCGCGATTACAGATTACAGGGCCCAAATTTGGGC", np.uint8)
    qry = np.frombuffer(b"TTGACCATGCATGCCCGGGAAATTTACGTACGTAGCTAGCTAGGATCCGGAATTCCTTAAGGCCA", np.uint8)
    #                rpos qpos len chr pos kind block
    V = np.array([(10, 20, 0, 0, 11, 0, 0), (5, 7, 3, 0, 6, 1, 0), (30, 2, 4, 1, 31, 2, 1), (40, 33, 2, 1, 41, 3, 2), (50, 12, 6, 0, 51, 4, 2), (0, 0, 1, 0, 1, 3, 0)], capi.VARIANT_DT)
    want = capi.variant_alleles(V, ref, qry)
    assert [(len(r), len(a)) for r, a in want] == [(1, 1), (1, 4), (5, 1), (1, 3), (7, 1), (1, 2)]
    rb, qb = ref.tobytes(), qry.tobytes()
    for i in range(V.size):
        r_out, a_out, n = C.create_string_buffer(16), C.create_string_buffer(16), (C.c_uint32 * 2)()
        x.alleles(C.c_void_p(V[i:i + 1].ctypes.data), rb, qb, r_out, a_out, n)
        assert (r_out.raw[:n[0]], a_out.raw[:n[1]]) == want[i], i
    # kind 3 takes its REF byte from the QUERY (the reference's own quirk), kind 4 its ALT from the reference
    assert want[3][0] == qb[33:34] and want[4][1] == rb[50:51]


def vcf_tuples(path):
    out = []
    for ln in open(path, "rb").read().split(b"\n"):
        if ln and not ln.startswith(b"#"):
            f = ln.split(b"\t")
            out.append((f[0], int(f[1]), f[3], f[4], f[7]))
    return out


def record_tuples(V, idx, names, query):
    al = capi.variant_alleles(V, idx.ref, query)
    return [(names[int(v["chr"])], int(v["pos"]), r, a, b"TYPE=" + capi.VCF_TYPE[int(v["kind"])].encode()) for v, (r, a) in zip(V, al)]


def chr_names(prefix):
    lines = open(prefix + ".ann").read().split("\n")
    n = int(lines[0].split()[1])
    return [lines[1 + 2 * i].split()[1].encode() for i in range(n)]


@pytest.mark.parametrize("name,params,vcf", [("cx", {}, "cx.vcf"), ("cx", dict(sen=1, clr=50), "cx_sen.vcf"), ("small", {}, "small.vcf")])
def test_host_variant_records_give_the_reference_vcf(oracle_built, golden_dir, name, params, vcf):
    """Records -> alleles -> (chrom, pos, ref, alt, type), as a sorted multiset against the body lines of the reference's VCF, plus the three counts."""
    px = os.path.join(golden_dir, name)
    idx = indexio.load_index(px)
    names = chr_names(px)
    o = oracle_built.Oracle(idx, params)
    got, counts, kinds, rev = [], np.zeros(3, np.int64), Counter(), 0
    for _, seq in synth.read_fasta(os.path.join(golden_dir, f"{name}.qry.fa")):
        o.set_query(seq); o.run_to(8)
        V, cnt = hostlib.variants(px, seq, o.blocks(with_aln=True))
        assert sum(cnt) == V.size
        assert (np.bincount(np.array([0, 1, 2, 1, 2])[V["kind"]], minlength=3) == np.array(cnt)).all()
        got += record_tuples(V, idx, names, seq); counts += np.array(cnt); kinds.update(V["kind"].tolist()); rev += int((V["rpos"] >= idx.G).sum())
    o.close()
    want = vcf_tuples(os.path.join(golden_dir, vcf))
    assert sorted(got) == sorted(want)
    t = Counter(w[4] for w in want)
    assert counts.tolist() == [t[b"TYPE=SUBSTITUTE"], t[b"TYPE=INSERT"], t[b"TYPE=DELETE"]]
    # (what the GPU parity test stands on: every input has variants on the reverse strand, and cx -sen every kind -- the default runs have no pure-deletion record)
    assert rev > 0 and set(kinds) >= {0, 1, 3, 4}, (kinds, rev)
    if params:
        assert set(kinds) == {0, 1, 2, 3, 4}, kinds
