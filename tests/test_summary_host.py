"""CPU tests of the PAF emitter on SUMMARY results (ContigResult::summary): a ContigResult that holds only the blocks and
the first / last record of every block, with the CIGARs supplied, must give the PAF bytes the full result gives (no GPU needed)."""
import os

import pytest

import paf_from_maf as pm
from gsalign_amd import hostlib, indexio, synth
from test_cigars_host import overrun_case      # noqa: F401  (fixture)


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


@pytest.mark.parametrize("name,params,maf", [("cx", {}, "cx.maf"), ("cx", dict(sen=1, clr=50), "cx_sen.maf"), ("small", {}, "small.maf")])
def test_summary_paf_is_the_reference_maf(oracle_built, golden_dir, tmp_path, name, params, maf):
    """blocks + block ends + comparator CIGARs of the oracle's stage-8 dumps -> exactly the PAF the reference's MAF implies; no VCF is written"""
    px = os.path.join(golden_dir, name)
    o = oracle_built.Oracle(indexio.load_index(px), params)

    def per_contig(ci, seq):
        o.set_query(seq); o.run_to(8)
        return o.blocks(with_aln=True)

    out_paf, out_vcf = str(tmp_path / "o.paf"), str(tmp_path / "o.vcf")
    hostlib.emit(px, px + ".qry.fa", out_paf, out_vcf, name, per_contig, fmt=3, summary=True)
    o.close()
    got = open(out_paf, "rb").read()
    assert len(got) > 1000 and got == pm.paf_of_maf(os.path.join(golden_dir, maf))
    assert not os.path.exists(out_vcf)


@pytest.mark.parametrize("allow_dup", [True, False])
def test_summary_paf_trims_like_the_full_result(overrun_case, tmp_path, allow_dup):
    """iExtension on the ends: the PAF from blocks + ends == the PAF the full-result emitter writes, for all six hand-made blocks.  Two of them END IN A GAP
    record, which the library never produces (a block is seed [gap] seed ... seed, and the ends format says both ends are seeds); the ends format still
    expresses them here because those blocks have exactly two records, so the seed a gap record is expanded against is the block's first end."""
    px, qfa, qry, dump = overrun_case
    assert [int(n) for n, s in zip(dump["b_nfrag"], dump["b_score"])] == [3, 2, 3, 2, 1, 3]
    cp = lambda: {k: v.copy() for k, v in dump.items()}
    hostlib.emit(px, qfa, str(tmp_path / "full.paf"), str(tmp_path / "full.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3)
    hostlib.emit(px, qfa, str(tmp_path / "sum.paf"), str(tmp_path / "sum.vcf"), "r", lambda ci, seq: cp(), allow_dup=allow_dup, fmt=3, summary=True)
    want = open(tmp_path / "full.paf", "rb").read()
    assert want.count(b"\n") == (6 if allow_dup else 5)
    assert open(tmp_path / "sum.paf", "rb").read() == want


def test_summary_needs_fmt3(tmp_path):
    with pytest.raises(ValueError):
        hostlib.emit("x", "y", str(tmp_path / "o"), str(tmp_path / "v"), "r", lambda ci, seq: {}, fmt=1, summary=True)
