"""gsah_reference_from_fasta (hostlib.reference_from_fasta): the FASTA half of the index builder without the index -- the .pac bytes, the sequence
names and lengths -- against the golden index files and against what the builder itself writes for a FASTA with every parsing case.  It touches no
file but the FASTA.  Every comparison is exact."""
import os

import numpy as np
import pytest

from gsalign_amd import hostlib, indexio


@pytest.fixture(scope="module", autouse=True)
def built():
    hostlib.build()


def _ann(prefix):
    idx_lines = open(prefix + ".ann").read().split("\n")
    G, n = int(idx_lines[0].split()[0]), int(idx_lines[0].split()[1])
    names = [idx_lines[1 + 2 * k].split()[1] for k in range(n)]
    lens = [int(idx_lines[2 + 2 * k].split()[1]) for k in range(n)]
    return G, names, lens


@pytest.mark.parametrize("name", ["cx", "small"])
def test_golden_pac_and_ann(golden_dir, name):
    before = sorted(os.listdir(golden_dir))
    pac, G, names, lens = hostlib.reference_from_fasta(os.path.join(golden_dir, name + ".ref.fa"))
    assert sorted(os.listdir(golden_dir)) == before
    want_G, want_names, want_lens = _ann(os.path.join(golden_dir, name))
    assert G == want_G and names == want_names and lens.tolist() == want_lens and lens.dtype == np.int32
    want = np.fromfile(os.path.join(golden_dir, name + ".pac"), dtype=np.uint8)[:(G + 3) // 4]
    assert pac.dtype == np.uint8 and pac.size == (G + 3) // 4 and np.array_equal(pac, want)


# two contigs; a header comment; lower case; IUPAC letters; N runs at a contig's start and end and across a 4-base boundary (bases 7..10 of the first contig); the run that
# ends the first contig is followed by the run that starts the second
FASTA = (">one a comment with blanks\r\n"
         "NNNacgtNNNNRYKMacgtacgtacgtTTGACCA\r\n"
         "ggcatSWBDHVnacgtacgtacgNNN\n"
         ">two\n"
         "NNacgtacgtaccgtXacgtacgtnnNN\n"
         "ACGTACGGTN\n")


def test_fasta_cases_against_the_builder(tmp_path, monkeypatch):
    monkeypatch.setenv("GSA_INDEX_THREADS", "1")
    d = tmp_path / "ref"; d.mkdir()
    fa = str(d / "r.fa")
    with open(fa, "w", newline="") as fh:
        fh.write(FASTA)
    before = sorted(os.listdir(d))
    pac, G, names, lens = hostlib.reference_from_fasta(fa)
    assert sorted(os.listdir(d)) == before == ["r.fa"]
    assert names == ["one", "two"] and lens.tolist() == [60, 38] and G == 98
    out = tmp_path / "idx"; out.mkdir()
    hostlib.build_index(fa, str(out / "r"))
    want_G, want_names, want_lens = _ann(str(out / "r"))
    assert (G, names, lens.tolist()) == (want_G, want_names, want_lens)
    assert np.array_equal(pac, np.fromfile(str(out / "r.pac"), dtype=np.uint8)[:(G + 3) // 4])
    idx = indexio.load_index(str(out / "r"))
    assert np.array_equal(indexio.unpack_pac(pac, G), idx.ref)
    # a second call gives the same bytes (srand48(11) starts every call)
    pac2, G2, names2, lens2 = hostlib.reference_from_fasta(fa)
    assert G2 == G and names2 == names and np.array_equal(pac2, pac) and np.array_equal(lens2, lens)


def test_unreadable_fasta_is_an_error(tmp_path):
    with pytest.raises(RuntimeError, match="cannot read FASTA"):
        hostlib.reference_from_fasta(str(tmp_path / "missing.fa"))
    assert os.listdir(tmp_path) == []
