"""-m gpu: translate_dna_to_protein / Translate (csrc/translate.hip) against a plain Python translation of strings."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TABLE = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CUSTOM = "".join(chr(48 + i) for i in range(64))               # another letter for every codon
COMPLEMENT = str.maketrans("ACGTacgt", "TGCAtgca")


def reference(rows, table=TABLE, frame=0, reverse=False, unknown=None):
    codon = {a + b + c: table[16 * i + 4 * j + k] for i, a in enumerate("TCAG") for j, b in enumerate("TCAG")
             for k, c in enumerate("TCAG")}
    out = []
    for row in rows:
        s = (row[::-1].translate(COMPLEMENT) if reverse else row).upper()[frame:]
        out.append("".join(codon.get(s[i:i + 3], unknown) for i in range(0, len(s) - len(s) % 3, 3)))
    return out


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


def test_reference_goldens(bnp):
    translate = bnp.sequence.translate.Translate
    assert translate().window_size == 3
    assert translate().windowed(["TTTTTC", "GGG"]).tolist() == ["FF", "G"]
    entry = bnp.SequenceEntry(name=bnp.as_encoded_array(["seq1"]), sequence=bnp.as_encoded_array(["ACGTAT"]))
    protein = bnp.sequence.translate_dna_to_protein(entry)
    assert protein.sequence.tolist() == ["TY"] and protein.name.tolist() == ["seq1"]
    all_codons = "".join(a + b + c for a in "TCAG" for b in "TCAG" for c in "TCAG")
    assert bnp.sequence.translate_dna_to_protein(all_codons).to_string() == TABLE
    assert bnp.sequence.translate_dna_to_protein([all_codons], table=CUSTOM).tolist() == [CUSTOM]
    assert bnp.sequence.translate_dna_to_protein([], trim=True).tolist() == []
    assert bnp.sequence.translate_dna_to_protein(bnp.as_encoded_array([], bnp.DNAEncoding), trim=True).tolist() == []


@pytest.fixture(scope="module")
def shapes(bnp, tmp_path_factory):
    """one row set at the kernels' edges (a lane owns 16 codons = 48 bases, a packed word 32 bases, a tile 4096 codons), in
    the three input forms"""
    rng = random.Random(20261126)
    lengths = [0, 0, 1, 2, 3, 4, 5, 47, 48, 49, 50, 51, 95, 96, 97] + [150] * 40 + [3] * 600 + [13000] + [151] * 40 + [0]
    rows = ["".join(rng.choice("ACGTacgt") for _ in range(n)) for n in lengths]
    path = tmp_path_factory.mktemp("translate") / "rows.fa"
    path.write_text("".join(">r%d\n%s\n" % (i, row) for i, row in enumerate(rows)))
    view = bnp.open(str(path), buffer_type=bnp.TwoLineFastaBuffer).read().sequence
    assert not view.is_compact()
    return rows, {"text": bnp.as_encoded_array(rows), "view": view, "packed": bnp.as_encoded_array(rows, bnp.DNAEncoding)}


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("frame", [0, 1, 2])
@pytest.mark.parametrize("form", ["text", "view", "packed"])
def test_shapes(bnp, shapes, form, frame, reverse):
    rows, forms = shapes
    got = bnp.sequence.translate_dna_to_protein(forms[form], frame=frame, reverse_complement=reverse, trim=True)
    assert got.encoding == bnp.BaseEncoding
    assert got.tolist() == reference(rows, frame=frame, reverse=reverse)


def test_strict_lengths(bnp):
    with pytest.raises(AssertionError):
        bnp.sequence.translate_dna_to_protein(["ACGACG", "ACGT"])
    assert bnp.sequence.translate_dna_to_protein(["ACGACG", "", "ACG"]).tolist() == ["TT", "", "T"]
    assert bnp.sequence.translate_dna_to_protein(["ACGACG", "ACGT"], trim=True).tolist() == ["TT", "T"]


# three rows of 20 codons: lane 0 owns the codons 0 .. 15 of row 0, lane 1 the rest of row 0 and the start of row 1
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("row,at", [(1, 1), (1, 58), (0, 47), (0, 48)],
                         ids=["first-codon", "last-codon", "before-lane-boundary", "behind-lane-boundary"])
def test_unknown_base(bnp, row, at, reverse):
    rng = random.Random(7)
    rows = ["".join(rng.choice("ACGT") for _ in range(60)) for _ in range(3)]
    rows[row] = rows[row][:at] + "N" + rows[row][at + 1:]
    with pytest.raises(bnp.EncodingError) as e:
        bnp.sequence.translate_dna_to_protein(rows, reverse_complement=reverse)
    assert e.value.offset == 60 * row + at
    got = bnp.sequence.translate_dna_to_protein(rows, reverse_complement=reverse, unknown="X").tolist()
    assert got == reference(rows, reverse=reverse, unknown="X") and "".join(got).count("X") == 1


def test_unknown_base_outside_the_codons(bnp):
    assert bnp.sequence.translate_dna_to_protein(["ACGAN", "ACG"], trim=True).tolist() == ["T", "T"]
    assert bnp.sequence.translate_dna_to_protein(["NACG"], frame=1, trim=True).tolist() == ["T"]
    assert bnp.sequence.translate_dna_to_protein(["NACGT"], reverse_complement=True, trim=True).tolist() == ["T"]


def test_abi_argument_checks(bnp):
    from bionumpy_amd import _native
    from bionumpy_amd.device import HArray, ptr
    ops = bnp.ops.get_ops()
    text = HArray(host=np.frombuffer(b"ACGTAT" + b"A" * 58, dtype=np.uint8)).dev()
    in_off, out_off = HArray(host=np.array([0, 6])).dev(), HArray(host=np.array([0, 2])).dev()
    out, cell, table = ops._empty(16, np.uint8), ops._err_cell(), (C.c_uint8 * 64)(*TABLE.encode())

    def call(frame=0, d_out=out, n_rows=1):
        return _native.lib.bnpk_translate_rows(ops.ctx, ptr(text), 64, None, ptr(in_off), n_rows, 6, ptr(out_off), 2, table,
                                               frame, 0, 0, ptr(cell), ptr(d_out), ops._s())
    assert call(frame=3) == -1                                # BNPK_ERR_ARG
    assert call(d_out=text) == -1
    assert call(n_rows=0) == 0
    assert call() == 0 and bytes(out.cpu().numpy()[:2]) == b"TY"
