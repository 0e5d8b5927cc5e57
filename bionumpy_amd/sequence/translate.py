"""DNA -> protein on the MI355X path (bionumpy/sequence/translate.py).

``translate_dna_to_protein(sequence)`` / ``Translate().windowed(sequences)``: every row of bases becomes a row of amino-acid
letters (``BaseEncoding``), three bases per letter, through the reference's 64-letter table (index 16 c0 + 4 c1 + c2 with
T C A G = 0 1 2 3).  The kernels (``csrc/translate.hip``) take the input as it lies in HBM — 2-bit DNA stays packed, a
sequence column of a text chunk is translated where it lies, not gathered first — and give what the reference cannot:
a reading ``frame`` (0, 1, 2), the reverse strand, and rows whose length is no multiple of three (``trim=True``).
"""
import numpy as np

from ..encoded_array import (EncodedArray, EncodedRaggedArray, BaseEncoding, AlphabetEncoding, as_encoded_array,
                             packed_words)
from ..ops import get_ops
from ..streams import streamable


class DNAToProtein:
    """the codon table (translate.py:12-20); ``DNAToProtein(amino_acids=...)`` is another genetic code in the same order"""
    amino_acids = 'FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG'
    from_encoding = AlphabetEncoding("TCAG")
    to_encoding = BaseEncoding

    def __init__(self, amino_acids=None):
        if amino_acids is not None:
            assert len(amino_acids) == 64, "a codon table has 64 letters"
            self.amino_acids = str(amino_acids)

    def _letters(self):
        return np.frombuffer(self.amino_acids.encode("ascii"), dtype=np.uint8)


def _check_encoding(encoding):
    """the input forms the kernels cover, told apart the way get_reverse_complement does"""
    if encoding == BaseEncoding:
        return "ascii"
    if isinstance(encoding, AlphabetEncoding):
        alphabet = "".join(encoding.get_alphabet()).upper()
        if alphabet == "ACGT":
            return "dna"
        for c in alphabet:
            if c not in "ACGT":
                raise KeyError(c)
        return "alphabet"                                    # the same four letters in another order: by way of the letters
    raise ValueError("Invalid encoding for translation: %s" % (encoding,))


class Translate:
    """translate.py:23-48, plus ``frame`` (0, 1, 2: bases skipped in front of the first codon), ``reverse_complement`` (the
    codons of the row's reverse complement), ``trim`` (False: a row of ``(length - frame) % 3 != 0`` is an AssertionError, the
    reference's contract; True: the bases behind the last codon are dropped) and ``unknown`` (None: a byte other than
    A C G T inside a translated codon is an EncodingError carrying its flat offset; a letter: that codon's amino acid)"""

    def __init__(self, table=None, frame=0, reverse_complement=False, trim=False, unknown=None):
        if table is None or isinstance(table, str):
            table = DNAToProtein(table)
        assert frame in (0, 1, 2), "frame is 0, 1 or 2"
        assert unknown is None or (isinstance(unknown, str) and len(unknown) == 1 and 0 < ord(unknown) < 128)
        self._table = table
        self._encoding = table.from_encoding
        self._frame, self._reverse, self._trim = int(frame), bool(reverse_complement), bool(trim)
        self._unknown = 0 if unknown is None else ord(unknown)

    @property
    def window_size(self):
        return 3

    def windowed(self, sequences):
        sequences = as_encoded_array(sequences)
        kind = _check_encoding(sequences.encoding)
        single = isinstance(sequences, EncodedArray)
        ragged = EncodedRaggedArray(sequences.ravel(), [sequences.size]) if single else sequences
        if kind == "alphabet":
            ragged = sequences.encoding.decode(ragged)
        ops = get_ops()
        n_rows, total, offsets = len(ragged), ragged.total(), ragged.offsets()
        out_lens, out_offsets, n_out, n_partial = ops.translate_plan(offsets, n_rows, self._frame)
        assert self._trim or n_partial == 0, \
            "%d sequence(s) whose length behind frame %d is no multiple of 3 (trim=True drops the rest)" % (n_partial, self._frame)
        letters = self._table._letters()
        if kind == "dna":
            ragged._compact()
            out = ops.translate_packed(packed_words(ragged._data), offsets, n_rows, total, out_offsets, n_out, letters,
                                       self._frame, self._reverse)
        else:                                                # (a column of a text chunk is read through its row starts)
            out = ops.translate_rows(ragged._flat_data(), ragged._starts, offsets, n_rows, total, out_offsets, n_out, letters,
                                     self._frame, self._reverse, self._unknown)
        if single:
            return EncodedArray(out, self._table.to_encoding)
        return EncodedRaggedArray._from_parts(out, None, out_lens, out_offsets, n_rows, n_out, self._table.to_encoding)

    __call__ = windowed


@streamable()
def translate_dna_to_protein(sequence, table=None, frame=0, reverse_complement=False, trim=False, unknown=None):
    """Translate DNA to protein (translate.py:51-77).  ``sequence``: str, list of str, EncodedArray, EncodedRaggedArray
    (ASCII or DNA-encoded), or an entry object with a ``sequence`` field (SequenceEntry, a FASTA / FASTQ chunk), which
    comes back with that field replaced.  Keywords: see ``Translate``."""
    translate = Translate(table, frame, reverse_complement, trim, unknown)
    if hasattr(sequence, "_replace") and hasattr(sequence, "sequence"):
        return sequence._replace(sequence=translate.windowed(sequence.sequence))
    return translate.windowed(sequence)
