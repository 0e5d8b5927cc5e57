"""Seed-and-vote read placement on the MI355X path (csrc/seeds.hip, ``bnpk_seed_*``).

``SeedIndex.from_sequences(reference, k)`` keeps, for every k-mer of a DNA reference, where it starts; ``place_reads(reads,
index)`` looks up the k-mers of every read and of its reverse complement, lets the hits vote for the diagonal the read would
start at, and gives per read the strand, the reference row and the position of the locus with the most votes;
``Placements.windows(reads, pad)`` cuts the stretch of reference around every placed read, ready as ``targets`` of
``align_pairs``.  Hits, votes, the winner among equals and the windows are those written into include/bnpk.h.
"""
from ..encoded_array import EncodedArray, EncodedRaggedArray, DNAEncoding, as_encoded_array, packed_words, _PackedDna
from .. import _native
from ..ops import get_ops


def _dna_rows(sequences, what):
    """compact rows under DNAEncoding (a chunk gives its ``.sequence``, text is encoded); any other encoding is a ValueError"""
    from ..datatypes import SequenceEntry
    if isinstance(sequences, SequenceEntry):
        sequences = sequences.sequence
    if not isinstance(sequences, (EncodedArray, EncodedRaggedArray)):
        sequences = as_encoded_array(sequences, DNAEncoding)
    if isinstance(sequences, EncodedArray):
        sequences = EncodedRaggedArray(sequences.ravel(), [sequences.size])
    if not (hasattr(sequences.encoding, "_is_dna") and sequences.encoding._is_dna()):
        raise ValueError("%s under %s: seeds are placed over DNAEncoding only (strands need a complement)" % (what, sequences.encoding))
    sequences._compact()
    return sequences


class SeedIndex:
    """the k-mer position index of a reference, in HBM, and the reference itself: ``keys`` (the distinct k-mers, ascending),
    ``starts`` and ``positions`` (``positions[starts[u]:starts[u + 1]]``: the global start coordinates of key u, ascending; the
    global coordinate of position x of row r is ``reference.offsets()[r] + x``) as DeviceVectors; ``len(index)`` distinct k-mers"""

    def __init__(self, k, reference, parts):
        from ..device_vector import DeviceVector
        self.k, self.reference, self._parts = k, reference, parts
        self.keys, self.starts, self.positions = (DeviceVector(p) for p in parts[:3])

    @classmethod
    def from_sequences(cls, reference, k=15):
        """``reference``: an EncodedRaggedArray under DNAEncoding, a chunk or a list of strings, fewer than 2^31 - 512 bases
        in all; 8 <= ``k`` <= 31"""
        if not _native.SEED_MIN_K <= k <= _native.SEED_MAX_K:
            raise ValueError("k must lie in %d .. %d" % (_native.SEED_MIN_K, _native.SEED_MAX_K))
        rows = _dna_rows(reference, "a reference")
        if rows.total() >= 2 ** 31 - _native.SEED_MAX_LEN:
            raise ValueError("a reference of %d bases: the index holds fewer than 2^31 - %d" % (rows.total(), _native.SEED_MAX_LEN))
        words = packed_words(rows._data) if rows.total() else None
        return cls(int(k), rows, get_ops().seed_index(words, rows.offsets(), rows._lens, len(rows), rows.total(), int(k)))

    def __len__(self):
        return len(self.keys)

    def __repr__(self):
        return "%d-mer SeedIndex of %d sequences, %d distinct k-mers" % (self.k, len(self.reference), len(self))


class ReferenceWindows:
    """what ``Placements.windows`` returns: ``sequences`` (an EncodedRaggedArray under DNAEncoding, one window per read, empty
    for an unplaced one, reverse complemented for strand 1) and ``start`` (int32 DeviceVector: where the window starts in its
    reference row, before the reverse complement)"""

    def __init__(self, sequences, start):
        self.sequences, self.start = sequences, start


class Placements:
    """what ``place_reads`` returns, one entry per read and in HBM until looked at (DeviceVectors of int32): ``strand`` (0, 1 for
    the reverse complement, -1 unplaced), ``row`` and ``position`` (where the read, or its reverse complement, starts in that
    reference row; negative when it hangs over the row's start), ``votes`` and ``second`` (the winner's and the runner-up's
    hits); ``is_placed`` is the device mask ``strand >= 0``"""

    def __init__(self, parts, index):
        from ..device_vector import DeviceVector
        self.votes, self.second, self.strand, self.row, self.position = (DeviceVector(p) for p in parts)
        self.is_placed = self.strand >= 0
        self._index = index

    def __len__(self):
        return len(self.strand)

    def windows(self, reads, pad=24):
        """the reference around every placed read, ``pad`` bases more on either side and clamped to the row: a
        ``ReferenceWindows``.  For ``strand == 1`` the window is reverse complemented, so ``align_pairs(reads, w.sequences)``
        gives target coordinates in the reverse-complemented window"""
        from ..device_vector import DeviceVector
        if pad < 0:
            raise ValueError("pad must not be negative")
        rows, ref = _dna_rows(reads, "reads"), self._index.reference
        if len(rows) != len(self):
            raise ValueError("%d reads and %d placements" % (len(rows), len(self)))
        words, lens, offsets, total, start = get_ops().seed_windows(
            packed_words(ref._data) if ref.total() else None, ref.offsets(), len(ref), self.strand.harray(), self.row.harray(),
            self.position.harray(), rows.offsets(), len(rows), pad)
        sequences = EncodedRaggedArray._from_parts(_PackedDna(words, total), None, lens, offsets, len(rows), total, DNAEncoding)
        return ReferenceWindows(sequences, DeviceVector(start))


def place_reads(reads, index, max_occurrences=8, band=16, min_votes=2):
    """Places every read on the index's reference: a ``Placements``.  ``reads``: an EncodedRaggedArray under DNAEncoding, a
    chunk or a list of strings, rows of up to 512 bases.  A k-mer that occurs more than ``max_occurrences`` times in the
    reference is not used; hits whose diagonals fall into two neighbouring bins of ``band`` (a power of two up to 256) bases
    count for one locus; a read is placed when its best locus has at least ``min_votes`` hits.  A read with more than 4096
    possible hits (2 x k-mers x ``max_occurrences``) raises NotImplementedError."""
    if not 1 <= max_occurrences <= _native.SEED_MAX_OCCURRENCES:
        raise ValueError("max_occurrences must lie in 1 .. %d" % _native.SEED_MAX_OCCURRENCES)
    if not 1 <= band <= _native.SEED_MAX_BAND or band & (band - 1):
        raise ValueError("band must be a power of two in 1 .. %d" % _native.SEED_MAX_BAND)
    if min_votes < 1:
        raise ValueError("min_votes must be at least 1")
    rows, ref = _dna_rows(reads, "reads"), index.reference
    parts = get_ops().seed_place(packed_words(rows._data) if rows.total() else None, rows.offsets(), rows.total(), len(rows),
                                 index._parts, ref.offsets(), len(ref), index.k, max_occurrences, band, min_votes)
    return Placements(parts, index)
