"""Paired-end read merging on the MI355X path (csrc/mates.hip, ``bnpk_mates_*``).

Row i of ``mates1`` and row i of ``mates2`` are the two reads of one fragment.  ``find_mate_overlaps`` finds per pair the
offset at which mate 1 and the reverse complement of mate 2 overlap best — the largest overlap within the mismatch limits,
then the fewest mismatches, then the smallest offset — and with it the fragment's length; ``merge_pairs`` writes the pairs
that overlap as one read each, with consensus bases and qualities.  A fragment shorter than a read (adapter read-through)
is found the same way, without knowing the adapter.  The semantics are those written into include/bnpk.h.
"""
from ..encoded_array import EncodedRaggedArray, ACGTnEncoding, packed_words
from ..ragged import RaggedArray
from .. import _native
from ..ops import get_ops
from .approximate import _alphabet_rows


class MateOverlaps:
    """what ``find_mate_overlaps`` returns, one entry per pair and in HBM until looked at (DeviceVectors: ``length >= 0`` is a
    mask on the device): ``length`` (int64: the fragment's length, -1 where the mates do not overlap well enough), ``overlap``
    (int32: the columns both mates cover, 0 where none) and ``mismatches`` (int32: those in which they differ)"""

    def __init__(self, parts):
        from ..device_vector import DeviceVector
        self.length, self.overlap, self.mismatches = (DeviceVector(p) for p in parts)

    def __len__(self):
        return len(self.length)


class MergedPairs:
    """what ``merge_pairs`` returns: ``merged`` (the pairs that merged, as one read each: a chunk where chunks went in, else
    the sequences), ``is_merged`` (the device mask over all pairs: the others are ``mates1[~is_merged]`` and
    ``mates2[~is_merged]``) and ``overlaps`` (the ``MateOverlaps``)"""

    def __init__(self, merged, is_merged, overlaps):
        self.merged, self.is_merged, self.overlaps = merged, is_merged, overlaps


def _mate_rows(mates1, mates2):
    """(rows1, rows2, packed): both sides compact under one encoding, ACGT (2-bit words) or ACGTn (code bytes)"""
    from ..datatypes import SequenceEntry
    sides = [_alphabet_rows(m.sequence if isinstance(m, SequenceEntry) else m) for m in (mates1, mates2)]
    for rows in sides:
        if not rows.encoding._is_dna() and "".join(rows.encoding.get_alphabet()).upper() != "ACGTN":
            raise NotImplementedError("mates over ACGT or ACGTn are merged, not over %s" % "".join(rows.encoding.get_alphabet()))
    if len(sides[0]) != len(sides[1]):
        raise ValueError("%d first mates and %d second mates: row i of one is the mate of row i of the other"
                         % (len(sides[0]), len(sides[1])))
    packed = all(rows.encoding._is_dna() for rows in sides)
    for i, rows in enumerate(sides):
        rows._compact()
        if not packed and rows.encoding._is_dna():           # (the codes of A, C, G and T are the same under both)
            sides[i] = EncodedRaggedArray._from_parts(rows._as_plain(rows._data), None, rows._lens, rows._offsets, len(rows),
                                                      rows._total, ACGTnEncoding)
    return sides[0], sides[1], packed


def _check(min_overlap, max_mismatches, max_mismatch_percent, quality_cap=41):
    if min_overlap < 1:
        raise ValueError("min_overlap must be at least 1")
    if max_mismatches < 0:
        raise ValueError("max_mismatches must not be negative")
    if not 0 <= max_mismatch_percent <= 100:
        raise ValueError("max_mismatch_percent must lie in 0 .. 100")
    if not 0 <= quality_cap <= 93:
        raise ValueError("quality_cap must lie in 0 .. 93")


def _overlaps(rows1, rows2, packed, min_overlap, max_mismatches, max_mismatch_percent, read_through):
    data = [packed_words(rows._data) if packed else rows._as_plain(rows._data) for rows in (rows1, rows2)]
    limit = min(int(max_mismatches), _native.MATES_MAX_LEN)  # (no pair has more mismatches than symbols)
    parts = get_ops().mates_overlap(data[0], rows1.offsets(), rows1.total(), data[1], rows2.offsets(), rows2.total(), len(rows1),
                                    min_overlap, limit, max_mismatch_percent, read_through, packed)
    return MateOverlaps(parts), data


def find_mate_overlaps(mates1, mates2, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, read_through=True):
    """Where the mates of every pair overlap: a ``MateOverlaps``.  ``mates1``, ``mates2``: EncodedRaggedArrays over ACGT or
    ACGTn, chunks (their ``.sequence``) or lists of strings, with as many rows each; mate 2 as it was read (it is reverse
    complemented on the fly).  An offset counts when at least ``min_overlap`` columns overlap, at most ``max_mismatches`` of
    them differ and at most ``max_mismatch_percent`` percent; an N differs from everything.  ``read_through=False`` leaves
    out the offsets at which a mate runs past the other's start (fragments shorter than a read)."""
    _check(min_overlap, max_mismatches, max_mismatch_percent)
    rows1, rows2, packed = _mate_rows(mates1, mates2)
    return _overlaps(rows1, rows2, packed, min_overlap, max_mismatches, max_mismatch_percent, read_through)[0]


def merge_pairs(mates1, mates2, min_overlap=30, max_mismatches=5, max_mismatch_percent=20, read_through=True, quality_cap=41):
    """Merges every pair whose mates overlap (``find_mate_overlaps``) into one read: a ``MergedPairs``.  Where both mates cover
    a column and agree the qualities add up (to ``quality_cap`` at most); where they differ the base of the higher quality
    stands — mate 1's on a tie — with the difference as its quality; a letter beats an N.  Two ``SequenceEntryWithQuality``
    chunks give a chunk of merged reads under mate 1's names; anything else gives the merged sequences."""
    from ..datatypes import SequenceEntry, replace
    _check(min_overlap, max_mismatches, max_mismatch_percent, quality_cap)
    rows1, rows2, packed = _mate_rows(mates1, mates2)
    overlaps, data = _overlaps(rows1, rows2, packed, min_overlap, max_mismatches, max_mismatch_percent, read_through)
    chunks = isinstance(mates1, SequenceEntry) and isinstance(mates2, SequenceEntry)
    quals = [None, None]
    if chunks and ("quality" in mates1._fields) != ("quality" in mates2._fields):
        raise ValueError("one chunk of mates has qualities and the other has none")
    if chunks and "quality" in mates1._fields:
        quals = [m.quality for m in (mates1, mates2)]
        for q in quals:
            q._compact()
        quals = [q._data for q in quals]
    ops = get_ops()
    codes, qual, _, total = ops.mates_merge(data[0], rows1.offsets(), quals[0], data[1], rows2.offsets(), quals[1], len(rows1),
                                            overlaps.length.harray(), quality_cap, packed)
    is_merged = overlaps.length >= 0
    picked = is_merged.nonzero_rows()
    lens = ops.take_i64(overlaps.length.harray(), picked)    # the merged rows lie back to back: the others wrote nothing
    sequence = EncodedRaggedArray._from_parts(codes, None, lens, None, picked.size, total, rows1.encoding)
    if not chunks:
        return MergedPairs(sequence, is_merged, overlaps)
    fields = {"sequence": sequence}
    if qual is not None:
        fields["quality"] = RaggedArray._from_parts(qual, None, lens, None, picked.size, total)
    return MergedPairs(replace(mates1[is_merged], **fields), is_merged, overlaps)
