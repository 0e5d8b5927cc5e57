"""Approximate pattern search and adapter trimming on the MI355X path (csrc/approx.hip, ``bnpk_approx_rows_*``).

``find_approximate(sequences, patterns, max_errors)`` answers per (pattern, row) whether the pattern occurs in the row with at
most ``max_errors`` substitutions, insertions and deletions, where the best occurrence lies and how many errors it has; with
``min_overlap`` a pattern may also run off the 3' end of a row, its error budget scaled to the part that is there.  The
semantics are those written into include/bnpk.h.  ``trim_adapters`` cuts every read where its adapter starts.
"""
import numpy as np

from ..encoded_array import (EncodedArray, EncodedRaggedArray, AlphabetEncoding, DNAEncoding, ACGTnEncoding, as_encoded_array,
                             packed_words)
from ..exceptions import EncodingError
from .. import _native
from ..ops import get_ops
from .position_weight_matrix import _MotifRows


class ApproxScan:
    """what ``find_approximate`` returns, each n_patterns x n_rows and in HBM until looked at: ``distance`` (uint8), ``start``
    and ``end`` (int64, -1 where the pattern was not found), ``overlap`` (uint8: the pattern's positions that lie in the row,
    0 where not found) and, if asked for, ``n_hits`` (int64: the end positions within ``max_errors``)"""

    def __init__(self, parts, n_patterns, n_rows):
        dist, start, end, overlap, hits = parts
        self.distance = _MotifRows(dist, n_patterns, n_rows)
        self.start = _MotifRows(start, n_patterns, n_rows)
        self.end = _MotifRows(end, n_patterns, n_rows)
        self.overlap = _MotifRows(overlap, n_patterns, n_rows)
        self.n_hits = None if hits is None else _MotifRows(hits, n_patterns, n_rows)


def _masks(pattern, alphabet):
    """uint64 per code: bit i is set iff position i of the pattern accepts the code (``.`` accepts every code)"""
    masks = np.zeros(len(alphabet), dtype=np.uint64)
    for i, letter in enumerate(pattern):
        if letter == ".":
            masks |= np.uint64(1 << i)
        elif letter.upper() in alphabet:
            masks[alphabet.index(letter.upper())] |= np.uint64(1 << i)
        else:
            raise ValueError("%r of pattern %r is no letter of the alphabet %s" % (letter, pattern, "".join(alphabet)))
    return masks


def _alphabet_rows(sequences):
    """the rows as an EncodedRaggedArray under an AlphabetEncoding; text becomes ACGT, or ACGTn where it holds other letters"""
    if not isinstance(sequences, (EncodedArray, EncodedRaggedArray)):
        sequences = as_encoded_array(sequences)
    if not isinstance(sequences.encoding, AlphabetEncoding):
        try:
            sequences = as_encoded_array(sequences, DNAEncoding)
        except EncodingError:
            sequences = as_encoded_array(sequences, ACGTnEncoding)
    if isinstance(sequences, EncodedArray):
        sequences = EncodedRaggedArray(sequences.ravel(), [sequences.size])
    return sequences


def find_approximate(sequences, patterns, max_errors, min_overlap=0, count_hits=False):
    """The best occurrence of every pattern in every row under the edit distance: an ``ApproxScan``.  ``patterns``: one string
    or a list of strings over the sequences' alphabet, ``.`` for a position that accepts everything; ``max_errors``: one int or
    one per pattern; ``min_overlap`` > 0: a pattern that is not found whole may overhang the row's end with at least that many
    positions and ``max_errors * overlap // len(pattern)`` errors."""
    patterns = [patterns] if isinstance(patterns, str) else list(patterns)
    if not patterns:
        raise ValueError("find_approximate needs at least one pattern")
    if len(patterns) > _native.APPROX_MAX_PATTERNS:
        raise NotImplementedError("more than %d patterns in one search" % _native.APPROX_MAX_PATTERNS)
    lengths = np.array([len(p) for p in patterns], dtype=np.int32)
    if lengths.max() > _native.APPROX_MAX_LEN:
        raise NotImplementedError("patterns longer than %d positions are not on the MI355X path" % _native.APPROX_MAX_LEN)
    k = np.broadcast_to(np.asarray(max_errors, dtype=np.int32), lengths.shape)
    o = np.broadcast_to(np.asarray(min_overlap, dtype=np.int32), lengths.shape)
    if lengths.min() < 1 or (k < 0).any() or (k >= lengths).any():
        raise ValueError("max_errors must be at least 0 and less than the pattern's length")
    if (o < 0).any() or (o >= lengths).any():
        raise ValueError("min_overlap must be less than the pattern's length")
    sequences = _alphabet_rows(sequences)
    alphabet = sequences.encoding.get_alphabet()
    if len(alphabet) > _native.APPROX_MAX_ALPHABET:
        raise NotImplementedError("alphabets of more than %d letters" % _native.APPROX_MAX_ALPHABET)
    masks = np.stack([_masks(p, alphabet) for p in patterns])
    sequences._compact()
    packed = sequences.encoding._is_dna()
    data = packed_words(sequences._data) if packed else sequences._as_plain(sequences._data)
    parts = get_ops().approx_rows(data, sequences.offsets(), len(sequences), sequences.total(), masks, k, o, lengths, packed,
                                  count_hits)
    return ApproxScan(parts, len(patterns), len(sequences))


def _cut(rows, keep):
    """the rows cut to ``keep`` symbols each: a (start, length) view of the same flat data"""
    rows._compact()
    ops = get_ops()
    return rows._like(rows._data, ops.slice_copy(rows.offsets(), 0, len(rows)), keep, None, len(rows), None)


def trim_adapters(reads, adapter, max_errors, min_overlap=3):
    """Cuts every row in which ``adapter`` is found — whole, or overhanging the row's end by at least ``min_overlap``
    positions — at the adapter's start; other rows stay whole.  ``reads``: an EncodedRaggedArray, or a chunk (SequenceEntry,
    SequenceEntryWithQuality), whose sequences and qualities are cut alike."""
    from ..datatypes import SequenceEntry, replace
    chunk = reads if isinstance(reads, SequenceEntry) else None
    rows = chunk.sequence if chunk is not None else reads
    if not isinstance(rows, EncodedRaggedArray):
        rows = as_encoded_array(rows)
    scan = find_approximate(rows, adapter, max_errors, min_overlap)
    rows._compact()
    keep = get_ops().approx_trim_lens(scan.start[0].harray(), rows._lens, len(rows))
    if chunk is None:
        return _cut(rows, keep)
    fields = {"sequence": _cut(rows, keep)}
    if "quality" in chunk._fields:
        fields["quality"] = _cut(chunk.quality, keep)
    return replace(chunk, **fields)
