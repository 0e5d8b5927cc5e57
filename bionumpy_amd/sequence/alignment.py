"""Pairwise alignment with affine gaps on the MI355X path (csrc/align.hip, ``bnpk_align_*``).

``align_pairs(queries, targets)`` aligns row i of the queries with row i of the targets (or every query with the targets' only
row) under a substitution matrix and a gap cost of ``gap_open + length * gap_extend``: locally, with the whole query and free
ends in the target ("semiglobal"), or end to end ("global").  Per pair it gives the score, where the alignment ends and — with
``traceback`` — where it starts and its CIGAR.  The recurrences, the choice among equal ends and among equal paths are those
written into include/bnpk.h.
"""
import numpy as np

from ..encoded_array import EncodedRaggedArray, CigarOpEncoding, packed_words
from ..ragged import RaggedArray
from .. import _native
from ..ops import get_ops
from .approximate import _alphabet_rows


class PairwiseAlignments:
    """what ``align_pairs`` returns, one entry per pair and in HBM until looked at (DeviceVectors: ``score >= 200`` is a mask
    on the device, usable as a read filter): ``score``, ``query_end``, ``target_end`` (int32; ends are half-open and relative to
    the row) and, with the traceback, ``query_start``, ``target_start``, ``cigar_op`` (an EncodedRaggedArray under
    ``CigarOpEncoding``: M, I — consumes the query — and D — consumes the target) and ``cigar_length`` (a RaggedArray of int32
    with the same rows); without it these four are None"""

    def __init__(self, parts, n_rows):
        from ..device_vector import DeviceVector
        self.score, self.query_end, self.target_end, self.query_start, self.target_start = (
            None if p is None else DeviceVector(p) for p in parts[:5])
        self.cigar_op = self.cigar_length = None
        if parts[5] is not None:
            ops, lengths, runs, offsets, total = parts[5]
            self.cigar_op = EncodedRaggedArray._from_parts(ops, None, runs, offsets, n_rows, total, CigarOpEncoding)
            self.cigar_length = RaggedArray._from_parts(lengths, None, runs, offsets, n_rows, total)

    def __len__(self):
        return len(self.score)


def count_reference_length(cigar_op, cigar_length):
    """int64 per row: the target symbols a CIGAR covers, the lengths of its M, D, N, = and X runs added up"""
    consumes = np.isin(np.asarray(CigarOpEncoding.get_alphabet()), list("MDN=X"))
    cigar_op._compact()
    cigar_length._compact()
    covered = np.where(consumes[cigar_op._data.host()], cigar_length._data.host(), 0).astype(np.int64)
    return np.add.reduceat(np.append(covered, 0), cigar_op.offsets().host()[:-1]) * (cigar_op._lens.host() > 0)


def _scoring(alphabet_size, match, mismatch, matrix, gap_open, gap_extend):
    if matrix is None:
        matrix = np.full((alphabet_size, alphabet_size), int(mismatch), dtype=np.int64)
        np.fill_diagonal(matrix, int(match))
    matrix = np.asarray(matrix)
    if matrix.shape != (alphabet_size, alphabet_size) or not np.issubdtype(matrix.dtype, np.integer):
        raise ValueError("matrix must be %d x %d integers, [query code][target code]" % (alphabet_size, alphabet_size))
    if matrix.min() < -128 or matrix.max() > 127:
        raise ValueError("scores must lie in -128 .. 127")
    if not (0 <= gap_open <= 127 and 0 <= gap_extend <= 127):
        raise ValueError("gap_open and gap_extend must lie in 0 .. 127")
    return matrix


def align_pairs(queries, targets, match=2, mismatch=-3, matrix=None, gap_open=5, gap_extend=2, mode="local", traceback=True):
    """Aligns every query with its target: a ``PairwiseAlignments``.  ``queries``, ``targets``: EncodedRaggedArrays of one
    alphabet of at most 32 letters (or lists of strings: ACGT), with as many rows each, or one target for all queries.
    ``matrix``: integers in -128 .. 127, [query code][target code], instead of ``match`` / ``mismatch``; a gap of L columns
    costs ``gap_open + L * gap_extend``.  ``mode``: "local", "semiglobal" (the whole query, free ends in the target) or
    "global".  ``traceback=False`` gives score and ends only, which is faster.  Rows of up to 512 symbols."""
    if mode not in _native.ALIGN_MODES:
        raise ValueError("mode must be one of %s" % ", ".join(_native.ALIGN_MODES))
    rows_q, rows_t = _alphabet_rows(queries), _alphabet_rows(targets)
    if rows_q.encoding != rows_t.encoding:
        raise ValueError("queries under %s and targets under %s: both sides need one encoding" % (rows_q.encoding, rows_t.encoding))
    alphabet_size = len(rows_q.encoding.get_alphabet())
    if alphabet_size > _native.APPROX_MAX_ALPHABET:
        raise NotImplementedError("alphabets of more than %d letters" % _native.APPROX_MAX_ALPHABET)
    matrix = _scoring(alphabet_size, match, mismatch, matrix, gap_open, gap_extend)
    if len(rows_t) != len(rows_q) and len(rows_t) != 1:
        raise ValueError("%d queries and %d targets: row i of one is aligned with row i of the other, or all with one target"
                         % (len(rows_q), len(rows_t)))
    packed = rows_q.encoding._is_dna()
    for rows in (rows_q, rows_t):
        rows._compact()
    data = [packed_words(rows._data) if packed else rows._as_plain(rows._data) for rows in (rows_q, rows_t)]
    parts = get_ops().align_pairs(data[0], rows_q.offsets(), rows_q.total(), data[1], rows_t.offsets(), rows_t.total(), len(rows_q),
                                  len(rows_t), matrix, gap_open, gap_extend, _native.ALIGN_MODES.index(mode), traceback, packed)
    return PairwiseAlignments(parts, len(rows_q))
