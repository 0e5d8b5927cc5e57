"""Barcode assignment (demultiplexing) on the MI355X path (csrc/demux.hip, ``bnpk_demux_rows_*``).

``assign_barcodes(reads, barcodes)`` answers per read which barcode of a whitelist its barcode window — the symbols
``[start, start + L)`` — is nearest to under the Hamming distance, how far it is and how far the runner-up is; a read is
assigned when the nearest is within ``max_mismatches`` and the runner-up at least ``min_delta`` farther.  The semantics are
those written into include/bnpk.h.
"""
import numpy as np

from ..encoded_array import EncodedArray, EncodedRaggedArray, packed_words
from .. import _native
from ..ops import get_ops
from .approximate import _alphabet_rows


class BarcodeAssignment:
    """what ``assign_barcodes`` returns, one entry per read and in HBM until looked at (DeviceVectors: ``index == 3`` is a
    mask on the device, usable as a read filter): ``index`` (int32: the barcode, -1 where none is assigned), ``distance``
    (uint8: mismatches to the nearest barcode) and ``second`` (uint8: mismatches to the runner-up); the last two are 255 for
    a read too short to hold the window, ``second`` also where the whitelist has one barcode"""

    def __init__(self, parts):
        from ..device_vector import DeviceVector
        self.index, self.distance, self.second = (DeviceVector(p) for p in parts)

    def __len__(self):
        return len(self.index)


def _barcode_codes(barcodes):
    """uint8 [barcode][position] over ACGT from a list of strings or an encoded array of equal-length rows"""
    if isinstance(barcodes, (EncodedArray, EncodedRaggedArray)):
        barcodes = barcodes.tolist()
    barcodes = [barcodes] if isinstance(barcodes, str) else [str(b) for b in barcodes]
    if not barcodes or not barcodes[0]:
        raise ValueError("assign_barcodes needs at least one barcode of at least one letter")
    if len({len(b) for b in barcodes}) != 1:
        raise ValueError("barcodes must all have the same length")
    if len(barcodes[0]) > _native.DEMUX_MAX_LEN:
        raise NotImplementedError("barcodes longer than %d positions are not on the MI355X path" % _native.DEMUX_MAX_LEN)
    if len(barcodes) > _native.DEMUX_MAX_BARCODES:
        raise NotImplementedError("more than %d barcodes in one whitelist" % _native.DEMUX_MAX_BARCODES)
    text = np.frombuffer("".join(barcodes).upper().encode("latin-1", "replace"), dtype=np.uint8).reshape(len(barcodes), -1)
    lut = np.full(256, 255, dtype=np.uint8)
    lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4)
    codes = lut[text]
    if (codes == 255).any():
        raise ValueError("barcode %r has a letter outside ACGT" % barcodes[int(np.flatnonzero((codes == 255).any(axis=1))[0])])
    if np.unique(codes, axis=0).shape[0] != codes.shape[0]:
        raise ValueError("duplicate barcodes: the later of two equal barcodes could never be assigned")
    return codes


def assign_barcodes(reads, barcodes, max_mismatches=1, start=0, min_delta=1):
    """The nearest barcode of every read under the Hamming distance: a ``BarcodeAssignment``.  ``reads``: an
    EncodedRaggedArray over ACGT or ACGTn, a chunk (its ``.sequence``) or a list of strings; ``barcodes``: strings, or an
    encoded array, of one length L <= 32 over ACGT.  The barcode window is the symbols ``[start, start + L)`` of a read; an
    N in it differs from every letter.  A read is assigned to the nearest barcode (the smallest index among equals) when
    that is within ``max_mismatches`` and the runner-up is at least ``min_delta`` farther away."""
    from ..datatypes import SequenceEntry
    codes = _barcode_codes(barcodes)
    if not 0 <= max_mismatches <= codes.shape[1]:
        raise ValueError("max_mismatches must lie in 0 .. the barcodes' length")
    if start < 0 or min_delta < 0:
        raise ValueError("start and min_delta must not be negative")
    if start > (1 << 31) - 1 - codes.shape[1]:
        raise ValueError("start is beyond any read")
    rows = _alphabet_rows(reads.sequence if isinstance(reads, SequenceEntry) else reads)
    packed = rows.encoding._is_dna()
    if not packed and "".join(rows.encoding.get_alphabet()).upper() != "ACGTN":
        raise NotImplementedError("assign_barcodes takes reads over ACGT or ACGTn, not %s" % "".join(rows.encoding.get_alphabet()))
    rows._compact()
    data = packed_words(rows._data) if packed else rows._as_plain(rows._data)
    return BarcodeAssignment(get_ops().demux_rows(data, rows.offsets(), len(rows), rows.total(), codes, int(start),
                                                  int(max_mismatches), int(min_delta), packed))
