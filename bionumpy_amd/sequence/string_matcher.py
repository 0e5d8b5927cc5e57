"""match_string and the matcher classes on the MI355X path (bionumpy/sequence/string_matcher.py).

match_string: a boolean ragged array with one entry per window of ``len(matching_sequence)`` symbols of every row (rows
shorter than the pattern give empty rows), True where the window equals the pattern.  2-bit DNA is matched as a k-mer hash
comparison on the packed form, every other one-to-one encoding byte by byte (``bnpk_match_windows_*``).

StringMatcher / MaskedStringMatcher / FixedLenRegexMatcher / RegexMatcher: patterns with wildcards (``.``), character
classes (``[AG]``) and bounded gaps (``.{a,b}``).  The pattern is compiled on the host into a motif program — segments of
fixed positions, gap ranges between them, a table of classes; no class and no gap is expanded into alternatives — and
matched in one bit-parallel pass (csrc/motif.hip, ``bnpk_motif_*``).  Departure from the reference: a match must lie inside
its row (the reference's RegexMatcher lets windows run into the next row and past the buffer).
"""
import re

import numpy as np

from ..encoded_array import (EncodedArray, EncodedRaggedArray, AlphabetEncoding, as_encoded_array, packed_words,
                             _PackedDna)
from ..ops import get_ops
from ..ragged import RaggedArray


def _match_long(ops, ragged, offsets, n_rows, total, codes, n_out):
    """a pattern of more than 64 symbols (what one launch of the byte kernel compares): its pieces of at most 64 symbols are
    matched on their own and a window matches iff every piece matches at its offset inside the window — the flags of piece j
    for row r start at (windows of piece j before row r) + offset of the piece"""
    m = codes.size
    lens = ragged.lengths
    n_win = np.maximum(lens - (m - 1), 0)                      # windows of the whole pattern per row
    row_of = np.repeat(np.arange(n_rows), n_win)
    within = np.arange(int(n_win.sum())) - np.repeat(np.cumsum(n_win) - n_win, n_win)
    flags = np.ones(int(n_win.sum()), dtype=bool)
    for o in range(0, m, 64):
        piece = codes[o:o + 64]
        _, n_piece = ops.row_offsets(ragged._lens, piece.size)
        hit = ops.match_windows(ragged._flat_data(), offsets, n_rows, total, n_piece, piece, False).host().astype(bool)
        per_row = np.maximum(lens - (piece.size - 1), 0)
        starts = np.cumsum(per_row) - per_row
        flags &= hit[starts[row_of] + within + o]
    assert flags.size == n_out
    return flags


class _DeferredMatches(RaggedArray):
    """match_string's flags over 2-bit DNA, not written yet.  What the reference's callers do with them — ``.any(axis=-1)``,
    ``.sum(axis=-1)``, ``np.sum(flags)`` — is answered by one kernel that counts every row's matching windows from the packed
    words (``bnpk_match_rows_packed``: 1.9 GB read per 50 M reads instead of 7.2 GB of flags written and read back); anything
    else that looks at the flags has them written first, transparently: ``_data`` is a property (ragged._DeferredRows is the
    same idea for a quality column)."""

    @classmethod
    def _defer(cls, words, in_offsets, total_in, codes, lens, offsets, n_rows, total):
        obj = cls.__new__(cls)
        obj._pending = (words, in_offsets, int(total_in), codes)
        obj._real = None
        obj._init(None, None, lens, offsets, n_rows, total)
        return obj

    @property
    def _data(self):
        if self._pending is not None:
            from ..device import as_bool
            self._real = as_bool(self._write_flags())
            self._pending = None
        return self._real

    @_data.setter
    def _data(self, value):
        self._real = value
        if value is not None:
            self._pending = None

    @property
    def dtype(self):
        return np.dtype(np.bool_)

    def _write_flags(self):
        words, in_offsets, total_in, codes = self._pending
        return get_ops().match_windows(words, in_offsets, self._n_rows, total_in, self._total, codes, True)

    def _row_counts(self):
        words, in_offsets, total_in, codes = self._pending
        return get_ops().match_rows(words, in_offsets, self._n_rows, total_in, codes)

    def _row_reduce(self, what, as_float=False):
        if self._pending is None or what != "sum" or as_float:
            return RaggedArray._row_reduce(self, what, as_float)
        from ..device_vector import DeviceVector
        return DeviceVector(self._row_counts())

    def _n_true(self):
        if self._pending is None or not self._n_rows:
            return RaggedArray._n_true(self)
        counts = self._row_counts()
        return int(counts.dev().sum().item()) if counts.on_device else int(counts.host().sum())


def match_string(sequence, matching_sequence):
    sequence = as_encoded_array(sequence)
    pattern = as_encoded_array(matching_sequence, sequence.encoding)
    assert isinstance(pattern, EncodedArray) and pattern.ndim == 1, "the pattern is a single sequence"
    codes = np.asarray(pattern.raw()).astype(np.uint8)
    m = codes.size
    if m == 0:
        raise ValueError("empty matching sequence")
    single = isinstance(sequence, EncodedArray)
    ragged = EncodedRaggedArray(sequence.ravel(), [sequence.size]) if single else sequence
    ragged._compact()
    ops = get_ops()
    n_rows, total, offsets = len(ragged), ragged.total(), ragged.offsets()
    out_off, n_out = ops.row_offsets(ragged._lens, m)
    enc = sequence.encoding
    packed = isinstance(enc, AlphabetEncoding) and enc.alphabet_size == 4 and m <= 31 and \
        (isinstance(ragged._data, _PackedDna) or total >= 4096)
    from ..device import HArray, as_bool
    from .kmers import _LazyLens
    if packed and not single:
        # the flags are written only if somebody looks at them: sums / any / all per row come straight from the 2-bit words
        return _DeferredMatches._defer(packed_words(ragged._data), offsets, total, codes, _LazyLens(out_off) if m > 1 else ragged._lens,
                                       out_off, n_rows, n_out)
    if packed:
        flags = as_bool(ops.match_windows(packed_words(ragged._data), offsets, n_rows, total, n_out, codes, True))
    elif m > 64:
        flags = HArray(host=_match_long(ops, ragged, offsets, n_rows, total, codes, n_out))
    else:
        flags = as_bool(ops.match_windows(ragged._flat_data(), offsets, n_rows, total, n_out, codes, False))
    if single:
        return flags.host()
    # the flags stay where the kernel wrote them (bool over the 0/1 bytes), the row lengths come from the trimmed offsets
    # only if somebody asks: ``match_string(reads, "GATTACA").any(axis=-1)`` is two kernels and no copy (string_matcher.py:16-55
    # of the reference returns a ragged array the caller reduces)
    return RaggedArray._from_parts(flags, None, _LazyLens(out_off) if m > 1 else ragged._lens, out_off, n_rows, n_out)


# ---- class-and-gap motifs ---------------------------------------------------------------------------------------------------------
MAX_SPAN, MAX_CLASSES = 64, 16          # BNPK_MOTIF_MAX_SPAN / BNPK_MOTIF_MAX_CLASSES of include/bnpk.h
_ANY = None
_ITEM = re.compile(r"\.\{(\d*),(\d+)\}|(\.)|\[([^\]]+)\]|(.)", re.S)


def _parse(pattern, encoding):
    """pattern text -> items: ("gap", a, b) | _ANY | frozenset of symbol codes.  The grammar is the reference's
    (string_matcher.py:135-164): literals, ``.``, ``[`` literals ``]``, ``.{a,b}`` / ``.{,b}``."""
    found = [m.groups() for m in _ITEM.finditer(pattern)]
    letters = "".join((cls or lit or "") for _, _, _, cls, lit in found)
    codes = iter(np.asarray(as_encoded_array(letters, encoding).raw()).astype(np.uint8).tolist() if letters else [])
    items = []
    for a, b, dot, cls, lit in found:
        if b is not None:
            a, b = int(a or 0), int(b)
            if a > b:
                raise ValueError("gap .{%d,%d}: the minimum exceeds the maximum" % (a, b))
            items.append(("gap", a, b))
        elif dot:
            items.append(_ANY)
        else:
            items.append(frozenset(next(codes) for _ in (cls or lit)))
    return items


class _Program:
    """the motif program of a list of items: segments (runs of fixed positions: a class id or any), the gap range between
    neighbouring segments, the distinct classes.  A gap of one fixed length is that many "any" positions."""

    def __init__(self, items):
        if not items or (isinstance(items[0], tuple) or isinstance(items[-1], tuple)):
            raise ValueError("a pattern is not empty and neither begins nor ends with a gap")
        self.classes, self.segments, self.gaps = [], [[]], []
        for item in items:
            if isinstance(item, tuple) and item[1] == item[2]:
                self.segments[-1].extend([_ANY] * item[1])
            elif isinstance(item, tuple):
                if not self.segments[-1]:                        # a gap right behind a gap: one gap
                    self.gaps[-1] = (self.gaps[-1][0] + item[1], self.gaps[-1][1] + item[2])
                else:
                    self.gaps.append((item[1], item[2]))
                    self.segments.append([])
            elif item is _ANY:
                self.segments[-1].append(_ANY)
            else:
                if item not in self.classes:
                    self.classes.append(item)
                self.segments[-1].append(self.classes.index(item))
        fixed = sum(len(seg) for seg in self.segments)
        self.min_span, self.max_span = fixed + sum(a for a, _ in self.gaps), fixed + sum(b for _, b in self.gaps)
        if self.max_span > MAX_SPAN:
            raise ValueError("the longest possible match has %d symbols, the limit is %d" % (self.max_span, MAX_SPAN))
        if len(self.classes) > MAX_CLASSES:
            raise ValueError("%d distinct classes, the limit is %d" % (len(self.classes), MAX_CLASSES))

    def native(self):
        """the bnpk_motif the C-ABI takes"""
        from .._native import Motif, MOTIF_ANY
        m = Motif()
        m.n_segments, m.n_classes = len(self.segments), len(self.classes)
        at = 0
        for k, seg in enumerate(self.segments):
            m.seg_len[k] = len(seg)
            if k < len(self.gaps):
                m.gap_min[k], m.gap_max[k] = self.gaps[k]
            for c in seg:
                m.pos_class[at] = MOTIF_ANY if c is _ANY else c
                at += 1
        for k, codes in enumerate(self.classes):
            for code in codes:
                m.class_mask[code] |= 1 << k
                if code < 4:
                    m.class_set4[k] |= 1 << code
        return m


class _DeferredMotifFlags(_DeferredMatches):
    """a motif's "same" flags over 2-bit DNA, not written yet; row sums / any come from bnpk_motif_rows_packed.  With
    ``_starts`` set this is the "valid" view of them (rows trimmed by window - 1): the trimmed flags are never set, so the
    rows' counts are the same."""

    @classmethod
    def _defer(cls, words, in_offsets, total_in, program, starts, lens, offsets, n_rows, total):
        obj = cls.__new__(cls)
        obj._pending = (words, in_offsets, int(total_in), program)
        obj._real = None
        obj._init(None, starts, lens, offsets, n_rows, total)
        return obj

    def _write_flags(self):
        words, in_offsets, total_in, program = self._pending
        return get_ops().motif_flags(words, in_offsets, self._n_rows, total_in, program, True)

    def _row_counts(self):
        words, in_offsets, total_in, program = self._pending
        return get_ops().motif_rows(words, in_offsets, self._n_rows, total_in, program)


class _MotifMatcher:
    """what the four matcher classes share: a compiled program and rolling_window over it"""
    _default_mode = "valid"

    def _compile(self, items, encoding):
        assert encoding.is_one_to_one_encoding(), "motifs are matched on one-to-one encodings"
        self._encoding = encoding
        self._program = _Program(items)
        self._native = self._program.native()

    @property
    def window_size(self):
        return self._program.max_span

    def __call__(self, sequence):
        raise NotImplementedError("the matchers work on whole sequences: use rolling_window")

    def _fixed_length(self):
        if self._program.min_span != self._program.max_span:
            raise ValueError("a pattern of %d to %d symbols has no fixed length: use RegexMatcher"
                             % (self._program.min_span, self._program.max_span))

    def rolling_window(self, sequence, window_size=None, mode=None):
        mode = mode or self._default_mode
        assert mode in ("valid", "same"), mode
        window = self._program.max_span
        assert window_size is None or window_size == window, "the pattern sets the window"
        sequence = as_encoded_array(sequence, self._encoding)
        single = isinstance(sequence, EncodedArray)
        ragged = EncodedRaggedArray(sequence.ravel(), [sequence.size]) if single else sequence
        ragged._compact()
        ops = get_ops()
        from ..device import HArray, as_bool
        from .kmers import _LazyLens
        n_rows, total, offsets = len(ragged), ragged.total(), ragged.offsets()
        enc = self._encoding
        packed = isinstance(enc, AlphabetEncoding) and enc.alphabet_size == 4
        data = packed_words(ragged._data) if packed else ragged._flat_data()
        if mode == "valid" and window > 1 and not single:
            # the "same" flags seen through a ragged view: the rows start where the input's do and are window - 1 shorter
            out_off, n_out = ops.row_offsets(ragged._lens, window)
            starts = HArray(dev=offsets.dev()[:n_rows]) if offsets.on_device else HArray(host=offsets.host()[:n_rows])
            shape = (starts, _LazyLens(out_off), out_off, n_rows, n_out)
        else:
            shape = (None, ragged._lens, offsets, n_rows, total)
        if packed and not single and total:
            return _DeferredMotifFlags._defer(data, offsets, total, self._native, *shape)
        flags = as_bool(ops.motif_flags(data, offsets, n_rows, total, self._native, packed))
        if single:
            flags = flags.host()
            return flags[:max(total - (window - 1), 0)] if mode == "valid" else flags
        return RaggedArray._from_parts(flags, *shape)


class StringMatcher(_MotifMatcher):
    """string_matcher.py:45-55: the windows that equal ``matching_sequence``"""

    def __init__(self, matching_sequence, encoding):
        pattern = as_encoded_array(matching_sequence, encoding)
        assert isinstance(pattern, EncodedArray) and pattern.ndim == 1, "the pattern is a single sequence"
        self._matching_sequence_array = pattern
        self._compile([frozenset([int(c)]) for c in np.asarray(pattern.raw())], encoding)


class MaskedStringMatcher(_MotifMatcher):
    """string_matcher.py:116-132: as StringMatcher, but positions where ``mask`` is set match any symbol"""

    def __init__(self, matching_sequence_array, mask):
        assert isinstance(mask, np.ndarray) and isinstance(matching_sequence_array, EncodedArray)
        assert matching_sequence_array.shape == mask.shape
        self._matching_sequence_array, self._mask = matching_sequence_array, mask
        codes = np.asarray(matching_sequence_array.raw())
        self._compile([_ANY if hidden else frozenset([int(c)]) for c, hidden in zip(codes, mask)], matching_sequence_array.encoding)


class FixedLenRegexMatcher(_MotifMatcher):
    """string_matcher.py:100-113: literals, ``.`` and ``[...]`` classes (gaps of one fixed length are accepted too)"""

    def __init__(self, matching_regex, encoding):
        self._compile(_parse(matching_regex, encoding), encoding)
        self._fixed_length()


class RegexMatcher(_MotifMatcher):
    """string_matcher.py:58-97: as FixedLenRegexMatcher plus bounded gaps ``.{a,b}``; always answers in "same" mode (flag i:
    a match starts at symbol i), as the reference's does"""

    def __init__(self, matching_regex, encoding):
        self._compile(_parse(matching_regex, encoding), encoding)

    @property
    def window_size(self):
        """the lengths a match can have"""
        return list(range(self._program.min_span, self._program.max_span + 1))

    def rolling_window(self, sequence, window_size=None, mode="same"):
        return _MotifMatcher.rolling_window(self, sequence, None, "same")
