"""Position weight matrix scores on the MI355X path (bionumpy/sequence/position_weight_matrix.py).

``PWM`` keeps the reference's constructor and factories (log-likelihood-ratio matrix, ``matrix[letter][position]``);
``get_motif_scores(sequence, pwm)`` returns a ragged float64 array with one score per window of ``pwm.window_size``
bases of every row.  The scores are accumulated in double precision in the reference's order (offset 0, 1, ...), on
the packed 2-bit form (``bnpk_pwm_scores``).

``scan_motifs(sequence, pwms)`` answers what a motif-library scan asks per read — the best window of every PWM, where it
is, on which strand, how many windows clear a threshold — in one pass that writes no scores (``bnpk_pwm_rows_*``), for any
``AlphabetEncoding``.
"""
import numpy as np

from ..encoded_array import (EncodedArray, EncodedRaggedArray, AlphabetEncoding, as_encoded_array, packed_words)
from .. import _native
from ..device import HArray
from ..ops import get_ops
from ..ragged import RaggedArray


def _pwm_from_counts(count_matrix):
    with_pseudo = count_matrix + 1                                            # position_weight_matrix.py:29-31
    return np.log(with_pseudo / with_pseudo.sum(axis=0, keepdims=True))


class PWM:
    """position_weight_matrix.py:34-148"""

    def __init__(self, matrix, alphabet):
        self._matrix = np.asarray(matrix, dtype=float)
        self._alphabet = alphabet
        self._encoding = AlphabetEncoding(alphabet)

    @property
    def alphabet(self):
        return self._alphabet

    @property
    def window_size(self):
        return self._matrix.shape[-1]

    def as_valid_encoded_array(self, sequence):
        if isinstance(sequence, (EncodedArray, EncodedRaggedArray)) and isinstance(sequence.encoding, AlphabetEncoding):
            alphabet = list(sequence.encoding.get_alphabet())
            if alphabet[:len(self._alphabet)] != list(self._alphabet):
                raise Exception("Could not calculate pwm for alphabet %s on %s encoded array"
                                % (list(self._alphabet), alphabet))
            return sequence
        return as_encoded_array(sequence, self._encoding)

    def _scores(self, sequence):
        sequence = self.as_valid_encoded_array(sequence)
        if "".join(self._alphabet).upper() != "ACGT":
            raise NotImplementedError("motif scores on the MI355X path: the ACGT alphabet (2-bit codes)")
        if self.window_size > 64:
            raise NotImplementedError("motifs longer than 64 positions are not on the MI355X path")
        single = isinstance(sequence, EncodedArray)
        ragged = EncodedRaggedArray(sequence.ravel(), [sequence.size]) if single else sequence
        ragged._compact()
        ops = get_ops()
        n_rows, total = len(ragged), ragged.total()
        out_off, n_out = ops.row_offsets(ragged._lens, self.window_size)
        scores = ops.pwm_scores(packed_words(ragged._data), ragged.offsets(), n_rows, total, n_out, self._matrix)
        self._last_offsets = out_off
        return scores, ragged, single

    def calculate_score(self, sequence):
        """score of one window of exactly window_size symbols (position_weight_matrix.py:67-80)"""
        sequence = self.as_valid_encoded_array(sequence)
        assert sequence.shape[-1] == self.window_size
        scores, _, _ = self._scores(sequence)
        return float(scores.host()[0])

    @classmethod
    def from_dict(cls, dictionary, background=None):
        """position probabilities -> log-likelihood ratios (position_weight_matrix.py:106-134)"""
        if background is None:
            background = {key: 1 / len(dictionary) for key in dictionary}
        alphabet = "".join(dictionary.keys())
        with np.errstate(divide="ignore"):
            matrix = np.log(np.array(list(dictionary.values()), dtype=float)) - \
                np.log([background[key] for key in dictionary])[:, np.newaxis]
        return cls(matrix, alphabet)

    @classmethod
    def from_counts(cls, counts):
        return cls(_pwm_from_counts(np.array(list(counts.values()))), "".join(counts.keys()))

    def __str__(self):
        matrix = self._matrix.transpose()
        return "PWM with alphabet " + self._alphabet + "\n" + \
            "\n".join(" ".join(str(round(c, 2)) for c in row) for row in matrix)


def get_motif_scores(sequence, pwm):
    """motif score at every position of every read (position_weight_matrix.py:177-196): a ragged float64 array,
    row r holds max(0, L_r - window_size + 1) scores"""
    scores, ragged, single = pwm._scores(as_encoded_array(sequence) if not isinstance(
        sequence, (EncodedArray, EncodedRaggedArray)) else sequence)
    if single:
        return scores.host()
    # the scores stay in HBM (a float64 per window: 56 GB for 50 M reads would not cross PCIe in the time of a thousand such
    # kernels); ``.max(axis=-1)`` / ``.sum(axis=-1)`` reduce them there (position_weight_matrix.py:177-196 returns a ragged array)
    from .kmers import _LazyLens
    out_off = pwm._last_offsets
    lens = _LazyLens(out_off) if pwm.window_size > 1 else ragged._lens
    return RaggedArray._from_parts(scores, None, lens, out_off, len(ragged), scores.size)


class _MotifRows:
    """n_motifs x n_rows results of a scan, in HBM until looked at: ``x[m]`` is motif m's per-row vector (a DeviceVector: its
    comparisons are masks on the device, usable as read filters), anything else goes through the numpy array"""

    def __init__(self, data, n_motifs, n_rows):
        self._data, self.shape = data, (n_motifs, n_rows)

    def __len__(self):
        return self.shape[0]

    @property
    def dtype(self):
        return self._data.dtype

    def __getitem__(self, idx):
        if isinstance(idx, (int, np.integer)):
            from ..device_vector import DeviceVector
            m = int(idx) + (self.shape[0] if idx < 0 else 0)
            if not 0 <= m < self.shape[0]:
                raise IndexError("motif %d of %d" % (idx, self.shape[0]))
            return DeviceVector(get_ops().slice_copy(self._data, m * self.shape[1], (m + 1) * self.shape[1]))
        return np.asarray(self)[idx]

    def __array__(self, dtype=None, copy=None):
        a = self._data.host().reshape(self.shape)
        return a if dtype is None else a.astype(dtype, copy=False)

    def __repr__(self):
        return repr(np.asarray(self))


class MotifScan:
    """what ``scan_motifs`` returns: ``best_score`` (float64, -inf where a row has no window), ``best_position`` (int64, -1
    there), ``best_strand`` (uint8: 1 = the reverse complement scores best) and, with thresholds, ``n_hits`` (int64)"""

    def __init__(self, parts, n_motifs, n_rows):
        best, pos, strand, hits = parts
        self.best_score = _MotifRows(best, n_motifs, n_rows)
        self.best_position = _MotifRows(pos, n_motifs, n_rows)
        self.best_strand = _MotifRows(strand, n_motifs, n_rows)
        self.n_hits = None if hits is None else _MotifRows(hits, n_motifs, n_rows)


def scan_motifs(sequence, pwms, both_strands=False, thresholds=None):
    """Scores every PWM of ``pwms`` over every window of every row and keeps, per (motif, row): the best score, its window's
    start and strand, and — with ``thresholds`` (one number, or one per motif) — how many (window, strand) pairs reach it.
    Scores are those of ``get_motif_scores`` (and of it on ``get_reverse_complement(sequence)`` for the reverse strand), bit
    for bit; among equal scores the forward strand, then the smaller start wins."""
    pwms = list(pwms)
    if not pwms:
        raise ValueError("scan_motifs needs at least one PWM")
    alphabet = "".join(pwms[0].alphabet)
    if any("".join(p.alphabet) != alphabet for p in pwms):
        raise ValueError("the PWMs of one scan share one alphabet")
    if max(p.window_size for p in pwms) > _native.PWM_MAX_WIDTH:
        raise NotImplementedError("motifs longer than 64 positions are not on the MI355X path")
    if len(pwms) > _native.PWM_MAX_MOTIFS:
        raise NotImplementedError("more than %d motifs in one scan" % _native.PWM_MAX_MOTIFS)
    packed = alphabet.upper() == "ACGT"
    if both_strands and not packed:
        raise ValueError("both_strands needs the ACGT alphabet (complement = 3 - code), not %r" % alphabet)
    if len(alphabet) > _native.PWM_MAX_ALPHABET:
        raise NotImplementedError("alphabets of more than %d letters" % _native.PWM_MAX_ALPHABET)
    if thresholds is not None:
        thresholds = np.broadcast_to(np.asarray(thresholds, dtype=np.float64), (len(pwms),))
    if not isinstance(sequence, (EncodedArray, EncodedRaggedArray)):
        sequence = as_encoded_array(sequence)
    sequence = pwms[0].as_valid_encoded_array(sequence)
    if isinstance(sequence, EncodedArray):
        sequence = EncodedRaggedArray(sequence.ravel(), [sequence.size])
    if sequence.encoding.alphabet_size != len(alphabet):      # (ACGTn rows under ACGT matrices: code 4 has no column)
        raise ValueError("the sequences' alphabet %s is not the PWMs' (%r)" % (sequence.encoding.get_alphabet(), alphabet))
    sequence._compact()
    data = packed_words(sequence._data) if packed else sequence._data
    parts = get_ops().pwm_rows(data, sequence.offsets(), len(sequence), sequence.total(), [p._matrix for p in pwms], packed,
                               both_strands, thresholds)
    if parts[2] is None:                                      # (the byte path is forward only)
        parts = (parts[0], parts[1], HArray(dev=get_ops().device.zeros(len(pwms) * len(sequence), np.uint8)), parts[3])
    return MotifScan(parts, len(pwms), len(sequence))


class PositionWeightMatrix:
    """PositionWeightMatrix (sequence/position_weight_matrix.py:13-25): the rollable form of a PWM — a call scores one window
    of window_size symbols, ``rolling_window`` every window of every row (== get_motif_scores)."""

    def __init__(self, pwm):
        self._pwm = pwm
        self._encoding = pwm._encoding
        self.window_size = pwm.window_size

    def __call__(self, sequence):
        return self._pwm.calculate_score(sequence)

    def rolling_window(self, sequence):
        return get_motif_scores(sequence, self._pwm)

