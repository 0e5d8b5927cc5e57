"""-m gpu: StringMatcher / MaskedStringMatcher / FixedLenRegexMatcher / RegexMatcher (csrc/motif.hip) against Python's re on
the row strings: flags[r][i] = re.compile(pattern).match(row, i) is not None."""
import ctypes as C
import random
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DNA_PATTERNS = ["AC", "[AG].[AT]", "AA.{,1}[CT]", "G.{2,5}[ACG]T.{0,3}CA", "A" + "." * 62 + "T", "TT.{1,40}GG"]
AMINO_PATTERNS = ["M[KR].{,3}[DE]", "C..C", "[ST].{2,6}P"]
CASES = [(form, p) for p in DNA_PATTERNS for form in ("packed", "text")] + [("amino", p) for p in AMINO_PATTERNS]


def reference(rows, pattern):
    rx = re.compile(pattern)
    return [[rx.match(row, i) is not None for i in range(len(row))] for row in rows]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


@pytest.fixture(scope="module")
def matchers(bnp):
    return bnp.sequence.string_matcher


def test_reference_goldens(bnp, matchers):
    plain = matchers.StringMatcher("V1-1", bnp.BaseEncoding)
    assert plain.window_size == 4
    assert plain.rolling_window(bnp.as_encoded_array(["V1-1", "V2-1", "V1-1*2"])).tolist() == [[True], [False], [True, False, False]]
    fixed = matchers.FixedLenRegexMatcher("[AG].[AT]", bnp.DNAEncoding)
    assert fixed.window_size == 3
    assert fixed.rolling_window(bnp.as_encoded_array(["ACGT", "AATGAT"], bnp.DNAEncoding)).tolist() == \
        [[False, False], [True, False, False, True]]
    flexible = matchers.RegexMatcher("AA.{,1}[CT]", bnp.DNAEncoding)
    assert flexible.window_size == [3, 4]
    assert flexible.rolling_window(bnp.as_encoded_array(["ACGTTCG", "AATGAAAC"], bnp.DNAEncoding)).tolist() == \
        [[False] * 7, [True, False, False, False, True, True, False, False]]
    assert matchers.RegexMatcher("AGT", bnp.DNAEncoding).rolling_window(["AAG", "TAA"]).tolist() == [[False] * 3] * 2
    masked = matchers.MaskedStringMatcher(bnp.as_encoded_array("ACGT", bnp.DNAEncoding), np.array([False, True, True, False]))
    assert masked.window_size == 4
    assert masked.rolling_window(["ACGTAGGT", "AT"]).tolist() == [[True, False, False, False, True], []]
    with pytest.raises(NotImplementedError):
        flexible(np.zeros((2, 3), dtype=np.uint8))


@pytest.fixture(scope="module")
def shapes(bnp):
    """one row set at the kernels' edges (a lane owns 32 starts and looks 63 symbols ahead, a packed word holds 32 bases, a
    workgroup of the byte kernel 8192 symbols, the row counts hand rows of more than 4096 to the whole wavefront), in three
    forms, and the reference's flags of every case — each with matches, non-matches and starts that match only across a row end"""
    rng = random.Random(20261126)
    lengths = [0, 0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129] + [150] * 30 + [3] * 700 + \
        [2047, 2048, 2049, 9000] + [151] * 20 + [0, 5]
    dna = ["".join(rng.choice("ACGT") for _ in range(n)) for n in lengths]
    amino = ["".join(rng.choice("ACDEFGHIKLMNPQRSTVWY") for _ in range(n)) for n in lengths]
    forms = {"packed": (dna, bnp.DNAEncoding), "text": (dna, bnp.BaseEncoding), "amino": (amino, bnp.AminoAcidEncoding)}
    arrays = {form: bnp.as_encoded_array(rows, enc) for form, (rows, enc) in forms.items()}
    want = {}
    for form, pattern in CASES:
        rows = forms[form][0]
        want[form, pattern] = flags = reference(rows, pattern)
        flat = [f for row in flags for f in row]
        joined = reference(["".join(rows)], pattern)[0]
        assert any(flat) and not all(flat), pattern
        assert any(a and not b for a, b in zip(joined, flat)), "no start of %s matches only across a row end" % pattern
    return forms, arrays, want


@pytest.mark.parametrize("form,pattern", CASES)
def test_shapes(matchers, shapes, form, pattern):
    forms, arrays, want = shapes
    got = matchers.RegexMatcher(pattern, forms[form][1]).rolling_window(arrays[form])
    if form == "packed":                                      # the rows' counts, before anything writes the flags
        assert np.asarray(got.sum(axis=-1)).tolist() == [sum(row) for row in want[form, pattern]]
    assert got.tolist() == want[form, pattern]


@pytest.mark.parametrize("form,pattern", [("packed", "[AG].[AT]"), ("amino", "C..C")])
def test_modes(bnp, matchers, form, pattern):
    rng = random.Random(3)
    rows = ["".join(rng.choice("ACGT" if form == "packed" else "ACDE") for _ in range(n)) for n in [0, 1, 2, 3, 4, 40, 2, 33]]
    enc = bnp.DNAEncoding if form == "packed" else bnp.AminoAcidEncoding
    matcher = matchers.FixedLenRegexMatcher(pattern, enc)
    same = reference(rows, pattern)
    w = matcher.window_size
    assert matcher.rolling_window(rows, mode="same").tolist() == same
    valid = matcher.rolling_window(rows)
    assert valid.tolist() == [row[:max(len(row) - (w - 1), 0)] for row in same]
    assert np.asarray(valid.sum(axis=-1)).tolist() == [sum(row) for row in same]
    assert np.asarray(matcher.rolling_window(rows).any(axis=-1)).tolist() == [any(row) for row in same]
    single = matcher.rolling_window(bnp.as_encoded_array(rows[5], enc))
    assert isinstance(single, np.ndarray) and single.dtype == bool and single.tolist() == same[5][:40 - (w - 1)]
    assert matcher.rolling_window(bnp.as_encoded_array(rows[5], enc), mode="same").tolist() == same[5]
    assert matcher.rolling_window([]).tolist() == [] and matcher.rolling_window([], mode="same").tolist() == []


def test_errors(bnp, matchers):
    with pytest.raises(ValueError, match="gap"):
        matchers.RegexMatcher("AC.{1,2}", bnp.DNAEncoding)
    with pytest.raises(ValueError, match="64"):
        matchers.RegexMatcher("A.{1,70}C", bnp.DNAEncoding)
    letters = "ACDEFGHIKLMNPQRSTV"
    with pytest.raises(ValueError, match="16"):
        matchers.RegexMatcher("".join("[%s%s]" % pair for pair in zip(letters[:17], letters[1:])), bnp.AminoAcidEncoding)
    with pytest.raises(ValueError):
        matchers.FixedLenRegexMatcher("A.{1,2}C", bnp.DNAEncoding)
    with pytest.raises(bnp.EncodingError):
        matchers.RegexMatcher("A[CX]", bnp.DNAEncoding)


def test_abi_argument_checks(bnp, matchers):
    from bionumpy_amd import _native
    from bionumpy_amd.device import HArray, ptr
    ops = bnp.ops.get_ops()
    program = matchers.FixedLenRegexMatcher("A.G", bnp.DNAEncoding)._native
    packed = bnp.as_encoded_array("ACGTAAGC", bnp.DNAEncoding)._harray().packed.dev()
    ends = ops.row_end_mask(HArray(host=np.array([0, 8])), 1, 8).dev()
    out = ops._empty(16, np.uint8)

    def call(n=8, motif=program, d_out=out):
        return _native.lib.bnpk_motif_flags_packed(ops.ctx, ptr(packed), ptr(ends), n, C.byref(motif), ptr(d_out), ops._s())
    broken = _native.Motif.from_buffer_copy(program)
    broken.n_segments = 0
    assert call(motif=broken) == -1                           # BNPK_ERR_ARG
    assert call(d_out=None) == -1
    assert call(n=0, d_out=None) == 0
    assert call() == 0 and out.cpu().numpy()[:8].tolist() == [1, 0, 0, 0, 1, 0, 0, 0]
