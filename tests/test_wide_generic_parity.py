"""-m gpu: the wide, generic and weighted kernels through the C-ABI against plain numpy / Python on the shapes where they take
another branch — the kernels the suite reached through docstring-sized API examples only.  One CPU test at the end runs the
same functions against the oracle-backed stand-in (tests/oracle_ops.py), which proves the expectations, the generators' own
assertions and the two summation bounds on the reference alone.

What every case is there for:

``bnpk_row_reduce_wide`` (rowops.hip, eight lanes per row, a shuffle merge that carries ``any`` and NaN):
  rows of 0..9 elements (lanes without a first element in the merge), 15 / 16 / 17 and 63 / 64 / 65 (around the group's
  stride), 1000 and 100 003 (far longer than the stride), empty rows between them, 300 rows of 3 (more than one workgroup of
  32 rows); a NaN in each of the eight lane slots, in the first and in the second element of a lane, in a row whose other lanes
  are empty, in two lanes, everywhere; +inf, -inf, both (sum NaN); INT64_MIN / INT64_MAX and a sum that wraps.
``bnpk_kmers_generic`` / ``bnpk_minimizers_generic`` (kmers.hip: kmer_generic_kernel, 1024 outputs per tile, tile -> row table):
  five tiles; a tile boundary that is a row boundary; runs of rows without output (empty, shorter than k, shorter than the
  window) at two tile boundaries; one row over three tiles; first and last row without output; alphabets of 2 and 255
  letters, k = 1, window == k, hashes that wrap (negative ones in the minimum), k = 31 against the 2-bit kernel.
``bnpk_count_weighted`` (count.hip: hist_weighted_kernel): LDS bins up to 4096, global atomics from 4097; one workgroup per
  row with n around 256 (its grid-stride loop from 257); one row of 1.2 M values (the capped grid's loop); 65 535 rows
  (gridDim.y); the three stride forms; int64 sums that wrap; a bin whose LDS sum is exactly zero (not flushed); NaN and inf
  weights; a value of -1 or n_bins (the out-of-range flag) on both paths.
``bnpk_count_dense_rows`` (count.hip: hist_rows_kernel, a row search per element): empty rows first, last and in a run, one
  row, 1000 rows of one element; n around 256 and 70 001 (more than one workgroup); values outside the bins, skipped.
``bnpk_multiline_wrap`` (multiline.hip): sequences of 0, 1, w - 1, w, w + 1, 2w, 2w + 1 and 10 000 w + 3 letters for w = 1, 7,
  80; names of 0, 1 and 300 bytes; 1, 2 and 2000 records (more than one workgroup of the size kernel); the sizes-only call
  against the second one; a capacity one byte short.
``bnpk_packed_rows_slice`` (encode.hip): a first base at 0, 1, 16 and 31 mod 32; slices that end in the input's last word;
  0, 31, 32, 33 and 64 bases; ones in the input's words behind its last base, zeros behind the slice's.

Integer results are compared with np.array_equal.  The only tolerances are the two summation bounds, derived where they are
used (_sum_bound)."""
import ctypes as C
import math
from contextlib import contextmanager

import numpy as np
import pytest

import oracle
from bionumpy_amd.device import HArray

I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
TILE_OUT = 1024                    # outputs per workgroup of kmer_generic_kernel (kmers.hip)
ERR_ARG, ERR_RANGE = -1, -6


@pytest.fixture(scope="module")
def ops():
    from bionumpy_amd import ops as ops_mod
    ops_mod.set_ops(None)
    return ops_mod.get_ops()


def _h(a):
    return HArray(host=np.ascontiguousarray(a))


def _hd(a, dtype):
    """a flat buffer for the device; an empty one becomes one element that nobody reads (torch gives empty tensors no address)"""
    a = np.ascontiguousarray(a, dtype=dtype)
    return _h(a if a.size else np.zeros(1, dtype=dtype))


def _offsets(lens):
    return np.concatenate(([0], np.cumsum(lens))).astype(np.int64)


@contextmanager
def _as_the_ops(ops):
    """the package's own classes (RaggedArray, count_encoded) on ``ops`` for the duration"""
    from bionumpy_amd import ops as ops_mod
    before = ops_mod._ops
    ops_mod.set_ops(ops)
    try:
        yield
    finally:
        ops_mod.set_ops(before)


def _sum_bound(n, sum_abs):
    """|any order of n float64 additions - math.fsum| <= n * 2**-52 * sum|x|: a sum of n terms in ANY order is off by at most
    (n - 1) * 2**-53 * sum|x| to first order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2); doubled, which also
    covers the one rounding of fsum's exact result and the higher-order terms.  Derived, not measured."""
    return n * 2.0 ** -52 * sum_abs


# ------------------------------------------------------------------------------------ 1. row_reduce_wide
def _check_wide(ops, rows):
    dtype = rows[0].dtype
    lens = np.array([r.size for r in rows], dtype=np.int64)
    flat = np.concatenate(rows)
    got = ops.row_reduce_wide(_hd(flat, dtype), _h(_offsets(lens)), len(rows), want=("sum", "min", "max"))
    gs, gmn, gmx = got["sum"].host(), got["min"].host(), got["max"].host()
    assert gs.dtype == gmn.dtype == gmx.dtype == dtype
    full = np.flatnonzero(lens > 0)
    assert not gs[lens == 0].any()                                      # an empty row: sum 0 (its min / max are nobody's to read)
    with np.errstate(invalid="ignore", over="ignore"):
        emn = np.array([np.min(rows[r]) for r in full], dtype=dtype)    # (propagate NaN)
        emx = np.array([np.max(rows[r]) for r in full], dtype=dtype)
        assert np.array_equal(gmn[full], emn, equal_nan=True)
        assert np.array_equal(gmx[full], emx, equal_nan=True)
        if dtype == np.int64:
            es = np.array([np.sum(rows[r]) for r in full], dtype=np.int64)          # (wraps, as the kernel's additions do)
            assert np.array_equal(gs[full], es)
        else:
            for r in full:
                row = rows[r]
                if np.all(np.isfinite(row)):
                    exact, bound = math.fsum(row), _sum_bound(row.size, math.fsum(np.abs(row)))
                    assert abs(gs[r] - exact) <= bound, (r, row.size, gs[r], exact, bound)
                else:                                                   # NaN, or inf of one sign, or both (NaN): numpy's own sum
                    assert np.array_equal(gs[r], np.sum(row), equal_nan=True), (r, gs[r], np.sum(row))
    if np.any(lens == 0):                                               # the host refuses before anybody reads such a min / max
        from bionumpy_amd.ragged import RaggedArray
        with _as_the_ops(ops):
            with pytest.raises(ValueError):
                RaggedArray(flat, lens).min(axis=-1)
            with pytest.raises(ValueError):
                RaggedArray(flat, lens).max(axis=-1)


def _values(rng, n, dtype):
    if dtype == np.int64:
        return rng.integers(-(1 << 40), 1 << 58, size=n, dtype=np.int64)
    return rng.normal(size=n) * 10.0 ** rng.integers(-3, 6, size=n)


WIDE_LENGTHS = [0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 1000, 100_003]


def _wide_edge_rows(dtype):
    rng = np.random.default_rng(101)
    rows = []
    for n in WIDE_LENGTHS:
        rows += [_values(rng, n, dtype), np.zeros(0, dtype=dtype)]
    rows += [np.zeros(0, dtype=dtype)] * 3
    rows += [_values(rng, 3, dtype) for _ in range(300)]
    if dtype == np.float64:
        def spoiled(n, where, value=np.nan):
            row = _values(rng, n, dtype)
            row[where] = value
            return row
        for p in range(8):
            rows += [spoiled(20, [p]), spoiled(20, [p + 8])]           # the first / the second element of lane p
        rows += [spoiled(3, [2]), spoiled(3, [0]), spoiled(20, [1, 6]), spoiled(20, [5, 10]), np.full(20, np.nan), np.full(5, np.nan)]
        rows += [spoiled(20, [3], np.inf), spoiled(20, [11], -np.inf), spoiled(20, [2, 13], np.inf)]
        both = spoiled(20, [4], np.inf)
        both[17] = -np.inf
        rows += [both, spoiled(2, [0], np.inf), spoiled(9, [8], -np.inf), np.array([np.inf, -np.inf, np.nan])]
    else:
        def holding(n, where, values):
            row = rng.integers(-1000, 1000, size=n, dtype=np.int64)
            row[where] = values
            return row
        rows += [holding(20, [3], [I64_MIN]), holding(20, [12], [I64_MAX]), holding(20, [0, 19], [I64_MAX, I64_MIN]),
                 holding(3, [2], [I64_MIN]), holding(1, [0], [I64_MAX]), np.full(9, I64_MIN), np.full(9, I64_MAX),
                 np.full(40, 1 << 61, dtype=np.int64),                  # 40 * 2^61 wraps five times over
                 holding(17, [0, 1, 16], [I64_MAX, I64_MAX, 5])]
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int64, np.float64], ids=["int64", "float64"])
def test_row_reduce_wide_at_the_edges(ops, dtype):
    """per-row sum / min / max of int64 and float64 rows against numpy (min / max, int64 sums) and math.fsum (float64 sums,
    within _sum_bound).  The kernel's grid-stride loop over rows starts beyond 5 * 10^8 rows (32 rows per workgroup, the grid
    capped in common.h) and is NOT exercised here."""
    _check_wide(ops, _wide_edge_rows(dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_rows,max_len", [(1, 1, 1), (2, 100, 7), (3, 5000, 160), (4, 5, 100_000)])
def test_row_reduce_wide_random(ops, seed, n_rows, max_len):
    rng = np.random.default_rng(seed)
    for dtype in (np.int64, np.float64):
        lens = rng.integers(0, max_len + 1, size=n_rows)
        lens[rng.integers(0, n_rows, size=max(1, n_rows // 8))] = 0
        lens[rng.integers(0, n_rows)] = max_len                        # (never all empty)
        rows = [_values(rng, int(n), dtype) for n in lens]
        for r in rng.integers(0, n_rows, size=max(1, n_rows // 20)):    # a few rows with NaN / inf, or with the largest integers
            if rows[r].size:
                rows[r][rng.integers(0, rows[r].size)] = rng.choice([np.nan, np.inf, -np.inf]) if dtype == np.float64 \
                    else rng.choice([I64_MIN, I64_MAX])
        _check_wide(ops, rows)


# ------------------------------------------------------------------------------------ 2. kmers_generic / minimizers_generic
def _tile_edge_lengths(k, window):
    """row lengths whose windows of ``window`` letters fill five tiles of 1024 outputs, with the properties below — asserted
    here from the output offsets, so that an edit of the numbers cannot lose them"""
    none = sorted({0, window - 1, k - 1, min(1, window - 1), (window - 1) // 2})      # lengths without an output
    quiet = lambda n: [none[i % len(none)] for i in range(n)]
    with_out = lambda *counts: [c + window - 1 for c in counts]
    lens = quiet(1) + with_out(400, 624) + quiet(5) + with_out(2600, 472) + quiet(6) + with_out(300, 7, 1, 100) + [0]
    lens = np.array(lens, dtype=np.int64)
    out_off = _offsets(np.maximum(lens - window + 1, 0))
    n_out, per_row = int(out_off[-1]), np.diff(out_off)
    assert n_out >= 4 * TILE_OUT
    assert np.any((out_off[1:] == TILE_OUT) & (per_row > 0))           # some row's last output is output 1023
    at_boundary = set()
    run = 0
    for r in range(lens.size):                                         # runs of >= 5 rows without output that lie AT a tile boundary:
        run = run + 1 if per_row[r] == 0 else 0                        # behind the tile that ends there, in front of the next one
        if run >= 5 and 0 < out_off[r] < n_out and out_off[r] % TILE_OUT == 0:
            at_boundary.add(int(out_off[r]))
    assert len(at_boundary) >= 2, at_boundary
    assert per_row.max() > 2500 and per_row[0] == 0 and per_row[-1] == 0
    return lens


def _python_hash(codes, at, k, alphabet):
    h = sum(int(codes[at + j]) * alphabet ** j for j in range(k)) % (1 << 64)           # plain Python integers, then int64
    return h - (1 << 64) if h >= 1 << 63 else h


def _check_generic(ops, codes, lens, alphabet, k, window, seed):
    lens = np.asarray(lens, dtype=np.int64)
    n_rows, in_off = lens.size, _offsets(lens)
    d_codes, d_in = _hd(codes, np.uint8), _h(in_off)
    rng = np.random.default_rng(seed)
    for w in sorted({k, window}):                                      # w == k: the hashes themselves; else the windows' minima
        out_off = _offsets(np.maximum(lens - w + 1, 0))
        n_out = int(out_off[-1])
        if w == k:
            got = ops.kmers_generic(d_codes, d_in, _h(out_off), n_rows, n_out, k, alphabet).host()
            assert np.array_equal(got, oracle.get_kmers_generic(codes, lens, k, alphabet)[0])
        if window == w:
            mins = ops.minimizers_generic(d_codes, d_in, _h(out_off), n_rows, n_out, k, w, alphabet).host()
            assert np.array_equal(mins, oracle.get_minimizers(codes, lens, k, w, alphabet)[0])
        if n_out == 0:
            continue
        for o in rng.integers(0, n_out, size=50):                      # independent of the oracle's numpy: Python integers
            row = int(np.searchsorted(out_off, o, side="right")) - 1
            at = int(in_off[row] + o - out_off[row])
            if w == k:
                assert got[o] == _python_hash(codes, at, k, alphabet), (o, row)
            if window == w:
                assert mins[o] == min(_python_hash(codes, at + m, k, alphabet) for m in range(w - k + 1)), (o, row)
    if alphabet == 4 and k <= 31:                                      # the 2-bit kernel on the packed form of the same rows
        out_off = _offsets(np.maximum(lens - k + 1, 0))
        n_out = int(out_off[-1])
        if n_out:
            packed = ops.pack_codes(_hd(codes, np.uint8))
            two_bit = ops.kmers(packed, d_in, _h(out_off), n_rows, n_out, k, total=int(in_off[-1])).host()
            assert np.array_equal(two_bit, ops.kmers_generic(d_codes, d_in, _h(out_off), n_rows, n_out, k, 4).host())


GENERIC_PARAMETERS = [(2, 1, 1), (5, 3, 6), (20, 15, 17), (255, 8, 8), (255, 31, 40), (4, 31, 31)]


@pytest.mark.gpu
@pytest.mark.parametrize("alphabet,k,window", GENERIC_PARAMETERS)
def test_generic_kmers_and_minimizers_across_tiles(ops, alphabet, k, window):
    """hashes sum code * A^j in wrapping int64 and the signed minimum per window, rows laid out around the kernel's tiles
    (_tile_edge_lengths, once for the k-mers and once for the windows), against the oracle and against Python integers"""
    for w in sorted({k, window}):
        lens = _tile_edge_lengths(k, w)
        rng = np.random.default_rng(alphabet * 1000 + k * 40 + w)
        codes = rng.integers(0, alphabet, size=int(lens.sum())).astype(np.uint8)
        assert lens[-1] == 0 and lens[-2] >= w                         # the last row WITH output ends the buffer:
        codes[-1] = alphabet - 1                                        # the largest code in its last letter
        _check_generic(ops, codes, lens, alphabet, k, w, seed=k)
        if (alphabet, k) == (20, 15):                                  # 20^15 > 2^63: wrapped hashes, negative ones in the minimum
            assert oracle.get_kmers_generic(codes, lens, k, alphabet)[0].min() < 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_rows,max_len,alphabet,k,window", [(1, 1, 5, 3, 2, 4), (2, 300, 40, 21, 5, 9), (3, 3000, 60, 255, 31, 33),
                                                                  (4, 7, 20_000, 7, 12, 12)])
def test_generic_kmers_and_minimizers_random(ops, seed, n_rows, max_len, alphabet, k, window):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n_rows).astype(np.int64)
    codes = rng.integers(0, alphabet, size=int(lens.sum())).astype(np.uint8)
    _check_generic(ops, codes, lens, alphabet, k, window, seed)


# ------------------------------------------------------------------------------------ 3. count_weighted
def _weighted_case(seed, form, n, n_rows, n_bins, dtype):
    """(values, weights, value_stride, weight_stride, facts): form "flat" = one row; "w2d" = flat values under a matrix of
    weights (strides 0, n); "v2d" = a matrix of values under one row of weights (strides n, 0)"""
    rng = np.random.default_rng(seed)
    assert (form == "flat") == (n_rows == 1)
    v_shape = (n_rows, n) if form == "v2d" else (1, n)
    w_shape = (n_rows, n) if form == "w2d" else (1, n)
    facts = {}
    # the last bin is kept for the +x / -x pairs of the float case
    pairs = dtype == np.float64 and n_bins >= 2 and n >= 8
    values = rng.integers(0, n_bins - 1 if pairs else n_bins, size=v_shape, dtype=np.int64)
    if dtype == np.int64:
        weights = rng.integers(-1000, 1000, size=w_shape, dtype=np.int64)
        if n >= 4:                                                      # bin 0 wraps: 2^63 + 6 on top of the small ones
            weights[:, :4] = [1 << 62, 1 << 62, (1 << 62) - 1, 7]
            values[:, :4] = 0
        if n >= 6 and n_bins >= 2:                                      # ... and the last bin wraps the other way
            weights[:, 4:6] = [-(1 << 62), -(1 << 62) - 9]
            values[:, 4:6] = n_bins - 1
    else:
        weights = rng.choice([-1.0, 1.0], size=w_shape) * 10.0 ** rng.uniform(-3, 5, size=w_shape)
        if pairs:                                                       # +1.5 and -1.5, three times: every partial sum is a small multiple
            cols = rng.choice(n, size=6, replace=False)                 # of 1.5, so the bin's sum is EXACTLY 0 in any order (and an
            values[:, cols] = n_bins - 1                                # LDS bin that holds 0 is not flushed)
            weights[:, cols] = [1.5, -1.5, 1.5, -1.5, -1.5, 1.5]
            facts["zero_bin"] = n_bins - 1
            if n_bins >= 3:
                rest = np.setdiff1d(np.arange(n), cols)
                a, b = rng.choice(rest, size=2, replace=False)
                values[:, a], weights[:, a] = 0, np.nan
                values[:, b], weights[:, b] = 1, np.inf
    vstride, wstride = (n if form == "v2d" else 0), (n if form == "w2d" else 0)
    return values, weights, vstride, wstride, facts


def _weighted_expectation(values, weights, n_rows, n_bins):
    """int64: the whole histogram by np.add.at, which wraps like the kernel.  float64: for every (row, bin) that receives a
    weight — (its flat index, math.fsum of its weights, their number, their sum of |w|); NaN / inf bins as numpy sums them"""
    n = values.shape[1]
    V, W = np.broadcast_to(values, (n_rows, n)), np.broadcast_to(weights, (n_rows, n))
    key = (np.arange(n_rows, dtype=np.int64)[:, None] * n_bins + V).reshape(-1)
    w = W.reshape(-1)
    if w.dtype == np.int64:
        out = np.zeros(n_rows * n_bins, dtype=np.int64)
        np.add.at(out, key, w)
        return out
    order = np.argsort(key, kind="stable")
    key, w = key[order], w[order]
    starts = np.flatnonzero(np.concatenate(([True], key[1:] != key[:-1])))
    counts = np.diff(np.concatenate((starts, [key.size])))
    sums = w[starts].copy()                                             # (a bin with one weight is that weight)
    with np.errstate(invalid="ignore"):
        sum_abs = np.add.reduceat(np.abs(w), starts)                    # (the bound's scale; its own rounding is nothing to the bound)
        for g in np.flatnonzero(counts > 1):
            part = w[starts[g]:starts[g] + counts[g]]
            sums[g] = math.fsum(part) if np.all(np.isfinite(part)) else np.sum(part)
    return key[starts], sums, counts, sum_abs


def _check_weighted(ops, seed, form, n, n_rows, n_bins, dtype):
    values, weights, vstride, wstride, facts = _weighted_case(seed, form, n, n_rows, n_bins, dtype)
    got = ops.count_weighted(_h(values.reshape(-1)), _h(weights.reshape(-1)), n, n_rows, vstride, wstride, n_bins).host()
    assert got.dtype == dtype and got.size == n_rows * n_bins
    if dtype == np.int64:
        expect = _weighted_expectation(values, weights, n_rows, n_bins)
        assert np.array_equal(got, expect), np.flatnonzero(got != expect)[:5]
        return
    bins, sums, counts, sum_abs = _weighted_expectation(values, weights, n_rows, n_bins)
    at = got[bins]
    finite = np.isfinite(sums)
    assert np.array_equal(at[~finite], sums[~finite], equal_nan=True)
    with np.errstate(invalid="ignore"):
        bad = np.flatnonzero(finite & ~(np.abs(at - sums) <= _sum_bound(counts, sum_abs)))
    assert bad.size == 0, [(int(bins[i]), at[i], sums[i], int(counts[i]), sum_abs[i]) for i in bad[:5]]
    rest = got.copy()
    rest[bins] = 0
    assert not rest.any()                                               # the bins nobody added to
    if "zero_bin" in facts:
        assert not got.reshape(n_rows, n_bins)[:, facts["zero_bin"]].any()


WEIGHTED_CASES = [
    # one workgroup per row (5000 rows): its loop runs for n > 256
    ("v2d", 1, 5000, 4, np.int64), ("w2d", 255, 5000, 1, np.float64), ("v2d", 256, 5000, 4, np.float64),
    ("w2d", 257, 5000, 4097, np.int64), ("w2d", 257, 5000, 4096, np.float64), ("v2d", 700, 5000, 4, np.int64),
    ("v2d", 700, 5000, 4, np.float64), ("w2d", 700, 5000, 1, np.int64),
    # one row: the bins on either side of the LDS limit, the capped grid's loop
    ("flat", 1, 1, 1, np.int64), ("flat", 5000, 1, 4096, np.int64), ("flat", 5000, 1, 4097, np.float64),
    ("flat", 5000, 1, 4096, np.float64), ("flat", 5000, 1, 4097, np.int64),
    ("flat", 1_200_000, 1, 70_000, np.float64), ("flat", 1_200_000, 1, 4, np.int64), ("flat", 1_200_000, 1, 4096, np.float64),
    # many bins and several rows; the limit of gridDim.y
    ("w2d", 300, 40, 70_000, np.float64), ("v2d", 300, 40, 70_000, np.int64),
    ("v2d", 2, 65_535, 4, np.int64), ("w2d", 2, 65_535, 1, np.float64)]


@pytest.mark.gpu
@pytest.mark.parametrize("form,n,n_rows,n_bins,dtype", WEIGHTED_CASES)
def test_count_weighted_paths_and_strides(ops, form, n, n_rows, n_bins, dtype):
    """hist[r, values[r * vstride + i]] += weights[r * wstride + i] against np.add.at (int64, wrapping) and math.fsum per bin
    (float64, within _sum_bound(weights in the bin, their sum of |w|); NaN / inf bins as numpy sums them)"""
    _check_weighted(ops, n + n_bins, form, n, n_rows, n_bins, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", [4, 4096, 4097, 70_000])
@pytest.mark.parametrize("bad", [-1, 0])
def test_count_weighted_refuses_a_value_outside_the_bins(ops, n_bins, bad):
    """-1, and n_bins itself (bad = 0), in an otherwise valid input: the flag of the LDS and of the global path"""
    rng = np.random.default_rng(n_bins)
    for dtype in (np.int64, np.float64):
        values = rng.integers(0, n_bins, size=1000, dtype=np.int64)
        weights = np.ones(1000, dtype=dtype)
        assert ops.count_weighted(_h(values), _h(weights), 1000, 1, 0, 0, n_bins).host().sum() == 1000
        values[517] = bad if bad < 0 else n_bins
        with pytest.raises(ValueError, match="outside the alphabet"):
            ops.count_weighted(_h(values), _h(weights), 1000, 1, 0, 0, n_bins)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_rows,max_len", [(1, 1, 1), (2, 17, 300), (3, 3000, 40), (4, 1, 100_000)])
def test_count_weighted_random(ops, seed, n_rows, max_len):
    rng = np.random.default_rng(seed)
    n_rows = min(n_rows, 65_535)
    n = int(rng.integers(1, max(1, min(max_len, 4_000_000 // n_rows)) + 1))        # (a few million weights at the most)
    fits = [b for b in (1, 4, 64, 4096, 4097, 70_000) if b * n_rows <= 1 << 24]
    for dtype in (np.int64, np.float64):
        form = "flat" if n_rows == 1 else str(rng.choice(["w2d", "v2d"]))
        _check_weighted(ops, seed, form, n, n_rows, int(rng.choice(fits)), dtype)


# ------------------------------------------------------------------------------------ 4. count_dense_rows
def _check_dense_rows(ops, seed, lens, n_bins):
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n, n_rows = int(lens.sum()), lens.size
    values = rng.integers(0, n_bins, size=n, dtype=np.int64)
    spoil = rng.random(n)
    values[spoil < 0.05] = -1                                           # outside the bins: skipped, silently
    values[(spoil >= 0.05) & (spoil < 0.10)] = n_bins
    values[(spoil >= 0.10) & (spoil < 0.15)] = 1 << 62
    got = ops.count_dense_rows(_h(values), _h(_offsets(lens)), n_rows, n_bins).host().reshape(n_rows, n_bins)
    off = _offsets(lens)
    for r in range(n_rows):
        row = values[off[r]:off[r + 1]]
        row = row[(row >= 0) & (row < n_bins)]
        assert np.array_equal(got[r], np.bincount(row, minlength=n_bins)), r


def _dense_rows_lengths(shape, n):
    """row lengths that add up to n: "edges" = 3 empty rows first, 3 last and a run of 10 between two halves; "single" = one row"""
    if shape == "single":
        return [n]
    rng = np.random.default_rng(n)
    def pieces(total, k):
        cuts = np.sort(rng.integers(0, total + 1, size=k - 1))
        return np.diff(np.concatenate(([0], cuts, [total]))).tolist()
    lens = [0, 0, 0] + pieces(n // 2, 9) + [0] * 10 + pieces(n - n // 2, 9) + [0, 0, 0]
    assert sum(lens) == n
    return lens


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["edges", "single"])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70_001])
def test_count_dense_rows_with_empty_rows_and_foreign_values(ops, shape, n):
    """one np.bincount per row over the values inside the bins (-1, n_bins and 2^62 among them are ignored)"""
    for n_bins in (1, 64, 5000):
        _check_dense_rows(ops, n + n_bins, _dense_rows_lengths(shape, n), n_bins)


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", [1, 64, 5000])
def test_count_dense_rows_of_one_element_each(ops, n_bins):
    _check_dense_rows(ops, n_bins, [1] * 1000, n_bins)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,n_rows,max_len", [(1, 1, 1), (2, 300, 50), (3, 4000, 151), (4, 3, 40_000)])
def test_count_dense_rows_random(ops, seed, n_rows, max_len):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, max_len + 1, size=n_rows)
    lens[rng.integers(0, n_rows, size=max(1, n_rows // 8))] = 0
    lens[rng.integers(0, n_rows)] = max_len
    _check_dense_rows(ops, seed, lens, int(rng.choice([1, 4, 64, 1000])))


# ------------------------------------------------------------------------------------ 5. multiline_wrap
def _wrapped(name, seq, width, marker=b">"):
    """marker + name + newline, then the sequence in slices of ``width``, each followed by a newline.  A record with an EMPTY
    sequence is its header line alone: the reference's from_data (io/multiline_buffer.py:71-76) gets n_lines = 0 for it and then
    writes last_length + 1 over the header's own line length — it has no answer for that record — and the project's restatement
    says what is written instead (oracle/text.py: multiline_from_data, "written as their header line only")."""
    return marker + name + b"\n" + b"".join(seq[i:i + width] + b"\n" for i in range(0, len(seq), width))


def _check_wrap(ops, width, seq_lens, name_lens, seed):
    rng = np.random.default_rng(seed)
    seqs = [rng.choice(np.frombuffer(b"ACGTNacgt", dtype=np.uint8), size=n).tobytes() for n in seq_lens]
    names = [rng.integers(33, 127, size=n).astype(np.uint8).tobytes() for n in name_lens]
    n_rec = len(seqs)
    records = [_wrapped(nm, sq, width) for nm, sq in zip(names, seqs)]
    expect = np.frombuffer(b"".join(records), dtype=np.uint8)
    # (buffers without a byte in them stay empty: records without names, or without sequences, are legal input)
    d_names, d_seq = _h(np.frombuffer(b"".join(names), dtype=np.uint8).copy()), _h(np.frombuffer(b"".join(seqs), dtype=np.uint8).copy())
    d_noff, d_soff = _h(_offsets(name_lens)), _h(_offsets(seq_lens))
    got = ops.multiline_wrap(d_names, d_noff, d_seq, d_soff, n_rec, width, ord(">")).host()
    assert np.array_equal(got, expect)
    if getattr(ops, "host_only", False):                                # (the stand-in has no two-call form)
        return
    from bionumpy_amd._native import lib
    from bionumpy_amd.device import ptr
    out_off, total = ops._empty(n_rec + 1, np.int64), C.c_int64(-1)
    args = (ptr(d_names.dev()), ptr(d_noff.dev()), ptr(d_seq.dev()), ptr(d_soff.dev()), n_rec, width, ord(">"), ptr(out_off))
    assert lib.bnpk_multiline_wrap(ops.ctx, *args, None, 0, C.byref(total), ops._s()) == 0         # sizes only
    assert total.value == expect.size
    assert np.array_equal(out_off.cpu().numpy(), _offsets([len(r) for r in records]))
    out = ops._empty(expect.size + 1, np.uint8)
    out[:] = 7
    assert lib.bnpk_multiline_wrap(ops.ctx, *args, ptr(out), expect.size - 1, C.byref(total), ops._s()) == ERR_ARG
    assert total.value == expect.size and bool((out == 7).all())                                   # refused: nothing written
    assert lib.bnpk_multiline_wrap(ops.ctx, *args, ptr(out), expect.size, C.byref(total), ops._s()) == 0
    assert total.value == expect.size and np.array_equal(out.cpu().numpy()[:-1], expect) and int(out[-1]) == 7
    assert np.array_equal(out_off.cpu().numpy(), _offsets([len(r) for r in records]))


def _wrap_lengths(width):
    return [0, 1, width - 1, width, width + 1, 2 * width, 2 * width + 1, 10_000 * width + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("width", [1, 7, 80])
@pytest.mark.parametrize("n_records", [1, 2, 2000])
def test_multiline_wrap_line_and_record_edges(ops, width, n_records):
    """the text of multi-line FASTA records against plain Python slices: out_offsets and the total of the sizes-only call, the
    bytes, and BNPK_ERR_ARG for a buffer one byte short"""
    lengths, name_lengths = _wrap_lengths(width), [0, 1, 300]
    if n_records == 1:
        for i, n in enumerate(lengths):
            _check_wrap(ops, width, [n], [name_lengths[i % 3]], i)
        _check_wrap(ops, width, [0], [0], 99)                           # the smallest text there is: ">\n"
    elif n_records == 2:
        for i in range(len(lengths)):
            _check_wrap(ops, width, [lengths[i], lengths[i - 1]], [name_lengths[i % 3], name_lengths[(i + 1) % 3]], i)
        _check_wrap(ops, width, [0, 0], [5, 0], 98)                     # no sequence at all
        _check_wrap(ops, width, [width, 3], [0, 0], 97)                 # no name at all
    else:                                                               # (the longest record once: it is most of the text already)
        seq_lens = [lengths[i % 7] for i in range(n_records)]
        seq_lens[1234] = lengths[7]
        _check_wrap(ops, width, seq_lens, [name_lengths[i % 3] for i in range(n_records)], n_records)


# ------------------------------------------------------------------------------------ 6. packed_rows_slice
SLICE_LENGTHS = [32, 1, 31, 7, 0, 0, 0, 33, 64, 16, 31, 200, 7, 0, 100, 150, 199, 63, 5, 27, 1, 0, 0, 180, 90, 45, 2, 3, 128, 96, 11,
                 13, 17, 19, 160, 170, 0, 31, 32, 33, 64, 9]


def _slice_pairs(lens):
    """(first_row, n_rows) pairs: every seventh of all of them, and by name the ones the kernel's branches need — asserted"""
    off = _offsets(lens)
    n, total = len(lens), int(off[-1])
    everything = [(r0, m) for r0 in range(n + 1) for m in range(n - r0 + 1)]
    def first_with(pred):
        found = [p for p in everything if pred(int(off[p[0]]), int(off[p[0] + p[1]] - off[p[0]]), p)]
        assert found, "SLICE_LENGTHS lost a slice the test is there for"
        return found[0]
    named = [(0, n)]                                                    # the whole batch
    for residue in (0, 1, 31, 16):
        named.append(first_with(lambda first, nb, p: first % 32 == residue and nb > 40 and first > 0))
    named.append(first_with(lambda first, nb, p: first % 32 not in (0,) and first + nb == total and nb > 0))   # ends in the last word
    named.append(first_with(lambda first, nb, p: nb == 0 and p[1] >= 3 and first % 32 != 0))                   # empty rows only
    for want in (31, 32, 33, 64):
        named.append(first_with(lambda first, nb, p: nb == want and first % 32 != 0))
        named.append(first_with(lambda first, nb, p: nb == want))
    assert total % 32 != 0                                              # the input's last word is a partial one
    return sorted(set(named + everything[::7]))


@pytest.mark.gpu
def test_packed_rows_slice_at_every_shift(ops):
    """rows [first_row, first_row + n_rows) of a packed batch == the same rows packed from scratch (pack_codes of their codes:
    the words, the zero bits behind the last base and the two zero words) and their offsets minus the first base — with ones
    in every bit of the input behind its last base"""
    rng = np.random.default_rng(6)
    lens = np.array(SLICE_LENGTHS, dtype=np.int64)
    assert lens.min() == 0 and lens.max() == 200
    off = _offsets(lens)
    total = int(off[-1])
    codes = rng.integers(0, 4, size=total).astype(np.uint8)
    words = ops.pack_codes(_h(codes)).host().view(np.uint64).copy()
    assert words.size == total // 32 + 2
    words[total // 32] |= ~np.uint64((1 << (2 * (total % 32))) - 1)     # ones behind the last base, in its word ...
    words[total // 32 + 1:] = ~np.uint64(0)                             # ... and in the padding word
    packed = _h(words.view(np.int64))
    for r0, m in _slice_pairs(lens):
        first, n_bases = int(off[r0]), int(off[r0 + m] - off[r0])
        out, out_off = ops.packed_rows_slice(packed, total, _h(off), r0, m, first, n_bases)
        n_words = (n_bases + 31) // 32                                  # the words that hold bases, then zero words (pack_codes itself
        fresh = np.zeros(n_bases // 32 + 2, dtype=np.int64)             # writes one word behind them and leaves a second one alone)
        fresh[:n_words] = ops.pack_codes(_hd(codes[first:first + n_bases], np.uint8)).host()[:n_words]
        assert out.host().size == n_bases // 32 + 2 and np.array_equal(out.host(), fresh), (r0, m, first % 32, n_bases)
        assert not out.host()[(n_bases + 31) // 32:].any()
        assert np.array_equal(out_off.host(), off[r0:r0 + m + 1] - first), (r0, m)


# ------------------------------------------------------------------------------------ the same functions on the host
def test_the_expectations_hold_for_the_reference_alone():
    """every parity function above at its fixed cases with the oracle-backed stand-in for ``ops``: the expectations, the
    generators' assertions about their own shapes and the two summation bounds hold where no kernel is involved.  Nothing is
    left out: the cases of 65 535 rows and of 1.2 M values take about a second each in numpy."""
    from oracle_ops import OracleOps
    ops = OracleOps()
    for dtype in (np.int64, np.float64):
        _check_wide(ops, _wide_edge_rows(dtype))
    for alphabet, k, window in GENERIC_PARAMETERS:
        test_generic_kmers_and_minimizers_across_tiles(ops, alphabet, k, window)
    for case in WEIGHTED_CASES:
        test_count_weighted_paths_and_strides(ops, *case)
    for n_bins in (4, 4096, 4097, 70_000):
        for bad in (-1, 0):
            test_count_weighted_refuses_a_value_outside_the_bins(ops, n_bins, bad)
    for shape in ("edges", "single"):
        for n in (1, 255, 256, 257, 70_001):
            test_count_dense_rows_with_empty_rows_and_foreign_values(ops, shape, n)
    for n_bins in (1, 64, 5000):
        test_count_dense_rows_of_one_element_each(ops, n_bins)
    for width in (1, 7, 80):
        for n_records in (1, 2, 2000):
            test_multiline_wrap_line_and_record_edges(ops, width, n_records)
    test_packed_rows_slice_at_every_shift(ops)
