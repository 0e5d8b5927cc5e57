"""-m gpu: BloomFilter (csrc/bloom.hip) against a numpy restatement of the placement written out in include/bnpk.h.  Every
comparison is exact: filter words, flags and per-row hit counts are integers and booleans."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = np.uint64
COMPLEMENT = str.maketrans("ACGT", "TGCA")
FILTERS = [(1, 1), (3, 5), (64, 4), (1000, 4), (2 ** 20 + 7, 4)]          # (n_blocks, n_hashes)


def fmix(x):
    x = x.astype(U).copy()
    x ^= x >> U(33); x *= U(0xff51afd7ed558ccd); x ^= x >> U(33); x *= U(0xc4ceb9fe1a85ec53); x ^= x >> U(33)
    return x


def rc(h, k):
    out = np.zeros_like(h)
    for i in range(k):
        out |= (U(3) - ((h >> U(2 * i)) & U(3))) << U(2 * (k - 1 - i))
    return out


def place(kmers, k, n_blocks, n_hashes, seed, canonical):
    h = kmers.astype(U)
    if canonical:
        h = np.minimum(h, rc(h, k))
    g = fmix(h ^ U(seed))
    block = ((g >> U(32)) * U(n_blocks)) >> U(32)
    bits = np.zeros_like(g)
    for j in range(n_hashes):
        bits |= U(1) << ((g >> U(6 * j)) & U(63))
    return block.astype(np.int64), bits


def build(kmers, k, n_blocks, n_hashes, seed, canonical):
    words = np.zeros(n_blocks, dtype=U)
    np.bitwise_or.at(words, *place(kmers, k, n_blocks, n_hashes, seed, canonical))
    return words


def query(words, kmers, k, n_hashes, seed, canonical):
    block, bits = place(kmers, k, len(words), n_hashes, seed, canonical)
    return (words[block] & bits) == bits


def kmers_of(row, k):
    """int64 hashes of the k-mers of a string, first base in the low 2 bits"""
    codes = np.array(["ACGT".index(c) for c in row], dtype=np.int64)
    if codes.size < k:
        return np.zeros(0, dtype=np.int64)
    return np.lib.stride_tricks.sliding_window_view(codes, k) @ (4 ** np.arange(k, dtype=np.int64))


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


@pytest.fixture(scope="module")
def data(bnp):
    """rows at the kernels' edges (a lane owns 8 positions, a packed word 32 bases, a tile 2048 positions, the LDS table 510
    rows); every third row is cut from the genome the filters of test_count_hits are built from, every third from its reverse
    complement, the rest is random.  Computed once: the rows' k-mers per k."""
    rng = random.Random(20261126)
    genome = ["".join(rng.choice("ACGT") for _ in range(6000)) for _ in range(2)]
    lengths = [0, 0, 1, 2, 3, 4, 31, 32, 33, 63, 64, 65] + [150] * 30 + [3] * 700 + [2047, 2048, 2049, 9000] + [151] * 20 + [0, 5]
    rows = []
    for i, n in enumerate(lengths):
        at = rng.randrange(6000 - n) if n < 6000 else 0
        cut = genome[i % 2][at:at + n]
        rows.append("".join(rng.choice("ACGT") for _ in range(n)) if i % 3 == 2 or n >= 6000 else
                    cut if i % 3 == 0 else cut.translate(COMPLEMENT)[::-1])
    per_row = {k: [kmers_of(row, k) for row in rows] for k in (1, 3, 5, 21, 31)}
    return genome, rows, bnp.as_encoded_array(rows, bnp.DNAEncoding), per_row


@pytest.mark.parametrize("n_blocks,n_hashes", FILTERS)
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k", [1, 5, 21, 31])
def test_filter_words(bnp, data, k, canonical, n_blocks, n_hashes):
    _, _, reads, per_row = data
    want = build(np.concatenate(per_row[k]), k, n_blocks, n_hashes, 7, canonical)
    by_hashes = bnp.BloomFilter(n_blocks, n_hashes=n_hashes, seed=7, k=k, canonical=canonical)
    by_hashes.insert(bnp.get_kmers(reads, k))
    fused = bnp.BloomFilter(n_blocks, n_hashes=n_hashes, seed=7, k=k, canonical=canonical)
    fused.insert(reads)
    assert np.array_equal(by_hashes.words().host(), want)
    assert np.array_equal(fused.words().host(), want)


@pytest.mark.parametrize("k", [21, 31])
def test_query(bnp, data, k):
    rng = np.random.default_rng(k)
    inserted = rng.integers(0, 4 ** k, 700, dtype=np.int64)
    others = np.setdiff1d(rng.integers(0, 4 ** k, 2000, dtype=np.int64), inserted)
    bf = bnp.BloomFilter(64, n_hashes=4, seed=0, k=k)
    bf.insert(inserted[:350])
    bf.insert(inserted[350:].tolist())                        # (a list of ints is k-mers, as for bf[...])
    asked = np.concatenate([inserted, others])                # (2700 or so: not a multiple of a lane's eight)
    want = query(build(inserted, k, 64, 4, 0, False), asked, k, 4, 0, False)
    assert want[:700].all() and want[700:].any() and not want[700:].all()     # members, false positives, negatives
    got = bf[asked]
    assert np.asarray(got).dtype == bool and np.array_equal(np.asarray(got), want)
    assert np.array_equal(np.asarray(bf[asked.astype(np.uint64)]), want) and np.asarray(bf[asked[:5].tolist()]).all()
    with pytest.raises(TypeError):
        bf[asked.astype(np.int32)]
    _, _, reads, per_row = data
    ragged = bf[bnp.get_kmers(reads, k)]
    assert [len(row) for row in ragged.tolist()] == [len(row) for row in per_row[k]]
    assert np.array_equal(np.asarray(ragged.ravel()), query(bf.words().host(), np.concatenate(per_row[k]), k, 4, 0, False))


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,ref_len", [(3, 30), (21, 6000), (31, 6000)])
def test_count_hits(bnp, data, k, ref_len, canonical):
    genome, _, reads, per_row = data
    ref = [g[:ref_len] for g in genome] + ["ACG"[:k - 1]]        # (text in, and a row too short for a k-mer)
    ref_kmers = np.concatenate([kmers_of(g, k) for g in ref])
    bf = bnp.BloomFilter.from_sequences(ref, k=k, bits_per_kmer=16, n_hashes=4, canonical=canonical, seed=3)
    assert bf.n_blocks == -(-ref_kmers.size * 16 // 64)
    words = build(ref_kmers, k, bf.n_blocks, 4, 3, canonical)
    assert np.array_equal(bf.words().host(), words)
    want = [int(query(words, row, k, 4, 3, canonical).sum()) for row in per_row[k]]
    with_kmers = [n for n, row in zip(want, per_row[k]) if row.size]
    assert any(with_kmers) and not all(with_kmers)            # reads that hit, and reads with k-mers that miss
    assert np.asarray(bf.count_hits(reads)).tolist() == want


def test_cumulative_and_contended(bnp, data):
    _, rows, reads, per_row = data
    one = bnp.BloomFilter(1000, k=21, canonical=True)
    one.insert(reads)
    two = bnp.BloomFilter(1000, k=21, canonical=True)
    two.insert(bnp.as_encoded_array(rows[:400], bnp.DNAEncoding))
    two.insert(rows[400:])
    assert np.array_equal(one.words().host(), two.words().host())
    kmers = np.concatenate([np.full(100_000, per_row[21][6][0]), per_row[21][7], np.full(100_000, per_row[21][8][2])])
    bf = bnp.BloomFilter(3, n_hashes=5, k=21)
    bf.insert(kmers[:150_000])
    bf.insert(kmers[150_000:])
    assert np.array_equal(bf.words().host(), build(kmers, 21, 3, 5, 0, False))


def test_refusals(bnp, data):
    from bionumpy_amd import _native
    from bionumpy_amd.device import ptr
    for bad in (dict(k=32), dict(n_hashes=6), dict(n_blocks=0), dict(n_blocks=2 ** 32)):
        with pytest.raises(ValueError):
            bnp.BloomFilter(**{"n_blocks": 64, **bad})
    bf = bnp.BloomFilter(64, k=21)
    with pytest.raises(ValueError):
        bf.insert(bnp.get_kmers(data[2], 31))
    ops = bnp.ops.get_ops()
    kmers, flags = ops._empty(8, np.int64), ops._empty(8, np.uint8)

    def call(n=8, **changed):
        desc = _native.Bloom.from_buffer_copy(bf._native)
        for name, value in changed.items():
            setattr(desc, name, value)
        return _native.lib.bnpk_bloom_query_hashes(ops.ctx, C.byref(desc), ptr(kmers), n, ptr(flags), ops._s())
    assert call(k=32) == -1 and call(k=0) == -1 and call(n_hashes=6) == -1 and call(d_words=None) == -1     # BNPK_ERR_ARG
    assert call(n_blocks=0) == -6 and call(n_blocks=2 ** 32) == -6                                          # BNPK_ERR_RANGE
    assert call(n=0) == 0
