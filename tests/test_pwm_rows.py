"""-m gpu: bnpk_pwm_rows_packed / _bytes and bnp.scan_motifs (csrc/pwm_rows.hip) against numpy's calculate_scores loop, restated
here.  Every comparison is exact (np.array_equal): the kernel adds in the reference's order, so scores are bit-identical."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECE = 2048                                                   # positions of a row per piece (csrc/pwm_rows.hip)
EDGE_WIDTHS = [1, 2, 31, 32, 33, 64]
PLANTED = np.array([2, 0, 3, 3, 0, 1, 0, 2])                   # the window the "planted" motif scores highest
LONG = 4 * PIECE + 500                                         # more than three pieces and a remainder
PLANTS = {0: 100, 1: 2 * PIECE + 7, 2: 4 * PIECE + 300}        # long row -> where PLANTED lies: first, a middle, the last piece
# W - 1, W, W + 1 of every edge width; a word's and a lane's edges; a piece's length - 1, 0, + 1; reads
LENGTHS = [0, 1, 2, 3, 30, 31, 32, 33, 34, 63, 64, 65, 150, PIECE - 1, PIECE, PIECE + 1]


def ref_scores(codes, matrix):
    """PWM.calculate_scores of the reference on one row; matrix[code][position]"""
    n, width = codes.size, matrix.shape[1]
    if n < width:
        return np.zeros(0)
    scores = np.zeros(n, dtype=np.float64)
    for offset, row in enumerate(matrix.T):
        scores[:n - offset] += row[codes[offset:]]
    return scores[:n - width + 1]


def reference(rows, matrices, both, thresholds):
    """(best, position, strand, hits), each n_motifs x n_rows; thresholds: per motif a number or ("row", r): the best forward
    score of row r (a value from the data: >= must count equality)"""
    shape = (len(matrices), len(rows))
    best, pos = np.full(shape, -np.inf), np.full(shape, -1, dtype=np.int64)
    strand, hits, thr = np.zeros(shape, dtype=np.uint8), np.zeros(shape, dtype=np.int64), np.zeros(len(matrices))
    for m, matrix in enumerate(matrices):
        t = thresholds[m]
        thr[m] = ref_scores(rows[t[1]], matrix).max() if isinstance(t, tuple) else t
        for r, codes in enumerate(rows):
            fwd = ref_scores(codes, matrix)
            rev = ref_scores(3 - codes[::-1], matrix)[::-1] if both else np.zeros(0)
            scores = np.concatenate([fwd, rev])
            if scores.size:
                k = int(np.argmax(scores))
                best[m, r], strand[m, r], pos[m, r] = scores[k], k >= fwd.size, k % fwd.size
                hits[m, r] = (scores >= thr[m]).sum()
    return best, pos, strand, hits, thr


def make_rows(alphabet_size):
    rng = np.random.default_rng(20261126 + alphabet_size)
    lengths = LENGTHS + [LONG, 0, 0, LONG] + [3] * 300 + [0, LONG, 0, 5]
    rows = [rng.integers(0, alphabet_size, n).astype(np.uint8) for n in lengths]
    for i, r in enumerate(k for k, n in enumerate(lengths) if n == LONG):
        rows[r][PLANTS[i]:PLANTS[i] + PLANTED.size] = PLANTED % alphabet_size
    return rows


def make_library(kind, widths, alphabet_size, seed):
    rng = np.random.default_rng(seed)
    out = []
    for w in widths:
        if kind == "binary":                                   # ties are the rule: forward before reverse, then the smaller p
            m = rng.integers(0, 2, (alphabet_size, w)).astype(np.float64)
        elif kind == "planted":
            m = -rng.random((alphabet_size, w))
            m[PLANTED % alphabet_size, np.arange(w)] = 2.0
        else:
            m = rng.normal(size=(alphabet_size, w)) * 3
            m[rng.random((alphabet_size, w)) < 0.1] = -np.inf
        out.append(m)
    if kind == "minus_inf":
        out[1][:] = -np.inf                                    # every window -inf: position 0, not -1
    return out


LIBRARIES = {"edges": ("random", EDGE_WIDTHS), "ties": ("binary", EDGE_WIDTHS), "one": ("random", [8]),
             "three": ("minus_inf", [5, 12, 20]), "planted": ("planted", [PLANTED.size]),
             "group_plus_one": ("random", [6 + (i * 5) % 17 for i in range(17)])}


def thresholds_for(n_motifs):
    return [(("row", 12), -np.inf, 1e300)[m % 3] for m in range(n_motifs)]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    yield bionumpy_amd
    bionumpy_amd._native.lib.bnpk_set_option(ops.get_ops().ctx, b"pwm_split", 0)


@pytest.fixture(scope="module")
def inputs(bnp):
    """per alphabet size: the rows, their codes / 2-bit words and offsets in HBM; and the references, computed once per case"""
    from bionumpy_amd.device import HArray
    ops, made, cache = bnp.ops.get_ops(), {}, {}
    for a in (4, 20, 32):
        rows = make_rows(a)
        flat = HArray(host=np.concatenate(rows))
        offsets = HArray(host=np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64))
        made[a] = (rows, ops.pack_codes(flat) if a == 4 else flat, offsets, flat.size)

    def expect(a, name, both):
        if (a, name, both) not in cache:
            kind, widths = LIBRARIES[name]
            matrices = make_library(kind, widths, a, seed=len(name) + a)
            cache[a, name, both] = (matrices,) + reference(made[a][0], matrices, both, thresholds_for(len(matrices)))
        return cache[a, name, both]
    return made, expect


def run(bnp, inputs, a, name, both, split):
    made, expect = inputs
    rows, data, offsets, total = made[a]
    matrices, best, pos, strand, hits, thr = expect(a, name, both)
    ops = bnp.ops.get_ops()
    assert bnp._native.lib.bnpk_set_option(ops.ctx, b"pwm_split", split) == 0
    got = ops.pwm_rows(data, offsets, len(rows), total, matrices, a == 4, both, thr)
    shape = (len(matrices), len(rows))
    assert np.array_equal(got[0].host().reshape(shape), best)
    assert np.array_equal(got[1].host().reshape(shape), pos)
    assert np.array_equal(got[3].host().reshape(shape), hits)
    if a == 4:
        assert np.array_equal(got[2].host().reshape(shape), strand)
    return rows, best, pos, strand, hits


@pytest.mark.parametrize("split", [1, 2])                       # a piece goes to one lane / to one workgroup
@pytest.mark.parametrize("both", [False, True])
@pytest.mark.parametrize("name", sorted(LIBRARIES))
def test_packed(bnp, inputs, name, both, split):
    rows, best, pos, strand, hits = run(bnp, inputs, 4, name, both, split)
    long_rows = [r for r, codes in enumerate(rows) if codes.size == LONG]
    if name == "planted":                                      # the merge sees its maximum in a first, a middle and the last piece
        assert [int(pos[0, r]) for r in long_rows] == [PLANTS[i] for i in range(3)]
        assert [int(pos[0, r]) // PIECE for r in long_rows] == [0, 2, 4] and not strand[0, long_rows].any()
    if name == "ties":
        assert (hits[1::3] > 1).any() and (both is False or strand.any())
    if name == "three":
        assert (pos[1, [r for r, c in enumerate(rows) if c.size >= 12]] == 0).all() and np.isneginf(best[1]).all()
        assert (pos[1, [r for r, c in enumerate(rows) if c.size < 12]] == -1).all()
    assert bnp._native.PWM_GROUP_MOTIFS + 1 == len(LIBRARIES["group_plus_one"][1])


@pytest.mark.parametrize("split", [1, 2])
@pytest.mark.parametrize("a", [20, 32])
@pytest.mark.parametrize("name", ["edges", "ties", "three", "group_plus_one"])
def test_bytes(bnp, inputs, name, a, split):
    run(bnp, inputs, a, name, False, split)


def test_scan_motifs(bnp, inputs):
    rng = np.random.default_rng(5)
    for alphabet, both in (("ACGT", True), ("ACDEFGHIKLMNPQRSTVWY", False)):
        a = len(alphabet)
        rows = make_rows(a)[:len(LENGTHS) + 1]                  # (the edge lengths and a row of several pieces)
        text = ["".join(alphabet[c] for c in r) for r in rows]
        matrices = make_library("random", [3, 12, 33], a, seed=a)
        best, pos, strand, hits, _ = reference(rows, matrices, both, [0.5, 0.5, 0.5])
        seqs = bnp.as_encoded_array(text, bnp.AlphabetEncoding(alphabet))
        scan = bnp.scan_motifs(seqs if a == 4 else text, [bnp.PWM(m, alphabet) for m in matrices], both_strands=both, thresholds=0.5)
        for got, want in ((scan.best_score, best), (scan.best_position, pos), (scan.best_strand, strand), (scan.n_hits, hits)):
            assert got.shape == want.shape and np.array_equal(np.asarray(got), want)
        keep = scan.best_score[1] > 0.0                       # a per-motif row is a device vector: a read filter
        assert np.array_equal(np.asarray(keep), best[1] > 0.0) and len(seqs[np.asarray(keep)]) == int((best[1] > 0.0).sum())
        assert bnp.scan_motifs(seqs, [bnp.PWM(matrices[0], alphabet)]).n_hits is None
    pwm = bnp.PWM(rng.normal(size=(4, 5)), "ACGT")
    with pytest.raises(ValueError):
        bnp.scan_motifs(["ACGT"], [pwm, bnp.PWM(rng.normal(size=(4, 5)), "ACTG")])
    with pytest.raises(ValueError):
        bnp.scan_motifs(["ACD"], [bnp.PWM(rng.normal(size=(20, 2)), "ACDEFGHIKLMNPQRSTVWY")], both_strands=True)
    with pytest.raises(NotImplementedError):
        bnp.scan_motifs(["ACGT"], [bnp.PWM(rng.normal(size=(4, 65)), "ACGT")])


@pytest.mark.parametrize("case", ["nan", "inf_threshold", "width_0", "width_65", "hits_without_thresholds", "ok"])
def test_bad_arguments(bnp, inputs, case):
    from bionumpy_amd._native import lib, PwmLibrary
    from bionumpy_amd.device import ptr
    ops = bnp.ops.get_ops()
    rows, data, offsets, total = inputs[0][4]
    width = np.array([{"width_0": 0, "width_65": 65}.get(case, 4)], dtype=np.int32)
    matrix = np.zeros(65 * 4)
    matrix[5] = np.nan if case == "nan" else -np.inf
    thr = None if case == "hits_without_thresholds" else np.array([np.inf if case == "inf_threshold" else 0.0])
    desc = PwmLibrary(1, 4, width.ctypes.data, matrix.ctypes.data, None if thr is None else thr.ctypes.data)
    out = [ops.device.zeros(len(rows), t) for t in (np.float64, np.int64, np.uint8, np.int64)]
    status = lib.bnpk_pwm_rows_packed(ops.ctx, C.byref(desc), ptr(data.dev()), total, ptr(offsets.dev()), len(rows), 1,
                                      ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), ops._s())
    assert status == (0 if case == "ok" else -1)
    assert lib.bnpk_pwm_rows_packed(ops.ctx, C.byref(desc), None, 0, None, 0, 0, None, None, None, None, ops._s()) == \
        (0 if case in ("ok", "hits_without_thresholds") else -1)                   # no rows: nothing launched
