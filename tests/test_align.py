"""-m gpu: bnp.align_pairs / bnpk_align_* (csrc/align.hip) against the definition of include/bnpk.h written out as loops over
exact integers: H, E, F, the end rule and the walk.  Every comparison is exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG = -10 ** 9
MODES = ["local", "semiglobal", "global"]
SIZES = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 150, 159, 160, 161]      # 160 = 16 lanes x 10 rows: the small class
MATRIX21 = np.random.default_rng(21).integers(-9, 12, (21, 21))                 # asymmetric
SCORINGS = {"2-3-5-2": (2, -3, 5, 2), "1-1-0-1": (1, -1, 0, 1), "0-1-0-1": (0, -1, 0, 1), "matrix21": (MATRIX21, None, 11, 1)}


def ref_align(q, t, S, go, ge, mode):
    """(score, query_start, target_start, query_end, target_end, [(op, length)]) by the definition; ops 0 = M, 1 = I, 2 = D"""
    n, m = len(q), len(t)
    H, E, F = ([[v] * (m + 1) for _ in range(n + 1)] for v in (0, NEG, NEG))
    for i in range(n + 1):
        for j in range(m + 1):
            if j:
                E[i][j] = max(H[i][j - 1] - go - ge, E[i][j - 1] - ge)
            if i:
                F[i][j] = max(H[i - 1][j] - go - ge, F[i - 1][j] - ge)
            if (i or j) and not (mode == "local" and (i == 0 or j == 0)) and not (mode == "semiglobal" and i == 0):
                h = max(E[i][j], F[i][j], H[i - 1][j - 1] + S[q[i - 1]][t[j - 1]] if i and j else NEG)
                H[i][j] = max(h, 0) if mode == "local" else h
    if mode == "global":
        i, j = n, m
    elif mode == "semiglobal":
        i, j = n, max(range(m + 1), key=lambda c: (H[n][c], -c))
    else:
        i, j = max(((a, b) for a in range(n + 1) for b in range(m + 1)), key=lambda c: (H[c[0]][c[1]], -c[0], -c[1]))
        if H[i][j] == 0:
            i = j = 0
    score, end, state, walk = H[i][j], (i, j), "H", []
    while True:
        if state == "H":
            if (mode == "local" and H[i][j] == 0) or (mode == "semiglobal" and i == 0) or (i == 0 and j == 0):
                break
            if i and j and H[i][j] == H[i - 1][j - 1] + S[q[i - 1]][t[j - 1]]:
                walk.append(0)
                i, j = i - 1, j - 1
            else:
                state = "E" if H[i][j] == E[i][j] else "F"
        elif state == "E":
            walk.append(2)
            state = "H" if E[i][j] == H[i][j - 1] - go - ge else "E"
            j -= 1
        else:
            walk.append(1)
            state = "H" if F[i][j] == H[i - 1][j] - go - ge else "F"
            i -= 1
    cigar = []
    for op in reversed(walk):
        cigar = cigar[:-1] + [(op, cigar[-1][1] + 1)] if cigar and cigar[-1][0] == op else cigar + [(op, 1)]
    return score, i, j, end[0], end[1], cigar


def make_pairs(A, big):
    rng = np.random.default_rng(A)
    rand = lambda n: rng.integers(0, A, n)

    def mutated(q):                                            # a few substitutions, one inserted run, one deleted run
        t = q.copy()
        t[rng.integers(0, max(t.size, 1), min(3, t.size))] = rand(min(3, t.size))
        a, b = sorted(rng.integers(0, t.size + 1, 2))
        return np.concatenate([t[:a], rand(3), t[a:b], t[b + 4:]])[:512]

    pairs = [(q, mutated(q)) for q in map(rand, SIZES)] + [(rand(n), rand(m)) for n, m in zip(SIZES, SIZES[::-1])]
    pairs += [(rand(161), rand(17)), (rand(16), rand(161)), (rand(40) % 2, rand(170) % 2)]
    rep = np.tile(np.arange(3) % A, 14)
    pairs += [(rand(1) * np.ones(20, int), rand(1) * np.ones(33, int)), (rep, rep[1:]), (rep[2:], rep), (rep, rep)]   # ties
    if big:
        q = rand(512)
        pairs += [(q, mutated(q)[:511]), (rand(511), rand(512)), (rand(150), mutated(rand(512)))]
    return [(q.astype(np.uint8), t.astype(np.uint8)) for q, t in pairs]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


def rows(bnp, seqs, packed):
    letters = "ACGT" if packed else "ACDEFGHIKLMNPQRSTVWY*"
    return bnp.as_encoded_array(["".join(letters[c] for c in s) for s in seqs], bnp.DNAEncoding if packed else bnp.AminoAcidEncoding)


def run(bnp, pairs, packed, scoring, mode, traceback=True):
    """the public call on code rows -> (score, query_start, target_start, query_end, target_end, cigar) per pair"""
    first, second, go, ge = scoring
    kw = dict(matrix=first) if second is None else dict(match=first, mismatch=second)
    al = bnp.align_pairs(rows(bnp, [p[0] for p in pairs], packed), rows(bnp, [p[1] for p in pairs], packed), gap_open=go,
                         gap_extend=ge, mode=mode, traceback=traceback, **kw)
    cols = [np.asarray(x).tolist() for x in (al.score, al.query_end, al.target_end)]
    if not traceback:
        assert al.cigar_op is None and al.query_start is None
        return list(zip(*cols))
    op, length, off = al.cigar_op.raw().ravel(), al.cigar_length.ravel(), al.cigar_op.offsets().host()
    assert np.array_equal(off, al.cigar_length.offsets().host()) and off[0] == 0 and off[-1] == op.size == length.size
    cigars = [list(zip(op[a:b].tolist(), np.asarray(length[a:b]).tolist())) for a, b in zip(off, off[1:])]
    return list(zip(cols[0], np.asarray(al.query_start).tolist(), np.asarray(al.target_start).tolist(), cols[1], cols[2], cigars))


def matrix_of(scoring, A):
    return scoring[0] if scoring[1] is None else np.where(np.eye(A, dtype=bool), scoring[0], scoring[1])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("packed,name", [(p, s) for p in (True, False) for s in SCORINGS if not (p and s == "matrix21")])
def test_against_definition(bnp, packed, name, mode):
    A, scoring = 4 if packed else 21, SCORINGS[name]
    pairs = make_pairs(A, big=True)
    want = [ref_align(q.tolist(), t.tolist(), matrix_of(scoring, A).tolist(), scoring[2], scoring[3], mode) for q, t in pairs]
    got = run(bnp, pairs, packed, scoring, mode)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, pairs[k][0].size, pairs[k][1].size)
    assert name == "0-1-0-1" or {op for w in want for op, _ in w[5]} == {0, 1, 2}     # (a match of 0 aligns nothing locally)


@pytest.mark.parametrize("mode", MODES)
def test_score_beyond_16_bits(bnp, mode):
    row = np.arange(512) % 21
    m = np.full((21, 21), -128)
    np.fill_diagonal(m, 127)
    assert run(bnp, [(row, row)], False, (m, None, 127, 127), mode) == [(65024, 0, 0, 512, 512, [(0, 512)])]


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "bytes"])
def test_one_target_batches_and_score_only(bnp, packed):
    pairs = make_pairs(4 if packed else 21, big=False)[:40]
    scoring, ops = SCORINGS["1-1-0-1"], bnp.ops.get_ops()
    for mode in MODES:
        whole = run(bnp, pairs, packed, scoring, mode)
        assert [w[:1] + w[3:5] for w in whole] == run(bnp, pairs, packed, scoring, mode, traceback=False)
        ops.align_batch_pairs = 7                            # six batches of path slots
        try:
            assert run(bnp, pairs, packed, scoring, mode) == whole
        finally:
            del ops.align_batch_pairs
        target = pairs[12][1]
        al = bnp.align_pairs(rows(bnp, [p[0] for p in pairs], packed), rows(bnp, [target], packed), 1, -1, None, 0, 1, mode)
        same = run(bnp, [(p[0], target) for p in pairs], packed, scoring, mode)
        assert np.asarray(al.score).tolist() == [s[0] for s in same] and np.asarray(al.target_start).tolist() == [s[2] for s in same]
        assert al.cigar_op.tolist() == ["".join("MID"[op] for op, _ in s[5]) for s in same]


def test_edit_distance_cross_checks(bnp):
    def levenshtein(a, b):
        d = list(range(len(b) + 1))
        for i, x in enumerate(a, 1):
            d, prev = [i] + [0] * len(b), d
            for j, y in enumerate(b, 1):
                d[j] = min(prev[j] + 1, d[j - 1] + 1, prev[j - 1] + (x != y))
        return d[-1]
    pairs, unit = make_pairs(4, big=False), SCORINGS["0-1-0-1"]
    assert [-g[0] for g in run(bnp, pairs, True, unit, "global")] == [levenshtein(q.tolist(), t.tolist()) for q, t in pairs]
    pattern = pairs[5][0]                                      # 17 letters against every target
    reads = rows(bnp, [p[1] for p in pairs], True)
    scan = bnp.find_approximate(reads, "".join("ACGT"[c] for c in pattern), max_errors=16)
    got = run(bnp, [(pattern, p[1]) for p in pairs], True, unit, "semiglobal", traceback=False)
    assert [-g[0] for g in got] == np.asarray(scan.distance[0]).tolist()


def test_errors_and_public_interface(bnp):
    from bionumpy_amd.sequence.alignment import count_reference_length
    long_row, ok = "A" * 513, ["ACGT", "ACGT"]
    for q, t in (([ok[0], long_row], ok), (ok, [ok[0], long_row])):
        with pytest.raises(NotImplementedError, match="pair 1 "):
            bnp.align_pairs(q, t)
    amino = bnp.as_encoded_array(["ACDE"], bnp.AminoAcidEncoding)
    for n in (2, 0):                                           # the arguments are checked without rows too
        q = bnp.as_encoded_array(ok[:n], bnp.DNAEncoding)
        for bad in (dict(mode="banded"), dict(gap_open=128), dict(gap_extend=-1), dict(matrix=np.full((4, 4), 128)),
                    dict(matrix=np.zeros((5, 5), int)), dict(targets=amino), dict(targets=bnp.as_encoded_array(ok + ok + ok, bnp.DNAEncoding))):
            with pytest.raises(ValueError):
                bnp.align_pairs(q, **{"targets": q, **bad})
    params = bnp._native.AlignParams(4, 3, 5, 2, 0, 0, np.zeros(16, np.int32).ctypes.data)
    import ctypes as C
    assert bnp._native.lib.bnpk_align_pairs_packed(bnp.ops.get_ops().ctx, C.byref(params), *([0] * 19)) == -1          # BNPK_ERR_ARG
    reads = bnp.as_encoded_array(["TTACGTACGTTT", "ACGTAACGT", "GGGG", ""], bnp.DNAEncoding)
    al = bnp.align_pairs(reads, ["ACGTACGT"], gap_open=2, gap_extend=1)
    assert np.asarray(al.score).tolist() == [16, 13, 2, 0] and al.cigar_op.tolist() == ["M", "MIM", "M", ""]
    assert al.cigar_length.tolist() == [[8], [4, 1, 4], [1], []] and np.asarray(al.query_start).tolist() == [2, 0, 0, 0]
    assert count_reference_length(al.cigar_op, al.cigar_length).tolist() == (np.asarray(al.target_end) - np.asarray(al.target_start)).tolist()
    assert reads[np.asarray(al.score >= 13)].tolist() == ["TTACGTACGTTT", "ACGTAACGT"]
