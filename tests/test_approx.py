"""-m gpu: bnpk_approx_rows_packed / _bytes, bnp.find_approximate and bnp.trim_adapters (csrc/approx.hip) against the plain
column-by-column dynamic programme (Sellers), restated here.  Every comparison is exact (np.array_equal)."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIECE = 256                                                    # the piece length the tests force (the smallest there is)
LONG = 4 * PIECE + 100
EDGE_M = [1, 2, 31, 32, 33, 63, 64]                            # both word widths and their edges
AMINO = "ACDEFGHIKLMNPQRSTVWY"
KINDS = [0, 1, 3, "m-1"]


def dp(acc, codes, anchored=False):
    """D[i][j] = min over s of ed(P[0:i], c[s:j]) (anchored: s = 0) for all i, j; acc[i][a]: position i accepts code a"""
    m, ar = acc.shape[0], np.arange(acc.shape[0] + 1)
    D = np.empty((m + 1, codes.size + 1), dtype=np.int64)
    D[:, 0] = ar
    for j, c in enumerate(codes, 1):
        old = D[:, j - 1]
        x = np.concatenate([[j if anchored else 0], np.minimum(old[1:] + 1, old[:-1] + 1 - acc[:, c])])
        D[:, j] = np.minimum.accumulate(x - ar) + ar           # (the vertical step: D[i] <= D[i - 1] + 1)
    return D


def outputs(acc, codes, D, k, o):
    """(dist, start, end, overlap, hits) of include/bnpk.h from D"""
    m, L = acc.shape[0], codes.size
    dist, end, hits = int(D[m].min()), int(D[m].argmin()), int((D[m, 1:] <= k).sum())
    over = m if dist <= k else 0
    if not over and o > 0:
        ok = [i for i in range(o, m) if D[i, L] <= k * i // m]
        if ok:
            over, dist, end = ok[-1], int(D[ok[-1], L]), L
    if not over:
        return dist, -1, -1, 0, hits
    lo = max(0, end - over - dist)                             # the shortest match ending at end: anchored, both reversed
    back = dp(acc[:over][::-1], codes[lo:end][::-1], True)[-1]
    return dist, end - int(np.flatnonzero(back == dist)[0]), end, over, hits


def masks_of(acc):
    return (acc.astype(np.uint64) << np.arange(acc.shape[0], dtype=np.uint64)[:, None]).sum(axis=0, dtype=np.uint64)


class World:
    """the patterns of one alphabet, rows with their occurrences planted, everything in HBM, and the references by k"""

    def __init__(self, bnp, n_codes, n_letters, lengths, seed):
        from bionumpy_amd.device import HArray
        rng = np.random.default_rng(seed)
        self.pats = [rng.integers(0, n_letters, m) for m in lengths] + [rng.integers(0, n_letters, 13)]
        self.acc = [np.eye(n_codes, dtype=np.int64)[p] for p in self.pats]
        self.acc[-1][[2, 3, 9]] = 1                            # the last pattern has three positions that accept everything
        self.o = [min(3, a.shape[0] - 1) for a in self.acc]
        big = [p for p in self.pats if p.size >= 13]
        rnd = lambda n: rng.integers(0, n_letters, n)
        lens = sorted({n for m in lengths for n in (m - 1, m, m + 1)} | {0, 1, 31, 32, 33, 34, 63, 64, 65, 150, PIECE - 1, PIECE, PIECE + 1})
        rows = [rnd(n) for n in lens]
        if n_codes > n_letters:                                # ACGTn: a code that no position but a wildcard accepts
            for r in rows[5:]:
                r[::7] = n_codes - 1
        self.long = []
        for i in range(10):                                    # one error each: a substitution, an insertion, a deletion
            p, h = big[i % len(big)], big[i % len(big)].size // 2
            plant = [np.concatenate([p[:h], [(p[h] + 1) % n_letters], p[h + 1:]]), np.insert(p, h, (p[h] + 1) % n_letters), np.delete(p, h)][i % 3]
            at = [50, 2 * PIECE + 40, 4 * PIECE + 20, 2 * PIECE - plant.size // 2, 3 * PIECE - plant.size][i % 5]
            row = rnd(LONG)
            row[at:at + plant.size] = plant                    # first, a middle, the last piece; across a boundary; ending at one
            if i == 5:
                rows += [rnd(3) for _ in range(300)]           # a run of short rows between the long ones
            self.long.append(len(rows))
            rows.append(row)
        self.overhang = {}
        for pi, p in enumerate(self.pats):                     # the first i letters at the very end of a row
            for i in ({self.o[pi] - 1, self.o[pi], p.size - 1} - {0} if self.o[pi] else ()):
                self.overhang[pi, i] = len(rows)
                rows.append(np.concatenate([rnd(40), p[:i]]))
        self.rows = [r.astype(np.uint8) for r in rows]
        ops = bnp.ops.get_ops()
        flat = HArray(host=np.concatenate(self.rows))
        self.total, self.packed = flat.size, n_codes == 4
        self.data = ops.pack_codes(flat) if self.packed else flat
        self.offsets = HArray(host=np.concatenate([[0], np.cumsum([r.size for r in self.rows])]).astype(np.int64))
        self.masks = np.stack([masks_of(a) for a in self.acc])
        self.D = [[dp(a, r) for r in self.rows] for a in self.acc]
        self._by_k = {}

    def ks(self, kind):
        return [a.shape[0] - 1 if kind == "m-1" else min(kind, a.shape[0] - 1) for a in self.acc]

    def expect(self, kind):
        if kind not in self._by_k:
            out = [[outputs(a, r, self.D[pi][ri], k, o) for ri, r in enumerate(self.rows)]
                   for pi, (a, k, o) in enumerate(zip(self.acc, self.ks(kind), self.o))]
            self._by_k[kind] = np.array(out, dtype=np.int64).transpose(2, 0, 1)      # field x pattern x row
        return self._by_k[kind]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    yield bionumpy_amd
    bionumpy_amd._native.lib.bnpk_set_option(ops.get_ops().ctx, b"approx_piece", 0)


@pytest.fixture(scope="module")
def worlds(bnp):
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(bnp, *{"ACGT": (4, 4, EDGE_M, 1), "ACGTn": (5, 4, [5, 13, 33], 2), AMINO: (20, 20, [5, 13, 33], 3)}[name])
        return made[name]
    return get


@pytest.mark.parametrize("piece", [PIECE, 0])                  # forced to the smallest / chosen by the library
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["ACGT", "ACGTn", AMINO])
def test_rows(bnp, worlds, name, kind, piece):
    w = worlds(name)
    want = w.expect(kind)
    dist, start, end, over, hits = want
    if kind != 0:                                              # the fixture holds every kind of row
        whole, hang = over == np.array([a.shape[0] for a in w.acc])[:, None], (over > 0) & (end >= 0)
        assert whole.any() and (over == 0).any() and (end[:, w.long] > PIECE).any()
        # (with k = m - 1 every row of a symbol or more holds the pattern whole: nothing is left to overhang)
        assert kind == "m-1" or (hang & ~whole).any()
    if kind == 0 and name == "ACGT":                           # the planted prefixes: one too short, the shortest, the longest
        for (pi, i), r in w.overhang.items():
            if w.pats[pi].size >= 31:
                assert over[pi, r] == (i if i >= w.o[pi] else 0), (pi, i)
    ops = bnp.ops.get_ops()
    assert bnp._native.lib.bnpk_set_option(ops.ctx, b"approx_piece", piece) == 0
    got = ops.approx_rows(w.data, w.offsets, len(w.rows), w.total, w.masks, w.ks(kind), w.o, [a.shape[0] for a in w.acc], w.packed, True)
    for g, e, what in zip(got, want, ("dist", "start", "end", "overlap", "hits")):
        assert np.array_equal(g.host().reshape(e.shape).astype(np.int64), e), what


def test_public_interface(bnp, worlds):
    for name in ("ACGT", AMINO):
        w = worlds(name)
        rows = list(range(12)) + w.long[:2] + sorted(w.overhang.values())[:6]
        text = ["".join(name[c] for c in w.rows[r]) for r in rows]
        pats = ["".join("." if a.all() else name[c] for c, a in zip(p, acc)) for p, acc in zip(w.pats, w.acc)]
        seqs = text if name == "ACGT" else bnp.as_encoded_array(text, bnp.AlphabetEncoding(name))
        scan = bnp.find_approximate(seqs, pats, w.ks(3), w.o, count_hits=True)
        for got, want in zip((scan.distance, scan.start, scan.end, scan.overlap, scan.n_hits), w.expect(3)):
            assert np.array_equal(np.asarray(got), want[:, rows])
        keep = scan.distance[2] <= 1                           # a per-pattern row is a device vector: a read filter
        assert np.array_equal(np.asarray(keep), w.expect(3)[0][2, rows] <= 1)
        assert len(bnp.as_encoded_array(text)[np.asarray(keep)]) == int(np.asarray(keep).sum())
    # ties: the smallest end, the shortest match, several hits
    row, acc = np.array([0, 1] * 10), np.eye(4, dtype=np.int64)[[0, 1, 0, 1]]
    scan = bnp.find_approximate(["AC" * 10], "ACAC", 1, count_hits=True)
    want = outputs(acc, row, dp(acc, row), 1, 0)
    assert [int(np.asarray(x)[0, 0]) for x in (scan.distance, scan.start, scan.end, scan.overlap, scan.n_hits)] == list(want)
    assert want[:3] == (0, 0, 4) and want[4] > 1 and bnp.find_approximate(["ACGT"], "AC", 0).n_hits is None
    for bad in (dict(patterns="ACXT", max_errors=1), dict(patterns="ACGT", max_errors=4), dict(patterns="ACGT", max_errors=1, min_overlap=4)):
        with pytest.raises(ValueError):
            bnp.find_approximate(["ACGT"], **bad)
    with pytest.raises(NotImplementedError):
        bnp.find_approximate(["ACGT"], "A" * 65, 1)


def test_trim_adapters(bnp, tmp_path):
    lines = open(os.path.join(os.path.dirname(__file__), "golden", "reads.fq")).read().split("\n")
    adapter, tails = "AGATCGGAAGAGCACACGTC", ["", "AGATCGGAAGAGCACACGTCTGAA", "AGATCGTAAGAGCACACGTC", "AGATCGGAAGAG", "AGAT", "AG"]
    names = [lines[4 * (i % 2)][1:] + str(i) for i in range(12)]
    seqs = [lines[4 * (i % 2) + 1] * 3 + tails[i % 6] for i in range(12)]
    quals = [(lines[4 * (i % 2) + 3] * 15)[:len(s)] for i, s in enumerate(seqs)]
    path = str(tmp_path / "in.fq")
    open(path, "w").write("".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, seqs, quals)))
    chunk = bnp.open(path).read()
    assert isinstance(chunk, bnp.SequenceEntryWithQuality)
    acc = np.eye(4, dtype=np.int64)[["ACGT".index(c) for c in adapter]]
    codes = [np.array(["ACGT".index(c) for c in s]) for s in seqs]
    cut = [outputs(acc, c, dp(acc, c), 2, 3)[1] for c in codes]
    assert sum(c >= 0 for c in cut) >= 8 and sum(c < 0 for c in cut) >= 2      # (whole, overhanging, and left alone)
    want_s = [s[:c] if c >= 0 else s for s, c in zip(seqs, cut)]
    want_q = [q[:c] if c >= 0 else q for q, c in zip(quals, cut)]
    trimmed = bnp.trim_adapters(chunk, adapter, 2, min_overlap=3)
    assert trimmed.sequence.tolist() == want_s and trimmed.name.tolist() == names
    assert [bytes(np.asarray(q) + 33).decode() for q in trimmed.quality] == want_q
    assert bnp.trim_adapters(bnp.as_encoded_array(seqs, bnp.DNAEncoding), adapter, 2).tolist() == want_s
    out = str(tmp_path / "out.fq")
    with bnp.open(out, "w") as f:
        f.write(trimmed)
    assert open(out).read() == "".join("@%s\n%s\n+\n%s\n" % t for t in zip(names, want_s, want_q))
    back = bnp.open(out).read()
    assert back.sequence.tolist() == want_s


@pytest.mark.parametrize("case", ["m_0", "m_65", "k_is_m", "overlap_is_m", "mask_above_m", "no_patterns", "too_many", "ok"])
def test_bad_arguments(bnp, worlds, case):
    from bionumpy_amd._native import lib, ApproxLibrary, APPROX_MAX_PATTERNS
    from bionumpy_amd.device import ptr
    w, ops = worlds("ACGT"), bnp.ops.get_ops()
    n = {"no_patterns": 0, "too_many": APPROX_MAX_PATTERNS + 1}.get(case, 1)
    m = np.full(max(n, 1), {"m_0": 0, "m_65": 65}.get(case, 4), dtype=np.int32)
    k = np.full(m.size, 4 if case == "k_is_m" else 1, dtype=np.int32)
    o = np.full(m.size, 4 if case == "overlap_is_m" else 0, dtype=np.int32)
    eq = np.full((m.size, 4), 0x1f if case == "mask_above_m" else 0x5, dtype=np.uint64)
    desc = ApproxLibrary(n, 4, m.ctypes.data, k.ctypes.data, o.ctypes.data, eq.ctypes.data)
    out = [ops.device.zeros(len(w.rows), t) for t in (np.uint8, np.int64, np.int64, np.uint8)]
    for rows in (len(w.rows), 0):                              # (no rows: nothing launched, the library is still checked)
        status = lib.bnpk_approx_rows_packed(ops.ctx, C.byref(desc), ptr(w.data.dev()), w.total, ptr(w.offsets.dev()), rows,
                                             ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3]), None, ops._s())
        assert status == (0 if case == "ok" else -1)
    assert lib.bnpk_set_option(ops.ctx, b"approx_piece", 300) == -1 and lib.bnpk_set_option(ops.ctx, b"approx_piece", 128) == -1
