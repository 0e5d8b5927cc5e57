"""-m gpu: bnpk_mates_overlap_* / bnpk_mates_merge_* and bnp.find_mate_overlaps / bnp.merge_pairs (csrc/mates.hip) against the
definition of include/bnpk.h written out: every offset of every pair, column by column.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX = 512
SIZES = [0, 1, 31, 32, 33, 63, 64, 65, 150, MAX - 1, MAX]
PARAMS = [(30, 5, 20, True), (4, 0, 0, True), (10, 2, 100, False), (1, MAX, 100, True), (30, 5, 10, True)]
# (the last: 5 mismatches in 40 columns pass the absolute limit and miss the percent limit; in 50 columns they meet both)


def revcomp(m, q=None):
    b = np.where(m[::-1] < 4, 3 - m[::-1], m[::-1])
    return b if q is None else (b, q[::-1])


def ref_overlap(a, m2, min_overlap, max_mm, percent, read_through):
    """(length, overlap, mismatches, offsets that tie on the overlap, of those on the mismatches too) by the definition"""
    b, n1, n2, found = revcomp(m2), a.size, m2.size, []
    for s in range(1 - n2, n1):
        lo, hi = max(0, s), min(n1, s + n2)
        if hi - lo < min_overlap or (not read_through and (s < 0 or s + n2 < n1)):
            continue
        x, y = a[lo:hi], b[lo - s:hi - s]
        mm = int(((x != y) | (x >= 4) | (y >= 4)).sum())
        if mm <= max_mm and 100 * mm <= percent * (hi - lo):
            found.append((lo - hi, mm, s))
    if not found:
        return -1, 0, 0, 0, 0
    ov, mm, s = min(found)
    return s + n2, -ov, mm, sum(f[0] == ov for f in found), sum(f[:2] == (ov, mm) for f in found)


def ref_merge(a, qa, m2, q2, f, cap):
    b, qb = revcomp(m2, q2)
    s, codes, qual = f - b.size, [], []
    for t in range(f):
        if t < a.size and t >= s:
            ca, cb, x, y = a[t], b[t - s], int(qa[t]), int(qb[t - s])
            if ca >= 4 or cb >= 4:
                c, q = (cb, y) if ca >= 4 and cb < 4 else (ca, x)
            elif ca == cb:
                c, q = ca, min(x + y, cap)
            else:
                c, q = (cb, y - x) if y > x else (ca, x - y)
        else:
            c, q = (a[t], qa[t]) if t < a.size else (b[t - s], qb[t - s])
        codes.append(c)
        qual.append(q)
    return codes, qual


class World:
    """about 330 pairs in HBM: pairs cut from a fragment so that the answer under PARAMS[0] is known, and unrelated mates of
    every pair of SIZES; qualities from {0, 2, 20, 40, 41}"""

    def __init__(self, bnp, packed):
        from bionumpy_amd.device import HArray
        rng = np.random.default_rng(77 + packed)
        rnd = lambda n: rng.integers(0, 4, n)

        def cut(F, n1, n2, subs=0, n_a=(), n_b=(), sub_a=()):
            """the mates of fragment F: a = its first n1 letters, b its last n2, each with an adapter tail where F is shorter;
            `subs` overlap columns of b changed, an N at the columns n_a of a and n_b of b, a's column sub_a changed"""
            f, s = F.size, F.size - n2
            a, b = np.concatenate([F[:n1], rnd(max(0, n1 - f))]), np.concatenate([rnd(max(0, -s)), F[max(0, s):]])
            cols = rng.permutation(np.arange(max(0, s), min(n1, f)))[:subs]
            b[cols - s] = (b[cols - s] + rng.integers(1, 4, cols.size)) % 4
            a[list(sub_a)] = (a[list(sub_a)] + 1) % 4
            a[list(n_a)] = 4
            b[[t - s for t in n_b]] = 4
            return a, revcomp(b)

        unit = rnd(10)
        repeat = np.tile(unit, 15)                             # a = repeat, b = repeat[50:]: every s = 0, 10, .. 50 has ov 100
        made = [(cut(rnd(320), 150, 150), -1), (cut(rnd(270), 150, 150), 270), (cut(rnd(271), 150, 150), -1),
                (cut(rnd(150), 150, 150), 150), (cut(rnd(100), 150, 150), 100), (cut(rnd(100), 150, 65), 100),
                (cut(rnd(200), 150, 150, subs=5), 200), (cut(rnd(200), 150, 150, subs=6), -1),
                (cut(rnd(260), 150, 150, subs=5), 260), (cut(rnd(250), 150, 150, subs=5), 250),
                (cut(repeat, 150, 100, sub_a=(5,)), 110)]      # s = 0 has a mismatch the others do not: s = 10
        self.tie = len(made) - 1
        if not packed:
            made += [(cut(rnd(200), 150, 150, n_a=(60,)), 200), (cut(rnd(200), 150, 150, n_b=(70,)), 200),
                     (cut(rnd(200), 150, 150, n_a=(80,), n_b=(80,)), 200)]
        self.known = {i: f for i, (_, f) in enumerate(made)}
        pairs = [p for p, _ in made]
        self.unrelated = range(len(pairs), len(pairs) + len(SIZES) * (len(SIZES) - 1))
        pairs += [(rnd(n1), rnd(n2)) for n1 in SIZES for n2 in SIZES if n1 != n2]
        sizes = [n for n in SIZES if n]
        while len(pairs) < 330:                                # related mates of every size, at every 2-bit phase
            n1, n2 = rng.choice(sizes, 2)
            pairs.append(cut(rnd(rng.integers(max(n1, n2) // 2 + 1, n1 + n2)), n1, n2, subs=rng.integers(0, 4)))
        if not packed:
            for a, m2 in pairs[-40:]:
                a[rng.integers(0, a.size, 2)] = 4
                m2[rng.integers(0, m2.size)] = 4
        self.pairs = [(a.astype(np.uint8), m.astype(np.uint8)) for a, m in pairs]
        self.quals = [tuple(rng.choice([0, 2, 20, 40, 41], x.size).astype(np.uint8) for x in p) for p in self.pairs]
        self.packed, ops = packed, bnp.ops.get_ops()
        self.side = []
        for k in (0, 1):
            flat = HArray(host=np.concatenate([p[k] for p in self.pairs]))
            offsets = HArray(host=np.concatenate([[0], np.cumsum([p[k].size for p in self.pairs])]).astype(np.int64))
            qual = HArray(host=np.concatenate([q[k] for q in self.quals]))
            self.side.append((ops.pack_codes(flat) if packed else flat, offsets, flat.size, qual))
        self._expect = {}

    def expect(self, params):
        if params not in self._expect:
            self._expect[params] = np.array([ref_overlap(a, m, *params) for a, m in self.pairs], dtype=np.int64)
        return self._expect[params]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


@pytest.fixture(scope="module")
def worlds(bnp):
    made = {}

    def world(packed):
        if packed not in made:
            w = made[packed] = World(bnp, packed)              # the fixture holds every kind of pair (on the reference alone)
            e, n1 = w.expect(PARAMS[0]), np.array([a.size for a, _ in w.pairs])
            assert all(e[i, 0] == f for i, f in w.known.items())
            assert (e[:, 0] < 0).any() and ((e[:, 0] >= 0) & (e[:, 0] < n1)).any() and ((e[:, 0] >= n1) & (e[:, 1] > 0)).any()
            assert tuple(e[w.tie]) == (110, 100, 0, 6, 5)      # all three levels of the rule decide here
            assert tuple(w.expect(PARAMS[4])[[8, 9], 0]) == (-1, 250)
            assert (w.expect(PARAMS[1])[list(w.unrelated), 0] >= 0).mean() <= 0.25
        return made[packed]
    return world


@pytest.mark.parametrize("params", PARAMS, ids=lambda p: "-".join(str(int(x)) for x in p))
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "bytes"])
def test_overlap(bnp, worlds, packed, params):
    w = worlds(packed)
    (d1, o1, t1, _), (d2, o2, t2, _) = w.side
    got = bnp.ops.get_ops().mates_overlap(d1, o1, t1, d2, o2, t2, len(w.pairs), *params, packed)
    for g, e, what in zip(got, w.expect(params).T, ("length", "overlap", "mismatches")):
        assert np.array_equal(g.host().astype(np.int64), e), what


@pytest.mark.parametrize("params,cap,with_qual", [(PARAMS[0], 41, True), (PARAMS[3], 93, True), (PARAMS[3], 41, False)],
                         ids=["cap41", "cap93", "no_qualities"])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "bytes"])
def test_merge(bnp, worlds, packed, params, cap, with_qual):
    from bionumpy_amd.device import HArray
    w = worlds(packed)
    (d1, o1, _, q1), (d2, o2, _, q2) = w.side
    length = w.expect(params)[:, 0]
    codes, qual, offsets, total = bnp.ops.get_ops().mates_merge(d1, o1, q1 if with_qual else None, d2, o2, q2 if with_qual else None,
                                                                len(w.pairs), HArray(host=length), cap, packed)
    want_c, want_q = [], []
    for (a, m2), (qa, qb), f in zip(w.pairs, w.quals, length):
        c, q = ref_merge(a, qa if with_qual else 0 * qa, m2, qb if with_qual else 0 * qb, max(f, 0), cap)
        want_c += c
        want_q += q
    assert total == len(want_c) and np.array_equal(offsets.host(), np.concatenate([[0], np.cumsum(np.maximum(length, 0))]))
    assert np.array_equal(codes.host(), np.array(want_c, dtype=np.uint8))
    assert (qual is None) if not with_qual else np.array_equal(qual.host(), np.array(want_q, dtype=np.uint8))
    assert not with_qual or cap != 41 or (np.array(want_q) == 41).any()      # the sum saturates somewhere


def test_public_interface(bnp, worlds, tmp_path):
    w = worlds(False)
    text = [["".join("ACGTN"[c] for c in p[k]) for p in w.pairs] for k in (0, 1)]
    want = w.expect(PARAMS[0])
    for m1, m2 in (text, (bnp.as_encoded_array(text[0], bnp.ACGTnEncoding), bnp.as_encoded_array(text[1], bnp.ACGTnEncoding))):
        ov = bnp.find_mate_overlaps(m1, m2)
        for got, e in zip((ov.length, ov.overlap, ov.mismatches), want.T):
            assert np.array_equal(np.asarray(got).astype(np.int64), e)
    # two FASTQ chunks: pair 0 merges (ACGTACGTAC + its tail), pair 1 does not; ACGT on one side and an N on the other
    f1, f2 = tmp_path / "r1.fq", tmp_path / "r2.fq"
    f1.write_text("@p0\nAAACCCGGGT\n+\nIIIIIIIII5\n@p1\nAAAAAAAAAA\n+\nIIIIIIIIII\n")
    f2.write_text("@p0\nGGNACCCGGG\n+\n5I#IIIIIII\n@p1\nCCCCCCCCCC\n+\nIIIIIIIIII\n")
    chunk1, chunk2 = bnp.open(str(f1)).read(), bnp.open(str(f2)).read()
    m = bnp.merge_pairs(chunk1, chunk2, min_overlap=4, max_mismatches=1)
    assert np.asarray(m.is_merged).tolist() == [True, False] and np.asarray(m.overlaps.length).tolist() == [13, -1]
    assert m.merged.sequence.tolist() == ["AAACCCGGGTNCC"] and m.merged.name.tolist() == ["p0"]
    assert np.asarray(m.merged.quality[0]).tolist() == [40] * 3 + [41] * 7 + [2, 40, 20]
    assert chunk1[~np.asarray(m.is_merged)].name.tolist() == ["p1"]
    out = tmp_path / "merged.fq"
    with bnp.open(str(out), "w") as f:
        f.write(m.merged)
    assert out.read_text() == "@p0\nAAACCCGGGTNCC\n+\nIIIJJJJJJJ#I5\n"
    assert bnp.merge_pairs(chunk1.sequence, chunk2.sequence, min_overlap=4, max_mismatches=1).merged.tolist() == ["AAACCCGGGTNCC"]
    for bad in (dict(min_overlap=0), dict(max_mismatches=-1), dict(max_mismatch_percent=101), dict(max_mismatch_percent=-1),
                dict(quality_cap=94), dict(quality_cap=-1)):
        with pytest.raises(ValueError):
            bnp.merge_pairs(["ACGT"], ["ACGT"], **bad)
    with pytest.raises(ValueError):
        bnp.find_mate_overlaps(["ACGT", "ACGT"], ["ACGT"])
    with pytest.raises(NotImplementedError):
        bnp.find_mate_overlaps(bnp.as_encoded_array(["ACDE"], bnp.AminoAcidEncoding), ["ACGT"])
    with pytest.raises(NotImplementedError):
        bnp.find_mate_overlaps(["ACGT", "A" * (MAX + 1)], ["ACGT", "ACGT"])


@pytest.mark.parametrize("case", ["overlap_0", "mismatches_negative", "percent_negative", "percent_101", "read_through_2", "cap_94",
                                  "cap_negative", "one_quality", "ok"])
def test_bad_arguments(bnp, worlds, case):
    from bionumpy_amd._native import lib, MatesParams
    from bionumpy_amd.device import ptr
    w, ops = worlds(True), bnp.ops.get_ops()
    (d1, o1, t1, q1), (d2, o2, t2, q2) = w.side
    h = MatesParams(0 if case == "overlap_0" else 30, -1 if case == "mismatches_negative" else 5,
                    {"percent_negative": -1, "percent_101": 101}.get(case, 20), 2 if case == "read_through_2" else 1,
                    {"cap_94": 94, "cap_negative": -1}.get(case, 41))
    n = len(w.pairs)
    length, overlap, mismatches = (ops.device.zeros(n, t) for t in (np.int64, np.int32, np.int32))
    out_off, cell = ops.device.zeros(n + 1, np.int64), ops._err_cell()
    for rows in (n, 0):                                        # (no rows: nothing launched, the parameters are still checked)
        status = lib.bnpk_mates_overlap_packed(ops.ctx, C.byref(h), ptr(d1.dev()), t1, ptr(o1.dev()), ptr(d2.dev()), t2, ptr(o2.dev()),
                                               rows, ptr(length), ptr(overlap), ptr(mismatches), ptr(cell), ops._s())
        assert status == (0 if case in ("ok", "one_quality") else -1)
        length.fill_(-1)                                       # nothing to write: the merge call is about its arguments
        status = lib.bnpk_mates_merge_packed(ops.ctx, C.byref(h), ptr(d1.dev()), ptr(o1.dev()), ptr(q1.dev()), ptr(d2.dev()),
                                             ptr(o2.dev()), None if case == "one_quality" else ptr(q2.dev()), rows, ptr(length),
                                             ptr(out_off), None, None, ops._s())
        assert status == (0 if case == "ok" else -1)
