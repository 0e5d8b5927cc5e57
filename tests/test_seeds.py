"""-m gpu: bnp.SeedIndex / place_reads / Placements.windows (csrc/seeds.hip) against the definition of include/bnpk.h written
out over lists and a dict from k-mer to positions.  Every comparison is exact."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COMPLEMENT = str.maketrans("ACGT", "TGCA")
LENGTHS = [700, 0, 37, 1500]


def rc(s):
    return s.translate(COMPLEMENT)[::-1]


def rand(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def make_reference():
    """four rows; a 40-base segment in 3 places, another in 9 and a 120-base segment in exactly 2"""
    rng = np.random.default_rng(2026)
    rows = [list(rand(rng, n)) for n in LENGTHS]
    seg3, seg9, seg120 = rand(rng, 40), rand(rng, 40), rand(rng, 120)
    for seg, places in ((seg3, [(0, 520), (0, 600), (3, 1100)]), (seg120, [(3, 100), (3, 900)]),
                        (seg9, [(0, 120), (0, 220), (0, 320), (0, 420), (3, 300), (3, 400), (3, 500), (3, 600), (3, 700)])):
        for r, at in places:
            rows[r][at:at + len(seg)] = seg
    return ["".join(r) for r in rows], seg3, seg9, seg120


REF, SEG3, SEG9, SEG120 = make_reference()
OFF = np.concatenate([[0], np.cumsum(LENGTHS)]).tolist()
INDEXES = {}


def ref_index(k):
    if k not in INDEXES:
        INDEXES[k] = {}
        for r, row in enumerate(REF):
            for x in range(len(row) - k + 1):
                INDEXES[k].setdefault(row[x:x + k], []).append(OFF[r] + x)
    return INDEXES[k]


def ref_place(read, k, max_occ, band, min_votes):
    """(votes, second, strand, row, position) by the definition"""
    index, L, hits = ref_index(k), len(read), []
    for p in range(L - k + 1):
        kmer = read[p:p + k]
        for s, key, at in ((0, kmer, p), (1, rc(kmer), L - k - p)):
            occ = index.get(key, [])
            if 1 <= len(occ) <= max_occ:
                hits += [(s, g - at, g) for g in occ]
    c = Counter((s, d // band) for s, d, _ in hits)
    W = {sb: n + c.get((sb[0], sb[1] + 1), 0) for sb, n in c.items()}
    if not W:
        return 0, 0, -1, -1, 0
    s, b = min(W, key=lambda sb: (-W[sb], sb))
    second = max([w for sb, w in W.items() if sb[0] != s or abs(sb[1] - b) >= 2], default=0)
    if W[s, b] < min_votes:
        return W[s, b], second, -1, -1, 0
    D, g = min((d, g) for s2, d, g in hits if s2 == s and d // band in (b, b + 1))
    row = max(r for r in range(len(REF)) if OFF[r] <= g and LENGTHS[r])
    return W[s, b], second, s, row, D - OFF[row]


def make_reads(k, min_votes=2):
    """[(name, read, (row, start) of a clean forward read | None)]"""
    rng, reads = np.random.default_rng(k), []
    for L in (0, k - 1, k, k + 1, k + 62, k + 63, k + 64, 150, 511, 512):    # k + 63: 64 k-mers, the wavefront's edge
        for r, at in ((3, 200),) if L > 150 else ((3, 1150 + L % 7), (0, 5 + L % 5)):
            src = REF[r][at:at + L]
            reads += [("clean%d" % L, src, (r, at)), ("clean%d-" % L, rc(src), None)]
    src = REF[3][1200:1350]
    for j in range(3):
        sub = list(REF[3][220 + 300 * j:370 + 300 * j])
        for x in (20, 75, 130):
            sub[x] = "ACGT"["ACGT".index(sub[x]) ^ 1 + j]
        reads += [("subs%d" % j, "".join(sub), None), ("subs%d-" % j, rc("".join(sub)), None)]
    reads += [("ins", src[:70] + "GCA" + src[70:147], None), ("del", src[:70] + src[73:], None)]
    edge = [REF[3][at:at + 153] for at in (1310, 1311)]        # global starts 2047 and 2048: B - 1 and 0 modulo every band
    reads += [("edge-1", edge[0][:70] + edge[0][73:], None), ("edge0", rc(edge[1][:70] + "TTG" + edge[1][70:150]), None)]
    reads += [("before row 0", rand(rng, 10) + REF[0][:100], None), ("behind row 0", REF[0][620:] + rand(rng, 30), None),
              ("rows 2 and 3", REF[2][-20:] + REF[3][:60], None)]
    half = REF[3][1220:1280]
    reads += [("3 copies", SEG3, None), ("9 copies", SEG9, None), ("tie", SEG120, None), ("palindrome", half + rc(half), None),
              ("tiled", SEG3 * 12, None), ("tiled-", rc(SEG3 * 12), None)]          # k = 8: over 1024 hits, the large class
    reads += [("random%d" % j, rand(rng, 60), None) for j in range(3)]
    m = k + min_votes - 2                                      # min_votes - 1 k-mers between flanks that differ in every base
    flanked = REF[3][1380:1400].translate(COMPLEMENT) + REF[3][1400:1400 + m] + REF[3][1400 + m:1420 + m].translate(COMPLEMENT)
    return reads + [("one vote short", flanked, None)]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


@pytest.fixture(scope="module")
def index_of(bnp):
    built = {}

    def get(k):
        if k not in built:
            built[k] = bnp.SeedIndex.from_sequences(REF, k=k)
        return built[k]
    return get


def columns(p):
    return list(zip(*(np.asarray(x).tolist() for x in (p.votes, p.second, p.strand, p.row, p.position))))


@pytest.mark.parametrize("min_votes", [1, 3])
@pytest.mark.parametrize("max_occ,band", [(1, 1), (3, 16), (8, 64), (9, 256)])
@pytest.mark.parametrize("k", [8, 15, 31])
def test_against_definition(bnp, index_of, k, max_occ, band, min_votes):
    reads = [r for r in make_reads(k, min_votes) if 2 * (len(r[1]) - k + 1) * max_occ <= 4096]
    want = [ref_place(r[1], k, max_occ, band, min_votes) for r in reads]
    p = bnp.place_reads([r[1] for r in reads], index_of(k), max_occurrences=max_occ, band=band, min_votes=min_votes)
    for got, w, r in zip(columns(p), want, reads):
        assert got == w, (r[0], len(r[1]))
    assert np.asarray(p.is_placed).tolist() == [w[2] >= 0 for w in want] and len(p) == len(reads)
    assert {w[2] for w in want} == {0, 1, -1} and min(w[4] for w in want) < 0 and max(w[1] for w in want) > 0
    assert ref_place(SEG9, k, 8, band, min_votes) != ref_place(SEG9, k, 9, band, min_votes)
    tie = want[[r[0] for r in reads].index("tie")]
    assert max_occ < 2 or (tie[0] == tie[1] and tie[2:] == (0, 3, 100))


@pytest.mark.parametrize("k", [8, 31])
def test_index_arrays(bnp, index_of, k):
    codes = [np.array(["ACGT".index(c) for c in row], dtype=np.int64) for row in REF]
    kmers = np.concatenate([sum(row[j:len(row) - k + 1 + j] << 2 * j for j in range(k)) if len(row) >= k else row[:0] for row in codes])
    where = np.concatenate([OFF[r] + np.arange(max(0, n - k + 1)) for r, n in enumerate(LENGTHS)])
    order = np.lexsort((where, kmers))
    keys, first = np.unique(kmers[order], return_index=True)
    idx = index_of(k)
    assert idx.k == k and len(idx) == keys.size and np.asarray(idx.positions).dtype == np.int32
    assert np.array_equal(np.asarray(idx.keys), keys) and np.array_equal(np.asarray(idx.starts), np.append(first, kmers.size))
    assert np.array_equal(np.asarray(idx.positions), where[order])


def test_windows_feed_align_pairs(bnp, index_of):
    reads = [r for r in make_reads(15) if 2 * (len(r[1]) - 14) * 8 <= 4096]
    seqs =bnp.as_encoded_array([r[1] for r in reads], bnp.DNAEncoding)
    p = bnp.place_reads(seqs, index_of(15))
    placed = columns(p)
    assert placed == [ref_place(r[1], 15, 8, 16, 2) for r in reads]
    for pad in (0, 24):
        w, cut, starts = p.windows(seqs, pad=pad), [], []
        for (_, _, strand, row, at), r in zip(placed, reads):
            a, b = (max(0, at - pad), min(LENGTHS[row], at + len(r[1]) + pad)) if strand >= 0 else (0, 0)
            piece = REF[row][a:b] if strand >= 0 else ""
            cut.append(rc(piece) if strand == 1 else piece)
            starts.append(a)
        assert w.sequences.tolist() == cut and np.asarray(w.start).tolist() == starts and w.sequences.encoding == bnp.DNAEncoding
        clean = [i for i, r in enumerate(reads) if r[0].startswith("clean") and placed[i][2] >= 0]
        assert len(clean) >= 20
        sub = bnp.place_reads([reads[i][1] for i in clean], index_of(15))
        ws = sub.windows([reads[i][1] for i in clean], pad=pad)
        al = bnp.align_pairs([reads[i][1] for i in clean], ws.sequences, match=1, mismatch=-1, gap_open=1, gap_extend=1, mode="semiglobal")
        assert np.asarray(al.score).tolist() == [len(reads[i][1]) for i in clean]
        for j, i in enumerate(clean):
            if reads[i][2] is not None:
                assert (placed[i][2], placed[i][3]) == (0, reads[i][2][0])
                assert int(np.asarray(ws.start)[j]) + int(np.asarray(al.target_start)[j]) == reads[i][2][1]


def test_capacity_and_errors(bnp, index_of):
    long_read, ok = REF[3][200:712], REF[3][50:120]
    p = bnp.place_reads([ok, long_read], index_of(8), max_occurrences=4)       # 2 x 505 x 4 = 4040 possible hits
    assert columns(p) == [ref_place(r, 8, 4, 16, 2) for r in (ok, long_read)] and columns(p)[1][2:] == (0, 3, 200)
    for rows, bad in (([ok, long_read], 1), ([long_read, ok], 0)):             # 2 x 505 x 5 = 5050
        with pytest.raises(NotImplementedError, match="read %d " % bad):
            bnp.place_reads(rows, index_of(8), max_occurrences=5)
    with pytest.raises(NotImplementedError, match="read 2 "):
        bnp.place_reads([ok, ok, REF[3][:513]], index_of(15), max_occurrences=1)
    amino = bnp.as_encoded_array(["ACDE"], bnp.AminoAcidEncoding)
    for rows in ([ok, ok], []):                                # the arguments are checked without rows too
        reads = bnp.as_encoded_array(rows, bnp.DNAEncoding)
        for bad in (dict(max_occurrences=0), dict(max_occurrences=2049), dict(band=0), dict(band=24), dict(band=512), dict(min_votes=0)):
            with pytest.raises(ValueError):
                bnp.place_reads(reads, index_of(15), **bad)
    for call in (lambda: bnp.place_reads(amino, index_of(15)), lambda: bnp.SeedIndex.from_sequences(amino), lambda: bnp.SeedIndex.from_sequences(REF, k=7),
                 lambda: bnp.SeedIndex.from_sequences(REF, k=32)):
        with pytest.raises(ValueError):
            call()
    lib, ctx = bnp._native.lib, bnp.ops.get_ops().ctx
    for block in ((7, 8, 16, 2, 10), (15, 0, 16, 2, 10), (15, 8, 48, 2, 10), (15, 8, 16, 0, 10), (15, 8, 16, 2, 31)):
        assert lib.bnpk_seed_place_packed(ctx, C.byref(bnp._native.SeedParams(*block, 0)), *([0] * 18)) == -1      # BNPK_ERR_ARG
    assert lib.bnpk_seed_place_packed(ctx, None, *([0] * 18)) == -1
    none = bnp.place_reads([], index_of(15))
    assert len(none) == 0 and columns(none) == [] and np.asarray(none.is_placed).size == 0
    assert none.windows([]).sequences.tolist() == [] and len(bnp.SeedIndex.from_sequences(["ACGT", ""], k=8)) == 0
