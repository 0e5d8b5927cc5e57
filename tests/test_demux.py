"""-m gpu: bnpk_demux_rows_packed / _bytes and bnp.assign_barcodes (csrc/demux.hip) against the Hamming distances numpy counts,
d = (win[:, None, :] != lib[None, :, :]).sum(-1), and the rules of include/bnpk.h written out.  Every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3), (4, 17), (8, 1), (15, 16), (16, 300), (17, 15), (32, 300)]     # (L, n_barcodes): n <= 4^L
N_ROWS = 330                                                   # crosses the 16-, 64- and 256-row edges, with a remainder
NONE = 255


class World:
    """a library of n distinct barcodes of L letters and about N_ROWS rows with their windows at `start`, in HBM, and the
    distances to every barcode"""

    def __init__(self, bnp, L, n, start, packed):
        from bionumpy_amd.device import HArray
        rng = np.random.default_rng(1000 * L + n)
        if 4 ** L <= 4096:
            lib = (rng.permutation(4 ** L)[:n, None] >> (2 * np.arange(L))) & 3
        else:
            lib = rng.permutation(np.unique(rng.integers(0, 4, (2 * n + 2, L)), axis=0))[:n]
        if L >= 8 and n >= 2:
            lib[1] = lib[0]
            lib[1, 2] = (lib[0, 2] + 1) % 4                    # two barcodes one letter apart
        assert np.unique(lib, axis=0).shape[0] == n
        rnd = lambda m: rng.integers(0, 4, m)
        row = lambda window: np.concatenate([rnd(start), window, rnd(rng.integers(0, 40))])
        rows, self.ambiguous = [], None
        for b in sorted({0, n - 1, (n - 1) // 16 * 16, n // 2}):  # first, last, the first of the last (partial) tile, one more
            for subs in range(4):
                w = lib[b].copy()
                at = rng.permutation(L)[:subs]
                w[at] = (w[at] + rng.integers(1, 4, at.size)) % 4
                rows.append(row(w))
        if L >= 8 and n >= 2:
            w = lib[0].copy()
            w[2] = (lib[0, 2] + 2) % 4                         # a third letter there: one mismatch to both
            self.ambiguous = len(rows)
            rows.append(row(w))
        if not packed:
            for b in (0, n - 1):
                w = lib[b].copy()
                w[rng.integers(0, L)] = 4                      # an N in the window
                rows.append(row(w))
        rows += [rnd(m) for m in (0, start, start + L - 1, start + L)]
        rows += [row(rnd(L)) for _ in range(N_ROWS - len(rows))]
        order = rng.permutation(len(rows))
        if self.ambiguous is not None:
            self.ambiguous = int(np.flatnonzero(order == self.ambiguous)[0])
        self.rows = [rows[i].astype(np.uint8) for i in order]
        self.lib, self.start, self.packed = lib.astype(np.uint8), start, packed
        ops = bnp.ops.get_ops()
        flat = HArray(host=np.concatenate(self.rows))
        self.total = flat.size
        self.data = ops.pack_codes(flat) if packed else flat
        self.offsets = HArray(host=np.concatenate([[0], np.cumsum([r.size for r in self.rows])]).astype(np.int64))
        self.whole = np.array([r.size >= start + L for r in self.rows])
        win = np.stack([r[start:start + L] if ok else np.full(L, 4) for r, ok in zip(self.rows, self.whole)])
        self.d = (win[:, None, :] != self.lib[None, :, :]).sum(-1).astype(np.int64)

    def expect(self, k, min_delta):
        """(index, dist, second) of include/bnpk.h from the distances"""
        d, n, at = self.d, self.lib.shape[0], np.arange(len(self.rows))
        best = d.argmin(axis=1)                                # (the smallest index among equals)
        dist = d[at, best]
        rest = d.copy()
        rest[at, best] = 1 << 30
        second = rest.min(axis=1) if n > 1 else np.full(len(self.rows), NONE)
        index = np.where((dist <= k) & ((n == 1) | (second - dist >= min_delta)), best, -1)
        return [np.where(self.whole, x, short) for x, short in ((index, -1), (dist, NONE), (second, NONE))]


@pytest.fixture(scope="module")
def bnp():
    import bionumpy_amd
    from bionumpy_amd import ops
    ops.set_ops(None)
    return bionumpy_amd


@pytest.fixture(scope="module")
def worlds(bnp):
    made = {}
    return lambda *key: made[key] if key in made else made.setdefault(key, World(bnp, *key))


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "bytes"])
@pytest.mark.parametrize("start", [0, 3, 29])
@pytest.mark.parametrize("L,n", SHAPES)
def test_rows(bnp, worlds, L, n, start, packed):
    w = worlds(L, n, start, packed)
    ops = bnp.ops.get_ops()
    for k, min_delta in ((0, 1), (1, 1), (2, 2), (L, 0)):      # (the last: the plain argmin)
        k = min(k, L)                                          # (L = 1: max_mismatches = 2 would be a bad argument)
        want = w.expect(k, min_delta)
        if L >= 8 and k == 1:                                  # the fixture holds every kind of row (on the reference alone)
            index, dist, second = want
            assert (index >= 0).any() and ((index < 0) & (dist > 1) & w.whole).any() and not w.whole.all()
            if n >= 2:                                         # (one barcode has no runner-up to be ambiguous with)
                assert (index[w.ambiguous], dist[w.ambiguous], second[w.ambiguous]) == (-1, 1, 1)
        got = ops.demux_rows(w.data, w.offsets, len(w.rows), w.total, w.lib, start, k, min_delta, packed)
        for g, e, what in zip(got, want, ("index", "dist", "second")):
            assert np.array_equal(g.host().astype(np.int64), e), (what, k, min_delta)


def test_public_interface(bnp, worlds):
    w = worlds(16, 300, 3, False)
    text = ["".join("ACGTN"[c] for c in r) for r in w.rows]
    barcodes = ["".join("ACGT"[c] for c in b) for b in w.lib]
    for reads in (text, bnp.as_encoded_array(text, bnp.ACGTnEncoding)):
        a = bnp.assign_barcodes(reads, barcodes, max_mismatches=1, start=3, min_delta=1)
        for got, want in zip((a.index, a.distance, a.second), w.expect(1, 1)):
            assert np.array_equal(np.asarray(got).astype(np.int64), want)
    # a.index == j is a mask on the device: a read filter on a chunk
    chunk = bnp.open(os.path.join(os.path.dirname(__file__), "golden", "reads.fq")).read()
    a = bnp.assign_barcodes(chunk, bnp.as_encoded_array(["CTT", "CGG"], bnp.DNAEncoding), max_mismatches=0)
    mask = a.index == 1
    assert isinstance(mask, type(a.index)) and mask.dtype == np.bool_ and np.asarray(a.index).tolist() == [0, 1]
    assert chunk[np.asarray(mask)].sequence.tolist() == ["CGG"]
    for bad in (dict(barcodes=["ACG", "AC"]), dict(barcodes=["ACX"]), dict(barcodes=["ACG", "TTT", "ACG"]),
                dict(barcodes=["ACG"], max_mismatches=4), dict(barcodes=["ACG"], max_mismatches=-1),
                dict(barcodes=["ACG"], start=-1), dict(barcodes=["ACG"], min_delta=-1)):
        with pytest.raises(ValueError):
            bnp.assign_barcodes(["ACGT"], **bad)
    with pytest.raises(ValueError, match="duplicate"):
        bnp.assign_barcodes(["ACGT"], ["ACG", "ACG"])
    for reads, barcodes in ((["ACGT"], ["A" * 33]), (bnp.as_encoded_array(["ACDE"], bnp.AminoAcidEncoding), ["AC"]),
                            (["ACGT"], np.full((1 << 20) + 1, "ACGTACGTACGT"))):
        with pytest.raises(NotImplementedError):
            bnp.assign_barcodes(reads, barcodes)


@pytest.mark.parametrize("case", ["no_barcodes", "too_many", "length_0", "length_33", "start_negative", "k_negative", "k_above_length",
                                  "delta_negative", "code_4", "no_codes", "ok"])
def test_bad_arguments(bnp, worlds, case):
    from bionumpy_amd._native import lib, DemuxLibrary, DEMUX_MAX_BARCODES
    from bionumpy_amd.device import ptr
    w, ops = worlds(8, 1, 0, True), bnp.ops.get_ops()
    codes = np.zeros((2, 8), dtype=np.uint8)
    codes[1, 7] = 4 if case == "code_4" else 1
    n = {"no_barcodes": 0, "too_many": DEMUX_MAX_BARCODES + 1}.get(case, 2)
    length = {"length_0": 0, "length_33": 33}.get(case, 8)
    k = {"k_negative": -1, "k_above_length": 9}.get(case, 1)
    desc = DemuxLibrary(n, length, -1 if case == "start_negative" else 0, k, -1 if case == "delta_negative" else 1,
                        None if case == "no_codes" else codes.ctypes.data)
    out = [ops.device.zeros(len(w.rows), t) for t in (np.int32, np.uint8, np.uint8)]
    for rows in (len(w.rows), 0):                              # (no rows: nothing launched, the library is still checked)
        status = lib.bnpk_demux_rows_packed(ops.ctx, C.byref(desc), ptr(w.data.dev()), w.total, ptr(w.offsets.dev()), rows,
                                            ptr(out[0]), ptr(out[1]), ptr(out[2]), ops._s())
        assert status == (0 if case == "ok" else -1)
