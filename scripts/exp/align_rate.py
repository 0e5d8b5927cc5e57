"""align_pairs (csrc/align.hip) at the size of a sequencing run: pairs of rows resident in HBM, cell updates per second.

    python scripts/exp/align_rate.py [--pairs 50000000] [--long-pairs 1000000] [--runs 3]

Two shapes: ``--pairs`` pairs of 150 x 150 (the small class: 16 lanes a pair) and ``--long-pairs`` of 512 x 512 (64 lanes a
pair).  A block of ``--block`` pairs is made on the host (seeded: the target is the query with 2 % substitutions, one
inserted and one deleted run of three) and repeated on the device.  Cases: local alignment under (2, -3, 5, 2), score only and
with traceback (the CIGAR columns included), on 2-bit words and on code bytes.  The yardstick of the package is
find_approximate with one 32-letter pattern on the same reads, against align_pairs semiglobal with that pattern as every
pair's query under (0, -1, 0, 1), whose -score is the same distance (checked).  The cases alternate, ``--runs`` times each
after a warm-up call; CALL time is a host clock around a device synchronise, all of them printed; KERNEL time is one profiled
call per case (bnpk_prof_*).  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--long-pairs", type=int, default=1_000_000)
    ap.add_argument("--block", type=int, default=100_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd.device import Device, HArray

    dev, ops = Device.get(), bnp.ops.get_ops()
    rng = np.random.default_rng(args.seed)
    matrix = np.where(np.eye(4, dtype=bool), 2, -3)
    unit = np.where(np.eye(4, dtype=bool), 0, -1)

    def shape(n_pairs, L):
        """(codes, packed, offsets, n, total) of both sides: n pairs of L x L"""
        block = min(args.block, n_pairs)
        reps = n_pairs // block
        q = rng.integers(0, 4, (block, L), dtype=np.uint8)
        t = np.where(rng.random(q.shape) < 0.02, rng.integers(0, 4, q.shape, dtype=np.uint8), q)
        a, b = L // 3, 2 * L // 3                                # three symbols inserted at a, three deleted at b: still L
        t = np.concatenate([t[:, :a], rng.integers(0, 4, (block, 3), dtype=np.uint8), t[:, a:b], t[:, b + 3:]], axis=1)[:, :L]
        t = np.concatenate([t, rng.integers(0, 4, (block, L - t.shape[1]), dtype=np.uint8)], axis=1)
        codes = [HArray(dev=dev.upload(np.ascontiguousarray(x).ravel()).repeat(reps)) for x in (q, t)]
        n = reps * block
        offsets = HArray(host=np.arange(n + 1, dtype=np.int64) * L)
        offsets.dev()
        return codes, [ops.pack_codes(c) for c in codes], offsets, n, n * L

    def align(s, packed, traceback, mode=0, m=matrix, go=5, ge=2, queries=None):
        codes, words, offsets, n, total = s
        data = words if packed else codes
        q, qoff, qtotal = (data[0], offsets, total) if queries is None else queries
        return ops.align_pairs(q, qoff, qtotal, data[1], offsets, total, n, n, m, go, ge, mode, traceback, packed)

    result = {"cases": {}}
    shapes = {"150x150": shape(args.pairs, 150), "512x512": shape(args.long_pairs, 512)}
    cases = {}
    for name, s in shapes.items():
        base = align(s, True, True)
        assert all(np.array_equal(x.host(), y.host()) for x, y in zip(align(s, False, False)[:3], base[:3])), "bytes differ from packed"
        for packed in (True, False):
            for tb in (False, True):
                cases["%s %s %s" % (name, "packed" if packed else "bytes", "traceback" if tb else "score")] = (
                    s[3] * int(name[:3]) ** 2, lambda s=s, packed=packed, tb=tb: align(s, packed, tb))
    # the yardstick: one 32-letter pattern against the 150-symbol targets
    reads = shapes["150x150"]
    pattern = rng.integers(0, 4, 32, dtype=np.uint8)
    n = reads[3]
    pat_rows = (ops.pack_codes(HArray(dev=dev.upload(pattern).repeat(n))), HArray(host=np.arange(n + 1, dtype=np.int64) * 32), n * 32)
    pat_rows[1].dev()
    masks = np.array([[sum(1 << i for i in range(32) if pattern[i] == c) for c in range(4)]], dtype=np.uint64)
    approx = lambda: ops.approx_rows(reads[1][1], reads[2], n, reads[4], masks, 31, 0, [32], True)
    semi = lambda: align(reads, True, False, mode=1, m=unit, go=0, ge=1, queries=pat_rows)
    assert np.array_equal(-semi()[0].host(), approx()[0].host().astype(np.int32)), "-score differs from find_approximate's distance"
    cases["find_approximate, 32 letters"] = (n * 32 * 150, approx)
    cases["align_pairs semiglobal, 32 rows"] = (n * 32 * 150, semi)

    ms = {name: [] for name in cases}
    for _ in range(args.runs):
        for name, (_, call) in cases.items():
            dev.synchronize()
            t0 = time.perf_counter()
            out = call()
            dev.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            del out
    dev.prof_enable(True)
    for name, (cells, call) in cases.items():
        dev.prof_reset()
        call()
        dev.synchronize()
        kernels = {k: round(v["total_ms"], 3) for k, v in dev.prof_report().items()}
        total_ms = sum(kernels.values())
        result["cases"][name] = {"cells": cells, "call_ms": [round(t, 2) for t in ms[name]], "kernel_ms": kernels,
                                 "giga_cells_per_s": round(cells / total_ms / 1e6, 1)}
        print("%-36s call %s ms  kernels %8.2f ms = %7.1f G cells/s  %s" % (name, " / ".join("%8.2f" % t for t in ms[name]), total_ms,
                                                                           cells / total_ms / 1e6, kernels), flush=True)
    dev.prof_enable(False)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
