"""find_mate_overlaps / merge_pairs (csrc/mates.hip) at the size of a sequencing run: pairs of 2 x 150 bp resident in HBM.

    python scripts/exp/mates_rate.py [--pairs 50000000] [--read-len 150] [--runs 5]

The pairs are cut on the host (seeded) from a random genome in a block of ``--block`` pairs, which is repeated on the device to
``--pairs``: 70 % overlapping fragments (read-len .. 2 read-len - 30), 10 % read-through (read-len / 2 .. read-len - 1; the
tails are whatever follows in the genome) and 20 % unrelated mates, 1 % substitutions in mate 2; qualities 2 .. 41.  Cases: the
overlap kernel on 2-bit words and on ACGTn code bytes, the merge kernel on 2-bit words with qualities, and
bnpk_reverse_complement_packed over mate 2 alone — the pass over HBM the overlap kernel does without.  The cases alternate,
``--runs`` times each after a warm-up call; CALL time is a host clock around a device synchronise, all of them printed (their
spread is the noise); KERNEL time is one profiled call per case (bnpk_prof_*: device events around the call's launches).  The
block's results are checked against the definition on a sample of pairs before anything is timed.  Symbol comparisons are
counted from the lengths: the sum of ov(s) over the candidate offsets.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

PARAMS = (30, 5, 20, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--block", type=int, default=500_000)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd.device import Device, HArray

    dev, ops = Device.get(), bnp.ops.get_ops()
    rng = np.random.default_rng(args.seed)
    L, block = args.read_len, min(args.block, args.pairs)
    reps = args.pairs // block
    n = reps * block

    genome = rng.integers(0, 4, block * 3 * L + 4 * L, dtype=np.uint8)
    kind = rng.choice(3, block, p=[0.7, 0.1, 0.2])
    f = np.where(kind == 1, rng.integers(L // 2, L, block), rng.integers(L, 2 * L - 29, block))
    p = np.arange(block, dtype=np.int64) * 3 * L + L
    at = np.arange(L)
    mate1 = genome[p[:, None] + at]
    start2 = np.where(kind == 2, p + 2 * L, p + f - L)       # (unrelated: the stretch behind the fragment)
    b = genome[start2[:, None] + at]
    subs = rng.random(b.shape) < 0.01
    b = np.where(subs, (b + rng.integers(1, 4, b.shape)) % 4, b).astype(np.uint8)
    mate2 = (3 - b)[:, ::-1]
    qual = rng.integers(2, 42, (2, block, L), dtype=np.uint8)

    def ref_length(a, m2):
        bb, found = 3 - m2[::-1], []
        for s in range(1 - L, L):
            lo, hi = max(0, s), min(L, s + L)
            mm = int((a[lo:hi] != bb[lo - s:hi - s]).sum())
            if hi - lo >= PARAMS[0] and mm <= PARAMS[1] and 100 * mm <= PARAMS[2] * (hi - lo):
                found.append((lo - hi, mm, s))
        return min(found)[2] + L if found else -1

    def resident(rows):
        t = dev.upload(np.ascontiguousarray(rows).ravel())
        return HArray(dev=t.repeat(reps))

    codes = [resident(mate1), resident(mate2)]
    quals = [resident(qual[0]), resident(qual[1])]
    packed = [ops.pack_codes(c) for c in codes]
    offsets = HArray(host=np.arange(n + 1, dtype=np.int64) * L)
    offsets.dev()
    total = n * L

    def overlap(data, is_packed):
        return ops.mates_overlap(data[0], offsets, total, data[1], offsets, total, n, *PARAMS, is_packed)

    length = overlap(packed, True)[0]
    got = length.host()
    sample = rng.choice(block, min(args.sample, block), replace=False)
    want = np.array([ref_length(mate1[i], mate2[i]) for i in sample])
    assert np.array_equal(got[sample], want) and np.array_equal(got[n - block + sample], want), "differs from the definition"
    assert np.array_equal(overlap(codes, False)[0].host(), got), "the bytes path differs from the packed one"
    merged = float((got >= 0).mean())
    comparisons = n * sum(min(L, s + L) - max(0, s) for s in range(PARAMS[0] - L, L - PARAMS[0] + 1))

    cases = {
        "mates_overlap packed": lambda: overlap(packed, True),
        "mates_overlap bytes": lambda: overlap(codes, False),
        "mates_merge packed + qualities": lambda: ops.mates_merge(packed[0], offsets, quals[0], packed[1], offsets, quals[1], n, length,
                                                                  41, True),
        "reverse_complement_packed (mate 2)": lambda: ops.reverse_complement_packed(packed[1], offsets, n, total),
    }
    ms = {name: [] for name in cases}
    for call in cases.values():
        call()                                               # warm-up
    for _ in range(args.runs):
        for name, call in cases.items():
            dev.synchronize()
            t0 = time.perf_counter()
            out = call()
            dev.synchronize()
            ms[name].append((time.perf_counter() - t0) * 1e3)
            del out
    result = {"pairs": n, "read_len": L, "merged_fraction": round(merged, 4), "symbol_comparisons": comparisons, "cases": {}}
    dev.prof_enable(True)
    for name, call in cases.items():
        dev.prof_reset()
        call()
        dev.synchronize()
        kernels = {k: round(v["total_ms"], 3) for k, v in dev.prof_report().items()}
        result["cases"][name] = {"call_ms": [round(t, 2) for t in ms[name]], "kernel_ms": kernels}
        print("%-36s call %s ms  kernels %s" % (name, " / ".join("%8.2f" % t for t in ms[name]), kernels), flush=True)
    dev.prof_enable(False)
    k = result["cases"]["mates_overlap packed"]["kernel_ms"]["mates_overlap_packed"]
    rc = result["cases"]["reverse_complement_packed (mate 2)"]["kernel_ms"]["reverse_complement_packed"]
    result["overlap_packed_tera_comparisons_per_s"] = round(comparisons / k / 1e9, 2)
    result["overlap_packed_over_reverse_complement"] = round(k / rc, 2)
    print("%d pairs, %.1f %% merged; overlap (packed) %.2f ms = %.2f T symbol comparisons/s = %.1f x the reverse complement pass (%.2f ms)"
          % (n, 100 * merged, k, comparisons / k / 1e9, k / rc, rc))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
