"""assign_barcodes (csrc/demux.hip) at the sizes of a pooled run, and next to it the nearest thing the library had before:
find_approximate with the barcodes as patterns (csrc/approx.hip), on a subset of the reads small enough to hold its
pattern-major outputs.

    python scripts/exp/demux_rate.py [--reads 50000000] [--read-len 150] [--subset 2000000] [--runs 5]

Inputs are uniform random bases (seeded) in HBM, as 2-bit words (_packed) and as ACGTn code bytes (_bytes); the barcodes are
seeded random and distinct, the window starts at symbol 0.  Cases: (L, n) = (8, 96), (8, 384), (16, 1536), (16, 65536), both
layouts, max_mismatches = 1; on the subset (8, 96) through assign_barcodes and through find_approximate(max_errors=1).  The
cases of a group alternate, ``--runs`` times each after a warm-up call; CALL time is a host clock around a device
synchronise, all of them printed (their spread is the noise).  KERNEL time is one profiled call per case (bnpk_prof_*: device
events around the call's launches, the library upload included).  Matrix operations are counted from the shapes — rows
padded to 256, barcodes to 16, 64 * KSTEPS i8 multiply-adds, 2 operations each — over that kernel time.  Every case is
checked against numpy on a seeded sample of rows before it is timed.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

CASES = [(8, 96), (8, 384), (16, 1536), (16, 65536)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--subset", type=int, default=2_000_000)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd.device import Device

    dev = Device.get()
    rng = np.random.default_rng(args.seed)
    ops = bnp.ops.get_ops()

    def rows_of(n_rows, seed):
        fastq = ops.synth_fastq(n_rows, args.read_len, seed, mode=0, genome_len=0, first_read=0)
        field = bnp.FastQBuffer.from_raw_buffer(fastq).get_field_by_number(1)
        packed, plain = bnp.change_encoding(field, bnp.DNAEncoding), bnp.change_encoding(field, bnp.ACGTnEncoding)
        packed._compact()
        plain._compact()
        return packed, plain

    def library(L, n):
        codes = rng.permutation(np.unique(rng.integers(0, 4, (n + n // 2 + 8, L)), axis=0))[:n]
        assert codes.shape[0] == n
        return codes, ["".join("ACGT"[c] for c in b) for b in codes]

    def check(seqs, codes, text, mask):
        """all three vectors of a call against numpy on the sampled rows"""
        a = bnp.assign_barcodes(seqs, text, max_mismatches=1)
        got = [np.asarray(x)[mask].astype(np.int64) for x in (a.index, a.distance, a.second)]
        L, at = codes.shape[1], np.arange(int(mask.sum()))
        win = np.array([["ACGT".index(c) for c in s[:L]] for s in seqs[mask].tolist()])
        d = np.concatenate([(win[i:i + 32, None, :] != codes[None, :, :]).sum(-1) for i in range(0, len(win), 32)]).astype(np.int64)
        best = d.argmin(axis=1)
        dist = d[at, best]
        d[at, best] = 1 << 30
        second = d.min(axis=1)
        index = np.where((dist <= 1) & (second - dist >= 1), best, -1)
        assert all(np.array_equal(g, w) for g, w in zip(got, (index, dist, second))), "differs from numpy on the sample"
        return int((index >= 0).sum())

    def measure(cases):
        """{name: (call, pairs, matrix operations)} -> per name: call times, kernel times"""
        ms = {name: [] for name in cases}
        for call, _, _ in cases.values():
            call()                                           # warm-up
        for _ in range(args.runs):
            for name, (call, _, _) in cases.items():
                dev.synchronize()
                t0 = time.perf_counter()
                out = call()
                dev.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
                del out
        out = {}
        dev.prof_enable(True)
        for name, (call, pairs, matrix_ops) in cases.items():
            dev.prof_reset()
            call()
            dev.synchronize()
            kernels = {k: round(v["total_ms"], 3) for k, v in dev.prof_report().items()}
            kernel_ms = sum(v for k, v in kernels.items() if k.startswith(("demux", "approx")))
            out[name] = {"call_ms": [round(t, 2) for t in ms[name]], "kernel_ms": kernels,
                         "ps_per_pair_call": round(min(ms[name]) * 1e9 / pairs, 3),
                         "ps_per_pair_call_worst": round(max(ms[name]) * 1e9 / pairs, 3)}
            line = "%-44s call %s ms  %8.3f ps/pair  kernels %s" % (name, " / ".join("%8.2f" % t for t in ms[name]),
                                                                    min(ms[name]) * 1e9 / pairs, kernels)
            if matrix_ops:
                out[name]["matrix_tops"] = round(matrix_ops / kernel_ms / 1e9, 1)
                line += "  %7.1f matrix Top/s (shapes over kernel time)" % (matrix_ops / kernel_ms / 1e9)
            print(line, flush=True)
        dev.prof_enable(False)
        return out

    def pad(x, to):
        return (x + to - 1) // to * to

    result = {"reads": args.reads, "read_len": args.read_len, "subset_rows": args.subset}
    packed, plain = rows_of(args.reads, args.seed)
    mask = np.zeros(args.reads, dtype=bool)
    mask[rng.choice(args.reads, min(args.sample, args.reads), replace=False)] = True
    cases, assigned = {}, {}
    for L, n in CASES:
        codes, text = library(L, n)
        for label, seqs in (("packed", packed), ("bytes", plain)):
            name = "assign_barcodes L=%d n=%d %s" % (L, n, label)
            assigned[name] = check(seqs, codes, text, mask)
            cases[name] = (lambda s=seqs, t=text: bnp.assign_barcodes(s, t, max_mismatches=1), args.reads * n,
                           pad(args.reads, 256) * pad(n, 16) * 64 * (2 if L > 16 else 1) * 2)
    result["full"] = measure(cases)
    result["sample_rows_assigned"] = assigned
    del packed, plain, cases

    # the parent's nearest offer: every barcode as a pattern under the edit distance, pattern-major outputs
    packed, _ = rows_of(args.subset, args.seed + 1)
    codes, text = library(8, 96)
    pairs = args.subset * 96
    result["subset"] = measure({
        "subset: assign_barcodes L=8 n=96 packed": (lambda: bnp.assign_barcodes(packed, text, max_mismatches=1), pairs,
                                                    pad(args.subset, 256) * 96 * 64 * 2),
        "subset: find_approximate m=8 n=96 k=1": (lambda: bnp.find_approximate(packed, text, 1), pairs, 0)})
    print(json.dumps(result))


if __name__ == "__main__":
    main()
