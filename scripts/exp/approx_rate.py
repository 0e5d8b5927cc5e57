"""find_approximate (csrc/approx.hip) against scan_motifs with one PWM of the same width (csrc/pwm_rows.hip) on the same
resident inputs: no earlier approximate path exists, the PWM scan is the yardstick.

    python scripts/exp/approx_rate.py [--reads 50000000] [--read-len 150] [--chromosome 12000000] [--runs 5]

Inputs are uniform random bases (seeded) in HBM in their 2-bit form: ``--reads`` reads of ``--read-len``, and one row of
``--chromosome`` bases.  Cases per input and per width (13 and 33): find_approximate at max_errors = 3, the same with
min_overlap = 3 (the trimming call), scan_motifs forward with one random PWM.  The cases alternate, ``--runs`` times each after
a warm-up call, timed with a host clock around a device synchronise; all times are printed (their spread is the noise).  Then
one profiled call per case gives the kernels' share (bnpk_prof_*).  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--chromosome", type=int, default=12_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd.device import Device

    dev = Device.get()
    rng = np.random.default_rng(args.seed)
    ops = bnp.ops.get_ops()
    adapter = "AGATCGGAAGAGCACACGTCTGAACTCCAGTCA"

    def rows_of(n_rows, length):
        if n_rows == 1:
            text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].tobytes().decode()
            one = bnp.as_encoded_array(text, bnp.DNAEncoding)
            seqs = bnp.EncodedRaggedArray(one.ravel(), [one.size])
        else:
            fastq = ops.synth_fastq(n_rows, length, args.seed, mode=0, genome_len=0, first_read=0)
            seqs = bnp.change_encoding(bnp.FastQBuffer.from_raw_buffer(fastq).get_field_by_number(1), bnp.DNAEncoding)
        seqs._compact()
        return seqs

    result = {"inputs": {}}
    for label, n_rows, length in (("reads", args.reads, args.read_len), ("chromosome", 1, args.chromosome)):
        seqs = rows_of(n_rows, length)
        cases = {}
        for width in (13, 33):
            pwm = bnp.PWM(rng.normal(size=(4, width)) * 2, "ACGT")
            cases["find_approximate m=%d k=3" % width] = lambda w=width: bnp.find_approximate(seqs, adapter[:w], 3)
            cases["find_approximate m=%d k=3 min_overlap=3" % width] = lambda w=width: bnp.find_approximate(seqs, adapter[:w], 3, 3)
            cases["scan_motifs width=%d" % width] = lambda p=pwm: bnp.scan_motifs(seqs, [p])
        ms = {name: [] for name in cases}
        for call in cases.values():
            call()                                           # warm-up
        for _ in range(args.runs):
            for name, call in cases.items():
                dev.synchronize()
                t0 = time.perf_counter()
                out = call()
                dev.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3)
                del out
        kernels = {}
        dev.prof_enable(True)
        for name, call in cases.items():
            dev.prof_reset()
            call()
            dev.synchronize()
            kernels[name] = {k: round(v["total_ms"], 3) for k, v in dev.prof_report().items()}
        dev.prof_enable(False)
        found = int(np.asarray(bnp.find_approximate(seqs, adapter[:13], 3).overlap[0] > 0).sum())
        entry = {"rows": n_rows, "row_len": length, "rows_found_m13": found, "cases": {}}
        for name in cases:
            entry["cases"][name] = {"ms": [round(t, 2) for t in ms[name]], "gbases_per_s": round(n_rows * length / min(ms[name]) / 1e6, 1),
                                    "kernels_ms": kernels[name]}
            print("%-11s %-42s %s ms  %8.1f Gbases/s  kernels %s" % (label, name, " / ".join("%8.2f" % t for t in ms[name]),
                                                                    n_rows * length / min(ms[name]) / 1e6, kernels[name]))
        result["inputs"][label] = entry
        del seqs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
