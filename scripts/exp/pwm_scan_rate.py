"""scan_motifs (csrc/pwm_rows.hip) against the way the same answer was had before it: get_motif_scores(reads, p).max(axis=-1)
per motif, on the same resident inputs.

    python scripts/exp/pwm_scan_rate.py [--reads 5000000] [--read-len 150] [--motifs 16] [--chromosome 10000000] [--runs 3]

Inputs are uniform random bases (seeded) in HBM in their 2-bit form: ``--reads`` reads of ``--read-len``, and one row of
``--chromosome`` bases.  The motifs are random log-odds matrices of widths 8 .. 20.  Cases per input: the old way (forward
strand: it has no other), scan_motifs forward, scan_motifs on both strands with thresholds.  The cases alternate, ``--runs``
times each after a warm-up call, timed with a host clock around a device synchronise; all times are printed (their spread
is the noise).  The forward results are compared before anything is timed.  Then one profiled call per scan case gives the
kernels' share (bnpk_prof_*).  A lookup is one M[j][code] added: windows x width (x 2 on both strands).  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--motifs", type=int, default=16)
    ap.add_argument("--chromosome", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd.device import Device

    dev = Device.get()
    rng = np.random.default_rng(args.seed)
    widths = [8 + (5 * i) % 13 for i in range(args.motifs)]
    pwms = [bnp.PWM(rng.normal(size=(4, w)) * 2, "ACGT") for w in widths]
    ops = bnp.ops.get_ops()

    def rows_of(n_rows, length):
        if n_rows == 1:                                      # one long row: text through the encoder
            text = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, length)].tobytes().decode()
            one = bnp.as_encoded_array(text, bnp.DNAEncoding)
            seqs = bnp.EncodedRaggedArray(one.ravel(), [one.size])
        else:                                                # uniform random reads from the device generator
            fastq = ops.synth_fastq(n_rows, length, args.seed, mode=0, genome_len=0, first_read=0)
            seqs = bnp.change_encoding(bnp.FastQBuffer.from_raw_buffer(fastq).get_field_by_number(1), bnp.DNAEncoding)
        seqs._compact()
        return seqs

    def old_way(seqs):
        return [bnp.get_motif_scores(seqs, p).max(axis=-1) for p in pwms]

    result = {"motifs": args.motifs, "widths": widths, "inputs": {}}
    for label, n_rows, length in (("reads", args.reads, args.read_len), ("chromosome", 1, args.chromosome)):
        seqs = rows_of(n_rows, length)
        cases = {"get_motif_scores().max() per motif": lambda: old_way(seqs),
                 "scan_motifs forward": lambda: bnp.scan_motifs(seqs, pwms),
                 "scan_motifs both strands + thresholds": lambda: bnp.scan_motifs(seqs, pwms, both_strands=True, thresholds=8.0)}
        old, new = old_way(seqs), bnp.scan_motifs(seqs, pwms)
        same = all(np.array_equal(np.asarray(old[m]), np.asarray(new.best_score[m])) for m in range(args.motifs))
        del old, new
        ms = {name: [] for name in cases}
        for name, call in cases.items():
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
        for name in list(cases)[1:]:
            dev.prof_reset()
            cases[name]()
            dev.synchronize()
            kernels[name] = {k: round(v["total_ms"], 3) for k, v in dev.prof_report().items()}
        dev.prof_enable(False)
        lookups = sum(n_rows * max(length - w + 1, 0) * w for w in widths)
        entry = {"rows": n_rows, "row_len": length, "lookups_forward": lookups, "same_best_scores": bool(same), "cases": {}}
        for name in cases:
            n = lookups * (2 if "both" in name else 1)
            entry["cases"][name] = {"ms": [round(t, 2) for t in ms[name]], "glookups_per_s": round(n / min(ms[name]) / 1e6, 1),
                                    "kernels_ms": kernels.get(name)}
            print("%-11s %-40s %s ms  %8.1f G lookups/s  kernels %s" % (label, name, " / ".join("%9.2f" % t for t in ms[name]),
                                                                       n / min(ms[name]) / 1e6, kernels.get(name)))
        print("%-11s forward best scores equal to the old way's: %s" % (label, same))
        result["inputs"][label] = entry
        del seqs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
