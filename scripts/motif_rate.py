"""Rates of the motif kernels (csrc/motif.hip) on a batch of synthetic reads, next to the literal match_string kernels and
to what the chip copies at.

    python scripts/motif_rate.py [--reads 50000000] [--read-len 150] [--steps 5]

Times, with the library's hipEvent timers and after a warm-up call, on the 2-bit sequence column of a synthetic FASTQ batch:
the "same" flags (bnpk_motif_flags_packed: 1 byte written per base) and the rows' counts (bnpk_motif_rows_packed: nothing
written but 8 bytes per read) of "[AG].[AT]", "AA.{,1}[CT]" and the literal "GATTACA"; and, from the unchanged literal
kernels, match_string(reads, "GATTACA")'s flags (row ends + start mask + bnpk_match_windows_packed) and its ``.any(axis=-1)``
(bnpk_match_rows_packed).  Prints per case: ms, GB/s of the bytes read + written, and that rate as a fraction of the
fastest device copy (bnpk_copy_rates).  One JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=20260925)
    args = ap.parse_args()

    import numpy as np
    import torch
    import bionumpy_amd as bnp
    from bionumpy_amd._native import lib
    from bionumpy_amd.device import Device
    from bionumpy_amd.encoded_array import packed_words
    from bionumpy_amd.ops import get_ops
    from bionumpy_amd.sequence.string_matcher import RegexMatcher

    ops, dev = get_ops(), Device.get()
    text = ops.synth_fastq(args.reads, args.read_len, args.seed)
    view = bnp.FastQBuffer.from_raw_buffer(text).get_field_by_number(1)
    dna = bnp.change_encoding(view, bnp.DNAEncoding)
    n_rows, total, offsets = len(dna), dna.total(), dna.offsets()
    packed = packed_words(dna._data)
    del text, view
    ends = ops.row_end_mask(offsets, n_rows, total)
    literal = np.asarray(bnp.as_encoded_array("GATTACA", bnp.DNAEncoding).raw()).astype(np.uint8)
    _, n_windows = ops.row_offsets(dna._lens, literal.size)

    src = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rates = (C.c_double * 4)()
    assert lib.bnpk_copy_rates(dev.ctx, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel(), 5, rates, None) == 0
    copy_rate = max(rates)
    del src, dst

    words, table = total / 4, 8 * n_rows
    cases = []
    for pattern in ("[AG].[AT]", "AA.{,1}[CT]", "GATTACA"):
        program = RegexMatcher(pattern, bnp.DNAEncoding)._native
        cases.append(("motif flags %s" % pattern, ["motif_flags_packed"], words + total / 8 + total,
                      lambda p=program: ops.motif_flags(packed, offsets, n_rows, total, p, True, row_ends=ends)))
        cases.append(("motif rows %s" % pattern, ["motif_rows_packed"], words + 2 * table,
                      lambda p=program: ops.motif_rows(packed, offsets, n_rows, total, p)))
    cases.append(("match_string flags GATTACA", ["row_end_mask", "kmer_starts_from_ends", "match_windows_packed"], words + total / 8 + n_windows + table,
                  lambda: ops.match_windows(packed, offsets, n_rows, total, n_windows, literal, True)))
    cases.append(("match_string rows GATTACA", ["match_rows_packed"], words + 2 * table,
                  lambda: ops.match_rows(packed, offsets, n_rows, total, literal)))

    result = {"reads": args.reads, "read_len": args.read_len, "bases": total, "copy_gb_per_s": round(copy_rate, 1), "cases": {}}
    for label, timers, nbytes, call in cases:
        call()                                               # warm-up
        dev.prof_enable(True)
        dev.prof_reset()
        for _ in range(args.steps):
            call()
        dev.synchronize()
        prof = dev.prof_report()
        dev.prof_enable(False)
        ms = sum(prof[t]["total_ms"] for t in timers if t in prof) / args.steps
        gbs = nbytes / (ms * 1e-3) / 1e9
        print("%-34s %8.3f ms  %8.1f GB/s  %.2f of the copy rate (%.0f GB/s)" % (label, ms, gbs, gbs / copy_rate, copy_rate))
        result["cases"][label] = {"ms": round(ms, 3), "gb_per_s": round(gbs, 1), "frac_of_copy": round(gbs / copy_rate, 3)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
