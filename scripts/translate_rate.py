"""Rates of the translation kernels (csrc/translate.hip) on a batch of synthetic reads, next to what the chip copies at.

    python scripts/translate_rate.py [--reads 50000000] [--read-len 150] [--steps 5]

Times, with the library's hipEvent timers and after a warm-up call, translate_dna_to_protein's two kernels on the
sequence column of a synthetic FASTQ batch — the text where it lies in the chunk (bnpk_translate_rows) and the 2-bit
form (bnpk_translate_packed), forward and reverse strand — and bnpk_reverse_complement_rows on the same column.  Prints
per case: ms, GB/s of the bytes read + written, and that rate as a fraction of the fastest device copy
(bnpk_copy_rates, the figure bench.py --full reports as measured_copy_gb_per_s).  One JSON line at the end.
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

    import torch
    import bionumpy_amd as bnp
    from bionumpy_amd._native import lib
    from bionumpy_amd.device import Device
    from bionumpy_amd.encoded_array import packed_words
    from bionumpy_amd.ops import get_ops
    from bionumpy_amd.sequence.translate import DNAToProtein

    ops, dev = get_ops(), Device.get()
    text = ops.synth_fastq(args.reads, args.read_len, args.seed)
    view = bnp.FastQBuffer.from_raw_buffer(text).get_field_by_number(1)      # the sequence lines, not gathered
    assert not view.is_compact()
    n_rows, total, offsets = len(view), view.total(), view.offsets()
    dna = bnp.change_encoding(view, bnp.DNAEncoding)
    packed = packed_words(dna._data)
    out_lens, out_offsets, n_out, _ = ops.translate_plan(offsets, n_rows, 0)
    table = DNAToProtein()._letters()

    src = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rates = (C.c_double * 4)()
    assert lib.bnpk_copy_rates(dev.ctx, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel(), 5, rates, None) == 0
    copy_rate = max(rates)
    del src, dst

    cases = [
        ("translate text view", "translate_bytes", total + n_out,
         lambda: ops.translate_rows(view._flat_data(), view._starts, offsets, n_rows, total, out_offsets, n_out, table, 0, 0)),
        ("translate text view, reverse", "translate_bytes", total + n_out,
         lambda: ops.translate_rows(view._flat_data(), view._starts, offsets, n_rows, total, out_offsets, n_out, table, 0, 1)),
        ("translate packed", "translate_packed", total / 4 + n_out,
         lambda: ops.translate_packed(packed, offsets, n_rows, total, out_offsets, n_out, table, 0, 0)),
        ("translate packed, reverse", "translate_packed", total / 4 + n_out,
         lambda: ops.translate_packed(packed, offsets, n_rows, total, out_offsets, n_out, table, 0, 1)),
        ("reverse_complement_rows", "reverse_complement_bytes", 2 * total,
         lambda: ops.reverse_complement_rows(view._flat_data(), view._starts, offsets, n_rows, total)),
    ]
    result = {"reads": args.reads, "read_len": args.read_len, "bases": total, "letters": n_out,
              "copy_gb_per_s": round(copy_rate, 1), "cases": {}}
    for label, timer, nbytes, call in cases:
        call()                                               # warm-up
        dev.prof_enable(True)
        dev.prof_reset()
        for _ in range(args.steps):
            call()
        dev.synchronize()
        prof = dev.prof_report()[timer]
        dev.prof_enable(False)
        ms = prof["total_ms"] / prof["launches"]
        gbs = nbytes / (ms * 1e-3) / 1e9
        print("%-32s %8.3f ms  %8.1f GB/s  %.2f of the copy rate (%.0f GB/s)" % (label, ms, gbs, gbs / copy_rate, copy_rate))
        result["cases"][label] = {"ms": round(ms, 3), "gb_per_s": round(gbs, 1), "frac_of_copy": round(gbs / copy_rate, 3)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
