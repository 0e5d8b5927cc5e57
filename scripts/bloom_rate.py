"""Rates of the Bloom filter kernels (csrc/bloom.hip) on resident synthetic reads, against two filter sizes, next to the
k-mer index's lookups and to what the chip copies at.

    python scripts/bloom_rate.py [--reads 50000000] [--read-len 150] [--k 31] [--batch-reads 10000000] [--runs 2]

The reference set is a pseudo-random genome of ``--genome`` bases (5 M: a bacterium), given as synthetic reads at coverage 3.
Its k-mers go into two filters: one of 16 bits per genome base (10 MB: fits the on-chip caches) and one of ``--large-gib``
GiB (far larger than them: every lookup is a random 64-byte sector of HBM); and into a KmerIndex.  The queries are uniform
random reads, ``--reads`` of them, taken in batches of ``--batch-reads`` that are resident in HBM in their 2-bit form when
they are timed; per case the times of the batches are added up.  Cases, per filter:

    count_hits            BloomFilter.count_hits: bnpk_bloom_rows_packed, no hashes and no flags in HBM
    get_kmers + bf[kmers] the unfused pair: the hashes are written (8 bytes per k-mer), read again, a flag byte per k-mer written
    KmerIndex.count_hits  two binary searches per k-mer over the sorted pair list, on the same hashes (independent of the filter)

Every case runs ``--runs`` times after a warm-up call, timed with a host clock around a device synchronise; both times are
printed (their spread is the noise).  One JSON line at the end.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--batch-reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--large-gib", type=float, default=2.0)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=20260925)
    args = ap.parse_args()

    import torch
    import bionumpy_amd as bnp
    from bionumpy_amd._native import lib
    from bionumpy_amd.device import Device, HArray

    ops, dev, k = bnp.ops.get_ops(), Device.get(), args.k

    def reads_of(n, first, mode, genome_len=0):
        text = ops.synth_fastq(n, args.read_len, args.seed, mode=mode, genome_len=genome_len, first_read=first)
        return bnp.change_encoding(bnp.FastQBuffer.from_raw_buffer(text).get_field_by_number(1), bnp.DNAEncoding)

    def timed(call):
        call()                                               # warm-up (code objects, the allocator's blocks)
        out = []
        for _ in range(args.runs):
            dev.synchronize()
            t0 = time.perf_counter()
            call()
            dev.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    src = torch.empty(1 << 31, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    rates = (C.c_double * 4)()
    assert lib.bnpk_copy_rates(dev.ctx, C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), src.numel(), 5, rates, None) == 0
    copy_rate = max(rates)
    del src, dst

    reference = reads_of(3 * args.genome // args.read_len, 0, 1, args.genome)
    filters = {"small": bnp.BloomFilter(max(args.genome * 16 // 64, 1), k=k),
               "large": bnp.BloomFilter(int(args.large_gib * 2 ** 30) // 8, k=k)}
    for bf in filters.values():
        bf.insert(reference)
    index = bnp.KmerIndex.create_index(reference, k)

    cases = ["%s %s" % (name, what) for name in filters for what in ("count_hits", "get_kmers + bf[kmers]")] + ["KmerIndex.count_hits"]
    ms = {case: [0.0] * args.runs for case in cases}
    n_kmers = hits = 0
    for first in range(0, args.reads, args.batch_reads):
        reads = reads_of(min(args.batch_reads, args.reads - first), first, 0)
        reads._compact()
        n_rows, total = len(reads), reads.total()
        n_out = n_rows * max(args.read_len - k + 1, 0)
        n_kmers += n_out
        done = {}
        for name, bf in filters.items():
            done["%s count_hits" % name] = timed(lambda: bf.count_hits(reads))
            done["%s get_kmers + bf[kmers]" % name] = timed(lambda: bf[bnp.get_kmers(reads, k)])
        kmers = bnp.get_kmers(reads, k)._flat_data()
        done["KmerIndex.count_hits"] = timed(lambda: index.count_hits(kmers))
        hits += int(filters["small"].count_hits(reads).harray().dev().sum().item())
        del kmers, reads
        for case, times in done.items():
            ms[case] = [a + b for a, b in zip(ms[case], times)]

    result = {"reads": args.reads, "read_len": args.read_len, "k": k, "kmers": n_kmers, "copy_gb_per_s": round(copy_rate, 1),
              "filter_bytes": {name: bf.n_blocks * 8 for name, bf in filters.items()}, "hits_small": hits, "cases": {}}
    for case in cases:
        best = min(ms[case])
        print("%-34s %s ms   %7.2f G k-mers/s" % (case, " / ".join("%9.2f" % t for t in ms[case]), n_kmers / best / 1e6))
        result["cases"][case] = {"ms": [round(t, 2) for t in ms[case]], "gkmers_per_s": round(n_kmers / best / 1e6, 2)}
    print("device copy: %.0f GB/s; the packed reads are %.2f bytes per k-mer" % (copy_rate, args.reads * args.read_len / 4 / max(n_kmers, 1)))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
