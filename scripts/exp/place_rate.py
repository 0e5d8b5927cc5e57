"""SeedIndex / place_reads / windows (csrc/seeds.hip) at the size of a sequencing run: reads of a genome placed back on it.

    python scripts/exp/place_rate.py [--genome 12000000] [--reads 50000000] [--runs 3]

The genome is ``synth`` mode 1's (``read_codes(1, G, seed, mode=1, genome_len=G)``), the reads are its mode-1 reads of 150
bases: a block of ``--block`` of them is made on the host and repeated on the device, and the true start of read ``id`` is
``mix64(seed + id) % (G - L + 1)``.  Checked on the FULL batch: every read is placed on strand 0 of row 0 at its true start.
CALL time is a host clock around a device synchronise after a warm-up call, all ``--runs`` printed; KERNEL time is one profiled
call (bnpk_prof_*).  From the placement's kernel time: lookups per second (two per k-mer: both strands) and the bytes a lookup
reads by design — table 8, keys ~24 (three steps), and for one that hits starts 16 and 4 per occurrence.  One JSON line at the end.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=12_000_000)
    ap.add_argument("--reads", type=int, default=50_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--block", type=int, default=100_000)
    ap.add_argument("-k", type=int, default=15)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261126)
    args = ap.parse_args()

    import numpy as np
    import bionumpy_amd as bnp
    from bionumpy_amd import synth
    from bionumpy_amd.device import Device, HArray
    from bionumpy_amd.encoded_array import EncodedArray, EncodedRaggedArray

    dev, ops = Device.get(), bnp.ops.get_ops()
    G, L, k = args.genome, args.read_len, args.k
    block = min(args.block, args.reads)
    reps = args.reads // block
    n = reps * block
    genome = EncodedRaggedArray(EncodedArray(synth.read_codes(1, G, args.seed, 1, G)[0], bnp.DNAEncoding), [G])
    codes = dev.upload(synth.read_codes(block, L, args.seed, 1, G).ravel()).repeat(reps)
    words = ops.pack_codes(HArray(dev=codes))
    del codes
    offsets = HArray(host=np.arange(n + 1, dtype=np.int64) * L)
    offsets.dev()
    truth = (synth.mix64(np.uint64(args.seed) + np.arange(block, dtype=np.uint64)) % np.uint64(G - L + 1)).astype(np.int32)
    truth = dev.upload(truth).repeat(reps)

    index = bnp.SeedIndex.from_sequences(genome, k=k)
    ref = index.reference
    ref_words = bnp.encoded_array.packed_words(ref._data)

    def place():
        return ops.seed_place(words, offsets, n * L, n, index._parts, ref.offsets(), 1, k, 8, 16, 2)

    placed = place()
    votes, second, strand, row, position = placed
    ok = bool((strand.dev() == 0).all() and (row.dev() == 0).all() and (position.dev() == truth).all())
    print("full-size check: %d reads of %d on %d bases, all on strand 0 at their true start: %s" % (n, L, G, ok), flush=True)
    assert ok, "a read was not placed at its true start"

    cases = {"index build": lambda: bnp.SeedIndex.from_sequences(genome, k=k), "placement": place,
             "windows": lambda: ops.seed_windows(ref_words, ref.offsets(), 1, strand, row, position, offsets, n, 24)}
    result = {"genome": G, "reads": n, "read_len": L, "k": k, "distinct_kmers": len(index), "cases": {}}
    lookups = 2 * n * (L - k + 1)
    for name, call in cases.items():
        call()
        ms = []
        for _ in range(args.runs):
            dev.synchronize()
            t0 = time.perf_counter()
            out = call()
            dev.synchronize()
            ms.append(round((time.perf_counter() - t0) * 1e3, 2))
            del out
        dev.prof_enable(True)
        dev.prof_reset()
        call()
        dev.synchronize()
        kernels = {key: round(v["total_ms"], 3) for key, v in dev.prof_report().items()}
        dev.prof_enable(False)
        result["cases"][name] = {"call_ms": ms, "kernel_ms": kernels}
        print("%-12s call %s ms  kernels %9.2f ms  %s" % (name, " / ".join("%9.2f" % t for t in ms), sum(kernels.values()), kernels), flush=True)
    kernel_s = result["cases"]["placement"]["kernel_ms"]["seed_place_packed"] / 1e3
    # by design: every lookup reads the table and ~3 keys, the half that hits (the forward strand) also starts and one position
    bytes_per_lookup = 8 + 24 + (16 + 4) / 2
    result["placement"] = {"reads_per_s": round(n / kernel_s), "lookups_per_s": round(lookups / kernel_s), "bytes_per_lookup": bytes_per_lookup,
                           "lookup_GB_per_s": round(lookups * bytes_per_lookup / kernel_s / 1e9, 1)}
    print("placement: %.1f M reads/s, %.2f G lookups/s, %.0f bytes a lookup by design = %.1f GB/s of dependent loads"
          % (n / kernel_s / 1e6, lookups / kernel_s / 1e9, bytes_per_lookup, lookups * bytes_per_lookup / kernel_s / 1e9), flush=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
