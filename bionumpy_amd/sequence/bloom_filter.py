"""BloomFilter: a blocked Bloom filter over k-mers on the MI355X path (bionumpy/sequence/bloom_filter.py: "8 bits per kmer /
cache optimized bloom filter", a stub in the reference).

"Which of these reads share k-mers with that reference set?" — host or PhiX depletion, rRNA removal, contamination screens:

    bf = BloomFilter.from_sequences(reference_seqs, k=21, canonical=True)
    keep = bf.count_hits(reads) == 0

The filter is ``n_blocks`` 64-bit words in HBM; a k-mer lives in one word (the placement is written out in include/bnpk.h), so
membership is one 8-byte load and insertion one atomic OR.  DNA goes in and is asked about in its 2-bit form with the k-mers
rolled inside the kernels (csrc/bloom.hip): ``insert`` and ``count_hits`` write no hashes and no flags.

Departures from the reference's stub: the hash is the fixed one (no Python callables as hash functions),
``from_hash_functions_and_seqeuences`` and ``InterleavedBloomFilter`` are not provided.
"""
import numpy as np

from .._native import Bloom
from ..device import HArray, as_bool, as_harray
from ..encoded_array import EncodedArray, EncodedRaggedArray, as_encoded_array
from ..encodings.kmer_encodings import KmerEncoding
from ..ops import get_ops
from ..ragged import RaggedArray
from .kmers import _as_dna_ragged, _as_four_letter


class BloomFilter:
    def __init__(self, n_blocks, n_hashes=4, seed=0, k=21, canonical=False):
        if not 0 < k < 32:
            raise ValueError("k must be larger than 0 and smaller than 32")
        if not 1 <= n_hashes <= 5:
            raise ValueError("n_hashes must be 1 to 5 (bits per k-mer inside its 64-bit word)")
        if not 1 <= n_blocks < 2 ** 32:
            raise ValueError("n_blocks must be at least 1 and smaller than 2^32")
        self.n_blocks, self.n_hashes, self.seed, self.k, self.canonical = int(n_blocks), int(n_hashes), int(seed), int(k), bool(canonical)
        self._words = get_ops().device.zeros(self.n_blocks, np.int64)
        self._native = Bloom(self._words.data_ptr(), self.n_blocks, self.seed % 2 ** 64, self.n_hashes, self.k, int(self.canonical), 0)

    def __repr__(self):
        return "BloomFilter(%d blocks, n_hashes=%d, k=%d%s)" % (self.n_blocks, self.n_hashes, self.k, ", canonical" if self.canonical else "")

    @classmethod
    def from_sequences(cls, sequences, k=21, bits_per_kmer=16, n_hashes=4, canonical=False, seed=0):
        """a filter of ceil(windows * bits_per_kmer / 64) words that holds the k-mers of ``sequences``; the number of k-mer
        windows bounds the distinct k-mers from above, so nothing is counted first"""
        if not 0 < k < 32:
            raise ValueError("k must be larger than 0 and smaller than 32")
        parts = cls._packed_rows(sequences, canonical)
        _, windows = get_ops().row_offsets(parts[2], k)
        bf = cls(max(-(-windows * bits_per_kmer // 64), 1), n_hashes=n_hashes, seed=seed, k=k, canonical=canonical)
        bf._insert_packed(parts)
        return bf

    # -- what goes in ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _packed_rows(sequences, canonical):
        """(packed words, offsets, lens, n_rows, total) of sequences in a text or 4-letter encoding"""
        sequences = _as_four_letter(as_encoded_array(sequences))
        if sequences.encoding.alphabet_size != 4:
            raise ValueError("a BloomFilter takes sequences over a 4-letter alphabet, not %s" % sequences.encoding)
        if canonical and "".join(sequences.encoding.get_alphabet()).upper() != "ACGT":
            raise NotImplementedError("canonical k-mers need the ACGT alphabet (complement = 3 - code)")
        return _as_dna_ragged(sequences)

    def _hashes(self, kmers):
        """(flat int64 HArray, the ragged array the k-mers came as or None) of get_kmers() output / ints"""
        if isinstance(kmers, (EncodedArray, EncodedRaggedArray)):
            enc = kmers.encoding
            if enc.k != self.k or enc._alphabet_encoding.alphabet_size != 4:
                raise ValueError("the filter holds %d-mers of a 4-letter alphabet, these are %s" % (self.k, enc))
        ragged = kmers if isinstance(kmers, RaggedArray) else None
        if ragged is not None:
            ragged._compact()
            flat = ragged._flat_data()
        elif isinstance(kmers, EncodedArray):
            flat = kmers._harray()
        elif isinstance(kmers, (list, tuple)):
            flat = HArray(host=np.asarray(kmers, dtype=np.int64))
        else:
            flat = as_harray(kmers)
        if flat.dtype == np.uint64:                              # the same 64 bits: a view, where the words lie
            import torch
            flat = HArray(dev=flat.dev().view(torch.int64)) if flat.on_device else HArray(host=flat.host().view(np.int64))
        if flat.dtype != np.int64:                               # (nothing is converted on the host behind the caller's back)
            raise TypeError("k-mers are int64 (or uint64) hashes as get_kmers gives them, not %s" % flat.dtype)
        return flat, ragged

    @staticmethod
    def _is_kmers(x):
        """k-mers (get_kmers() output, int arrays, lists of ints) or sequences (everything else: text, DNA-encoded arrays)?"""
        if isinstance(x, (EncodedArray, EncodedRaggedArray)):
            return isinstance(x.encoding, KmerEncoding)
        if isinstance(x, (list, tuple)):
            return all(isinstance(v, (int, np.integer)) for v in x)
        return isinstance(x, (HArray, RaggedArray, np.ndarray)) or (hasattr(x, "host") and hasattr(x, "dev"))

    def _insert_packed(self, parts):
        packed, offsets, _, n_rows, total = parts
        if total:
            ops = get_ops()
            ops.bloom_insert_packed(self._native, packed, ops.kmer_start_mask(offsets, n_rows, total, self.k), total)

    # -- public ---------------------------------------------------------------------------------------------------------------
    def insert(self, x):
        """adds k-mers to the filter: those of DNA sequences (rolled from their 2-bit form inside the kernel), or k-mers given
        as get_kmers() output / an int64 array.  Cumulative: chunk after chunk builds one filter."""
        if self._is_kmers(x):
            get_ops().bloom_insert_hashes(self._native, self._hashes(x)[0])
        else:
            self._insert_packed(self._packed_rows(x, self.canonical))

    def __getitem__(self, kmers):
        """flags with the shape of ``kmers`` (ragged in, ragged out), resident in HBM: is the k-mer in the filter"""
        flat, ragged = self._hashes(kmers)
        flags = get_ops().bloom_query_hashes(self._native, flat)
        if ragged is not None:
            return RaggedArray._from_parts(as_bool(flags), None, ragged._lens, ragged.offsets(), len(ragged), ragged.total())
        from ..device_vector import DeviceVector
        return DeviceVector(flags, np.bool_)                   # (a bool vector is kept as its 0 / 1 bytes)

    def count_hits(self, sequences):
        """per sequence: how many of its k-mers are in the filter, device-resident; no hashes and no flags are written"""
        packed, offsets, _, n_rows, total = self._packed_rows(sequences, self.canonical)
        from ..device_vector import DeviceVector
        return DeviceVector(get_ops().bloom_rows(self._native, packed, offsets, n_rows, total))

    def words(self):
        """the filter: n_blocks uint64 words"""
        import torch
        return HArray(dev=self._words.view(torch.uint64))
