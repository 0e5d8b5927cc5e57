// Blocked Bloom filter over 2-bit k-mers ("8 bits per kmer / cache optimized bloom filter", bionumpy/sequence/bloom_filter.py:37-42:
// BloomFilter.insert / __getitem__), gfx950.
//
//   The filter is n_blocks 64-bit words.  A k-mer lives in ONE word: g = fmix64(h ^ seed) picks the word with its high 32 bits
//   (block = (g >> 32) * n_blocks >> 32, no power of two needed) and n_hashes <= 5 bits inside it with 6-bit fields of its low
//   30 bits.  Membership is therefore one 8-byte load, insertion one 64-bit atomic OR — and the OR is skipped when a plain load
//   shows the bits set already (the k-mers of a genome at coverage c are c - 1 times repeats).
//
//   Hash path (int64 k-mers in HBM): a lane takes several k-mers, computes all their places, issues all their filter loads, and
//   only then looks at the first answer; eight 0 / 1 flags leave as one 8-byte store.
//
//   Packed path (2-bit bases in HBM, no hashes anywhere): position-flat like wf_generate_kernel (kmers.hip) — a lane owns 8
//   consecutive positions: two packed words (positions 8 i .. 8 i + 7 + 30 end inside them), one funnel shift for the first
//   k-mer, a 2-bit roll for each further one; the canonical form rolls the reverse-complement hash alongside (rc' = rc << 2 |
//   3 - b), so nothing is reversed per position.
//     insert: the k-mer start mask says which of the 8 positions hold a k-mer; their 8 loads, then their conditional atomics.
//     rows  : the tile's rows (their offsets staged in LDS, as rc_packed_kernel does) say it themselves: one lane per ROW sets
//             the <= k - 1 positions in front of its end in a 2048-bit "no k-mer here" plane in LDS (two 32-bit atomic ORs at
//             most), a lane reads its byte of that plane, does its 8 loads and writes its byte of the HIT plane in LDS, and one
//             lane per row takes the popcount of the row's span of the hit plane.  Neither pass over the rows searches anything,
//             so a tile whose rows do not fit the LDS table (rows of a few bases) runs the same code on the offsets in global
//             memory.  A row inside the tile is stored, a row that crosses a tile edge adds its part atomically to counts the
//             call has zeroed.
#include "common.h"
#include "rows.h"

namespace {

constexpr int BL_ITEMS = 8;                                  // positions (packed path) / k-mers (query) per lane
constexpr int BL_TILE = BNPK_BLOCK * BL_ITEMS;               // 2048 positions per workgroup
constexpr int BL_LDS_ROWS = 510;                             // rows of a tile whose offsets are staged
constexpr int BL_INSERT_ITEMS = 4;                           // k-mers a lane of the hash-path insert has in flight

// the filter as the kernels read it (by value: wave-uniform)
struct bl_desc {
  unsigned long long* words;
  uint64_t seed;
  uint32_t n_blocks;
  int n_hashes, k, canonical;
};

__device__ __forceinline__ uint64_t fmix64(uint64_t x) {
  x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the word and the bits inside it of the k-mer with (canonical, if asked) hash h
__device__ __forceinline__ void bl_place(const bl_desc& F, uint64_t h, uint32_t& block, uint64_t& bits) {
  const uint64_t g = fmix64(h ^ F.seed);
  block = __umulhi((uint32_t)(g >> 32), F.n_blocks);
  const uint32_t lo = (uint32_t)g;                           // (five 6-bit fields: bits 0 .. 29)
  bits = 1ull << (lo & 63u);
#pragma unroll
  for (int j = 1; j < 5; ++j)
    if (j < F.n_hashes) bits |= 1ull << ((lo >> (6 * j)) & 63u);
}

__device__ __forceinline__ uint64_t bl_canonical(uint64_t h, int k) {
  const uint64_t rc = ~(reverse_2bit_groups(h) >> (64 - 2 * k)) & ((1ull << (2 * k)) - 1ull);
  return min(h, rc);
}

// ---- hash path -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BNPK_BLOCK) void bl_insert_hashes_kernel(const int64_t* __restrict__ kmers, int64_t n, bl_desc F) {
  const int64_t stride = (int64_t)gridDim.x * BNPK_BLOCK;
  for (int64_t i0 = (int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x; i0 < n; i0 += stride * BL_INSERT_ITEMS) {
    uint32_t block[BL_INSERT_ITEMS];
    uint64_t bits[BL_INSERT_ITEMS], have[BL_INSERT_ITEMS];
#pragma unroll
    for (int q = 0; q < BL_INSERT_ITEMS; ++q) {
      const int64_t i = i0 + q * stride;
      const uint64_t h = i < n ? (uint64_t)kmers[i] : 0ull;
      bl_place(F, F.canonical ? bl_canonical(h, F.k) : h, block[q], bits[q]);
    }
#pragma unroll
    for (int q = 0; q < BL_INSERT_ITEMS; ++q) have[q] = i0 + q * stride < n ? F.words[block[q]] : ~0ull;
#pragma unroll
    for (int q = 0; q < BL_INSERT_ITEMS; ++q)
      if ((have[q] & bits[q]) != bits[q]) atomicOr(&F.words[block[q]], (unsigned long long)bits[q]);
  }
}

// kmers 16-byte aligned, flags 8-byte aligned: a lane's eight k-mers are four 16-byte loads, its flags one 8-byte store
__global__ __launch_bounds__(BNPK_BLOCK) void bl_query_hashes_kernel(const int64_t* __restrict__ kmers, int64_t n, bl_desc F,
                                                                    uint8_t* __restrict__ flags) {
  const unsigned long long* __restrict__ words = F.words;
  const int64_t n_chunks = (n + BL_ITEMS - 1) / BL_ITEMS;
  for (int64_t c = (int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * BNPK_BLOCK) {
    const int64_t base = c * BL_ITEMS;
    const int left = (int)min((int64_t)BL_ITEMS, n - base);
    uint64_t h[BL_ITEMS];
    if (left == BL_ITEMS) {
#pragma unroll
      for (int q = 0; q < BL_ITEMS; q += 2) {
        const ulonglong2 two = *reinterpret_cast<const ulonglong2*>(kmers + base + q);
        h[q] = two.x; h[q + 1] = two.y;
      }
    } else {
#pragma unroll
      for (int q = 0; q < BL_ITEMS; ++q) h[q] = q < left ? (uint64_t)kmers[base + q] : 0ull;
    }
    uint32_t block[BL_ITEMS];
    uint64_t bits[BL_ITEMS], have[BL_ITEMS];
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) bl_place(F, F.canonical ? bl_canonical(h[q], F.k) : h[q], block[q], bits[q]);
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) have[q] = q < left ? words[block[q]] : 0ull;
    uint64_t out = 0;
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) out |= (uint64_t)((have[q] & bits[q]) == bits[q]) << (8 * q);
    if (left == BL_ITEMS) {
      *reinterpret_cast<uint64_t*>(flags + base) = out;
    } else {
      for (int q = 0; q < left; ++q) flags[base + q] = (uint8_t)(out >> (8 * q));
    }
  }
}

// ---- packed path -----------------------------------------------------------------------------------------------------------------
// the (canonical, if asked) hashes of the k-mers that start at positions o .. o + 7, o a multiple of 8 inside the data; W has
// n_words = ceil(n_bases / 32) words.  What a hash takes from behind the last base belongs to no marked position.
__device__ __forceinline__ void bl_roll8(const uint64_t* __restrict__ W, int64_t n_words, int64_t o, const bl_desc& F,
                                         uint64_t (&h8)[BL_ITEMS]) {
  const int64_t wi = o >> 5;
  const uint64_t w0 = W[wi], w1 = wi + 1 < n_words ? W[wi + 1] : 0ull;
  const int k = F.k, sh0 = 2 * (int)(o & 31), top = 2 * k - 2;
  const uint64_t kmask = (1ull << (2 * k)) - 1ull;
  uint64_t h = (sh0 ? (w0 >> sh0) | (w1 << (64 - sh0)) : w0) & kmask;
  const int sn = sh0 + 2 * k;                                // 2 .. 110: the seven bases that enter behind the first k-mer
  const uint32_t next = (uint32_t)(sn < 64 ? (w0 >> sn) | (w1 << (64 - sn)) : w1 >> (sn - 64));
  uint64_t rc = ~(reverse_2bit_groups(h) >> (64 - 2 * k)) & kmask;
#pragma unroll
  for (int q = 0; q < BL_ITEMS; ++q) {
    if (q) {
      const uint64_t b = (next >> (2 * (q - 1))) & 3u;
      h = (h >> 2) | (b << top);
      rc = ((rc << 2) & kmask) | (3ull - b);
    }
    h8[q] = F.canonical ? min(h, rc) : h;
  }
}

__global__ __launch_bounds__(BNPK_BLOCK) void bl_insert_packed_kernel(const uint64_t* __restrict__ W, int64_t n_words,
                                                                     const uint8_t* __restrict__ mask8, int64_t n_bases, bl_desc F) {
  const int64_t n_chunks = (n_bases + BL_ITEMS - 1) / BL_ITEMS;
  for (int64_t c = (int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * BNPK_BLOCK) {
    const unsigned v = mask8[c];
    if (!v) continue;
    uint64_t h8[BL_ITEMS], bits[BL_ITEMS], have[BL_ITEMS];
    uint32_t block[BL_ITEMS];
    bl_roll8(W, n_words, c * BL_ITEMS, F, h8);
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) bl_place(F, h8[q], block[q], bits[q]);
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) have[q] = ((v >> q) & 1u) ? F.words[block[q]] : ~0ull;
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q)
      if ((have[q] & bits[q]) != bits[q]) atomicOr(&F.words[block[q]], (unsigned long long)bits[q]);
  }
}

__global__ void bl_zero_kernel(unsigned long long* __restrict__ x, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) x[i] = 0ull;
}

// bits [a, b) of a plane of 32-bit words, 0 <= a < b
__device__ __forceinline__ uint32_t bl_span32(int a, int b, int w) {
  const int lo = max(a - 32 * w, 0), hi = min(b - 32 * w, 32);
  return (hi >= 32 ? ~0u : (1u << hi) - 1u) & ~((1u << lo) - 1u);
}

// one workgroup per tile of 2048 positions; counts zeroed by the caller
__global__ __launch_bounds__(BNPK_BLOCK) void bl_rows_kernel(const uint64_t* __restrict__ W, int64_t n_words,
                                                            const int64_t* __restrict__ off, int64_t n_rows, int64_t total,
                                                            const int64_t* __restrict__ tile_rows, int64_t n_tiles, bl_desc F,
                                                            unsigned long long* __restrict__ counts) {
  __shared__ int64_t srow[BL_LDS_ROWS + 2];
  __shared__ uint32_t none[BL_TILE / 32];                    // bit p: no k-mer starts at position tile0 + p
  __shared__ uint64_t hit[BL_TILE / 64];                     // bit p: the k-mer at tile0 + p is in the filter
  const unsigned long long* __restrict__ words = F.words;
  const int64_t tile0 = (int64_t)blockIdx.x * BL_TILE, tile1 = min(tile0 + BL_TILE, total);
  const int64_t o = tile0 + (int64_t)threadIdx.x * BL_ITEMS;
  const bool live = o < total;
  uint64_t h8[BL_ITEMS];
  if (live) bl_roll8(W, n_words, o, F, h8);                  // (the packed words are asked for before the rows are looked at)
  int64_t lo, hi;
  tile_row_range(tile_rows, blockIdx.x, n_tiles, n_rows, lo, hi);
  lo = min(max(lo, (int64_t)0), n_rows - 1);                 // (offsets that do not end at n_bases must not lead outside them)
  hi = min(max(hi, lo), n_rows - 1);
  const int64_t nr = hi - lo + 1;                            // rows lo .. hi can have positions in the tile
  const bool staged = nr + 1 <= BL_LDS_ROWS + 2;             // (uniform) offsets lo .. hi + 1
  if (threadIdx.x < BL_TILE / 32) none[threadIdx.x] = 0u;
  if (staged)
    for (int i = threadIdx.x; i <= (int)nr; i += BNPK_BLOCK) srow[i] = off[lo + i];
  __syncthreads();
  auto offset_of = [&](int64_t i) { return staged ? srow[i] : off[lo + i]; };
  // a row's last k - 1 positions (all of them, if it is shorter) start no k-mer
  for (int64_t i = threadIdx.x; i < nr; i += BNPK_BLOCK) {
    const int64_t s = offset_of(i), e = offset_of(i + 1);
    const int64_t b0 = max(max(s, e - (F.k - 1)), tile0), b1 = min(e, tile1);
    if (b0 < b1) {
      const int a = (int)(b0 - tile0), b = (int)(b1 - tile0);
      for (int w = a >> 5; w <= (b - 1) >> 5; ++w) atomicOr(&none[w], bl_span32(a, b, w));
    }
  }
  __syncthreads();
  unsigned hits = 0u;
  if (live) {
    const int64_t left = total - o;
    const unsigned v = ~(unsigned)reinterpret_cast<const uint8_t*>(none)[threadIdx.x] & (left >= BL_ITEMS ? 0xffu : (1u << (int)left) - 1u);
    uint64_t bits[BL_ITEMS], have[BL_ITEMS];
    uint32_t block[BL_ITEMS];
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) bl_place(F, h8[q], block[q], bits[q]);
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) have[q] = ((v >> q) & 1u) ? words[block[q]] : 0ull;
#pragma unroll
    for (int q = 0; q < BL_ITEMS; ++q) hits |= (unsigned)((have[q] & bits[q]) == bits[q]) << q;
    hits &= v;
  }
  reinterpret_cast<uint8_t*>(hit)[threadIdx.x] = (uint8_t)hits;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < nr; i += BNPK_BLOCK) {
    const int64_t s = offset_of(i), e = offset_of(i + 1);
    const int64_t c0 = max(s, tile0), c1 = min(e, tile1);
    if (c0 >= c1) continue;
    const int a = (int)(c0 - tile0), b = (int)(c1 - tile0);
    unsigned n = 0u;
    for (int w = a >> 6; w <= (b - 1) >> 6; ++w) {
      uint64_t x = hit[w];
      if (a > 64 * w) x &= ~0ull << (a - 64 * w);
      if (b < 64 * w + 64) x &= (1ull << (b - 64 * w)) - 1ull;
      n += (unsigned)__popcll(x);
    }
    if (s >= tile0 && e <= tile1) counts[lo + i] = n;         // the whole row lies in this tile
    else if (n) atomicAdd(&counts[lo + i], (unsigned long long)n);
  }
}

// ---- the filter: checked, and put into the kernels' form (host) ---------------------------------------------------------------------
static int bl_prepare(const bnpk_bloom* f, bl_desc* F) {
  if (!f || f->k < 1 || f->k > 31 || f->n_hashes < 1 || f->n_hashes > 5) return BNPK_ERR_ARG;
  if (f->n_blocks < 1 || f->n_blocks >= (1ull << 32)) return BNPK_ERR_RANGE;
  if (!f->d_words) return BNPK_ERR_ARG;
  F->words = reinterpret_cast<unsigned long long*>(f->d_words);
  F->seed = f->seed;
  F->n_blocks = (uint32_t)f->n_blocks;
  F->n_hashes = f->n_hashes;
  F->k = f->k;
  F->canonical = f->canonical ? 1 : 0;
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_bloom_insert_hashes(bnpk_ctx* ctx, const bnpk_bloom* h_filter, const int64_t* d_kmers, int64_t n, void* stream) {
  if (!ctx || n < 0) return BNPK_ERR_ARG;
  bl_desc F;
  BNPK_CHECK(bl_prepare(h_filter, &F));
  if (n == 0) return BNPK_OK;
  if (!d_kmers) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "bloom_insert_hashes", s);
  hipLaunchKernelGGL(bl_insert_hashes_kernel, dim3(grid_for(ceil_div(n, (int64_t)BNPK_BLOCK * BL_INSERT_ITEMS))), dim3(BNPK_BLOCK), 0, s,
                     d_kmers, n, F);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_bloom_query_hashes(bnpk_ctx* ctx, const bnpk_bloom* h_filter, const int64_t* d_kmers, int64_t n, uint8_t* d_flags,
                            void* stream) {
  if (!ctx || n < 0) return BNPK_ERR_ARG;
  bl_desc F;
  BNPK_CHECK(bl_prepare(h_filter, &F));
  if (n == 0) return BNPK_OK;
  if (!d_kmers || !d_flags) return BNPK_ERR_ARG;
  if (((uintptr_t)d_kmers & 15u) || ((uintptr_t)d_flags & 7u)) return BNPK_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "bloom_query_hashes", s);
  hipLaunchKernelGGL(bl_query_hashes_kernel, dim3(grid_for(ceil_div(ceil_div(n, BL_ITEMS), BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_kmers,
                     n, F, d_flags);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_bloom_insert_packed(bnpk_ctx* ctx, const bnpk_bloom* h_filter, const uint64_t* d_packed, const uint64_t* d_start_mask,
                             int64_t n_bases, void* stream) {
  if (!ctx || n_bases < 0) return BNPK_ERR_ARG;
  bl_desc F;
  BNPK_CHECK(bl_prepare(h_filter, &F));
  if (n_bases == 0) return BNPK_OK;
  if (!d_packed || !d_start_mask) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "bloom_insert_packed", s);
  hipLaunchKernelGGL(bl_insert_packed_kernel, dim3(grid_for(ceil_div(ceil_div(n_bases, BL_ITEMS), BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s,
                     d_packed, ceil_div(n_bases, (int64_t)32), reinterpret_cast<const uint8_t*>(d_start_mask), n_bases, F);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_bloom_rows_packed(bnpk_ctx* ctx, const bnpk_bloom* h_filter, const uint64_t* d_packed, int64_t n_bases,
                           const int64_t* d_offsets, int64_t n_rows, int64_t* d_counts, void* stream) {
  if (!ctx || n_bases < 0 || n_rows < 0) return BNPK_ERR_ARG;
  bl_desc F;
  BNPK_CHECK(bl_prepare(h_filter, &F));
  if (n_rows == 0) return BNPK_OK;
  if (!d_offsets || !d_counts || (n_bases > 0 && !d_packed)) return BNPK_ERR_ARG;
  const int64_t n_tiles = ceil_div(n_bases, (int64_t)BL_TILE);
  if (n_tiles > BNPK_MAX_BLOCKS) return BNPK_ERR_RANGE;
  hipStream_t s = (hipStream_t)stream;
  void* table = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, tile_rows_bytes(n_tiles), &table, s));
  bnpk_timer t(ctx, "bloom_rows_packed", s);
  unsigned long long* counts = reinterpret_cast<unsigned long long*>(d_counts);
  hipLaunchKernelGGL(bl_zero_kernel, dim3(grid_for(ceil_div(n_rows, 256))), dim3(256), 0, s, counts, n_rows);
  BNPK_HIP(ctx, hipGetLastError());
  if (n_bases == 0) return BNPK_OK;
  BNPK_CHECK(build_tile_rows(ctx, d_offsets, n_rows, BL_TILE, (int64_t*)table, s));
  hipLaunchKernelGGL(bl_rows_kernel, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_packed, ceil_div(n_bases, (int64_t)32), d_offsets,
                     n_rows, n_bases, (const int64_t*)table, n_tiles, F, counts);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
