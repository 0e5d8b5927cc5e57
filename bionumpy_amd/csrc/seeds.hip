// Seed-and-vote read placement on a k-mer position index (bnpk_seed_index_positions / _finish, bnpk_seed_place_packed) and the
// reference windows that align_pairs takes (bnpk_seed_window_lengths, bnpk_seed_windows_packed).  The semantics are those of
// include/bnpk.h; DESIGN.md 4d.
//
//   Split.  A read belongs to one wavefront, a wavefront is a workgroup, and the grid is as many workgroups as the card holds
//   at once (the LDS of one permitting), striding over the reads: the lookups are chains of dependent global loads, and what
//   hides them is the number of reads in flight.  Lane l takes the k-mers at the read positions l, l + 64, ...: the k-mer out
//   of two packed words, rc(h) from reverse_2bit_groups of the same register, so both strands' lookups come from one
//   extraction.
//
//   Lookup.  table[h >> (2k - T)] and its neighbour bound the binary search in `keys` (T is chosen by the build so that a
//   bucket holds ~8 keys: three steps), then starts[u], starts[u + 1] and the occurrences themselves.  A lookup that hits
//   reads 8 (table) + ~24 (keys) + 16 (starts) + 4 occ (positions) bytes; one that misses stops after the keys.
//
//   Hits.  A hit is ONE 64-bit word in LDS: strand << 41 | (d + 512) << 10 | p', p' the k-mer's start in the oriented read
//   (g = d + p').  The issue's 32-bit hit has no room for p', and the anchor needs it: with p' in the low bits, sorting the
//   words puts the anchor (smallest d, then smallest g) FIRST in its bin, and nothing has to be looked up twice.  The slots
//   come from a wavefront prefix sum over the lanes' occurrence counts; the words are then sorted where they lie by a
//   bitonic network over the next power of two (>= 64) of the read's hit count, every stage a pass of the 64 lanes.
//
//   Votes.  Sorted, a (strand, bin) is a run and its neighbour bin, if it has hits, is the NEXT run.  A lane that finds a
//   run's head (its bin differs from the word before) gets W = c(s, b) + c(s, b + 1) with one binary search for the end of
//   bin b + 1 — a bin of the other strand is never b + 1: the strand bit is compared —, keeps the first largest W of its heads,
//   and V_MAX over W << 12 | 4095 - t across the lanes gives the winner, the first in sorted order among equals: smaller s,
//   then smaller b.  A second pass of the same shape, without the winner's strand's bins b - 1 .. b + 1, gives the runner-up.
//   The winner's head word is the anchor.
//
//   Two size classes, two launches of one template.  Small: 1024 hits, 8 KB of LDS, 20 reads a CU in flight; it takes EVERY
//   read (a 150-base read in unique sequence has ~136 hits whatever max_occurrences allows) and hands the read whose hits do
//   not fit — known only after the lookups — to a list in HBM.  Large: 4096 hits, 32 KB, 5 reads a CU; it takes that list.
//   4096 is the bound of the interface (2 n max_occurrences), so no hit is ever dropped; a read over the bound, or over 512
//   symbols, is refused before any lookup.  Registers hold a lane's counts and starts of one step only.
//
//   Windows.  One thread per 64-bit word of the output: it finds the rows the word's 32 bases belong to from the scanned
//   offsets, takes each piece out of two words of the packed reference at its bit offset and, for strand 1, reverses and
//   complements it in the register.  Every word is written once, whole; no atomics.
//
//   No matrix instructions: lookups, a sort and counts of equal keys; nothing is a product.
#include <algorithm>

#include "common.h"

namespace {

constexpr int SD_SMALL_CAP = 1024, SD_LARGE_CAP = BNPK_SEED_MAX_HITS;
constexpr int SD_P_BITS = 10, SD_D_BITS = 31;                  // hit = strand << 41 | (d + 512) << 10 | p'
constexpr int SD_SHIFT = 512;                                  // added to d: the smallest d is -(512 - 8)
static_assert(BNPK_SEED_MAX_LEN <= (1 << SD_P_BITS) && BNPK_SEED_MAX_LEN <= SD_SHIFT, "p' and -d fit their fields");
static_assert(SD_LARGE_CAP <= 4096, "W << 12 | 4095 - t is one 32-bit word");

struct sd_args {
  const uint64_t* reads; const int64_t* off; int64_t n_reads;
  const int64_t* keys; const int64_t* starts; const int32_t* positions; const int32_t* table;
  const int64_t* ref_off; int64_t n_ref_rows;
  int k, max_occ, log_band, min_votes, table_shift;            // table_shift = 2k - T
  int32_t* list; int32_t* count;                               // the reads handed to the large class
  int32_t* votes; int32_t* second; int32_t* strand; int32_t* row; int32_t* position;
  unsigned long long* error;
};

__device__ __forceinline__ void sd_wave_sync() {               // the wavefront's LDS writes before this are seen by its reads after
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the occurrences of h: their number (0: none, or more than max_occ) and where they start in `positions`
__device__ __forceinline__ int sd_lookup(const sd_args& p, uint64_t h, int64_t* first) {
  const uint64_t b = h >> p.table_shift;
  int lo = p.table[b];
  const int end = p.table[b + 1];
  int hi = end;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((uint64_t)p.keys[mid] < h) lo = mid + 1; else hi = mid;
  }
  if (lo >= end || (uint64_t)p.keys[lo] != h) return 0;
  const int64_t s0 = p.starts[lo], occ = p.starts[lo + 1] - s0;
  *first = s0;
  return occ > p.max_occ ? 0 : (int)occ;
}

// W of the run that starts at t, 0 if none starts there.  S[0 .. n) sorted; `shift` takes a word to its (strand, bin)
__device__ __forceinline__ int sd_head_score(const uint64_t* S, int n, int t, int shift, int strand_shift, uint64_t* bin) {
  const uint64_t K = S[t] >> shift;
  *bin = K;
  if (t > 0 && (S[t - 1] >> shift) == K) return 0;
  const uint64_t last = ((K + 1) >> strand_shift) == (K >> strand_shift) ? K + 1 : K;   // bin b + 1, if the strand has one
  int lo = t + 1, hi = n;                                      // first word behind bin `last`
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((S[mid] >> shift) <= last) lo = mid + 1; else hi = mid;
  }
  return lo - t;
}

__global__ void sd_reset_kernel(int32_t* count) {
  if (threadIdx.x == 0) *count = 0;
}

// one wavefront per workgroup.  CAP = SD_SMALL_CAP: every read, the ones with more hits go to p.list; SD_LARGE_CAP: p.list
template <int CAP>
__global__ __launch_bounds__(BNPK_WAVE) void sd_place_kernel(sd_args p) {
  constexpr bool SMALL = CAP == SD_SMALL_CAP;
  __shared__ uint64_t S[CAP];
  BNPK_VGPR_FLOOR_32();
  const int lane = threadIdx.x, k = p.k;
  const uint64_t mask = (1ull << (2 * k)) - 1ull;
  const int bin_shift = SD_P_BITS + p.log_band, strand_shift = SD_D_BITS - p.log_band;
  const int64_t todo = SMALL ? p.n_reads : (int64_t)*p.count;
  for (int64_t slot = blockIdx.x; slot < todo; slot += gridDim.x) {
    const int64_t read = SMALL ? slot : (int64_t)p.list[slot];
    const int64_t base = p.off[read], L = p.off[read + 1] - base;
    const int64_t n = L - k + 1;                               // k-mers of the read
    int votes = 0, second = 0, strand = -1, row = -1, position = 0;
    int n_hits = 0;
    bool defer = false;
    if (L > BNPK_SEED_MAX_LEN || (n > 0 && 2 * n * (int64_t)p.max_occ > BNPK_SEED_MAX_HITS)) {
      if (lane == 0) atomicMin(p.error, (unsigned long long)read);
    } else if (n > 0) {
      sd_wave_sync();                                          // (the read before is done with S)
      for (int c = 0; c < (int)n && !defer; c += BNPK_WAVE) {
        const int q = c + lane;
        int occ0 = 0, occ1 = 0;
        int64_t first0 = 0, first1 = 0;
        if (q < n) {
          const int64_t at = base + q;
          const int sh = 2 * (int)(at & 31);
          uint64_t h = p.reads[at >> 5] >> sh;
          if (sh && 64 - sh < 2 * k) h |= p.reads[(at >> 5) + 1] << (64 - sh);
          h &= mask;
          const uint64_t rc = ~(reverse_2bit_groups(h) >> (64 - 2 * k)) & mask;
          occ0 = sd_lookup(p, h, &first0);
          occ1 = sd_lookup(p, rc, &first1);
        }
        const int mine = occ0 + occ1;
        const int upto = wave_inclusive_scan(mine);
        const int total = __builtin_amdgcn_readlane(upto, 63);
        if (SMALL && n_hits + total > CAP) { defer = true; break; }
        int at = n_hits + upto - mine;
        for (int j = 0; j < occ0; ++j, ++at) {
          const int64_t d = (int64_t)p.positions[first0 + j] - q + SD_SHIFT;
          if (at < CAP) S[at] = ((uint64_t)d << SD_P_BITS) | (uint64_t)q;
        }
        const int qr = (int)n - 1 - q;                         // where the k-mer starts in the read's reverse complement
        for (int j = 0; j < occ1; ++j, ++at) {
          const int64_t d = (int64_t)p.positions[first1 + j] - qr + SD_SHIFT;
          if (at < CAP) S[at] = (1ull << (SD_P_BITS + SD_D_BITS)) | ((uint64_t)d << SD_P_BITS) | (uint64_t)qr;
        }
        n_hits = min(n_hits + total, CAP);                     // (the bound of the interface keeps total within CAP)
      }
      if (defer) {
        if (lane == 0) p.list[atomicAdd(p.count, 1)] = (int32_t)read;
        continue;
      }
      if (n_hits > 0) {
        int P = BNPK_WAVE;
        while (P < n_hits) P <<= 1;
        for (int t = n_hits + lane; t < P; t += BNPK_WAVE) S[t] = ~0ull;
        sd_wave_sync();
        for (int size = 2; size <= P; size <<= 1) {
          for (int j = size >> 1; j > 0; j >>= 1) {
            for (int x = lane; x < P / 2; x += BNPK_WAVE) {
              const int lo = ((x & ~(j - 1)) << 1) | (x & (j - 1)), hi = lo | j;
              const uint64_t a = S[lo], b = S[hi];
              if ((a > b) == ((lo & size) == 0)) { S[lo] = b; S[hi] = a; }
            }
            sd_wave_sync();
          }
        }
        // the winner: the largest W, the first in sorted order among equals
        unsigned best = 0;
        uint64_t bin;
        for (int t = lane; t < n_hits; t += BNPK_WAVE) {
          const int w = sd_head_score(S, n_hits, t, bin_shift, strand_shift, &bin);
          if (w > 0) best = max(best, ((unsigned)w << 12) | (unsigned)(4095 - t));
        }
        best = wave_max(best);
        votes = (int)(best >> 12);
        const uint64_t head = S[4095 - (int)(best & 4095u)];
        const uint64_t wbin = head >> bin_shift;
        unsigned runner = 0;
        for (int t = lane; t < n_hits; t += BNPK_WAVE) {
          const int w = sd_head_score(S, n_hits, t, bin_shift, strand_shift, &bin);
          const bool near = (bin >> strand_shift) == (wbin >> strand_shift) && bin + 1 >= wbin && bin <= wbin + 1;
          if (!near) runner = max(runner, (unsigned)w);
        }
        second = (int)wave_max(runner);
        if (votes >= p.min_votes) {
          strand = (int)(head >> (SD_P_BITS + SD_D_BITS));
          const int64_t D = (int64_t)((head >> SD_P_BITS) & ((1ull << SD_D_BITS) - 1ull)) - SD_SHIFT;
          const int64_t g = D + (int64_t)(head & ((1ull << SD_P_BITS) - 1ull));
          const int64_t r = find_row(p.ref_off, 0, p.n_ref_rows - 1, g);
          row = (int)r;
          position = (int)(D - p.ref_off[r]);
        }
      }
    }
    if (lane == 0) {
      p.votes[read] = votes;
      p.second[read] = second;
      p.strand[read] = strand;
      p.row[read] = row;
      p.position[read] = position;
    }
  }
}

// the global coordinate of every k-mer of the rows: in_off[r] + (j - out_off[r]) for the k-mer j of row r
__global__ __launch_bounds__(BNPK_BLOCK) void sd_positions_kernel(const int64_t* __restrict__ in_off, const int64_t* __restrict__ out_off,
                                                                 int64_t n_rows, int64_t n, int64_t* __restrict__ out) {
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = find_row(out_off, 0, n_rows - 1, j);
    out[j] = in_off[r] + (j - out_off[r]);
  }
}

// positions as int32, and table[b] = the first key whose top bits are >= b (b = 0 .. 2^T): a key writes the entries
// between its predecessor's bucket and its own, the last key also those behind it
__global__ __launch_bounds__(BNPK_BLOCK) void sd_finish_kernel(const int64_t* __restrict__ keys, int64_t n_keys, const int64_t* __restrict__ pos64,
                                                              int64_t n, int shift, int64_t buckets, int32_t* __restrict__ positions,
                                                              int32_t* __restrict__ table) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, me = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t j = me; j < n; j += stride) positions[j] = (int32_t)pos64[j];
  for (int64_t u = me; u < n_keys; u += stride) {
    const int64_t b = (int64_t)((uint64_t)keys[u] >> shift), before = u ? (int64_t)((uint64_t)keys[u - 1] >> shift) : -1;
    for (int64_t x = before + 1; x <= b; ++x) table[x] = (int32_t)u;
    if (u == n_keys - 1)
      for (int64_t x = b + 1; x <= buckets; ++x) table[x] = (int32_t)n_keys;
  }
  if (n_keys == 0)
    for (int64_t x = me; x <= buckets; x += stride) table[x] = 0;
}

__global__ __launch_bounds__(BNPK_BLOCK) void sd_window_lengths_kernel(const int32_t* __restrict__ strand, const int32_t* __restrict__ row,
                                                                      const int32_t* __restrict__ position, const int64_t* __restrict__ off,
                                                                      const int64_t* __restrict__ ref_off, int64_t n_ref_rows, int64_t n_reads,
                                                                      int64_t pad, int64_t* __restrict__ lengths, int32_t* __restrict__ start) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_reads; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t a = 0, len = 0;
    const int64_t r = row[i];
    if (strand[i] >= 0 && r >= 0 && r < n_ref_rows) {
      const int64_t row_len = ref_off[r + 1] - ref_off[r], at = position[i];
      a = std::max<int64_t>(0, at - pad);
      const int64_t b = std::min<int64_t>(row_len, at + (off[i + 1] - off[i]) + pad);
      len = b > a ? b - a : 0;
    }
    lengths[i] = len;
    start[i] = (int32_t)a;
  }
}

// `count` bases (1 .. 32) of the packed layout from base `at` on
__device__ __forceinline__ uint64_t sd_bases(const uint64_t* __restrict__ words, int64_t at, int count) {
  const int sh = 2 * (int)(at & 31);
  uint64_t x = words[at >> 5] >> sh;
  if (sh && 64 - sh < 2 * count) x |= words[(at >> 5) + 1] << (64 - sh);
  return count == 32 ? x : x & ((1ull << (2 * count)) - 1ull);
}

__global__ __launch_bounds__(BNPK_BLOCK) void sd_windows_kernel(const uint64_t* __restrict__ ref, const int64_t* __restrict__ ref_off,
                                                               const int32_t* __restrict__ strand, const int32_t* __restrict__ row,
                                                               const int32_t* __restrict__ start, const int64_t* __restrict__ out_off,
                                                               int64_t n_reads, int64_t total, uint64_t* __restrict__ out) {
  BNPK_VGPR_FLOOR_32();
  const int64_t n_words = total / 32 + 2;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < n_words; w += (int64_t)gridDim.x * blockDim.x) {
    uint64_t word = 0;
    const int64_t end = std::min<int64_t>(total, 32 * w + 32);
    int64_t x = 32 * w, i = 0;
    while (x < end) {
      i = find_row(out_off, i, n_reads - 1, x);                // the non-empty window that holds x
      const int64_t lo = out_off[i], hi = out_off[i + 1], stop = std::min<int64_t>(end, hi);
      const int count = (int)(stop - x);
      const int64_t from = ref_off[row[i]] + start[i];         // the window's first base in the reference
      uint64_t piece;
      if (strand[i] == 0) {
        piece = sd_bases(ref, from + (x - lo), count);
      } else {                                                 // window position j is the complement of base len - 1 - j
        const uint64_t fwd = sd_bases(ref, from + (hi - stop), count);
        piece = ~(reverse_2bit_groups(fwd) >> (64 - 2 * count));
        if (count < 32) piece &= (1ull << (2 * count)) - 1ull;
      }
      word |= piece << (2 * (int)(x & 31));
      x = stop;
    }
    out[w] = word;
  }
}

template <int CAP>
static int sd_launch(bnpk_ctx* ctx, const sd_args& a, int64_t most, hipStream_t s) {
  // as many wavefronts as the card holds at once, the LDS of a workgroup permitting; the kernel strides over its reads
  const int64_t per_cu = std::min<int64_t>(32, (160 * 1024) / (CAP * 8));
  hipLaunchKernelGGL(sd_place_kernel<CAP>, dim3(grid_for(std::min<int64_t>(most, ctx->compute_units * per_cu))), dim3(BNPK_WAVE), 0, s, a);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

static bool sd_k_ok(int k) { return k >= BNPK_SEED_MIN_K && k <= BNPK_SEED_MAX_K; }

}  // namespace

extern "C" {

int bnpk_seed_table_bits(int64_t n_keys, int k) {
  int bits = 0;
  while (bits < 40 && (n_keys >> bits) > 8) ++bits;            // ~8 keys to a bucket
  return std::max(1, std::min(bits, std::min(2 * k, BNPK_SEED_MAX_TABLE_BITS)));
}

int bnpk_seed_index_positions(bnpk_ctx* ctx, const int64_t* d_in_offsets, const int64_t* d_out_offsets, int64_t n_rows, int64_t n,
                              int64_t* d_positions, void* stream) {
  if (!ctx || n_rows < 0 || n < 0 || (n > 0 && (!d_in_offsets || !d_out_offsets || !d_positions || n_rows < 1))) return BNPK_ERR_ARG;
  if (n == 0) return BNPK_OK;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "seed_index_positions", s);
  hipLaunchKernelGGL(sd_positions_kernel, dim3(grid_for(ceil_div(n, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_in_offsets, d_out_offsets,
                     n_rows, n, d_positions);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_seed_index_finish(bnpk_ctx* ctx, const int64_t* d_keys, int64_t n_keys, const int64_t* d_positions64, int64_t n, int k,
                           int table_bits, int32_t* d_positions, int32_t* d_table, void* stream) {
  if (!ctx || !sd_k_ok(k) || table_bits < 1 || table_bits > std::min(2 * k, BNPK_SEED_MAX_TABLE_BITS) || n_keys < 0 || n < n_keys ||
      n > INT32_MAX || !d_table || (n > 0 && (!d_keys || !d_positions64 || !d_positions)))
    return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "seed_index_finish", s);
  hipLaunchKernelGGL(sd_finish_kernel, dim3(grid_for(ceil_div(std::max<int64_t>(n, (int64_t)1 << table_bits), BNPK_BLOCK))), dim3(BNPK_BLOCK),
                     0, s, d_keys, n_keys, d_positions64, n, 2 * k - table_bits, (int64_t)1 << table_bits, d_positions, d_table);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_seed_place_packed(bnpk_ctx* ctx, const bnpk_seed_params* h, const uint64_t* d_packed, int64_t n_bases, const int64_t* d_offsets,
                           int64_t n_reads, const int64_t* d_keys, int64_t n_keys, const int64_t* d_starts, const int32_t* d_positions,
                           const int32_t* d_table, const int64_t* d_ref_offsets, int64_t n_ref_rows, int32_t* d_votes, int32_t* d_second,
                           int32_t* d_strand, int32_t* d_row, int32_t* d_position, int64_t* d_error, void* stream) {
  if (!ctx || !h || n_bases < 0 || n_reads < 0 || n_reads > INT32_MAX || n_keys < 0 || n_ref_rows < 0) return BNPK_ERR_ARG;
  if (!sd_k_ok(h->k) || h->max_occurrences < 1 || h->max_occurrences > BNPK_SEED_MAX_OCCURRENCES || h->min_votes < 1) return BNPK_ERR_ARG;
  if (h->band < 1 || h->band > BNPK_SEED_MAX_BAND || (h->band & (h->band - 1))) return BNPK_ERR_ARG;
  if (h->table_bits < 1 || h->table_bits > std::min(2 * h->k, BNPK_SEED_MAX_TABLE_BITS)) return BNPK_ERR_ARG;
  if (n_reads > 0 && (!d_offsets || !d_table || !d_votes || !d_second || !d_strand || !d_row || !d_position || !d_error ||
                      (n_bases > 0 && !d_packed) || (n_keys > 0 && (!d_keys || !d_starts || !d_positions || !d_ref_offsets || n_ref_rows < 1))))
    return BNPK_ERR_ARG;
  if (n_reads == 0) return BNPK_OK;
  hipStream_t s = (hipStream_t)stream;
  sd_args a = {};
  a.reads = d_packed; a.off = d_offsets; a.n_reads = n_reads;
  a.keys = d_keys; a.starts = d_starts; a.positions = d_positions; a.table = d_table;
  a.ref_off = d_ref_offsets; a.n_ref_rows = n_ref_rows;
  a.k = h->k; a.max_occ = h->max_occurrences; a.min_votes = h->min_votes; a.table_shift = 2 * h->k - h->table_bits;
  while ((1 << a.log_band) < h->band) ++a.log_band;
  void* scratch = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, 16 + (size_t)n_reads * 4, &scratch, s));
  a.count = (int32_t*)scratch;
  a.list = a.count + 4;
  a.votes = d_votes; a.second = d_second; a.strand = d_strand; a.row = d_row; a.position = d_position;
  a.error = (unsigned long long*)d_error;
  bnpk_timer t(ctx, "seed_place_packed", s);
  hipLaunchKernelGGL(sd_reset_kernel, dim3(1), dim3(BNPK_WAVE), 0, s, a.count);
  BNPK_CHECK(sd_launch<SD_SMALL_CAP>(ctx, a, n_reads, s));
  return sd_launch<SD_LARGE_CAP>(ctx, a, n_reads, s);
}

int bnpk_seed_window_lengths(bnpk_ctx* ctx, const int32_t* d_strand, const int32_t* d_row, const int32_t* d_position,
                             const int64_t* d_offsets, const int64_t* d_ref_offsets, int64_t n_ref_rows, int64_t n_reads, int64_t pad,
                             int64_t* d_lengths, int32_t* d_start, void* stream) {
  if (!ctx || n_reads < 0 || n_ref_rows < 0 || pad < 0 || pad > INT32_MAX) return BNPK_ERR_ARG;
  if (n_reads > 0 && (!d_strand || !d_row || !d_position || !d_offsets || !d_ref_offsets || !d_lengths || !d_start)) return BNPK_ERR_ARG;
  if (n_reads == 0) return BNPK_OK;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "seed_window_lengths", s);
  hipLaunchKernelGGL(sd_window_lengths_kernel, dim3(grid_for(ceil_div(n_reads, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_strand, d_row,
                     d_position, d_offsets, d_ref_offsets, n_ref_rows, n_reads, pad, d_lengths, d_start);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_seed_windows_packed(bnpk_ctx* ctx, const uint64_t* d_ref_packed, const int64_t* d_ref_offsets, const int32_t* d_strand,
                             const int32_t* d_row, const int32_t* d_start, const int64_t* d_out_offsets, int64_t n_reads, int64_t total,
                             uint64_t* d_out, void* stream) {
  if (!ctx || n_reads < 0 || total < 0 || !d_out) return BNPK_ERR_ARG;
  if (total > 0 && (!d_ref_packed || !d_ref_offsets || !d_strand || !d_row || !d_start || !d_out_offsets || n_reads < 1)) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "seed_windows_packed", s);
  hipLaunchKernelGGL(sd_windows_kernel, dim3(grid_for(ceil_div(total / 32 + 2, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_ref_packed,
                     d_ref_offsets, d_strand, d_row, d_start, d_out_offsets, n_reads, total, d_out);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
