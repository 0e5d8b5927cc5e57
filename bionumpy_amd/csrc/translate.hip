// DNA -> protein translation of ragged rows (bionumpy/sequence/translate.py), gfx950.
//
//   Row r of L_r bases gives P_r = max(0, L_r - frame) / 3 amino-acid letters, written as one compact ASCII column
//   (out_offsets = exclusive scan of P_r).  Forward strand: codon j = bases frame + 3j .. frame + 3j + 2.  Reverse strand:
//   codon j = codon j of the row's reverse complement = bases L - 1 - frame - 3j down to L - 3 - frame - 3j, complemented.
//   The frame's leading bases and the 1-2 bases behind the last codon are never looked at — in the text form that
//   includes the validity check: only bytes inside translated codons are examined.
//
//   The table is prepared, not the data.  The caller's 64 letters are indexed 16 c0 + 4 c1 + c2 with T C A G = 0 1 2 3
//   (translate.py:13-14).  The host derives one 64-byte table per (input form, strand) that is indexed with the six raw
//   bits the kernel finds: 2 bits per base in the input's own code (packed: A C G T = 0 1 2 3; text: (byte >> 1) & 3, i.e.
//   A C T G = 0 1 2 3 in both letter cases), the base at the LOWER address in the lower bits.  For the reverse strand
//   the derived table also holds the complement and the reversed base order, so the loop spends no instruction on
//   either: the strands differ only in the direction in which a lane walks its 96 bits.
//
//   A lane owns 16 output letters = 16 codons = 96 bits of 2-bit codes; a workgroup 4096 letters (a tile), made from
//   ~3 KB of packed words or 12 KB of text.  The rows of a tile come from the rows.h tile -> row table over the OUTPUT
//   offsets; their output / input offsets (and row starts, for text that was never gathered) are staged in LDS.
#include "common.h"
#include "rows.h"

namespace {

typedef unsigned __int128 u128;

constexpr int TR_LPL = 16;                                   // letters (codons) per lane
constexpr int64_t TR_TILE = (int64_t)BNPK_BLOCK * TR_LPL;    // letters per tile
constexpr int TR_LDS_ROWS = 510;                             // rows of a tile whose offsets are staged (reads of 24 bases and more)
constexpr int TR_SRC_WORDS = 400;                            // packed words of the tile's rows that are staged (12 800 bases: a tile and a read on either side)

struct tr_table { uint32_t w[16]; };                         // the derived 64-byte table, passed by value

// ---- the derived tables (host) ----------------------------------------------------------------------------------
// code_to_tcag: the input's 2-bit code -> the base's rank in T C A G; comp: the code of the complement
static void derive_table(const uint8_t* table64, const int* code_to_tcag, const int* comp, int reverse, tr_table* out) {
  uint8_t t[64];
  for (int g = 0; g < 64; ++g) {
    const int lo = g & 3, mid = (g >> 2) & 3, hi = (g >> 4) & 3;        // lo = the base at the lowest address
    const int c0 = reverse ? comp[hi] : lo, c1 = reverse ? comp[mid] : mid, c2 = reverse ? comp[lo] : hi;
    t[g] = table64[16 * code_to_tcag[c0] + 4 * code_to_tcag[c1] + code_to_tcag[c2]];
  }
  memcpy(out->w, t, 64);
}
static const int PACKED_TO_TCAG[4] = {2, 1, 3, 0}, PACKED_COMP[4] = {3, 2, 1, 0};   // A C G T
static const int TEXT_TO_TCAG[4] = {2, 1, 0, 3}, TEXT_COMP[4] = {2, 3, 0, 1};       // A C T G

// ---- what a lane accumulates ---------------------------------------------------------------------------------------
// bits: the 6-bit groups of the lane's codons — forward: letter m at bit 6m; reverse: letter m at bit 6 (15 - m) once
// finish() has run.  bad: one bit per LETTER whose codon holds a byte that is no A C G T (text form), err: the smallest
// flat offset of such a byte.
template <bool REV>
struct tr_acc {
  u128 bits = 0;
  uint32_t bad = 0;
  int done = 0;
  int64_t err = INT64_MAX;
  // n codons that lie at increasing addresses in the low 6n bits of `piece`; bad48: one bit per byte of them, flat0: the
  // flat offset of their first byte
  __device__ __forceinline__ void add(u128 piece, int n, uint64_t bad48 = 0, int64_t flat0 = 0) {
    if (REV) bits = (bits << (6 * n)) | piece;
    else bits |= piece << (6 * done);
    if (bad48) {                                             // rare
      for (int k = 0; k < n; ++k)
        if ((bad48 >> (3 * k)) & 7u) bad |= 1u << (REV ? done + n - 1 - k : done + k);
      err = min(err, flat0 + (int64_t)__builtin_ctzll(bad48));
    }
    done += n;
  }
  __device__ __forceinline__ void finish() {
    if (REV && done < TR_LPL) bits <<= 6 * (TR_LPL - done);   // (the last lane of the output)
  }
};

__device__ __forceinline__ u128 low_groups(u128 v, int n) { return v & ((((u128)1) << (6 * n)) - 1); }

// the lane's letters: sixteen look-ups in the 64-byte LDS table (sixteen banks, so lanes never conflict)
template <bool REV>
__device__ __forceinline__ void tr_lookup(const uint8_t* __restrict__ stab, u128 bits, uint32_t w[4]) {
  const uint64_t lo = (uint64_t)bits;
  const uint32_t hi = (uint32_t)(bits >> 64);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int m = 4 * q + b, at = 6 * (REV ? TR_LPL - 1 - m : m);
      uint32_t g;
      if (at + 6 <= 64) g = (uint32_t)(lo >> at);
      else if (at >= 64) g = hi >> (at - 64);
      else g = (uint32_t)(lo >> at) | (hi << (64 - at));
      word |= (uint32_t)stab[g & 63u] << (8 * b);
    }
    w[q] = word;
  }
}

__device__ __forceinline__ void tr_store(uint8_t* __restrict__ out, int64_t q0, int n, const uint32_t w[4]) {
  if (n == TR_LPL) {                                         // (q0 is a multiple of 16; so is the buffer's address)
    *reinterpret_cast<uint4*>(out + q0) = make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    for (int j = 0; j < n; ++j) out[q0 + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
  }
}

// The rows of a tile.  ooff / ioff: output (letters) and input (bases) offsets of the rows; staged: rows lo .. hi + 1 of
// both are in LDS.  A tile of more rows than fit searches global memory.
struct tr_rows {
  const int64_t* __restrict__ ooff;
  const int64_t* __restrict__ ioff;
  const int64_t* so;
  const int64_t* si;
  int64_t lo, hi;
  bool staged;
  __device__ __forceinline__ int64_t o(int64_t row) const { return (staged && row <= hi + 1) ? so[row - lo] : ooff[row]; }
  __device__ __forceinline__ int64_t i(int64_t row) const { return (staged && row <= hi + 1) ? si[row - lo] : ioff[row]; }
  // last row in [lo, hi] whose letters start at or before q
  __device__ __forceinline__ int64_t find(int64_t q) const {
    if (!staged) return find_row(ooff, lo, hi, q);
    int a = 0, b = (int)(hi - lo);
    while (a < b) {
      const int mid = a + ((b - a + 1) >> 1);
      if (so[mid] <= q) a = mid; else b = mid - 1;
    }
    return lo + a;
  }
};

// where the n codons j .. j + n - 1 of row `row` begin, as a flat base position (they are 3n consecutive bases on either strand)
template <bool REV>
__device__ __forceinline__ int64_t codons_at(const tr_rows& R, int64_t row, int64_t j, int n, int frame) {
  return REV ? R.i(row + 1) - frame - 3 * (j + n) : R.i(row) + frame + 3 * j;
}

// The lane's letters [q0, q1) gathered piece by piece: one piece where they lie in one row; two — fetched without waiting
// for each other — where they lie in the end of a row and the start of the next (reads are longer than 48 bases); rows
// shorter than that, and empty rows, are walked.  fetch2(row_a, pos_a, n_a, row_b, pos_b, n_b, acc): adds the n_a codons of
// row_a at flat base position pos_a and, if n_b, the n_b codons of row_b at pos_b.
template <bool REV, class F>
__device__ __forceinline__ void tr_gather(const tr_rows& R, int64_t n_rows, int64_t q0, int64_t q1, int frame, tr_acc<REV>& acc,
                                          F fetch2) {
  const int64_t r = R.find(q0);
  const int64_t o0 = R.o(r), o1 = R.o(r + 1);                 // (o1 > q0: r is the LAST row that starts at or before q0)
  const int n_a = (int)(min(o1, q1) - q0);
  const int64_t o2 = (q0 + n_a < q1 && r + 2 <= n_rows) ? R.o(r + 2) : o1;
  const int n_b = (int)(min(o2, q1) - o1);
  if (q0 + n_a == q1) {
    fetch2(r, codons_at<REV>(R, r, q0 - o0, n_a, frame), n_a, r, 0, 0, acc);
  } else if (n_b > 0 && o1 + n_b == q1) {
    fetch2(r, codons_at<REV>(R, r, q0 - o0, n_a, frame), n_a, r + 1, codons_at<REV>(R, r + 1, 0, n_b, frame), n_b, acc);
  } else {
    int64_t p = q0, row = r, os = o0, oe = o1;
    while (p < q1) {
      while (oe <= p) { ++row; os = oe; oe = R.o(row + 1); }
      const int n = (int)(min(oe, q1) - p);
      fetch2(row, codons_at<REV>(R, row, p - os, n, frame), n, row, 0, 0, acc);
      p += n;
    }
  }
  acc.finish();
}

// stage the offsets of the tile's rows (and the table); true if they fit
__device__ __forceinline__ bool tr_stage(const tr_table& t, uint32_t* stab, const int64_t* __restrict__ ooff,
                                         const int64_t* __restrict__ ioff, const int64_t* __restrict__ starts, int64_t n_rows,
                                         int64_t lo, int64_t hi, int64_t* so, int64_t* si, int64_t* ss) {
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 16; ++k) stab[k] = t.w[k];
  }
  const bool staged = hi - lo + 2 <= TR_LDS_ROWS + 2;         // (uniform) offsets lo .. hi + 1
  if (staged) {
    for (int64_t i = threadIdx.x; i <= hi - lo + 1; i += BNPK_BLOCK) {
      so[i] = ooff[lo + i];
      si[i] = ioff[lo + i];
      if (starts && lo + i < n_rows) ss[i] = starts[lo + i];
    }
  }
  __syncthreads();
  return staged;
}

// ---- 2-bit input ---------------------------------------------------------------------------------------------------------
// 3n <= 48 bases from flat position pos of the packed stream: the 96 bits are funnel-shifted out of three words
template <class W>
__device__ __forceinline__ u128 packed_bits(W word, int64_t pos, int n) {
  const int64_t i = pos >> 5;
  const int sh = 2 * (int)(pos & 31);
  const uint64_t a = word(i), b = word(i + 1), c = word(i + 2);
  u128 v = ((((u128)b) << 64) | a) >> sh;
  if (sh) v |= ((u128)c) << (128 - sh);
  return low_groups(v, n);
}

template <bool REV>
__global__ __launch_bounds__(BNPK_BLOCK) void tr_packed_kernel(const uint64_t* __restrict__ in, int64_t n_words,
                                                               const int64_t* __restrict__ ioff,
                                                               const int64_t* __restrict__ ooff, int64_t n_rows, int64_t n_out,
                                                               const int64_t* __restrict__ tile_rows, int64_t n_tiles,
                                                               tr_table table, int frame, uint8_t* __restrict__ out) {
  __shared__ int64_t so[TR_LDS_ROWS + 2], si[TR_LDS_ROWS + 2];
  __shared__ uint64_t ssrc[TR_SRC_WORDS + 2];
  __shared__ uint32_t stab[16];
  tr_rows R;
  R.ooff = ooff; R.ioff = ioff; R.so = so; R.si = si;
  tile_row_range(tile_rows, blockIdx.x, n_tiles, n_rows, R.lo, R.hi);
  R.staged = tr_stage(table, stab, ooff, ioff, nullptr, n_rows, R.lo, R.hi, so, si, nullptr);
  // The bases the tile's letters are made of are the tile's own rows: for reads, the tile's stretch of the packed stream and a
  // read on either side.  It comes into LDS with coalesced loads and every lane cuts its 96 bits out of LDS at whatever bit
  // offset they start.  Rows much longer than a tile (a chromosome) are read from global memory.
  int64_t word0 = 0;
  bool src_staged = false;                                   // (uniform)
  if (R.staged) {
    const int64_t first = si[0] >> 5, last = (si[R.hi - R.lo + 1] + 31) >> 5;      // words [first, last) hold the rows lo .. hi
    if (last - first <= TR_SRC_WORDS) {
      src_staged = true;
      word0 = first;
      for (int64_t i = threadIdx.x; i < last - first + 2; i += BNPK_BLOCK) ssrc[i] = first + i < n_words ? in[first + i] : 0ull;
      __syncthreads();
    }
  }
  const int64_t q0 = ((int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x) * TR_LPL;
  if (q0 >= n_out) return;
  const int64_t q1 = min(q0 + TR_LPL, n_out);
  tr_acc<REV> acc;
  auto from_lds = [&](int64_t i) { return ssrc[(int)(i - word0)]; };
  auto from_global = [&](int64_t i) { return i < n_words ? in[i] : 0ull; };
  auto fetch2 = [&](int64_t, int64_t pos_a, int n_a, int64_t, int64_t pos_b, int n_b, tr_acc<REV>& A) {
    u128 a, b = 0;
    if (src_staged) {
      a = packed_bits(from_lds, pos_a, n_a);
      if (n_b) b = packed_bits(from_lds, pos_b, n_b);
    } else {
      a = packed_bits(from_global, pos_a, n_a);
      if (n_b) b = packed_bits(from_global, pos_b, n_b);
    }
    A.add(a, n_a);
    if (n_b) A.add(b, n_b);
  };
  tr_gather<REV>(R, n_rows, q0, q1, frame, acc, fetch2);
  uint32_t w[4];
  tr_lookup<REV>((const uint8_t*)stab, acc.bits, w);
  tr_store(out, q0, (int)(q1 - q0), w);
}

// ---- text input -------------------------------------------------------------------------------------------------------------
// Four letters -> eight bits: (x >> 1) & 3 separates A C T G (0 1 2 3) in both cases, one multiply closes the four 2-bit fields
// up (the partial products land on distinct bits: no carries).  z: the bytes that are not the letter their two bits promise,
// i.e. anything but A C G T a c g t, are non-zero.
__device__ __forceinline__ uint32_t text_codes4(uint32_t x, uint32_t& z) {
  const uint32_t y = (x >> 1) & 0x03030303u;
  z = (x & 0xdfdfdfdfu) ^ __builtin_amdgcn_perm(0u, 0x47544341u, y);                // G T C A
  return (y * 0x01041040u) >> 24;
}

// the 3n <= 48 bytes at p: their 2-bit codes in the low 6n bits, and one bit per byte that is no A C G T in bad48.  Forty-eight
// bytes are loaded whenever the buffer has them (what lies behind the 3n is cut off); at the buffer's end, byte by byte.
__device__ __forceinline__ u128 text_bits(const uint8_t* __restrict__ in, int64_t in_size, int64_t p, int n, uint64_t& bad48) {
  uint32_t c[3] = {0, 0, 0};
  bad48 = 0;
  if (p >= 0 && p + 3 * TR_LPL <= in_size) {
    uint32_t x[12], z[12], zor = 0;
    __builtin_memcpy(x, in + p, 48);
#pragma unroll
    for (int q = 0; q < 12; ++q) {
      c[q >> 2] |= text_codes4(x[q], z[q]) << (8 * (q & 3));
      zor |= z[q];
    }
    if (zor) {                                               // a byte that is no base, in the codons or behind them
      const uint64_t f0 = nomatch16(z[0], z[1], z[2], z[3], 0u), f1 = nomatch16(z[4], z[5], z[6], z[7], 0u),
                     f2 = nomatch16(z[8], z[9], z[10], z[11], 0u);
      bad48 = (f0 | (f1 << 16) | (f2 << 32)) & ((1ull << (3 * n)) - 1ull);
    }
  } else {
    for (int k = 0; k < 3 * n; ++k) {
      uint32_t z;
      c[k >> 4] |= text_codes4(in[p + k], z) << (2 * (k & 15));
      if (z & 0xffu) bad48 |= 1ull << k;
    }
  }
  return low_groups((((u128)c[2]) << 64) | (((u128)c[1]) << 32) | c[0], n);
}

// in_starts (optional): the rows were never gathered — row r lies at in[in_starts[r] ..) in a buffer of in_size bytes.
// unknown == 0: the smallest flat offset (position in the concatenated rows) of a byte that is no base, inside a translated
// codon, goes to err_cell; otherwise the codon's letter is `unknown`.
template <bool REV>
__global__ __launch_bounds__(BNPK_BLOCK) void tr_bytes_kernel(const uint8_t* __restrict__ in, int64_t in_size,
                                                              const int64_t* __restrict__ in_starts,
                                                              const int64_t* __restrict__ ioff,
                                                              const int64_t* __restrict__ ooff, int64_t n_rows, int64_t n_out,
                                                              const int64_t* __restrict__ tile_rows, int64_t n_tiles,
                                                              tr_table table, int frame, uint32_t unknown,
                                                              int64_t* __restrict__ err_cell, uint8_t* __restrict__ out) {
  __shared__ int64_t so[TR_LDS_ROWS + 2], si[TR_LDS_ROWS + 2], ss[TR_LDS_ROWS + 2];
  __shared__ uint32_t stab[16];
  tr_rows R;
  R.ooff = ooff; R.ioff = ioff; R.so = so; R.si = si;
  tile_row_range(tile_rows, blockIdx.x, n_tiles, n_rows, R.lo, R.hi);
  R.staged = tr_stage(table, stab, ooff, ioff, in_starts, n_rows, R.lo, R.hi, so, si, ss);
  const int64_t q0 = ((int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x) * TR_LPL;
  if (q0 >= n_out) return;
  const int64_t q1 = min(q0 + TR_LPL, n_out);
  // flat base position -> address: rows that were gathered lie at their flat positions
  auto address = [&](int64_t row, int64_t pos) {
    if (!in_starts) return pos;
    return ((R.staged && row <= R.hi) ? ss[row - R.lo] : in_starts[row]) + (pos - R.i(row));
  };
  tr_acc<REV> acc;
  auto fetch2 = [&](int64_t row_a, int64_t pos_a, int n_a, int64_t row_b, int64_t pos_b, int n_b, tr_acc<REV>& A) {
    uint64_t bad_a, bad_b = 0;
    u128 b = 0;
    const u128 a = text_bits(in, in_size, address(row_a, pos_a), n_a, bad_a);
    if (n_b) b = text_bits(in, in_size, address(row_b, pos_b), n_b, bad_b);
    A.add(a, n_a, bad_a, pos_a);
    if (n_b) A.add(b, n_b, bad_b, pos_b);
  };
  tr_gather<REV>(R, n_rows, q0, q1, frame, acc, fetch2);
  uint32_t w[4];
  tr_lookup<REV>((const uint8_t*)stab, acc.bits, w);
  if (acc.bad) {                                             // rare
    if (unknown) {
      for (int m = 0; m < TR_LPL; ++m)
        if ((acc.bad >> m) & 1u) w[m >> 2] = (w[m >> 2] & ~(0xffu << (8 * (m & 3)))) | (unknown << (8 * (m & 3)));
    } else {
      atomicMin((unsigned long long*)err_cell, (unsigned long long)acc.err);
    }
  }
  tr_store(out, q0, (int)(q1 - q0), w);
}

// ---- the plan: letters per row, and the rows that do not end on a codon -----------------------------------------------------------
__global__ void tr_plan_zero_kernel(int64_t* __restrict__ cell) { *cell = 0; }

__global__ __launch_bounds__(BNPK_BLOCK) void tr_plan_kernel(const int64_t* __restrict__ ioff, int64_t n_rows, int frame,
                                                             int64_t* __restrict__ out_lens, int64_t* __restrict__ partial_rows) {
  int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  unsigned partial = 0;
  for (; r < n_rows; r += stride) {
    const int64_t rest = ioff[r + 1] - ioff[r] - frame;
    out_lens[r] = rest > 0 ? rest / 3 : 0;
    partial += rest % 3 != 0;
  }
  partial = wave_reduce_sum(partial);
  if (lane_id() == 0 && partial) atomicAdd((unsigned long long*)partial_rows, (unsigned long long)partial);
}

static int check_common(bnpk_ctx* ctx, const void* d_in_offsets, int64_t n_rows, int64_t total, const void* d_out_offsets,
                        int64_t n_out, const uint8_t* table64, int frame, int reverse) {
  if (!ctx || n_rows < 0 || total < 0 || n_out < 0 || !d_in_offsets || !d_out_offsets || !table64 || frame < 0 || frame > 2 ||
      reverse < 0 || reverse > 1)
    return BNPK_ERR_ARG;
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_translate_plan(bnpk_ctx* ctx, const int64_t* d_in_offsets, int64_t n_rows, int frame, int64_t* d_out_lens,
                        int64_t* d_partial_rows, void* stream) {
  if (!ctx || n_rows < 0 || frame < 0 || frame > 2 || !d_in_offsets || !d_partial_rows || (n_rows > 0 && !d_out_lens))
    return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tr_plan_zero_kernel, dim3(1), dim3(1), 0, s, d_partial_rows);
  if (n_rows > 0)
    hipLaunchKernelGGL(tr_plan_kernel, dim3(grid_for(ceil_div(n_rows, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_in_offsets, n_rows,
                       frame, d_out_lens, d_partial_rows);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_translate_packed(bnpk_ctx* ctx, const uint64_t* d_packed, const int64_t* d_in_offsets, int64_t n_rows, int64_t total,
                          const int64_t* d_out_offsets, int64_t n_out, const uint8_t* table64, int frame, int reverse,
                          uint8_t* d_out, void* stream) {
  BNPK_CHECK(check_common(ctx, d_in_offsets, n_rows, total, d_out_offsets, n_out, table64, frame, reverse));
  if (d_out && (const void*)d_out == (const void*)d_packed) return BNPK_ERR_ARG;
  if (n_rows == 0 || n_out == 0) return BNPK_OK;
  if (!d_packed || !d_out) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = ceil_div(n_out, TR_TILE);
  if (n_tiles > BNPK_MAX_BLOCKS) return BNPK_ERR_RANGE;
  void* rows = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, tile_rows_bytes(n_tiles), &rows, s));
  tr_table t;
  derive_table(table64, PACKED_TO_TCAG, PACKED_COMP, reverse, &t);
  bnpk_timer timer(ctx, "translate_packed", s);
  BNPK_CHECK(build_tile_rows(ctx, d_out_offsets, n_rows, TR_TILE, (int64_t*)rows, s));
  const int64_t n_words = total / 32 + 2;                    // the packed layout of bnpk_gather_encode_dna
  if (reverse)
    hipLaunchKernelGGL(tr_packed_kernel<true>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_packed, n_words, d_in_offsets,
                       d_out_offsets, n_rows, n_out, (const int64_t*)rows, n_tiles, t, frame, d_out);
  else
    hipLaunchKernelGGL(tr_packed_kernel<false>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_packed, n_words, d_in_offsets,
                       d_out_offsets, n_rows, n_out, (const int64_t*)rows, n_tiles, t, frame, d_out);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_translate_rows(bnpk_ctx* ctx, const uint8_t* d_bytes, int64_t in_size, const int64_t* d_in_starts,
                        const int64_t* d_in_offsets, int64_t n_rows, int64_t total, const int64_t* d_out_offsets, int64_t n_out,
                        const uint8_t* table64, int frame, int reverse, uint8_t unknown, int64_t* d_err_cell, uint8_t* d_out,
                        void* stream) {
  BNPK_CHECK(check_common(ctx, d_in_offsets, n_rows, total, d_out_offsets, n_out, table64, frame, reverse));
  if (in_size < 0 || (!unknown && !d_err_cell) || (d_out && d_out == d_bytes)) return BNPK_ERR_ARG;
  if (n_rows == 0 || n_out == 0) return BNPK_OK;
  if (!d_bytes || !d_out) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = ceil_div(n_out, TR_TILE);
  if (n_tiles > BNPK_MAX_BLOCKS) return BNPK_ERR_RANGE;
  void* rows = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, tile_rows_bytes(n_tiles), &rows, s));
  tr_table t;
  derive_table(table64, TEXT_TO_TCAG, TEXT_COMP, reverse, &t);
  bnpk_timer timer(ctx, "translate_bytes", s);
  BNPK_CHECK(build_tile_rows(ctx, d_out_offsets, n_rows, TR_TILE, (int64_t*)rows, s));
  if (reverse)
    hipLaunchKernelGGL(tr_bytes_kernel<true>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_bytes, in_size, d_in_starts,
                       d_in_offsets, d_out_offsets, n_rows, n_out, (const int64_t*)rows, n_tiles, t, frame, (uint32_t)unknown,
                       d_err_cell, d_out);
  else
    hipLaunchKernelGGL(tr_bytes_kernel<false>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_bytes, in_size, d_in_starts,
                       d_in_offsets, d_out_offsets, n_rows, n_out, (const int64_t*)rows, n_tiles, t, frame, (uint32_t)unknown,
                       d_err_cell, d_out);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
