// A library of position weight matrices scored per row in one pass (best window, its place and strand, windows over a threshold;
// include/bnpk.h: bnpk_pwm_rows_packed / bnpk_pwm_rows_bytes), gfx950.  No score reaches HBM; DESIGN.md 4f.
//
//   Split of work.  Every row is cut into PIECES of PW_PIECE positions (a row of 0 bases is one piece, so that every row has
//   somebody who writes its outputs); a scan over the rows' piece counts numbers the pieces.  A piece is scored by one lane
//   (rows are reads: a lane per read, neighbouring lanes on neighbouring reads) or by a workgroup (rows are long: a lane takes
//   8 starts, the 256 answers meet in six xor-shuffles and four LDS slots); the host picks by the mean row length, both serve
//   every input.  A row of one piece — every read — writes its outputs itself; the pieces of a longer row leave (score, key,
//   hits) in scratch that holds only such pieces (at most 2 n / PW_PIECE of them, whatever the rows look like: 0.4 bytes per
//   base) and pw_merge_kernel, one wavefront per such row, folds them.  Candidates are compared as (score, strand, position):
//   a total order, so neither the split nor the order of the merge can show in the result, and nothing is added atomically.
//
//   Operands.  The matrices of a GROUP of motifs (at most PW_GROUP, at most PW_LDS_DOUBLES entries: 32 KB) lie in LDS as
//   [position][code].  For a given (motif, position j) every lane of a wavefront reads one of the A entries of row j: at most
//   A distinct addresses, 4 consecutive doubles on the 2-bit path (eight banks, no conflict).  The alternative — M[j][0..3]
//   in scalar registers and a select per lane — costs about eight vector instructions per addition (two bit tests, six
//   V_CNDMASK for the two halves of a double) against one DS_READ_B64 and four (shift, mask, address) here (NOTES.md).
//
//   Registers.  A lane scores PW_ITEMS = 8 consecutive starts side by side: 8 (16 with the reverse strand) independent
//   accumulators, so that eight LDS reads are in flight before the first addition needs its operand.  The 71 bases these
//   windows cover are three 64-bit registers, shifted so that bit 0 is the lane's first start; the codes of position j of all
//   eight windows are the 16 bits at offset 2 j (one funnel shift, the word chosen uniformly).  The reverse strand reads the
//   complemented words at offset 2 (W - 1 - j).  In-window order: acc = ((0.0 + M[0][c]) + M[1][c']) + ..., never reassociated.
//   The byte path shares all of it but the fetch: the eight codes of offset j are eight bytes at the lane's start + j.
//
//   Motif loop.  The running (best, key, hits) of a lane are per motif, so the motif loop is the outer one and the lane's
//   three words are fetched again per motif — from L1 / L2: HBM sees the bases once per group.
#include <math.h>

#include "common.h"
#include "scan.h"

namespace {

constexpr int PW_ITEMS = 8;                                  // window starts a lane scores side by side
constexpr int PW_PIECE = 2048;                               // positions of a row per piece
constexpr int PW_WIDE = BNPK_BLOCK;                          // lanes per piece where the rows are long
static_assert(PW_WIDE * PW_ITEMS == PW_PIECE, "a workgroup's lanes cover a piece once");
constexpr int PW_GROUP = BNPK_PWM_GROUP_MOTIFS;
constexpr int PW_LDS_DOUBLES = 4096;                         // 16 motifs of 64 x 4
constexpr int64_t PW_WIDE_MEAN = 2 * PW_PIECE;               // mean row length from which a piece gets a workgroup
constexpr int64_t PW_NONE = INT64_MAX;                       // key of "no window"
constexpr int64_t PW_REV = 1ll << 62;                        // key = strand * PW_REV + position in the row

// a group of motifs as the kernels get it (by value: wave-uniform)
struct pw_group {
  int n, first, A, has_thr, tot;                             // motifs, index of the first, alphabet, thresholds given, matrix entries
  int64_t mat_off;                                           // the group's first entry in the device copy of the library
  int width[PW_GROUP], lds_off[PW_GROUP];
  double thr[PW_GROUP];
};

struct pw_out {
  double* best; int64_t* pos; uint8_t* strand; int64_t* hits;         // motif-major, n_rows per motif
  double* p_best; int64_t* p_key; int64_t* p_hits; int64_t p_stride;  // pieces of rows of several: p_stride per motif of the group
};

struct pw_cand { double best; int64_t key, hits; };

// (score, strand, position): larger score, then forward strand, then smaller position — np.argmax(concatenate([fwd, rev]))
__device__ __forceinline__ void pw_fold(pw_cand& a, const pw_cand& b) {
  if (b.best > a.best || (b.best == a.best && b.key < a.key)) { a.best = b.best; a.key = b.key; }
  a.hits += b.hits;
}

// over the wavefront (all 64 lanes active)
__device__ __forceinline__ void pw_fold_lanes(pw_cand& c) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    pw_cand o;
    o.best = __shfl_xor(c.best, d, 64);
    o.key = __shfl_xor((long long)c.key, d, 64);
    o.hits = __shfl_xor((long long)c.hits, d, 64);
    pw_fold(c, o);
  }
}

__device__ __forceinline__ void pw_write(const pw_out& o, int64_t idx, const pw_cand& c) {
  o.best[idx] = c.best;
  o.pos[idx] = c.key == PW_NONE ? -1 : (c.key & (PW_REV - 1));
  if (o.strand) o.strand[idx] = (uint8_t)(c.key != PW_NONE && (c.key & PW_REV));
  if (o.hits) o.hits[idx] = c.hits;
}

// ---- the symbol fetch: all that differs between the two paths ----------------------------------------------------------------------
struct pw_src_packed { const uint64_t* W; int64_t n_words; };
struct pw_win_packed {
  typedef uint32_t word;
  static constexpr bool BOTH_STRANDS = true;
  uint64_t s0, s1, s2;                                       // bases 0 .. 95 behind the lane's first start, 2 bits each
  __device__ __forceinline__ void load(const pw_src_packed& S, int64_t g) {
    const int64_t wi = g >> 5;
    const int sh = 2 * (int)(g & 31);
    uint64_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = wi + i < S.n_words ? S.W[wi + i] : 0ull;
    s0 = sh ? (w[0] >> sh) | (w[1] << (64 - sh)) : w[0];
    s1 = sh ? (w[1] >> sh) | (w[2] << (64 - sh)) : w[1];
    s2 = sh ? (w[2] >> sh) | (w[3] << (64 - sh)) : w[2];
  }
  // the codes of bases o .. o + 7 (o uniform, 0 .. 63), and their complements
  __device__ __forceinline__ word at(int o) const {
    const uint64_t a = o < 32 ? s0 : s1, b = o < 32 ? s1 : s2;
    const int sh = 2 * (o & 31);
    return (word)(sh ? (a >> sh) | (b << (64 - sh)) : a);
  }
  __device__ __forceinline__ word rc_at(int o) const { return ~at(o); }
  static __device__ __forceinline__ int code(word x, int q, int) { return (int)((x >> (2 * q)) & 3u); }
};

struct pw_src_bytes { const uint8_t* codes; int64_t n; };
struct pw_win_bytes {
  typedef uint64_t word;
  static constexpr bool BOTH_STRANDS = false;
  const uint8_t* p;
  int64_t left;                                              // symbols from the lane's first start to the end of the data
  __device__ __forceinline__ void load(const pw_src_bytes& S, int64_t g) { p = S.codes + g; left = S.n - g; }
  __device__ __forceinline__ word at(int o) const {
    word x = 0;
    if (o + PW_ITEMS <= left) {
      __builtin_memcpy(&x, p + o, 8);
    } else {
#pragma unroll
      for (int q = 0; q < PW_ITEMS; ++q)
        if (o + q < left) x |= (word)p[o + q] << (8 * q);
    }
    return x;
  }
  __device__ __forceinline__ word rc_at(int o) const { return at(o); }   // (no reverse strand on this path)
  // a byte that is no code of the alphabet must not lead outside the motif's table
  static __device__ __forceinline__ int code(word x, int q, int A) { return min((int)((x >> (8 * q)) & 255u), A - 1); }
};

// scores the windows at starts c0 .. c0 + nv - 1 (nv <= 8) of a row and folds them into f (forward) and r (reverse).  M: the
// motif in LDS, [position][code].  Within a lane the starts come in ascending order, so "larger" is all a candidate has to be.
template <class Win, bool BOTH>
__device__ __forceinline__ void pw_chunk(const Win& w, const double* __restrict__ M, int W, int A, int nv, int64_t c0, double thr,
                                         bool count, pw_cand& f, pw_cand& r) {
  double acc[PW_ITEMS], rac[PW_ITEMS];
#pragma unroll
  for (int q = 0; q < PW_ITEMS; ++q) acc[q] = rac[q] = 0.0;
  for (int j = 0; j < W; ++j) {
    const double* __restrict__ Mj = M + j * A;
    const typename Win::word x = w.at(j);
#pragma unroll
    for (int q = 0; q < PW_ITEMS; ++q) acc[q] += Mj[Win::code(x, q, A)];
    if (BOTH) {
      const typename Win::word y = w.rc_at(W - 1 - j);
#pragma unroll
      for (int q = 0; q < PW_ITEMS; ++q) rac[q] += Mj[Win::code(y, q, A)];
    }
  }
#pragma unroll
  for (int q = 0; q < PW_ITEMS; ++q) {
    if (q < nv) {
      if (acc[q] > f.best || f.key == PW_NONE) { f.best = acc[q]; f.key = c0 + q; }
      if (count) f.hits += acc[q] >= thr;
      if (BOTH) {
        if (rac[q] > r.best || r.key == PW_NONE) { r.best = rac[q]; r.key = PW_REV + c0 + q; }
        if (count) r.hits += rac[q] >= thr;
      }
    }
  }
}

// piece_first[r] = pieces of the rows before r (n_rows + 1 entries), multi_first: the same over rows of two pieces or more
template <class Src, class Win, bool BOTH, int SUB>
__global__ __launch_bounds__(BNPK_BLOCK) void pw_rows_kernel(Src src, const int64_t* __restrict__ off, int64_t n_rows,
                                                            const int64_t* __restrict__ piece_first,
                                                            const int64_t* __restrict__ multi_first,
                                                            const double* __restrict__ mats, pw_group g, pw_out o) {
  __shared__ double mat[PW_LDS_DOUBLES];
  __shared__ pw_cand red[BNPK_BLOCK / 64];
  for (int i = threadIdx.x; i < g.tot; i += BNPK_BLOCK) mat[i] = mats[g.mat_off + i];
  __syncthreads();
  const int64_t n_pieces = piece_first[n_rows];
  const int sub = threadIdx.x % SUB;
  const int64_t stride = (int64_t)gridDim.x * (BNPK_BLOCK / SUB);
  for (int64_t slot = (int64_t)blockIdx.x * (BNPK_BLOCK / SUB) + threadIdx.x / SUB; slot < n_pieces; slot += stride) {
    // (every row has a piece: piece_first is strictly increasing; where every row has ONE, the piece is the row)
    const int64_t r = n_pieces == n_rows ? slot : find_row(piece_first, 0, n_rows - 1, slot);
    const int64_t first = piece_first[r], pieces = piece_first[r + 1] - first;
    const int64_t s = off[r], L = off[r + 1] - s;
    const int64_t p0 = (slot - first) * PW_PIECE, p1 = min(L, p0 + PW_PIECE);
    for (int m = 0; m < g.n; ++m) {
      const int W = g.width[m];
      const double* M = mat + g.lds_off[m];
      const int64_t end = min(p1, L - W + 1);                // the piece's window starts are p0 .. end - 1
      pw_cand f = {-INFINITY, PW_NONE, 0}, rv = {-INFINITY, PW_NONE, 0};
      for (int64_t c0 = p0 + sub * PW_ITEMS; c0 < end; c0 += SUB * PW_ITEMS) {
        Win w;
        w.load(src, s + c0);
        pw_chunk<Win, BOTH>(w, M, W, g.A, (int)min((int64_t)PW_ITEMS, end - c0), c0, g.thr[m], g.has_thr != 0, f, rv);
      }
      if (BOTH) pw_fold(f, rv);
      if (SUB > 1) {                                         // (slot and m are the workgroup's: every lane is here)
        pw_fold_lanes(f);
        if (lane_id() == 0) red[wave_id()] = f;
        __syncthreads();
        if (threadIdx.x == 0)
          for (int w = 1; w < BNPK_BLOCK / 64; ++w) pw_fold(f, red[w]);
        __syncthreads();
      }
      if (sub == 0) {
        if (pieces == 1) {
          pw_write(o, (int64_t)(g.first + m) * n_rows + r, f);
        } else {
          const int64_t at = multi_first[r] + (slot - first);
          if (at < o.p_stride) {                             // (holds for offsets that are what the header asks for)
            o.p_best[m * o.p_stride + at] = f.best;
            o.p_key[m * o.p_stride + at] = f.key;
            o.p_hits[m * o.p_stride + at] = f.hits;
          }
        }
      }
    }
  }
}

// a lane per row looks for the rows of several pieces; the wavefront then folds the pieces of each, motif by motif
__global__ __launch_bounds__(BNPK_BLOCK) void pw_merge_kernel(const int64_t* __restrict__ piece_first,
                                                             const int64_t* __restrict__ multi_first, int64_t n_rows, pw_group g,
                                                             pw_out o) {
  const int lane = lane_id();
  const int64_t stride = (int64_t)gridDim.x * BNPK_BLOCK;
  for (int64_t base = (int64_t)blockIdx.x * BNPK_BLOCK + wave_id() * 64; base < n_rows; base += stride) {
    const int64_t r = base + lane;
    const int64_t mine = r < n_rows ? piece_first[r + 1] - piece_first[r] : 0;
    uint64_t todo = __ballot(mine >= 2);
    while (todo) {
      const int b = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int64_t row = base + b;
      const int64_t pieces = piece_first[row + 1] - piece_first[row], at = multi_first[row];
      for (int m = 0; m < g.n; ++m) {
        pw_cand c = {-INFINITY, PW_NONE, 0};
        for (int64_t k = lane; k < pieces && at + k < o.p_stride; k += 64) {
          const int64_t i = m * o.p_stride + at + k;
          const pw_cand p = {o.p_best[i], o.p_key[i], o.p_hits[i]};
          pw_fold(c, p);
        }
        pw_fold_lanes(c);
        if (lane == 0) pw_write(o, (int64_t)(g.first + m) * n_rows + row, c);
      }
    }
  }
}

__global__ void pw_pieces_kernel(const int64_t* __restrict__ off, int64_t n_rows, int64_t* __restrict__ pieces,
                                 int64_t* __restrict__ multi) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t L = off[r + 1] - off[r];
    const int64_t n = max((L + PW_PIECE - 1) / PW_PIECE, (int64_t)1);
    pieces[r] = n;
    multi[r] = n >= 2 ? n : 0;
  }
}

static inline size_t pw_align(size_t b) { return (b + 63) & ~(size_t)63; }

template <class Src, class Win>
static int pw_run(bnpk_ctx* ctx, const bnpk_pwm_library* lib, Src src, int64_t n, const int64_t* d_offsets, int64_t n_rows,
                  int both, double* d_best, int64_t* d_pos, uint8_t* d_strand, int64_t* d_hits, const char* name, hipStream_t s) {
  // the library: checked, and cut into groups that fit the LDS table
  const int A = lib->alphabet_size;
  std::vector<pw_group> groups;
  int64_t entries = 0;
  for (int m = 0; m < lib->n_motifs; ++m) {
    const int W = lib->width[m];
    if (W < 1 || W > BNPK_PWM_MAX_WIDTH) return BNPK_ERR_ARG;
    for (int64_t i = 0; i < (int64_t)W * A; ++i)
      if (!(lib->matrix[entries + i] < INFINITY)) return BNPK_ERR_ARG;          // NaN or +inf
    if (lib->threshold && !(lib->threshold[m] < INFINITY)) return BNPK_ERR_ARG;
    if (groups.empty() || groups.back().n == PW_GROUP || groups.back().tot + W * A > PW_LDS_DOUBLES) {
      pw_group g = {};
      g.first = m; g.A = A; g.has_thr = lib->threshold ? 1 : 0; g.mat_off = entries;
      groups.push_back(g);
    }
    pw_group& g = groups.back();
    g.width[g.n] = W;
    g.lds_off[g.n] = g.tot;
    g.thr[g.n] = lib->threshold ? lib->threshold[m] : 0.0;
    g.tot += W * A;
    g.n += 1;
    entries += (int64_t)W * A;
  }
  if (n_rows == 0) return BNPK_OK;
  const int64_t p_stride = 2 * (n / PW_PIECE) + 2;           // pieces of rows of two or more: fewer than 2 L / PW_PIECE each
  const int64_t max_pieces = n_rows + n / PW_PIECE;
  const size_t b_mat = pw_align((size_t)entries * 8), b_tab = pw_align((size_t)(n_rows + 1) * 8);
  const size_t b_scan = pw_align(bnpk_scan_scratch_bytes(n_rows)), b_part = pw_align((size_t)PW_GROUP * p_stride * 8);
  void* scratch = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, b_mat + 2 * b_tab + b_scan + 3 * b_part, &scratch, s));
  char* at = (char*)scratch;
  double* d_mats = (double*)at; at += b_mat;
  int64_t* piece_first = (int64_t*)at; at += b_tab;
  int64_t* multi_first = (int64_t*)at; at += b_tab;
  int64_t* scan_scratch = (int64_t*)at; at += b_scan;
  pw_out o = {d_best, d_pos, d_strand, d_hits, (double*)at, (int64_t*)(at + b_part), (int64_t*)(at + 2 * b_part), p_stride};
  BNPK_HIP(ctx, hipMemcpyAsync(d_mats, lib->matrix, (size_t)entries * 8, hipMemcpyHostToDevice, s));
  bnpk_timer t(ctx, name, s);
  hipLaunchKernelGGL(pw_pieces_kernel, dim3(grid_for(ceil_div(n_rows, 256))), dim3(256), 0, s, d_offsets, n_rows, piece_first,
                     multi_first);
  BNPK_HIP(ctx, hipGetLastError());
  BNPK_CHECK(bnpk_scan_launch(ctx, piece_first, n_rows, 1, piece_first, true, scan_scratch, s));
  BNPK_CHECK(bnpk_scan_launch(ctx, multi_first, n_rows, 1, multi_first, true, scan_scratch, s));
  const bool wide = ctx->pwm_split ? ctx->pwm_split == 2 : n / n_rows >= PW_WIDE_MEAN;
  const unsigned grid = grid_for(ceil_div(max_pieces, BNPK_BLOCK / (wide ? PW_WIDE : 1)));
  void (*kernel)(Src, const int64_t*, int64_t, const int64_t*, const int64_t*, const double*, pw_group, pw_out) =
      wide ? pw_rows_kernel<Src, Win, false, PW_WIDE> : pw_rows_kernel<Src, Win, false, 1>;
  if constexpr (Win::BOTH_STRANDS)
    if (both) kernel = wide ? pw_rows_kernel<Src, Win, true, PW_WIDE> : pw_rows_kernel<Src, Win, true, 1>;
  for (const pw_group& g : groups) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(BNPK_BLOCK), 0, s, src, d_offsets, n_rows, piece_first, multi_first, d_mats, g, o);
    BNPK_HIP(ctx, hipGetLastError());
    if (n > PW_PIECE) {                                      // (else no row has a second piece)
      hipLaunchKernelGGL(pw_merge_kernel, dim3(grid_for(ceil_div(n_rows, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, piece_first, multi_first,
                         n_rows, g, o);
      BNPK_HIP(ctx, hipGetLastError());
    }
  }
  return BNPK_OK;
}

static int pw_check(bnpk_ctx* ctx, const bnpk_pwm_library* lib, int a_lo, int a_hi, int64_t n, const void* d_data,
                    const int64_t* d_offsets, int64_t n_rows, const double* d_best, const int64_t* d_pos, const int64_t* d_hits) {
  if (!ctx || !lib || n < 0 || n_rows < 0) return BNPK_ERR_ARG;
  if (lib->n_motifs < 1 || lib->n_motifs > BNPK_PWM_MAX_MOTIFS || lib->alphabet_size < a_lo || lib->alphabet_size > a_hi)
    return BNPK_ERR_ARG;
  if (!lib->width || !lib->matrix || (d_hits && !lib->threshold)) return BNPK_ERR_ARG;
  if (n_rows > 0 && (!d_offsets || !d_best || !d_pos || (n > 0 && !d_data))) return BNPK_ERR_ARG;
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_pwm_rows_packed(bnpk_ctx* ctx, const bnpk_pwm_library* h_lib, const uint64_t* d_packed, int64_t n_bases,
                         const int64_t* d_offsets, int64_t n_rows, int both_strands, double* d_best, int64_t* d_pos,
                         uint8_t* d_strand, int64_t* d_hits, void* stream) {
  BNPK_CHECK(pw_check(ctx, h_lib, 4, 4, n_bases, d_packed, d_offsets, n_rows, d_best, d_pos, d_hits));
  const pw_src_packed src = {d_packed, ceil_div(n_bases, (int64_t)32)};
  return pw_run<pw_src_packed, pw_win_packed>(ctx, h_lib, src, n_bases, d_offsets, n_rows, both_strands != 0, d_best, d_pos, d_strand,
                                              d_hits, "pwm_rows_packed", (hipStream_t)stream);
}

int bnpk_pwm_rows_bytes(bnpk_ctx* ctx, const bnpk_pwm_library* h_lib, const uint8_t* d_codes, int64_t n, const int64_t* d_offsets,
                        int64_t n_rows, double* d_best, int64_t* d_pos, int64_t* d_hits, void* stream) {
  BNPK_CHECK(pw_check(ctx, h_lib, 2, BNPK_PWM_MAX_ALPHABET, n, d_codes, d_offsets, n_rows, d_best, d_pos, d_hits));
  const pw_src_bytes src = {d_codes, n};
  return pw_run<pw_src_bytes, pw_win_bytes>(ctx, h_lib, src, n, d_offsets, n_rows, 0, d_best, d_pos, nullptr, d_hits,
                                            "pwm_rows_bytes", (hipStream_t)stream);
}

}  // extern "C"
