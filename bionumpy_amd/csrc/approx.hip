// Approximate (edit distance) search of a library of patterns per row, and the place to cut an adapter (include/bnpk.h:
// bnpk_approx_rows_packed / bnpk_approx_rows_bytes), gfx950.  Nothing reaches HBM but a few words per (pattern, row); DESIGN.md 4d.
//
//   Inner loop.  Myers' bit-vector recurrence: the column D[0..m][j] of the dynamic programme is two m-bit words of vertical
//   deltas (Pv: +1, Mv: -1) and the running D[m][j]; a symbol costs about 17 word operations, one of them an addition whose
//   carry runs up the column, and no memory traffic but the symbol.  Bits at and above m hold garbage that never comes down
//   (the addition carries upwards, the shifts go left), so nothing is masked.  Shifting a 1 in place of a 0 into the
//   horizontal delta of row 0 turns the search (D[0][j] = 0, free start) into the ANCHORED problem (D[0][j] = j), which is
//   what the start of a match is found with.  Two instantiations: 32-bit words for patterns of up to 32 positions (half the
//   vector instructions: every adapter prefix and barcode), 64-bit words for the rest; the host groups the library by it.
//
//   Split of work.  A row is cut into PIECES of `piece` positions (a power of two the host picks so that a single
//   chromosome still fills the card; a row of 0 symbols is one piece).  A lane takes a piece — rows are reads: neighbouring
//   lanes on neighbouring reads.  Its column is exact once it has run over the 2 m symbols in front of the piece (an optimal
//   alignment of P[0:i] uses at most 2 i symbols), so every piece but a row's first warms up over those and then reports
//   (dist, end, hits) for its own end positions only.  A row of one piece — every read — is finished by its lane; the pieces
//   of a longer row leave (dist << 56 | end, hits) in scratch and ax_merge_kernel, one wavefront per such row, folds them:
//   the smaller word wins (smaller dist, then smaller end: a total order), hits are added, nothing atomically, so neither the
//   split nor the order of the merge can show.  The lanes 0 .. patterns - 1 of that wavefront then finish the row.
//
//   Finishing a (pattern, row), ax_finish.  Not found and an overhang allowed: D[i][L] for i = m - 1 down to min_overlap from
//   the vertical deltas of the last column (the merge has no column: it runs the last 2 m symbols of the row again).  Found,
//   whole or overhanging: the anchored recurrence over the reversed pattern walks back from end - 1 until it meets dist, at
//   most m + dist symbols.  The reversed prefix of i positions is the top i bits of the reversed pattern: its masks shifted
//   right by m - i.
//
//   Operands.  The acceptance masks of a group of patterns travel in the kernel's arguments (at most 2 KB) and are laid into
//   LDS as [pattern][code], forward and bit-reversed; a lane reads Eq with one DS_READ at one of at most `alphabet` distinct
//   addresses per wavefront.  (The 2-bit path could keep the four masks in scalar registers and select: NOTES.md.)
//   The pattern loop is the outer one; a lane's few words of symbols come again per pattern from L1 / L2.
//   The packed and the byte path differ in the fetch alone: ax_packed / ax_bytes hand out up to 32 / 8 symbols per load.
#include "common.h"
#include "scan.h"

namespace {

constexpr int AX_GROUP = 16;                                 // patterns per launch, at most
constexpr int AX_MASKS = 256;                                // masks per launch, at most (2 KB of kernel arguments)
constexpr int AX_MIN_PIECE = 256;
constexpr int AX_MAX_PIECE = 1 << 16;
constexpr int AX_LANES_PER_CU = 1024;                        // pieces per compute unit the automatic piece length aims at
static_assert(AX_MASKS >= BNPK_APPROX_MAX_ALPHABET, "a pattern's masks fit one launch");

// a group of patterns as the kernels get it (by value: wave-uniform)
struct ax_group {
  int n, first, A;                                           // patterns, index of the first, alphabet
  int m[AX_GROUP], k[AX_GROUP], o[AX_GROUP];                 // positions, max_errors, min_overlap
  uint64_t eq[AX_MASKS];                                     // [pattern][code]
};

struct ax_out {
  uint8_t* dist; int64_t* start; int64_t* end; uint8_t* overlap; int64_t* hits;   // pattern-major, n_rows per pattern
  uint64_t* p_key; int64_t* p_hits; int64_t p_stride;        // pieces of rows of several: p_stride per pattern of the group
};

template <class W>
struct ax_col { W Pv, Mv; int score; };

// one symbol.  Eq: the positions that accept it; top: bit m - 1; in: 0 = search, 1 = anchored
template <class W>
__device__ __forceinline__ void ax_step(ax_col<W>& c, W Eq, W top, W in) {
  const W Xv = Eq | c.Mv;
  const W Xh = (((Eq & c.Pv) + c.Pv) ^ c.Pv) | Eq;
  W Ph = c.Mv | ~(Xh | c.Pv);
  W Mh = c.Pv & Xh;
  c.score += (Ph & top) != 0;
  c.score -= (Mh & top) != 0;
  Ph = (Ph << 1) | in;
  Mh <<= 1;
  c.Pv = Mh | ~(Xv | Ph);
  c.Mv = Ph & Xv;
}

// ---- the symbol fetch: all that differs between the two paths ----------------------------------------------------------------------
// fwd(g, cnt): the symbols g .. g + cnt - 1 from bit 0 upwards; bwd(g, cnt): the symbols g, g - 1, .. g - cnt + 1 from the top
// bit downwards.  g is a position of the flat data; cnt may reach past the caller's range, who stops by its own count.
struct ax_packed {
  static constexpr int BITS = 2;
  const uint64_t* W; int64_t n;
  __device__ __forceinline__ uint64_t fwd(int64_t g, int& cnt) const {
    const int q = (int)(g & 31);
    cnt = 32 - q;
    return W[g >> 5] >> (2 * q);
  }
  __device__ __forceinline__ uint64_t bwd(int64_t g, int& cnt) const {
    const int q = (int)(g & 31);
    cnt = q + 1;
    return W[g >> 5] << (62 - 2 * q);
  }
};

struct ax_bytes {
  static constexpr int BITS = 8;
  const uint8_t* p; int64_t n;
  __device__ __forceinline__ uint64_t fwd(int64_t g, int& cnt) const {
    uint64_t x = 0;
    cnt = 8;
    if (g + 8 <= n) {
      __builtin_memcpy(&x, p + g, 8);
    } else {
      for (int q = 0; q < 8; ++q)
        if (g + q < n) x |= (uint64_t)p[g + q] << (8 * q);
    }
    return x;
  }
  __device__ __forceinline__ uint64_t bwd(int64_t g, int& cnt) const {
    uint64_t x = 0;
    cnt = 8;
    if (g >= 7) {
      __builtin_memcpy(&x, p + g - 7, 8);
    } else {
      for (int q = 0; q < 8; ++q)
        if (g - q >= 0) x |= (uint64_t)p[g - q] << (56 - 8 * q);
    }
    return x;
  }
};

// a byte that is no code of the alphabet accepts nothing and reads nothing outside the pattern's masks
template <class W, class Src>
__device__ __forceinline__ W ax_eq(const W* __restrict__ eq, unsigned c, int A) {
  if (Src::BITS == 2) return eq[c];
  return c < (unsigned)A ? eq[c] : (W)0;
}

// the column over the symbols g0 .. g0 + count - 1 of the flat data, nothing reported (warm-up; the merge's last column)
template <class W, class Src>
__device__ __forceinline__ void ax_warm(const Src& src, int64_t g0, int64_t count, const W* __restrict__ eq, int A, W top,
                                        ax_col<W>& c) {
  for (int64_t done = 0; done < count;) {
    int cnt;
    uint64_t w = src.fwd(g0 + done, cnt);
    cnt = (int)min((int64_t)cnt, count - done);
    for (int q = 0; q < cnt; ++q, w >>= Src::BITS) ax_step<W>(c, ax_eq<W, Src>(eq, (unsigned)(w & ((1u << Src::BITS) - 1)), A), top, (W)0);
    done += cnt;
  }
}

// the same, and every end position j0 + 1 .. j0 + count (j0 = symbols of the row before g0) is a candidate
template <class W, class Src>
__device__ __forceinline__ void ax_search(const Src& src, int64_t g0, int64_t count, const W* __restrict__ eq, int A, W top, int k,
                                          ax_col<W>& c, int& best, int& best_at, int& hits) {
  for (int done = 0; done < count;) {
    int cnt;
    uint64_t w = src.fwd(g0 + done, cnt);
    cnt = (int)min((int64_t)cnt, count - done);
    for (int q = 0; q < cnt; ++q, w >>= Src::BITS) {
      ax_step<W>(c, ax_eq<W, Src>(eq, (unsigned)(w & ((1u << Src::BITS) - 1)), A), top, (W)0);
      hits += c.score <= k;
      if (c.score < best) { best = c.score; best_at = done + q + 1; }          // (strictly: the smallest end stays)
    }
    done += cnt;
  }
}

// the smallest t <= limit with ed(P[0:i], c[e - t : e]) == dist; g_last: the flat position of symbol e - 1; req: the reversed
// masks of the whole pattern, shift = m - i
template <class W, class Src>
__device__ __forceinline__ int ax_start(const Src& src, int64_t g_last, int limit, const W* __restrict__ req, int shift, int A,
                                        int i, int dist) {
  ax_col<W> c = {(W)~(W)0, (W)0, i};
  const W top = (W)1 << (i - 1);
  for (int done = 0; done < limit;) {
    int cnt;
    uint64_t w = src.bwd(g_last - done, cnt);
    cnt = min(cnt, limit - done);
    for (int q = 0; q < cnt; ++q, w <<= Src::BITS) {
      ax_step<W>(c, (W)(ax_eq<W, Src>(req, (unsigned)(w >> (64 - Src::BITS)), A) >> shift), top, (W)1);
      if (c.score == dist) return done + q + 1;
    }
    done += cnt;
  }
  return limit;                                              // (not reached: a t <= i + dist exists)
}

// what is known of a (pattern, row) after the search -> its five outputs.  s: the row's first position in the flat data
template <class W, class Src>
__device__ __forceinline__ void ax_finish(const Src& src, int64_t s, int64_t L, int m, int k, int o, const W* __restrict__ eq,
                                          const W* __restrict__ req, int A, int dist, int64_t end, int64_t hits, bool have_col,
                                          ax_col<W> c, const ax_out& out, int64_t idx) {
  int overlap = dist <= k ? m : 0;
  if (!overlap && o > 0) {
    if (!have_col) {                                         // the column at L from the last 2 m symbols
      const int64_t w = min(L, (int64_t)2 * m);
      c = {(W)~(W)0, (W)0, m};
      ax_warm<W, Src>(src, s + L - w, w, eq, A, (W)1 << (m - 1), c);
    }
    int d = c.score;                                         // D[m][L]
    for (int i = m - 1; i >= o; --i) {
      d += (int)((c.Mv >> i) & 1) - (int)((c.Pv >> i) & 1);  // D[i][L]
      if (d <= k * i / m) { overlap = i; dist = d; end = L; break; }
    }
  }
  int64_t start = -1;
  if (overlap) {
    const int limit = (int)min((int64_t)(overlap + dist), end);
    start = end - ax_start<W, Src>(src, s + end - 1, limit, req, m - overlap, A, overlap, dist);
  } else {
    end = -1;
  }
  out.dist[idx] = (uint8_t)dist;
  out.start[idx] = start;
  out.end[idx] = end;
  out.overlap[idx] = (uint8_t)overlap;
  if (out.hits) out.hits[idx] = hits;
}

// the group's masks into LDS: eq as given, req bit-reversed within each pattern's m positions
template <class W>
__device__ __forceinline__ void ax_load_masks(const ax_group& g, W* eq, W* req) {
  for (int i = threadIdx.x; i < g.n * g.A; i += BNPK_BLOCK) {
    const uint64_t e = g.eq[i];
    eq[i] = (W)e;
    req[i] = (W)(__brevll(e) >> (64 - g.m[i / g.A]));
  }
  __syncthreads();
}

// piece_first[r] = pieces of the rows before r (n_rows + 1 entries), multi_first: the same over rows of two pieces or more
template <class W, class Src>
__global__ __launch_bounds__(BNPK_BLOCK) void ax_rows_kernel(Src src, const int64_t* __restrict__ off, int64_t n_rows, int piece,
                                                            const int64_t* __restrict__ piece_first,
                                                            const int64_t* __restrict__ multi_first, ax_group g, ax_out o) {
  __shared__ W eq[AX_MASKS], req[AX_MASKS];
  ax_load_masks<W>(g, eq, req);
  const int64_t n_pieces = piece_first[n_rows];
  const int64_t stride = (int64_t)gridDim.x * BNPK_BLOCK;
  for (int64_t slot = (int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x; slot < n_pieces; slot += stride) {
    // (every row has a piece: piece_first is strictly increasing; where every row has ONE, the piece is the row)
    const int64_t r = n_pieces == n_rows ? slot : find_row(piece_first, 0, n_rows - 1, slot);
    const int64_t first = piece_first[r], pieces = piece_first[r + 1] - first;
    const int64_t s = off[r], L = off[r + 1] - s;
    const int64_t p0 = (slot - first) * piece;
    const int count = (int)(min(L, p0 + piece) - p0);
    for (int pi = 0; pi < g.n; ++pi) {
      const int m = g.m[pi], k = g.k[pi];
      const W* e = eq + pi * g.A;
      const W top = (W)1 << (m - 1);
      ax_col<W> c = {(W)~(W)0, (W)0, m};
      const int64_t warm = min(p0, (int64_t)2 * m);
      ax_warm<W, Src>(src, s + p0 - warm, warm, e, g.A, top, c);
      int best = p0 == 0 ? m : 255, best_at = 0, hits = 0;   // (end 0 is the first piece's; 255: larger than any distance)
      ax_search<W, Src>(src, s + p0, count, e, g.A, top, k, c, best, best_at, hits);
      if (pieces == 1) {
        ax_finish<W, Src>(src, s, L, m, k, g.o[pi], e, req + pi * g.A, g.A, best, best_at, hits, true, c, o,
                          (int64_t)(g.first + pi) * n_rows + r);
      } else {
        const int64_t at = multi_first[r] + (slot - first);
        if (at < o.p_stride) {                               // (holds for offsets that are what the header asks for)
          o.p_key[pi * o.p_stride + at] = (uint64_t)best << 56 | (uint64_t)(p0 + best_at);
          o.p_hits[pi * o.p_stride + at] = hits;
        }
      }
    }
  }
}

// a lane per row looks for the rows of several pieces; the wavefront then folds the pieces of each, pattern by pattern, and
// lane pi finishes pattern pi
template <class W, class Src>
__global__ __launch_bounds__(BNPK_BLOCK) void ax_merge_kernel(Src src, const int64_t* __restrict__ off, int64_t n_rows,
                                                             const int64_t* __restrict__ piece_first,
                                                             const int64_t* __restrict__ multi_first, ax_group g, ax_out o) {
  __shared__ W eq[AX_MASKS], req[AX_MASKS];
  ax_load_masks<W>(g, eq, req);
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
      unsigned long long my_key = ~0ull;
      long long my_hits = 0;
      for (int pi = 0; pi < g.n; ++pi) {
        unsigned long long key = ~0ull;
        long long hits = 0;
        for (int64_t q = lane; q < pieces && at + q < o.p_stride; q += 64) {
          key = min(key, (unsigned long long)o.p_key[pi * o.p_stride + at + q]);
          hits += o.p_hits[pi * o.p_stride + at + q];
        }
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
          key = min(key, (unsigned long long)__shfl_xor(key, d, 64));
          hits += __shfl_xor(hits, d, 64);
        }
        if (lane == pi) { my_key = key; my_hits = hits; }
      }
      if (lane < g.n) {
        const int64_t s = off[row];
        const ax_col<W> none = {(W)0, (W)0, 0};
        ax_finish<W, Src>(src, s, off[row + 1] - s, g.m[lane], g.k[lane], g.o[lane], eq + lane * g.A, req + lane * g.A, g.A,
                          (int)(my_key >> 56), (int64_t)(my_key & ((1ull << 56) - 1)), my_hits, false, none, o,
                          (int64_t)(g.first + lane) * n_rows + row);
      }
    }
  }
}

__global__ void ax_pieces_kernel(const int64_t* __restrict__ off, int64_t n_rows, int piece, int64_t* __restrict__ pieces,
                                 int64_t* __restrict__ multi) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t L = off[r + 1] - off[r];
    const int64_t n = max((L + piece - 1) / piece, (int64_t)1);
    pieces[r] = n;
    multi[r] = n >= 2 ? n : 0;
  }
}

// out[r] = the length a row keeps: up to the adapter's start where one was found
__global__ void ax_trim_kernel(const int64_t* __restrict__ start, const int64_t* __restrict__ lens, int64_t n,
                               int64_t* __restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    out[r] = start[r] >= 0 ? min(start[r], lens[r]) : lens[r];
}

static inline size_t ax_align(size_t b) { return (b + 63) & ~(size_t)63; }

template <class W, class Src>
static int ax_launch(bnpk_ctx* ctx, Src src, const int64_t* d_offsets, int64_t n_rows, int piece, bool any_multi, unsigned grid,
                     const int64_t* piece_first, const int64_t* multi_first, const ax_group& g, const ax_out& o, hipStream_t s) {
  hipLaunchKernelGGL((ax_rows_kernel<W, Src>), dim3(grid), dim3(BNPK_BLOCK), 0, s, src, d_offsets, n_rows, piece, piece_first,
                     multi_first, g, o);
  BNPK_HIP(ctx, hipGetLastError());
  if (any_multi) {
    hipLaunchKernelGGL((ax_merge_kernel<W, Src>), dim3(grid_for(ceil_div(n_rows, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, src, d_offsets,
                       n_rows, piece_first, multi_first, g, o);
    BNPK_HIP(ctx, hipGetLastError());
  }
  return BNPK_OK;
}

template <class Src>
static int ax_run(bnpk_ctx* ctx, const bnpk_approx_library* lib, int a_lo, int a_hi, Src src, const void* d_data,
                  const int64_t* d_offsets, int64_t n_rows, uint8_t* d_dist, int64_t* d_start, int64_t* d_end, uint8_t* d_overlap,
                  int64_t* d_hits, const char* name, hipStream_t s) {
  const int64_t n = src.n;
  if (!ctx || !lib || n < 0 || n_rows < 0) return BNPK_ERR_ARG;
  const int A = lib->alphabet_size;
  if (lib->n_patterns < 1 || lib->n_patterns > BNPK_APPROX_MAX_PATTERNS || A < a_lo || A > a_hi) return BNPK_ERR_ARG;
  if (!lib->m || !lib->max_errors || !lib->min_overlap || !lib->eq) return BNPK_ERR_ARG;
  if (n_rows > 0 && (!d_offsets || !d_dist || !d_start || !d_end || !d_overlap || (n > 0 && !d_data))) return BNPK_ERR_ARG;
  // the library: checked, and cut into groups of one word width that fit a launch's arguments
  std::vector<ax_group> groups;
  std::vector<char> wide;
  for (int p = 0; p < lib->n_patterns; ++p) {
    const int m = lib->m[p], k = lib->max_errors[p], o = lib->min_overlap[p];
    if (m < 1 || m > BNPK_APPROX_MAX_LEN || k < 0 || k >= m || o < 0 || o >= m) return BNPK_ERR_ARG;
    const uint64_t* e = lib->eq + (int64_t)p * A;
    for (int a = 0; a < A; ++a)
      if (m < 64 && (e[a] >> m)) return BNPK_ERR_ARG;
    const char w = m > 32;
    if (groups.empty() || wide.back() != w || groups.back().n == AX_GROUP || (groups.back().n + 1) * A > AX_MASKS) {
      ax_group g = {};
      g.first = p; g.A = A;
      groups.push_back(g);
      wide.push_back(w);
    }
    ax_group& g = groups.back();
    g.m[g.n] = m; g.k[g.n] = k; g.o[g.n] = o;
    memcpy(g.eq + g.n * A, e, (size_t)A * 8);
    g.n += 1;
  }
  if (n_rows == 0) return BNPK_OK;
  int piece = ctx->approx_piece;
  if (!piece) {                                              // so many pieces that a single long row still fills the card
    const int64_t want = n / ((int64_t)ctx->compute_units * AX_LANES_PER_CU);
    piece = AX_MIN_PIECE;
    while (piece < AX_MAX_PIECE && piece < want) piece *= 2;
  }
  const int64_t p_stride = 2 * (n / piece) + 2;              // pieces of rows of two or more: fewer than 2 L / piece each
  const int64_t max_pieces = n_rows + n / piece;
  const size_t b_tab = ax_align((size_t)(n_rows + 1) * 8), b_scan = ax_align(bnpk_scan_scratch_bytes(n_rows));
  const size_t b_part = ax_align((size_t)AX_GROUP * p_stride * 8);
  void* scratch = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, 2 * b_tab + b_scan + 2 * b_part, &scratch, s));
  char* at = (char*)scratch;
  int64_t* piece_first = (int64_t*)at; at += b_tab;
  int64_t* multi_first = (int64_t*)at; at += b_tab;
  int64_t* scan_scratch = (int64_t*)at; at += b_scan;
  const ax_out o = {d_dist, d_start, d_end, d_overlap, d_hits, (uint64_t*)at, (int64_t*)(at + b_part), p_stride};
  bnpk_timer t(ctx, name, s);
  hipLaunchKernelGGL(ax_pieces_kernel, dim3(grid_for(ceil_div(n_rows, 256))), dim3(256), 0, s, d_offsets, n_rows, piece, piece_first,
                     multi_first);
  BNPK_HIP(ctx, hipGetLastError());
  BNPK_CHECK(bnpk_scan_launch(ctx, piece_first, n_rows, 1, piece_first, true, scan_scratch, s));
  BNPK_CHECK(bnpk_scan_launch(ctx, multi_first, n_rows, 1, multi_first, true, scan_scratch, s));
  const unsigned grid = grid_for(ceil_div(max_pieces, BNPK_BLOCK));
  for (size_t i = 0; i < groups.size(); ++i) {
    if (wide[i])
      BNPK_CHECK((ax_launch<uint64_t, Src>(ctx, src, d_offsets, n_rows, piece, n > piece, grid, piece_first, multi_first, groups[i], o, s)));
    else
      BNPK_CHECK((ax_launch<uint32_t, Src>(ctx, src, d_offsets, n_rows, piece, n > piece, grid, piece_first, multi_first, groups[i], o, s)));
  }
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_approx_rows_packed(bnpk_ctx* ctx, const bnpk_approx_library* h_lib, const uint64_t* d_packed, int64_t n_bases,
                            const int64_t* d_offsets, int64_t n_rows, uint8_t* d_dist, int64_t* d_start, int64_t* d_end,
                            uint8_t* d_overlap, int64_t* d_hits, void* stream) {
  const ax_packed src = {d_packed, n_bases};
  return ax_run<ax_packed>(ctx, h_lib, 4, 4, src, d_packed, d_offsets, n_rows, d_dist, d_start, d_end, d_overlap, d_hits,
                           "approx_rows_packed", (hipStream_t)stream);
}

int bnpk_approx_rows_bytes(bnpk_ctx* ctx, const bnpk_approx_library* h_lib, const uint8_t* d_codes, int64_t n,
                           const int64_t* d_offsets, int64_t n_rows, uint8_t* d_dist, int64_t* d_start, int64_t* d_end,
                           uint8_t* d_overlap, int64_t* d_hits, void* stream) {
  const ax_bytes src = {d_codes, n};
  return ax_run<ax_bytes>(ctx, h_lib, 1, BNPK_APPROX_MAX_ALPHABET, src, d_codes, d_offsets, n_rows, d_dist, d_start, d_end, d_overlap,
                          d_hits, "approx_rows_bytes", (hipStream_t)stream);
}

int bnpk_approx_trim_lens(bnpk_ctx* ctx, const int64_t* d_start, const int64_t* d_lens, int64_t n_rows, int64_t* d_out, void* stream) {
  if (!ctx || n_rows < 0 || (n_rows > 0 && (!d_start || !d_lens || !d_out))) return BNPK_ERR_ARG;
  if (n_rows == 0) return BNPK_OK;
  hipLaunchKernelGGL(ax_trim_kernel, dim3(grid_for(ceil_div(n_rows, 256))), dim3(256), 0, (hipStream_t)stream, d_start, d_lens, n_rows,
                     d_out);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
