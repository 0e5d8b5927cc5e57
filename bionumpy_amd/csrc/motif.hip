// Class-and-gap motif matching over ragged rows (StringMatcher / MaskedStringMatcher / FixedLenRegexMatcher / RegexMatcher of
// bionumpy/sequence/string_matcher.py), gfx950.
//
//   The pattern arrives compiled (bnpk_motif, include/bnpk.h): segments of fixed positions, each position a class id or
//   "any", a gap range [a, b] between neighbouring segments, and the table of distinct classes.  Nothing is expanded into
//   alternatives: one pass, bit-parallel over the start positions.
//
//   Split of work.  Flat over the symbol positions of the column; flag i belongs to position i, so there is no ranking
//   scan.  A lane owns 32 consecutive starts and looks at most 63 symbols further: everything a lane handles is a 96-bit
//   plane (mo_p96), bit q = position q of the lane's stretch.
//
//   Class planes.  Bit q of a class plane: symbol q is in the class.
//     2-bit input: the lane's three packed words are unshuffled into the two bit planes of the codes, those give the four
//       one-hot planes, and a class plane is the OR of the one-hot planes its 4-bit set selects (the selection is
//       wave-uniform: masks in scalar registers).
//     byte input: a lane reads only its own 32 bytes (two 16-byte loads), looks each up in the 256-entry class-mask table
//       in LDS, and writes one 32-bit word per class to LDS as [class][lane]; the look-ahead of a lane are the words of
//       the next two lanes, for the last lanes of the workgroup those of a 64-byte halo the workgroup also converts.
//
//   Row ends.  A match lies inside one row.  N = ~E, E the row-end plane of bnpk_row_end_mask (bit on the last symbol of
//   every non-empty row): a stretch [i, i + n) crosses no row end iff N is set on [i, i + n - 1).  The row-count kernel
//   knows its row and builds N from the row's end instead.
//
//   Combine, right to left over the segments, for all 32 starts at once:
//     S_k(i)     = AND over the non-"any" positions j of segment k of plane[class(j)](i + j)
//     M_last(i)  = S_last(i) & N on [i, i + len_last - 1)
//     M_{k-1}(i) = S_{k-1}(i) & OR_{g = a..b} ( N on [i, i + len_{k-1} + g)  &  M_k(i + len_{k-1} + g) )
//   The gap's "N on [...)" is a running AND as g grows; the low 32 bits of M_0 are the lane's flags.  Shifts pull zeros in
//   at the top of the 96 bits; with a span of at most 64 no flag of the 32 starts depends on them.
#include "common.h"

namespace {

constexpr int MO_ANY = BNPK_MOTIF_ANY;
constexpr int MO_CHUNK = 32;                                 // starts per lane
constexpr int MO_TILE_CHUNKS = BNPK_BLOCK;                   // byte kernel: chunks of a workgroup (8192 symbols), plus two of halo
constexpr int MO_LONG = 4096, MO_PIECE = 1024;               // row counts: rows of more symbols are taken by the whole wavefront, a piece per lane

// the program as the kernels read it (by value: every index into it is wave-uniform, so it is read with scalar loads)
struct mo_prog {
  int32_t n_seg, n_pos, min_span, pad;
  uint32_t seg[BNPK_MOTIF_MAX_SPAN];                         // length | gap_min << 8 | gap_max << 16 (the gap BEHIND the segment)
  uint32_t pos[BNPK_MOTIF_MAX_SPAN];                         // class id or MO_ANY, the segments' positions one after the other
  uint64_t set4;                                             // 2-bit input: four bits per class, bit c = code c is in it
};
struct mo_table { uint16_t m[256]; };                        // byte input: bit k of entry v = byte value v is in class k

// ---- 96-bit planes ---------------------------------------------------------------------------------------------------------
struct mo_p96 { uint32_t w0, w1, w2; };
__device__ __forceinline__ mo_p96 operator&(mo_p96 a, mo_p96 b) { return {a.w0 & b.w0, a.w1 & b.w1, a.w2 & b.w2}; }
__device__ __forceinline__ mo_p96 operator|(mo_p96 a, mo_p96 b) { return {a.w0 | b.w0, a.w1 | b.w1, a.w2 | b.w2}; }
__device__ __forceinline__ mo_p96 operator~(mo_p96 a) { return {~a.w0, ~a.w1, ~a.w2}; }
// a >> j, 0 <= j < 96, j wave-uniform
__device__ __forceinline__ mo_p96 shr(mo_p96 a, int j) {
  if (j >= 64) return {a.w2 >> (j - 64), 0u, 0u};
  if (j >= 32) return {__builtin_amdgcn_alignbit(a.w2, a.w1, j - 32), a.w2 >> (j - 32), 0u};
  return {__builtin_amdgcn_alignbit(a.w1, a.w0, j), __builtin_amdgcn_alignbit(a.w2, a.w1, j), a.w2 >> j};
}
__device__ __forceinline__ uint32_t ones32(int64_t n) { return n <= 0 ? 0u : n >= 32 ? ~0u : (1u << (int)n) - 1u; }
__device__ __forceinline__ mo_p96 low_ones(int64_t n) { return {ones32(n), ones32(n - 32), ones32(n - 64)}; }

// bit i: N is set on [i, i + n); n wave-uniform (doubling: at most seven shifts for n <= 95)
__device__ __forceinline__ mo_p96 run_free(mo_p96 N, int n) {
  if (n <= 0) return {~0u, ~0u, ~0u};
  mo_p96 r = N;
  int have = 1;
  for (; 2 * have <= n; have *= 2) r = r & shr(r, have);
  if (have < n) r = r & shr(r, n - have);
  return r;
}

// the flags of the lane's 32 starts; plane(k): the plane of class k
template <class F>
__device__ __forceinline__ uint32_t mo_combine(const mo_prog& P, F plane, mo_p96 N) {
  mo_p96 M = {0u, 0u, 0u};
  int first = P.n_pos;
  for (int k = P.n_seg - 1; k >= 0; --k) {
    const uint32_t s = P.seg[k];
    const int len = (int)(s & 0xffu), a = (int)((s >> 8) & 0xffu), b = (int)((s >> 16) & 0xffu);
    first -= len;
    mo_p96 S = {~0u, ~0u, ~0u};
    for (int j = 0; j < len; ++j) {
      const int c = (int)P.pos[first + j];
      if (c != MO_ANY) S = S & shr(plane(c), j);
    }
    if (k == P.n_seg - 1) {
      M = S & run_free(N, len - 1);
    } else {
      mo_p96 R = run_free(N, len + a), T = {0u, 0u, 0u};
      for (int g = a; g <= b; ++g) {
        T = T | (R & shr(M, len + g));
        R = R & shr(N, len + g);
      }
      M = S & T;
    }
  }
  return M.w0;
}

// ---- 2-bit input ----------------------------------------------------------------------------------------------------------------
// sixteen 2-bit codes -> their low bits in the low half, their high bits in the high half (a perfect unshuffle)
__device__ __forceinline__ uint32_t unshuffle16(uint32_t x) {
  uint32_t t;
  t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
  t = (x ^ (x >> 2)) & 0x0c0c0c0cu; x ^= t ^ (t << 2);
  t = (x ^ (x >> 4)) & 0x00f000f0u; x ^= t ^ (t << 4);
  t = (x ^ (x >> 8)) & 0x0000ff00u; x ^= t ^ (t << 8);
  return x;
}
// 32 codes of a packed word -> (plane of their low bits, plane of their high bits)
__device__ __forceinline__ void code_planes(uint64_t w, uint32_t& b0, uint32_t& b1) {
  const uint32_t lo = unshuffle16((uint32_t)w), hi = unshuffle16((uint32_t)(w >> 32));
  b0 = (lo & 0xffffu) | (hi << 16);
  b1 = (lo >> 16) | (hi & 0xffff0000u);
}

struct mo_onehot {
  mo_p96 c[4];                                               // A C G T = codes 0 1 2 3
  __device__ __forceinline__ mo_onehot(uint64_t x0, uint64_t x1, uint64_t x2) {
    mo_p96 b0, b1;
    code_planes(x0, b0.w0, b1.w0);
    code_planes(x1, b0.w1, b1.w1);
    code_planes(x2, b0.w2, b1.w2);
    c[0] = ~b1 & ~b0; c[1] = ~b1 & b0; c[2] = b1 & ~b0; c[3] = b1 & b0;
  }
  // the OR of the one-hot planes the class's 4-bit set selects
  __device__ __forceinline__ mo_p96 plane(uint64_t set4, int k) const {
    const uint32_t set = (uint32_t)(set4 >> (4 * k));
    const uint32_t m0 = 0u - (set & 1u), m1 = 0u - ((set >> 1) & 1u), m2 = 0u - ((set >> 2) & 1u), m3 = 0u - ((set >> 3) & 1u);
    return {(c[0].w0 & m0) | (c[1].w0 & m1) | (c[2].w0 & m2) | (c[3].w0 & m3),
            (c[0].w1 & m0) | (c[1].w1 & m1) | (c[2].w1 & m2) | (c[3].w1 & m3),
            (c[0].w2 & m0) | (c[1].w2 & m1) | (c[2].w2 & m2) | (c[3].w2 & m3)};
  }
};

// 32 flags -> 32 bytes of 0 / 1 at out + p (p a multiple of 32, out 16-byte aligned); n < 32: only the first n
__device__ __forceinline__ void store_flags(uint8_t* __restrict__ out, int64_t p, int64_t n, uint32_t f) {
  uint32_t o[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) o[q] = (((f >> (4 * q)) & 0xfu) * 0x00204081u) & 0x01010101u;   // bit b of a nibble -> byte b
  if (n >= MO_CHUNK) {
    *reinterpret_cast<uint4*>(out + p) = make_uint4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<uint4*>(out + p + 16) = make_uint4(o[4], o[5], o[6], o[7]);
  } else {
    for (int j = 0; j < (int)n; ++j) out[p + j] = (uint8_t)((f >> j) & 1u);
  }
}

// the row-end plane of the chunk's 96 positions, complemented (E32: n_e 32-bit words)
__device__ __forceinline__ mo_p96 not_row_ends(const uint32_t* __restrict__ E32, int64_t n_e, int64_t chunk) {
  auto e = [&](int64_t i) -> uint32_t { return i < n_e ? E32[i] : 0u; };
  return {~e(chunk), ~e(chunk + 1), ~e(chunk + 2)};
}

__global__ __launch_bounds__(BNPK_BLOCK) void mo_flags_packed_kernel(const uint64_t* __restrict__ W, int64_t n_words,
                                                                    const uint32_t* __restrict__ E32, int64_t n_e, int64_t total,
                                                                    mo_prog P, uint8_t* __restrict__ out) {
  const int64_t n_chunks = (total + MO_CHUNK - 1) / MO_CHUNK;
  for (int64_t c = (int64_t)blockIdx.x * BNPK_BLOCK + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * BNPK_BLOCK) {
    auto word = [&](int64_t i) -> uint64_t { return i < n_words ? W[i] : 0ull; };
    const mo_onehot H(word(c), word(c + 1), word(c + 2));     // the chunk is word c: bases 32 c .. 32 c + 95
    const uint64_t set4 = P.set4;
    const uint32_t f = mo_combine(P, [&](int k) { return H.plane(set4, k); }, not_row_ends(E32, n_e, c));
    const int64_t left = total - c * MO_CHUNK;
    store_flags(out, c * MO_CHUNK, left, f & ones32(left));
  }
}

// ---- 2-bit input, counted per row ---------------------------------------------------------------------------------------------
// starts [p, p + n_starts) of a row that ends at `end` (exclusive): how many match
__device__ __forceinline__ unsigned mo_count(const uint64_t* __restrict__ W, int64_t n_words, int64_t p, int64_t n_starts,
                                             int64_t end, const mo_prog& P) {
  if (n_starts <= 0) return 0u;
  int64_t wi = p >> 5;
  const int sh = 2 * (int)(p & 31);
  auto word = [&](int64_t i) -> uint64_t { return i < n_words ? W[i] : 0ull; };
  auto funnel = [&](uint64_t lo, uint64_t hi) -> uint64_t { return sh ? (lo >> sh) | (hi << (64 - sh)) : lo; };
  uint64_t w0 = word(wi), w1 = word(wi + 1), w2 = word(wi + 2);
  const uint64_t set4 = P.set4;
  unsigned n = 0;
  for (int64_t done = 0; done < n_starts; done += MO_CHUNK) {
    const uint64_t w3 = word(wi + 3);
    const mo_onehot H(funnel(w0, w1), funnel(w1, w2), funnel(w2, w3));      // bases p + done .. + 95
    // the row's last symbol, and whatever lies behind it, ends every window: N is set in front of it only
    const mo_p96 N = low_ones(end - 1 - (p + done));
    const uint32_t f = mo_combine(P, [&](int k) { return H.plane(set4, k); }, N);
    n += __popc(f & ones32(n_starts - done));
    w0 = w1; w1 = w2; w2 = w3;
    ++wi;
  }
  return n;
}

__global__ __launch_bounds__(BNPK_BLOCK) void mo_rows_packed_kernel(const uint64_t* __restrict__ W, int64_t n_words,
                                                                   const int64_t* __restrict__ off, int64_t n_rows, mo_prog P,
                                                                   int64_t* __restrict__ counts) {
  const int lane = lane_id();
  const int64_t n_groups = (n_rows + 63) / 64;
  for (int64_t g = (int64_t)blockIdx.x * (BNPK_BLOCK / 64) + wave_id(); g < n_groups; g += (int64_t)gridDim.x * (BNPK_BLOCK / 64)) {
    const int64_t r = g * 64 + lane;
    const int64_t lo = r < n_rows ? off[r] : 0, hi = r < n_rows ? off[r + 1] : 0;
    const int64_t n_starts = hi - lo - (P.min_span - 1);      // (later starts cannot hold the shortest match)
    const bool is_long = hi - lo > MO_LONG;
    int64_t n = is_long ? 0 : (int64_t)mo_count(W, n_words, lo, n_starts, hi, P);
    uint64_t todo = __ballot(is_long);
    while (todo) {                                             // (uniform: every lane sees the same ballot)
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const int64_t rlo = __shfl((long long)lo, src), rhi = __shfl((long long)hi, src), rstarts = __shfl((long long)n_starts, src);
      int64_t part = 0;
      for (int64_t c = (int64_t)lane * MO_PIECE; c < rstarts; c += 64 * MO_PIECE)
        part += mo_count(W, n_words, rlo + c, min((int64_t)MO_PIECE, rstarts - c), rhi, P);
      part = __shfl(wave_reduce_sum(part), 0);
      if (lane == src) n = part;
    }
    if (r < n_rows) counts[r] = n;
  }
}

// ---- byte input -----------------------------------------------------------------------------------------------------------------
// NC: the classes a lane transposes (the program's class count rounded up to 4 or 16)
template <int NC>
__global__ __launch_bounds__(BNPK_BLOCK) void mo_flags_bytes_kernel(const uint8_t* __restrict__ in, const uint32_t* __restrict__ E32,
                                                                   int64_t n_e, int64_t total, mo_prog P, mo_table T,
                                                                   uint8_t* __restrict__ out) {
  __shared__ uint16_t tab[256];
  __shared__ uint32_t planes[NC][MO_TILE_CHUNKS + 2];
  tab[threadIdx.x] = T.m[threadIdx.x];
  __syncthreads();
  const int64_t chunk0 = (int64_t)blockIdx.x * MO_TILE_CHUNKS;
  for (int c = threadIdx.x; c < MO_TILE_CHUNKS + 2; c += BNPK_BLOCK) {      // the lane's own chunk; lanes 0 and 1: the halo too
    const int64_t base = (chunk0 + c) * MO_CHUNK;
    const int64_t left = total - base;
    uint32_t x[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (left >= MO_CHUNK) {
      const uint4 lo = *reinterpret_cast<const uint4*>(in + base), hi = *reinterpret_cast<const uint4*>(in + base + 16);
      x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    } else {
      for (int j = 0; j < (int)left; ++j) x[j >> 2] |= (uint32_t)in[base + j] << (8 * (j & 3));
    }
    uint32_t pl[NC];
#pragma unroll
    for (int k = 0; k < NC; ++k) pl[k] = 0u;
#pragma unroll
    for (int q = 0; q < MO_CHUNK; ++q) {
      const uint32_t m = tab[(x[q >> 2] >> (8 * (q & 3))) & 0xffu];
#pragma unroll
      for (int k = 0; k < NC; ++k) pl[k] |= ((m >> k) & 1u) << q;
    }
    const uint32_t valid = ones32(left);                       // (what lies behind the column is in no class)
#pragma unroll
    for (int k = 0; k < NC; ++k) planes[k][c] = pl[k] & valid;
  }
  __syncthreads();
  const int64_t c = chunk0 + threadIdx.x;
  const int64_t left = total - c * MO_CHUNK;
  if (left <= 0) return;
  const int t = threadIdx.x;
  const uint32_t f = mo_combine(P, [&](int k) { return mo_p96{planes[k][t], planes[k][t + 1], planes[k][t + 2]}; },
                                not_row_ends(E32, n_e, c));
  store_flags(out, c * MO_CHUNK, left, f & ones32(left));
}

// ---- the program: checked, and put into the kernels' form (host) -------------------------------------------------------------------
static int mo_prepare(const bnpk_motif* m, mo_prog* P, mo_table* T) {
  if (m->n_segments < 1 || m->n_segments > BNPK_MOTIF_MAX_SPAN || m->n_classes < 0 || m->n_classes > BNPK_MOTIF_MAX_CLASSES)
    return BNPK_ERR_ARG;
  memset(P, 0, sizeof(*P));
  int n_pos = 0, span = 0, min_span = 0;
  for (int k = 0; k < m->n_segments; ++k) {
    const int len = m->seg_len[k], a = k + 1 < m->n_segments ? m->gap_min[k] : 0, b = k + 1 < m->n_segments ? m->gap_max[k] : 0;
    if (len < 1 || a > b) return BNPK_ERR_ARG;
    span += len + b;
    min_span += len + a;
    if (span > BNPK_MOTIF_MAX_SPAN) return BNPK_ERR_RANGE;
    P->seg[k] = (uint32_t)len | ((uint32_t)a << 8) | ((uint32_t)b << 16);
    for (int j = 0; j < len; ++j, ++n_pos) {
      const int c = m->pos_class[n_pos];
      if (c != BNPK_MOTIF_ANY && c >= m->n_classes) return BNPK_ERR_ARG;
      P->pos[n_pos] = (uint32_t)c;
    }
  }
  P->n_seg = m->n_segments;
  P->n_pos = n_pos;
  P->min_span = min_span;
  for (int k = 0; k < m->n_classes; ++k) P->set4 |= (uint64_t)(m->class_set4[k] & 0xfu) << (4 * k);
  if (T) memcpy(T->m, m->class_mask, sizeof(T->m));
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_motif_flags_packed(bnpk_ctx* ctx, const uint64_t* d_packed, const uint64_t* d_row_ends, int64_t n_bases,
                            const bnpk_motif* h_motif, uint8_t* d_flags, void* stream) {
  if (!ctx || n_bases < 0 || !h_motif) return BNPK_ERR_ARG;
  mo_prog P;
  BNPK_CHECK(mo_prepare(h_motif, &P, nullptr));
  if (n_bases == 0) return BNPK_OK;
  if (!d_packed || !d_row_ends || !d_flags) return BNPK_ERR_ARG;
  if ((uintptr_t)d_flags & 15u) return BNPK_ERR_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "motif_flags_packed", s);
  hipLaunchKernelGGL(mo_flags_packed_kernel, dim3(grid_for(ceil_div(ceil_div(n_bases, MO_CHUNK), BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s,
                     d_packed, n_bases / 32 + 2, reinterpret_cast<const uint32_t*>(d_row_ends), 2 * (n_bases / 64 + 2), n_bases, P,
                     d_flags);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_motif_flags_bytes(bnpk_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_row_ends, int64_t n_bytes,
                           const bnpk_motif* h_motif, uint8_t* d_flags, void* stream) {
  if (!ctx || n_bytes < 0 || !h_motif) return BNPK_ERR_ARG;
  mo_prog P;
  mo_table T;
  BNPK_CHECK(mo_prepare(h_motif, &P, &T));
  if (n_bytes == 0) return BNPK_OK;
  if (!d_bytes || !d_row_ends || !d_flags) return BNPK_ERR_ARG;
  if (((uintptr_t)d_flags | (uintptr_t)d_bytes) & 15u) return BNPK_ERR_ALIGN;
  const int64_t n_tiles = ceil_div(n_bytes, (int64_t)MO_TILE_CHUNKS * MO_CHUNK);
  if (n_tiles > BNPK_MAX_BLOCKS) return BNPK_ERR_RANGE;
  hipStream_t s = (hipStream_t)stream;
  const uint32_t* ends = reinterpret_cast<const uint32_t*>(d_row_ends);
  bnpk_timer t(ctx, "motif_flags_bytes", s);
  if (h_motif->n_classes <= 4)
    hipLaunchKernelGGL(mo_flags_bytes_kernel<4>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_bytes, ends, 2 * (n_bytes / 64 + 2),
                       n_bytes, P, T, d_flags);
  else
    hipLaunchKernelGGL(mo_flags_bytes_kernel<16>, dim3((unsigned)n_tiles), dim3(BNPK_BLOCK), 0, s, d_bytes, ends, 2 * (n_bytes / 64 + 2),
                       n_bytes, P, T, d_flags);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_motif_rows_packed(bnpk_ctx* ctx, const uint64_t* d_packed, int64_t n_bases, const int64_t* d_offsets, int64_t n_rows,
                           const bnpk_motif* h_motif, int64_t* d_counts, void* stream) {
  if (!ctx || n_bases < 0 || n_rows < 0 || !h_motif) return BNPK_ERR_ARG;
  mo_prog P;
  BNPK_CHECK(mo_prepare(h_motif, &P, nullptr));
  if (n_rows == 0) return BNPK_OK;
  if (!d_offsets || !d_counts || (n_bases > 0 && !d_packed)) return BNPK_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "motif_rows_packed", s);
  hipLaunchKernelGGL(mo_rows_packed_kernel, dim3(grid_for(ceil_div(n_rows, (int64_t)BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_packed,
                     ceil_div(n_bases, (int64_t)32), d_offsets, n_rows, P, d_counts);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
