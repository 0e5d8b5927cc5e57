// Barcode assignment (demultiplexing): the Hamming distance between a fixed window of every row and every barcode of a
// library, and per row the nearest barcode, its distance and the runner-up's (include/bnpk.h: bnpk_demux_rows_packed /
// bnpk_demux_rows_bytes), on the gfx950 matrix units.  Nothing reaches HBM but six bytes per row; DESIGN.md 4d.
//
//   The product.  With a position one-hot over A/C/G/T — one dword, 1u << (8 * code), so four i8 of which one is 1 —
//   matches(row, barcode) = onehot(window) . onehot(barcode) and distance = L - matches.  V_MFMA_I32_16X16X64_I8 takes
//   16 rows x 16 barcodes x 64 i8 = 16 positions (a K-STEP) in exact integer arithmetic; L <= 16 is one K-step, L <= 32 two.
//
//   Operands.  Lane l of a wavefront gives the instruction 16 bytes of A (row l % 16 of an A-TILE of 16 rows) and 16 of B
//   (barcode l % 16 of a TILE of 16 barcodes): here the positions 4 * (l / 16) .. + 3 of the K-step, a dword each.  Which of
//   the 64 K indices the hardware gives byte j of lane group l / 16 does not matter and is not relied on: it is the same
//   function for A and for B, and the product is a sum over K.  A position at or above L and a barcode at or above
//   n_barcodes are zero in B; a code >= 4 (_bytes) and every position of a row too short for the window are zero in A.
//   dx_library_kernel writes B for every (tile, K-step) once per call, 64 lanes x 16 bytes in lane order, so that an
//   operand is one 16-byte load per lane.
//
//   Split of work, dx_rows_kernel.  A workgroup of 4 wavefronts takes 256 rows, a wavefront 64 of them as 4 A-tiles; a
//   lane builds its A dwords once (16 VGPRs per K-step) and keeps them for the whole library.  The library then streams
//   through LDS in CHUNKS of 8 tiles, double-buffered: the workgroup's 256 lanes fetch chunk c + 1 into registers, all four
//   wavefronts work through chunk c out of LDS, the registers go to the other buffer, one barrier.  L2 is read once per
//   workgroup.  Per tile a wavefront issues 4 x KSTEPS matrix instructions; their accumulators start at 1, so that a key
//   (below) is never 0 and 0 can stand for "none".
//
//   Epilogue.  The result lane l holds for A-tile t is D[4 * (l / 16) + v][l % 16], v = 0 .. 3: four rows, one barcode.
//   Per (A-tile, v) the lane keeps the best as ONE word, (matches + 1) << 20 | (2^20 - 1 - barcode): a max keeps the smallest
//   index among equal distances; and the runner-up the same way: second = max(second, min(best, key)).  Keys of different
//   barcodes differ, so the second largest key carries the runner-up's matches.  The columns of the last tile at or above
//   n_barcodes enter as 0.  After the last tile the 16 lanes of a DPP row hold 16 states each for the same 16 rows: four
//   DPP exchanges (row_ror:8, row_half_mirror, quad_perm xor 2, xor 1) halve the states a lane keeps while they double
//   the barcodes a state covers — 15 merges of two (best, second) pairs instead of 64 — and leave lane l with the
//   finished state l % 16: every lane writes one row.  Short rows take the same path (their A is zero) and are overridden
//   at the write, so that a wavefront is whole at every matrix instruction.
#include "common.h"

namespace {

typedef int dx_v4i __attribute__((ext_vector_type(4)));

constexpr int DX_TILE = 16;                                  // barcodes per tile, rows per A-tile
constexpr int DX_A_TILES = 4;                                // A-tiles per wavefront
constexpr int DX_STATES = 4 * DX_A_TILES;                    // (best, second) pairs per lane
constexpr int DX_ROWS = BNPK_BLOCK / BNPK_WAVE * DX_A_TILES * DX_TILE;   // rows per workgroup: 256
constexpr int DX_CHUNK = 8;                                  // tiles per LDS buffer
constexpr int DX_INDEX_BITS = 20;
constexpr uint32_t DX_INDEX_MASK = (1u << DX_INDEX_BITS) - 1;
static_assert(BNPK_DEMUX_MAX_BARCODES <= (1 << DX_INDEX_BITS), "a barcode index fits the low bits of a key");
static_assert(BNPK_DEMUX_MAX_LEN <= 32, "two K-steps at most; a window is one 64-bit word of 2-bit codes");
static_assert(DX_ROWS == BNPK_BLOCK, "a lane writes one row");

struct dx_args {
  const dx_v4i* ops;                                         // B operands: [tile][K-step][lane], whole chunks
  const int64_t* off;
  int64_t n, n_rows, start;
  int n_barcodes, L, k, min_delta;
  int32_t* index; uint8_t* dist; uint8_t* second;
};

// codes: n_barcodes * L bytes -> ops (n_tiles tiles, a multiple of DX_CHUNK; what lies past the library is zero)
__global__ __launch_bounds__(256) void dx_library_kernel(const uint8_t* __restrict__ codes, int n_barcodes, int L, int ksteps,
                                                         int64_t n_tiles, dx_v4i* __restrict__ ops) {
  const int64_t total = n_tiles * ksteps * 64;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    const int ks = (int)((i >> 6) % ksteps);
    const int64_t b = (i >> 6) / ksteps * DX_TILE + (lane & 15);
    const int p0 = 16 * ks + 4 * (lane >> 4);
    dx_v4i w;
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = b < n_barcodes && p0 + j < L ? (int)(1u << (8 * codes[b * L + p0 + j])) : 0;
    ops[i] = w;
  }
}

// the A operand of one lane for one K-step: the positions p0 .. p0 + 3 of the window that starts at flat position g0
template <bool PACKED>
__device__ __forceinline__ dx_v4i dx_operand(const void* __restrict__ data, int64_t g0, uint64_t window, int p0, int L) {
  dx_v4i a;
  if (PACKED) {
    const uint32_t bits = (uint32_t)(window >> (2 * p0));    // (positions at or above L: whatever follows; B is zero there)
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = (int)(1u << (((bits >> (2 * j)) & 3) << 3));
  } else {
    const uint8_t* c = (const uint8_t*)data;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const unsigned code = p0 + j < L ? c[g0 + p0 + j] : 4u;
      a[j] = code < 4 ? (int)(1u << (8 * code)) : 0;
    }
  }
  return a;
}

// up to 32 2-bit codes from flat position g0 on, bit 0 upwards; the second word is read only where the window reaches it
__device__ __forceinline__ uint64_t dx_window(const uint64_t* __restrict__ W, int64_t g0, int L) {
  const int q = (int)(g0 & 31);
  uint64_t w = W[g0 >> 5] >> (2 * q);
  if (q + L > 32) w |= W[(g0 >> 5) + 1] << (64 - 2 * q);
  return w;
}

template <int CTRL>
__device__ __forceinline__ uint32_t dx_dpp(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false);
}

// the lanes of a pair (CTRL) hold N + N states of the same rows over disjoint sets of barcodes: the one with `upper` keeps
// the upper N and hands over the lower N, the other the other way round, and each merges what it gets into what it keeps
template <int N, int CTRL>
__device__ __forceinline__ void dx_halve(uint32_t (&best)[DX_STATES], uint32_t (&second)[DX_STATES], bool upper) {
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const uint32_t kb = upper ? best[i + N] : best[i], ks = upper ? second[i + N] : second[i];
    const uint32_t ob = dx_dpp<CTRL>(upper ? best[i] : best[i + N]), os = dx_dpp<CTRL>(upper ? second[i] : second[i + N]);
    second[i] = max(max(ks, os), min(kb, ob));
    best[i] = max(kb, ob);
  }
}

// one tile out of LDS: 4 x KSTEPS matrix instructions, and their accumulators into the lane's states.  LAST: the tile may
// reach past the library (a variant of its own, not a flag: the loop over the tiles before it then carries no select)
template <bool LAST, int KSTEPS>
__device__ __forceinline__ void dx_tile(const dx_v4i* buf, int lane, int tile, int n_barcodes, const dx_v4i (&A)[DX_A_TILES][KSTEPS],
                                        uint32_t (&best)[DX_STATES], uint32_t (&second)[DX_STATES]) {
  dx_v4i B[KSTEPS];
#pragma unroll
  for (int ks = 0; ks < KSTEPS; ++ks) B[ks] = buf[ks * 64 + lane];
  const int b = tile * DX_TILE + (lane & 15);
  const uint32_t inv = DX_INDEX_MASK - (uint32_t)b;
#pragma unroll
  for (int t = 0; t < DX_A_TILES; ++t) {
    dx_v4i acc = {1, 1, 1, 1};
#pragma unroll
    for (int ks = 0; ks < KSTEPS; ++ks) acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A[t][ks], B[ks], acc, 0, 0, 0);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      uint32_t key = ((uint32_t)acc[v] << DX_INDEX_BITS) | inv;
      if (LAST) key = b < n_barcodes ? key : 0u;
      second[4 * t + v] = max(second[4 * t + v], min(best[4 * t + v], key));
      best[4 * t + v] = max(best[4 * t + v], key);
    }
  }
}

template <bool PACKED, int KSTEPS>
__global__ __launch_bounds__(BNPK_BLOCK) void dx_rows_kernel(const void* __restrict__ data, dx_args a) {
  constexpr int CHUNK_WORDS = DX_CHUNK * KSTEPS * 64;        // 16-byte words per chunk
  constexpr int PER_LANE = CHUNK_WORDS / BNPK_BLOCK;
  __shared__ dx_v4i stage[2][CHUNK_WORDS];
  const int lane = lane_id(), col = lane & 15, grp = lane >> 4;
  const int n_tiles = (a.n_barcodes + DX_TILE - 1) / DX_TILE, n_chunks = (n_tiles + DX_CHUNK - 1) / DX_CHUNK;
  const int64_t need = a.start + a.L;
  for (int64_t first = (int64_t)blockIdx.x * DX_ROWS; first < a.n_rows; first += (int64_t)gridDim.x * DX_ROWS) {
    const int64_t base = first + wave_id() * (DX_A_TILES * DX_TILE);
    dx_v4i A[DX_A_TILES][KSTEPS];
#pragma unroll
    for (int t = 0; t < DX_A_TILES; ++t) {
      const int64_t r = base + t * DX_TILE + col;
      int64_t g0 = 0;
      bool whole = false;
      if (r < a.n_rows) {
        const int64_t s = a.off[r];
        whole = a.off[r + 1] - s >= need;
        g0 = s + a.start;
      }
      uint64_t window = 0;
      if (PACKED && whole) window = dx_window((const uint64_t*)data, g0, a.L);
#pragma unroll
      for (int ks = 0; ks < KSTEPS; ++ks) {
        const dx_v4i none = {0, 0, 0, 0};
        A[t][ks] = none;
        if (whole) A[t][ks] = dx_operand<PACKED>(data, g0, window, 16 * ks + 4 * grp, a.L);
      }
    }
    uint32_t best[DX_STATES], second[DX_STATES];
#pragma unroll
    for (int i = 0; i < DX_STATES; ++i) best[i] = second[i] = 0;

    dx_v4i next[PER_LANE];
#pragma unroll
    for (int i = 0; i < PER_LANE; ++i) stage[0][i * BNPK_BLOCK + threadIdx.x] = a.ops[i * BNPK_BLOCK + threadIdx.x];
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
      const bool more = c + 1 < n_chunks;
      if (more) {
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) next[i] = a.ops[(int64_t)(c + 1) * CHUNK_WORDS + i * BNPK_BLOCK + threadIdx.x];
      }
      const dx_v4i* buf = stage[c & 1];
      const int tile0 = c * DX_CHUNK, plain = more ? DX_CHUNK : n_tiles - 1 - tile0;      // (the last tile is in the last chunk)
      for (int tt = 0; tt < plain; ++tt)
        dx_tile<false, KSTEPS>(buf + tt * KSTEPS * 64, lane, tile0 + tt, a.n_barcodes, A, best, second);
      if (!more) dx_tile<true, KSTEPS>(buf + plain * KSTEPS * 64, lane, n_tiles - 1, a.n_barcodes, A, best, second);
      if (more) {
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) stage[(c + 1) & 1][i * BNPK_BLOCK + threadIdx.x] = next[i];
      }
      __syncthreads();                                       // chunk c + 1 is in place, and nobody reads chunk c any more
    }

    dx_halve<8, 0x128>(best, second, (col & 8) != 0);        // row_ror:8
    dx_halve<4, 0x141>(best, second, (col & 4) != 0);        // row_half_mirror
    dx_halve<2, 0x04e>(best, second, (col & 2) != 0);        // quad_perm:[2,3,0,1]
    dx_halve<1, 0x0b1>(best, second, (col & 1) != 0);        // quad_perm:[1,0,3,2]
    // state col = 4 * t + v of this lane group: row 16 * t + 4 * grp + v of the wavefront's
    const int64_t r = base + (col >> 2) * DX_TILE + 4 * grp + (col & 3);
    if (r < a.n_rows) {
      int index = -1, dist = BNPK_DEMUX_NONE, runner = BNPK_DEMUX_NONE;
      if (a.off[r + 1] - a.off[r] >= need) {
        dist = a.L + 1 - (int)(best[0] >> DX_INDEX_BITS);
        if (second[0]) runner = a.L + 1 - (int)(second[0] >> DX_INDEX_BITS);
        if (dist <= a.k && (!second[0] || runner - dist >= a.min_delta)) index = (int)(DX_INDEX_MASK - (best[0] & DX_INDEX_MASK));
      }
      a.index[r] = index;
      a.dist[r] = (uint8_t)dist;
      a.second[r] = (uint8_t)runner;
    }
  }
}

static inline size_t dx_align(size_t b) { return (b + 255) & ~(size_t)255; }

template <bool PACKED>
static int dx_run(bnpk_ctx* ctx, const bnpk_demux_library* lib, const void* d_data, int64_t n, const int64_t* d_offsets,
                  int64_t n_rows, int32_t* d_index, uint8_t* d_dist, uint8_t* d_second, const char* name, hipStream_t s) {
  if (!ctx || !lib || n < 0 || n_rows < 0) return BNPK_ERR_ARG;
  const int nb = lib->n_barcodes, L = lib->length;
  if (nb < 1 || nb > BNPK_DEMUX_MAX_BARCODES || L < 1 || L > BNPK_DEMUX_MAX_LEN || !lib->codes) return BNPK_ERR_ARG;
  if (lib->start < 0 || lib->max_mismatches < 0 || lib->max_mismatches > L || lib->min_delta < 0) return BNPK_ERR_ARG;
  const size_t n_codes = (size_t)nb * L;
  for (size_t i = 0; i < n_codes; ++i)
    if (lib->codes[i] >= 4) return BNPK_ERR_ARG;
  if (n_rows > 0 && (!d_offsets || !d_index || !d_dist || !d_second || (n > 0 && !d_data))) return BNPK_ERR_ARG;
  if (n_rows == 0) return BNPK_OK;
  const int ksteps = L > 16 ? 2 : 1;
  const int64_t n_tiles = ceil_div(ceil_div(nb, DX_TILE), DX_CHUNK) * DX_CHUNK;       // whole chunks: a chunk is fetched whole
  const size_t b_ops = (size_t)n_tiles * ksteps * 64 * sizeof(dx_v4i);
  void* scratch = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, b_ops + dx_align(n_codes), &scratch, s));
  dx_v4i* ops = (dx_v4i*)scratch;
  uint8_t* codes = (uint8_t*)scratch + b_ops;
  bnpk_timer t(ctx, name, s);
  BNPK_HIP(ctx, hipMemcpyAsync(codes, lib->codes, n_codes, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(dx_library_kernel, dim3(grid_for(ceil_div(n_tiles * ksteps * 64, 256))), dim3(256), 0, s, codes, nb, L, ksteps,
                     n_tiles, ops);
  BNPK_HIP(ctx, hipGetLastError());
  const dx_args a = {ops, d_offsets, n, n_rows, lib->start, nb, L, lib->max_mismatches, lib->min_delta, d_index, d_dist, d_second};
  const dim3 grid(grid_for(ceil_div(n_rows, DX_ROWS))), block(BNPK_BLOCK);
  if (ksteps == 1) hipLaunchKernelGGL((dx_rows_kernel<PACKED, 1>), grid, block, 0, s, d_data, a);
  else hipLaunchKernelGGL((dx_rows_kernel<PACKED, 2>), grid, block, 0, s, d_data, a);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_demux_rows_packed(bnpk_ctx* ctx, const bnpk_demux_library* h_lib, const uint64_t* d_packed, int64_t n_bases,
                           const int64_t* d_offsets, int64_t n_rows, int32_t* d_index, uint8_t* d_dist, uint8_t* d_second,
                           void* stream) {
  return dx_run<true>(ctx, h_lib, d_packed, n_bases, d_offsets, n_rows, d_index, d_dist, d_second, "demux_rows_packed",
                      (hipStream_t)stream);
}

int bnpk_demux_rows_bytes(bnpk_ctx* ctx, const bnpk_demux_library* h_lib, const uint8_t* d_codes, int64_t n, const int64_t* d_offsets,
                          int64_t n_rows, int32_t* d_index, uint8_t* d_dist, uint8_t* d_second, void* stream) {
  return dx_run<false>(ctx, h_lib, d_codes, n, d_offsets, n_rows, d_index, d_dist, d_second, "demux_rows_bytes", (hipStream_t)stream);
}

}  // extern "C"
