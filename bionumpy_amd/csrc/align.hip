// Pairwise alignment with affine gaps (Gotoh): score, ends and the path of every pair of rows (bnpk_align_pairs_packed / _bytes),
// and the paths as CIGAR columns (bnpk_align_cigar).  The semantics are those of include/bnpk.h; DESIGN.md 4d.
//
//   Split.  A pair belongs to a group of G lanes, lane l of the group owns the query rows l R + 1 .. l R + R and keeps their H
//   and E in registers (2 R words), with the score row of each of its query symbols next to them.  The lanes are a skewed
//   pipeline over the target's columns: at step s lane l works on column s - l + 1, top to bottom through its strip, and
//   hands the H and the F of its last row to lane l + 1 with ONE DPP move each (row_shr:1 inside a row of 16 lanes,
//   wave_shr:1 across the wavefront); the lane a move has no source for keeps the `old` operand, which is row 0 of the matrix.
//   No DP value goes through LDS or HBM.  Two size classes: G = 16, R = 10 (queries of up to 160 rows, four pairs per
//   wavefront: 15 steps of fill and drain) and G = 64, R = 8 (up to 512).  al_classify_kernel sorts the pairs of a call into
//   the two from the row offsets: one list, the small class from its front and the large one from its back.
//
//   Symbols.  A group stages its target in LDS as code bytes (the only place where _packed and _bytes differ, with the fetch
//   of the lane's query symbols): every lane reads the byte of its column, neighbours read neighbouring bytes.  The score of
//   a cell is V_BFE_I32 out of the lane's word of four scores on the 2-bit path, one LDS byte of the (A + 1) x (A + 1) table
//   on the byte path, whose last row and column hold the smallest entry (a code >= A is clamped to A).
//
//   Score.  int32 throughout: 512 x 127 does not fit 16 bits.  Local: a cell's key is h << 10 | 1023 - i (h < 2^17), a row
//   beyond the query has the sign bit in its constant, V_MAX3 folds a column, and one compare per column keeps the first
//   column of the largest key: largest h, smallest i, smallest j, and across lanes the keys differ (a row has one owner).
//
//   Traceback.  Four bits per cell (source of H: diagonal, E, F, stop; E opened; F opened), a lane's column in one 32-bit
//   word (R = 8) or a word and a byte (R = 10), in LDS only: word (lane L, column c) at L CAP + c + 16 (L / G).  At a step
//   lane l stores column s - l, so the bank is s - l + 16 pair (G = 16, CAP = 160) or s + 511 L (G = 64, CAP = 512) modulo
//   32: every bank takes two of the 64 stores, the least possible.  That is 128 KB for a 512 x 512 pair and 12.8 KB for a
//   pair of the small class (both sides <= 160; a longer target puts a short query into the large class when the path is
//   asked for).  The lane that owns the end walks back through LDS and writes 2 bits per step into the pair's slot.
//   Without traceback the kernel has neither the bits nor the walk.
//
//   No matrix instructions: the recurrence is a wavefront of dependent max-plus steps on one pair; nothing is a product.
#include <algorithm>

#include "common.h"

namespace {

constexpr int AL_NEG = -(1 << 29);                           // "does not exist": survives 512 subtractions of 127
constexpr int AL_SMALL_R = 10, AL_LARGE_R = 8;
constexpr int AL_SMALL = 16 * AL_SMALL_R;                    // rows of a query of the small class; columns too, with traceback
constexpr int AL_TABLE = BNPK_APPROX_MAX_ALPHABET + 1;       // the byte path's table: one row and column more than letters
constexpr int AL_TABLE_BYTES = (AL_TABLE * AL_TABLE + 15) / 16 * 16;
constexpr int AL_STEPS_AT = BNPK_ALIGN_PATH_WORDS - 1;       // the word of a slot that holds the number of steps
static_assert(BNPK_ALIGN_MAX_LEN == 64 * AL_LARGE_R, "64 lanes of R rows hold the longest query");
static_assert(2 * BNPK_ALIGN_MAX_LEN <= 16 * AL_STEPS_AT, "a path has at most n + m steps of 2 bits");

struct al_args {
  const void* q; const int64_t* qoff;
  const void* t; const int64_t* toff;
  int64_t first, n_pairs;
  int one_target, go, ge, A;
  uint32_t rows4[4];                                         // _packed: the four scores of a query code, one byte each
  const int8_t* table;                                       // _bytes: AL_TABLE x AL_TABLE in HBM
  int32_t* list; int32_t* counts;                            // the pairs by class (relative to first), and how many
  int32_t* score; int32_t* qend; int32_t* tend; int32_t* qstart; int32_t* tstart;
  int64_t* runs; uint32_t* paths;
  unsigned long long* error;
};

__global__ void al_reset_kernel(int32_t* counts) {
  if (threadIdx.x < 2) counts[threadIdx.x] = 0;
}

template <bool TB>
__global__ __launch_bounds__(BNPK_BLOCK) void al_classify_kernel(al_args p) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < p.n_pairs; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t pair = p.first + k, trow = p.one_target ? 0 : pair;
    const int64_t n = p.qoff[pair + 1] - p.qoff[pair], m = p.toff[trow + 1] - p.toff[trow];
    if (n < 0 || m < 0 || n > BNPK_ALIGN_MAX_LEN || m > BNPK_ALIGN_MAX_LEN) {
      atomicMin(p.error, (unsigned long long)pair);
      p.score[pair] = p.qend[pair] = p.tend[pair] = 0;
      if (TB) {
        p.qstart[pair] = p.tstart[pair] = 0;
        p.runs[pair] = 0;
        p.paths[k * BNPK_ALIGN_PATH_WORDS + AL_STEPS_AT] = 0;
      }
      continue;
    }
    const int large = n > AL_SMALL || (TB && m > AL_SMALL);
    const int32_t at = atomicAdd(&p.counts[large], 1);
    p.list[large ? p.n_pairs - 1 - at : at] = (int32_t)k;
  }
}

template <bool PACKED>
__device__ __forceinline__ uint32_t al_code(const void* __restrict__ data, int64_t pos) {
  if (PACKED) return (uint32_t)(((const uint64_t*)data)[pos >> 5] >> (2 * (int)(pos & 31))) & 3u;
  return ((const uint8_t*)data)[pos];
}

template <int G>
__device__ __forceinline__ int al_from_above(int boundary, int v) {      // lane l - 1's v; the group's first lane: boundary
  return __builtin_amdgcn_update_dpp(boundary, v, G == 16 ? 0x111 : 0x138, 0xf, 0xf, false);
}

__device__ __forceinline__ void al_wave_sync() {             // the wavefront's LDS writes before this are seen by its reads after
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <bool PACKED, int G, bool TB>
struct al_cfg {
  static constexpr int R = G == 16 ? AL_SMALL_R : AL_LARGE_R;
  static constexpr int PPW = BNPK_WAVE / G;                                  // pairs per wavefront
  static constexpr int TCAP = (G == 16 && TB) ? AL_SMALL : BNPK_ALIGN_MAX_LEN;   // target symbols staged per pair
  static constexpr int CAP = G == 16 ? AL_SMALL : BNPK_ALIGN_MAX_LEN;        // columns of traceback bits per lane
  static constexpr int B_TABLE = PACKED ? 0 : AL_TABLE_BYTES;
  static constexpr int B_TARGET = PPW * TCAP;
  static constexpr int B_WORDS = TB ? 4 * (BNPK_WAVE * CAP + 16 * (PPW - 1)) : 0;
  static constexpr int B_BYTES = (TB && R > 8) ? BNPK_WAVE * CAP : 0;
  static constexpr int LDS = B_TABLE + B_TARGET + B_WORDS + B_BYTES;
};

// one wavefront per workgroup; MODE: BNPK_ALIGN_LOCAL / _SEMIGLOBAL / _GLOBAL
template <bool PACKED, int G, int MODE, bool TB>
__global__ __launch_bounds__(BNPK_WAVE) void al_dp_kernel(al_args p) {
  using cfg = al_cfg<PACKED, G, TB>;
  constexpr int R = cfg::R, PPW = cfg::PPW, TCAP = cfg::TCAP, CAP = cfg::CAP;
  constexpr bool LOCAL = MODE == BNPK_ALIGN_LOCAL, GLOBAL = MODE == BNPK_ALIGN_GLOBAL;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int8_t* const tab = (int8_t*)smem;
  uint8_t* const T = smem + cfg::B_TABLE;
  uint32_t* const W = (uint32_t*)(smem + cfg::B_TABLE + cfg::B_TARGET);      // (B_TABLE and B_TARGET are multiples of 16)
  uint8_t* const B = smem + cfg::B_TABLE + cfg::B_TARGET + cfg::B_WORDS;
  BNPK_VGPR_FLOOR_32();
  const int lane = threadIdx.x, l = lane % G, pw = lane / G;
  const int go = p.go, ge = p.ge, goe = go + ge, A1 = p.A + 1;
  const int total = p.counts[G == 16 ? 0 : 1];
  if (!PACKED) {
    for (int i = lane; i < AL_TABLE_BYTES / 4; i += BNPK_WAVE) ((uint32_t*)tab)[i] = ((const uint32_t*)p.table)[i];
  }
  uint8_t* const Tp = T + pw * TCAP;
  uint32_t* const Wl = W + lane * CAP + 16 * pw;
  uint8_t* const Bl = B + lane * CAP;
  for (int64_t slot = blockIdx.x; slot * PPW < total; slot += gridDim.x) {
    const int64_t k = slot * PPW + pw;
    const bool have = k < total;
    const int64_t rel = have ? p.list[G == 16 ? k : p.n_pairs - 1 - k] : 0;
    const int64_t pair = p.first + rel, trow = p.one_target ? 0 : pair;
    const int64_t qg = p.qoff[pair], tg = p.toff[trow];
    const int n = have ? (int)(p.qoff[pair + 1] - qg) : 0, m = have ? (int)(p.toff[trow + 1] - tg) : 0;
    al_wave_sync();                                          // (the pair before is done with T and the bits)
    for (int c = l; c < m; c += G) {
      const uint32_t code = al_code<PACKED>(p.t, tg + c);
      Tp[c] = (uint8_t)(PACKED ? code : min(code, (uint32_t)p.A));
    }
    // the lane's strip: rows i0 + 1 .. i0 + R
    const int i0 = l * R;
    int H[R], E[R], qs[R], ck[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int i = i0 + r + 1;
      const uint32_t code = i <= n ? al_code<PACKED>(p.q, qg + i - 1) : 0u;
      if (PACKED) qs[r] = (int)(code == 0 ? p.rows4[0] : code == 1 ? p.rows4[1] : code == 2 ? p.rows4[2] : p.rows4[3]);
      else qs[r] = (int)min(code, (uint32_t)p.A) * A1;
      H[r] = LOCAL ? 0 : -(go + i * ge);
      E[r] = AL_NEG;
      ck[r] = i <= n ? 1023 - i : (int)0x80000000u;
    }
    const int nl = (n + R - 1) / R;                          // lanes with rows
    const int last = n > 0 ? (n - 1) / R : 0, rn = n - 1 - last * R;         // the lane and the register of row n
    const bool lane_on = l < nl, owns_n = have && l == last;
    const int steps = (int)wave_max((unsigned)((n > 0 && m > 0) ? m + nl - 1 : 0));
    int diag = (LOCAL || i0 == 0) ? 0 : -(go + i0 * ge);     // H[i0][0]
    int bot_h = 0, bot_f = AL_NEG;
    int bestk = 0, bestj = 0;                                // local: the key and its column
    int hn = n > 0 ? (LOCAL ? 0 : -(go + n * ge)) : 0;       // H[n][j] of the owner's last column
    int best = hn;                                           // semiglobal: the largest H[n][j], at bestj
    al_wave_sync();
    for (int s = 0; s < steps; ++s) {
      const int j = s - l + 1;
      const int up_h = al_from_above<G>(GLOBAL ? -(go + j * ge) : 0, bot_h);
      const int up_f = al_from_above<G>(AL_NEG, bot_f);
      if (lane_on && j >= 1 && j <= m) {
        const int tc = Tp[j - 1];
        int up = up_h, f = up_f, d = diag, colk = (int)0x80000000u;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int sc = PACKED ? (int)((int32_t)((uint32_t)qs[r] << (24 - 8 * tc)) >> 24) : (int)tab[qs[r] + tc];
          const int eo = H[r] - goe, ee = E[r] - ge, e = max(eo, ee);
          const int fo = up - goe, fe = f - ge;
          f = max(fo, fe);
          const int hd = d + sc;
          int h = max(hd, max(e, f));
          if (LOCAL) h = max(h, 0);
          if (TB) {
            const uint32_t src = (LOCAL && h == 0) ? 3u : hd == h ? 0u : e == h ? 1u : 2u;
            const uint32_t nib = src | (eo >= ee ? 4u : 0u) | (fo >= fe ? 8u : 0u);
            if (r < 8) lo |= nib << (4 * r); else hi |= nib << (4 * (r - 8));
          }
          d = H[r];
          H[r] = h;
          E[r] = e;
          up = h;
          if (LOCAL) colk = max(colk, (h << 10) | ck[r]);
          else if (r == rn) hn = h;
        }
        bot_h = up;
        bot_f = f;
        diag = up_h;
        if (TB) {
          Wl[j - 1] = lo;
          if (R > 8) Bl[j - 1] = (uint8_t)hi;
        }
        if (LOCAL) {
          if (colk > bestk) { bestk = colk; bestj = j; }
        } else if (!GLOBAL) {
          if (hn > best) { best = hn; bestj = j; }
        }
      }
    }
    // the end, and the lane that owns it
    int score, qe, te;
    bool owner;
    if (LOCAL) {
      int gk = bestk;
#pragma unroll
      for (int dd = 1; dd < G; dd <<= 1) gk = max(gk, __shfl_xor(gk, dd, BNPK_WAVE));
      score = gk >> 10;
      owner = have && (score > 0 ? bestk == gk : l == 0);
      qe = score > 0 ? 1023 - (gk & 1023) : 0;
      te = score > 0 ? bestj : 0;
    } else if (GLOBAL) {
      owner = owns_n;
      score = n > 0 ? hn : (m > 0 ? -(go + m * ge) : 0);
      qe = n;
      te = m;
    } else {
      owner = owns_n;
      score = n > 0 ? best : 0;
      qe = n;
      te = n > 0 ? bestj : 0;
    }
    if (TB) al_wave_sync();
    if (owner) {
      p.score[pair] = score;
      p.qend[pair] = qe;
      p.tend[pair] = te;
      if (TB) {
        // the walk: 2 bits per step, M = 0, I = 1, D = 2
        uint32_t* const slot_words = p.paths + rel * BNPK_ALIGN_PATH_WORDS;
        const uint32_t* const Wp = W + (pw * G) * CAP + 16 * pw;             // lane 0 of this pair's group
        const uint8_t* const Bp = B + (pw * G) * CAP;
        int i = qe, j = te, state = 0, n_steps = 0, n_runs = 0, prev = -1;
        uint32_t word = 0;
        while (n_steps < 16 * AL_STEPS_AT) {                   // (i + j falls with every step: at most n + m of them)
          int op;
          if (state == 0) {
            if (i == 0 && j == 0) break;
            if (LOCAL && (i == 0 || j == 0)) break;
            if (!LOCAL && !GLOBAL && i == 0) break;
            if (i == 0) { op = 2; --j; }                     // (global: along row 0)
            else if (j == 0) { op = 1; --i; }                // (along column 0)
            else {
              const int L = (i - 1) / R, r = (i - 1) - L * R;
              const uint32_t nib = (r < 8 ? Wp[L * CAP + j - 1] >> (4 * r) : (uint32_t)Bp[L * CAP + j - 1] >> (4 * (r - 8))) & 15u;
              const uint32_t src = nib & 3u;
              if (src == 3u) break;
              if (src == 0u) { op = 0; --i; --j; }
              else { state = (int)src; continue; }
            }
          } else {
            const int L = (i - 1) / R, r = (i - 1) - L * R;
            const uint32_t nib = (r < 8 ? Wp[L * CAP + j - 1] >> (4 * r) : (uint32_t)Bp[L * CAP + j - 1] >> (4 * (r - 8))) & 15u;
            if (state == 1) { op = 2; if ((nib & 4u) || j == 1) state = 0; --j; }            // (E[i][1] and F[1][j] open: there is nothing to extend)
            else { op = 1; if ((nib & 8u) || i == 1) state = 0; --i; }
          }
          word |= (uint32_t)op << (2 * (n_steps & 15));
          if ((++n_steps & 15) == 0) { slot_words[(n_steps >> 4) - 1] = word; word = 0; }
          if (op != prev) { ++n_runs; prev = op; }
        }
        if (n_steps & 15) slot_words[n_steps >> 4] = word;
        slot_words[AL_STEPS_AT] = (uint32_t)n_steps;
        p.qstart[pair] = i;
        p.tstart[pair] = j;
        p.runs[pair] = n_runs;
      }
    }
  }
}

// the runs of slot k's walk, last step first
__global__ __launch_bounds__(BNPK_BLOCK) void al_cigar_kernel(const uint32_t* __restrict__ paths, const int64_t* __restrict__ offsets, int64_t n_pairs,
                                                             uint8_t* __restrict__ ops, int32_t* __restrict__ lengths) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_pairs; k += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t* slot = paths + k * BNPK_ALIGN_PATH_WORDS;
    const int n_steps = (int)min(slot[AL_STEPS_AT], (uint32_t)(16 * AL_STEPS_AT));
    int64_t at = offsets[k];
    const int64_t end = offsets[k + 1];                      // (a slot that disagrees with the scan writes nothing beyond its runs)
    int prev = -1, len = 0;
    for (int s = n_steps - 1; s >= 0; --s) {
      const int op = (int)(slot[s >> 4] >> (2 * (s & 15))) & 3;
      if (op != prev && prev >= 0) {
        if (at < end) { ops[at] = (uint8_t)prev; lengths[at] = len; }
        ++at;
        len = 0;
      }
      prev = op;
      ++len;
    }
    if (prev >= 0 && at < end) { ops[at] = (uint8_t)prev; lengths[at] = len; }
  }
}

template <bool PACKED, int G, int MODE, bool TB>
static int al_launch_one(bnpk_ctx* ctx, const al_args& a, hipStream_t s) {
  using cfg = al_cfg<PACKED, G, TB>;
  auto kernel = al_dp_kernel<PACKED, G, MODE, TB>;
  if (cfg::LDS > 65536) BNPK_HIP(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cfg::LDS));
  // as many wavefronts as the card holds at once, the LDS of a workgroup permitting; the kernel strides over the class's list
  const int64_t per_cu = cfg::LDS ? std::min<int64_t>(32, (160 * 1024) / cfg::LDS) : 32;
  const int64_t slots = ceil_div(a.n_pairs, cfg::PPW);
  hipLaunchKernelGGL(kernel, dim3(grid_for(std::min<int64_t>(slots, ctx->compute_units * std::max<int64_t>(per_cu, 1)))), dim3(BNPK_WAVE),
                     cfg::LDS, s, a);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

template <bool PACKED, int MODE, bool TB>
static int al_launch_mode(bnpk_ctx* ctx, const al_args& a, hipStream_t s) {
  BNPK_CHECK((al_launch_one<PACKED, 16, MODE, TB>(ctx, a, s)));
  return al_launch_one<PACKED, 64, MODE, TB>(ctx, a, s);
}

template <bool PACKED, bool TB>
static int al_launch(bnpk_ctx* ctx, int mode, const al_args& a, hipStream_t s) {
  hipLaunchKernelGGL(al_reset_kernel, dim3(1), dim3(BNPK_WAVE), 0, s, a.counts);
  hipLaunchKernelGGL(al_classify_kernel<TB>, dim3(grid_for(ceil_div(a.n_pairs, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, a);
  BNPK_HIP(ctx, hipGetLastError());
  if (mode == BNPK_ALIGN_LOCAL) return al_launch_mode<PACKED, BNPK_ALIGN_LOCAL, TB>(ctx, a, s);
  if (mode == BNPK_ALIGN_SEMIGLOBAL) return al_launch_mode<PACKED, BNPK_ALIGN_SEMIGLOBAL, TB>(ctx, a, s);
  return al_launch_mode<PACKED, BNPK_ALIGN_GLOBAL, TB>(ctx, a, s);
}

template <bool PACKED>
static int al_run(bnpk_ctx* ctx, const bnpk_align_params* h, const void* dq, int64_t nq, const int64_t* qoff, const void* dt, int64_t nt,
                  const int64_t* toff, int64_t n_targets, int64_t n_rows, int64_t first, int64_t n_pairs, int32_t* d_score,
                  int32_t* d_qend, int32_t* d_tend, int32_t* d_qstart, int32_t* d_tstart, int64_t* d_runs, uint32_t* d_paths,
                  int64_t* d_error, const char* name, hipStream_t s) {
  if (!ctx || !h || !h->matrix || nq < 0 || nt < 0 || n_rows < 0) return BNPK_ERR_ARG;
  const int A = h->alphabet_size;
  if (PACKED ? A != 4 : (A < 1 || A > BNPK_APPROX_MAX_ALPHABET)) return BNPK_ERR_ARG;
  if (h->mode < BNPK_ALIGN_LOCAL || h->mode > BNPK_ALIGN_GLOBAL || h->gap_open < 0 || h->gap_open > 127 || h->gap_extend < 0 ||
      h->gap_extend > 127)
    return BNPK_ERR_ARG;
  int lowest = 127;
  for (int i = 0; i < A * A; ++i) {
    if (h->matrix[i] < -128 || h->matrix[i] > 127) return BNPK_ERR_ARG;
    lowest = std::min(lowest, (int)h->matrix[i]);
  }
  if (n_targets != n_rows && n_targets != 1) return BNPK_ERR_ARG;
  if (first < 0 || n_pairs < 0 || first + n_pairs > n_rows || n_pairs > INT32_MAX) return BNPK_ERR_ARG;
  const bool tb = h->traceback != 0;
  if (n_pairs > 0 && (!qoff || !toff || !d_score || !d_qend || !d_tend || !d_error || (nq > 0 && !dq) || (nt > 0 && !dt))) return BNPK_ERR_ARG;
  if (n_pairs > 0 && tb && (!d_qstart || !d_tstart || !d_runs || !d_paths)) return BNPK_ERR_ARG;
  if (n_pairs == 0) return BNPK_OK;
  al_args a = {};
  a.q = dq; a.qoff = qoff; a.t = dt; a.toff = toff;
  a.first = first; a.n_pairs = n_pairs;
  a.one_target = (n_targets == 1 && n_rows != 1) ? 1 : 0;
  a.go = h->gap_open; a.ge = h->gap_extend; a.A = A;
  int8_t table[AL_TABLE_BYTES];
  if (PACKED) {
    for (int qc = 0; qc < 4; ++qc)
      for (int tc = 0; tc < 4; ++tc) a.rows4[qc] |= (uint32_t)(uint8_t)h->matrix[qc * 4 + tc] << (8 * tc);
  } else {
    memset(table, 0, sizeof(table));
    for (int qc = 0; qc <= A; ++qc)
      for (int tc = 0; tc <= A; ++tc) table[qc * (A + 1) + tc] = (int8_t)((qc < A && tc < A) ? h->matrix[qc * A + tc] : lowest);
  }
  void* scratch = nullptr;
  BNPK_CHECK(bnpk_scratch(ctx, (size_t)AL_TABLE_BYTES + 16 + (size_t)n_pairs * 4, &scratch, s));
  a.table = (const int8_t*)scratch;
  a.counts = (int32_t*)((char*)scratch + AL_TABLE_BYTES);
  a.list = a.counts + 4;
  a.score = d_score; a.qend = d_qend; a.tend = d_tend; a.qstart = d_qstart; a.tstart = d_tstart;
  a.runs = d_runs; a.paths = d_paths; a.error = (unsigned long long*)d_error;
  bnpk_timer t(ctx, name, s);
  if (!PACKED) BNPK_HIP(ctx, hipMemcpyAsync(scratch, table, AL_TABLE_BYTES, hipMemcpyHostToDevice, s));
  return tb ? al_launch<PACKED, true>(ctx, h->mode, a, s) : al_launch<PACKED, false>(ctx, h->mode, a, s);
}

}  // namespace

extern "C" {

int bnpk_align_pairs_packed(bnpk_ctx* ctx, const bnpk_align_params* h, const uint64_t* d_packed_q, int64_t n_bases_q,
                            const int64_t* d_offsets_q, const uint64_t* d_packed_t, int64_t n_bases_t, const int64_t* d_offsets_t,
                            int64_t n_targets, int64_t n_rows, int64_t first, int64_t n_pairs, int32_t* d_score,
                            int32_t* d_query_end, int32_t* d_target_end, int32_t* d_query_start, int32_t* d_target_start,
                            int64_t* d_runs, uint32_t* d_paths, int64_t* d_error, void* stream) {
  return al_run<true>(ctx, h, d_packed_q, n_bases_q, d_offsets_q, d_packed_t, n_bases_t, d_offsets_t, n_targets, n_rows, first, n_pairs,
                      d_score, d_query_end, d_target_end, d_query_start, d_target_start, d_runs, d_paths, d_error,
                      h && h->traceback ? "align_pairs_packed_tb" : "align_pairs_packed", (hipStream_t)stream);
}

int bnpk_align_pairs_bytes(bnpk_ctx* ctx, const bnpk_align_params* h, const uint8_t* d_codes_q, int64_t n_q,
                           const int64_t* d_offsets_q, const uint8_t* d_codes_t, int64_t n_t, const int64_t* d_offsets_t,
                           int64_t n_targets, int64_t n_rows, int64_t first, int64_t n_pairs, int32_t* d_score,
                           int32_t* d_query_end, int32_t* d_target_end, int32_t* d_query_start, int32_t* d_target_start,
                           int64_t* d_runs, uint32_t* d_paths, int64_t* d_error, void* stream) {
  return al_run<false>(ctx, h, d_codes_q, n_q, d_offsets_q, d_codes_t, n_t, d_offsets_t, n_targets, n_rows, first, n_pairs, d_score,
                       d_query_end, d_target_end, d_query_start, d_target_start, d_runs, d_paths, d_error,
                       h && h->traceback ? "align_pairs_bytes_tb" : "align_pairs_bytes", (hipStream_t)stream);
}

int bnpk_align_cigar(bnpk_ctx* ctx, const uint32_t* d_paths, const int64_t* d_run_offsets, int64_t n_pairs, uint8_t* d_ops,
                     int32_t* d_lengths, void* stream) {
  if (!ctx || n_pairs < 0 || (n_pairs > 0 && (!d_paths || !d_run_offsets))) return BNPK_ERR_ARG;
  if (n_pairs == 0) return BNPK_OK;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "align_cigar", s);
  hipLaunchKernelGGL(al_cigar_kernel, dim3(grid_for(ceil_div(n_pairs, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_paths, d_run_offsets,
                     n_pairs, d_ops, d_lengths);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // extern "C"
