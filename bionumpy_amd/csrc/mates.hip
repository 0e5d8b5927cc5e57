// Paired-end read merging: per pair of mates the offset at which mate 1 and the reverse complement of mate 2 overlap best
// (bnpk_mates_overlap_packed / _bytes), and the consensus read with its qualities (bnpk_mates_merge_packed / _bytes).  The
// semantics are those of include/bnpk.h; DESIGN.md 4d.
//
//   Words.  A mate is MT_WORDS words of 16 symbols, 2 bits each, bit 0 upwards.  a = mate 1; b = the reverse complement of
//   mate 2, which exists in LDS only.  The bytes path has a PLANE per mate next to it: bit 2j + 1 of a plane word is set iff
//   symbol j of the word is no letter (a code >= 4; its two code bits are 0).  The packed path has no planes (template
//   parameter: they compile away).
//
//   Staging, mt_overlap_kernel.  A wavefront takes one pair at a time and owns 32 + 36 words of LDS (twice that with
//   planes), so it never waits for another wavefront (no workgroup barrier; LDS traffic of one wavefront is in order).  Lane
//   l < 32 makes word l of a:
//   sixteen symbols from the flat 2-bit position offsets1[i] + 16 l, cut out of one or two 64-bit words.  Lane 32 + k makes
//   word k of b from the sixteen symbols that END at position n2 - 16 k of mate 2: V_BFREV_B32 reverses the bits, a swap
//   inside every bit pair makes that a reversal of symbols, a shift brings the row's start to bit 0 and a NOT complements.
//   The bytes path gathers the same words (and planes) from sixteen code bytes per lane.  b has a zero word in front and
//   zero words behind, so that the word loop below never leaves the array.
//
//   Offsets across lanes.  The candidate offsets of the pair are s_lo .. s_hi (from min_overlap and read_through); they go
//   through the wavefront 64 at a time, lane l takes s = s0 + l.  The overlap of s is the columns [lo, hi) of a, the words
//   lo / 16 .. (hi - 1) / 16.  Per word: b's sixteen symbols that face it straddle two of b's words, of which one is carried
//   over from the word before — ONE LDS read of b, one of a, V_ALIGNBIT_B32 (the funnel shift, by 2 * ((16 w - s) mod 16)),
//   XOR, (x << 1 | x) — bit 2j + 1 is now "symbol j differs" — OR of the two planes, AND 0xAAAAAAAA, V_BCNT (which adds).
//   The first and the last word of an overlap are AND-ed with the overlap's ends as well; they are peeled, so that the loop
//   over the words between them has no mask to compute.  The 64 offsets of a round differ by at most 63 columns: the trip
//   counts of the lanes differ by four words at the most, whatever n1 and n2 are, and no lane holds a mate in registers.
//   One pair per lane (the obvious alternative) would put 2 x 32 words per lane into registers or scratch, make the trip count
//   of a wavefront that of its longest pair, and scatter the loads of 64 rows; it was not built.
//
//   Choice.  A qualifying offset is ONE word, ov << 21 | (1023 - mm) << 11 | (1023 - s): the maximum over rounds and then over
//   the lanes (wave_max: six DPP moves) is the largest overlap, among those the fewest mismatches, among those the smallest
//   offset.  ov >= 1, so 0 stands for "none".  Lane 0 writes the pair's twelve bytes.
//
//   No matrix instructions: the two operands of the correlation belong to one pair; nothing is shared across 16 rows the way
//   the barcode library of demux.hip was, so an MFMA would multiply mostly zeros.
//
//   Merge, mt_merge_kernel.  A wavefront takes a pair with length >= 0, the lanes its columns t, t + 64, ...: codes and
//   qualities are written coalesced, mate 1 is read forwards and mate 2 backwards in place (column t faces position
//   n2 - 1 - (t - s) of mate 2).  One 2-bit extraction per mate and column, one byte per lane and store.
#include "common.h"

namespace {

constexpr int MT_WORDS = BNPK_MATES_MAX_LEN / 16;            // 32-bit words of 16 symbols per mate
constexpr int MT_B_WORDS = MT_WORDS + 4;                     // b: one zero word in front, three behind
constexpr int MT_WAVES = BNPK_BLOCK / BNPK_WAVE;             // pairs in flight per workgroup
constexpr uint32_t MT_ODD = 0xAAAAAAAAu;                     // bit 2j + 1: the flag of symbol j
static_assert(MT_WORDS == 32, "lane l stages word l of a, lane 32 + k word k of b");
static_assert(BNPK_MATES_MAX_LEN <= 512, "ov and mm take 10 bits of a key, s + 1023 eleven");

struct mt_args {
  const int64_t* off1; const int64_t* off2;
  int64_t n_rows;
  int min_overlap, max_mm, max_percent, read_through, cap;
  int64_t* length; int32_t* overlap; int32_t* mismatches;
  unsigned long long* error;
};

// cnt <= 16 symbols from flat 2-bit position pos on, in the low 2 * cnt bits; the second word is read only where they reach it
__device__ __forceinline__ uint32_t mt_run(const uint64_t* __restrict__ W, int64_t pos, int cnt) {
  const int64_t i = pos >> 5;
  const int sh = 2 * (int)(pos & 31);
  uint64_t v = W[i] >> sh;
  if (sh + 2 * cnt > 64) v |= W[i + 1] << (64 - sh);
  return cnt >= 16 ? (uint32_t)v : ((uint32_t)v & ((1u << (2 * cnt)) - 1u));
}

// word k of a (REV = false: the symbols 16 k .. of the row at g) or of b (REV = true: the reverse complement of the row),
// and its plane
template <bool PACKED, bool REV>
__device__ __forceinline__ void mt_stage_word(const void* __restrict__ data, int64_t g, int n, int k, uint32_t& word, uint32_t& plane) {
  word = plane = 0;
  const int cnt = min(16, n - 16 * k);
  if (cnt <= 0) return;
  const int64_t from = REV ? g + n - 16 * k - cnt : g + 16 * k;
  if (PACKED) {
    uint32_t v = mt_run((const uint64_t*)data, from, cnt);
    if (REV) {
      v = __builtin_bitreverse32(v);
      v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);            // symbol j of the run is now symbol 15 - j
      v = ~(v >> (32 - 2 * cnt));
      if (cnt < 16) v &= (1u << (2 * cnt)) - 1u;
    }
    word = v;
  } else {
    const uint8_t* c = (const uint8_t*)data + from;
    for (int j = 0; j < cnt; ++j) {
      const uint32_t code = REV ? c[cnt - 1 - j] : c[j];
      if (code < 4) word |= (REV ? 3u - code : code) << (2 * j);
      else plane |= 2u << (2 * j);
    }
  }
}

template <bool PACKED>
__global__ __launch_bounds__(BNPK_BLOCK) void mt_overlap_kernel(const void* __restrict__ data1, const void* __restrict__ data2, mt_args p) {
  __shared__ uint32_t sa[MT_WAVES][PACKED ? 1 : 2][MT_WORDS];
  __shared__ uint32_t sb[MT_WAVES][PACKED ? 1 : 2][MT_B_WORDS];
  BNPK_VGPR_FLOOR_32();
  const int lane = lane_id(), wv = wave_id();
  uint32_t* A = sa[wv][0];
  uint32_t* B = sb[wv][0];
  uint32_t* PA = sa[wv][PACKED ? 0 : 1];
  uint32_t* PB = sb[wv][PACKED ? 0 : 1];
  if (lane < MT_B_WORDS) {                                   // the zero words around b; the 32 between them change per pair
    B[lane] = 0;
    if (!PACKED) PB[lane] = 0;
  }
  for (int64_t pair = (int64_t)blockIdx.x * MT_WAVES + wv; pair < p.n_rows; pair += (int64_t)gridDim.x * MT_WAVES) {
    const int64_t g1 = p.off1[pair], g2 = p.off2[pair];
    const int64_t len1 = p.off1[pair + 1] - g1, len2 = p.off2[pair + 1] - g2;
    if (len1 > BNPK_MATES_MAX_LEN || len2 > BNPK_MATES_MAX_LEN || len1 < 0 || len2 < 0) {     // (uniform)
      if (lane == 0) {
        atomicMin(p.error, (unsigned long long)pair);
        p.length[pair] = -1;
        p.overlap[pair] = 0;
        p.mismatches[pair] = 0;
      }
      continue;
    }
    const int n1 = (int)len1, n2 = (int)len2;
    int s_lo = p.min_overlap - n2, s_hi = n1 - p.min_overlap;
    if (!p.read_through) s_lo = max(s_lo, max(0, n1 - n2));
    if (n1 < p.min_overlap || n2 < p.min_overlap) s_hi = s_lo - 1;
    uint32_t best = 0;
    if (s_lo <= s_hi) {                                      // (uniform)
      uint32_t word, plane;
      if (lane < MT_WORDS) {
        mt_stage_word<PACKED, false>(data1, g1, n1, lane, word, plane);
        A[lane] = word;
        if (!PACKED) PA[lane] = plane;
      } else {
        mt_stage_word<PACKED, true>(data2, g2, n2, lane - MT_WORDS, word, plane);
        B[lane - MT_WORDS + 1] = word;
        if (!PACKED) PB[lane - MT_WORDS + 1] = plane;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                       // (the wavefront's LDS writes are in order before its reads)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      for (int s0 = s_lo; s0 <= s_hi; s0 += BNPK_WAVE) {
        const int s = s0 + lane;
        const int lo = max(0, s), hi = min(n1, s + n2), ov = hi - lo;
        if (s > s_hi || ov < p.min_overlap) continue;
        const int wf = lo >> 4, wl = (hi - 1) >> 4;
        const int at = 16 * wf - s;                          // b's symbol that faces symbol 0 of word wf: -15 .. n2 - 1
        const int shift = 2 * (at & 15);
        int q = (at >> 4) + 1;                               // its word, in B's indices: 0 ..
        uint32_t cur = B[q], pcur = PACKED ? 0u : PB[q];
        // the flags of word w: bit 2j + 1 = its symbol j differs from the symbol of b it faces
        auto flags = [&](int w) -> uint32_t {
          ++q;
          const uint32_t next = B[q];
          const uint32_t x = A[w] ^ __builtin_amdgcn_alignbit(next, cur, shift);
          cur = next;
          uint32_t y = (x << 1) | x;
          if (!PACKED) {
            const uint32_t pnext = PB[q];
            y |= PA[w] | __builtin_amdgcn_alignbit(pnext, pcur, shift);
            pcur = pnext;
          }
          return y;
        };
        const uint32_t first = MT_ODD & (0xffffffffu << (2 * (lo - 16 * wf)));
        const uint32_t last = MT_ODD & (0xffffffffu >> (32 - 2 * (hi - 16 * wl)));
        int mm;
        if (wf == wl) {
          mm = __builtin_popcount(flags(wf) & first & last);
        } else {
          mm = __builtin_popcount(flags(wf) & first);
          for (int w = wf + 1; w < wl; ++w) mm += __builtin_popcount(flags(w) & MT_ODD);
          mm += __builtin_popcount(flags(wl) & last);
        }
        if (mm <= p.max_mm && 100 * mm <= p.max_percent * ov)
          best = max(best, ((uint32_t)ov << 21) | ((uint32_t)(1023 - mm) << 11) | (uint32_t)(1023 - s));
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();                       // (nobody reads this pair's words any more)
    }
    best = wave_max(best);
    if (lane == 0) {
      const int s = 1023 - (int)(best & 2047u);
      p.length[pair] = best ? (int64_t)(s + n2) : -1;
      p.overlap[pair] = (int32_t)(best >> 21);
      p.mismatches[pair] = best ? 1023 - (int32_t)((best >> 11) & 1023u) : 0;
    }
  }
}

__global__ __launch_bounds__(BNPK_BLOCK) void mt_lengths_kernel(const int64_t* __restrict__ length, int64_t n, int64_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = max(length[i], (int64_t)0);
}

struct mt_merge_args {
  const int64_t* off1; const int64_t* off2;
  const uint8_t* qual1; const uint8_t* qual2;
  int64_t n_rows;
  int cap;
  const int64_t* length; const int64_t* out_off;
  uint8_t* codes; uint8_t* qual;
};

template <bool PACKED>
__device__ __forceinline__ uint32_t mt_code(const void* __restrict__ data, int64_t pos) {
  if (PACKED) return (uint32_t)(((const uint64_t*)data)[pos >> 5] >> (2 * (int)(pos & 31))) & 3u;
  return ((const uint8_t*)data)[pos];
}

template <bool PACKED>
__global__ __launch_bounds__(BNPK_BLOCK) void mt_merge_kernel(const void* __restrict__ data1, const void* __restrict__ data2, mt_merge_args p) {
  BNPK_VGPR_FLOOR_32();
  const int lane = lane_id();
  for (int64_t pair = (int64_t)blockIdx.x * MT_WAVES + wave_id(); pair < p.n_rows; pair += (int64_t)gridDim.x * MT_WAVES) {
    const int64_t f = p.length[pair];
    if (f < 0) continue;
    const int64_t g1 = p.off1[pair], g2 = p.off2[pair];
    const int64_t n1 = p.off1[pair + 1] - g1, n2 = p.off2[pair + 1] - g2;
    const int64_t s = f - n2, out0 = p.out_off[pair];
    for (int64_t t = lane; t < f; t += BNPK_WAVE) {
      const int64_t j = t - s;                               // b[j] = the complement of mate 2's symbol n2 - 1 - j
      const bool in_a = t < n1, in_b = j >= 0 && j < n2;
      uint32_t ca = 0, cb = 0, qa = 0, qb = 0;
      if (in_a) {
        ca = mt_code<PACKED>(data1, g1 + t);
        if (p.qual1) qa = p.qual1[g1 + t];
      }
      if (in_b) {
        cb = mt_code<PACKED>(data2, g2 + n2 - 1 - j);
        if (cb < 4) cb = 3 - cb;
        if (p.qual2) qb = p.qual2[g2 + n2 - 1 - j];
      }
      uint32_t c = ca, q = qa;                               // a alone, two non-letters, or neither mate (0, 0)
      if (in_b && !in_a) {
        c = cb; q = qb;
      } else if (in_a && in_b) {
        if (ca >= 4 || cb >= 4) {
          if (ca >= 4 && cb < 4) { c = cb; q = qb; }
        } else if (ca == cb) {
          q = min(qa + qb, (uint32_t)p.cap);
        } else if (qb > qa) {
          c = cb; q = qb - qa;
        } else {
          q = qa - qb;
        }
      }
      p.codes[out0 + t] = (uint8_t)c;
      if (p.qual) p.qual[out0 + t] = (uint8_t)q;
    }
  }
}

static bool mt_bad(const bnpk_mates_params* h) {
  return !h || h->min_overlap < 1 || h->max_mismatches < 0 || h->max_mismatch_percent < 0 || h->max_mismatch_percent > 100 ||
         h->read_through < 0 || h->read_through > 1 || h->quality_cap < 0 || h->quality_cap > 93;
}

static unsigned mt_grid(const bnpk_ctx* ctx, int64_t n_rows) {
  return grid_for(min(ceil_div(n_rows, MT_WAVES), (int64_t)ctx->compute_units * 64));
}

template <bool PACKED>
static int mt_overlap(bnpk_ctx* ctx, const bnpk_mates_params* h, const void* d1, int64_t n1, const int64_t* off1, const void* d2,
                      int64_t n2, const int64_t* off2, int64_t n_rows, int64_t* d_length, int32_t* d_overlap, int32_t* d_mismatches,
                      int64_t* d_error, const char* name, hipStream_t s) {
  if (!ctx || mt_bad(h) || n1 < 0 || n2 < 0 || n_rows < 0) return BNPK_ERR_ARG;
  if (n_rows > 0 && (!off1 || !off2 || !d_length || !d_overlap || !d_mismatches || !d_error || (n1 > 0 && !d1) || (n2 > 0 && !d2)))
    return BNPK_ERR_ARG;
  if (n_rows == 0) return BNPK_OK;
  // (a limit above 1023 would not fit the key; no pair has more than BNPK_MATES_MAX_LEN mismatches)
  const mt_args a = {off1, off2, n_rows, h->min_overlap, min(h->max_mismatches, BNPK_MATES_MAX_LEN), h->max_mismatch_percent,
                     h->read_through, h->quality_cap, d_length, d_overlap, d_mismatches, (unsigned long long*)d_error};
  bnpk_timer t(ctx, name, s);
  hipLaunchKernelGGL((mt_overlap_kernel<PACKED>), dim3(mt_grid(ctx, n_rows)), dim3(BNPK_BLOCK), 0, s, d1, d2, a);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

template <bool PACKED>
static int mt_merge(bnpk_ctx* ctx, const bnpk_mates_params* h, const void* d1, const int64_t* off1, const uint8_t* q1, const void* d2,
                    const int64_t* off2, const uint8_t* q2, int64_t n_rows, const int64_t* d_length, const int64_t* d_out_offsets,
                    uint8_t* d_out_codes, uint8_t* d_out_qual, const char* name, hipStream_t s) {
  if (!ctx || mt_bad(h) || n_rows < 0 || (q1 == nullptr) != (q2 == nullptr)) return BNPK_ERR_ARG;
  if (n_rows > 0 && (!off1 || !off2 || !d_length || !d_out_offsets)) return BNPK_ERR_ARG;
  if (n_rows == 0) return BNPK_OK;
  const mt_merge_args a = {off1, off2, q1, q2, n_rows, h->quality_cap, d_length, d_out_offsets, d_out_codes, q1 ? d_out_qual : nullptr};
  bnpk_timer t(ctx, name, s);
  hipLaunchKernelGGL((mt_merge_kernel<PACKED>), dim3(mt_grid(ctx, n_rows)), dim3(BNPK_BLOCK), 0, s, d1, d2, a);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

}  // namespace

extern "C" {

int bnpk_mates_overlap_packed(bnpk_ctx* ctx, const bnpk_mates_params* h, const uint64_t* d_packed1, int64_t n_bases1,
                              const int64_t* d_offsets1, const uint64_t* d_packed2, int64_t n_bases2, const int64_t* d_offsets2,
                              int64_t n_rows, int64_t* d_length, int32_t* d_overlap, int32_t* d_mismatches, int64_t* d_error,
                              void* stream) {
  return mt_overlap<true>(ctx, h, d_packed1, n_bases1, d_offsets1, d_packed2, n_bases2, d_offsets2, n_rows, d_length, d_overlap,
                          d_mismatches, d_error, "mates_overlap_packed", (hipStream_t)stream);
}

int bnpk_mates_overlap_bytes(bnpk_ctx* ctx, const bnpk_mates_params* h, const uint8_t* d_codes1, int64_t n1,
                             const int64_t* d_offsets1, const uint8_t* d_codes2, int64_t n2, const int64_t* d_offsets2,
                             int64_t n_rows, int64_t* d_length, int32_t* d_overlap, int32_t* d_mismatches, int64_t* d_error,
                             void* stream) {
  return mt_overlap<false>(ctx, h, d_codes1, n1, d_offsets1, d_codes2, n2, d_offsets2, n_rows, d_length, d_overlap, d_mismatches,
                           d_error, "mates_overlap_bytes", (hipStream_t)stream);
}

int bnpk_mates_lengths(bnpk_ctx* ctx, const int64_t* d_length, int64_t n_rows, int64_t* d_out, void* stream) {
  if (!ctx || n_rows < 0 || (n_rows > 0 && (!d_length || !d_out))) return BNPK_ERR_ARG;
  if (n_rows == 0) return BNPK_OK;
  hipStream_t s = (hipStream_t)stream;
  bnpk_timer t(ctx, "mates_lengths", s);
  hipLaunchKernelGGL(mt_lengths_kernel, dim3(grid_for(ceil_div(n_rows, BNPK_BLOCK))), dim3(BNPK_BLOCK), 0, s, d_length, n_rows, d_out);
  BNPK_HIP(ctx, hipGetLastError());
  return BNPK_OK;
}

int bnpk_mates_merge_packed(bnpk_ctx* ctx, const bnpk_mates_params* h, const uint64_t* d_packed1, const int64_t* d_offsets1,
                            const uint8_t* d_qual1, const uint64_t* d_packed2, const int64_t* d_offsets2, const uint8_t* d_qual2,
                            int64_t n_rows, const int64_t* d_length, const int64_t* d_out_offsets, uint8_t* d_out_codes,
                            uint8_t* d_out_qual, void* stream) {
  return mt_merge<true>(ctx, h, d_packed1, d_offsets1, d_qual1, d_packed2, d_offsets2, d_qual2, n_rows, d_length, d_out_offsets,
                        d_out_codes, d_out_qual, "mates_merge_packed", (hipStream_t)stream);
}

int bnpk_mates_merge_bytes(bnpk_ctx* ctx, const bnpk_mates_params* h, const uint8_t* d_codes1, const int64_t* d_offsets1,
                           const uint8_t* d_qual1, const uint8_t* d_codes2, const int64_t* d_offsets2, const uint8_t* d_qual2,
                           int64_t n_rows, const int64_t* d_length, const int64_t* d_out_offsets, uint8_t* d_out_codes,
                           uint8_t* d_out_qual, void* stream) {
  return mt_merge<false>(ctx, h, d_codes1, d_offsets1, d_qual1, d_codes2, d_offsets2, d_qual2, n_rows, d_length, d_out_offsets,
                         d_out_codes, d_out_qual, "mates_merge_bytes", (hipStream_t)stream);
}

}  // extern "C"
