// shz_resample_i16: rational resampling of 16-bit PCM by an integer polyphase filter, so that audio at any rate meets a
// table built at another.  The result is defined in integers (include/shz.h) and computed exactly:
//   out[m] = sat16((sum_k taps[p][k] * x[i0 - k] + 2^29) >> 30),  p = (m M) mod L,  i0 = (m M) div L + T/2
// with 64-bit multiply-adds (v_mad_i64_i32); no floating point anywhere.
#include <algorithm>

#include "shz_internal.h"

#define RS_THREADS 256
#define RS_TILE_MAX 8192u          // outputs of one workgroup
#define RS_LDS_BYTES 65536u        // dynamic LDS of one workgroup: tap table (when it fits) + the tile's input span
#define RS_TAPS_LDS_MAX 61440u     // largest padded tap table kept in LDS
#define RS_SPAN_SLACK 24u          // span samples beyond the ones read: alignment of the first 16-byte chunk, rounding to chunks
#define RS_KERNEL_SLOT 5           // shz_get_kernel_ms(which)

// one clip of a call: x_abs[i] = pcm[src + i - in_base] for in_base <= i < in_base + n, 0 elsewhere;
// outputs m in [m_first, m_first + m_count) go to out[out + m - m_first]
struct rs_clip {
  uint64_t src, n, in_base, m_first, m_count, out;
};

// Row stride of the tap table as the kernel reads it: the smallest S >= T with S = 2 (mod 4).  Rows stay 8-byte aligned
// for ds_read_b64, and S / 2 is odd, so lanes whose phases differ mod 32 read 32 different bank pairs.
static inline uint32_t rs_stride(uint32_t T) { return (T & 2u) ? T : T + 2; }

// One workgroup per (clip, tile of outputs).  Lane j of a pass takes output m0 + j: neighbouring lanes step the phase by
// M mod L and the input position by M div L (or one more), so x is read from neighbouring LDS words and the taps from rows
// S words apart.
template <bool TAPS_LDS>
__global__ __launch_bounds__(RS_THREADS) void resample_i16_kernel(const int16_t* __restrict__ pcm, const rs_clip* __restrict__ clips,
                                                                   const uint32_t* __restrict__ tile_off, uint32_t n_clips,
                                                                   const int32_t* __restrict__ taps, uint32_t L, uint32_t M,
                                                                   uint32_t T, uint32_t S, uint32_t tile, uint32_t taps_bytes,
                                                                   int16_t* __restrict__ out) {
  extern __shared__ __align__(16) unsigned char rs_smem[];
  int32_t* s_taps = (int32_t*)rs_smem;
  int16_t* s_x = (int16_t*)(rs_smem + (TAPS_LDS ? taps_bytes : 0u));
  const uint32_t tid = threadIdx.x, b = blockIdx.x;

  uint32_t lo = 0, hi = n_clips;   // the last clip whose first tile is at or before b (clips without outputs own no tile)
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tile_off[mid] <= b) lo = mid; else hi = mid;
  }
  const rs_clip cl = clips[lo];
  const uint64_t m0 = cl.m_first + (uint64_t)(b - tile_off[lo]) * tile;
  const uint64_t left = cl.m_first + cl.m_count - m0;
  const uint32_t cnt = left < tile ? (uint32_t)left : tile;

  if (TAPS_LDS) {   // padded on the host: a straight 16-byte copy
    const uint4* g = (const uint4*)taps;
    for (uint32_t i = tid; i < taps_bytes / 16; i += RS_THREADS) ((uint4*)s_taps)[i] = g[i];
  }

  // the samples the tile reads: x_abs[lo_abs .. hi_abs]; the LDS image starts at a0 <= lo_abs, where a 16-byte load is aligned
  const int64_t half = (int64_t)(T >> 1);
  const int64_t lo_abs = (int64_t)((m0 * M) / L) + half - (int64_t)(T - 1);
  const int64_t hi_abs = (int64_t)(((m0 + cnt - 1) * M) / L) + half;
  const int64_t e_lo = (int64_t)(((uintptr_t)pcm >> 1) + cl.src) + (lo_abs - (int64_t)cl.in_base);   // element address of lo_abs
  const int64_t a0 = lo_abs - (e_lo & 7);
  const uint32_t chunks = (uint32_t)((hi_abs - a0 + 8) >> 3);
  const int64_t v_lo = (int64_t)cl.in_base, v_hi = (int64_t)(cl.in_base + cl.n);
  for (uint32_t j = tid; j < chunks; j += RS_THREADS) {
    const int64_t a = a0 + 8 * (int64_t)j;
    uint4 v;
    if (a >= v_lo && a + 8 <= v_hi) {
      v = *(const uint4*)(pcm + cl.src + (uint64_t)(a - v_lo));
    } else {   // a chunk that crosses the clip's edge: nothing outside the clip is read
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t a1 = a + 2 * q, a2 = a1 + 1;
        const uint32_t x1 = (a1 >= v_lo && a1 < v_hi) ? (uint16_t)pcm[cl.src + (uint64_t)(a1 - v_lo)] : 0u;
        const uint32_t x2 = (a2 >= v_lo && a2 < v_hi) ? (uint16_t)pcm[cl.src + (uint64_t)(a2 - v_lo)] : 0u;
        w[q] = x1 | (x2 << 16);
      }
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    ((uint4*)s_x)[j] = v;
  }
  __syncthreads();

  // (m M) div L and mod L of the lane's first output by one division, then by steps of RS_THREADS outputs
  const uint64_t step = (uint64_t)RS_THREADS * M;
  const uint64_t step_d = step / L;
  const uint32_t step_p = (uint32_t)(step - step_d * L);
  uint64_t q0 = (m0 + tid) * M;
  uint64_t d = q0 / L;
  uint32_t p = (uint32_t)(q0 - d * L);
  for (uint32_t j = tid; j < cnt; j += RS_THREADS) {
    const int32_t* tp = (TAPS_LDS ? (const int32_t*)s_taps : taps) + (uint64_t)p * S;
    const int16_t* xp = s_x + (int32_t)((int64_t)d + half - a0);   // x[i0]
    long long acc0 = 0, acc1 = 0;
#pragma unroll 8
    for (uint32_t k = 0; k < T; k += 2) {
      const int2 t2 = *(const int2*)(tp + k);
      acc0 += (long long)t2.x * (int)xp[-(int32_t)k];
      acc1 += (long long)t2.y * (int)xp[-(int32_t)k - 1];
    }
    long long r = (acc0 + acc1 + (1ll << 29)) >> 30;
    r = r < -32768 ? -32768 : (r > 32767 ? 32767 : r);
    out[cl.out + (m0 - cl.m_first) + j] = (int16_t)r;
    d += step_d;
    p += step_p;
    if (p >= L) { p -= L; d += 1; }
  }
}

extern "C" int32_t shz_resample_i16(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, uint32_t L,
                                    uint32_t M, uint32_t T, const int32_t* taps, const uint64_t* in_base, const uint64_t* m_first,
                                    const uint64_t* m_end, uint32_t flags, int16_t* out, uint64_t* out_off, uint64_t cap,
                                    uint64_t* count) {
  if (!ctx) return SHZ_E_INVALID;
  if (!clip_off || !taps || !out_off || !count || (!m_first) != (!m_end)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: null argument");
  if (L == 0 || M == 0 || T == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: L, M and T must be positive");
  if ((T & 1u) || T > SHZ_RESAMPLE_MAX_TAPS) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: T must be even and at most %u", SHZ_RESAMPLE_MAX_TAPS);
  if (L > SHZ_RESAMPLE_MAX_RATIO || M > SHZ_RESAMPLE_MAX_RATIO || (uint64_t)L * T > SHZ_RESAMPLE_MAX_TABLE)
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_resample_i16: L and M at most %u and L * T at most %u", SHZ_RESAMPLE_MAX_RATIO, SHZ_RESAMPLE_MAX_TABLE);
  for (uint32_t c = 0; c < n_clips; ++c) {
    if (clip_off[c + 1] < clip_off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: clip_off decreases at clip %u", c);
    if (m_first && (m_end[c] < m_first[c] || m_end[c] > (1ull << 39))) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: bad output range of clip %u", c);
    if (clip_off[c + 1] - clip_off[c] > (1ull << 39) || (in_base && in_base[c] > (1ull << 39)))
      SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: clip %u too long", c);
  }
  SHZ_HIP(ctx, hipSetDevice(ctx->device));

  // the plan: where the taps live, how many outputs a workgroup takes so that its input span fits the LDS
  const uint32_t S = rs_stride(T);
  const uint64_t table_bytes = ((uint64_t)L * S * 4 + 15) & ~15ull;
  bool taps_lds = table_bytes <= RS_TAPS_LDS_MAX && (RS_LDS_BYTES - table_bytes) / 2 >= T + RS_SPAN_SLACK + 1;
  const uint32_t span_cap = taps_lds ? (uint32_t)((RS_LDS_BYTES - table_bytes) / 2) : RS_LDS_BYTES / 4;   // samples
  // span of a tile = ((m0 + tile - 1) M) div L - (m0 M) div L + T  <=  ceil((tile - 1) M / L) + T
  const uint64_t room = span_cap - T - RS_SPAN_SLACK;
  const uint32_t tile = (uint32_t)std::min<uint64_t>(RS_TILE_MAX, 1 + room * L / M);
  const uint32_t lds_bytes = (taps_lds ? (uint32_t)table_bytes : 0u) + span_cap * 2;

  std::vector<rs_clip> clips(n_clips);
  std::vector<uint32_t> tile_off(n_clips + 1);
  uint64_t total = 0, tiles = 0;
  for (uint32_t c = 0; c < n_clips; ++c) {
    rs_clip& k = clips[c];
    k.src = clip_off[c] - ((flags & SHZ_PCM_DEVICE) ? 0 : clip_off[0]);
    k.n = clip_off[c + 1] - clip_off[c];
    k.in_base = in_base ? in_base[c] : 0;
    k.m_first = m_first ? m_first[c] : 0;
    k.m_count = m_first ? m_end[c] - m_first[c] : (k.n * L + M - 1) / M;
    k.out = total;
    out_off[c] = total;
    tile_off[c] = (uint32_t)tiles;
    total += k.m_count;
    tiles += (k.m_count + tile - 1) / tile;
    if (tiles > 0x7FFFFFFFull) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_resample_i16: too many output tiles for one call");
  }
  out_off[n_clips] = total;
  tile_off[n_clips] = (uint32_t)tiles;
  *count = total;
  if (total > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_resample_i16: %llu samples needed, room for %llu", (unsigned long long)total, (unsigned long long)cap);
  if (total == 0) return SHZ_OK;
  if (!out || !pcm) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_resample_i16: null buffer");

  const int16_t* d_pcm = pcm;
  if (!(flags & SHZ_PCM_DEVICE)) {
    const uint64_t s0 = clip_off[0], s1 = clip_off[n_clips];
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_PCM, (s1 - s0) * 2 + 64, &p));
    if (s1 > s0) SHZ_HIP(ctx, shz_memcpy(ctx, p, pcm + s0, (s1 - s0) * 2, hipMemcpyHostToDevice));
    d_pcm = (const int16_t*)p;
  }
  int16_t* d_out = out;
  if (!(flags & SHZ_OUT_DEVICE)) {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_DB, total * 2 + 64, &p));
    d_out = (int16_t*)p;
  }
  std::vector<int32_t> padded(table_bytes / 4, 0);   // rows of S words: T taps, then zeros
  for (uint32_t r = 0; r < L; ++r) memcpy(&padded[(uint64_t)r * S], taps + (uint64_t)r * T, (uint64_t)T * 4);
  void *d_taps, *d_clips, *d_tiles;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC0, table_bytes, &d_taps));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_META, clips.size() * sizeof(rs_clip) + 64, &d_clips));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC1, tile_off.size() * 4 + 64, &d_tiles));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_taps, padded.data(), table_bytes, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_clips, clips.data(), clips.size() * sizeof(rs_clip), hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_tiles, tile_off.data(), tile_off.size() * 4, hipMemcpyHostToDevice));
  {
    shz_prof_scope ps(ctx, RS_KERNEL_SLOT);
    if (taps_lds)
      hipLaunchKernelGGL(resample_i16_kernel<true>, dim3((unsigned)tiles), dim3(RS_THREADS), lds_bytes, ctx->stream, d_pcm,
                         (const rs_clip*)d_clips, (const uint32_t*)d_tiles, n_clips, (const int32_t*)d_taps, L, M, T, S, tile,
                         (uint32_t)table_bytes, d_out);
    else
      hipLaunchKernelGGL(resample_i16_kernel<false>, dim3((unsigned)tiles), dim3(RS_THREADS), lds_bytes, ctx->stream, d_pcm,
                         (const rs_clip*)d_clips, (const uint32_t*)d_tiles, n_clips, (const int32_t*)d_taps, L, M, T, S, tile,
                         (uint32_t)table_bytes, d_out);
  }
  SHZ_HIP(ctx, hipGetLastError());
  if (!(flags & SHZ_OUT_DEVICE)) SHZ_HIP(ctx, shz_memcpy(ctx, out, d_out, total * 2, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}
