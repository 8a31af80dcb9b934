// Live streams: fingerprints of many audio streams that arrive chunk by chunk (the reference's recogniser reads the
// microphone in CHUNK = 8192-sample pieces per channel, recognizer.py:21-25, 357-392), bit for bit the hashes, in the order,
// of fingerprint() on the concatenation of the chunks (__init__.py:212-245).
//
// Locality.  Frame k is x[k hop : k hop + 4096]; whether a cell of frame t is a peak depends on frames
// t-10 .. t+10 only (21x21 maximum filter, __init__.py:137-149), the frequency axis is always whole.  Once C frames are
// complete, frames t < H = C - 10 are SETTLED.  A push settles [H_prev, H) by extracting one WINDOW CLIP per stream that
// starts at frame w0 = max(0, H_prev - 10) and ends with the last complete frame (at the stream's end: with its last sample):
// its peaks with frame in [H_prev - w0, H - w0) are exact, the frames in front are halo.  The stream's carried PCM tail
// always starts at sample w0 hop of the NEXT push, so the window is the tail plus the new chunk, cut at the last frame.
//
// Emission (generate_hashes order, __init__.py:194-209).  Settled peaks in (t, f) order; peak i pairs with i + 1 .. i + fan - 1
// where dt <= 200.  Its hashes are final once (a) fan - 1 settled peaks follow it, or (b) H > t_i + 200 (no later peak can
// pair with it), or (c) the stream ends.  Both (a) and (b) hold for a prefix of the list, so a push emits a prefix and
// carries the rest -- at most fan - 1 <= 63 peaks, by (a) -- to the next push.
//
// One push = one pass over all streams: stream_gather_kernel (tails + chunks -> window clips, new tails), the extraction
// pass on the windows (shz_peaks, device in / device out), stream_count_kernel (settled range, emission prefix, hash count
// per stream), a scan over the streams, stream_write_kernel (hashes in order, pending peaks carried), one read-back.
#include <algorithm>

#include "shz_internal.h"
#include "shz_table_int.h"

#define ST_PEND 64            // carried peaks per stream slot: at most fan - 1 <= 63 after a push (rule (a))
#define ST_THREADS 256
#define ST_MAX_STREAMS 65535u // one workgroup row per stream (grid.y)

// per-push work of one stream (built on the host, one upload)
struct st_job {
  uint64_t src;       // first sample of the chunk in the pushed PCM (device)
  uint64_t chunk;     // samples of the chunk
  uint64_t tail;      // samples of the carried tail (the chunk follows it: together the stream's samples from tail start)
  uint64_t win_len;   // window = the first win_len samples of tail ++ chunk (0: no window)
  uint64_t win_dst;   // where the window starts in the window buffer
  uint64_t ntail_lo;  // new tail = tail ++ chunk from here on (written only if do_tail)
  uint32_t stream;
  uint32_t tail_in, tail_out;   // parity slots of the tail
  uint32_t pend_in, pend_out;   // parity slots of the carried peaks
  uint32_t do_tail;             // write the new tail
  uint32_t settle;              // the stream settles frames or ends in this push
  uint32_t win;                 // index of the window among the push's windows (~0u: none)
  uint32_t w0;                  // absolute frame of the window's first frame
  uint32_t keep_lo, keep_hi;    // settled frames, relative to the window: [H_prev - w0, H - w0)
  uint32_t h_new;               // settled horizon after the push (absolute frames)
  uint32_t ending;
  uint32_t pend_n;              // carried peaks before the push
};

// per-job results the write kernel and the host read: [0] = total hashes (u64, by the scan); then h[J] u64, e[J] u32,
// m[J] u32, kl[J] u32, kh[J] u32
struct st_ctl_view {
  unsigned long long* total;
  uint64_t* h;
  uint32_t *e, *m, *kl, *kh;
};

// where the peaks that a push settled lie, per stream, for the peak-window listeners (internal: not on the ABI): pf / pt of
// the object at [at, at + n), frames relative to w0.  Valid from a push that succeeded until the next call on the streams
struct st_hand {
  uint64_t at;
  uint32_t n, w0;
};

struct shz_streams {
  shz_ctx* ctx = nullptr;
  uint32_t n = 0, fs = 0, fan = 0, hop = 0;
  double amp_min = 0.0;
  uint64_t tail_cap = 0;                   // samples per tail slot (a tail is < 20 hop + 4096)
  int16_t* d_tail = nullptr;               // [2][n][tail_cap]
  uint16_t* d_pend_f = nullptr;            // [2][n][ST_PEND]
  uint32_t* d_pend_t = nullptr;
  std::vector<uint64_t> samples, settled, emitted;
  std::vector<uint32_t> pending;
  std::vector<uint8_t> ended, par_tail, par_pend;
  shz_buf win, pf, pt, pcm, jobs, poff, ctl, offs, ok, ot;   // grow-only device scratch of the object
  uint64_t peak_cap = 0;                   // peak list capacity the windows needed so far
  std::vector<st_hand> hand;               // the last push's newly settled peaks (n = 0: none)
};

// ---- kernels -------------------------------------------------------------------------------------------------------
// tail ++ chunk of job blockIdx.y -> its window (first win_len samples) and its new tail (from ntail_lo on)
__global__ __launch_bounds__(ST_THREADS) void stream_gather_kernel(const st_job* __restrict__ jobs, const int16_t* __restrict__ pcm,
                                                                   int16_t* __restrict__ tails, uint64_t tail_cap, uint32_t n_streams,
                                                                   int16_t* __restrict__ win) {
  const st_job j = jobs[blockIdx.y];
  const uint64_t len = j.tail + j.chunk;
  const uint64_t lim = j.do_tail ? len : j.win_len;   // (no new tail: nothing behind the window is needed)
  const int16_t* tin = tails + ((uint64_t)j.tail_in * n_streams + j.stream) * tail_cap;
  int16_t* tout = tails + ((uint64_t)j.tail_out * n_streams + j.stream) * tail_cap;
  for (uint64_t k = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x; k < lim; k += (uint64_t)gridDim.x * ST_THREADS) {
    const int16_t v = k < j.tail ? tin[k] : pcm[j.src + (k - j.tail)];
    if (k < j.win_len) win[j.win_dst + k] = v;
    if (j.do_tail && k >= j.ntail_lo) tout[k - j.ntail_lo] = v;
  }
}

// the settled list of a stream: carried peaks, then the window's kept peaks shifted to absolute frames
struct st_list {
  const uint16_t* cf;
  const uint32_t* ct;
  uint32_t p;
  const uint16_t* nf;
  const uint32_t* nt;
  uint32_t w0;
  __device__ uint32_t t(uint32_t i) const { return i < p ? ct[i] : nt[i - p] + w0; }
  __device__ uint32_t f(uint32_t i) const { return i < p ? (uint32_t)cf[i] : (uint32_t)nf[i - p]; }
};

// first index in [lo, hi) of a[] with a[i] >= x (a ascending)
__device__ inline uint64_t st_lower_bound(const uint32_t* a, uint64_t lo, uint64_t hi, uint32_t x) {
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// partners of peak i of the list (the rule of generate_hashes: i + 1 .. i + fan - 1 inside the list, 0 <= dt <= 200)
__device__ inline uint32_t st_partners(const st_list& L, uint32_t i, uint32_t m, uint32_t fan) {
  const uint32_t t1 = L.t(i);
  uint32_t c = 0;
  for (uint32_t jn = 1; jn < fan && i + jn < m; ++jn)
    if (L.t(i + jn) - t1 <= SHZ_MAX_DT) ++c;
  return c;
}

// exclusive prefix of v over the 256 threads (4 waves of 64), block total in *tot
__device__ inline uint32_t st_block_scan(uint32_t v, uint32_t* s_w, uint32_t* tot) {
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t x = v;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  uint32_t pre = 0, all = 0;
  for (uint32_t i = 0; i < ST_THREADS / 64; ++i) {
    const uint32_t s = s_w[i];
    if (i < w) pre += s;
    all += s;
  }
  __syncthreads();
  *tot = all;
  return pre + x - v;
}

__device__ inline st_list st_make_list(const st_job& j, uint32_t n_streams, const uint16_t* pend_f, const uint32_t* pend_t,
                                       const uint16_t* pf, const uint32_t* pt, const uint64_t* poff, uint32_t kl) {
  st_list L;
  const uint64_t slot = ((uint64_t)j.pend_in * n_streams + j.stream) * ST_PEND;
  L.cf = pend_f + slot;
  L.ct = pend_t + slot;
  L.p = j.pend_n;
  const uint64_t k0 = j.win != ~0u ? poff[j.win] + kl : 0;
  L.nf = pf + k0;
  L.nt = pt + k0;
  L.w0 = j.w0;
  return L;
}

// per job: the window's settled peaks [kl, kh), the list length m, the emitted prefix e and its number of hashes
__global__ __launch_bounds__(ST_THREADS) void stream_count_kernel(const st_job* __restrict__ jobs, uint32_t n_streams, uint32_t fan,
                                                                  const uint16_t* __restrict__ pend_f, const uint32_t* __restrict__ pend_t,
                                                                  const uint16_t* __restrict__ pf, const uint32_t* __restrict__ pt,
                                                                  const uint64_t* __restrict__ poff, st_ctl_view cv) {
  const uint32_t ji = blockIdx.x;
  const st_job j = jobs[ji];
  __shared__ uint32_t s_kl, s_kh, s_m, s_e, s_w[ST_THREADS / 64];
  if (!j.settle) {
    if (threadIdx.x == 0) { cv.h[ji] = 0; cv.e[ji] = 0; cv.m[ji] = j.pend_n; cv.kl[ji] = 0; cv.kh[ji] = 0; }
    return;
  }
  if (threadIdx.x == 0) {
    uint32_t kl = 0, kh = 0;
    if (j.win != ~0u) {
      const uint64_t a = poff[j.win], b = poff[j.win + 1];
      kl = (uint32_t)(st_lower_bound(pt, a, b, j.keep_lo) - a);
      kh = (uint32_t)(st_lower_bound(pt, a, b, j.keep_hi) - a);
    }
    const st_list L = st_make_list(j, n_streams, pend_f, pend_t, pf, pt, poff, kl);
    const uint32_t m = j.pend_n + (kh - kl);
    uint32_t e = m;
    if (!j.ending) {
      const uint32_t by_fan = m >= fan - 1 ? m - (fan - 1) : 0;             // (a)
      uint32_t by_dt = 0;                                                    // (b): t_i + 200 < H
      if (j.h_new > SHZ_MAX_DT) {
        uint32_t lo = 0, hi = m;
        const uint32_t x = j.h_new - SHZ_MAX_DT;
        while (lo < hi) {
          const uint32_t mid = (lo + hi) >> 1;
          if (L.t(mid) < x) lo = mid + 1;
          else hi = mid;
        }
        by_dt = lo;
      }
      e = by_fan > by_dt ? by_fan : by_dt;
    }
    s_kl = kl;
    s_kh = kh;
    s_m = m;
    s_e = e;
  }
  __syncthreads();
  const uint32_t kl = s_kl, m = s_m, e = s_e;
  const st_list L = st_make_list(j, n_streams, pend_f, pend_t, pf, pt, poff, kl);
  uint64_t h = 0;
  for (uint32_t i0 = 0; i0 < e; i0 += ST_THREADS) {
    const uint32_t i = i0 + threadIdx.x;
    uint32_t tot;
    (void)st_block_scan(i < e ? st_partners(L, i, m, fan) : 0, s_w, &tot);
    h += tot;
  }
  if (threadIdx.x == 0) {
    cv.h[ji] = h;
    cv.e[ji] = e;
    cv.m[ji] = m;
    cv.kl[ji] = kl;
    cv.kh[ji] = s_kh;
  }
}

// per job: the emitted prefix's hashes at offs[ji] (if the total fits cap), the rest of the list into the other pending slot
__global__ __launch_bounds__(ST_THREADS) void stream_write_kernel(const st_job* __restrict__ jobs, uint32_t n_streams, uint32_t fan,
                                                                  uint16_t* __restrict__ pend_f, uint32_t* __restrict__ pend_t,
                                                                  const uint16_t* __restrict__ pf, const uint32_t* __restrict__ pt,
                                                                  const uint64_t* __restrict__ poff, st_ctl_view cv,
                                                                  const uint64_t* __restrict__ offs, uint32_t* __restrict__ key32,
                                                                  uint32_t* __restrict__ t1out, uint64_t cap) {
  const uint32_t ji = blockIdx.x;
  const st_job j = jobs[ji];
  if (!j.settle) return;
  __shared__ uint32_t s_w[ST_THREADS / 64];
  const uint32_t e = cv.e[ji], m = cv.m[ji];
  const st_list L = st_make_list(j, n_streams, pend_f, pend_t, pf, pt, poff, cv.kl[ji]);
  if (*cv.total <= cap) {   // (uniform) otherwise the call reports SHZ_E_CAPACITY and writes nothing
    uint64_t o = offs[ji];
    for (uint32_t i0 = 0; i0 < e; i0 += ST_THREADS) {
      const uint32_t i = i0 + threadIdx.x;
      uint32_t tot;
      const uint32_t ex = st_block_scan(i < e ? st_partners(L, i, m, fan) : 0, s_w, &tot);
      if (i < e) {
        const uint32_t ta = L.t(i), fa = L.f(i);
        uint64_t q = o + ex;
        for (uint32_t jn = 1; jn < fan && i + jn < m; ++jn) {
          const uint32_t dt = L.t(i + jn) - ta;
          if (dt <= SHZ_MAX_DT) {
            key32[q] = (fa << 20) | (L.f(i + jn) << 8) | dt;
            t1out[q] = ta;
            ++q;
          }
        }
      }
      o += tot;
    }
  }
  // carried peaks: list[e, m) (at most fan - 1 of them) into the other slot -- the input slot stays intact, so a call
  // that fails leaves the stream as it was
  const uint64_t slot = ((uint64_t)j.pend_out * n_streams + j.stream) * ST_PEND;
  const uint32_t r = m - e;
  if (threadIdx.x < r && threadIdx.x < ST_PEND) {
    pend_f[slot + threadIdx.x] = (uint16_t)L.f(e + threadIdx.x);
    pend_t[slot + threadIdx.x] = L.t(e + threadIdx.x);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
static inline uint64_t st_frames_complete(uint64_t n, uint32_t hop) { return n >= SHZ_NFFT ? (n - SHZ_NFFT) / hop + 1 : 0; }

extern "C" int32_t shz_stream_plan(uint64_t samples_before, uint64_t samples_after, uint64_t settled_before, uint32_t hop,
                                   int32_t ending, uint64_t* win_frame0, uint64_t* win_s0, uint64_t* win_s1,
                                   uint64_t* settled_after) {
  if (hop < 1 || hop > SHZ_NFFT || samples_after < samples_before) return SHZ_E_INVALID;
  const uint64_t c = st_frames_complete(samples_after, hop);
  // at the end the true right edge settles every frame (a stream shorter than 4096 samples: one zero-padded frame)
  const uint64_t h = ending ? (samples_after >= SHZ_NFFT ? c : 1) : (c > SHZ_PEAK_RADIUS ? c - SHZ_PEAK_RADIUS : 0);
  if (h < settled_before) return SHZ_E_INVALID;   // settled_before is not a horizon of this stream
  const uint64_t w0 = settled_before > SHZ_PEAK_RADIUS ? settled_before - SHZ_PEAK_RADIUS : 0;
  if (win_frame0) *win_frame0 = w0;
  if (win_s0) *win_s0 = w0 * hop;
  if (win_s1) *win_s1 = h == settled_before ? w0 * hop : ending ? samples_after : (c - 1) * hop + SHZ_NFFT;
  if (settled_after) *settled_after = h;
  return SHZ_OK;
}

static void st_free(shz_buf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

// grow-only device buffer of the stream object (contents not kept)
static int32_t st_reserve(shz_ctx* ctx, shz_buf& b, uint64_t bytes, void** out) {
  if (bytes == 0) bytes = 256;
  if (b.cap < bytes) {
    if (b.p) {
      SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
      st_free(b);
    }
    const uint64_t want = bytes + bytes / 4;
    if (hipMalloc(&b.p, want) != hipSuccess) {
      b.p = nullptr;
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "streams: hipMalloc(%llu) failed", (unsigned long long)want);
    }
    b.cap = want;
  }
  *out = b.p;
  return SHZ_OK;
}

extern "C" int32_t shz_streams_create(shz_ctx* ctx, uint32_t n_streams, uint32_t fs, double amp_min, uint32_t fan_value,
                                      shz_streams** out) {
  if (!ctx || !out) return SHZ_E_INVALID;
  *out = nullptr;
  if (n_streams == 0 || n_streams > ST_MAX_STREAMS) SHZ_FAIL(ctx, SHZ_E_INVALID, "n_streams must be in [1, %u]", ST_MAX_STREAMS);
  if (fs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "Fs must be > 0");
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  shz_streams* s = new shz_streams();
  s->ctx = ctx;
  s->n = n_streams;
  s->fs = fs;
  s->fan = fan_value;
  s->hop = ctx->hop;
  s->amp_min = amp_min;
  s->tail_cap = 20ull * s->hop + SHZ_NFFT;
  s->samples.assign(n_streams, 0);
  s->settled.assign(n_streams, 0);
  s->emitted.assign(n_streams, 0);
  s->pending.assign(n_streams, 0);
  s->ended.assign(n_streams, 0);
  s->par_tail.assign(n_streams, 0);
  s->par_pend.assign(n_streams, 0);
  s->hand.assign(n_streams, st_hand{0, 0, 0});
  const uint64_t tb = 2ull * n_streams * s->tail_cap * 2, pb = 2ull * n_streams * ST_PEND;
  if (hipMalloc(&s->d_tail, tb) != hipSuccess || hipMalloc(&s->d_pend_f, pb * 2) != hipSuccess ||
      hipMalloc(&s->d_pend_t, pb * 4) != hipSuccess) {
    shz_streams_destroy(s);
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "streams: %u streams need %llu bytes of device memory", n_streams,
             (unsigned long long)(tb + pb * 6));
  }
  *out = s;
  return SHZ_OK;
}

extern "C" int32_t shz_streams_destroy(shz_streams* s) {
  if (!s) return SHZ_E_INVALID;
  if (s->ctx) {
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
  }
  if (s->d_tail) (void)hipFree(s->d_tail);
  if (s->d_pend_f) (void)hipFree(s->d_pend_f);
  if (s->d_pend_t) (void)hipFree(s->d_pend_t);
  for (shz_buf* b : {&s->win, &s->pf, &s->pt, &s->pcm, &s->jobs, &s->poff, &s->ctl, &s->offs, &s->ok, &s->ot}) st_free(*b);
  delete s;
  return SHZ_OK;
}

static int32_t st_check(shz_streams* s) {
  if (!s || !s->ctx) return SHZ_E_INVALID;
  if (s->ctx->hop != s->hop)
    SHZ_FAIL(s->ctx, SHZ_E_STATE, "streams were created with hop %u, the context's hop is now %u", s->hop, s->ctx->hop);
  return SHZ_OK;
}

extern "C" int32_t shz_streams_reset(shz_streams* s, const uint32_t* which, uint32_t n) {
  SHZ_TRY(st_check(s));
  if (n && !which) SHZ_FAIL(s->ctx, SHZ_E_INVALID, "which is NULL");
  for (uint32_t i = 0; i < n; ++i)
    if (which[i] >= s->n) SHZ_FAIL(s->ctx, SHZ_E_INVALID, "stream %u out of range (%u streams)", which[i], s->n);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t k = which[i];
    s->samples[k] = s->settled[k] = s->emitted[k] = 0;
    s->pending[k] = 0;
    s->ended[k] = 0;
  }
  return SHZ_OK;
}

extern "C" int32_t shz_streams_state(shz_streams* s, uint32_t i, uint64_t* samples, uint64_t* settled, uint64_t* pending,
                                     uint64_t* emitted) {
  SHZ_TRY(st_check(s));
  if (i >= s->n) SHZ_FAIL(s->ctx, SHZ_E_INVALID, "stream %u out of range (%u streams)", i, s->n);
  if (samples) *samples = s->samples[i];
  if (settled) *settled = s->settled[i];
  if (pending) *pending = s->pending[i];
  if (emitted) *emitted = s->emitted[i];
  return SHZ_OK;
}

extern "C" int32_t shz_streams_push(shz_streams* s, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                    uint32_t flags, uint32_t* key32, uint32_t* t1, uint64_t* hash_off, uint64_t cap,
                                    uint64_t* count) {
  SHZ_TRY(st_check(s));
  shz_ctx* ctx = s->ctx;
  if (count) *count = 0;
  if (!chunk_off || !hash_off || !count) SHZ_FAIL(ctx, SHZ_E_INVALID, "chunk_off, hash_off and count must not be NULL");
  const uint32_t n = s->n, hop = s->hop;
  s->hand.assign(n, st_hand{0, 0, 0});
  for (uint32_t i = 0; i < n; ++i)
    if (chunk_off[i + 1] < chunk_off[i]) SHZ_FAIL(ctx, SHZ_E_INVALID, "chunk_off decreases at stream %u", i);
  const uint64_t in_total = chunk_off[n] - chunk_off[0];
  if (in_total && !pcm) SHZ_FAIL(ctx, SHZ_E_INVALID, "pcm is NULL");
  if (cap && (!key32 || !t1)) SHZ_FAIL(ctx, SHZ_E_INVALID, "key32 / t1 is NULL");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  // 1) the plan of every stream, on the host
  std::vector<st_job> jobs;
  std::vector<uint64_t> win_off(1, 0);   // window clips, CSR in the window buffer
  std::vector<uint64_t> h_after(n);
  uint64_t win_frames = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t len = chunk_off[i + 1] - chunk_off[i];
    const bool e = end && ((end[i >> 5] >> (i & 31)) & 1u);
    if (s->ended[i]) {
      if (len || e) SHZ_FAIL(ctx, SHZ_E_STATE, "stream %u has ended; reset it before pushing to it again", i);
      continue;
    }
    if (!len && !e) continue;
    const uint64_t sb = s->samples[i], sa = sb + len, hb = s->settled[i];
    uint64_t wf0, ws0, ws1, ha;
    if (shz_stream_plan(sb, sa, hb, hop, e ? 1 : 0, &wf0, &ws0, &ws1, &ha) != SHZ_OK)
      SHZ_FAIL(ctx, SHZ_E_STATE, "stream %u: inconsistent state (samples %llu, settled %llu)", i, (unsigned long long)sb,
               (unsigned long long)hb);
    if (ha >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "stream %u: more than 2^31 frames", i);
    const uint64_t tail_s0 = (hb > SHZ_PEAK_RADIUS ? hb - SHZ_PEAK_RADIUS : 0) * hop;   // == ws0
    st_job j;
    memset(&j, 0, sizeof(j));
    j.src = chunk_off[i] - ((flags & SHZ_PCM_DEVICE) ? 0 : chunk_off[0]);
    j.chunk = len;
    j.tail = sb - tail_s0;
    j.win_len = ws1 - ws0;
    j.win_dst = win_off.back();
    j.stream = i;
    j.tail_in = s->par_tail[i];
    j.tail_out = s->par_tail[i] ^ 1u;
    j.pend_in = s->par_pend[i];
    j.pend_out = s->par_pend[i] ^ 1u;
    j.do_tail = !e && len;
    const uint64_t ntail_s0 = (ha > SHZ_PEAK_RADIUS ? ha - SHZ_PEAK_RADIUS : 0) * hop;
    j.ntail_lo = ntail_s0 - tail_s0;
    if (j.do_tail && sa - ntail_s0 > s->tail_cap)
      SHZ_FAIL(ctx, SHZ_E_STATE, "stream %u: carried tail of %llu samples exceeds its slot (%llu)", i,
               (unsigned long long)(sa - ntail_s0), (unsigned long long)s->tail_cap);
    j.settle = ha > hb || e;
    j.win = ~0u;
    if (ha > hb) {
      j.win = (uint32_t)(win_off.size() - 1);
      win_off.push_back(win_off.back() + j.win_len);
      win_frames += shz_frame_count_hop(j.win_len, hop);
    }
    j.w0 = (uint32_t)wf0;
    j.keep_lo = (uint32_t)(hb - wf0);
    j.keep_hi = (uint32_t)(ha - wf0);
    j.h_new = (uint32_t)ha;
    j.ending = e;
    j.pend_n = s->pending[i];
    h_after[i] = ha;
    jobs.push_back(j);
  }
  for (uint32_t i = 0; i <= n; ++i) hash_off[i] = 0;
  if (jobs.empty()) return SHZ_OK;
  const uint32_t nj = (uint32_t)jobs.size(), nw = (uint32_t)(win_off.size() - 1);
  // 2) PCM on the device, jobs up, windows and new tails in one launch
  const int16_t* d_pcm = pcm;
  if (!(flags & SHZ_PCM_DEVICE) && in_total) {
    void* p;
    SHZ_TRY(st_reserve(ctx, s->pcm, in_total * 2, &p));
    SHZ_HIP(ctx, shz_memcpy(ctx, p, pcm + chunk_off[0], in_total * 2, hipMemcpyHostToDevice));
    d_pcm = (const int16_t*)p;
  }
  void *d_jobs, *d_win;
  SHZ_TRY(st_reserve(ctx, s->jobs, (uint64_t)nj * sizeof(st_job), &d_jobs));
  SHZ_TRY(st_reserve(ctx, s->win, win_off.back() * 2 + 64, &d_win));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_jobs, jobs.data(), (uint64_t)nj * sizeof(st_job), hipMemcpyHostToDevice));
  uint64_t max_len = 0;
  for (const st_job& j : jobs) max_len = std::max(max_len, j.do_tail ? j.tail + j.chunk : j.win_len);
  if (max_len) {
    const uint32_t gx = (uint32_t)std::min<uint64_t>((max_len + ST_THREADS * 4 - 1) / (ST_THREADS * 4), 64);
    hipLaunchKernelGGL(stream_gather_kernel, dim3(gx, nj), dim3(ST_THREADS), 0, ctx->stream, (const st_job*)d_jobs, d_pcm,
                       s->d_tail, s->tail_cap, n, (int16_t*)d_win);
    SHZ_HIP(ctx, hipGetLastError());
  }
  bool any_settle = false;
  for (const st_job& j : jobs) any_settle |= j.settle != 0;
  if (!any_settle) {   // samples arrived, nothing settles: the tails are all that changes (no read-back, no sync)
    for (const st_job& j : jobs) {
      s->samples[j.stream] += j.chunk;
      if (j.do_tail) s->par_tail[j.stream] ^= 1u;
    }
    return SHZ_OK;
  }
  // 3) the windows as clips through the extraction pass; peaks stay on the device
  std::vector<uint64_t> poff(nw + 1, 0);
  void *d_pf = nullptr, *d_pt = nullptr, *d_poff;
  if (nw) {
    uint64_t pcap = std::max<uint64_t>(s->peak_cap, win_frames * 16 + 4096);
    for (int attempt = 0;; ++attempt) {
      SHZ_TRY(st_reserve(ctx, s->pf, pcap * 2 + 64, &d_pf));
      SHZ_TRY(st_reserve(ctx, s->pt, pcap * 4 + 64, &d_pt));
      uint64_t cnt = 0;
      const int32_t rc = shz_peaks(ctx, (const int16_t*)d_win, win_off.data(), nw, s->fs, s->amp_min,
                                   SHZ_PCM_DEVICE | SHZ_OUT_DEVICE, (uint16_t*)d_pf, (uint32_t*)d_pt, poff.data(), pcap, &cnt);
      if (rc == SHZ_E_CAPACITY && attempt < 4) {
        pcap = std::max(cnt + cnt / 8, 2 * pcap);
        continue;
      }
      SHZ_TRY(rc);
      s->peak_cap = std::max(s->peak_cap, cnt + cnt / 8);
      break;
    }
    if (poff[nw] >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "more than 2^31 peaks in one push");
  }
  SHZ_TRY(st_reserve(ctx, s->poff, (uint64_t)(nw + 1) * 8, &d_poff));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_poff, poff.data(), (uint64_t)(nw + 1) * 8, hipMemcpyHostToDevice));
  // upper bound of this push's hashes: every settled peak with all fan - 1 partners
  uint64_t bound = 0;
  for (const st_job& j : jobs)
    if (j.settle) bound += ((uint64_t)j.pend_n + (j.win != ~0u ? poff[j.win + 1] - poff[j.win] : 0)) * (s->fan - 1);
  // 4) count, scan over the jobs, write
  const uint64_t c_h = 64, c_e = c_h + ((uint64_t)nj * 8 + 63) / 64 * 64, c_m = c_e + ((uint64_t)nj * 4 + 63) / 64 * 64,
                 c_kl = c_m + ((uint64_t)nj * 4 + 63) / 64 * 64, c_kh = c_kl + ((uint64_t)nj * 4 + 63) / 64 * 64,
                 c_bytes = c_kh + (uint64_t)nj * 4;
  void *d_ctl, *d_offs;
  SHZ_TRY(st_reserve(ctx, s->ctl, c_bytes, &d_ctl));
  SHZ_TRY(st_reserve(ctx, s->offs, (uint64_t)nj * 8, &d_offs));
  char* cb = (char*)d_ctl;
  st_ctl_view cv{(unsigned long long*)cb, (uint64_t*)(cb + c_h), (uint32_t*)(cb + c_e), (uint32_t*)(cb + c_m),
                 (uint32_t*)(cb + c_kl), (uint32_t*)(cb + c_kh)};
  const bool out_dev = (flags & SHZ_OUT_DEVICE) != 0;
  uint32_t *o_k = key32, *o_t = t1;
  uint64_t o_cap = cap;
  if (!out_dev) {   // staging sized by the bound: it never overflows; the caller's cap is checked on the host
    void *a, *b;
    SHZ_TRY(st_reserve(ctx, s->ok, bound * 4 + 64, &a));
    SHZ_TRY(st_reserve(ctx, s->ot, bound * 4 + 64, &b));
    o_k = (uint32_t*)a;
    o_t = (uint32_t*)b;
    o_cap = std::min(cap, bound);
  }
  hipLaunchKernelGGL(stream_count_kernel, dim3(nj), dim3(ST_THREADS), 0, ctx->stream, (const st_job*)d_jobs, n, s->fan,
                     (const uint16_t*)s->d_pend_f, (const uint32_t*)s->d_pend_t, (const uint16_t*)d_pf, (const uint32_t*)d_pt,
                     (const uint64_t*)d_poff, cv);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u64(ctx, cv.h, (uint64_t*)d_offs, nj, (uint64_t*)cv.total));
  hipLaunchKernelGGL(stream_write_kernel, dim3(nj), dim3(ST_THREADS), 0, ctx->stream, (const st_job*)d_jobs, n, s->fan,
                     s->d_pend_f, s->d_pend_t, (const uint16_t*)d_pf, (const uint32_t*)d_pt, (const uint64_t*)d_poff, cv,
                     (const uint64_t*)d_offs, o_k, o_t, o_cap);
  SHZ_HIP(ctx, hipGetLastError());
  // 5) one read-back: total, per-job hash counts, emitted prefixes, list lengths and settled ranges
  void* mailp;
  SHZ_TRY(shz_mailbox(ctx, c_bytes, &mailp));
  SHZ_HIP(ctx, hipMemcpyAsync(mailp, d_ctl, c_bytes, hipMemcpyDeviceToHost, ctx->stream));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const char* mb = (const char*)mailp;
  const uint64_t total = *(const uint64_t*)mb;
  *count = total;
  if (total > bound) SHZ_FAIL(ctx, SHZ_E_STATE, "streams: %llu hashes exceed their bound %llu", (unsigned long long)total,
                              (unsigned long long)bound);
  if (total > cap)
    SHZ_FAIL(ctx, SHZ_E_CAPACITY, "output needs %llu entries, capacity %llu", (unsigned long long)total, (unsigned long long)cap);
  const uint64_t* hh = (const uint64_t*)(mb + c_h);
  const uint32_t *ee = (const uint32_t*)(mb + c_e), *mm = (const uint32_t*)(mb + c_m), *kkl = (const uint32_t*)(mb + c_kl),
                 *kkh = (const uint32_t*)(mb + c_kh);
  std::vector<uint64_t> per(n, 0);
  for (uint32_t k = 0; k < nj; ++k) per[jobs[k].stream] = hh[k];
  if (!out_dev && total) {
    SHZ_HIP(ctx, shz_memcpy(ctx, key32, o_k, total * 4, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, shz_memcpy(ctx, t1, o_t, total * 4, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  // 6) commit: the streams advance only now
  for (uint32_t i = 0; i < n; ++i) hash_off[i + 1] = hash_off[i] + per[i];
  for (uint32_t k = 0; k < nj; ++k) {
    const st_job& j = jobs[k];
    const uint32_t i = j.stream;
    s->samples[i] += j.chunk;
    if (j.do_tail) s->par_tail[i] ^= 1u;
    if (j.settle) {
      s->settled[i] = h_after[i];
      s->pending[i] = mm[k] - ee[k];
      s->emitted[i] += hh[k];
      s->par_pend[i] ^= 1u;
      if (j.win != ~0u && kkh[k] >= kkl[k] && poff[j.win] + kkh[k] <= poff[j.win + 1])
        s->hand[i] = st_hand{poff[j.win] + kkl[k], kkh[k] - kkl[k], j.w0};
    }
    if (j.ending) s->ended[i] = 1;
  }
  return SHZ_OK;
}

// ---- device-resident listeners -------------------------------------------------------------------------------------
// A listener is `channels` adjacent streams whose settled hashes are unioned (recognizer.py:377-382) and recognised from a
// sliding window: the hashes with t1 >= w0 = max(0, H - window_frames), H the smallest settled horizon of its channels,
// query offsets t1 - w0.  The windows live on the device as two packed slots of (key32, absolute t1) columns, listener l's
// entries at [w_at[l], w_at[l] + w_n[l]) of the current slot.  One push: the streams' push with device output, one small
// upload (per listener: where its old and its new entries are, and w0), window_count_kernel, a scan over the listeners,
// window_write_kernel -- kept old entries, then kept new ones, compacted in order into the OTHER slot, and in the same
// pass the query offsets t1 - w0 beside them (the query's key column is the new window's) -- one read-back of the counts,
// which are the match's query_off, and the match on device input.  The slots flip once the counts are back, so a push that
// fails before leaves every window as it was.

#define LS_THREADS 256

// One job of the window stage, which hash windows (one job per listener) and peak windows (one per stream) share.
struct win_job {
  uint64_t old_at, new_at;   // first old entry in the current slot; first new entry in the push's lists
  uint32_t old_n, new_n;
  uint32_t w0, add;          // the window start; what makes a new t absolute (peaks: the first frame of the stream's window clip)
};

struct shz_listeners {
  shz_streams* s = nullptr;
  shz_table* t = nullptr;
  shz_ctx* ctx = nullptr;
  uint32_t n = 0, channels = 0, window_frames = 0;
  shz_buf wk[2], wt[2];            // the two window slots
  uint32_t cur = 0;                // the slot that holds the windows
  std::vector<uint64_t> w_at;
  std::vector<uint32_t> w_n, w0;
  shz_buf nk, nt;                  // the hashes of a push
  uint64_t new_cap = 0;            // entries nk / nt hold
  shz_buf qo, jobs, ctl;           // query offsets; the window stage's jobs; total | counts | offsets
  // peak windows (shz_listeners_create_peaks): per STREAM, the settled peaks with t >= w0 of its listener
  bool peaks = false;
  shz_buf pf[2], pt[2], pr;        // the two slots of (f, absolute t); the times t - w0 beside the current slot
  std::vector<uint64_t> p_at;      // per stream: its window in the current slot
  std::vector<uint32_t> p_n, last_nhash;   // ...; per listener: out_nhash of the last push's chosen variant
  bool timed = false;              // shz_listeners_timing
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // push begun, streams done, windows done
  float ms[4] = {0.f, 0.f, 0.f, 0.f};               // streams, window, warp, match of the last push
};

// entry i of a job's old-then-new list (payload, absolute t) and whether the window keeps it
template <class P>
__device__ __forceinline__ bool win_entry(const win_job& j, uint32_t i, const P* __restrict__ wp, const uint32_t* __restrict__ wt,
                                          const P* __restrict__ np, const uint32_t* __restrict__ nt, P* p, uint32_t* t) {
  if (i >= j.old_n + j.new_n) return false;
  if (i < j.old_n) {
    *t = wt[j.old_at + i];
    if (p) *p = wp[j.old_at + i];
  } else {
    *t = nt[j.new_at + (i - j.old_n)] + j.add;
    if (p) *p = np[j.new_at + (i - j.old_n)];
  }
  return *t >= j.w0;
}

// per job: entries its window keeps (one ballot per 64 entries, the waves' sums through LDS)
__global__ __launch_bounds__(LS_THREADS) void window_count_kernel(const win_job* __restrict__ jobs, const uint32_t* __restrict__ wt,
                                                                  const uint32_t* __restrict__ nt, uint64_t* __restrict__ cnt) {
  const win_job j = jobs[blockIdx.x];
  const uint32_t n = j.old_n + j.new_n;
  __shared__ uint32_t s_w[LS_THREADS / 64];
  uint32_t c = 0;   // (the same in every lane of a wave)
  for (uint32_t i0 = 0; i0 < n; i0 += LS_THREADS) {
    uint32_t t;
    const bool keep = win_entry<uint32_t>(j, i0 + threadIdx.x, nullptr, wt, nullptr, nt, nullptr, &t);
    c += (uint32_t)__popcll(__ballot(keep));
  }
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t all = 0;
    for (uint32_t i = 0; i < LS_THREADS / 64; ++i) all += s_w[i];
    cnt[blockIdx.x] = all;
  }
}

// per job: the kept entries, in order, at offs[job] of the other slot, and their times relative to the window start
template <class P>
__global__ __launch_bounds__(LS_THREADS) void window_write_kernel(const win_job* __restrict__ jobs, const P* __restrict__ wp,
                                                                  const uint32_t* __restrict__ wt, const P* __restrict__ np,
                                                                  const uint32_t* __restrict__ nt, const uint64_t* __restrict__ offs,
                                                                  const unsigned long long* __restrict__ total, uint64_t cap,
                                                                  P* __restrict__ wp_out, uint32_t* __restrict__ wt_out,
                                                                  uint32_t* __restrict__ rel) {
  if (*total > cap) return;   // (uniform; the host sizes the slots by a bound, so this never holds: it keeps a wrong bound harmless)
  const win_job j = jobs[blockIdx.x];
  const uint32_t n = j.old_n + j.new_n, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __shared__ uint32_t s_w[2][LS_THREADS / 64];
  uint64_t o = offs[blockIdx.x];
  for (uint32_t i0 = 0, it = 0; i0 < n; i0 += LS_THREADS, ++it) {   // (n is the block's: every wave makes every round)
    P v = 0;
    uint32_t t = 0;
    const bool keep = win_entry<P>(j, i0 + threadIdx.x, wp, wt, np, nt, &v, &t);
    const unsigned long long b = __ballot(keep);
    const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    uint32_t* sw = s_w[it & 1];   // (two rows: a wave may start the next round while another still reads this one's sums)
    if (lane == 0) sw[w] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (uint32_t i = 0; i < LS_THREADS / 64; ++i) {
      const uint32_t x = sw[i];
      if (i < w) base += x;
      all += x;
    }
    if (keep) {
      const uint64_t q = o + base + pre;
      wp_out[q] = v;
      wt_out[q] = t;
      rel[q] = t - j.w0;
    }
    o += all;
  }
}

static int32_t ls_create(shz_streams* s, shz_table* t, uint32_t n_listeners, uint32_t window_frames, bool peaks,
                         shz_listeners** out) {
  if (!s || !s->ctx || !out) return SHZ_E_INVALID;
  *out = nullptr;
  shz_ctx* ctx = s->ctx;
  if (!t || t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "listeners: the table must belong to the streams' ctx");
  if (n_listeners == 0 || s->n % n_listeners != 0)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "listeners: %u listeners do not divide %u streams into channels", n_listeners, s->n);
  if (window_frames >= (1u << 20)) SHZ_FAIL(ctx, SHZ_E_INVALID, "listeners: window_frames must be < 2^20 (query offsets)");
  shz_listeners* L = new shz_listeners();
  L->s = s;
  L->t = t;
  L->ctx = ctx;
  L->n = n_listeners;
  L->channels = s->n / n_listeners;
  L->window_frames = window_frames;
  L->w_at.assign(n_listeners, 0);
  L->w_n.assign(n_listeners, 0);
  L->w0.assign(n_listeners, 0);
  L->peaks = peaks;
  L->p_at.assign(s->n, 0);
  L->p_n.assign(s->n, 0);
  L->last_nhash.assign(n_listeners, 0);
  *out = L;
  return SHZ_OK;
}

extern "C" int32_t shz_listeners_create(shz_streams* s, shz_table* t, uint32_t n_listeners, uint32_t window_frames,
                                        shz_listeners** out) {
  return ls_create(s, t, n_listeners, window_frames, false, out);
}

extern "C" int32_t shz_listeners_create_peaks(shz_streams* s, shz_table* t, uint32_t n_listeners, uint32_t window_frames,
                                              shz_listeners** out) {
  return ls_create(s, t, n_listeners, window_frames, true, out);
}

extern "C" int32_t shz_listeners_destroy(shz_listeners* L) {
  if (!L) return SHZ_E_INVALID;
  if (L->ctx) {
    (void)hipSetDevice(L->ctx->device);
    (void)hipStreamSynchronize(L->ctx->stream);
  }
  for (shz_buf* b : {&L->wk[0], &L->wk[1], &L->wt[0], &L->wt[1], &L->nk, &L->nt, &L->qo, &L->jobs, &L->ctl, &L->pf[0], &L->pf[1],
                     &L->pt[0], &L->pt[1], &L->pr})
    st_free(*b);
  for (hipEvent_t e : L->ev)
    if (e) (void)hipEventDestroy(e);
  delete L;
  return SHZ_OK;
}

static int32_t ls_check(shz_listeners* L) {
  if (!L || !L->s) return SHZ_E_INVALID;
  return st_check(L->s);
}

extern "C" int32_t shz_listeners_reset(shz_listeners* L, const uint32_t* which, uint32_t n) {
  SHZ_TRY(ls_check(L));
  if (n && !which) SHZ_FAIL(L->ctx, SHZ_E_INVALID, "which is NULL");
  for (uint32_t i = 0; i < n; ++i)
    if (which[i] >= L->n) SHZ_FAIL(L->ctx, SHZ_E_INVALID, "listener %u out of range (%u listeners)", which[i], L->n);
  std::vector<uint32_t> streams;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t c = 0; c < L->channels; ++c) streams.push_back(which[i] * L->channels + c);
  SHZ_TRY(shz_streams_reset(L->s, streams.data(), (uint32_t)streams.size()));
  for (uint32_t i = 0; i < n; ++i) {
    L->w_n[which[i]] = L->w0[which[i]] = L->last_nhash[which[i]] = 0;
    for (uint32_t c = 0; c < L->channels; ++c) L->p_n[(size_t)which[i] * L->channels + c] = 0;
  }
  return SHZ_OK;
}

extern "C" int32_t shz_listeners_state(shz_listeners* L, uint32_t l, uint64_t* window_hashes, uint64_t* w0) {
  SHZ_TRY(ls_check(L));
  if (l >= L->n) SHZ_FAIL(L->ctx, SHZ_E_INVALID, "listener %u out of range (%u listeners)", l, L->n);
  if (window_hashes) *window_hashes = L->peaks ? L->last_nhash[l] : L->w_n[l];
  if (w0) *w0 = L->w0[l];
  return SHZ_OK;
}

// tests / tools: the entries of listener l's window as they lie in the current slot, with the query offsets the last push
// wrote beside them.  Reads only.
extern "C" int32_t shz_listeners_window(shz_listeners* L, uint32_t l, uint32_t* key32, uint32_t* t1, uint32_t* q_off, uint64_t cap,
                                        uint64_t* n) {
  SHZ_TRY(ls_check(L));
  shz_ctx* ctx = L->ctx;
  if (l >= L->n) SHZ_FAIL(ctx, SHZ_E_INVALID, "listener %u out of range (%u listeners)", l, L->n);
  if (!n) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_window: n is NULL");
  if (L->peaks) SHZ_FAIL(ctx, SHZ_E_STATE, "shz_listeners_window: the object keeps peak windows (shz_listeners_peaks)");
  const uint64_t at = L->w_at[l], cnt = L->w_n[l];
  *n = cnt;
  if (cnt > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "output needs %llu entries, capacity %llu", (unsigned long long)cnt, (unsigned long long)cap);
  if (cnt == 0) return SHZ_OK;
  if (!key32 || !t1 || !q_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_window: NULL buffer");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const shz_buf &wk = L->wk[L->cur], &wt = L->wt[L->cur];
  if (!wk.p || !wt.p || !L->qo.p || (at + cnt) * 4 > std::min(std::min(wk.cap, wt.cap), L->qo.cap))
    SHZ_FAIL(ctx, SHZ_E_STATE, "listeners: window [%llu, %llu) lies outside its slot", (unsigned long long)at, (unsigned long long)(at + cnt));
  SHZ_HIP(ctx, shz_memcpy(ctx, key32, (const uint32_t*)wk.p + at, cnt * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, t1, (const uint32_t*)wt.p + at, cnt * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, q_off, (const uint32_t*)L->qo.p + at, cnt * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_listener_window(const uint64_t* settled, uint32_t channels, uint32_t window_frames, uint64_t* horizon,
                                       uint64_t* w0) {
  if (!settled || channels == 0) return SHZ_E_INVALID;
  uint64_t h = settled[0];
  for (uint32_t c = 1; c < channels; ++c) h = std::min(h, settled[c]);
  if (horizon) *horizon = h;
  if (w0) *w0 = h > window_frames ? h - window_frames : 0;
  return SHZ_OK;
}

// The streams' push of a listeners' push: hashes to the object's own device buffers (L->nk / L->nt).  Its SHZ_E_CAPACITY changes
// no stream and names the room, so the buffers grow and the push is made again.
static int32_t ls_streams_push(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end, uint32_t flags,
                               uint64_t* hash_off) {
  shz_ctx* ctx = L->ctx;
  uint64_t count = 0;
  void *d_nk, *d_nt;
  if (L->new_cap == 0) L->new_cap = (uint64_t)L->s->n * 256 + 4096;
  for (int attempt = 0;; ++attempt) {
    SHZ_TRY(st_reserve(ctx, L->nk, L->new_cap * 4 + 64, &d_nk));
    SHZ_TRY(st_reserve(ctx, L->nt, L->new_cap * 4 + 64, &d_nt));
    const int32_t rc = shz_streams_push(L->s, pcm, chunk_off, end, (flags & SHZ_PCM_DEVICE) | SHZ_OUT_DEVICE, (uint32_t*)d_nk,
                                        (uint32_t*)d_nt, hash_off, L->new_cap, &count);
    if (rc == SHZ_E_CAPACITY && attempt < 2 && count > L->new_cap) {
      L->new_cap = count + count / 4;
      continue;
    }
    return rc;
  }
}

// The window stage's mailbox: nj jobs for the host to fill | total (64 bytes) and the nj counts read back.
static inline uint64_t win_jobs_bytes(uint32_t nj) { return ((uint64_t)nj * sizeof(win_job) + 255) & ~255ull; }

static int32_t win_mailbox(shz_ctx* ctx, uint32_t nj, win_job** hj) {
  void* mailp;
  SHZ_TRY(shz_mailbox(ctx, win_jobs_bytes(nj) + 64 + (uint64_t)nj * 8, &mailp));
  *hj = (win_job*)mailp;
  return SHZ_OK;
}

// The window stage on the nj jobs in the mailbox: one upload, count, a scan over the jobs, the kept old-then-new entries
// compacted in order into the output slot (sized by the caller for `bound` entries) with t - w0 beside them, and one read-back
// of the counts; csr is their CSR from 0.  Commits nothing: the caller flips the slots once this has returned SHZ_OK.
template <class P>
static int32_t win_compact(shz_listeners* L, uint32_t nj, const win_job* hj, uint64_t bound, const char* what, const P* wp_in,
                           const uint32_t* wt_in, const P* np, const uint32_t* nt, P* wp_out, uint32_t* wt_out, uint32_t* rel,
                           hipEvent_t queued, std::vector<uint64_t>& csr) {
  shz_ctx* ctx = L->ctx;
  void *d_jobs, *d_ctl;
  const uint64_t jb = win_jobs_bytes(nj), rb = 64 + (uint64_t)nj * 8;
  SHZ_TRY(st_reserve(ctx, L->jobs, jb, &d_jobs));
  SHZ_TRY(st_reserve(ctx, L->ctl, 64 + (uint64_t)nj * 16, &d_ctl));
  unsigned long long* d_total = (unsigned long long*)d_ctl;
  uint64_t *d_cnt = (uint64_t*)((char*)d_ctl + 64), *d_offs = d_cnt + nj;
  SHZ_HIP(ctx, hipMemcpyAsync(d_jobs, hj, (uint64_t)nj * sizeof(win_job), hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(window_count_kernel, dim3(nj), dim3(LS_THREADS), 0, ctx->stream, (const win_job*)d_jobs, wt_in, nt, d_cnt);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u64(ctx, d_cnt, d_offs, nj, (uint64_t*)d_total));
  hipLaunchKernelGGL(window_write_kernel<P>, dim3(nj), dim3(LS_THREADS), 0, ctx->stream, (const win_job*)d_jobs, wp_in, wt_in, np, nt,
                     (const uint64_t*)d_offs, (const unsigned long long*)d_total, bound, wp_out, wt_out, rel);
  SHZ_HIP(ctx, hipGetLastError());
  char* hr = (char*)hj + jb;
  SHZ_HIP(ctx, hipMemcpyAsync(hr, d_ctl, rb, hipMemcpyDeviceToHost, ctx->stream));
  if (queued) SHZ_HIP(ctx, hipEventRecord(queued, ctx->stream));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const uint64_t total = *(const uint64_t*)hr;
  const uint64_t* hc = (const uint64_t*)(hr + 64);
  if (total > bound)
    SHZ_FAIL(ctx, SHZ_E_STATE, "listeners: %llu window %s exceed their bound %llu", (unsigned long long)total, what, (unsigned long long)bound);
  csr.assign((size_t)nj + 1, 0);
  for (uint32_t k = 0; k < nj; ++k) csr[k + 1] = csr[k] + hc[k];
  return SHZ_OK;
}

extern "C" int32_t shz_listeners_push(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                      uint32_t topn, uint32_t flags, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                      uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                                      uint32_t* out_w0) {
  SHZ_TRY(ls_check(L));
  shz_ctx* ctx = L->ctx;
  shz_streams* s = L->s;
  const uint32_t n = L->n, ch = L->channels;
  if (L->peaks) SHZ_FAIL(ctx, SHZ_E_STATE, "shz_listeners_push: the object keeps peak windows (shz_listeners_push_warps)");
  // what the match would refuse is refused here, before any stream advances
  if (flags & ~(SHZ_PCM_DEVICE | SHZ_MATCH_FULL_SORT)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_push: flags may hold SHZ_PCM_DEVICE and SHZ_MATCH_FULL_SORT");
  if (!out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_push: NULL buffer");
  SHZ_TRY(shz_match_ready(ctx, L->t, topn));
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  // 1) the streams' push, hashes to the object's own device buffers
  std::vector<uint64_t> hash_off((size_t)s->n + 1, 0);
  SHZ_TRY(ls_streams_push(L, pcm, chunk_off, end, flags, hash_off.data()));
  // 2) w0 of every listener from the horizons, where its entries are, and a bound of what the windows can hold
  win_job* hj;
  SHZ_TRY(win_mailbox(ctx, n, &hj));
  uint64_t bound = 0, bias = 0;
  std::vector<uint32_t> w0_new(n);
  for (uint32_t l = 0; l < n; ++l) {
    uint64_t h, w0, top = 0;
    SHZ_TRY(shz_listener_window(s->settled.data() + (size_t)l * ch, ch, L->window_frames, &h, &w0));
    for (uint32_t c = 0; c < ch; ++c) top = std::max(top, s->settled[(size_t)l * ch + c]);
    const uint64_t a = hash_off[(size_t)l * ch], b = hash_off[(size_t)(l + 1) * ch];
    hj[l] = win_job{L->w_at[l], a, L->w_n[l], (uint32_t)(b - a), (uint32_t)w0, 0u};
    w0_new[l] = (uint32_t)w0;
    bound += (uint64_t)L->w_n[l] + (b - a);
    if ((uint64_t)L->w_n[l] + (b - a) >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "listener %u: 2^31 hashes in its window", l);
    // every t1 of a channel is below that channel's horizon: the largest query offset of the push is below this
    if (top > w0) bias = std::max(bias, top - w0 - 1);
  }
  // 3) count, scan over the listeners, compact into the other slot; 4) one read-back: the counts are the match's query_off
  const uint32_t out = L->cur ^ 1u;
  void *d_wk, *d_wt, *d_qo;
  SHZ_TRY(st_reserve(ctx, L->wk[out], bound * 4 + 64, &d_wk));
  SHZ_TRY(st_reserve(ctx, L->wt[out], bound * 4 + 64, &d_wt));
  SHZ_TRY(st_reserve(ctx, L->qo, bound * 4 + 64, &d_qo));
  std::vector<uint64_t> query_off;
  SHZ_TRY(win_compact<uint32_t>(L, n, hj, bound, "entries", (const uint32_t*)L->wk[L->cur].p, (const uint32_t*)L->wt[L->cur].p,
                                (const uint32_t*)L->nk.p, (const uint32_t*)L->nt.p, (uint32_t*)d_wk, (uint32_t*)d_wt, (uint32_t*)d_qo,
                                nullptr, query_off));
  // the windows advance: the streams have
  L->cur = out;
  for (uint32_t l = 0; l < n; ++l) {
    L->w_at[l] = query_off[l];
    L->w_n[l] = (uint32_t)(query_off[l + 1] - query_off[l]);
    L->w0[l] = w0_new[l];
    if (out_w0) out_w0[l] = w0_new[l];
  }
  // 5) all listeners in one match, on the columns where they are (a listener without hashes: nres = 0)
  return shz_match_device(ctx, L->t, (const uint32_t*)d_wk, (const uint32_t*)d_qo, query_off.data(), n, topn,
                          flags & SHZ_MATCH_FULL_SORT, (int64_t)bias, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash,
                          out_npairs);
}

// ---- listeners at a ladder: peak windows -----------------------------------------------------------------------------
// A warp acts on peaks -- they move in integer coordinates, change order and pair anew (shz_speed.hip) -- so a window of
// hashes cannot be warped.  A peak-window object keeps, per STREAM, the settled peaks (f, absolute t) with t >= w0 of its
// listener, in the stream's order, in two packed slots as the hash windows are.  One push: the streams' push, which says where
// every stream's newly settled peaks lie (st_hand); one small upload; the same window_count_kernel, a scan over the streams,
// window_write_kernel -- kept old entries, then the new ones with their window clip's first frame added, compacted in order
// into the OTHER slot, the times t - w0 beside them -- one read-back of the counts, which are the warp's peak_off; then every
// (listener, warp) through sp_match_fold on the slot's f column and the rebased times.

extern "C" int32_t shz_listeners_timing(shz_listeners* L, int32_t enable, float* ms) {
  SHZ_TRY(ls_check(L));
  if (!L->peaks) SHZ_FAIL(L->ctx, SHZ_E_STATE, "shz_listeners_timing: the object keeps hash windows");
  if (ms) memcpy(ms, L->ms, sizeof(L->ms));
  L->timed = enable != 0;
  return SHZ_OK;
}

extern "C" int32_t shz_listeners_peaks(shz_listeners* L, uint32_t l, uint32_t channel, uint16_t* f, uint32_t* t, uint64_t cap,
                                       uint64_t* n) {
  SHZ_TRY(ls_check(L));
  shz_ctx* ctx = L->ctx;
  if (!L->peaks) SHZ_FAIL(ctx, SHZ_E_STATE, "shz_listeners_peaks: the object keeps hash windows (shz_listeners_window)");
  if (l >= L->n) SHZ_FAIL(ctx, SHZ_E_INVALID, "listener %u out of range (%u listeners)", l, L->n);
  if (channel >= L->channels) SHZ_FAIL(ctx, SHZ_E_INVALID, "channel %u out of range (%u channels)", channel, L->channels);
  if (!n) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_peaks: n is NULL");
  const size_t i = (size_t)l * L->channels + channel;
  const uint64_t at = L->p_at[i], cnt = L->p_n[i];
  *n = cnt;
  if (cnt > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "output needs %llu entries, capacity %llu", (unsigned long long)cnt, (unsigned long long)cap);
  if (cnt == 0) return SHZ_OK;
  if (!f || !t) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_peaks: NULL buffer");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  const shz_buf &pf = L->pf[L->cur], &pt = L->pt[L->cur];
  if (!pf.p || !pt.p || (at + cnt) * 2 > pf.cap || (at + cnt) * 4 > pt.cap)
    SHZ_FAIL(ctx, SHZ_E_STATE, "listeners: window [%llu, %llu) lies outside its slot", (unsigned long long)at, (unsigned long long)(at + cnt));
  SHZ_HIP(ctx, shz_memcpy(ctx, f, (const uint16_t*)pf.p + at, cnt * 2, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, t, (const uint32_t*)pt.p + at, cnt * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_listeners_push_warps(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                            uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps,
                                            uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                            uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                            uint32_t* out_profile, uint32_t* out_w0) {
  SHZ_TRY(ls_check(L));
  shz_ctx* ctx = L->ctx;
  shz_streams* s = L->s;
  const uint32_t n = L->n, ch = L->channels, ns = s->n, K = n_warps;
  if (!L->peaks) SHZ_FAIL(ctx, SHZ_E_STATE, "shz_listeners_push_warps: the object keeps hash windows (shz_listeners_push)");
  // everything that can be refused is refused here, before any stream advances
  if (flags & ~(SHZ_PCM_DEVICE | SHZ_MATCH_FULL_SORT)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_push_warps: flags may hold SHZ_PCM_DEVICE and SHZ_MATCH_FULL_SORT");
  SHZ_TRY(sp_check_ladder(ctx, "shz_listeners_push_warps", "n_warps", "tempo", tempo_q16, "pitch", pitch_q16, n_warps, s->fan));
  if (!out_best || !out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_listeners_push_warps: NULL buffer");
  SHZ_TRY(shz_match_ready(ctx, L->t, topn));
  if (!chunk_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "chunk_off must not be NULL");
  for (uint32_t i = 0; i < ns; ++i)
    if (chunk_off[i + 1] < chunk_off[i]) SHZ_FAIL(ctx, SHZ_E_INVALID, "chunk_off decreases at stream %u", i);
  if (chunk_off[ns] > chunk_off[0] && !pcm) SHZ_FAIL(ctx, SHZ_E_INVALID, "pcm is NULL");
  // the horizons after the push follow from the plan alone: w0 of every listener and the largest warped time
  std::vector<uint64_t> h_after(ns);
  for (uint32_t i = 0; i < ns; ++i) {
    const uint64_t len = chunk_off[i + 1] - chunk_off[i];
    const bool e = end && ((end[i >> 5] >> (i & 31)) & 1u);
    h_after[i] = s->settled[i];
    if (s->ended[i]) {
      if (len || e) SHZ_FAIL(ctx, SHZ_E_STATE, "stream %u has ended; reset it before pushing to it again", i);
      continue;
    }
    if (!len && !e) continue;
    if (shz_stream_plan(s->samples[i], s->samples[i] + len, s->settled[i], s->hop, e ? 1 : 0, nullptr, nullptr, nullptr, &h_after[i]) != SHZ_OK)
      SHZ_FAIL(ctx, SHZ_E_STATE, "stream %u: inconsistent state (samples %llu, settled %llu)", i, (unsigned long long)s->samples[i],
               (unsigned long long)s->settled[i]);
  }
  const uint32_t s_max = *std::max_element(tempo_q16, tempo_q16 + K);   // (time alone: the bias bound)
  std::vector<uint32_t> w0_new(n);
  uint64_t t_max = 0;
  for (uint32_t l = 0; l < n; ++l) {
    uint64_t h, w0, top = 0;
    SHZ_TRY(shz_listener_window(h_after.data() + (size_t)l * ch, ch, L->window_frames, &h, &w0));
    for (uint32_t c = 0; c < ch; ++c) top = std::max(top, h_after[(size_t)l * ch + c]);
    w0_new[l] = (uint32_t)w0;
    // every settled t of a channel is below that channel's horizon
    if (top > w0) t_max = std::max(t_max, ((top - w0 - 1) * s_max + 32768) >> 16);
  }
  if (t_max >= (1ull << 20))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_listeners_push_warps: a window at time factor %u / 65536 reaches t' = %llu; query offsets must be < 2^20",
             s_max, (unsigned long long)t_max);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = L->timed;
  if (timed) {
    for (hipEvent_t& e : L->ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(L->ev[0], ctx->stream));
  }
  // 1) the streams' push; its hashes go to buffers of the object and are not used (the streams advance as they always do)
  std::vector<uint64_t> hash_off((size_t)ns + 1, 0);
  SHZ_TRY(ls_streams_push(L, pcm, chunk_off, end, flags, hash_off.data()));
  for (uint32_t i = 0; i < ns; ++i)
    if (s->settled[i] != h_after[i])
      SHZ_FAIL(ctx, SHZ_E_STATE, "listeners: stream %u settled %llu frames, its plan said %llu", i, (unsigned long long)s->settled[i],
               (unsigned long long)h_after[i]);
  if (timed) SHZ_HIP(ctx, hipEventRecord(L->ev[1], ctx->stream));
  // 2) per stream: where its old and its newly settled peaks are; the slots hold at most all of them
  win_job* hj;
  SHZ_TRY(win_mailbox(ctx, ns, &hj));
  uint64_t bound = 0;
  for (uint32_t i = 0; i < ns; ++i) {
    const st_hand& hd = s->hand[i];
    hj[i] = win_job{L->p_at[i], hd.at, L->p_n[i], hd.n, w0_new[i / ch], hd.w0};
    bound += (uint64_t)L->p_n[i] + hd.n;
  }
  if (bound >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "listeners: 2^31 peaks in the windows");
  // 3) count, scan over the streams, compact into the other slot; 4) one read-back: the counts are the warp's peak_off
  const uint32_t out = L->cur ^ 1u;
  void *d_wf, *d_wt, *d_rel;
  SHZ_TRY(st_reserve(ctx, L->pf[out], bound * 2 + 64, &d_wf));
  SHZ_TRY(st_reserve(ctx, L->pt[out], bound * 4 + 64, &d_wt));
  SHZ_TRY(st_reserve(ctx, L->pr, bound * 4 + 64, &d_rel));
  std::vector<uint64_t> peak_off;
  SHZ_TRY(win_compact<uint16_t>(L, ns, hj, bound, "peaks", (const uint16_t*)L->pf[L->cur].p, (const uint32_t*)L->pt[L->cur].p,
                                (const uint16_t*)s->pf.p, (const uint32_t*)s->pt.p, (uint16_t*)d_wf, (uint32_t*)d_wt, (uint32_t*)d_rel,
                                timed ? L->ev[2] : nullptr, peak_off));
  // the windows advance: the streams have
  L->cur = out;
  for (uint32_t i = 0; i < ns; ++i) {
    L->p_at[i] = peak_off[i];
    L->p_n[i] = (uint32_t)(peak_off[i + 1] - peak_off[i]);
  }
  for (uint32_t l = 0; l < n; ++l) {
    L->w0[l] = w0_new[l];
    L->last_nhash[l] = 0;
    if (out_w0) out_w0[l] = w0_new[l];
  }
  // 5) every (listener, warp) is one query: warped, hashed and matched as shz_recognize_warps does it
  std::vector<uint32_t> clip0((size_t)n + 1), nhash(n, 0);
  for (uint32_t l = 0; l <= n; ++l) clip0[l] = l * ch;
  float ms_warp = 0.f, ms_match = 0.f;
  SHZ_TRY(sp_match_fold(ctx, L->t, (const uint16_t*)d_wf, (const uint32_t*)d_rel, peak_off.data(), ns, clip0.data(), n, s->fan, topn,
                        tempo_q16, pitch_q16, K, flags & SHZ_MATCH_FULL_SORT, t_max, out_best, out_sid, out_delta, out_aligned,
                        out_dedup, out_nres, nhash.data(), out_profile, timed, &ms_warp, &ms_match));
  for (uint32_t l = 0; l < n; ++l) {
    L->last_nhash[l] = nhash[l];
    if (out_nhash) out_nhash[l] = nhash[l];
  }
  if (timed) {
    SHZ_HIP(ctx, hipEventElapsedTime(&L->ms[0], L->ev[0], L->ev[1]));
    SHZ_HIP(ctx, hipEventElapsedTime(&L->ms[1], L->ev[1], L->ev[2]));
    L->ms[2] = ms_warp;
    L->ms[3] = ms_match;
  }
  return SHZ_OK;
}

// the speed ladder: one table for time and frequency (its own names in what is refused about it)
extern "C" int32_t shz_listeners_push_speeds(shz_listeners* L, const int16_t* pcm, const uint64_t* chunk_off, const uint32_t* end,
                                             uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds, uint32_t flags,
                                             uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                             uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile,
                                             uint32_t* out_w0) {
  SHZ_TRY(ls_check(L));
  if (!L->peaks) SHZ_FAIL(L->ctx, SHZ_E_STATE, "shz_listeners_push_speeds: the object keeps hash windows (shz_listeners_push)");
  SHZ_TRY(sp_check_ladder(L->ctx, "shz_listeners_push_speeds", "n_speeds", "speed", speed_q16, "speed", speed_q16, n_speeds, L->s->fan));
  return shz_listeners_push_warps(L, pcm, chunk_off, end, topn, speed_q16, speed_q16, n_speeds, flags, out_best, out_sid, out_delta,
                                  out_aligned, out_dedup, out_nres, out_nhash, out_profile, out_w0);
}
