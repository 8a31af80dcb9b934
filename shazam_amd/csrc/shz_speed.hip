// Speed-tolerant recognition: audio played slightly fast or slow -- a radio station pitching a song up, a
// turntable that drifts -- shifts every constellation peak: a query that plays s times as fast as the table's copy has its
// peaks at frequency f s and time t / s.  The hash is an exact (f1, f2, dt) triple (recognizer.py:100-114), so 1 % already
// loses the match.  The spectrogram is left alone: the integer coordinates of the query's peaks are mapped back to the
// table's domain for every factor of a ladder, and each variant is paired, hashed and matched as a query of its own.
//
// The warp, in 64-bit integers (s16 = round(s 65536), 32768 .. 131072; numpy twin: tests/speed_twin.py):
//     t' = (t s16 + 32768) >> 16        f' = (2 65536 f + s16) / (2 s16)        peaks with f' > 2048 leave
// and the peaks of one (clip, speed) are ordered by (t', f', original index) -- what generate_hashes sees after its stable
// time sort.  Both maps are monotone and the input is (t asc, f asc): for s >= 1 the order is the input's; for s < 1 at most
// two neighbouring frames fall into one t', and a peak's place changes by a count over the neighbour frame.
//
// Two factors (numpy twin: tests/warp_twin.py): a time-stretch with the pitch kept, or a pitch shift with the
// tempo kept, moves time and frequency by factors of their own.  A warp is a pair (t16, f16): t' is formed with t16, f' with
// f16, and a speed is the pair (s16, s16).  The order argument per factor: f' is monotone in f at any f16, so inside one frame
// the order (f', index) is the input's; t' is strictly monotone for t16 >= 65536, so there the whole order is the input's
// whatever f16 is (f16 < 65536 spreads the bins and some leave, f16 > 65536 folds neighbouring bins into one f', and a tie
// keeps the index order).  For t16 < 65536 frames t and t + 2 are still 2 t16 >= 65536 apart before the shift, so at most two
// neighbouring frames share a t'; a peak then moves by the kept peaks of the OTHER frame that its f' passes, compared on f'
// with "equal f': the earlier index first" -- ties across the two frames are what f16 > 65536 adds (bins 2k - 1 and 2k at
// f16 = 131072), peaks of the neighbour frame that leave are what f16 < 65536 adds.  So the merge is switched by t16 alone.
//
// Work is laid out over (query, speed, clip, peak) items, so that a single short query with a ladder of a hundred factors
// still fills waves, and so that the compacted peaks -- and the hashes behind them -- come out in the order the match
// wants: for query q, for speed v, for every clip (channel) c of q.  (q, v) is then one contiguous query of the match.
//     sp_flag  : item -> keeps its peak?            scan -> place among the kept peaks, in item order
//     sp_place : item -> (f', t') at its place (the count over the neighbour frame for s < 1)
//     sp_seg   : first kept peak of every (q, v, c)
//     sp_count : partners of every kept peak         scan -> offsets;  sp_hoff: the exact CSR, read back once
//     sp_write : (key32, t1) as pair_write_kernel forms them
// The JOB form runs the same kernels over a list of jobs (clip, a range of its peaks, a pair of its own) in place
// of the product: the segments of a warped scan each play at their own pair, and only their frames need warping.
#include <algorithm>

#include "shz_internal.h"

#define SP_THREADS 256
#define SP_SMALL_SLICE 2u       // queries of a match slice under SHZ_DEBUG_SPEED_SMALL_SLICES

struct sp_item {
  uint32_t c, t16, f16;       // its clip, and the time and the frequency factor of its warp
  uint64_t g, c_lo, c_hi;     // the peak, and the peaks of its clip
  uint64_t seg0, seg_n;       // first item of its (query, speed, clip), items of it
};

// item w -> its query (the last q with qbase[q] <= w), speed, clip and peak.  Items of a query: speed-major, then its
// clips' peaks one behind the other -- a wave stays at one speed over consecutive peaks
__device__ __forceinline__ bool sp_decode(const sp_view& V, uint64_t w, sp_item* it) {
  uint32_t lo = 0, hi = V.nq;
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (V.qbase[mid] <= w) lo = mid; else hi = mid;
  }
  if (V.jobs) {   // (uniform: a kernel argument) the job form: nq jobs, qbase their first items.  Empty jobs share a base with
    // the job behind them, and the last of such a run is the one that holds w, because w exists
    const sp_job J = V.jobs[lo];
    it->c = lo;
    it->t16 = J.t16;
    it->f16 = J.f16;
    it->g = J.c_lo + (w - V.qbase[lo]);
    it->c_lo = J.c_lo;
    it->c_hi = J.c_hi;
    it->seg0 = V.qbase[lo];
    it->seg_n = J.c_hi - J.c_lo;
    return it->g < J.c_hi;
  }
  const uint32_t c0 = V.clip0[lo], c1 = V.clip0[lo + 1];
  const uint64_t p0 = V.poff[c0], nqp = V.poff[c1] - p0;
  if (nqp == 0) return false;
  const uint64_t rem = w - V.qbase[lo], v = rem / nqp, g = p0 + (rem - v * nqp);
  if (v >= V.K) return false;
  uint32_t c = c0;
  while (c + 1 < c1 && V.poff[c + 1] <= g) ++c;   // (the channels of one query: one or two)
  it->c = c;
  it->t16 = V.tempo[v];
  it->f16 = V.pitch[v];
  it->g = g;
  it->c_lo = V.poff[c];
  it->c_hi = V.poff[c + 1];
  it->seg0 = V.qbase[lo] + v * nqp + (it->c_lo - p0);
  it->seg_n = it->c_hi - it->c_lo;
  return true;
}

__global__ __launch_bounds__(SP_THREADS) void sp_flag_kernel(sp_view V, uint32_t* __restrict__ flag) {
  const uint64_t w = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (w >= V.n_items) return;
  sp_item it;
  flag[w] = sp_decode(V, w, &it) && sp_warp_f(V.pf[it.g], it.f16) <= SP_F_MAX ? 1u : 0u;
}

// pos: exclusive scan of the flags; *d_kept: their sum.  The kept peaks of (q, v, c) are [pos[seg0], pos[seg0 + seg_n]).
__global__ __launch_bounds__(SP_THREADS) void sp_place_kernel(sp_view V, const uint32_t* __restrict__ pos,
                                                               const unsigned long long* __restrict__ d_kept,
                                                               uint16_t* __restrict__ wf, uint32_t* __restrict__ wt) {
  const uint64_t w = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (w >= V.n_items) return;
  sp_item it;
  if (!sp_decode(V, w, &it)) return;
  const uint32_t t16 = it.t16, f16 = it.f16, fi = sp_warp_f(V.pf[it.g], f16);
  if (fi > SP_F_MAX) return;
  const uint32_t t = V.pt[it.g], ti = sp_warp_t(t, t16);
  const uint32_t base = pos[it.seg0];
  const uint64_t seg1 = it.seg0 + it.seg_n;
  const uint32_t end = seg1 < V.n_items ? pos[seg1] : (uint32_t)*d_kept;
  uint32_t rank = pos[w] - base;
  if (t16 < SP_S_ONE) {   // (the time factor alone decides whether frames merge; the comparisons below are on f' at any f16)
    // the frame in front of this peak's, if it falls into the same t': its kept peaks with a greater f' go behind this one
    uint64_t j = it.g;
    while (j > it.c_lo && V.pt[j - 1] == t) --j;
    if (j > it.c_lo && sp_warp_t(V.pt[j - 1], t16) == ti) {
      const uint32_t tn = V.pt[j - 1];
      for (; j > it.c_lo && V.pt[j - 1] == tn; --j) {
        const uint32_t fj = sp_warp_f(V.pf[j - 1], f16);
        if (fj <= SP_F_MAX && fj > fi) --rank;
      }
    }
    // the frame behind it, likewise: its kept peaks with a smaller f' go in front (equal f': the earlier index first)
    j = it.g + 1;
    while (j < it.c_hi && V.pt[j] == t) ++j;
    if (j < it.c_hi && sp_warp_t(V.pt[j], t16) == ti) {
      const uint32_t tn = V.pt[j];
      for (; j < it.c_hi && V.pt[j] == tn; ++j)
        if (sp_warp_f(V.pf[j], f16) < fi) ++rank;
    }
  }
  if (rank >= end - base) return;   // (peaks that are not in (t, f) order: nothing is written outside the segment)
  wf[base + rank] = (uint16_t)fi;
  wt[base + rank] = ti;
}

// segment e = (q, v, c) in output order, e in [0, n_seg]: segstart[e] = its first kept peak (segstart[n_seg] = all of them)
__global__ __launch_bounds__(SP_THREADS) void sp_seg_kernel(sp_view V, uint64_t n_seg, const uint32_t* __restrict__ pos,
                                                             const unsigned long long* __restrict__ d_kept,
                                                             uint32_t* __restrict__ segstart) {
  const uint64_t e = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (e > n_seg) return;
  uint64_t item0 = V.n_items;
  if (e < n_seg && V.jobs) {   // the job form: segment e is job e (an empty one starts where the next begins)
    item0 = V.qbase[e];
  } else if (e < n_seg) {
    const uint32_t cb = V.clip0[0];
    uint32_t lo = 0, hi = V.nq;   // the last query whose first segment is <= e
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((uint64_t)(V.clip0[mid] - cb) * V.K <= e) lo = mid; else hi = mid;
    }
    const uint32_t c0 = V.clip0[lo], nch = V.clip0[lo + 1] - c0;
    if (nch) {
      const uint64_t rem = e - (uint64_t)(c0 - cb) * V.K, v = rem / nch, c = c0 + (rem - v * nch);
      const uint64_t p0 = V.poff[c0], nqp = V.poff[c0 + nch] - p0;
      if (v < V.K) item0 = V.qbase[lo] + v * nqp + (V.poff[c] - p0);
    }
  }
  segstart[e] = item0 < V.n_items ? pos[item0] : (uint32_t)*d_kept;
}

// the segment of kept peak p: the last e with segstart[e] <= p (empty segments share a start)
__device__ __forceinline__ uint32_t sp_seg_end(const uint32_t* __restrict__ segstart, uint64_t n_seg, uint32_t p) {
  uint64_t lo = 0, hi = n_seg;
  while (lo + 1 < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (segstart[mid] <= p) lo = mid; else hi = mid;
  }
  return segstart[lo + 1];
}

// partners of every kept peak: the next fan - 1 of its segment with dt' <= 200 (pair_count_kernel on the warped list)
__global__ __launch_bounds__(SP_THREADS) void sp_count_kernel(uint64_t n_items, const unsigned long long* __restrict__ d_kept,
                                                               const uint32_t* __restrict__ segstart, uint64_t n_seg,
                                                               const uint32_t* __restrict__ wt, uint32_t fan,
                                                               uint32_t* __restrict__ cnt) {
  const uint64_t p = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= n_items) return;
  uint32_t c = 0;
  if (p < *d_kept) {
    const uint32_t end = sp_seg_end(segstart, n_seg, (uint32_t)p), t1 = wt[p];
    for (uint32_t jn = 1; jn < fan && p + jn < end; ++jn) {
      const uint32_t tj = wt[p + jn];
      if (tj >= t1 && tj - t1 <= SHZ_MAX_DT) ++c;
    }
  }
  cnt[p] = c;
}

// hash_off[e] = hashes in front of segment e; hash_off[n_seg] = all of them
__global__ __launch_bounds__(SP_THREADS) void sp_hoff_kernel(uint64_t n_seg, const uint32_t* __restrict__ segstart,
                                                              const unsigned long long* __restrict__ d_tot /* kept, hashes */,
                                                              const uint32_t* __restrict__ hoff,
                                                              unsigned long long* __restrict__ hash_off) {
  const uint64_t e = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (e > n_seg) return;
  const uint32_t s = segstart[e];
  hash_off[e] = s < d_tot[0] ? hoff[s] : d_tot[1];
}

__global__ __launch_bounds__(SP_THREADS) void sp_write_kernel(uint64_t n_items, const unsigned long long* __restrict__ d_kept,
                                                               const uint32_t* __restrict__ segstart, uint64_t n_seg,
                                                               const uint16_t* __restrict__ wf, const uint32_t* __restrict__ wt,
                                                               uint32_t fan, const uint32_t* __restrict__ hoff,
                                                               uint32_t* __restrict__ key32, uint32_t* __restrict__ t1out,
                                                               uint64_t cap) {
  const uint64_t p = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (p >= n_items || p >= *d_kept) return;
  const uint32_t end = sp_seg_end(segstart, n_seg, (uint32_t)p), t1 = wt[p], f1 = wf[p];
  uint64_t o = hoff[p];
  for (uint32_t jn = 1; jn < fan && p + jn < end; ++jn) {
    const uint32_t tj = wt[p + jn];
    if (tj >= t1 && tj - t1 <= SHZ_MAX_DT) {
      if (o < cap) {
        key32[o] = (f1 << 20) | ((uint32_t)wf[p + jn] << 8) | (tj - t1);
        t1out[o] = t1;
      }
      ++o;
    }
  }
}

// ---- one warp pass over the queries [q0, q0 + nq): count (exact CSR on the host), then write (sp_pass: shz_internal.h)
static unsigned sp_blocks(uint64_t n) { return (unsigned)((n + SP_THREADS - 1) / SP_THREADS); }

// items of the queries [q0, q0 + nq) at K speeds, and the entries they can yield at most
uint64_t sp_items(const uint64_t* peak_off, const uint32_t* clip0, uint32_t q0, uint32_t nq, uint32_t K) {
  return (peak_off[clip0[q0 + nq]] - peak_off[clip0[q0]]) * K;
}

// what a pass can hold: the places and the hash offsets of its items are 32 bits wide
static int32_t sp_fits(shz_ctx* ctx, uint64_t n_items, uint32_t fan) {
  if (n_items * std::max<uint32_t>(fan - 1, 1) >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "speed warp: %llu (peak, speed) pairs at fan_value %u in one pass (32-bit offsets)",
             (unsigned long long)n_items, fan);
  return SHZ_OK;
}

// The stages of a pass whose view is complete (P->V with its tables on the device, n_items > 0; P->n_seg): flag -> scan ->
// place -> segment starts -> count -> scan -> the exact CSR, read back once into hash_off.  Both forms run it: the product
// form (sp_count) and the job form (sp_count_jobs) differ in what an item decodes to (sp_decode, sp_seg_kernel) and in
// nothing else.  The stream is idle on return
static int32_t sp_run(shz_ctx* ctx, sp_pass* P, uint64_t* hash_off) {
  const uint64_t n_items = P->V.n_items, n_seg = P->n_seg;
  const uint32_t fan = P->V.fan;
  void *a, *b, *wf, *wt, *sg;
  const uint64_t seg_bytes = ((n_seg + 1) * 4 + 255) & ~255ull;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_A, n_items * 4, &a));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_B, n_items * 4, &b));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_WF, n_items * 2, &wf));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_WT, n_items * 4, &wt));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_SEG, seg_bytes + (n_seg + 1) * 8 + 64, &sg));
  P->a = (uint32_t*)a;
  P->b = (uint32_t*)b;
  P->wf = (uint16_t*)wf;
  P->wt = (uint32_t*)wt;
  P->segstart = (uint32_t*)sg;
  P->d_hoff = (unsigned long long*)((char*)sg + seg_bytes);
  P->d_tot = P->d_hoff + n_seg + 1;
  hipStream_t st = ctx->stream;
  hipLaunchKernelGGL(sp_flag_kernel, dim3(sp_blocks(n_items)), dim3(SP_THREADS), 0, st, P->V, P->a);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, P->a, P->b, n_items, (uint64_t*)P->d_tot));
  hipLaunchKernelGGL(sp_place_kernel, dim3(sp_blocks(n_items)), dim3(SP_THREADS), 0, st, P->V, (const uint32_t*)P->b,
                     (const unsigned long long*)P->d_tot, P->wf, P->wt);
  hipLaunchKernelGGL(sp_seg_kernel, dim3(sp_blocks(n_seg + 1)), dim3(SP_THREADS), 0, st, P->V, n_seg, (const uint32_t*)P->b,
                     (const unsigned long long*)P->d_tot, P->segstart);
  hipLaunchKernelGGL(sp_count_kernel, dim3(sp_blocks(n_items)), dim3(SP_THREADS), 0, st, n_items,
                     (const unsigned long long*)P->d_tot, (const uint32_t*)P->segstart, n_seg, (const uint32_t*)P->wt, fan, P->a);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, P->a, P->b, n_items, (uint64_t*)P->d_tot + 1));
  hipLaunchKernelGGL(sp_hoff_kernel, dim3(sp_blocks(n_seg + 1)), dim3(SP_THREADS), 0, st, n_seg, (const uint32_t*)P->segstart,
                     (const unsigned long long*)P->d_tot, (const uint32_t*)P->b, P->d_hoff);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, shz_memcpy(ctx, hash_off, P->d_hoff, (n_seg + 1) * 8, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  return SHZ_OK;
}

// hash_off: n_seg + 1 entries (host), relative to the pass.  d_poff / d_tempo / d_pitch: the call's tables on the device.
int32_t sp_count(shz_ctx* ctx, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* d_poff, const uint64_t* peak_off,
                        const uint32_t* clip0, uint32_t q0, uint32_t nq, const uint32_t* d_tempo, const uint32_t* d_pitch, uint32_t K,
                        uint32_t fan, sp_pass* P, uint64_t* hash_off) {
  const uint64_t n_items = sp_items(peak_off, clip0, q0, nq, K);
  const uint64_t n_seg = (uint64_t)(clip0[q0 + nq] - clip0[q0]) * K;
  P->n_seg = n_seg;
  for (uint64_t e = 0; e <= n_seg; ++e) hash_off[e] = 0;
  P->V = sp_view{d_pf, d_pt, d_poff, nullptr, nullptr, d_tempo, d_pitch, nq, K, fan, n_items};
  if (n_items == 0) return SHZ_OK;
  SHZ_TRY(sp_fits(ctx, n_items, fan));
  // the pass's own tables: qbase | clip0
  const uint64_t qb_bytes = ((uint64_t)nq + 1) * 8, tab_bytes = qb_bytes + ((uint64_t)nq + 1) * 4;
  void *hm, *d_q;
  SHZ_TRY(shz_mailbox(ctx, tab_bytes, &hm));
  uint64_t* hq = (uint64_t*)hm;
  uint32_t* hc = (uint32_t*)((char*)hm + qb_bytes);
  for (uint32_t q = 0; q <= nq; ++q) {
    hq[q] = (peak_off[clip0[q0 + q]] - peak_off[clip0[q0]]) * K;
    hc[q] = clip0[q0 + q];
  }
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_Q, tab_bytes, &d_q));
  SHZ_HIP(ctx, hipMemcpyAsync(d_q, hm, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
  P->V.qbase = (const uint64_t*)d_q;
  P->V.clip0 = (const uint32_t*)((char*)d_q + qb_bytes);
  return sp_run(ctx, P, hash_off);
}

// ---- the job form: the warp stage on a list of jobs (clip, a range of its peaks, its own pair) -------------
// first peak of [a, b) whose warped time is >= v (peak times do not decrease inside a clip, and neither does W)
__device__ __forceinline__ uint64_t sp_lower_bound_w(const uint32_t* __restrict__ pt, uint64_t a, uint64_t b, uint32_t t16, uint64_t v) {
  while (a < b) {
    const uint64_t mid = a + ((b - a) >> 1);
    if ((((uint64_t)pt[mid] * t16 + 32768u) >> 16) < v) a = mid + 1; else b = mid;
  }
  return a;
}

// job j comes in with all peaks of its clip and leaves with those whose warped time lies in [w_lo, w_end]; cnt[j]: how many
__global__ __launch_bounds__(SP_THREADS) void sp_job_range_kernel(const uint32_t* __restrict__ pt, sp_job* __restrict__ jobs,
                                                                   uint32_t n_jobs, uint64_t* __restrict__ cnt) {
  const uint64_t j = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (j >= n_jobs) return;
  const sp_job J = jobs[j];
  const uint64_t a = sp_lower_bound_w(pt, J.c_lo, J.c_hi, J.t16, J.w_lo);
  const uint64_t b = sp_lower_bound_w(pt, a, J.c_hi, J.t16, J.w_end + 1);
  jobs[j].c_lo = a;
  jobs[j].c_hi = b;
  cnt[j] = b - a;
}

// The warp stage on jobs: every item takes its factors, its peak range and its segment from its job (sp_decode), segment e
// of the CSR is job e.  jobs (host, n_jobs >= 1): c_lo / c_hi = the peaks of the job's clip in d_pt.  Two warped-time binary
// searches per job narrow them on the device, shz_scan_u64 gives the jobs' first items and one read-back their number
// (*n_items); then the stages of every pass (sp_run).  The job table lies in SHZ_WS_SP_Q, where the product form keeps its
// own: descriptors | items of every job | their scan.  hash_off: n_jobs + 1 entries (host).  No items: nothing is warped
// and P's pointers stay unset, as in sp_count
int32_t sp_count_jobs(shz_ctx* ctx, const uint16_t* d_pf, const uint32_t* d_pt, const sp_job* jobs, uint32_t n_jobs, uint32_t fan,
                      sp_pass* P, uint64_t* hash_off, uint64_t* n_items) {
  const uint64_t job_bytes = (uint64_t)n_jobs * sizeof(sp_job);
  void* d_q;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_Q, job_bytes + (2 * (uint64_t)n_jobs + 1) * 8, &d_q));
  sp_job* d_jobs = (sp_job*)d_q;
  uint64_t *d_cnt = (uint64_t*)((char*)d_q + job_bytes), *d_base = d_cnt + n_jobs;   // d_base[n_jobs] = the items of all jobs
  SHZ_HIP(ctx, shz_memcpy(ctx, d_jobs, jobs, job_bytes, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(sp_job_range_kernel, dim3(sp_blocks(n_jobs)), dim3(SP_THREADS), 0, ctx->stream, d_pt, d_jobs, n_jobs, d_cnt);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u64(ctx, d_cnt, d_base, n_jobs, d_base + n_jobs));
  SHZ_HIP(ctx, shz_memcpy(ctx, n_items, d_base + n_jobs, 8, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  P->n_seg = n_jobs;
  for (uint64_t e = 0; e <= n_jobs; ++e) hash_off[e] = 0;
  P->V = sp_view{d_pf, d_pt, nullptr, d_base, nullptr, nullptr, nullptr, n_jobs, 1, fan, *n_items, d_jobs};
  if (*n_items == 0) return SHZ_OK;
  SHZ_TRY(sp_fits(ctx, *n_items, fan));
  return sp_run(ctx, P, hash_off);
}

int32_t sp_write(shz_ctx* ctx, const sp_pass& P, uint32_t* d_key, uint32_t* d_t1, uint64_t cap) {
  if (P.V.n_items == 0) return SHZ_OK;
  hipLaunchKernelGGL(sp_write_kernel, dim3(sp_blocks(P.V.n_items)), dim3(SP_THREADS), 0, ctx->stream, P.V.n_items,
                     (const unsigned long long*)P.d_tot, (const uint32_t*)P.segstart, P.n_seg, (const uint16_t*)P.wf,
                     (const uint32_t*)P.wt, P.V.fan, (const uint32_t*)P.b, d_key, d_t1, cap);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// what every entry point with a ladder refuses about it, before anything is launched (names: shz_internal.h)
int32_t sp_check_ladder(shz_ctx* ctx, const char* who, const char* n_name, const char* t_name, const uint32_t* tempo_q16,
                        const char* f_name, const uint32_t* pitch_q16, uint32_t n, uint32_t fan_value) {
  if (n == 0 || n > SP_MAX_SPEEDS) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s must be in [1, %u], got %u", who, n_name, SP_MAX_SPEEDS, n);
  if (!tempo_q16) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s_q16 is NULL", who, t_name);
  if (!pitch_q16) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s_q16 is NULL", who, f_name);
  const uint32_t* tab[2] = {tempo_q16, pitch_q16};
  const char* name[2] = {t_name, f_name};
  for (int a = 0; a < (pitch_q16 == tempo_q16 ? 1 : 2); ++a)
    for (uint32_t v = 0; v < n; ++v)
      if (tab[a][v] < SP_S_MIN || tab[a][v] > SP_S_MAX)
        SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s %u is %u; factors are Q16 in [%u, %u] (0.5x .. 2x)", who, name[a], v, tab[a][v], SP_S_MIN,
                 SP_S_MAX);
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  return SHZ_OK;
}

// peak_off | tempo | pitch on the device (one block of the call)
int32_t sp_upload_tables(shz_ctx* ctx, const uint64_t* peak_off, uint32_t n_clips, const uint32_t* tempo_q16,
                         const uint32_t* pitch_q16, uint32_t K, const uint64_t** d_poff, const uint32_t** d_tempo,
                         const uint32_t** d_pitch) {
  const bool one = pitch_q16 == tempo_q16;
  const uint64_t po_bytes = ((uint64_t)n_clips + 1) * 8, tab_bytes = (uint64_t)K * 4, bytes = po_bytes + (one ? 1 : 2) * tab_bytes;
  std::vector<char> h(bytes);
  uint64_t* hp = (uint64_t*)h.data();
  for (uint32_t c = 0; c <= n_clips; ++c) hp[c] = peak_off[c] - peak_off[0];
  memcpy(h.data() + po_bytes, tempo_q16, tab_bytes);
  if (!one) memcpy(h.data() + po_bytes + tab_bytes, pitch_q16, tab_bytes);
  void* d;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_TAB, bytes, &d));
  SHZ_HIP(ctx, shz_memcpy(ctx, d, h.data(), bytes, hipMemcpyHostToDevice));
  *d_poff = (const uint64_t*)d;
  *d_tempo = (const uint32_t*)((char*)d + po_bytes);
  *d_pitch = one ? *d_tempo : (const uint32_t*)((char*)d + po_bytes + tab_bytes);
  return SHZ_OK;
}

extern "C" int32_t shz_warp_pair_hash_tf(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                                         uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries,
                                         const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t fan_value,
                                         uint32_t flags, uint32_t* key32, uint32_t* t1, uint64_t* hash_off, uint64_t cap,
                                         uint64_t* count) {
  if (!ctx) return SHZ_E_INVALID;
  if (count) *count = 0;
  // everything that can be refused is refused before the first launch
  if (flags & ~(SHZ_IN_DEVICE | SHZ_OUT_DEVICE)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: flags may hold SHZ_IN_DEVICE and SHZ_OUT_DEVICE");
  SHZ_TRY(sp_check_ladder(ctx, "shz_warp_pair_hash_tf", "n_warps", "tempo", tempo_q16, "pitch", pitch_q16, n_warps, fan_value));
  if (!peak_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: peak_off is NULL");
  for (uint32_t c = 0; c < n_clips; ++c)
    if (peak_off[c + 1] < peak_off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "peak_off decreases at clip %u", c);
  std::vector<uint32_t> own;   // no queries given: every clip is a query of its own
  if (!query_clip0) {
    own.resize((size_t)n_clips + 1);
    for (uint32_t c = 0; c <= n_clips; ++c) own[c] = c;
    query_clip0 = own.data();
    n_queries = n_clips;
  }
  SHZ_TRY(shz_check_clip0(ctx, "query_clip0", "query", query_clip0, n_queries, n_clips));
  const uint64_t n = peak_off[n_clips] - peak_off[0];
  if (n && (!peak_f || !peak_t)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: NULL buffer");
  if (cap && (!key32 || !t1)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: NULL buffer");
  const bool in_dev = (flags & SHZ_IN_DEVICE) != 0, out_dev = (flags & SHZ_OUT_DEVICE) != 0;
  if (!in_dev)   // (device lists are the caller's promise, as for shz_pair_hash: time does not decrease inside a clip, t < 2^31)
    for (uint32_t c = 0; c < n_clips; ++c)
      for (uint64_t i = peak_off[c]; i < peak_off[c + 1]; ++i) {
        if (peak_t[i] >= (1u << 31)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: peak %llu has t = %u; t must be < 2^31", (unsigned long long)i, peak_t[i]);
        if (i > peak_off[c] && peak_t[i] < peak_t[i - 1])
          SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_pair_hash_tf: peaks must be in (time asc, freq asc) order; t decreases at peak %llu", (unsigned long long)i);
      }
  const uint64_t n_seg = (uint64_t)n_clips * n_warps;
  if (hash_off) memset(hash_off, 0, (n_seg + 1) * 8);
  if (n_clips == 0 || n == 0) return SHZ_OK;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const uint16_t* d_pf = peak_f + peak_off[0];
  const uint32_t* d_pt = peak_t + peak_off[0];
  if (!in_dev) {
    void *a, *b;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_PF, n * 2 + 64, &a));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_PT, n * 4 + 64, &b));
    SHZ_HIP(ctx, shz_memcpy(ctx, a, d_pf, n * 2, hipMemcpyHostToDevice));
    SHZ_HIP(ctx, shz_memcpy(ctx, b, d_pt, n * 4, hipMemcpyHostToDevice));
    d_pf = (const uint16_t*)a;
    d_pt = (const uint32_t*)b;
  }
  const uint64_t* d_poff;
  const uint32_t *d_tempo, *d_pitch;
  SHZ_TRY(sp_upload_tables(ctx, peak_off, n_clips, tempo_q16, pitch_q16, n_warps, &d_poff, &d_tempo, &d_pitch));
  std::vector<uint64_t> rel((size_t)n_clips + 1), ho((size_t)n_seg + 1, 0);
  for (uint32_t c = 0; c <= n_clips; ++c) rel[c] = peak_off[c] - peak_off[0];
  sp_pass P;
  SHZ_TRY(sp_count(ctx, d_pf, d_pt, d_poff, rel.data(), query_clip0, 0, n_queries, d_tempo, d_pitch, n_warps, fan_value, &P, ho.data()));
  const uint64_t total = ho[n_seg];
  if (hash_off) memcpy(hash_off, ho.data(), (n_seg + 1) * 8);
  if (count) *count = total;
  if (total > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "need %llu hashes", (unsigned long long)total);
  if (total == 0) return SHZ_OK;
  if (out_dev) {
    SHZ_TRY(sp_write(ctx, P, key32, t1, cap));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SHZ_OK;
  }
  void *k, *o;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_KEY, total * 4 + 64, &k));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_T1, total * 4 + 64, &o));
  SHZ_TRY(sp_write(ctx, P, (uint32_t*)k, (uint32_t*)o, total));
  SHZ_HIP(ctx, shz_memcpy(ctx, key32, k, total * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, t1, o, total * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

// the speed ladder: one table for time and frequency (its own names in what is refused about it)
extern "C" int32_t shz_warp_pair_hash(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                                      uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries, const uint32_t* speed_q16,
                                      uint32_t n_speeds, uint32_t fan_value, uint32_t flags, uint32_t* key32, uint32_t* t1,
                                      uint64_t* hash_off, uint64_t cap, uint64_t* count) {
  if (!ctx) return SHZ_E_INVALID;
  if (count) *count = 0;
  SHZ_TRY(sp_check_ladder(ctx, "shz_warp_pair_hash", "n_speeds", "speed", speed_q16, "speed", speed_q16, n_speeds, fan_value));
  return shz_warp_pair_hash_tf(ctx, peak_f, peak_t, peak_off, n_clips, query_clip0, n_queries, speed_q16, speed_q16, n_speeds,
                               fan_value, flags, key32, t1, hash_off, cap, count);
}

// index of the greatest top-1 aligned count; ties to the smaller |t16 - 65536| + |f16 - 65536| (on a speed ladder: the factor
// nearest 65536), then to the lower index
uint32_t sp_best(const uint32_t* top1, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t K) {
  auto off = [](uint32_t s) { return s > SP_S_ONE ? s - SP_S_ONE : SP_S_ONE - s; };
  auto dist = [&](uint32_t v) { return off(tempo_q16[v]) + off(pitch_q16[v]); };
  uint32_t best = 0;
  for (uint32_t v = 1; v < K; ++v)
    if (top1[v] > top1[best] || (top1[v] == top1[best] && dist(v) < dist(best))) best = v;
  return best;
}

// shz_peaks of the clips into the slots SHZ_WS_SP_PF / SHZ_WS_SP_PT, sized from the frame counts and repeated with the room
// the pass asked for: *d_pf / *d_pt are the lists, peak_off[n_clips + 1] (host) their CSR.  frames: of all clips together.
// flags: SHZ_PCM_DEVICE.  No clips: nothing runs
int32_t sp_peaks_owned(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                       uint64_t frames, uint32_t fs, double amp_min, uint32_t flags, uint64_t* peak_off, const uint16_t** d_pf,
                       const uint32_t** d_pt) {
  void *pf = nullptr, *pt = nullptr;
  if (n_clips) {
    uint64_t pcap = frames * 16 + 4096;
    const uint64_t have = std::min(ctx->ws[SHZ_WS_SP_PF].cap / 2, ctx->ws[SHZ_WS_SP_PT].cap / 4);
    if (have > 64) pcap = std::max(pcap, have - 64);
    for (int attempt = 0;; ++attempt) {
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_PF, pcap * 2 + 64, &pf));
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_PT, pcap * 4 + 64, &pt));
      uint64_t cnt = 0;
      const int32_t rc = shz_peaks(ctx, pcm, clip_off, n_clips, fs, amp_min, (flags & SHZ_PCM_DEVICE) | SHZ_OUT_DEVICE,
                                   (uint16_t*)pf, (uint32_t*)pt, peak_off, pcap, &cnt);
      if (rc == SHZ_E_CAPACITY && attempt < 2 && cnt > pcap) {
        pcap = 2 * cnt + 4096;   // (twice: the per-clip fp64 splice parks a redone clip's entries behind the batch's)
        continue;
      }
      if (rc == SHZ_E_CAPACITY) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the extraction needs %llu peaks after it was given %llu", who, (unsigned long long)cnt, (unsigned long long)pcap);
      SHZ_TRY(rc);
      break;
    }
  }
  *d_pf = (const uint16_t*)pf;
  *d_pt = (const uint32_t*)pt;
  return SHZ_OK;
}

// the hashes of every query's best variant, packed: entry i of the packed columns belongs to the last query q with
// dst_off[q] <= i (empty queries share a start) and is entry src_off[q] + (i - dst_off[q]) of the slice's columns
__global__ __launch_bounds__(SP_THREADS) void sp_gather_kernel(const uint32_t* __restrict__ key32, const uint32_t* __restrict__ t1,
                                                                const uint64_t* __restrict__ src_off /* nq */,
                                                                const uint64_t* __restrict__ dst_off /* nq + 1 */, uint32_t nq,
                                                                uint32_t* __restrict__ out_key, uint32_t* __restrict__ out_t1) {
  const uint64_t i = (uint64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= dst_off[nq]) return;
  uint32_t lo = 0, hi = nq;
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (dst_off[mid] <= i) lo = mid; else hi = mid;
  }
  const uint64_t src = src_off[lo] + (i - dst_off[lo]);
  out_key[i] = key32[src];
  out_t1[i] = t1[src];
}

// The extent stage of one slice, between its match and the next slice's warp: the queries [q0, q0 + nq) of
// the call, whose variants' hashes lie in d_key / d_t1 under query_off (nq * K + 1 entries) and whose match results are v_*
// (of the whole call, variant-major per query).  The best variant of every query is chosen as step 4 chooses it; its hashes
// are packed into SHZ_WS_SP_XKEY / _XT1 and go through ex_device, which uses the slots SHZ_WS_EX_*, SORT_A / _B and M1 / _M2:
// none of them holds anything the later slices need (the peaks and the call's tables are in SHZ_WS_SP_PF / _PT / _TAB).
// The outputs go to the rows [q0, q0 + nq) of R, the call's own block
static int32_t sp_extent_slice(shz_ctx* ctx, shz_table* t, const uint32_t* d_key, const uint32_t* d_t1, const uint64_t* query_off,
                               uint32_t q0, uint32_t nq, uint32_t K, uint32_t topn, const uint32_t* tempo_q16,
                               const uint32_t* pitch_q16, const uint32_t* v_sid, const int32_t* v_delta, const uint32_t* v_aligned,
                               const uint32_t* v_nres, uint32_t w, const sp_extent& R) {
  std::vector<uint64_t> tab((size_t)2 * nq + 1);   // src_off [nq] | dst_off [nq + 1]
  std::vector<uint32_t> c_sid((size_t)nq * topn, 0), c_n(nq), top1(K);
  std::vector<int32_t> c_dlo((size_t)nq * topn, 0), c_dhi((size_t)nq * topn, 0);
  uint64_t* dst = tab.data() + nq;
  dst[0] = 0;
  for (uint32_t q = 0; q < nq; ++q) {
    const uint64_t o = (uint64_t)(q0 + q) * K;
    for (uint32_t v = 0; v < K; ++v) top1[v] = v_nres[o + v] ? v_aligned[(o + v) * topn] : 0u;
    const uint32_t b = sp_best(top1.data(), tempo_q16, pitch_q16, K);
    tab[q] = query_off[(size_t)q * K + b];
    dst[q + 1] = dst[q] + (query_off[(size_t)q * K + b + 1] - tab[q]);
    c_n[q] = std::min(v_nres[o + b], topn);
    for (uint32_t n = 0; n < c_n[q]; ++n) {
      const int64_t d = v_delta[(o + b) * topn + n];
      c_sid[(size_t)q * topn + n] = v_sid[(o + b) * topn + n];
      c_dlo[(size_t)q * topn + n] = (int32_t)std::max<int64_t>(d - w, INT32_MIN);
      c_dhi[(size_t)q * topn + n] = (int32_t)std::min<int64_t>(d + w, INT32_MAX);
    }
  }
  const uint64_t total = dst[nq];
  void *d_tab, *xk, *xt;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_XTAB, tab.size() * 8, &d_tab));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_XKEY, total * 4 + 64, &xk));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_XT1, total * 4 + 64, &xt));
  if (total) {
    SHZ_HIP(ctx, shz_memcpy(ctx, d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sp_gather_kernel, dim3(sp_blocks(total)), dim3(SP_THREADS), 0, ctx->stream, d_key, d_t1,
                       (const uint64_t*)d_tab, (const uint64_t*)d_tab + nq, nq, (uint32_t*)xk, (uint32_t*)xt);
    SHZ_HIP(ctx, hipGetLastError());
  }
  const uint64_t c0 = (uint64_t)q0 * topn;
  ex_args A{nq, topn, c_sid.data(), c_dlo.data(), c_dhi.data(), c_n.data(), R.count + c0, R.q_first + c0, R.q_last + c0,
            R.t_first + c0, R.t_last + c0, R.hist ? R.hist + c0 * 64 : nullptr, R.shift + q0};
  A.out_sum_q = R.sum_q + c0;
  A.out_sum_u = R.sum_u + c0;
  A.out_sum_qq = R.sum_qq + c0;
  A.out_sum_qu = R.sum_qu + c0;
  return ex_device(ctx, t, "shz_recognize_warps_extents", (const uint32_t*)xk, (const uint32_t*)xt, dst, A);
}

// Steps 2-4 of a recognition at a ladder, for peaks that lie on the device (shz_recognize_warps after its extraction; the
// peak-window listeners, shz_stream.hip): the K warps of every query warped, paired and hashed (sp_count / sp_write), all
// (query, warp) pairs matched as queries of their own, the best variant of every query folded out (sp_best).  d_pf / d_pt:
// the peaks of n_clips clips, peak_off their CSR from 0 (host); query q is the clips [query_clip0[q], query_clip0[q + 1]).
// t_max: the largest warped time, the bias bound of the match.  flags: SHZ_MATCH_FULL_SORT.  out_nhash / out_profile may be
// NULL.  timed: ms_warp / ms_match (may be NULL) get the hipEvent times of the two stages, summed over the slices.  X: the
// extent stage (shz_internal.h), run on every slice while its hashes are there
int32_t sp_match_fold(shz_ctx* ctx, shz_table* t, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* peak_off,
                      uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries, uint32_t fan_value, uint32_t topn,
                      const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t K, uint32_t flags, uint64_t t_max,
                      uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                      uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, bool timed, float* ms_warp, float* ms_match,
                      const sp_extent* X) {
  if (timed)
    for (hipEvent_t& e : ctx->sp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
  const uint64_t* d_poff;
  const uint32_t *d_tempo, *d_pitch;
  SHZ_TRY(sp_upload_tables(ctx, peak_off, n_clips, tempo_q16, pitch_q16, K, &d_poff, &d_tempo, &d_pitch));
  // 2) slices of whole queries: the entries a slice can yield at most (every peak with all its partners, at every factor)
  // stay within the match's pair budget and 1/8 of the workspace limit.  A query is never split: one beyond that is a
  // slice of its own
  const uint64_t per_item = std::max<uint32_t>(fan_value - 1, 1);
  const uint64_t max_entries = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 64, 1), 1ull << 28);
  const uint32_t max_q = (ctx->debug & SHZ_DEBUG_SPEED_SMALL_SLICES) ? SP_SMALL_SLICE : (1u << 24) / K;
  const uint64_t nv = (uint64_t)n_queries * K;
  std::vector<uint32_t> v_sid(nv * topn), v_aligned(nv * topn), v_dedup(nv * topn), v_nres(nv), v_nhash(nv);
  std::vector<int32_t> v_delta(nv * topn);
  std::vector<uint64_t> ho, query_off;
  float warp_ms = 0.f, match_ms = 0.f, extent_ms = 0.f;
  // the extent stage's results, in a block of this call: the caller's arrays are written when every slice is through
  const uint64_t xc = X ? (uint64_t)n_queries * topn : 0;
  std::vector<uint32_t> x32(xc * 5 + (X && X->hist ? xc * 64 : 0) + (X ? n_queries : 0));
  std::vector<uint64_t> x64(xc * 4);
  sp_extent R{};
  if (X) {
    uint32_t* p = x32.data();
    uint64_t* s = x64.data();
    R = sp_extent{X->w, p, p + xc, p + 2 * xc, p + 3 * xc, p + 4 * xc, s, s + xc, s + 2 * xc, s + 3 * xc,
                  X->hist ? p + 5 * xc : nullptr, p + 5 * xc + (X->hist ? xc * 64 : 0), nullptr};
  }
  for (uint32_t q0 = 0; q0 < n_queries;) {
    uint32_t nq = 1;
    while (q0 + nq < n_queries && nq < max_q &&
           sp_items(peak_off, query_clip0, q0, nq + 1, K) * per_item <= max_entries)
      ++nq;
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[2], ctx->stream));
    const uint64_t n_seg = (uint64_t)(query_clip0[q0 + nq] - query_clip0[q0]) * K;
    ho.assign((size_t)n_seg + 1, 0);
    sp_pass P;
    SHZ_TRY(sp_count(ctx, d_pf, d_pt, d_poff, peak_off, query_clip0, q0, nq, d_tempo, d_pitch, K,
                     fan_value, &P, ho.data()));
    const uint64_t total = ho[n_seg];
    void *d_key, *d_t1;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_KEY, total * 4 + 64, &d_key));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_T1, total * 4 + 64, &d_t1));
    if (total) SHZ_TRY(sp_write(ctx, P, (uint32_t*)d_key, (uint32_t*)d_t1, total));
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[3], ctx->stream));
    // 3) (query, speed) = one query of the match: the segments of its channels lie one behind the other
    const uint64_t nvq = (uint64_t)nq * K;
    query_off.resize((size_t)nvq + 1);
    for (uint32_t q = 0; q < nq; ++q) {
      const uint64_t e0 = (uint64_t)(query_clip0[q0 + q] - query_clip0[q0]) * K, nch = query_clip0[q0 + q + 1] - query_clip0[q0 + q];
      for (uint32_t v = 0; v < K; ++v) query_off[(size_t)q * K + v] = ho[e0 + v * nch];
    }
    query_off[nvq] = total;
    const uint64_t o = (uint64_t)q0 * K;
    SHZ_TRY(shz_match_device(ctx, t, (const uint32_t*)d_key, (const uint32_t*)d_t1, query_off.data(), (uint32_t)nvq, topn,
                             flags & SHZ_MATCH_FULL_SORT, (int64_t)t_max, v_sid.data() + o * topn, v_delta.data() + o * topn,
                             v_aligned.data() + o * topn, v_dedup.data() + o * topn, v_nres.data() + o, v_nhash.data() + o, nullptr));
    if (timed) {
      float a = 0.f, b = 0.f;
      SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[4], ctx->stream));
      SHZ_HIP(ctx, hipEventSynchronize(ctx->sp_ev[4]));
      SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->sp_ev[2], ctx->sp_ev[3]));
      SHZ_HIP(ctx, hipEventElapsedTime(&b, ctx->sp_ev[3], ctx->sp_ev[4]));
      warp_ms += a;
      match_ms += b;
    }
    if (X) {   // (the match's results of the slice are on the host, its hashes still on the device)
      SHZ_TRY(sp_extent_slice(ctx, t, (const uint32_t*)d_key, (const uint32_t*)d_t1, query_off.data(), q0, nq, K, topn, tempo_q16,
                              pitch_q16, v_sid.data(), v_delta.data(), v_aligned.data(), v_nres.data(), X->w, R));
      if (timed) {
        float c = 0.f;
        SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[5], ctx->stream));
        SHZ_HIP(ctx, hipEventSynchronize(ctx->sp_ev[5]));
        SHZ_HIP(ctx, hipEventElapsedTime(&c, ctx->sp_ev[4], ctx->sp_ev[5]));
        extent_ms += c;
      }
    }
    q0 += nq;
  }
  if (ms_warp) *ms_warp = warp_ms;
  if (ms_match) *ms_match = match_ms;
  if (X) {
    if (X->ms_extent) *X->ms_extent = extent_ms;
    uint32_t* o32[5] = {X->count, X->q_first, X->q_last, X->t_first, X->t_last};
    const uint32_t* r32[5] = {R.count, R.q_first, R.q_last, R.t_first, R.t_last};
    uint64_t* o64[4] = {X->sum_q, X->sum_u, X->sum_qq, X->sum_qu};
    const uint64_t* r64[4] = {R.sum_q, R.sum_u, R.sum_qq, R.sum_qu};
    for (int k = 0; k < 5; ++k) memcpy(o32[k], r32[k], xc * 4);
    for (int k = 0; k < 4; ++k) memcpy(o64[k], r64[k], xc * 8);
    if (X->hist) memcpy(X->hist, R.hist, xc * 64 * 4);
    memcpy(X->shift, R.shift, (size_t)n_queries * 4);
  }
  // 4) the best variant of every query
  std::vector<uint32_t> top1(K);
  for (uint32_t q = 0; q < n_queries; ++q) {
    const uint64_t o = (uint64_t)q * K;
    for (uint32_t v = 0; v < K; ++v) top1[v] = v_nres[o + v] ? v_aligned[(o + v) * topn] : 0u;
    if (out_profile) memcpy(out_profile + o, top1.data(), (size_t)K * 4);
    const uint32_t b = sp_best(top1.data(), tempo_q16, pitch_q16, K);
    const uint64_t src = (o + b) * topn, dst = (uint64_t)q * topn;
    out_best[q] = b;
    memcpy(out_sid + dst, v_sid.data() + src, (size_t)topn * 4);
    memcpy(out_delta + dst, v_delta.data() + src, (size_t)topn * 4);
    memcpy(out_aligned + dst, v_aligned.data() + src, (size_t)topn * 4);
    memcpy(out_dedup + dst, v_dedup.data() + src, (size_t)topn * 4);
    out_nres[q] = v_nres[o + b];
    if (out_nhash) out_nhash[q] = v_nhash[o + b];
  }
  return SHZ_OK;
}

// shz_recognize_warps, and with X shz_recognize_warps_extents: one driver, the extent stage optional
static int32_t sp_recognize(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                            const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value,
                            uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                            uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                            uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, float* ms_extract, float* ms_warp,
                            float* ms_match, const sp_extent* X) {
  if (ms_extract) *ms_extract = 0.f;
  if (ms_warp) *ms_warp = 0.f;
  if (ms_match) *ms_match = 0.f;
  if (X && X->ms_extent) *X->ms_extent = 0.f;
  // everything that can be refused is refused before the first launch
  if (flags & ~(SHZ_PCM_DEVICE | SHZ_MATCH_FULL_SORT)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_warps: flags may hold SHZ_PCM_DEVICE and SHZ_MATCH_FULL_SORT");
  SHZ_TRY(sp_check_ladder(ctx, "shz_recognize_warps", "n_warps", "tempo", tempo_q16, "pitch", pitch_q16, n_warps, fan_value));
  if (n_queries == 0) {
    if (n_clips) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_warps: %u clips belong to no query", n_clips);
    return SHZ_OK;
  }
  SHZ_TRY(shz_check_clip0(ctx, "query_clip0", "query", query_clip0, n_queries, n_clips));
  SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  if (fs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "Fs must be > 0");
  if (n_clips && !pcm && clip_off[n_clips] > clip_off[0]) SHZ_FAIL(ctx, SHZ_E_INVALID, "pcm is NULL");
  if (!out_best || !out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_recognize_warps: NULL buffer");
  if (X) {
    const char* who = "shz_recognize_warps_extents";
    if (!X->count || !X->q_first || !X->q_last || !X->t_first || !X->t_last || !X->sum_q || !X->sum_u || !X->sum_qq || !X->sum_qu ||
        !X->shift)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL extent array", who);
    if (topn > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: topn must be in [1,64], one candidate a result", who);
    if (2ull * X->w + 1 > EX_FIT_MAX_WIDTH)
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: vote tolerance + drift_bins = %u; a candidate's 2 w + 1 bins must be <= %d", who, X->w,
               EX_FIT_MAX_WIDTH);
    SHZ_TRY(ex_state(ctx, t, who, topn));
    SHZ_TRY(ex_table_limits(ctx, t, who));
  }
  const uint32_t K = n_warps, s_max = *std::max_element(tempo_q16, tempo_q16 + K);   // (time alone: the bias bound)
  uint64_t max_frames = 1, frames = 0;
  for (uint32_t c = 0; c < n_clips; ++c) {
    const uint64_t f = shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop);
    max_frames = std::max(max_frames, f);
    frames += f;
  }
  // the largest warped time: round((max_frames - 1) s_max), the bias bound of the match
  const uint64_t t_max = ((max_frames - 1) * s_max + 32768) >> 16;
  if (t_max >= (1ull << 20))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_recognize_warps: a clip of %llu frames at time factor %u / 65536 reaches t' = %llu; query offsets must be < 2^20",
             (unsigned long long)max_frames, s_max, (unsigned long long)t_max);
  SHZ_TRY(shz_match_ready(ctx, t, topn));
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = ms_extract || ms_warp || ms_match || (X && X->ms_extent);
  if (timed) {
    for (hipEvent_t& e : ctx->sp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[0], ctx->stream));
  }
  // 1) the peaks of every clip, once, into the library's own buffers
  std::vector<uint64_t> peak_off((size_t)n_clips + 1, 0);
  const uint16_t* d_pf = nullptr;
  const uint32_t* d_pt = nullptr;
  SHZ_TRY(sp_peaks_owned(ctx, "shz_recognize_warps", pcm, clip_off, n_clips, frames, fs, amp_min, flags & SHZ_PCM_DEVICE,
                         peak_off.data(), &d_pf, &d_pt));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[1], ctx->stream));
  // 2-4) warped, hashed, matched in slices of whole queries; the best variant of every query
  SHZ_TRY(sp_match_fold(ctx, t, d_pf, d_pt, peak_off.data(), n_clips, query_clip0, n_queries, fan_value, topn, tempo_q16, pitch_q16,
                        K, flags & SHZ_MATCH_FULL_SORT, t_max, out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres,
                        out_nhash, out_profile, timed, ms_warp, ms_match, X));
  if (timed && ms_extract) SHZ_HIP(ctx, hipEventElapsedTime(ms_extract, ctx->sp_ev[0], ctx->sp_ev[1]));
  return SHZ_OK;
}

extern "C" int32_t shz_recognize_warps(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                       const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min,
                                       uint32_t fan_value, uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16,
                                       uint32_t n_warps, uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                       uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                       uint32_t* out_profile, float* ms_extract, float* ms_warp, float* ms_match) {
  if (!ctx || !t) return SHZ_E_INVALID;
  return sp_recognize(ctx, t, pcm, clip_off, n_clips, query_clip0, n_queries, fs, amp_min, fan_value, topn, tempo_q16, pitch_q16,
                      n_warps, flags, out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_profile,
                      ms_extract, ms_warp, ms_match, nullptr);
}

extern "C" int32_t shz_recognize_warps_extents(
    shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* query_clip0,
    uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value, uint32_t topn, const uint32_t* tempo_q16,
    const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
    uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, float* ms_extract,
    float* ms_warp, float* ms_match, uint32_t drift_bins, uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last,
    uint32_t* out_t_first, uint32_t* out_t_last, uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq,
    uint64_t* out_sum_qu, uint32_t* out_hist, uint32_t* out_shift, float* ms_extent) {
  if (!ctx || !t) return SHZ_E_INVALID;
  const uint64_t w = (uint64_t)ctx->vote_tol + drift_bins;
  const sp_extent X{(uint32_t)std::min<uint64_t>(w, 0xFFFFFFFFull), out_count, out_q_first, out_q_last, out_t_first, out_t_last,
                    out_sum_q, out_sum_u, out_sum_qq, out_sum_qu, out_hist, out_shift, ms_extent};
  return sp_recognize(ctx, t, pcm, clip_off, n_clips, query_clip0, n_queries, fs, amp_min, fan_value, topn, tempo_q16, pitch_q16,
                      n_warps, flags, out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_profile,
                      ms_extract, ms_warp, ms_match, &X);
}

// the speed ladder: one table for time and frequency (its own names in what is refused about it)
extern "C" int32_t shz_recognize_speeds(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                        const uint32_t* query_clip0, uint32_t n_queries, uint32_t fs, double amp_min,
                                        uint32_t fan_value, uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds,
                                        uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                        uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                        uint32_t* out_profile, float* ms_extract, float* ms_warp, float* ms_match) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (ms_extract) *ms_extract = 0.f;
  if (ms_warp) *ms_warp = 0.f;
  if (ms_match) *ms_match = 0.f;
  SHZ_TRY(sp_check_ladder(ctx, "shz_recognize_speeds", "n_speeds", "speed", speed_q16, "speed", speed_q16, n_speeds, fan_value));
  return shz_recognize_warps(ctx, t, pcm, clip_off, n_clips, query_clip0, n_queries, fs, amp_min, fan_value, topn, speed_q16,
                             speed_q16, n_speeds, flags, out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash,
                             out_profile, ms_extract, ms_warp, ms_match);
}

extern "C" int32_t shz_recognize_speeds_extents(
    shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* query_clip0,
    uint32_t n_queries, uint32_t fs, double amp_min, uint32_t fan_value, uint32_t topn, const uint32_t* speed_q16, uint32_t n_speeds,
    uint32_t flags, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
    uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, float* ms_extract, float* ms_warp, float* ms_match,
    uint32_t drift_bins, uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
    uint32_t* out_t_last, uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq, uint64_t* out_sum_qu, uint32_t* out_hist,
    uint32_t* out_shift, float* ms_extent) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (ms_extract) *ms_extract = 0.f;
  if (ms_warp) *ms_warp = 0.f;
  if (ms_match) *ms_match = 0.f;
  if (ms_extent) *ms_extent = 0.f;
  SHZ_TRY(sp_check_ladder(ctx, "shz_recognize_speeds_extents", "n_speeds", "speed", speed_q16, "speed", speed_q16, n_speeds, fan_value));
  return shz_recognize_warps_extents(ctx, t, pcm, clip_off, n_clips, query_clip0, n_queries, fs, amp_min, fan_value, topn, speed_q16,
                                     speed_q16, n_speeds, flags, out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres,
                                     out_nhash, out_profile, ms_extract, ms_warp, ms_match, drift_bins, out_count, out_q_first,
                                     out_q_last, out_t_first, out_t_last, out_sum_q, out_sum_u, out_sum_qq, out_sum_qu, out_hist,
                                     out_shift, ms_extent);
}
