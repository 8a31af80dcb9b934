// Scanning long recordings (the loop a monitor puts around recognize(), recognizer.py:357-392: record a stretch, fingerprint
// every channel, union the hashes, match, align -- here for every overlapping stretch of a recording at once): each recording
// is fingerprinted ONCE, its device-resident hash list is cut into overlapping time windows, and all windows are matched
// together, recording-major; or its peaks are extracted once, warped for every rung of a speed ladder, and
// every window is matched at every rung.
//
// Both scans share one window stage (sc_windows).  Within a clip the hashes come out in generation order: peaks sorted by
// time, t1 the anchor's time (recognizer.py:100-114), so t1 never decreases, and neither does the warped t1' of one rung.
// The window that starts at recording frame s is, at rung v, the range W_v(s) <= t1' < W_v(s + window_frames) of every
// channel's list, W_v(x) = (x s16 + 32768) >> 16 -- two lower-bound searches.  A window's query at a rung is the union over
// the recording's channels of (key32, t1' - W_v(s)): what `offset` means for a clip recorded from frame s, as the listeners
// have it.  The plain scan is the unity case: one rung of factor 65536, W(x) = x, over the extraction's own hash lists.
// Nothing per window is built on the host: the kernels derive s and both bounds from one descriptor per recording and the
// rung table.  The items are (window, rung, channel), window-major, so that (window, rung) is one contiguous query of the
// match with its channels one behind the other.  The windows' columns are replicated ceil(window / step) times, so they
// are written group by group into two slots and each group is matched where it lies.  A scan over warp pairs may hand the
// stage a selection: every window tries a list of rungs of its own, a query is then a SLOT of that list, and
// the items are (slot, channel).
#include <algorithm>

#include "shz_internal.h"

#define SC_THREADS 256
#define SC_SMALL_GROUP 3u   // windows of a group under SHZ_DEBUG_SCAN_SMALL_GROUPS / SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES
#define SS_SMALL_RUNGS 2u   // rungs of a slice under SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES (and 1 recording a slice)

struct sc_rec {        // one recording of a slice; the entry behind the last one holds the slice's totals
  uint64_t win0;       // its first window among the slice's windows
  uint64_t slot0;      // its first query (window, rung): win0 x rungs, or with a selection the slots in front of it
  uint64_t item0;      // its first (window, rung, channel) item: the sum of queries x channels in front of it
  uint64_t seg0;       // its first segment of the hashes' CSR: (rung, channel) at seg0 + rung * nch + channel
  uint32_t nch, pad;
};

extern "C" uint64_t shz_scan_window_count(uint64_t frames, uint32_t window_frames, uint32_t step_frames) {
  if (frames == 0 || window_frames == 0 || step_frames == 0) return 0;
  if (frames <= window_frames) return 1;
  return (frames - window_frames + step_frames - 1) / step_frames + 1;
}

// first index in [a, b) whose t1 is >= v (t1 does not decrease inside a clip)
__device__ __forceinline__ uint64_t sc_lower_bound(const uint32_t* __restrict__ t1, uint64_t a, uint64_t b, uint64_t v) {
  while (a < b) {
    const uint64_t mid = a + ((b - a) >> 1);
    if ((uint64_t)t1[mid] < v) a = mid + 1; else b = mid;
  }
  return a;
}

// sp_warp_t, unclamped (x < 2^47: frame counts are far below); at s16 = 65536 it is x itself
__device__ __forceinline__ uint64_t sc_warp(uint64_t x, uint32_t s16) { return (x * s16 + 32768u) >> 16; }

// Query q of recording r -> its window (counted inside the recording) and its rung.  Dense: every window has the slice's kc
// rungs, so both follow from one division.  With a selection (slot_off != NULL) a query is a SLOT: slot_off is
// the CSR of the slots over the slice's windows and slot_warp the rung of every slot, so the window is the last one of the
// recording whose first slot is <= q -- windows with empty lists share a start with the window behind them, and the last
// of such a run is the one that holds q, because q exists -- and the rung is read from the slot.
__device__ __forceinline__ void sc_query(const sc_rec* __restrict__ recs, uint32_t r, const sc_rec& R, uint64_t q, uint32_t kc,
                                         const uint64_t* __restrict__ slot_off, const uint32_t* __restrict__ slot_warp,
                                         uint64_t* w, uint32_t* v) {
  if (!slot_off) {   // (uniform: a kernel argument)
    const uint64_t rem = q - R.slot0, ww = rem / kc;
    *w = ww;
    *v = (uint32_t)(rem - ww * kc);
    return;
  }
  uint64_t lo = R.win0, hi = recs[r + 1].win0;   // (the recording has a slot, so it has a window: lo < hi)
  while (lo + 1 < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (slot_off[mid] <= q) lo = mid; else hi = mid;
  }
  *w = lo - R.win0;
  *v = slot_warp[q];
}

// per (query, channel): where the window's hashes begin in the list of (rung, channel), and how many they are
__global__ __launch_bounds__(SC_THREADS) void sc_bounds_kernel(const sc_rec* __restrict__ recs, uint32_t nr, uint64_t n_items,
                                                               const uint32_t* __restrict__ speed, uint32_t kc,
                                                               const uint64_t* __restrict__ slot_off,
                                                               const uint32_t* __restrict__ slot_warp, uint32_t window_frames,
                                                               uint32_t step_frames, const uint64_t* __restrict__ hoff,
                                                               const uint32_t* __restrict__ t1, uint64_t* __restrict__ first,
                                                               uint64_t* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= n_items) return;
  uint32_t lo = 0, hi = nr;   // the last recording whose first item is <= i (recordings without items share a start)
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (recs[mid].item0 <= i) lo = mid; else hi = mid;
  }
  const sc_rec R = recs[lo];
  const uint64_t rem = i - R.item0, ql = rem / R.nch, c = rem - ql * R.nch;
  uint64_t w;
  uint32_t v;
  sc_query(recs, lo, R, R.slot0 + ql, kc, slot_off, slot_warp, &w, &v);
  if (v >= kc) {   // (the host checks every slot; a rung outside the slice's table would read outside the CSR)
    first[i] = 0;
    cnt[i] = 0;
    return;
  }
  const uint32_t s16 = speed[v];
  // (with step > window the last window may start behind the recording's end, above every t1: the searches compare in
  // 64 bits, so it is empty whatever its start is, with no clamp to the 32 bits of t1)
  const uint64_t s = w * step_frames, e = R.seg0 + (uint64_t)v * R.nch + c;
  const uint64_t a = hoff[e], b = hoff[e + 1];
  const uint64_t p = sc_lower_bound(t1, a, b, sc_warp(s, s16));
  const uint64_t q = sc_lower_bound(t1, p, b, sc_warp(s + window_frames, s16));
  first[i] = p;
  cnt[i] = q - p;
}

// one workgroup per query (window, rung) of the group [q0, q0 + gridDim.x) of the slice's queries: its channels' ranges, one
// behind the other, to offs[item] - base of the group's columns (offs: exclusive scan of the counts, the total behind it)
__global__ __launch_bounds__(SC_THREADS) void sc_gather_kernel(const sc_rec* __restrict__ recs, uint32_t nr, uint64_t q0,
                                                               const uint32_t* __restrict__ speed, uint32_t kc,
                                                               const uint64_t* __restrict__ slot_off,
                                                               const uint32_t* __restrict__ slot_warp, uint32_t step_frames,
                                                               const uint64_t* __restrict__ first, const uint64_t* __restrict__ offs,
                                                               uint64_t base, uint64_t cap, const uint32_t* __restrict__ key,
                                                               const uint32_t* __restrict__ t1, uint32_t* __restrict__ out_key,
                                                               uint32_t* __restrict__ out_qo) {
  const uint64_t q = q0 + blockIdx.x;
  uint32_t lo = 0, hi = nr;   // the last recording whose first query is <= q (recordings without queries share a start)
  while (lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (recs[mid].slot0 <= q) lo = mid; else hi = mid;
  }
  const sc_rec R = recs[lo];
  uint64_t w;
  uint32_t v;
  sc_query(recs, lo, R, q, kc, slot_off, slot_warp, &w, &v);
  if (v >= kc) return;   // (uniform; its items were counted as empty)
  const uint32_t t0 = (uint32_t)sc_warp(w * step_frames, speed[v]);   // (a window with entries starts below their t1' < 2^32)
  for (uint32_t c = 0; c < R.nch; ++c) {
    const uint64_t p = R.item0 + (q - R.slot0) * R.nch + c;
    const uint64_t src = first[p], dst = offs[p] - base, n = offs[p + 1] - offs[p];
    if (dst + n > cap) return;   // (uniform; the host sizes the columns from the same offsets, so this never holds)
    for (uint64_t i = threadIdx.x; i < n; i += SC_THREADS) {
      out_key[dst + i] = key[src + i];
      out_qo[dst + i] = t1[src + i] - t0;
    }
  }
}

// ---- what both scans refuse before the first launch ---------------------------------------------------------------------
// In three parts, because the order of the refusals is part of the ABI and the speed scan's own (ladder, warped window
// length; Fs, pcm) lie between them.
static int32_t sc_check(shz_ctx* ctx, const char* who, uint32_t flags, const uint64_t* win_off, const uint64_t* count,
                        uint32_t window_frames, uint32_t step_frames) {
  if (flags & ~(SHZ_PCM_DEVICE | SHZ_MATCH_FULL_SORT)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE and SHZ_MATCH_FULL_SORT", who);
  if (!win_off || !count) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: win_off or count is NULL", who);
  if (window_frames == 0 || window_frames >= (1u << 20))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: window_frames must be in [1, 2^20) (query offsets), got %u", who, window_frames);
  if (step_frames == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: step_frames must be at least 1", who);
  return SHZ_OK;
}
// the recordings' clips; without recordings there is nothing more to check, and the caller is done
static int32_t sc_check_recs(shz_ctx* ctx, const char* who, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* rec_clip0,
                             uint32_t n_recs, uint64_t* win_off) {
  win_off[0] = 0;
  if (n_recs == 0) {
    if (n_clips) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %u clips belong to no recording", who, n_clips);
    return SHZ_OK;
  }
  SHZ_TRY(shz_check_clip0(ctx, "rec_clip0", "recording", rec_clip0, n_recs, n_clips));
  return shz_check_clip_off(ctx, clip_off, n_clips);
}
// the windows: their number follows from the frame counts alone, in the recording's own frames.  win_off and *count are
// written whether or not the caller has room for them; *frames (if asked for): the frames of all clips together
static int32_t sc_count_windows(shz_ctx* ctx, const char* who, const uint64_t* clip_off, const uint32_t* rec_clip0, uint32_t n_recs,
                                uint32_t window_frames, uint32_t step_frames, uint64_t cap_windows, uint64_t* win_off,
                                uint64_t* count, uint64_t* frames) {
  uint64_t n_wins = 0, all = 0;
  for (uint32_t r = 0; r < n_recs; ++r) {
    uint64_t f = 0;
    for (uint32_t c = rec_clip0[r]; c < rec_clip0[r + 1]; ++c) {
      const uint64_t fc = shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop);
      f = std::max<uint64_t>(f, fc);
      all += fc;
    }
    n_wins += shz_scan_window_count(f, window_frames, step_frames);
    win_off[r + 1] = n_wins;
  }
  *count = n_wins;
  if (frames) *frames = all;
  if (n_wins > cap_windows)
    SHZ_FAIL(ctx, SHZ_E_CAPACITY, "%s: %llu windows, room for %llu", who, (unsigned long long)n_wins, (unsigned long long)cap_windows);
  return SHZ_OK;
}

// ---- the window stage ---------------------------------------------------------------------------------------------------
struct sc_slice {
  const uint32_t* clip0;         // rec_clip0 and win_off of the call from the slice's first recording on: nr + 1 entries
  const uint64_t* woff;          // (at least one of the nr recordings has a window)
  uint32_t nr, kc;
  const uint32_t* speed;         // the slice's kc rungs (Q16): their time factors
  const uint64_t* hoff;          // CSR of the segments (recording, rung, channel) over key / t1, relative to them
  bool tables_on_host;           // speed and hoff are on the host (they go up with the descriptors) / on the device
  const uint32_t *d_key, *d_t1;  // the hashes (device), `total` of them
  uint64_t total;
  uint32_t window_frames, step_frames, topn, flags;   // flags: SHZ_MATCH_FULL_SORT
  int64_t bias_bound;            // of the match: no query offset is above it
  uint64_t rep;                  // the windows a hash can lie in at one rung (the sanity bound)
  bool small_groups;             // SC_SMALL_GROUP windows a group (the callers' debug switches)
  uint32_t *sid, *aligned, *dedup, *nres, *nhash;   // results, query-major: (window, rung), or slot by slot; nhash and
  int32_t* delta;                                   // npairs may be NULL
  uint64_t* npairs;
  // a selection (host; NULL: every window at all kc rungs): slot_off = the CSR of the slots over the slice's windows from 0,
  // slot_warp = the rung of every slot, < kc and ascending inside a window.  They go up with the descriptors
  const uint64_t* slot_off;
  const uint32_t* slot_warp;
  uint64_t* entries;             // (may be NULL) the window entries handed to the match are added to it
};

// Cuts the slice's hash lists into its windows and matches every query.  Device times are added to *win_ms and
// *match_ms when `timed` (events sc_ev[2 .. 4]).  The stream is idle on return.
static int32_t sc_windows(shz_ctx* ctx, shz_table* t, const char* who, const sc_slice& S, bool timed, float* win_ms, float* match_ms) {
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[2], ctx->stream));
  const uint32_t nr = S.nr, kc = S.kc, topn = S.topn, *clip0 = S.clip0;
  const uint64_t* woff = S.woff;
  const bool sel = S.slot_off != nullptr;
  const uint64_t nws = woff[nr] - woff[0], n_seg = (uint64_t)(clip0[nr] - clip0[0]) * kc;
  auto slot_at = [&](uint64_t w) { return sel ? S.slot_off[w] : w * kc; };   // the first query of window w
  const uint64_t n_slots = slot_at(nws);
  // 1) one descriptor a recording (behind them, if they come from the host: hoff | speed; with a selection: the slot CSR),
  // and the first item of every window
  const uint64_t rec_bytes = ((uint64_t)nr + 1) * sizeof(sc_rec), hoff_bytes = S.tables_on_host ? (n_seg + 1) * 8 : 0;
  const uint64_t soff_bytes = sel ? (nws + 1) * 8 : 0, speed_bytes = S.tables_on_host ? (uint64_t)kc * 4 : 0;
  std::vector<char> block(rec_bytes + hoff_bytes + soff_bytes + speed_bytes + (sel ? n_slots * 4 : 0));
  sc_rec* hrec = (sc_rec*)block.data();
  std::vector<uint64_t> win_item((size_t)nws + 1), win_nch((size_t)nws);
  uint64_t n_items = 0;
  for (uint32_t r = 0; r < nr; ++r) {
    const uint32_t nch = clip0[r + 1] - clip0[r];
    const uint64_t w0 = woff[r] - woff[0], nw = woff[r + 1] - woff[r];
    hrec[r] = sc_rec{w0, slot_at(w0), n_items, (uint64_t)(clip0[r] - clip0[0]) * kc, nch, 0};
    for (uint64_t w = 0; w < nw; ++w) {
      win_item[w0 + w] = n_items + (slot_at(w0 + w) - slot_at(w0)) * nch;
      win_nch[w0 + w] = nch;
    }
    n_items += (slot_at(w0 + nw) - slot_at(w0)) * nch;
  }
  hrec[nr] = sc_rec{nws, n_slots, n_items, n_seg, 0, 0};
  win_item[nws] = n_items;
  if (n_items == 0) {   // (a selection that leaves the slice without a slot: nothing to cut, nothing to match)
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return SHZ_OK;
  }
  void *d_rec, *d_ctl;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_JOBS, block.size(), &d_rec));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_CTL, (3 * n_items + 1) * 8, &d_ctl));
  uint64_t *d_first = (uint64_t*)d_ctl, *d_cnt = d_first + n_items, *d_offs = d_cnt + n_items;   // d_offs[n_items] = the total
  const uint64_t* d_hoff = S.hoff;
  const uint32_t* d_speed = S.speed;
  const uint64_t* d_soff = nullptr;
  const uint32_t* d_swarp = nullptr;
  if (S.tables_on_host) {
    memcpy(block.data() + rec_bytes, S.hoff, hoff_bytes);
    memcpy(block.data() + rec_bytes + hoff_bytes + soff_bytes, S.speed, speed_bytes);
    d_hoff = (const uint64_t*)((char*)d_rec + rec_bytes);
    d_speed = (const uint32_t*)((char*)d_rec + rec_bytes + hoff_bytes + soff_bytes);
  }
  if (sel) {   // (8-byte entries in front of 4-byte ones: every table keeps its alignment)
    memcpy(block.data() + rec_bytes + hoff_bytes, S.slot_off, soff_bytes);
    memcpy(block.data() + rec_bytes + hoff_bytes + soff_bytes + speed_bytes, S.slot_warp, n_slots * 4);
    d_soff = (const uint64_t*)((char*)d_rec + rec_bytes + hoff_bytes);
    d_swarp = (const uint32_t*)((char*)d_rec + rec_bytes + hoff_bytes + soff_bytes + speed_bytes);
  }
  // 2) upload, 3) bounds, scan, one read-back: the offsets of every item
  std::vector<uint64_t> offs((size_t)n_items + 1, 0);
  if (S.total) {   // (without hashes every window is empty, and a warp pass has no CSR on the device)
    SHZ_HIP(ctx, shz_memcpy(ctx, d_rec, block.data(), block.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sc_bounds_kernel, dim3((unsigned)((n_items + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, ctx->stream,
                       (const sc_rec*)d_rec, nr, n_items, d_speed, kc, d_soff, d_swarp, S.window_frames, S.step_frames, d_hoff, S.d_t1,
                       d_first, d_cnt);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(shz_scan_u64(ctx, d_cnt, d_offs, n_items, d_offs + n_items));
    SHZ_HIP(ctx, shz_memcpy(ctx, offs.data(), d_offs, (n_items + 1) * 8, hipMemcpyDeviceToHost));
  }
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[3], ctx->stream));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (timed) {
    float a = 0.f;
    SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->sc_ev[2], ctx->sc_ev[3]));
    *win_ms += a;
  }
  // 4) a hash lies in at most `rep` windows
  if (offs[n_items] > S.total * S.rep)
    SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu window entries from %llu hashes", who, (unsigned long long)offs[n_items],
             (unsigned long long)S.total);
  if (S.entries) *S.entries += offs[n_items];
  auto win_at = [&](uint64_t w) { return offs[win_item[w]]; };
  // 5) the groups.  A group's columns take at most 1/8 of the workspace limit (the match sizes its own sub-batches inside a
  // group) and hold at most 2^24 queries; a window is never split and its rungs stay together, so one larger than that is
  // a group of its own
  const uint64_t max_entries = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 64, 1), 1ull << 30);
  const uint64_t max_wins = S.small_groups ? SC_SMALL_GROUP : ~0ull;
  std::vector<uint64_t> groups{0};   // first window of every group, nws behind them
  uint64_t m_max = 0;
  for (uint64_t g0 = 0; g0 < nws;) {
    uint64_t g1 = g0 + 1;
    while (g1 < nws && g1 - g0 < max_wins && slot_at(g1 + 1) - slot_at(g0) <= (1ull << 24) && win_at(g1 + 1) - win_at(g0) <= max_entries)
      ++g1;
    m_max = std::max(m_max, win_at(g1) - win_at(g0));
    groups.push_back(g1);
    g0 = g1;
  }
  // 6) the columns of the largest group, 7) group by group: gather the columns of every query, match them where they lie
  void *d_gk, *d_gq;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_KEY, m_max * 4 + 64, &d_gk));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_QO, m_max * 4 + 64, &d_gq));
  std::vector<uint64_t> query_off;
  for (size_t g = 0; g + 1 < groups.size(); ++g) {
    const uint64_t g0 = groups[g], g1 = groups[g + 1], base = win_at(g0), m = win_at(g1) - base, o = slot_at(g0), nq = slot_at(g1) - o;
    if (nq == 0) continue;   // (windows without a slot)
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[2], ctx->stream));
    if (m) {
      hipLaunchKernelGGL(sc_gather_kernel, dim3((unsigned)nq), dim3(SC_THREADS), 0, ctx->stream, (const sc_rec*)d_rec, nr, o, d_speed,
                         kc, d_soff, d_swarp, S.step_frames, (const uint64_t*)d_first, (const uint64_t*)d_offs, base, m, S.d_key,
                         S.d_t1, (uint32_t*)d_gk, (uint32_t*)d_gq);
      SHZ_HIP(ctx, hipGetLastError());
    }
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[3], ctx->stream));
    query_off.resize((size_t)nq + 1);
    for (uint64_t w = g0; w < g1; ++w)
      for (uint64_t j = 0, nj = slot_at(w + 1) - slot_at(w); j < nj; ++j)
        query_off[(size_t)(slot_at(w) - o + j)] = offs[win_item[w] + j * win_nch[w]] - base;
    query_off[nq] = m;
    SHZ_TRY(shz_match_device(ctx, t, (const uint32_t*)d_gk, (const uint32_t*)d_gq, query_off.data(), (uint32_t)nq, topn, S.flags,
                             S.bias_bound, S.sid + o * topn, S.delta + o * topn, S.aligned + o * topn, S.dedup + o * topn,
                             S.nres + o, S.nhash ? S.nhash + o : nullptr, S.npairs ? S.npairs + o : nullptr));
    if (timed) {
      float a = 0.f, b = 0.f;
      SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[4], ctx->stream));
      SHZ_HIP(ctx, hipEventSynchronize(ctx->sc_ev[4]));
      SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->sc_ev[2], ctx->sc_ev[3]));
      SHZ_HIP(ctx, hipEventElapsedTime(&b, ctx->sc_ev[3], ctx->sc_ev[4]));
      *win_ms += a;
      *match_ms += b;
    }
  }
  return SHZ_OK;
}

// ---- the plain scan: the body that shz_scan_batch and shz_scan_extents share, in its two halves -------------------------
struct sc_plain {      // the arguments of shz_scan_batch
  const int16_t* pcm;
  const uint64_t* clip_off;
  uint32_t n_clips;
  const uint32_t* rec_clip0;
  uint32_t n_recs, fs;
  double amp_min;
  uint32_t fan_value, window_frames, step_frames, topn, flags;
  uint64_t* win_off;
  uint32_t* out_sid;
  int32_t* out_delta;
  uint32_t *out_aligned, *out_dedup, *out_nres, *out_nhash;
  uint64_t* out_npairs;
  uint64_t cap_windows;
  uint64_t* count;
  float *ms_extract, *ms_window, *ms_match;
};

// everything the plain scan refuses, in its order, before the first launch.  *done: the call is over with SHZ_OK (no
// recording, or no window) and nothing is to be launched
static int32_t sc_plain_check(shz_ctx* ctx, shz_table* t, const char* who, const sc_plain& P, bool* done) {
  *done = true;
  if (P.ms_extract) *P.ms_extract = 0.f;
  if (P.ms_window) *P.ms_window = 0.f;
  if (P.ms_match) *P.ms_match = 0.f;
  if (P.count) *P.count = 0;
  SHZ_TRY(sc_check(ctx, who, P.flags, P.win_off, P.count, P.window_frames, P.step_frames));
  if (P.fan_value < 1 || P.fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  SHZ_TRY(sc_check_recs(ctx, who, P.clip_off, P.n_clips, P.rec_clip0, P.n_recs, P.win_off));
  if (P.n_recs == 0) return SHZ_OK;
  SHZ_TRY(shz_match_ready(ctx, t, P.topn));
  SHZ_TRY(sc_count_windows(ctx, who, P.clip_off, P.rec_clip0, P.n_recs, P.window_frames, P.step_frames, P.cap_windows, P.win_off,
                           P.count, nullptr));
  if (*P.count == 0) return SHZ_OK;
  if (!P.out_sid || !P.out_delta || !P.out_aligned || !P.out_dedup || !P.out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL buffer", who);
  *done = false;
  return SHZ_OK;
}

// extraction, window stage and match of a checked call.  hash_off (n_clips + 1, host) and *d_key / *d_t1 are the extraction's
// columns: they lie in SHZ_WS_RQ_KEY / _T1, which neither the window stage nor the match reserves, so they are intact -- and the
// stream idle (sc_windows) -- on return.  `timed` also when the caller times a stage of its own behind this
static int32_t sc_plain_run(shz_ctx* ctx, shz_table* t, const char* who, const sc_plain& P, bool timed, uint64_t* hash_off,
                            const uint32_t** d_key, const uint32_t** d_t1) {
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  if (timed) {
    for (hipEvent_t& e : ctx->sc_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[0], ctx->stream));
  }
  // 1) every clip fingerprinted once, into the library's own buffers
  SHZ_TRY(shz_extract_owned(ctx, who, P.pcm, P.clip_off, P.n_clips, P.fs, P.amp_min, P.fan_value, P.flags & SHZ_PCM_DEVICE, hash_off,
                            d_key, d_t1));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[1], ctx->stream));
  // 2) the window stage at unity: all recordings, one rung of factor 65536 over the extraction's own CSR.  A hash lies in
  // at most ceil(window / step) windows; no query offset reaches window_frames
  const uint32_t one = SP_S_ONE;
  float win_ms = 0.f, match_ms = 0.f;
  sc_slice S{P.rec_clip0, P.win_off, P.n_recs, 1, &one, hash_off, true, *d_key, *d_t1, hash_off[P.n_clips], P.window_frames,
             P.step_frames, P.topn, P.flags & SHZ_MATCH_FULL_SORT, (int64_t)P.window_frames - 1,
             ((uint64_t)P.window_frames + P.step_frames - 1) / P.step_frames, (ctx->debug & SHZ_DEBUG_SCAN_SMALL_GROUPS) != 0, P.out_sid,
             P.out_aligned, P.out_dedup, P.out_nres, P.out_nhash, P.out_delta, P.out_npairs};
  SHZ_TRY(sc_windows(ctx, t, who, S, timed, &win_ms, &match_ms));
  if (P.ms_extract) SHZ_HIP(ctx, hipEventElapsedTime(P.ms_extract, ctx->sc_ev[0], ctx->sc_ev[1]));
  if (P.ms_window) *P.ms_window = win_ms;
  if (P.ms_match) *P.ms_match = match_ms;
  return SHZ_OK;
}

extern "C" int32_t shz_scan_batch(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                  const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                  uint32_t window_frames, uint32_t step_frames, uint32_t topn, uint32_t flags, uint64_t* win_off,
                                  uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                                  uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs, uint64_t cap_windows,
                                  uint64_t* count, float* ms_extract, float* ms_window, float* ms_match) {
  const char* who = "shz_scan_batch";
  if (!ctx || !t) return SHZ_E_INVALID;
  const sc_plain P{pcm, clip_off, n_clips, rec_clip0, n_recs, fs, amp_min, fan_value, window_frames, step_frames, topn, flags, win_off,
                   out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, cap_windows, count, ms_extract,
                   ms_window, ms_match};
  // everything that can be refused is refused before the first launch
  bool done;
  SHZ_TRY(sc_plain_check(ctx, t, who, P, &done));
  if (done) return SHZ_OK;
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  return sc_plain_run(ctx, t, who, P, ms_extract || ms_window || ms_match, hash_off.data(), &d_key, &d_t1);
}

// ---- the timeline fold: the per-window answers of a scan folded into segments, on the host --------------------------------
// "Song X from window a to window b": a hit is a window whose best answer has min_aligned aligned hashes; a hit extends the
// open segment of its recording if it names the same song, lies at most max_gap windows behind the segment's last hit and the
// entry point's rule says it follows; any other hit closes the segment and opens one.  Segments beyond cap are counted and not
// written.  The three timelines differ in the rule alone:
//   follows(g, w, gap, delta)   does the hit at window w of its recording (g of all), gap windows after the last, continue?
//   take(g, w, delta, first)    the hit is the segment's (first: it opens one)
//   write(n)                    the rule's own outputs of the open segment, as segment n
static inline bool sc_hit(const uint32_t* aligned, const uint32_t* nres, uint32_t topn, uint32_t min_aligned, uint64_t g) {
  return nres[g] >= 1 && aligned[g * topn] >= min_aligned;
}

// win_off is a CSR whose recordings hold at most 2^32-1 windows each
static bool sc_win_off_ok(const uint64_t* win_off, uint32_t n_recs) {
  for (uint32_t r = 0; r < n_recs; ++r)
    if (win_off[r + 1] < win_off[r] || win_off[r + 1] - win_off[r] > 0xFFFFFFFFull) return false;
  return true;
}

static bool sc_factors_ok(const uint32_t* q16, uint32_t n) {
  for (uint32_t v = 0; v < n; ++v)
    if (q16[v] < SP_S_MIN || q16[v] > SP_S_MAX) return false;
  return true;
}

template <class Rule>
static int32_t sc_fold(const uint64_t* win_off, uint32_t n_recs, const uint32_t* sid, const int32_t* delta, const uint32_t* aligned,
                       const uint32_t* nres, uint32_t topn, uint32_t min_aligned, uint32_t max_gap, uint32_t* seg_rec,
                       uint32_t* seg_sid, uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best, uint64_t cap,
                       uint64_t* count, Rule& rule) {
  uint64_t n = 0;
  for (uint32_t r = 0; r < n_recs; ++r) {
    bool open = false;
    uint32_t o_sid = 0, o_first = 0, o_last = 0, o_hits = 0, o_best = 0;
    auto close = [&]() {
      if (open && n < cap) {
        seg_rec[n] = r;
        seg_sid[n] = o_sid;
        seg_first[n] = o_first;
        seg_last[n] = o_last;
        seg_hits[n] = o_hits;
        seg_best[n] = o_best;
        rule.write(n);
      }
      n += open ? 1 : 0;
      open = false;
    };
    const uint64_t nw = win_off[r + 1] - win_off[r];
    for (uint64_t w = 0; w < nw; ++w) {
      const uint64_t g = win_off[r] + w;
      if (!sc_hit(aligned, nres, topn, min_aligned, g)) continue;   // no hit: changes nothing
      const uint32_t s = sid[g * topn], a = aligned[g * topn];
      const int64_t d = delta[g * topn];
      const bool cont = open && s == o_sid && w - o_last - 1 <= max_gap && rule.follows(g, w, w - o_last, d);
      if (!cont) {
        close();
        open = true;
        o_sid = s;
        o_first = (uint32_t)w;
        o_hits = 0;
        o_best = a;
      }
      o_last = (uint32_t)w;
      ++o_hits;
      o_best = std::max(o_best, a);
      rule.take(g, w, d, !cont);
    }
    close();
  }
  *count = n;
  return n > cap ? SHZ_E_CAPACITY : SHZ_OK;
}

// plain: the shift, song frame - recording frame, is the segment's
struct sc_rule_shift {
  uint32_t step_frames;
  int64_t* seg_shift;
  int64_t o_shift = 0;
  int64_t shift(uint64_t w, int64_t d) const { return d - (int64_t)w * (int64_t)step_frames; }
  bool follows(uint64_t, uint64_t w, uint64_t, int64_t d) const { return shift(w, d) == o_shift; }
  void take(uint64_t, uint64_t w, int64_t d, bool first) {
    if (first) o_shift = shift(w, d);
  }
  void write(uint64_t n) const { seg_shift[n] = o_shift; }
};

extern "C" int32_t shz_scan_timeline(const uint64_t* win_off, uint32_t n_recs, const uint32_t* sid, const int32_t* delta,
                                     const uint32_t* aligned, const uint32_t* nres, uint32_t topn, uint32_t step_frames,
                                     uint32_t min_aligned, uint32_t max_gap, uint32_t* seg_rec, uint32_t* seg_sid, int64_t* seg_shift,
                                     uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best, uint64_t cap,
                                     uint64_t* count) {
  if (!count) return SHZ_E_INVALID;
  *count = 0;
  if (n_recs == 0) return SHZ_OK;
  if (!win_off || topn == 0) return SHZ_E_INVALID;
  if (!sc_win_off_ok(win_off, n_recs)) return SHZ_E_INVALID;
  if (win_off[n_recs] > win_off[0] && (!sid || !delta || !aligned || !nres)) return SHZ_E_INVALID;
  if (cap && (!seg_rec || !seg_sid || !seg_shift || !seg_first || !seg_last || !seg_hits || !seg_best)) return SHZ_E_INVALID;
  sc_rule_shift rule{step_frames, seg_shift};
  return sc_fold(win_off, n_recs, sid, delta, aligned, nres, topn, min_aligned, max_gap, seg_rec, seg_sid, seg_first, seg_last,
                 seg_hits, seg_best, cap, count, rule);
}

// ---- scan extents: frame-accurate start and end of every segment --------------------------------------
// Every segment of the timeline gets three ZONES of recording frames -- the whole play, its head and its tail, each with a
// margin -- and every zone is one query of the extent pass (shz_extent.hip) with the segment's identity as its one candidate.
// The zones' bounds, on the host: positions are formed in 64 bits and saturate far above every frame count (2^40), where
// only the clamp to the recording's frames is left of them.
extern "C" int32_t shz_scan_zones(const uint32_t* seg_rec, const uint32_t* seg_sid, const int64_t* seg_shift, const uint32_t* seg_first,
                                  const uint32_t* seg_last, uint64_t n_segs, const uint64_t* frames, uint32_t n_recs,
                                  uint32_t window_frames, uint32_t step_frames, uint32_t margin_frames, uint32_t* zone_lo,
                                  uint32_t* zone_hi) {
  if (window_frames == 0 || step_frames == 0) return SHZ_E_INVALID;
  if (n_recs && !frames) return SHZ_E_INVALID;
  for (uint32_t r = 0; r < n_recs; ++r)
    if (frames[r] > 0xFFFFFFFFull) return SHZ_E_INVALID;
  if (n_segs == 0) return SHZ_OK;
  if (!seg_rec || !seg_sid || !seg_shift || !seg_first || !seg_last || !zone_lo || !zone_hi) return SHZ_E_INVALID;
  for (uint64_t i = 0; i < n_segs; ++i) {
    if (seg_rec[i] >= n_recs || seg_first[i] > seg_last[i]) return SHZ_E_INVALID;
    if (i && (seg_rec[i] < seg_rec[i - 1] || (seg_rec[i] == seg_rec[i - 1] && seg_first[i] <= seg_last[i - 1]))) return SHZ_E_INVALID;
  }
  const uint64_t W = window_frames, M = margin_frames, top = 1ull << 40;
  auto at = [&](uint32_t w) { return std::min<uint64_t>((uint64_t)w * step_frames, top); };
  // the neighbours of the same identity inside a recording: windows ascend, so the nearest earlier one ends last and the
  // nearest later one begins first.  prev[i] / next[i]: their indices, or n_segs
  std::vector<uint64_t> prev((size_t)n_segs, n_segs), next((size_t)n_segs, n_segs);
  for (uint64_t r0 = 0; r0 < n_segs;) {
    uint64_t r1 = r0;
    while (r1 < n_segs && seg_rec[r1] == seg_rec[r0]) ++r1;
    std::vector<uint64_t> order;
    for (uint64_t i = r0; i < r1; ++i) order.push_back(i);
    std::stable_sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
      return seg_sid[a] != seg_sid[b] ? seg_sid[a] < seg_sid[b] : seg_shift[a] < seg_shift[b];
    });
    for (size_t j = 1; j < order.size(); ++j) {
      const uint64_t a = order[j - 1], b = order[j];
      if (seg_sid[a] == seg_sid[b] && seg_shift[a] == seg_shift[b]) {
        next[a] = b;
        prev[b] = a;
      }
    }
    r0 = r1;
  }
  for (uint64_t i = 0; i < n_segs; ++i) {
    const uint64_t F = frames[seg_rec[i]], a = at(seg_first[i]), b = at(seg_last[i]);
    uint64_t lo = a > M ? a - M : 0, hi = b + W + M;
    if (prev[i] != n_segs) lo = std::max(lo, std::min(at(seg_last[prev[i]]) + W, a));
    if (next[i] != n_segs) hi = std::min(hi, std::max(at(seg_first[next[i]]), b + W));
    const uint64_t zl[3] = {lo, lo, b}, zh[3] = {hi, a + W, hi};
    for (int z = 0; z < 3; ++z) {
      const uint64_t l = std::min(zl[z], F), h = std::min(zh[z], F);
      zone_lo[3 * i + z] = (uint32_t)l;
      zone_hi[3 * i + z] = (uint32_t)std::max(l, h);
    }
  }
  return SHZ_OK;
}

struct sc_zone {       // one zone of the zone stage; the entry behind the last one holds the total
  uint64_t item0;      // its first (zone, channel) item: the channels of the zones in front of it
  uint64_t seg0;       // channel c is segment seg0 + c of the hashes' CSR: the first clip of its recording (shz_scan_extents),
                       // the first job of its segment (shz_scan_plays)
  uint32_t lo, hi;     // frames [lo, hi) of the lists' t1: recording frames, or warped recording frames
  uint32_t nch, pad;
};

// per (zone, channel): where the zone's hashes begin in the channel's list, and how many they are.  Zones have arbitrary
// (recording, lo, hi): nothing here is derived from a window number.  (64-bit compares, as sc_bounds_kernel)
__global__ __launch_bounds__(SC_THREADS) void sc_zone_bounds_kernel(const sc_zone* __restrict__ zones, uint32_t nz, uint64_t n_items,
                                                                    const uint64_t* __restrict__ hoff, const uint32_t* __restrict__ t1,
                                                                    uint64_t* __restrict__ first, uint64_t* __restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= n_items) return;
  uint32_t l = 0, h = nz;   // the last zone whose first item is <= i (zones without a channel share a start with the next)
  while (l + 1 < h) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (zones[mid].item0 <= i) l = mid; else h = mid;
  }
  const sc_zone Z = zones[l];
  const uint64_t c = i - Z.item0;
  if (c >= Z.nch) {   // (never: the host builds item0 from nch)
    first[i] = 0;
    cnt[i] = 0;
    return;
  }
  const uint64_t a = hoff[Z.seg0 + c], b = hoff[Z.seg0 + c + 1];
  const uint64_t p = sc_lower_bound(t1, a, b, Z.lo);
  const uint64_t q = Z.hi > Z.lo ? sc_lower_bound(t1, p, b, Z.hi) : p;
  first[i] = p;
  cnt[i] = q - p;
}

// one workgroup per zone: its channels' ranges, one behind the other, to offs[item] of the columns (offs: exclusive scan of
// the counts, the total behind it): key32 and t1 - lo
__global__ __launch_bounds__(SC_THREADS) void sc_zone_gather_kernel(const sc_zone* __restrict__ zones, const uint64_t* __restrict__ first,
                                                                    const uint64_t* __restrict__ offs, uint64_t cap,
                                                                    const uint32_t* __restrict__ key, const uint32_t* __restrict__ t1,
                                                                    uint32_t* __restrict__ out_key, uint32_t* __restrict__ out_qo) {
  const sc_zone Z = zones[blockIdx.x];
  for (uint32_t c = 0; c < Z.nch; ++c) {
    const uint64_t p = Z.item0 + c;
    const uint64_t src = first[p], dst = offs[p], n = offs[p + 1] - offs[p];
    if (dst + n > cap) return;   // (uniform; the host sizes the columns from the same offsets, so this never holds)
    for (uint64_t i = threadIdx.x; i < n; i += SC_THREADS) {
      out_key[dst + i] = key[src + i];
      out_qo[dst + i] = t1[src + i] - Z.lo;
    }
  }
}

// The zone stage: cuts device-resident hash lists (d_key / d_t1, t1 never decreasing inside a list; hash_off, host, their CSR
// over n_csr lists) into the three zones of n_segs segments and leaves the zones' columns on the device, query_off (3 n_segs
// + 1, host) their CSR.  Zone z of segment i is [zone_lo[3 i + z], zone_hi[3 i + z]) of the lists seg_csr0[i] .. + seg_nch[i],
// one behind the other.  shz_scan_extents hands it the extraction's lists (alive in SHZ_WS_RQ_KEY / _T1; a segment's lists
// are its recording's clips, the borders recording frames); shz_scan_plays the warped lists of its jobs (SHZ_WS_SP_KEY / _T1;
// a segment's lists are its jobs, the borders warped).  It runs behind sc_windows, which returns with the stream idle and is
// done with its workspace, or in a call without a window stage: the slots SHZ_WS_SC_JOBS, _CTL, _KEY and _QO are REUSED here
// (descriptors | hash_off; first | count | offsets; the two columns) instead of adding slots that would only ever be live
// when those are dead.  The extent pass behind it reserves none of them.  The stream is idle on return.
static int32_t sc_zone_stage(shz_ctx* ctx, const char* who, const uint64_t* seg_csr0, const uint32_t* seg_nch, uint64_t n_segs,
                             uint64_t n_csr, const uint64_t* hash_off, const uint32_t* d_key, const uint32_t* d_t1,
                             const uint32_t* zone_lo, const uint32_t* zone_hi, uint64_t* query_off, const uint32_t** d_zk,
                             const uint32_t** d_zq) {
  const uint64_t nz = 3 * n_segs, total = hash_off[n_csr];
  const uint64_t zone_bytes = (nz + 1) * sizeof(sc_zone), hoff_bytes = (n_csr + 1) * 8;
  std::vector<char> block(zone_bytes + hoff_bytes);
  sc_zone* hz = (sc_zone*)block.data();
  uint64_t n_items = 0;
  for (uint64_t z = 0; z < nz; ++z) {
    hz[z] = sc_zone{n_items, seg_csr0[z / 3], zone_lo[z], zone_hi[z], seg_nch[z / 3], 0};
    n_items += seg_nch[z / 3];
  }
  hz[nz] = sc_zone{n_items, n_csr, 0, 0, 0, 0};
  memcpy(block.data() + zone_bytes, hash_off, hoff_bytes);
  void *d_blk, *d_ctl, *d_k, *d_q;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_JOBS, block.size(), &d_blk));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_CTL, (3 * n_items + 1) * 8, &d_ctl));
  uint64_t *d_first = (uint64_t*)d_ctl, *d_cnt = d_first + n_items, *d_offs = d_cnt + n_items;   // d_offs[n_items] = the total
  std::vector<uint64_t> offs((size_t)n_items + 1, 0);
  if (total && n_items) {   // (without hashes every zone is empty)
    SHZ_HIP(ctx, shz_memcpy(ctx, d_blk, block.data(), block.size(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sc_zone_bounds_kernel, dim3((unsigned)((n_items + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, ctx->stream,
                       (const sc_zone*)d_blk, (uint32_t)nz, n_items, (const uint64_t*)((char*)d_blk + zone_bytes), d_t1, d_first, d_cnt);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(shz_scan_u64(ctx, d_cnt, d_offs, n_items, d_offs + n_items));
    SHZ_HIP(ctx, shz_memcpy(ctx, offs.data(), d_offs, (n_items + 1) * 8, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  const uint64_t m = offs[n_items];
  if (m > total * nz)   // a hash lies at most once in a zone
    SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu zone entries from %llu hashes in %llu zones", who, (unsigned long long)m,
             (unsigned long long)total, (unsigned long long)nz);
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_KEY, m * 4 + 64, &d_k));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SC_QO, m * 4 + 64, &d_q));
  if (m) {
    hipLaunchKernelGGL(sc_zone_gather_kernel, dim3((unsigned)nz), dim3(SC_THREADS), 0, ctx->stream, (const sc_zone*)d_blk,
                       (const uint64_t*)d_first, (const uint64_t*)d_offs, m, d_key, d_t1, (uint32_t*)d_k, (uint32_t*)d_q);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  for (uint64_t z = 0; z <= nz; ++z) query_off[z] = offs[hz[z].item0];
  *d_zk = (const uint32_t*)d_k;
  *d_zq = (const uint32_t*)d_q;
  return SHZ_OK;
}

extern "C" int32_t shz_scan_extents(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                    const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                    uint32_t window_frames, uint32_t step_frames, uint32_t topn, uint32_t flags, uint32_t min_aligned,
                                    uint32_t max_gap, uint32_t margin_frames, uint32_t d_tol, uint64_t* win_off, uint32_t* out_sid,
                                    int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres,
                                    uint32_t* out_nhash, uint64_t* out_npairs, uint64_t cap_windows, uint64_t* count,
                                    uint32_t* seg_rec, uint32_t* seg_sid, int64_t* seg_shift, uint32_t* seg_first, uint32_t* seg_last,
                                    uint32_t* seg_hits, uint32_t* seg_best, uint64_t cap_segs, uint64_t* seg_count, uint32_t* zone_lo,
                                    uint32_t* zone_hi, uint32_t* zone_count, uint32_t* zone_q_first, uint32_t* zone_q_last,
                                    uint32_t* zone_t_first, uint32_t* zone_t_last, uint32_t* zone_shift, uint32_t* zone_hist,
                                    float* ms_extract, float* ms_window, float* ms_match, float* ms_extent) {
  const char* who = "shz_scan_extents";
  if (!ctx || !t) return SHZ_E_INVALID;
  if (ms_extent) *ms_extent = 0.f;
  if (seg_count) *seg_count = 0;
  // SHZ_SCAN_KEEP_MASK: the caller's keep mask arrives in out_nres, which the scan overwrites -- a copy of this call's own
  std::vector<uint8_t> keep;
  if ((flags & SHZ_SCAN_KEEP_MASK) && out_nres)
    for (uint64_t w = 0; w < cap_windows; ++w) keep.push_back(out_nres[w] != 0);
  const bool masked = (flags & SHZ_SCAN_KEEP_MASK) != 0;
  flags &= ~SHZ_SCAN_KEEP_MASK;
  const sc_plain P{pcm, clip_off, n_clips, rec_clip0, n_recs, fs, amp_min, fan_value, window_frames, step_frames, topn, flags, win_off,
                   out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, cap_windows, count, ms_extract,
                   ms_window, ms_match};
  // everything that can be refused is refused before the first launch: the plain scan's refusals, then this call's own
  bool done;
  SHZ_TRY(sc_plain_check(ctx, t, who, P, &done));
  if (d_tol > 31) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: d_tol must be in [0, 31], got %u", who, d_tol);
  if (margin_frames >= (1u << 20)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: margin_frames must be below 2^20, got %u", who, margin_frames);
  if (!seg_count) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: seg_count is NULL", who);
  if (cap_segs && (!seg_rec || !seg_sid || !seg_shift || !seg_first || !seg_last || !seg_hits || !seg_best))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL segment array", who);
  if (cap_segs && (!zone_lo || !zone_hi || !zone_count || !zone_q_first || !zone_q_last || !zone_t_first || !zone_t_last || !zone_shift))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL zone array", who);
  if (done) return SHZ_OK;   // no recording, or no window: no segment
  SHZ_TRY(ex_state(ctx, t, who, 1));
  SHZ_TRY(ex_table_limits(ctx, t, who));
  // 1) + 2) the plain scan; the extraction's columns stay where they are
  const bool timed = ms_extract || ms_window || ms_match || ms_extent;
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(sc_plain_run(ctx, t, who, P, timed, hash_off.data(), &d_key, &d_t1));
  if (masked)   // (the windows were counted: *count <= cap_windows = the mask's length)
    for (uint64_t w = 0; w < *count && w < keep.size(); ++w)
      if (!keep[w]) out_nres[w] = 0;
  // 3) the timeline, on the host
  const int32_t rc = shz_scan_timeline(win_off, n_recs, out_sid, out_delta, out_aligned, out_nres, topn, step_frames, min_aligned, max_gap,
                                       seg_rec, seg_sid, seg_shift, seg_first, seg_last, seg_hits, seg_best, cap_segs, seg_count);
  const uint64_t n_segs = *seg_count;
  if (rc == SHZ_E_CAPACITY)
    SHZ_FAIL(ctx, SHZ_E_CAPACITY, "%s: %llu segments, room for %llu", who, (unsigned long long)n_segs, (unsigned long long)cap_segs);
  if (rc != SHZ_OK) SHZ_FAIL(ctx, rc, "%s: the timeline refused the scan's own arrays", who);
  if (n_segs == 0) return SHZ_OK;
  if (3 * n_segs >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu segments in one call", who, (unsigned long long)n_segs);
  // 4) the zones and their candidates, on the host
  const uint64_t nz = 3 * n_segs;
  std::vector<uint64_t> frames((size_t)n_recs, 0);
  for (uint32_t r = 0; r < n_recs; ++r)
    for (uint32_t c = rec_clip0[r]; c < rec_clip0[r + 1]; ++c)
      frames[r] = std::max<uint64_t>(frames[r], shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop));
  std::vector<uint32_t> z_lo((size_t)nz), z_hi((size_t)nz), c_sid((size_t)nz), c_n((size_t)nz);
  std::vector<int32_t> c_dlo((size_t)nz), c_dhi((size_t)nz);
  if (shz_scan_zones(seg_rec, seg_sid, seg_shift, seg_first, seg_last, n_segs, frames.data(), n_recs, window_frames, step_frames,
                     margin_frames, z_lo.data(), z_hi.data()) != SHZ_OK)
    SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the zones refused the timeline's own segments", who);
  for (uint64_t z = 0; z < nz; ++z) {
    // off - (t1 - lo) = (off - t1) + lo, and off - t1 is the shift.  Every difference of a table offset < 2^31 and a query
    // offset < 2^20 fits 32 bits: a range that does not meet them holds no pair, the others lose nothing at the clamp
    const int64_t d = seg_shift[z / 3] + (int64_t)z_lo[z], lo = d - (int64_t)d_tol, hi = d + (int64_t)d_tol;
    const bool none = lo > INT32_MAX || hi < INT32_MIN;
    c_sid[z] = seg_sid[z / 3];
    c_dlo[z] = none ? 0 : (int32_t)std::max<int64_t>(lo, INT32_MIN);
    c_dhi[z] = none ? 0 : (int32_t)std::min<int64_t>(hi, INT32_MAX);
    c_n[z] = none ? 0u : 1u;
  }
  // 5) the zone stage, 6) the extent pass on its columns.  (events 2 and 3 are free again: the window stage is over)
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[2], ctx->stream));
  std::vector<uint64_t> query_off((size_t)nz + 1, 0);
  const uint32_t *d_zk = nullptr, *d_zq = nullptr;
  std::vector<uint64_t> seg_csr0((size_t)n_segs);   // a segment's lists: the clips of its recording
  std::vector<uint32_t> seg_nch((size_t)n_segs);
  for (uint64_t i = 0; i < n_segs; ++i) {
    seg_csr0[i] = rec_clip0[seg_rec[i]];
    seg_nch[i] = rec_clip0[seg_rec[i] + 1] - rec_clip0[seg_rec[i]];
  }
  SHZ_TRY(sc_zone_stage(ctx, who, seg_csr0.data(), seg_nch.data(), n_segs, n_clips, hash_off.data(), d_key, d_t1, z_lo.data(),
                        z_hi.data(), query_off.data(), &d_zk, &d_zq));
  const ex_args A{(uint32_t)nz, 1, c_sid.data(), c_dlo.data(), c_dhi.data(), c_n.data(), zone_count, zone_q_first, zone_q_last,
                  zone_t_first, zone_t_last, zone_hist, zone_shift};
  SHZ_TRY(ex_check(ctx, t, who, A));
  const int32_t rx = ex_device(ctx, t, who, d_zk, d_zq, query_off.data(), A);
  if (rx != SHZ_OK) {
    (void)hipStreamSynchronize(ctx->stream);   // (a refused pass may have queued work that reads the columns)
    return rx;
  }
  if (timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[3], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->sc_ev[3]));
    if (ms_extent) SHZ_HIP(ctx, hipEventElapsedTime(ms_extent, ctx->sc_ev[2], ctx->sc_ev[3]));
  }
  // the pass has written its outputs: the zones beside them, query frames -> recording frames
  for (uint64_t z = 0; z < nz; ++z) {
    zone_lo[z] = z_lo[z];
    zone_hi[z] = z_hi[z];
    if (zone_count[z]) {
      zone_q_first[z] += z_lo[z];
      zone_q_last[z] += z_lo[z];
    }
  }
  return SHZ_OK;
}

// ---- scanning at an unknown speed, or at unknown tempo and pitch -------------------------------
// The peaks of every recording are extracted once and warped for every variant of a list (shz_speed.hip); the warped hash
// list of (recording, warp, channel) has non-decreasing t1', so it goes through the window stage as it is.  Work goes in
// slices of (whole recordings x a contiguous chunk of warps): a warp pass and one call of the stage each.  Only the time
// factor of a warp enters a time: the window borders, the query offsets and the bias bound.  With a selection every window
// tries its own sub-list; warps that no window tries are dropped first, and a slice hands the stage the slots of its chunk.
static uint32_t sc_warp_dist(uint32_t t16, uint32_t f16) {
  auto off = [](uint32_t s) { return s > SP_S_ONE ? s - SP_S_ONE : SP_S_ONE - s; };
  return off(t16) + off(f16);
}

// The one driver of both entry points.  who, n_name, t_name, f_name: the caller's own names for the call, the list's length
// and its two tables in everything that is refused.
static int32_t sc_scan_warps(shz_ctx* ctx, shz_table* t, const char* who, const char* n_name, const char* t_name, const char* f_name,
                             const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* rec_clip0,
                             uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value, uint32_t window_frames,
                             uint32_t step_frames, uint32_t topn, const uint32_t* tempo_q16, const uint32_t* pitch_q16,
                             uint32_t n_warps, const uint64_t* sel_off, const uint32_t* sel_warp, uint32_t flags, uint64_t* win_off,
                             uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                             uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs, uint32_t* out_profile,
                             uint64_t* out_work, uint64_t cap_windows, uint64_t* count, float* ms_extract, float* ms_warp,
                             float* ms_window, float* ms_match) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (ms_extract) *ms_extract = 0.f;
  if (ms_warp) *ms_warp = 0.f;
  if (ms_window) *ms_window = 0.f;
  if (ms_match) *ms_match = 0.f;
  if (count) *count = 0;
  if (out_work) out_work[0] = out_work[1] = 0;
  // everything that can be refused is refused before the first launch
  SHZ_TRY(sc_check(ctx, who, flags, win_off, count, window_frames, step_frames));
  SHZ_TRY(sp_check_ladder(ctx, who, n_name, t_name, tempo_q16, f_name, pitch_q16, n_warps, fan_value));
  if ((sel_off == nullptr) != (sel_warp == nullptr))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: sel_off and sel_warp go together; one of them is NULL", who);
  const bool sel = sel_off != nullptr;
  const uint32_t s_max = *std::max_element(tempo_q16, tempo_q16 + n_warps);   // (time alone: pitch_q16 never enters a time)
  // no window is longer at any warp: W_v(s + window) - W_v(s) <= ceil(window t16 / 65536)
  const uint64_t len_max = ((uint64_t)window_frames * s_max + 65535) >> 16;
  if (len_max >= (1ull << 20))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: a window of %u frames at time factor %u / 65536 is %llu frames long; query offsets must be < 2^20",
             who, window_frames, s_max, (unsigned long long)len_max);
  SHZ_TRY(sc_check_recs(ctx, who, clip_off, n_clips, rec_clip0, n_recs, win_off));
  if (n_recs == 0) return SHZ_OK;
  if (fs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "Fs must be > 0");
  if (n_clips && !pcm && clip_off[n_clips] > clip_off[0]) SHZ_FAIL(ctx, SHZ_E_INVALID, "pcm is NULL");
  SHZ_TRY(shz_match_ready(ctx, t, topn));
  uint64_t frames = 0;
  SHZ_TRY(sc_count_windows(ctx, who, clip_off, rec_clip0, n_recs, window_frames, step_frames, cap_windows, win_off, count, &frames));
  const uint64_t n_wins = *count;
  if (n_wins == 0) return SHZ_OK;
  if (!out_best || !out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL buffer", who);
  // the selection: a CSR over the windows, every list strictly ascending and inside the warps.  used[v]: a window tries v
  std::vector<uint32_t> c_t16, c_f16, c_of, c_index;   // the warps in use (compacted), their old indices, old -> new
  if (sel) {
    if (sel_off[0] != 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: sel_off[0] is %llu, not 0", who, (unsigned long long)sel_off[0]);
    for (uint64_t w = 0; w < n_wins; ++w)
      if (sel_off[w + 1] < sel_off[w]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: sel_off decreases at window %llu", who, (unsigned long long)w);
    std::vector<uint8_t> used(n_warps, 0);
    for (uint64_t w = 0; w < n_wins; ++w)
      for (uint64_t j = sel_off[w]; j < sel_off[w + 1]; ++j) {
        if (sel_warp[j] >= n_warps)
          SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: slot %llu of window %llu is warp %u of %u", who, (unsigned long long)(j - sel_off[w]),
                   (unsigned long long)w, sel_warp[j], n_warps);
        if (j > sel_off[w] && sel_warp[j] <= sel_warp[j - 1])
          SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: the list of window %llu is not strictly ascending at slot %llu", who, (unsigned long long)w,
                   (unsigned long long)(j - sel_off[w]));
        used[sel_warp[j]] = 1;
      }
    c_index.assign(n_warps, 0);
    for (uint32_t v = 0; v < n_warps; ++v)
      if (used[v]) {
        c_index[v] = (uint32_t)c_of.size();
        c_of.push_back(v);
        c_t16.push_back(tempo_q16[v]);
        c_f16.push_back(pitch_q16[v]);
      }
    // windows without a slot keep this: no results, no variant
    memset(out_sid, 0, n_wins * topn * 4); memset(out_delta, 0, n_wins * topn * 4); memset(out_aligned, 0, n_wins * topn * 4);
    memset(out_dedup, 0, n_wins * topn * 4); memset(out_nres, 0, n_wins * 4);
    if (out_nhash) memset(out_nhash, 0, n_wins * 4);
    if (out_npairs) memset(out_npairs, 0, n_wins * 8);
    if (out_profile) memset(out_profile, 0, sel_off[n_wins] * 4);
    if (c_of.empty()) {   // nothing is selected: nothing is extracted
      for (uint64_t w = 0; w < n_wins; ++w) out_best[w] = SHZ_SCAN_NO_WARP;
      return SHZ_OK;
    }
  }
  const uint32_t K = sel ? (uint32_t)c_of.size() : n_warps;   // from here on: the compacted list
  const uint32_t* k_t16 = sel ? c_t16.data() : tempo_q16;
  const uint32_t* k_f16 = sel ? c_f16.data() : (pitch_q16 == tempo_q16 ? k_t16 : pitch_q16);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = ms_extract || ms_warp || ms_window || ms_match;
  if (timed) {
    for (hipEvent_t& e : ctx->sc_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[0], ctx->stream));
  }
  // 1) the peaks of every clip, once, into the library's own buffers
  std::vector<uint64_t> peak_off((size_t)n_clips + 1, 0);
  const uint16_t* d_pf = nullptr;
  const uint32_t* d_pt = nullptr;
  SHZ_TRY(sp_peaks_owned(ctx, who, pcm, clip_off, n_clips, frames, fs, amp_min, flags & SHZ_PCM_DEVICE, peak_off.data(), &d_pf, &d_pt));
  if (timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[1], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->sc_ev[1]));
    if (ms_extract) SHZ_HIP(ctx, hipEventElapsedTime(ms_extract, ctx->sc_ev[0], ctx->sc_ev[1]));
  }
  const uint64_t* d_poff;
  const uint32_t *d_tempo, *d_pitch;   // (a speed ladder: one table for time and frequency)
  SHZ_TRY(sp_upload_tables(ctx, peak_off.data(), n_clips, k_t16, k_f16, K, &d_poff, &d_tempo, &d_pitch));
  // 2) slices of whole recordings x a chunk of warps: the entries a slice's warp can yield at most (every peak with all its
  // partners, at every warp of the chunk) stay within the match's pair budget and 1/8 of the workspace limit.  The list
  // is cut only where one recording at all warps is beyond that; one (recording, warp) beyond it is a slice of its own
  const bool small = (ctx->debug & SHZ_DEBUG_SCAN_SPEED_SMALL_SLICES) != 0;
  const uint64_t per_item = std::max<uint32_t>(fan_value - 1, 1);
  const uint64_t warp_entries = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 64, 1), 1ull << 28);
  std::vector<uint32_t> best_top1((size_t)n_wins, 0);
  for (uint64_t w = 0; w < n_wins; ++w) out_best[w] = SHZ_SCAN_NO_WARP;   // (no variant tried yet)
  std::vector<uint32_t> v_sid, v_aligned, v_dedup, v_nres, v_nhash, s_warp;
  std::vector<int32_t> v_delta;
  std::vector<uint64_t> v_npairs, ho, s_off, s_first;
  uint64_t work_hashes = 0, work_entries = 0;
  float warp_ms = 0.f, win_ms = 0.f, match_ms = 0.f;
  for (uint32_t r0 = 0; r0 < n_recs;) {
    uint32_t nr = 1, kc = K;
    const uint64_t one = sp_items(peak_off.data(), rec_clip0, r0, 1, 1) * per_item;   // one warp of the first recording
    if (one * K > warp_entries) kc = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(warp_entries / std::max<uint64_t>(one, 1), 1), K);
    if (small) kc = std::min(kc, SS_SMALL_RUNGS);
    if (kc == K && !small)
      while (r0 + nr < n_recs && sp_items(peak_off.data(), rec_clip0, r0, nr + 1, K) * per_item <= warp_entries &&
             (win_off[r0 + nr + 1] - win_off[r0]) * K <= (1ull << 24))
        ++nr;
    const uint64_t nws = win_off[r0 + nr] - win_off[r0];   // windows of the slice
    if (nws == 0) {
      r0 += nr;
      continue;
    }
    for (uint32_t v0 = 0; v0 < K; v0 += kc) {
      const uint32_t kcc = std::min(kc, K - v0);
      // 2a) the warp of the slice: hashes of (recording, warp, channel), the exact CSR on both sides (events 0 and 1 are
      // free again: the window stage keeps to the others)
      if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[0], ctx->stream));
      const uint64_t n_seg = (uint64_t)(rec_clip0[r0 + nr] - rec_clip0[r0]) * kcc;
      ho.assign((size_t)n_seg + 1, 0);
      sp_pass P;
      SHZ_TRY(sp_count(ctx, d_pf, d_pt, d_poff, peak_off.data(), rec_clip0, r0, nr, d_tempo + v0, d_pitch + v0, kcc, fan_value, &P, ho.data()));
      const uint64_t total = ho[n_seg];
      work_hashes += total;
      void *d_key, *d_t1;
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_KEY, total * 4 + 64, &d_key));
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_T1, total * 4 + 64, &d_t1));
      if (total) SHZ_TRY(sp_write(ctx, P, (uint32_t*)d_key, (uint32_t*)d_t1, total));
      if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[1], ctx->stream));
      // the slots of the chunk: the part [v0, v0 + kcc) of every window's list (ascending, so one range of it), as indices
      // into the chunk.  s_first[w]: where that range begins in the call's sel_warp
      uint64_t nvq = nws * kcc;
      if (sel) {
        s_off.assign((size_t)nws + 1, 0);
        s_first.assign((size_t)nws, 0);
        s_warp.clear();
        for (uint64_t w = 0; w < nws; ++w) {
          const uint64_t gw = win_off[r0] + w;
          uint64_t j = sel_off[gw];
          while (j < sel_off[gw + 1] && c_index[sel_warp[j]] < v0) ++j;
          s_first[w] = j;
          for (; j < sel_off[gw + 1] && c_index[sel_warp[j]] < v0 + kcc; ++j) s_warp.push_back(c_index[sel_warp[j]] - v0);
          s_off[w + 1] = s_warp.size();
        }
        nvq = s_warp.size();
      }
      // 2b) + 2c) the window stage on the warped lists.  A hash lies in at most ceil(window / step) windows, +1 where the
      // warp's rounding moves a border; no query offset reaches len_max.  (A pass without hashes has no CSR on the device)
      v_sid.assign(nvq * topn, 0); v_aligned.assign(nvq * topn, 0); v_dedup.assign(nvq * topn, 0); v_delta.assign(nvq * topn, 0);
      v_nres.assign(nvq, 0); v_nhash.assign(nvq, 0); v_npairs.assign(nvq, 0);
      sc_slice S{rec_clip0 + r0, win_off + r0, nr, kcc, d_tempo + v0, total ? (const uint64_t*)P.d_hoff : nullptr, false,
                 (const uint32_t*)d_key, (const uint32_t*)d_t1, total, window_frames, step_frames, topn, flags & SHZ_MATCH_FULL_SORT,
                 (int64_t)len_max - 1, ((uint64_t)window_frames + step_frames - 1) / step_frames + 1, small, v_sid.data(),
                 v_aligned.data(), v_dedup.data(), v_nres.data(), v_nhash.data(), v_delta.data(), v_npairs.data(),
                 sel ? s_off.data() : nullptr, sel ? s_warp.data() : nullptr, &work_entries};
      SHZ_TRY(sc_windows(ctx, t, who, S, timed, &win_ms, &match_ms));
      if (timed) {
        float a = 0.f;
        SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->sc_ev[0], ctx->sc_ev[1]));
        warp_ms += a;
      }
      // 2d) the best variant of every window, folded over the chunks (sp_best's rule: variants come in index order)
      for (uint64_t w = 0; w < nws; ++w) {
        const uint64_t gw = win_off[r0] + w, q0 = sel ? s_off[w] : w * kcc, nq = sel ? s_off[w + 1] - s_off[w] : kcc;
        for (uint64_t j = 0; j < nq; ++j) {
          const uint64_t src = q0 + j;
          const uint32_t cv = v0 + (sel ? s_warp[src] : (uint32_t)j), gv = sel ? c_of[cv] : cv;   // compacted / the caller's index
          const uint32_t top1 = v_nres[src] ? v_aligned[src * topn] : 0u;
          if (out_profile) out_profile[sel ? s_first[w] + j : gw * K + gv] = top1;
          if (out_best[gw] != SHZ_SCAN_NO_WARP &&
              !(top1 > best_top1[gw] || (top1 == best_top1[gw] && sc_warp_dist(tempo_q16[gv], pitch_q16[gv]) <
                                                                      sc_warp_dist(tempo_q16[out_best[gw]], pitch_q16[out_best[gw]]))))
            continue;
          best_top1[gw] = top1;
          out_best[gw] = gv;
          memcpy(out_sid + gw * topn, v_sid.data() + src * topn, (size_t)topn * 4);
          memcpy(out_delta + gw * topn, v_delta.data() + src * topn, (size_t)topn * 4);
          memcpy(out_aligned + gw * topn, v_aligned.data() + src * topn, (size_t)topn * 4);
          memcpy(out_dedup + gw * topn, v_dedup.data() + src * topn, (size_t)topn * 4);
          out_nres[gw] = v_nres[src];
          if (out_nhash) out_nhash[gw] = v_nhash[src];
          if (out_npairs) out_npairs[gw] = v_npairs[src];
        }
      }
    }
    r0 += nr;
  }
  if (out_work) {
    out_work[0] = work_hashes;
    out_work[1] = work_entries;
  }
  if (ms_warp) *ms_warp = warp_ms;
  if (ms_window) *ms_window = win_ms;
  if (ms_match) *ms_match = match_ms;
  return SHZ_OK;
}

extern "C" int32_t shz_scan_warps(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                  const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                  uint32_t window_frames, uint32_t step_frames, uint32_t topn, const uint32_t* tempo_q16,
                                  const uint32_t* pitch_q16, uint32_t n_warps, const uint64_t* sel_off, const uint32_t* sel_warp,
                                  uint32_t flags, uint64_t* win_off, uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta,
                                  uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                                  uint64_t* out_npairs, uint32_t* out_profile, uint64_t* out_work, uint64_t cap_windows,
                                  uint64_t* count, float* ms_extract, float* ms_warp, float* ms_window, float* ms_match) {
  return sc_scan_warps(ctx, t, "shz_scan_warps", "n_warps", "tempo", "pitch", pcm, clip_off, n_clips, rec_clip0, n_recs, fs, amp_min,
                       fan_value, window_frames, step_frames, topn, tempo_q16, pitch_q16, n_warps, sel_off, sel_warp, flags, win_off,
                       out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, out_profile, out_work,
                       cap_windows, count, ms_extract, ms_warp, ms_window, ms_match);
}

// the speed ladder: one table for time and frequency, no selection (its own names in whatever is refused)
extern "C" int32_t shz_scan_speeds(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                   const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                   uint32_t window_frames, uint32_t step_frames, uint32_t topn, const uint32_t* speed_q16,
                                   uint32_t n_speeds, uint32_t flags, uint64_t* win_off, uint32_t* out_best, uint32_t* out_sid,
                                   int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres,
                                   uint32_t* out_nhash, uint64_t* out_npairs, uint32_t* out_profile, uint64_t cap_windows,
                                   uint64_t* count, float* ms_extract, float* ms_warp, float* ms_window, float* ms_match) {
  return sc_scan_warps(ctx, t, "shz_scan_speeds", "n_speeds", "speed", "speed", pcm, clip_off, n_clips, rec_clip0, n_recs, fs, amp_min,
                       fan_value, window_frames, step_frames, topn, speed_q16, speed_q16, n_speeds, nullptr, nullptr, flags, win_off,
                       out_best, out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, out_profile, nullptr,
                       cap_windows, count, ms_extract, ms_warp, ms_window, ms_match);
}

// The song's advance between the starts of two hit windows `gap` windows apart, W_t16(gap step) = (gap step t16 + 32768) >> 16,
// exact: gap and step are below 2^32 each and t16 at most 2^17, so the product needs 81 bits.  Positions are int32, so an
// advance of 2^40 or more fails every shift_tol as the exact value would; the result is clamped there.
static int64_t sc_advance(uint64_t gap, uint32_t step_frames, uint32_t t16) {
  const unsigned __int128 adv = ((unsigned __int128)gap * step_frames * t16 + 32768u) >> 16;
  const uint64_t top = 1ull << 40;
  return (int64_t)(adv > top ? top : (uint64_t)adv);
}

// A scan over variants: delta - w step is not constant when the recording plays at another tempo than the table's copy, so
// continuity is judged between neighbouring hits -- their variants at most rung_tol list places and tempo_tol / pitch_tol in the
// factors apart (~0u: that distance does not count), and the song's position advanced by what the hit's time factor says, within
// shift_tol.  The segment reports its first and last position and the variant most of its hits chose (sp_best on the histogram).
struct sc_rule_variant {
  const uint32_t *best, *tempo_q16, *pitch_q16;
  uint32_t n_variants, step_frames, rung_tol, tempo_tol, pitch_tol, shift_tol;
  int32_t *seg_pos_first, *seg_pos_last;
  uint32_t* seg_variant;
  std::vector<uint32_t> chosen;   // how often the open segment's hits chose every variant
  uint32_t o_v = 0;
  int64_t o_pos_first = 0, o_pos_last = 0;
  static uint32_t apart(uint32_t a, uint32_t b) { return a > b ? a - b : b - a; }
  bool follows(uint64_t g, uint64_t, uint64_t gap, int64_t pos) const {
    const uint32_t v = best[g];
    if (apart(v, o_v) > rung_tol || apart(tempo_q16[v], tempo_q16[o_v]) > tempo_tol || apart(pitch_q16[v], pitch_q16[o_v]) > pitch_tol)
      return false;
    // the song advances W_t16(gap step) frames between the two windows' starts
    const int64_t off = pos - o_pos_last - sc_advance(gap, step_frames, tempo_q16[v]);
    return (off < 0 ? -off : off) <= (int64_t)shift_tol;
  }
  void take(uint64_t g, uint64_t, int64_t pos, bool first) {
    if (first) {
      o_pos_first = pos;
      std::fill(chosen.begin(), chosen.end(), 0u);
    }
    o_pos_last = pos;
    o_v = best[g];
    ++chosen[o_v];
  }
  void write(uint64_t n) const {
    seg_pos_first[n] = (int32_t)o_pos_first;
    seg_pos_last[n] = (int32_t)o_pos_last;
    seg_variant[n] = sp_best(chosen.data(), tempo_q16, pitch_q16, n_variants);
  }
};

// The timeline of a speed-tolerant scan: one sorted ladder, neighbouring hits at most rung_tol rungs apart.
extern "C" int32_t shz_scan_timeline_speeds(const uint64_t* win_off, uint32_t n_recs, const uint32_t* sid, const int32_t* delta,
                                            const uint32_t* aligned, const uint32_t* nres, const uint32_t* best, uint32_t topn,
                                            uint32_t step_frames, const uint32_t* speed_q16, uint32_t n_speeds,
                                            uint32_t min_aligned, uint32_t max_gap, uint32_t rung_tol, uint32_t shift_tol,
                                            uint32_t* seg_rec, uint32_t* seg_sid, uint32_t* seg_first, uint32_t* seg_last,
                                            uint32_t* seg_hits, uint32_t* seg_best, int32_t* seg_pos_first, int32_t* seg_pos_last,
                                            uint32_t* seg_rung, uint64_t cap, uint64_t* count) {
  if (!count) return SHZ_E_INVALID;
  *count = 0;
  if (n_recs == 0) return SHZ_OK;
  if (!win_off || topn == 0 || !speed_q16 || n_speeds == 0 || n_speeds > SP_MAX_SPEEDS) return SHZ_E_INVALID;
  if (!sc_factors_ok(speed_q16, n_speeds)) return SHZ_E_INVALID;
  if (!sc_win_off_ok(win_off, n_recs)) return SHZ_E_INVALID;
  if (win_off[n_recs] > win_off[0] && (!sid || !delta || !aligned || !nres || !best)) return SHZ_E_INVALID;
  if (cap && (!seg_rec || !seg_sid || !seg_first || !seg_last || !seg_hits || !seg_best || !seg_pos_first || !seg_pos_last || !seg_rung))
    return SHZ_E_INVALID;
  for (uint64_t g = win_off[0]; g < win_off[n_recs]; ++g)
    if (best[g] >= n_speeds) return SHZ_E_INVALID;
  sc_rule_variant rule{best, speed_q16, speed_q16, n_speeds, step_frames, rung_tol, ~0u, ~0u, shift_tol, seg_pos_first, seg_pos_last,
                       seg_rung, std::vector<uint32_t>(n_speeds, 0)};
  return sc_fold(win_off, n_recs, sid, delta, aligned, nres, topn, min_aligned, max_gap, seg_rec, seg_sid, seg_first, seg_last,
                 seg_hits, seg_best, cap, count, rule);
}

// The timeline of a scan over warps: a tolerance for each factor in place of the rung distance, so the list need not be sorted
// (and may be longer than one call's ladder).  best is read for hits only.
extern "C" int32_t shz_scan_timeline_warps(const uint64_t* win_off, uint32_t n_recs, const uint32_t* sid, const int32_t* delta,
                                           const uint32_t* aligned, const uint32_t* nres, const uint32_t* best, uint32_t topn,
                                           uint32_t step_frames, const uint32_t* tempo_q16, const uint32_t* pitch_q16,
                                           uint32_t n_warps, uint32_t min_aligned, uint32_t max_gap, uint32_t tempo_tol_q16,
                                           uint32_t pitch_tol_q16, uint32_t shift_tol, uint32_t* seg_rec, uint32_t* seg_sid,
                                           uint32_t* seg_first, uint32_t* seg_last, uint32_t* seg_hits, uint32_t* seg_best,
                                           int32_t* seg_pos_first, int32_t* seg_pos_last, uint32_t* seg_warp, uint64_t cap,
                                           uint64_t* count) {
  if (!count) return SHZ_E_INVALID;
  *count = 0;
  if (n_recs == 0) return SHZ_OK;
  if (!win_off || topn == 0 || !tempo_q16 || !pitch_q16 || n_warps == 0) return SHZ_E_INVALID;
  if (!sc_factors_ok(tempo_q16, n_warps) || !sc_factors_ok(pitch_q16, n_warps)) return SHZ_E_INVALID;
  if (!sc_win_off_ok(win_off, n_recs)) return SHZ_E_INVALID;
  if (win_off[n_recs] > win_off[0] && (!sid || !delta || !aligned || !nres || !best)) return SHZ_E_INVALID;
  if (cap && (!seg_rec || !seg_sid || !seg_first || !seg_last || !seg_hits || !seg_best || !seg_pos_first || !seg_pos_last || !seg_warp))
    return SHZ_E_INVALID;
  for (uint64_t g = win_off[0]; g < win_off[n_recs]; ++g)
    if (sc_hit(aligned, nres, topn, min_aligned, g) && best[g] >= n_warps) return SHZ_E_INVALID;
  sc_rule_variant rule{best, tempo_q16, pitch_q16, n_warps, step_frames, ~0u, tempo_tol_q16, pitch_tol_q16, shift_tol, seg_pos_first,
                       seg_pos_last, seg_warp, std::vector<uint32_t>(n_warps, 0)};
  return sc_fold(win_off, n_recs, sid, delta, aligned, nres, topn, min_aligned, max_gap, seg_rec, seg_sid, seg_first, seg_last,
                 seg_hits, seg_best, cap, count, rule);
}

// ---- warped scan extents: frame-accurate play bounds and a tempo fit for the segments of a warped scan ----
// A segment of shz_scan_timeline_speeds / _warps has no constant shift, so its zones are clamped by (rec, sid) alone --
// shz_scan_zones with every shift 0 -- and every zone gets a WIDENED candidate: the drift line of a play that really runs
// at a tempo beside its rung leaves the rung's own offset bin by (true / rung - 1) frames per warped frame.  With W(x) =
// (x t16 + 32768) >> 16, p_a / p_b the song frames at the starts of the first / last window (a S, b S) and the zone's warped
// start W(lo), the offset difference off - (t1' - W(lo)) is c_a = p_a - W(a S) + W(lo) at the first window and c_b = p_b -
// W(b S) + W(lo) at the last one.  Positions are formed in 64 bits; a S saturates at 2^40 as shz_scan_zones' do, where c is
// below every int32 whatever the rest is.
extern "C" int32_t shz_scan_play_zones(const uint32_t* seg_rec, const uint32_t* seg_sid, const uint32_t* seg_first,
                                       const uint32_t* seg_last, const int32_t* seg_pos_first, const int32_t* seg_pos_last,
                                       const uint32_t* seg_t16, uint64_t n_segs, const uint64_t* frames, uint32_t n_recs,
                                       uint32_t window_frames, uint32_t step_frames, uint32_t margin_frames, uint32_t w,
                                       uint32_t* zone_lo, uint32_t* zone_hi, uint64_t* zone_wlo, uint64_t* zone_whi,
                                       int32_t* zone_d_lo, int32_t* zone_d_hi, uint32_t* cand_n) {
  const uint64_t nz = 3 * n_segs;
  std::vector<int64_t> shift((size_t)n_segs, 0);
  std::vector<uint32_t> lo((size_t)nz), hi((size_t)nz), cn((size_t)nz);
  // 1) the own-frame zones, and everything shz_scan_zones refuses
  const int32_t rc = shz_scan_zones(seg_rec, seg_sid, shift.data(), seg_first, seg_last, n_segs, frames, n_recs, window_frames,
                                    step_frames, margin_frames, lo.data(), hi.data());
  if (rc != SHZ_OK) return rc;
  if (n_segs == 0) return SHZ_OK;
  if (!seg_pos_first || !seg_pos_last || !seg_t16 || !zone_lo || !zone_hi || !zone_wlo || !zone_whi || !zone_d_lo || !zone_d_hi || !cand_n)
    return SHZ_E_INVALID;
  // 2) the factors, 3) the warped zones and their lengths, 4) the candidates and their widths
  for (uint64_t i = 0; i < n_segs; ++i)
    if (seg_t16[i] < SP_S_MIN || seg_t16[i] > SP_S_MAX) return SHZ_E_INVALID;
  auto warp = [](uint64_t x, uint32_t t16) { return (x * t16 + 32768u) >> 16; };   // (x <= 2^40, t16 <= 2^17)
  std::vector<uint64_t> wlo((size_t)nz), whi((size_t)nz);
  for (uint64_t z = 0; z < nz; ++z) {
    wlo[z] = warp(lo[z], seg_t16[z / 3]);
    whi[z] = warp(hi[z], seg_t16[z / 3]);
    if (whi[z] - wlo[z] >= (1ull << 20)) return SHZ_E_UNSUPPORTED;   // (a query offset of the extent pass)
  }
  std::vector<int32_t> dlo((size_t)nz), dhi((size_t)nz);
  const uint64_t top = 1ull << 40;
  for (uint64_t i = 0; i < n_segs; ++i) {
    const uint32_t t16 = seg_t16[i];
    const int64_t wa = (int64_t)warp(std::min<uint64_t>((uint64_t)seg_first[i] * step_frames, top), t16);
    const int64_t wb = (int64_t)warp(std::min<uint64_t>((uint64_t)seg_last[i] * step_frames, top), t16);
    for (int z = 0; z < 3; ++z) {
      const uint64_t k = 3 * i + z;
      const int64_t c_a = (int64_t)seg_pos_first[i] - wa + (int64_t)wlo[k], c_b = (int64_t)seg_pos_last[i] - wb + (int64_t)wlo[k];
      // whole: the drift line runs from one end to the other; head: where it starts; tail: where it ends
      const int64_t c_lo = z == 0 ? std::min(c_a, c_b) : (z == 1 ? c_a : c_b), c_hi = z == 0 ? std::max(c_a, c_b) : c_lo;
      const int64_t l = c_lo - (int64_t)w, h = c_hi + (int64_t)w;
      // (as shz_scan_extents: a range that does not meet the differences a table offset < 2^31 and a query offset < 2^20
      // can have holds no pair; the others lose nothing at the clamp)
      const bool none = l > INT32_MAX || h < INT32_MIN;
      dlo[k] = none ? 0 : (int32_t)std::max<int64_t>(l, INT32_MIN);
      dhi[k] = none ? 0 : (int32_t)std::min<int64_t>(h, INT32_MAX);
      cn[k] = none ? 0u : 1u;
      if (!none && (int64_t)dhi[k] - dlo[k] >= EX_FIT_MAX_WIDTH) return SHZ_E_UNSUPPORTED;   // (the moments: q u < 2^32)
    }
  }
  for (uint64_t z = 0; z < nz; ++z) {
    zone_lo[z] = lo[z];
    zone_hi[z] = hi[z];
    zone_wlo[z] = wlo[z];
    zone_whi[z] = whi[z];
    zone_d_lo[z] = dlo[z];
    zone_d_hi[z] = dhi[z];
    cand_n[z] = cn[z];
  }
  return SHZ_OK;
}

// The device stage.  Why a job's hashes are the full list's: a job is (segment, channel) and keeps the channel's peaks whose
// WARPED time lies in [W(lo0), W(hi0) - 1 + SHZ_MAX_DT], zone 0 being [lo0, hi0).  (1) Choosing by warped time keeps whole t'
// groups: every peak that shares a t' with a kept one is kept, so sp_place's merge of neighbouring frames (t16 < 65536) sees
// the peaks it sees on the whole channel, and the kept peaks stand in the order they have in the full warped list.  (2) An
// anchor with t1' < W(hi0) pairs with the next fan - 1 peaks of that order whose dt' <= SHZ_MAX_DT: all of them have t' <=
// W(hi0) - 1 + SHZ_MAX_DT and are kept, and a peak that is missing behind the range would have failed dt' <= SHZ_MAX_DT.  So
// the job's hashes with W(lo0) <= t1' < W(hi0) are the full list's, entry for entry, and the three zones -- which lie inside
// zone 0 -- are cut from them; anchors in the tail behind W(hi0) have lost partners and are never cut.
// tests/scan_play_twin.py cuts the full list; its equality with this call is the proof in practice.
// Workspace: the peaks in SHZ_WS_SP_PF / _PT, the job table in SHZ_WS_SP_Q, the pass in SHZ_WS_SP_A .. _SEG, the warped hashes
// in SHZ_WS_SP_KEY / _T1 -- all as the warped scan uses them; the zone stage REUSES SHZ_WS_SC_JOBS / _CTL / _KEY / _QO, whose
// owner (the window stage) does not run in this call; the extent pass keeps to its own.  No slot is added.
extern "C" int32_t shz_scan_plays(shz_ctx* ctx, shz_table* t, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                  const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                  uint32_t window_frames, uint32_t step_frames, uint32_t flags, const uint32_t* seg_rec,
                                  const uint32_t* seg_sid, const uint32_t* seg_first, const uint32_t* seg_last,
                                  const int32_t* seg_pos_first, const int32_t* seg_pos_last, const uint32_t* seg_t16,
                                  const uint32_t* seg_f16, uint64_t n_segs, uint32_t margin_frames, uint32_t drift_bins,
                                  uint32_t* zone_lo, uint32_t* zone_hi, int32_t* zone_d_lo, int32_t* zone_d_hi, uint32_t* zone_count,
                                  uint32_t* zone_q_first, uint32_t* zone_q_last, uint32_t* zone_t_first, uint32_t* zone_t_last,
                                  uint32_t* zone_shift, uint32_t* zone_hist, uint64_t* zone_sum_q, uint64_t* zone_sum_u,
                                  uint64_t* zone_sum_qq, uint64_t* zone_sum_qu, uint64_t* out_work, float* ms_extract,
                                  float* ms_warp, float* ms_extent) {
  const char* who = "shz_scan_plays";
  if (!ctx || !t) return SHZ_E_INVALID;
  // everything that can be refused is refused before the first launch, in this order
  if (flags & ~SHZ_PCM_DEVICE) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE", who);
  if (window_frames == 0 || window_frames >= (1u << 20))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: window_frames must be in [1, 2^20) (query offsets), got %u", who, window_frames);
  if (step_frames == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: step_frames must be at least 1", who);
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  if (margin_frames >= (1u << 20)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: margin_frames must be below 2^20, got %u", who, margin_frames);
  if (n_segs == 0) return SHZ_OK;   // no segment: nothing is launched, nothing is written
  if (3 * n_segs >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu segments in one call", who, (unsigned long long)n_segs);
  if (n_recs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %llu segments and no recording", who, (unsigned long long)n_segs);
  SHZ_TRY(shz_check_clip0(ctx, "rec_clip0", "recording", rec_clip0, n_recs, n_clips));
  SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  if (fs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "Fs must be > 0");
  if (n_clips && !pcm && clip_off[n_clips] > clip_off[0]) SHZ_FAIL(ctx, SHZ_E_INVALID, "pcm is NULL");
  if (!seg_rec || !seg_sid || !seg_first || !seg_last || !seg_pos_first || !seg_pos_last || !seg_t16 || !seg_f16)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL segment array", who);
  if (!zone_lo || !zone_hi || !zone_d_lo || !zone_d_hi || !zone_count || !zone_q_first || !zone_q_last || !zone_t_first ||
      !zone_t_last || !zone_shift || !zone_sum_q || !zone_sum_u || !zone_sum_qq || !zone_sum_qu)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL zone array", who);
  for (uint64_t i = 0; i < n_segs; ++i)
    if (seg_f16[i] < SP_S_MIN || seg_f16[i] > SP_S_MAX)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: pitch factor of segment %llu is %u; factors are Q16 in [%u, %u] (0.5x .. 2x)", who,
               (unsigned long long)i, seg_f16[i], SP_S_MIN, SP_S_MAX);
  SHZ_TRY(ex_state(ctx, t, who, 1));
  SHZ_TRY(ex_table_limits(ctx, t, who));
  // the zones and their candidates, on the host: shz_scan_play_zones, and what it refuses
  const uint64_t nz = 3 * n_segs;
  std::vector<uint64_t> frames((size_t)n_recs, 0);
  uint64_t all_frames = 0;
  for (uint32_t r = 0; r < n_recs; ++r)
    for (uint32_t c = rec_clip0[r]; c < rec_clip0[r + 1]; ++c) {
      const uint64_t fc = shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop);
      frames[r] = std::max<uint64_t>(frames[r], fc);
      all_frames += fc;
    }
  const uint32_t w = (uint32_t)std::min<uint64_t>((uint64_t)ctx->vote_tol + drift_bins, 0xFFFFFFFFull);
  std::vector<uint32_t> z_lo((size_t)nz), z_hi((size_t)nz), c_sid((size_t)nz), c_n((size_t)nz), w_lo((size_t)nz), w_hi((size_t)nz);
  std::vector<uint64_t> z_wlo((size_t)nz), z_whi((size_t)nz);
  std::vector<int32_t> c_dlo((size_t)nz), c_dhi((size_t)nz);
  const int32_t rz = shz_scan_play_zones(seg_rec, seg_sid, seg_first, seg_last, seg_pos_first, seg_pos_last, seg_t16, n_segs,
                                         frames.data(), n_recs, window_frames, step_frames, margin_frames, w, z_lo.data(), z_hi.data(),
                                         z_wlo.data(), z_whi.data(), c_dlo.data(), c_dhi.data(), c_n.data());
  if (rz == SHZ_E_INVALID)
    SHZ_FAIL(ctx, rz, "%s: segments must be a timeline's (recordings ascending and below n_recs, first <= last, windows ascending "
             "inside a recording), time factors Q16 in [%u, %u]", who, SP_S_MIN, SP_S_MAX);
  if (rz == SHZ_E_UNSUPPORTED)
    SHZ_FAIL(ctx, rz, "%s: a warped zone of 2^20 frames or more (query offsets), or a candidate %u bins or more wide at "
             "tolerance %u + drift_bins %u (the sums)", who, EX_FIT_MAX_WIDTH, ctx->vote_tol, drift_bins);
  SHZ_TRY(rz);
  for (uint64_t z = 0; z < nz; ++z) {
    if (z_whi[z] > 0xFFFFFFFFull) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: a warped frame beyond 2^32", who);
    w_lo[z] = (uint32_t)z_wlo[z];
    w_hi[z] = (uint32_t)z_whi[z];
    c_sid[z] = seg_sid[z / 3];
  }
  ex_args A{(uint32_t)nz, 1, c_sid.data(), c_dlo.data(), c_dhi.data(), c_n.data(), zone_count, zone_q_first, zone_q_last,
            zone_t_first, zone_t_last, zone_hist, zone_shift};
  A.out_sum_q = zone_sum_q;
  A.out_sum_u = zone_sum_u;
  A.out_sum_qq = zone_sum_qq;
  A.out_sum_qu = zone_sum_qu;
  SHZ_TRY(ex_check(ctx, t, who, A));
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = ms_extract || ms_warp || ms_extent;
  if (timed) {
    for (hipEvent_t& e : ctx->sc_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[0], ctx->stream));
  }
  // a) the peaks of every clip, once
  std::vector<uint64_t> peak_off((size_t)n_clips + 1, 0);
  const uint16_t* d_pf = nullptr;
  const uint32_t* d_pt = nullptr;
  SHZ_TRY(sp_peaks_owned(ctx, who, pcm, clip_off, n_clips, all_frames, fs, amp_min, flags & SHZ_PCM_DEVICE, peak_off.data(), &d_pf, &d_pt));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[1], ctx->stream));
  // b) one job per (segment, channel), covering zone 0 and SHZ_MAX_DT warped frames behind it
  std::vector<sp_job> jobs;
  std::vector<uint64_t> seg_job0((size_t)n_segs);
  std::vector<uint32_t> seg_nch((size_t)n_segs);
  for (uint64_t i = 0; i < n_segs; ++i) {
    const uint32_t c0 = rec_clip0[seg_rec[i]], c1 = rec_clip0[seg_rec[i] + 1];
    seg_job0[i] = jobs.size();
    seg_nch[i] = c1 - c0;
    for (uint32_t c = c0; c < c1; ++c)
      jobs.push_back(sp_job{peak_off[c] - peak_off[0], peak_off[c + 1] - peak_off[0], z_wlo[3 * i], z_whi[3 * i] + SHZ_MAX_DT - 1,
                            seg_t16[i], seg_f16[i]});
  }
  const uint64_t n_jobs = jobs.size();
  if (n_jobs >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu (segment, channel) jobs in one call", who, (unsigned long long)n_jobs);
  // c) the warp on the jobs: the exact CSR on both sides, the hashes stay on the device
  std::vector<uint64_t> ho((size_t)n_jobs + 1, 0);
  uint64_t n_items = 0, total = 0;
  void *d_key = nullptr, *d_t1 = nullptr;
  if (n_jobs) {
    sp_pass P;
    SHZ_TRY(sp_count_jobs(ctx, d_pf, d_pt, jobs.data(), (uint32_t)n_jobs, fan_value, &P, ho.data(), &n_items));
    total = ho[n_jobs];
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_KEY, total * 4 + 64, &d_key));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_T1, total * 4 + 64, &d_t1));
    if (total) SHZ_TRY(sp_write(ctx, P, (uint32_t*)d_key, (uint32_t*)d_t1, total));
  }
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[2], ctx->stream));
  // d) the cut: the zone stage over the jobs' CSR with the warped borders, e) the extent pass with the moments
  std::vector<uint64_t> query_off((size_t)nz + 1, 0);
  const uint32_t *d_zk = nullptr, *d_zq = nullptr;
  SHZ_TRY(sc_zone_stage(ctx, who, seg_job0.data(), seg_nch.data(), n_segs, n_jobs, ho.data(), (const uint32_t*)d_key,
                        (const uint32_t*)d_t1, w_lo.data(), w_hi.data(), query_off.data(), &d_zk, &d_zq));
  const int32_t rx = ex_device(ctx, t, who, d_zk, d_zq, query_off.data(), A);
  if (rx != SHZ_OK) {
    (void)hipStreamSynchronize(ctx->stream);   // (a refused pass may have queued work that reads the columns)
    return rx;
  }
  float ms[3] = {0.f, 0.f, 0.f};
  if (timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->sc_ev[3], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->sc_ev[3]));
    for (int k = 0; k < 3; ++k) SHZ_HIP(ctx, hipEventElapsedTime(&ms[k], ctx->sc_ev[k], ctx->sc_ev[k + 1]));
  }
  // the pass has written its outputs: the zones and candidates beside them, query frames -> warped recording frames
  for (uint64_t z = 0; z < nz; ++z) {
    zone_lo[z] = z_lo[z];
    zone_hi[z] = z_hi[z];
    zone_d_lo[z] = c_dlo[z];
    zone_d_hi[z] = c_dhi[z];
    if (zone_count[z]) {
      zone_q_first[z] += w_lo[z];
      zone_q_last[z] += w_lo[z];
    }
  }
  if (out_work) {
    out_work[0] = n_items;
    out_work[1] = total;
    out_work[2] = query_off[nz];
  }
  if (ms_extract) *ms_extract = ms[0];
  if (ms_warp) *ms_warp = ms[1];
  if (ms_extent) *ms_extent = ms[2];
  return SHZ_OK;
}
