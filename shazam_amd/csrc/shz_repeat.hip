// Repeated content inside a recording, without a table: the self-join of a recording's hashes as a lag
// histogram.  Two hashes of one recording with the same key at times t_i < t_j vote for the lag t_j - t_i; a stretch of audio
// that airs twice piles its votes on one lag over a contiguous stretch of t_i.  The chain is integer from end to end:
//
//   compose   rec << 52 | key32 << 20 | t1 of every hash (the recording by binary search in the CSR)
//   unique    shz_sort_u64 on the significant bits, head flags, scan, compaction             -> rec_hashes
//   runs      one key of one recording: head flags on key >> 20, scan, first element of every run
//   count     partners of element i: two binary searches for t_i + min_lag, t_i + max_lag in (i, run end); runs longer than
//             max_run count 0 and feed the skip counters; shz_scan_u64                         -> rec_pairs
//   expand    by OUTPUT tile: a workgroup owns consecutive pair positions and finds their owner elements in the scanned
//             counts, so the stores are coalesced whatever the run lengths: rec_in_slice << 40 | lag << 20 | t_i
//   cells     shz_sort_u64 on the bits from cell_shift up (the low bits of t ride along), head flags, scan; pairs = run length,
//             first / last = a wave-segmented min / max and one atomicMin / atomicMax per (wave, cell); the cells with
//             min_cell_pairs pairs compacted and copied out
//
// expand and cells run per slice of whole recordings whose two pair buffers fit 1/8 of the workspace limit.  Workspace: the
// slots SHZ_WS_RP_*, SHZ_WS_SORT_* and SHZ_WS_SCAN_TMP -- none of the extraction's, so shz_repeats_batch reads the hashes
// where shz_extract_owned left them.  shz_repeats_fold (host) joins the returned cells into repeats.
//
// Content shared between TWO recordings (shz_shared_*) is the same join over a list of jobs (a, b) with a
// signed lag: the elements and runs of all recordings once (rp_elements), one item per (job, element of a), the partners of an
// item in b's run of its key (sh_count_kernel), pairs job << 41 | (lag + 2^20) << 20 | t_a by output tile (sh_expand_kernel),
// and from there the cell stage above with a lag field of 21 bits (rp_cells).
//
// ALTERED shared content (shz_shared_warps_*) is that join at a table of warps: one warp pass in the job form
// (shz_speed.hip) over every clip as it is and over the clips of every distinct (recording, warp) the jobs name, its columns
// handed to sh_core as virtual recordings, and a lag window per job in sh_count_kernel.
#include <algorithm>
#include <numeric>

#include "shz_internal.h"

#define RP_THREADS 256
#define RP_SMALL 64u            // threads of a block and pairs of an expand tile under SHZ_DEBUG_REPEAT_SMALL_SLICES
#define RP_TILE 2048u           // pairs of an expand tile
#define RP_MAX_RECS 4096u       // recordings of a call: 12 bits above key32 << 20 | t1, and above lag << 20 | t
#define RP_T_BITS 20
#define RP_T_MASK 0xFFFFFu

struct rp_params {
  uint32_t min_lag, max_lag, max_run, cell_shift, min_cell_pairs;
};
struct rp_out {
  uint64_t* cell_off;
  uint32_t *cell_lag, *cell_block, *cell_pairs, *cell_first, *cell_last, *rec_hashes, *rec_skipped_keys;
  uint64_t *rec_pairs, *rec_skipped_rows, cap_cells, *count;
};

static inline unsigned rp_grid(uint64_t n, uint32_t bs) { return (unsigned)((n + bs - 1) / bs); }
static inline int rp_bits(uint32_t v) {   // bits that hold the values 0 .. v
  int b = 0;
  while (v >> b) ++b;
  return b;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
// rec_off[n_recs + 1]: first hash of every recording; entry i belongs to the last r with rec_off[r] <= i
__global__ __launch_bounds__(RP_THREADS) void rp_compose_kernel(const uint32_t* __restrict__ key32, const uint32_t* __restrict__ t1,
                                                                const uint64_t* __restrict__ rec_off, uint32_t n_recs, uint64_t n,
                                                                uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t lo = 0, hi = n_recs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (rec_off[mid] <= i) lo = mid; else hi = mid;
  }
  out[i] = ((uint64_t)lo << 52) | ((uint64_t)key32[i] << RP_T_BITS) | (t1[i] & RP_T_MASK);
}

// flag[i] = keys[i] >> shift differs from its left neighbour's (element 0: set)
__global__ __launch_bounds__(RP_THREADS) void rp_head_kernel(const uint64_t* __restrict__ keys, uint64_t n, int shift,
                                                             uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0 || (keys[i] >> shift) != (keys[i - 1] >> shift)) ? 1u : 0u;
}

__global__ __launch_bounds__(RP_THREADS) void rp_compact_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ flag,
                                                                const uint32_t* __restrict__ pos, uint64_t n,
                                                                uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flag[i]) out[pos[i]] = keys[i];
}

// rec_start[r] = first unique element of recording r, r = 0 .. n_recs (the last: n)
__global__ __launch_bounds__(RP_THREADS) void rp_rec_start_kernel(const uint64_t* __restrict__ U, uint32_t n, uint32_t n_recs,
                                                                  uint32_t* __restrict__ rec_start) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_recs) return;
  uint32_t lo = 0, hi = n;   // first element with U >> 52 >= r
  if (r == n_recs) lo = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)(U[mid] >> 52) < r) lo = mid + 1; else hi = mid;
  }
  rec_start[r] = lo;
}

// run_start[id] at the heads; the entry behind the last run (tot[1] runs) = n
__global__ __launch_bounds__(RP_THREADS) void rp_run_start_kernel(const uint32_t* __restrict__ head, const uint32_t* __restrict__ pos,
                                                                  uint32_t n, const uint64_t* __restrict__ n_runs,
                                                                  uint32_t* __restrict__ run_start) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (head[i]) run_start[pos[i]] = i;
  if (i == 0) run_start[*n_runs] = n;
}

// partners of element i in its run: the elements j in (i, run end) with min_lag <= t_j - t_i <= max_lag -- the times of a run
// ascend strictly -- as [lo[i], lo[i] + cnt[i]).  Runs longer than max_run: 0, and their heads count the skipped key and rows
__global__ __launch_bounds__(RP_THREADS) void rp_count_kernel(const uint64_t* __restrict__ U, const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ pos, const uint32_t* __restrict__ run_start,
                                                              uint32_t n, rp_params P, uint64_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ lo_out, uint32_t* __restrict__ skip_keys,
                                                              unsigned long long* __restrict__ skip_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t h = head[i], id = pos[i] + h - 1;
  const uint32_t b = run_start[id], e = run_start[id + 1];
  const uint64_t key = U[i];
  if (e - b > P.max_run) {
    cnt[i] = 0;
    lo_out[i] = 0;
    if (h) {
      const uint32_t r = (uint32_t)(key >> 52);
      atomicAdd(&skip_keys[r], 1u);
      atomicAdd(&skip_rows[r], (unsigned long long)(e - b));
    }
    return;
  }
  const uint32_t t = (uint32_t)key & RP_T_MASK, t_lo = t + P.min_lag, t_hi = t + P.max_lag;   // < 2^21
  uint32_t l = i + 1, r = e;   // first j with t_j >= t_lo
  while (l < r) {
    const uint32_t mid = l + ((r - l) >> 1);
    if (((uint32_t)U[mid] & RP_T_MASK) < t_lo) l = mid + 1; else r = mid;
  }
  const uint32_t first = l;
  r = e;                       // first j with t_j > t_hi
  while (l < r) {
    const uint32_t mid = l + ((r - l) >> 1);
    if (((uint32_t)U[mid] & RP_T_MASK) <= t_hi) l = mid + 1; else r = mid;
  }
  cnt[i] = l - first;
  lo_out[i] = first;
}

// rec_po[r] = pairs in front of recording r, r = 0 .. n_recs
__global__ __launch_bounds__(RP_THREADS) void rp_rec_pairs_kernel(const uint64_t* __restrict__ poff, const uint32_t* __restrict__ rec_start,
                                                                  uint32_t n_recs, uint64_t* __restrict__ rec_po) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r <= n_recs) rec_po[r] = poff[rec_start[r]];
}

// The pairs [P0, P0 + np) of the elements [e0, e1) go to out[0 .. np): block b owns the positions [b tile, (b + 1) tile).
// Pair g belongs to the last element x with poff[x] <= g (elements without partners share their successor's poff and are
// never that one); it is x's partner number g - poff[x].  The block finds the owners of its first and last pair, every lane
// searches between them
__global__ __launch_bounds__(RP_THREADS) void rp_expand_kernel(const uint64_t* __restrict__ U, const uint64_t* __restrict__ poff,
                                                               const uint32_t* __restrict__ lo, uint32_t e0, uint32_t e1, uint64_t P0,
                                                               uint64_t np, uint32_t tile, uint32_t r0, uint64_t* __restrict__ out) {
  const uint64_t base = (uint64_t)blockIdx.x * tile;
  if (base >= np) return;
  const uint64_t end = min(base + tile, np);
  uint32_t xA, xB;
  {
    const uint64_t gA = P0 + base, gB = P0 + end - 1;
    uint32_t l = e0, h = e1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= gA) l = mid; else h = mid;
    }
    xA = l;
    h = e1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= gB) l = mid; else h = mid;
    }
    xB = l;
  }
  for (uint64_t p = base + threadIdx.x; p < end; p += blockDim.x) {
    const uint64_t g = P0 + p;
    uint32_t l = xA, h = xB + 1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= g) l = mid; else h = mid;
    }
    const uint64_t key = U[l];
    const uint32_t j = lo[l] + (uint32_t)(g - poff[l]);
    const uint32_t ti = (uint32_t)key & RP_T_MASK, tj = (uint32_t)U[j] & RP_T_MASK;
    out[p] = ((uint64_t)((uint32_t)(key >> 52) - r0) << 40) | ((uint64_t)(tj - ti) << RP_T_BITS) | ti;
  }
}

__global__ __launch_bounds__(RP_THREADS) void rp_cell_init_kernel(uint32_t nc, uint32_t np, uint32_t* __restrict__ head_pos,
                                                                  uint32_t* __restrict__ first, uint32_t* __restrict__ last) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nc) {
    first[c] = 0xFFFFFFFFu;
    last[c] = 0u;
  }
  if (c == nc) head_pos[nc] = np;
}

// Pair i of the sorted slice lies in cell pos[i] + head[i] - 1; the heads write head_pos.  first / last: the lanes of a wave
// that share a cell are neighbours, so a segmented scan over the wave leaves the cell's min / max of the wave in its last lane
// there, which hands them to the cell record -- integers, the same whatever the order
__global__ __launch_bounds__(RP_THREADS) void rp_cell_reduce_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head,
                                                                    const uint32_t* __restrict__ pos, uint32_t np,
                                                                    uint32_t* __restrict__ head_pos, uint32_t* __restrict__ first,
                                                                    uint32_t* __restrict__ last) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool live = i < np;
  uint32_t id = 0xFFFFFFFFu, mn = 0xFFFFFFFFu, mx = 0u;
  if (live) {
    const uint32_t h = head[i];
    id = pos[i] + h - 1;
    mn = mx = (uint32_t)keys[i] & RP_T_MASK;
    if (h) head_pos[id] = i;
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t oid = __shfl_up(id, d, 64), omn = __shfl_up(mn, d, 64), omx = __shfl_up(mx, d, 64);
    if (lane >= d && oid == id) {
      mn = min(mn, omn);
      mx = max(mx, omx);
    }
  }
  const uint32_t nid = __shfl_down(id, 1, 64);
  if (live && (lane == 63 || nid != id)) {
    atomicMin(&first[id], mn);
    atomicMax(&last[id], mx);
  }
}

__global__ __launch_bounds__(RP_THREADS) void rp_keep_kernel(const uint32_t* __restrict__ head_pos, uint32_t nc, uint32_t min_pairs,
                                                             uint32_t* __restrict__ keep) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nc) keep[c] = (head_pos[c + 1] - head_pos[c]) >= min_pairs ? 1u : 0u;
}

// the kept cells in their order: out = rec | lag | block | pairs | first | last, nk entries each.  lag_bits: the width of the
// lag field above the 20 bits of t (20: the self-join's lag; 21: the biased signed lag of the join between two recordings)
__global__ __launch_bounds__(RP_THREADS) void rp_cell_out_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head_pos,
                                                                 const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
                                                                 const uint32_t* __restrict__ keep, const uint32_t* __restrict__ place,
                                                                 uint32_t nc, uint32_t nk, uint32_t r0, uint32_t cell_shift,
                                                                 int lag_bits, uint32_t* __restrict__ out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc || !keep[c]) return;
  const uint32_t o = place[c], hp = head_pos[c];
  if (o >= nk) return;
  const uint64_t key = keys[hp];
  out[o] = (uint32_t)(key >> (RP_T_BITS + lag_bits)) + r0;
  out[(uint64_t)nk + o] = (uint32_t)(key >> RP_T_BITS) & ((1u << lag_bits) - 1u);
  out[2ull * nk + o] = ((uint32_t)key & RP_T_MASK) >> cell_shift;
  out[3ull * nk + o] = head_pos[c + 1] - hp;
  out[4ull * nk + o] = first[c];
  out[5ull * nk + o] = last[c];
}

// ---- what both entry points refuse before anything is launched ------------------------------------------------------------
static int32_t rp_check_knobs(shz_ctx* ctx, const char* who, uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs) {
  if (max_run < 2 || max_run > 1024) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_run must be in [2, 1024], got %u", who, max_run);
  if (cell_shift > 19) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: cell_shift must be at most 19, got %u", who, cell_shift);
  if (min_cell_pairs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: min_cell_pairs must be at least 1", who);
  return SHZ_OK;
}
static int32_t rp_check(shz_ctx* ctx, const char* who, const rp_params& P, const rp_out& O) {
  if (!O.count || !O.cell_off || !O.rec_hashes || !O.rec_skipped_keys || !O.rec_pairs || !O.rec_skipped_rows)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: count, cell_off or a rec_* array is NULL", who);
  if (O.cap_cells && (!O.cell_lag || !O.cell_block || !O.cell_pairs || !O.cell_first || !O.cell_last))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL cell array with room for %llu cells", who, (unsigned long long)O.cap_cells);
  if (P.max_lag < P.min_lag) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_lag %u is below min_lag %u", who, P.max_lag, P.min_lag);
  if (P.max_lag >= (1u << RP_T_BITS)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_lag must be below 2^20, got %u", who, P.max_lag);
  return rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs);
}
// host columns: hash_off[n_clips + 1] from 0 and never decreasing, the columns there, fewer than 2^32 hashes, every t1 < 2^20
static int32_t rp_check_columns(shz_ctx* ctx, const char* who, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off,
                                uint32_t n_clips) {
  if (!hash_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: hash_off is NULL", who);
  if (hash_off[0] != 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: hash_off must start at 0 (it starts at %llu)", who, (unsigned long long)hash_off[0]);
  for (uint32_t c = 0; c < n_clips; ++c)
    if (hash_off[c + 1] < hash_off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: hash_off decreases at clip %u", who, c);
  const uint64_t N = hash_off[n_clips];
  if (N && (!key32 || !t1)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL column", who);
  if (N >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu hashes", who, (unsigned long long)N);
  for (uint64_t i = 0; i < N; ++i)
    if (t1[i] >> RP_T_BITS) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: t1[%llu] = %u, times must be below 2^20", who, (unsigned long long)i, t1[i]);
  return SHZ_OK;
}
// device copies of N >= 1 host hashes for the length of a call (tests / tools)
struct rp_columns {
  shz_ctx* ctx;
  void *key = nullptr, *t1 = nullptr;
  explicit rp_columns(shz_ctx* c) : ctx(c) {}
  int32_t upload(const char* who, const uint32_t* key32, const uint32_t* t1_, uint64_t N) {
    SHZ_HIP(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(&key, N * 4) != hipSuccess || hipMalloc(&t1, N * 4) != hipSuccess) {
      (void)hipGetLastError();
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(2 x %llu) failed", who, (unsigned long long)(N * 4));
    }
    if (shz_memcpy(ctx, key, key32, N * 4, hipMemcpyHostToDevice) != hipSuccess ||
        shz_memcpy(ctx, t1, t1_, N * 4, hipMemcpyHostToDevice) != hipSuccess)
      SHZ_FAIL(ctx, SHZ_E_HIP, "%s: copy of the columns failed", who);
    return SHZ_OK;
  }
  ~rp_columns() {
    if (key || t1) (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
    if (key) (void)hipFree(key);
    if (t1) (void)hipFree(t1);
  }
};
// the recordings' clips (no recording: no clips either, and the caller is done -- what it writes then: rp_empty)
static int32_t rp_check_recs(shz_ctx* ctx, const char* who, uint32_t n_clips, const uint32_t* rec_clip0, uint32_t n_recs) {
  if (n_recs == 0) {
    if (n_clips) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %u clips belong to no recording", who, n_clips);
    return SHZ_OK;
  }
  if (n_recs > RP_MAX_RECS) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %u recordings in one call, at most %u", who, n_recs, RP_MAX_RECS);
  return shz_check_clip0(ctx, "rec_clip0", "recording", rec_clip0, n_recs, n_clips);
}
static void rp_empty(const rp_out& O, uint32_t n_recs) {
  *O.count = 0;
  for (uint32_t r = 0; r <= n_recs; ++r) O.cell_off[r] = 0;
  for (uint32_t r = 0; r < n_recs; ++r) {
    O.rec_hashes[r] = O.rec_skipped_keys[r] = 0;
    O.rec_pairs[r] = O.rec_skipped_rows[r] = 0;
  }
}

// ---- the stages both joins share --------------------------------------------------------------------------------------------
struct rp_elems {
  const uint64_t* U;                        // the unique composed hashes, sorted
  uint32_t nu;
  const uint32_t *head, *pos, *run_start;   // run heads and their scan (SHZ_WS_RP_FLAG / _SCAN), first element of every run
};
// compose, sort + unique, the recordings' borders, the runs of the N >= 1 hashes.  d_rec_off[n_recs + 1]: first hash of every
// recording; d_tot[0] / d_tot[1] get the unique elements / the runs, d_rec_start[n_recs + 1] the borders in U.  One host
// read-back (the unique count); the stream is busy with the runs on return
static int32_t rp_elements(shz_ctx* ctx, const char* who, const uint32_t* d_key32, const uint32_t* d_t1, uint64_t N, uint32_t n_recs,
                           const uint64_t* d_rec_off, uint64_t* d_tot, uint32_t* d_rec_start, uint32_t bs, rp_elems* E) {
  hipStream_t st = ctx->stream;
  void *ka, *kb, *d_flag, *d_scan, *d_u, *d_run;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_A, N * 8, &ka));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_B, N * 8, &kb));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_FLAG, N * 4, &d_flag));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_SCAN, N * 4, &d_scan));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_U, N * 8, &d_u));
  hipLaunchKernelGGL(rp_compose_kernel, dim3(rp_grid(N, bs)), dim3(bs), 0, st, d_key32, d_t1, d_rec_off, n_recs, N, (uint64_t*)ka);
  SHZ_HIP(ctx, hipGetLastError());
  int sel = 0;
  SHZ_TRY(shz_sort_u64(ctx, (uint64_t*)ka, (uint64_t*)kb, nullptr, nullptr, 0, N, 0, 52 + rp_bits(n_recs - 1), &sel));
  const uint64_t* sorted = (const uint64_t*)(sel ? kb : ka);
  hipLaunchKernelGGL(rp_head_kernel, dim3(rp_grid(N, bs)), dim3(bs), 0, st, sorted, N, 0, (uint32_t*)d_flag);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)d_flag, (uint32_t*)d_scan, N, d_tot));
  hipLaunchKernelGGL(rp_compact_kernel, dim3(rp_grid(N, bs)), dim3(bs), 0, st, sorted, (const uint32_t*)d_flag, (const uint32_t*)d_scan,
                     N, (uint64_t*)d_u);
  SHZ_HIP(ctx, hipGetLastError());
  uint64_t nu64 = 0;
  SHZ_HIP(ctx, shz_memcpy(ctx, &nu64, d_tot, 8, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  if (nu64 == 0 || nu64 > N) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu unique hashes of %llu", who, (unsigned long long)nu64, (unsigned long long)N);
  const uint32_t nu = (uint32_t)nu64;
  const uint64_t* U = (const uint64_t*)d_u;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_RUN, ((uint64_t)nu + 1) * 4, &d_run));
  hipLaunchKernelGGL(rp_rec_start_kernel, dim3(rp_grid((uint64_t)n_recs + 1, bs)), dim3(bs), 0, st, U, nu, n_recs, d_rec_start);
  hipLaunchKernelGGL(rp_head_kernel, dim3(rp_grid(nu, bs)), dim3(bs), 0, st, U, (uint64_t)nu, RP_T_BITS, (uint32_t*)d_flag);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)d_flag, (uint32_t*)d_scan, nu, d_tot + 1));
  hipLaunchKernelGGL(rp_run_start_kernel, dim3(rp_grid(nu, bs)), dim3(bs), 0, st, (const uint32_t*)d_flag, (const uint32_t*)d_scan, nu,
                     (const uint64_t*)(d_tot + 1), (uint32_t*)d_run);
  SHZ_HIP(ctx, hipGetLastError());
  *E = rp_elems{U, nu, (const uint32_t*)d_flag, (const uint32_t*)d_scan, (const uint32_t*)d_run};
  return SHZ_OK;
}

// the slices: consecutive whole owners (recordings, jobs) whose pairs po[o + 1] - po[o] together stay within max_pairs, none
// larger than that alone; one owner a slice under SHZ_DEBUG_REPEAT_SMALL_SLICES.  Returns the slices' borders
static std::vector<uint32_t> rp_cut_slices(const uint64_t* po, uint32_t n, uint64_t max_pairs, bool small, uint64_t* np_max) {
  std::vector<uint32_t> slices{0};
  *np_max = 0;
  for (uint32_t r0 = 0; r0 < n;) {
    uint32_t r1 = r0 + 1;
    while (!small && r1 < n && po[r1 + 1] - po[r0] <= max_pairs) ++r1;
    *np_max = std::max(*np_max, po[r1] - po[r0]);
    slices.push_back(r1);
    r0 = r1;
  }
  return slices;
}

// The cell stage of a slice and the cells of the call.  A slice's np pair keys owner_in_slice << (20 + lag_bits) | lag << 20 | t
// lie in ka (the expand, queued behind rp_ev[0], wrote them); slice() sorts them on the bits from cell_shift up, reduces the
// cells and gathers the kept ones on the host, copy_out() hands them to the caller
struct rp_cells {
  shz_ctx* ctx;
  const char *who, *what;   // the entry point, and what owns cells ("recording", "job"), for messages
  uint32_t n_owners, bs;
  uint64_t cap;
  bool timed;
  uint64_t *ka = nullptr, *kb = nullptr;
  uint32_t *flag = nullptr, *scan = nullptr;
  std::vector<uint32_t> c_lag, c_block, c_pairs, c_first, c_last, blockbuf;
  std::vector<uint64_t> cell_off;
  uint64_t n_cells_all = 0;
  rp_cells(shz_ctx* c, const char* who_, const char* what_, uint32_t n, uint64_t cap_, uint32_t bs_, bool timed_)
      : ctx(c), who(who_), what(what_), n_owners(n), bs(bs_), cap(cap_), timed(timed_), cell_off((size_t)n + 1, 0) {}
  int32_t reserve(uint64_t np_max) {
    if (np_max == 0) return SHZ_OK;
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_A, np_max * 8, &p));
    ka = (uint64_t*)p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_B, np_max * 8, &p));
    kb = (uint64_t*)p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_FLAG, np_max * 4, &p));
    flag = (uint32_t*)p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_SCAN, np_max * 4, &p));
    scan = (uint32_t*)p;
    return SHZ_OK;
  }
  // d_tot[2] / d_tot[3]: the slice's cells / kept cells.  The owners [r0, r1) are in the slice.  The times of the expand and of
  // the cell stage are added to *ms_expand / *ms_cells when timed
  int32_t slice(uint64_t* d_tot, uint32_t np, uint32_t cell_shift, uint32_t min_cell_pairs, int lag_bits, uint32_t r0, uint32_t r1,
                float* ms_expand, float* ms_cells) {
    hipStream_t st = ctx->stream;
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], st));
    int sel = 0;
    SHZ_TRY(shz_sort_u64(ctx, ka, kb, nullptr, nullptr, 0, np, (int)cell_shift, RP_T_BITS + lag_bits + rp_bits(r1 - r0 - 1), &sel));
    const uint64_t* pk = sel ? kb : ka;
    hipLaunchKernelGGL(rp_head_kernel, dim3(rp_grid(np, bs)), dim3(bs), 0, st, pk, (uint64_t)np, (int)cell_shift, flag);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)flag, scan, np, d_tot + 2));
    uint64_t nc64 = 0;
    SHZ_HIP(ctx, shz_memcpy(ctx, &nc64, d_tot + 2, 8, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(st));
    if (nc64 == 0 || nc64 > np) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu cells of %u pairs", who, (unsigned long long)nc64, np);
    const uint32_t nc = (uint32_t)nc64;
    void* d_cell;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_CELL, (5ull * nc + 2) * 4, &d_cell));
    uint32_t *head_pos = (uint32_t*)d_cell, *cfirst = head_pos + nc + 1, *clast = cfirst + nc, *keep = clast + nc, *place = keep + nc;
    hipLaunchKernelGGL(rp_cell_init_kernel, dim3(rp_grid((uint64_t)nc + 1, bs)), dim3(bs), 0, st, nc, np, head_pos, cfirst, clast);
    hipLaunchKernelGGL(rp_cell_reduce_kernel, dim3(rp_grid(np, bs)), dim3(bs), 0, st, pk, (const uint32_t*)flag, (const uint32_t*)scan, np,
                       head_pos, cfirst, clast);
    hipLaunchKernelGGL(rp_keep_kernel, dim3(rp_grid(nc, bs)), dim3(bs), 0, st, (const uint32_t*)head_pos, nc, min_cell_pairs, keep);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)keep, place, nc, d_tot + 3));
    uint64_t nk64 = 0;
    SHZ_HIP(ctx, shz_memcpy(ctx, &nk64, d_tot + 3, 8, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(st));
    if (nk64 > nc) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu kept cells of %u", who, (unsigned long long)nk64, nc);
    const uint32_t nk = (uint32_t)nk64;
    if (nk) {
      void* d_out;
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_OUT, 6ull * nk * 4, &d_out));
      hipLaunchKernelGGL(rp_cell_out_kernel, dim3(rp_grid(nc, bs)), dim3(bs), 0, st, pk, (const uint32_t*)head_pos, (const uint32_t*)cfirst,
                         (const uint32_t*)clast, (const uint32_t*)keep, (const uint32_t*)place, nc, nk, r0, cell_shift, lag_bits,
                         (uint32_t*)d_out);
      SHZ_HIP(ctx, hipGetLastError());
      blockbuf.resize(6 * (size_t)nk);
      SHZ_HIP(ctx, shz_memcpy(ctx, blockbuf.data(), d_out, 6ull * nk * 4, hipMemcpyDeviceToHost));
    }
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[2], st));
    SHZ_HIP(ctx, hipStreamSynchronize(st));
    if (timed) {
      float a = 0.f, b = 0.f;
      SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->rp_ev[0], ctx->rp_ev[1]));
      SHZ_HIP(ctx, hipEventElapsedTime(&b, ctx->rp_ev[1], ctx->rp_ev[2]));
      *ms_expand += a;
      *ms_cells += b;
    }
    for (uint32_t k = 0; k < nk; ++k) {
      const uint32_t r = blockbuf[k];
      if (r < r0 || r >= r1) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: a cell of %s %u in the slice [%u, %u)", who, what, r, r0, r1);
      ++cell_off[r + 1];
      if (n_cells_all + k < cap) {   // (what has no room is counted only)
        c_lag.push_back(blockbuf[(size_t)nk + k]);
        c_block.push_back(blockbuf[2 * (size_t)nk + k]);
        c_pairs.push_back(blockbuf[3 * (size_t)nk + k]);
        c_first.push_back(blockbuf[4 * (size_t)nk + k]);
        c_last.push_back(blockbuf[5 * (size_t)nk + k]);
      }
    }
    n_cells_all += nk;
    return SHZ_OK;
  }
  // cell_off[n_owners + 1], *count and the cells there is room for; SHZ_E_CAPACITY when there are more
  int32_t copy_out(uint64_t* o_off, uint32_t* o_lag, uint32_t* o_block, uint32_t* o_pairs, uint32_t* o_first, uint32_t* o_last,
                   uint64_t* count) {
    for (uint32_t r = 0; r < n_owners; ++r) cell_off[r + 1] += cell_off[r];
    memcpy(o_off, cell_off.data(), ((size_t)n_owners + 1) * 8);
    *count = n_cells_all;
    const size_t nw = c_lag.size();
    if (nw) {
      memcpy(o_lag, c_lag.data(), nw * 4);
      memcpy(o_block, c_block.data(), nw * 4);
      memcpy(o_pairs, c_pairs.data(), nw * 4);
      memcpy(o_first, c_first.data(), nw * 4);
      memcpy(o_last, c_last.data(), nw * 4);
    }
    if (n_cells_all > cap)
      SHZ_FAIL(ctx, SHZ_E_CAPACITY, "%s: %llu cells, room for %llu", who, (unsigned long long)n_cells_all, (unsigned long long)cap);
    return SHZ_OK;
  }
};

// ---- the core on device columns -------------------------------------------------------------------------------------------
// d_key32 / d_t1: device columns of hash_off[n_clips] < 2^32 entries with t1 < 2^20, hash_off (host) their CSR over the clips;
// everything else is checked (rp_check, rp_check_recs; n_recs >= 1).  The outputs are written when the call ends with SHZ_OK
// or SHZ_E_CAPACITY; the stream is idle then.  ms_pairs / ms_cells (may be NULL) get the stages' hipEvent times
static int32_t rp_core(shz_ctx* ctx, const char* who, const uint32_t* d_key32, const uint32_t* d_t1, const uint64_t* hash_off,
                       const uint32_t* rec_clip0, uint32_t n_recs, const rp_params& P, const rp_out& O, float* ms_pairs,
                       float* ms_cells) {
  const uint64_t N = hash_off[rec_clip0[n_recs]];
  if (N == 0) {
    rp_empty(O, n_recs);
    return SHZ_OK;
  }
  const bool small = (ctx->debug & SHZ_DEBUG_REPEAT_SMALL_SLICES) != 0, timed = ms_pairs || ms_cells;
  const uint32_t bs = small ? RP_SMALL : RP_THREADS, tile = small ? RP_SMALL : RP_TILE;
  hipStream_t st = ctx->stream;
  float pairs_ms = 0.f, cells_ms = 0.f;
  if (timed) {
    for (hipEvent_t& e : ctx->rp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], st));
  }
  // the recordings' block: tot[4] (unique elements, runs, a slice's cells, its kept cells) | rec_off | rec_po | skip_rows (u64)
  // | rec_start | skip_keys (u32).  rec_off goes up, the rest comes back in one copy
  const uint64_t nr1 = (uint64_t)n_recs + 1;
  const uint64_t o_off = 4, o_po = o_off + nr1, o_rows = o_po + nr1, n64 = o_rows + n_recs;
  const uint64_t rec_bytes = n64 * 8 + (nr1 + n_recs) * 4;
  std::vector<uint64_t> hrec((size_t)((rec_bytes + 7) / 8), 0);
  for (uint32_t r = 0; r <= n_recs; ++r) hrec[o_off + r] = hash_off[rec_clip0[r]];
  void* d_rec;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_REC, hrec.size() * 8, &d_rec));
  uint64_t* d64 = (uint64_t*)d_rec;
  uint64_t *d_tot = d64, *d_rec_off = d64 + o_off, *d_rec_po = d64 + o_po, *d_skip_rows = d64 + o_rows;
  uint32_t *d_rec_start = (uint32_t*)(d64 + n64), *d_skip_keys = d_rec_start + nr1;
  SHZ_HIP(ctx, shz_memcpy(ctx, d_rec, hrec.data(), hrec.size() * 8, hipMemcpyHostToDevice));
  // 1) compose, 2) sort + unique, 3) runs
  rp_elems E;
  SHZ_TRY(rp_elements(ctx, who, d_key32, d_t1, N, n_recs, d_rec_off, d_tot, d_rec_start, bs, &E));
  const uint32_t nu = E.nu;
  const uint64_t* U = E.U;
  // 4) count, scan, the recordings' numbers
  void *d_lo, *d_cnt, *d_poff;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_LO, (uint64_t)nu * 4, &d_lo));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_CNT, (uint64_t)nu * 8, &d_cnt));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_POFF, ((uint64_t)nu + 1) * 8, &d_poff));
  hipLaunchKernelGGL(rp_count_kernel, dim3(rp_grid(nu, bs)), dim3(bs), 0, st, U, E.head, E.pos, E.run_start, nu, P, (uint64_t*)d_cnt,
                     (uint32_t*)d_lo, d_skip_keys, (unsigned long long*)d_skip_rows);
  SHZ_HIP(ctx, hipGetLastError());
  uint64_t* poff = (uint64_t*)d_poff;
  SHZ_TRY(shz_scan_u64(ctx, (const uint64_t*)d_cnt, poff, nu, poff + nu));
  hipLaunchKernelGGL(rp_rec_pairs_kernel, dim3(rp_grid(nr1, bs)), dim3(bs), 0, st, (const uint64_t*)poff, (const uint32_t*)d_rec_start,
                     n_recs, d_rec_po);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, shz_memcpy(ctx, hrec.data(), d_rec, hrec.size() * 8, hipMemcpyDeviceToHost));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], st));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  if (timed) {
    float a = 0.f;
    SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->rp_ev[0], ctx->rp_ev[1]));
    pairs_ms += a;
  }
  const uint64_t *rec_po = hrec.data() + o_po, *skip_rows = hrec.data() + o_rows;
  const uint32_t *rec_start = (const uint32_t*)(hrec.data() + n64), *skip_keys = rec_start + nr1;
  if (rec_start[0] != 0 || rec_start[n_recs] != nu || rec_po[0] != 0)
    SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the recordings' borders do not span the %u unique hashes", who, nu);
  for (uint32_t r = 0; r < n_recs; ++r)
    if (rec_start[r + 1] < rec_start[r] || rec_po[r + 1] < rec_po[r])
      SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the borders of recording %u decrease", who, r);
  // 5) the slices: consecutive whole recordings whose two pair buffers fit 1/8 of the workspace limit
  const uint64_t max_pairs = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 8 / 16, 1), 1ull << 31);
  for (uint32_t r = 0; r < n_recs; ++r)
    if (rec_po[r + 1] - rec_po[r] > max_pairs)
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED,
               "%s: recording %u has %llu pairs, a slice holds %llu (workspace limit): raise min_lag (%u) or lower max_run (%u)", who, r,
               (unsigned long long)(rec_po[r + 1] - rec_po[r]), (unsigned long long)max_pairs, P.min_lag, P.max_run);
  uint64_t np_max = 0;
  const std::vector<uint32_t> slices = rp_cut_slices(rec_po, n_recs, max_pairs, small, &np_max);
  // 6) slice by slice: expand, sort, cells
  rp_cells C(ctx, who, "recording", n_recs, O.cap_cells, bs, timed);
  SHZ_TRY(C.reserve(np_max));
  for (size_t s = 0; s + 1 < slices.size(); ++s) {
    const uint32_t r0 = slices[s], r1 = slices[s + 1], e0 = rec_start[r0], e1 = rec_start[r1];
    const uint64_t P0 = rec_po[r0], np64 = rec_po[r1] - P0;
    if (np64 == 0) continue;
    const uint32_t np = (uint32_t)np64;   // (<= 2^31)
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], st));
    hipLaunchKernelGGL(rp_expand_kernel, dim3(rp_grid(np, tile)), dim3(bs), 0, st, U, (const uint64_t*)poff, (const uint32_t*)d_lo, e0, e1,
                       P0, np64, tile, r0, C.ka);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(C.slice(d_tot, np, P.cell_shift, P.min_cell_pairs, RP_T_BITS, r0, r1, &pairs_ms, &cells_ms));
  }
  // 7) the outputs
  for (uint32_t r = 0; r < n_recs; ++r) {
    O.rec_hashes[r] = rec_start[r + 1] - rec_start[r];
    O.rec_pairs[r] = rec_po[r + 1] - rec_po[r];
    O.rec_skipped_keys[r] = skip_keys[r];
    O.rec_skipped_rows[r] = skip_rows[r];
  }
  if (ms_pairs) *ms_pairs = pairs_ms;
  if (ms_cells) *ms_cells = cells_ms;
  return C.copy_out(O.cell_off, O.cell_lag, O.cell_block, O.cell_pairs, O.cell_first, O.cell_last, O.count);
}

// ---- the extraction of the fused calls ----------------------------------------------------------------------------------------
// the three times of a fused call (each may be NULL), zeroed: the first write of the call.  A call that times anything hands
// the cores a place for both of their times
struct rp_times {
  float *extract, *p, *c, spare[2] = {0.f, 0.f};
  bool timed;
  rp_times(float* ms_extract, float* ms_pairs, float* ms_cells)
      : extract(ms_extract), p(ms_pairs), c(ms_cells), timed(ms_extract || ms_pairs || ms_cells) {
    if (extract) *extract = 0.f;
    if (p) *p = 0.f;
    if (c) *c = 0.f;
  }
  float* pairs() { return timed ? (p ? p : &spare[0]) : nullptr; }
  float* cells() { return timed ? (c ? c : &spare[1]) : nullptr; }
};
// the clips fingerprinted into the library's own columns (shz_extract_owned), timed; fewer than 2^32 hashes
static int32_t rp_extract(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, uint32_t fs,
                          double amp_min, uint32_t fan_value, uint32_t flags, rp_times& T, uint64_t* hash_off, const uint32_t** d_key,
                          const uint32_t** d_t1) {
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  if (T.timed) {
    for (hipEvent_t& e : ctx->rp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], ctx->stream));
  }
  SHZ_TRY(shz_extract_owned(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags & SHZ_PCM_DEVICE, hash_off, d_key, d_t1));
  if (T.timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->rp_ev[1]));
    if (T.extract) SHZ_HIP(ctx, hipEventElapsedTime(T.extract, ctx->rp_ev[0], ctx->rp_ev[1]));
  }
  if (hash_off[n_clips] >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu hashes", who, (unsigned long long)hash_off[n_clips]);
  return SHZ_OK;
}

// ---- the entry points -------------------------------------------------------------------------------------------------------
extern "C" int32_t shz_repeats_hashes(shz_ctx* ctx, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off, uint32_t n_clips,
                                      const uint32_t* rec_clip0, uint32_t n_recs, uint32_t min_lag, uint32_t max_lag, uint32_t max_run,
                                      uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                                      uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                                      uint32_t* rec_hashes, uint32_t* rec_skipped_keys, uint64_t* rec_pairs, uint64_t* rec_skipped_rows,
                                      uint64_t cap_cells, uint64_t* count) {
  const char* who = "shz_repeats_hashes";
  if (!ctx) return SHZ_E_INVALID;
  const rp_params P{min_lag, max_lag, max_run, cell_shift, min_cell_pairs};
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, rec_skipped_keys, rec_pairs,
                 rec_skipped_rows, cap_cells, count};
  // everything that can be refused is refused before the first launch
  if (flags) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags must be 0", who);
  SHZ_TRY(rp_check(ctx, who, P, O));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  SHZ_TRY(rp_check_columns(ctx, who, key32, t1, hash_off, n_clips));
  const uint64_t N = hash_off[n_clips];
  if (n_recs == 0 || N == 0) {
    rp_empty(O, n_recs);
    return SHZ_OK;
  }
  rp_columns C(ctx);
  SHZ_TRY(C.upload(who, key32, t1, N));
  return rp_core(ctx, who, (const uint32_t*)C.key, (const uint32_t*)C.t1, hash_off, rec_clip0, n_recs, P, O, nullptr, nullptr);
}

extern "C" int32_t shz_repeats_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                     const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                     uint32_t min_lag, uint32_t max_lag, uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs,
                                     uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag, uint32_t* cell_block, uint32_t* cell_pairs,
                                     uint32_t* cell_first, uint32_t* cell_last, uint32_t* rec_hashes, uint32_t* rec_skipped_keys,
                                     uint64_t* rec_pairs, uint64_t* rec_skipped_rows, uint64_t cap_cells, uint64_t* count,
                                     float* ms_extract, float* ms_pairs, float* ms_cells) {
  const char* who = "shz_repeats_batch";
  if (!ctx) return SHZ_E_INVALID;
  const rp_params P{min_lag, max_lag, max_run, cell_shift, min_cell_pairs};
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, rec_skipped_keys, rec_pairs,
                 rec_skipped_rows, cap_cells, count};
  if (flags & ~SHZ_PCM_DEVICE) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE", who);
  SHZ_TRY(rp_check(ctx, who, P, O));
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  if (n_recs) SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  // (nothing is refused behind this line without a launch: the first write)
  rp_times T(ms_extract, ms_pairs, ms_cells);
  if (n_recs == 0) {
    rp_empty(O, 0);
    return SHZ_OK;
  }
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(rp_extract(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags, T, hash_off.data(), &d_key, &d_t1));
  return rp_core(ctx, who, d_key, d_t1, hash_off.data(), rec_clip0, n_recs, P, O, T.pairs(), T.cells());
}

// ---- content shared between two recordings: the join over a list of jobs (a, b) -----------------------------
// The elements, the runs and the recordings' borders are the self-join's (rp_elements).  Job j owns one ITEM per unique element
// of its recording a; an item's partners are the elements of b with its key and lag_lo <= t_b - t_a <= lag_hi, a range of b's
// run of that key.  Pair key: job_in_slice << 41 | (lag + 2^20) << 20 | t_a; from there on the cell stage is the self-join's
// with a lag field of 21 bits, and the lag leaves the library biased by SHZ_SHARED_LAG_BIAS
#define SH_MAX_JOBS 4096u
#define SH_LAG_BITS 21

struct sh_params {
  int32_t lag_lo, lag_hi;
  uint32_t max_run, cell_shift, min_cell_pairs;
};
struct sh_out {
  uint64_t* cell_off;
  uint32_t *cell_lag, *cell_block, *cell_pairs, *cell_first, *cell_last, *rec_hashes, *job_skipped_keys;
  uint64_t *job_pairs, *job_skipped_rows, cap_cells, *count;
};

// Item i belongs to the last job j with item_off[j] <= i (jobs without items share their successor's offset and are never that
// one) and is element el = rec_start[a] + i - item_off[j].  b's run of the key: the elements x of [rec_start[b], rec_start[b + 1])
// with U[x] >> 20 == b << 32 | key32, by a lower and an upper bound.  A key that b lacks counts 0; one with more than max_run
// times in a or in b is a stop hash: 0, and a's run head counts the key and the rows of both runs; otherwise the partners are
// the entries of b's run with t in [t_a + lag_lo, t_a + lag_hi] cut to [0, 2^20 - 1] -- the times of a run ascend strictly --
// as [lo[i], lo[i] + cnt[i]).  job_lo / job_hi (both or neither; NULL: the call's window P.lag_lo .. P.lag_hi): a window per job,
// read once the item knows its job -- the lanes of a wave may hold jobs with different windows, nothing is uniform here
__global__ __launch_bounds__(RP_THREADS) void sh_count_kernel(const uint64_t* __restrict__ U, const uint32_t* __restrict__ head,
                                                              const uint32_t* __restrict__ pos, const uint32_t* __restrict__ run_start,
                                                              const uint32_t* __restrict__ rec_start, const uint32_t* __restrict__ item_off,
                                                              const uint32_t* __restrict__ job_a, const uint32_t* __restrict__ job_b,
                                                              const int32_t* __restrict__ job_lo, const int32_t* __restrict__ job_hi,
                                                              uint32_t n_jobs, uint32_t n_items, sh_params P, uint64_t* __restrict__ cnt,
                                                              uint32_t* __restrict__ lo_out, uint32_t* __restrict__ el_out,
                                                              uint32_t* __restrict__ skip_keys, unsigned long long* __restrict__ skip_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_items) return;
  uint32_t j = 0, jh = n_jobs;
  while (jh - j > 1) {
    const uint32_t mid = j + ((jh - j) >> 1);
    if (item_off[mid] <= i) j = mid; else jh = mid;
  }
  const uint32_t b = job_b[j], el = rec_start[job_a[j]] + (i - item_off[j]);
  const uint64_t key = U[el];
  const uint64_t want = ((uint64_t)b << 32) | (uint32_t)(key >> RP_T_BITS);
  const uint32_t b1 = rec_start[b + 1];
  uint32_t l = rec_start[b], r = b1;   // first x of b with U[x] >> 20 >= want
  while (l < r) {
    const uint32_t mid = l + ((r - l) >> 1);
    if ((U[mid] >> RP_T_BITS) < want) l = mid + 1; else r = mid;
  }
  const uint32_t rb = l;
  r = b1;                              // first x with U[x] >> 20 > want
  while (l < r) {
    const uint32_t mid = l + ((r - l) >> 1);
    if ((U[mid] >> RP_T_BITS) <= want) l = mid + 1; else r = mid;
  }
  const uint32_t re = l, m_b = re - rb;
  uint32_t first = 0, n = 0;
  if (m_b) {
    const uint32_t h = head[el], id = pos[el] + h - 1, m_a = run_start[id + 1] - run_start[id];
    if (m_a > P.max_run || m_b > P.max_run) {
      if (h) {
        atomicAdd(&skip_keys[j], 1u);
        atomicAdd(&skip_rows[j], (unsigned long long)m_a + m_b);
      }
    } else {
      const int32_t t = (int32_t)((uint32_t)key & RP_T_MASK);
      int32_t t_lo = t + (job_lo ? job_lo[j] : P.lag_lo), t_hi = t + (job_hi ? job_hi[j] : P.lag_hi);   // (|lag| < 2^20: no overflow)
      if (t_hi >= 0 && t_lo <= (int32_t)RP_T_MASK) {
        t_lo = max(t_lo, 0);
        t_hi = min(t_hi, (int32_t)RP_T_MASK);
        l = rb, r = re;                // first x with t_x >= t_lo
        while (l < r) {
          const uint32_t mid = l + ((r - l) >> 1);
          if (((uint32_t)U[mid] & RP_T_MASK) < (uint32_t)t_lo) l = mid + 1; else r = mid;
        }
        first = l;
        r = re;                        // first x with t_x > t_hi
        while (l < r) {
          const uint32_t mid = l + ((r - l) >> 1);
          if (((uint32_t)U[mid] & RP_T_MASK) <= (uint32_t)t_hi) l = mid + 1; else r = mid;
        }
        n = l - first;
      }
    }
  }
  cnt[i] = n;
  lo_out[i] = first;
  el_out[i] = el;
}

// rp_expand_kernel over items: the pairs [P0, P0 + np) of the items [x0, x1), which are those of the jobs [j0, j1), go to
// out[0 .. np).  The block finds the owner items of its first and last pair and their jobs; every lane searches its pair's owner
// between the two items and the owner's job between the two jobs
__global__ __launch_bounds__(RP_THREADS) void sh_expand_kernel(const uint64_t* __restrict__ U, const uint64_t* __restrict__ poff,
                                                               const uint32_t* __restrict__ lo, const uint32_t* __restrict__ el,
                                                               const uint32_t* __restrict__ item_off, uint32_t x0, uint32_t x1,
                                                               uint64_t P0, uint64_t np, uint32_t tile, uint32_t j0, uint32_t j1,
                                                               uint64_t* __restrict__ out) {
  const uint64_t base = (uint64_t)blockIdx.x * tile;
  if (base >= np) return;
  const uint64_t end = min(base + tile, np);
  uint32_t xA, xB, jA, jB;
  {
    const uint64_t gA = P0 + base, gB = P0 + end - 1;
    uint32_t l = x0, h = x1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= gA) l = mid; else h = mid;
    }
    xA = l;
    h = x1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= gB) l = mid; else h = mid;
    }
    xB = l;
    l = j0, h = j1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (item_off[mid] <= xA) l = mid; else h = mid;
    }
    jA = l;
    h = j1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (item_off[mid] <= xB) l = mid; else h = mid;
    }
    jB = l;
  }
  for (uint64_t p = base + threadIdx.x; p < end; p += blockDim.x) {
    const uint64_t g = P0 + p;
    uint32_t l = xA, h = xB + 1;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (poff[mid] <= g) l = mid; else h = mid;
    }
    uint32_t j = jA, jh = jB + 1;
    while (jh - j > 1) {
      const uint32_t mid = j + ((jh - j) >> 1);
      if (item_off[mid] <= l) j = mid; else jh = mid;
    }
    const uint32_t ta = (uint32_t)U[el[l]] & RP_T_MASK, tb = (uint32_t)U[lo[l] + (uint32_t)(g - poff[l])] & RP_T_MASK;
    out[p] = ((uint64_t)(j - j0) << (RP_T_BITS + SH_LAG_BITS)) | ((uint64_t)(tb + SHZ_SHARED_LAG_BIAS - ta) << RP_T_BITS) | ta;
  }
}

static int32_t sh_check(shz_ctx* ctx, const char* who, const sh_params& P, const sh_out& O, const uint32_t* job_a, const uint32_t* job_b,
                        uint32_t n_jobs, uint32_t n_recs) {
  if (!O.count || !O.cell_off || !O.rec_hashes || !O.job_pairs || !O.job_skipped_keys || !O.job_skipped_rows)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: count, cell_off, rec_hashes or a job_* array is NULL", who);
  if (O.cap_cells && (!O.cell_lag || !O.cell_block || !O.cell_pairs || !O.cell_first || !O.cell_last))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL cell array with room for %llu cells", who, (unsigned long long)O.cap_cells);
  const int32_t most = (int32_t)RP_T_MASK;
  if (P.lag_lo < -most || P.lag_hi > most)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: the lag window [%d, %d] must lie in [-(2^20 - 1), 2^20 - 1]", who, P.lag_lo, P.lag_hi);
  if (P.lag_hi < P.lag_lo) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: lag_hi %d is below lag_lo %d", who, P.lag_hi, P.lag_lo);
  SHZ_TRY(rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs));
  if (n_jobs > SH_MAX_JOBS) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %u jobs in one call, at most %u", who, n_jobs, SH_MAX_JOBS);
  if (n_jobs && (!job_a || !job_b)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL job list with %u jobs", who, n_jobs);
  for (uint32_t j = 0; j < n_jobs; ++j) {
    if (job_a[j] >= n_recs || job_b[j] >= n_recs)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u names the recordings %u and %u of %u", who, j, job_a[j], job_b[j], n_recs);
    if (job_a[j] == job_b[j])
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u joins recording %u with itself (that is shz_repeats_*)", who, j, job_a[j]);
  }
  return SHZ_OK;
}
static void sh_empty(const sh_out& O, uint32_t n_recs, uint32_t n_jobs) {
  *O.count = 0;
  for (uint32_t j = 0; j <= n_jobs; ++j) O.cell_off[j] = 0;
  for (uint32_t r = 0; r < n_recs; ++r) O.rec_hashes[r] = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    O.job_skipped_keys[j] = 0;
    O.job_pairs[j] = O.job_skipped_rows[j] = 0;
  }
}

// The core on device columns, as rp_core: everything is checked (sh_check, rp_check_recs), the outputs are written when the call
// ends with SHZ_OK or SHZ_E_CAPACITY.  job_lag_lo / job_lag_hi (host, both or neither; NULL: P's window for every job): the
// window of every job, checked by the caller
static int32_t sh_core(shz_ctx* ctx, const char* who, const uint32_t* d_key32, const uint32_t* d_t1, const uint64_t* hash_off,
                       const uint32_t* rec_clip0, uint32_t n_recs, const uint32_t* job_a, const uint32_t* job_b, uint32_t n_jobs,
                       const sh_params& P, const sh_out& O, float* ms_pairs, float* ms_cells, const int32_t* job_lag_lo = nullptr,
                       const int32_t* job_lag_hi = nullptr) {
  const uint64_t N = n_recs ? hash_off[rec_clip0[n_recs]] : 0;
  if (N == 0) {
    sh_empty(O, n_recs, n_jobs);
    return SHZ_OK;
  }
  const bool small = (ctx->debug & SHZ_DEBUG_REPEAT_SMALL_SLICES) != 0, timed = ms_pairs || ms_cells;
  const uint32_t bs = small ? RP_SMALL : RP_THREADS, tile = small ? RP_SMALL : RP_TILE;
  hipStream_t st = ctx->stream;
  float pairs_ms = 0.f, cells_ms = 0.f;
  if (timed) {
    for (hipEvent_t& e : ctx->rp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], st));
  }
  // the block of the recordings and jobs: tot[4] | rec_off | job_po | skip_rows (u64) | rec_start | item_off | job_a | job_b |
  // skip_keys (u32) | with a window per job: lag_lo | lag_hi (i32).  rec_off and the jobs go up, item_off follows once the borders
  // are known, the rest comes back in one copy
  const bool windows = job_lag_lo && job_lag_hi;
  const uint64_t nr1 = (uint64_t)n_recs + 1, nj1 = (uint64_t)n_jobs + 1;
  const uint64_t o_off = 4, o_po = o_off + nr1, o_rows = o_po + nj1, n64 = o_rows + n_jobs;
  const uint64_t blk_bytes = n64 * 8 + (nr1 + nj1 + (windows ? 5ull : 3ull) * n_jobs) * 4;
  std::vector<uint64_t> hblk((size_t)((blk_bytes + 7) / 8), 0);
  uint32_t *h_rec_start = (uint32_t*)(hblk.data() + n64), *h_item_off = h_rec_start + nr1, *h_job_a = h_item_off + nj1,
           *h_job_b = h_job_a + n_jobs, *h_skip_keys = h_job_b + n_jobs;
  for (uint32_t r = 0; r <= n_recs; ++r) hblk[o_off + r] = hash_off[rec_clip0[r]];
  for (uint32_t j = 0; j < n_jobs; ++j) {
    h_job_a[j] = job_a[j];
    h_job_b[j] = job_b[j];
  }
  if (windows) {
    memcpy(h_skip_keys + n_jobs, job_lag_lo, (size_t)n_jobs * 4);
    memcpy(h_skip_keys + 2 * (size_t)n_jobs, job_lag_hi, (size_t)n_jobs * 4);
  }
  void* d_blk;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_REC, hblk.size() * 8, &d_blk));
  uint64_t* d64 = (uint64_t*)d_blk;
  uint64_t *d_tot = d64, *d_rec_off = d64 + o_off, *d_job_po = d64 + o_po, *d_skip_rows = d64 + o_rows;
  uint32_t *d_rec_start = (uint32_t*)(d64 + n64), *d_item_off = d_rec_start + nr1, *d_job_a = d_item_off + nj1, *d_job_b = d_job_a + n_jobs,
           *d_skip_keys = d_job_b + n_jobs;
  const int32_t *d_job_lo = windows ? (const int32_t*)(d_skip_keys + n_jobs) : nullptr, *d_job_hi = windows ? d_job_lo + n_jobs : nullptr;
  SHZ_HIP(ctx, shz_memcpy(ctx, d_blk, hblk.data(), hblk.size() * 8, hipMemcpyHostToDevice));
  // 1) .. 3) the elements, as the self-join's
  rp_elems E;
  SHZ_TRY(rp_elements(ctx, who, d_key32, d_t1, N, n_recs, d_rec_off, d_tot, d_rec_start, bs, &E));
  const uint32_t nu = E.nu;
  // 4) the items: the borders come back (the count kernel's grid needs their total on the host anyway), item_off goes up
  SHZ_HIP(ctx, shz_memcpy(ctx, h_rec_start, d_rec_start, nr1 * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  if (h_rec_start[0] != 0 || h_rec_start[n_recs] != nu)
    SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the recordings' borders do not span the %u unique hashes", who, nu);
  for (uint32_t r = 0; r < n_recs; ++r)
    if (h_rec_start[r + 1] < h_rec_start[r]) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the borders of recording %u decrease", who, r);
  std::vector<uint32_t> rec_start(h_rec_start, h_rec_start + nr1), item_off((size_t)nj1, 0);
  uint64_t ni64 = 0;
  for (uint32_t j = 0; j < n_jobs; ++j) {
    ni64 += rec_start[job_a[j] + 1] - rec_start[job_a[j]];
    if (ni64 >> 32)
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: the jobs up to %u have %llu items (unique hashes of their first recordings), a call holds 2^32 - 1",
               who, j, (unsigned long long)ni64);
    item_off[j + 1] = (uint32_t)ni64;
  }
  const uint32_t ni = (uint32_t)ni64;
  // 5) count, scan, the jobs' numbers
  void *d_lo = nullptr, *d_el = nullptr, *d_cnt, *d_poff = nullptr;
  if (ni) {
    memcpy(h_item_off, item_off.data(), nj1 * 4);
    SHZ_HIP(ctx, shz_memcpy(ctx, d_item_off, h_item_off, nj1 * 4, hipMemcpyHostToDevice));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_LO, (uint64_t)ni * 4, &d_lo));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SH_EL, (uint64_t)ni * 4, &d_el));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_CNT, (uint64_t)ni * 8, &d_cnt));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_POFF, ((uint64_t)ni + 1) * 8, &d_poff));
    hipLaunchKernelGGL(sh_count_kernel, dim3(rp_grid(ni, bs)), dim3(bs), 0, st, E.U, E.head, E.pos, E.run_start, (const uint32_t*)d_rec_start,
                       (const uint32_t*)d_item_off, (const uint32_t*)d_job_a, (const uint32_t*)d_job_b, d_job_lo, d_job_hi, n_jobs, ni, P,
                       (uint64_t*)d_cnt,
                       (uint32_t*)d_lo, (uint32_t*)d_el, d_skip_keys, (unsigned long long*)d_skip_rows);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(shz_scan_u64(ctx, (const uint64_t*)d_cnt, (uint64_t*)d_poff, ni, (uint64_t*)d_poff + ni));
    hipLaunchKernelGGL(rp_rec_pairs_kernel, dim3(rp_grid(nj1, bs)), dim3(bs), 0, st, (const uint64_t*)d_poff, (const uint32_t*)d_item_off,
                       n_jobs, d_job_po);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_HIP(ctx, shz_memcpy(ctx, hblk.data(), d_blk, hblk.size() * 8, hipMemcpyDeviceToHost));
  }
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], st));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  if (timed) {
    float a = 0.f;
    SHZ_HIP(ctx, hipEventElapsedTime(&a, ctx->rp_ev[0], ctx->rp_ev[1]));
    pairs_ms += a;
  }
  const uint64_t *job_po = hblk.data() + o_po, *skip_rows = hblk.data() + o_rows;
  if (job_po[0] != 0) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu pairs in front of the first job", who, (unsigned long long)job_po[0]);
  for (uint32_t j = 0; j < n_jobs; ++j)
    if (job_po[j + 1] < job_po[j]) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the pairs in front of job %u decrease", who, j);
  // 6) the slices: consecutive whole jobs whose two pair buffers fit 1/8 of the workspace limit
  const uint64_t max_pairs = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 8 / 16, 1), 1ull << 31);
  for (uint32_t j = 0; j < n_jobs; ++j)
    if (job_po[j + 1] - job_po[j] > max_pairs)
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED,
               "%s: job %u (recordings %u and %u) has %llu pairs, a slice holds %llu (workspace limit): narrow the lag window [%d, %d] or "
               "lower max_run (%u)",
               who, j, job_a[j], job_b[j], (unsigned long long)(job_po[j + 1] - job_po[j]), (unsigned long long)max_pairs,
               windows ? job_lag_lo[j] : P.lag_lo, windows ? job_lag_hi[j] : P.lag_hi, P.max_run);
  uint64_t np_max = 0;
  const std::vector<uint32_t> slices = rp_cut_slices(job_po, n_jobs, max_pairs, small, &np_max);
  // 7) slice by slice: expand, then the self-join's cell stage on a lag field of 21 bits
  rp_cells C(ctx, who, "job", n_jobs, O.cap_cells, bs, timed);
  SHZ_TRY(C.reserve(np_max));
  for (size_t s = 0; s + 1 < slices.size(); ++s) {
    const uint32_t j0 = slices[s], j1 = slices[s + 1];
    const uint64_t P0 = job_po[j0], np64 = job_po[j1] - P0;
    if (np64 == 0) continue;
    const uint32_t np = (uint32_t)np64;   // (<= 2^31)
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], st));
    hipLaunchKernelGGL(sh_expand_kernel, dim3(rp_grid(np, tile)), dim3(bs), 0, st, E.U, (const uint64_t*)d_poff, (const uint32_t*)d_lo,
                       (const uint32_t*)d_el, (const uint32_t*)d_item_off, item_off[j0], item_off[j1], P0, np64, tile, j0, j1, C.ka);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(C.slice(d_tot, np, P.cell_shift, P.min_cell_pairs, SH_LAG_BITS, j0, j1, &pairs_ms, &cells_ms));
  }
  // 8) the outputs
  for (uint32_t r = 0; r < n_recs; ++r) O.rec_hashes[r] = rec_start[r + 1] - rec_start[r];
  for (uint32_t j = 0; j < n_jobs; ++j) {
    O.job_pairs[j] = job_po[j + 1] - job_po[j];
    O.job_skipped_keys[j] = h_skip_keys[j];
    O.job_skipped_rows[j] = skip_rows[j];
  }
  if (ms_pairs) *ms_pairs = pairs_ms;
  if (ms_cells) *ms_cells = cells_ms;
  return C.copy_out(O.cell_off, O.cell_lag, O.cell_block, O.cell_pairs, O.cell_first, O.cell_last, O.count);
}

extern "C" int32_t shz_shared_hashes(shz_ctx* ctx, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off, uint32_t n_clips,
                                     const uint32_t* rec_clip0, uint32_t n_recs, const uint32_t* job_a, const uint32_t* job_b,
                                     uint32_t n_jobs, int32_t lag_lo, int32_t lag_hi, uint32_t max_run, uint32_t cell_shift,
                                     uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag, uint32_t* cell_block,
                                     uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last, uint32_t* rec_hashes,
                                     uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows, uint64_t cap_cells,
                                     uint64_t* count) {
  const char* who = "shz_shared_hashes";
  if (!ctx) return SHZ_E_INVALID;
  const sh_params P{lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs};
  const sh_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  if (flags) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags must be 0", who);
  SHZ_TRY(sh_check(ctx, who, P, O, job_a, job_b, n_jobs, n_recs));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  SHZ_TRY(rp_check_columns(ctx, who, key32, t1, hash_off, n_clips));
  const uint64_t N = hash_off[n_clips];
  if (n_recs == 0 || N == 0) {
    sh_empty(O, n_recs, n_jobs);
    return SHZ_OK;
  }
  rp_columns C(ctx);
  SHZ_TRY(C.upload(who, key32, t1, N));
  return sh_core(ctx, who, (const uint32_t*)C.key, (const uint32_t*)C.t1, hash_off, rec_clip0, n_recs, job_a, job_b, n_jobs, P, O, nullptr,
                 nullptr);
}

extern "C" int32_t shz_shared_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, const uint32_t* rec_clip0,
                                    uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value, const uint32_t* job_a,
                                    const uint32_t* job_b, uint32_t n_jobs, int32_t lag_lo, int32_t lag_hi, uint32_t max_run,
                                    uint32_t cell_shift, uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                                    uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                                    uint32_t* rec_hashes, uint64_t* job_pairs, uint32_t* job_skipped_keys, uint64_t* job_skipped_rows,
                                    uint64_t cap_cells, uint64_t* count, float* ms_extract, float* ms_pairs, float* ms_cells) {
  const char* who = "shz_shared_batch";
  if (!ctx) return SHZ_E_INVALID;
  const sh_params P{lag_lo, lag_hi, max_run, cell_shift, min_cell_pairs};
  const sh_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  if (flags & ~SHZ_PCM_DEVICE) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE", who);
  SHZ_TRY(sh_check(ctx, who, P, O, job_a, job_b, n_jobs, n_recs));
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  if (n_recs) SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  // (nothing is refused behind this line without a launch: the first write)
  rp_times T(ms_extract, ms_pairs, ms_cells);
  if (n_recs == 0) {
    sh_empty(O, 0, 0);   // (without recordings sh_check let no job through)
    return SHZ_OK;
  }
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(rp_extract(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags, T, hash_off.data(), &d_key, &d_t1));
  return sh_core(ctx, who, d_key, d_t1, hash_off.data(), rec_clip0, n_recs, job_a, job_b, n_jobs, P, O, T.pairs(), T.cells());
}

// ---- ALTERED content shared between recordings: the join at a table of warps -----------------------------------
// Job j = (a, b, v, lag_lo, lag_hi): what of recording a, played tempo[v] / 65536 times as fast and sounding pitch[v] / 65536 times
// as high as b's copy, airs in b.  Nothing of the join is new: ONE warp pass in the job form (sp_count_jobs / sp_write, DESIGN.md
// 3.7n) pairs and hashes every clip at (65536, 65536) and the clips of every distinct (a, v) at its warp, whole peak ranges; its
// CSR over the warp jobs is the CSR of VIRTUAL clips, the plain recordings own the first n_clips of them and the k-th distinct
// (a, v) owns the next run as virtual recording n_recs + k; sh_core joins (virtual(a, v), b) with the window of its job.  The
// warped columns lie in SHZ_WS_SP_KEY / _T1, which no stage of the join touches.
#define SW_W_END (1ull << 40)   // above every warped time: a warp job keeps all peaks of its clip

struct sw_jobs {                // the job list of a call and the table it points into (host)
  const uint32_t *a, *b, *v;
  const int32_t *lo, *hi;
  uint32_t n;
  const uint32_t *tempo, *pitch;
  uint32_t n_warps;
};
struct sw_plan {
  std::vector<uint32_t> va_rec, va_warp;   // the distinct (a, v) in the order of their first job
  std::vector<uint32_t> job_virt;          // the virtual recording n_recs + k of every job
};

// what both entry points refuse about the outputs, the knobs, the table and the jobs: SHZ_E_INVALID first, then the limits that
// depend on the counts alone.  P's window is not read
static int32_t sw_check(shz_ctx* ctx, const char* who, const sh_params& P, const sh_out& O, const uint32_t* job_hashes, const sw_jobs& J,
                        uint32_t n_recs, uint32_t fan_value) {
  if (!O.count || !O.cell_off || !O.rec_hashes || !O.job_pairs || !O.job_skipped_keys || !O.job_skipped_rows || !job_hashes)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: count, cell_off, rec_hashes or a job_* array is NULL", who);
  if (O.cap_cells && (!O.cell_lag || !O.cell_block || !O.cell_pairs || !O.cell_first || !O.cell_last))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL cell array with room for %llu cells", who, (unsigned long long)O.cap_cells);
  SHZ_TRY(rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs));
  SHZ_TRY(sp_check_ladder(ctx, who, "n_warps", "tempo", J.tempo, "pitch", J.pitch, J.n_warps, fan_value));
  if (J.n && (!J.a || !J.b || !J.v || !J.lo || !J.hi)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL job array with %u jobs", who, J.n);
  const int32_t most = (int32_t)RP_T_MASK;
  for (uint32_t j = 0; j < J.n && j < SH_MAX_JOBS; ++j) {
    if (J.a[j] >= n_recs || J.b[j] >= n_recs)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u names the recordings %u and %u of %u", who, j, J.a[j], J.b[j], n_recs);
    if (J.v[j] >= J.n_warps) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u names warp %u of %u", who, j, J.v[j], J.n_warps);
    if (J.lo[j] < -most || J.hi[j] > most)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: the lag window [%d, %d] of job %u must lie in [-(2^20 - 1), 2^20 - 1]", who, J.lo[j], J.hi[j], j);
    if (J.hi[j] < J.lo[j]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u: lag_hi %d is below lag_lo %d", who, j, J.hi[j], J.lo[j]);
  }
  if (J.n > SH_MAX_JOBS) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %u jobs in one call, at most %u", who, J.n, SH_MAX_JOBS);
  return SHZ_OK;
}

// the distinct (a, v) of the jobs; more than 4,096 virtual recordings: SHZ_E_UNSUPPORTED
static int32_t sw_plan_jobs(shz_ctx* ctx, const char* who, const sw_jobs& J, uint32_t n_recs, sw_plan* L) {
  std::vector<std::pair<uint64_t, uint32_t>> idx;   // a << 32 | v, sorted, beside its k
  L->job_virt.resize(J.n);
  for (uint32_t j = 0; j < J.n; ++j) {
    const uint64_t key = ((uint64_t)J.a[j] << 32) | J.v[j];
    auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(key, 0u));
    if (it == idx.end() || it->first != key) {
      it = idx.insert(it, std::make_pair(key, (uint32_t)L->va_rec.size()));
      L->va_rec.push_back(J.a[j]);
      L->va_warp.push_back(J.v[j]);
    }
    L->job_virt[j] = n_recs + it->second;
  }
  if ((uint64_t)n_recs + L->va_rec.size() > RP_MAX_RECS)
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED,
             "%s: %u recordings and %llu distinct (recording, warp) pairs in one call, at most %u together (a warped recording "
             "is a recording of the join)", who, n_recs, (unsigned long long)L->va_rec.size(), RP_MAX_RECS);
  return SHZ_OK;
}

// last[c]: the largest frame a peak of clip c can have.  The clips of every distinct (a, v) must stay below 2^20 after the warp
static int32_t sw_check_times(shz_ctx* ctx, const char* who, const uint64_t* last, const uint8_t* has, const uint32_t* rec_clip0,
                              const sw_jobs& J, const sw_plan& L) {
  for (size_t k = 0; k < L.va_rec.size(); ++k) {
    const uint32_t a = L.va_rec[k], t16 = J.tempo[L.va_warp[k]];
    for (uint32_t c = rec_clip0[a]; c < rec_clip0[a + 1]; ++c) {
      if (!has[c]) continue;
      const uint64_t w = (last[c] * t16 + 32768u) >> 16;
      if (w >> RP_T_BITS)
        SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: frame %llu of clip %u (recording %u) lies at %llu at tempo %u / 65536 (warp %u); warped "
                 "times must be below 2^20", who, (unsigned long long)last[c], c, a, (unsigned long long)w, t16, L.va_warp[k]);
    }
  }
  return SHZ_OK;
}

static void sw_empty(const sh_out& O, uint32_t* job_hashes, uint32_t n_recs, uint32_t n_jobs) {
  sh_empty(O, n_recs, n_jobs);
  for (uint32_t j = 0; j < n_jobs; ++j) job_hashes[j] = 0;
}

// The core on device peak lists (d_pf / d_pt, peak_off their host CSR from 0 over the clips, at least one peak): everything is
// checked.  ms_warp (may be NULL) gets the warp pass's stream interval (rp_ev[0] .. rp_ev[1], the read-backs of the job ranges and
// of the CSR inside it)
static int32_t sw_core(shz_ctx* ctx, const char* who, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* peak_off, uint32_t n_clips,
                       const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fan_value, const sw_jobs& J, const sw_plan& L, const sh_params& P,
                       const sh_out& O, uint32_t* job_hashes, float* ms_warp, float* ms_pairs, float* ms_cells) {
  hipStream_t st = ctx->stream;
  const uint32_t n_virt = n_recs + (uint32_t)L.va_rec.size();
  uint64_t n_warped = peak_off[n_clips];   // the (peak, warp) items of the pass, known before it runs
  for (size_t k = 0; k < L.va_rec.size(); ++k) n_warped += peak_off[rec_clip0[L.va_rec[k] + 1]] - peak_off[rec_clip0[L.va_rec[k]]];
  if (n_warped * std::max<uint32_t>(fan_value - 1, 1) >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu (peak, warp) items at fan_value %u in the one warp pass (32-bit offsets): fewer jobs a call",
             who, (unsigned long long)n_warped, fan_value);
  // 1) the warp jobs = the virtual clips, and the virtual recordings over them
  std::vector<sp_job> wj;
  std::vector<uint32_t> vrec((size_t)n_virt + 1);
  for (uint32_t c = 0; c < n_clips; ++c) wj.push_back(sp_job{peak_off[c], peak_off[c + 1], 0, SW_W_END, SP_S_ONE, SP_S_ONE});
  for (uint32_t r = 0; r <= n_recs; ++r) vrec[r] = rec_clip0[r];
  for (size_t k = 0; k < L.va_rec.size(); ++k) {
    const uint32_t a = L.va_rec[k], v = L.va_warp[k];
    for (uint32_t c = rec_clip0[a]; c < rec_clip0[a + 1]; ++c)
      wj.push_back(sp_job{peak_off[c], peak_off[c + 1], 0, SW_W_END, J.tempo[v], J.pitch[v]});
    vrec[n_recs + k + 1] = (uint32_t)wj.size();
  }
  if (wj.size() >> 31) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu warped clips in one call", who, (unsigned long long)wj.size());
  const uint32_t n_wj = (uint32_t)wj.size();
  // 2) one warp pass over all of them; the hashes stay on the device
  if (ms_warp) SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], st));
  std::vector<uint64_t> ho((size_t)n_wj + 1, 0);
  uint64_t n_items = 0;
  sp_pass W;
  SHZ_TRY(sp_count_jobs(ctx, d_pf, d_pt, wj.data(), n_wj, fan_value, &W, ho.data(), &n_items));
  const uint64_t total = ho[n_wj];
  if (total >> 32) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu hashes of %u plain and warped clips, a call holds 2^32 - 1", who,
                            (unsigned long long)total, n_wj);
  void *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_KEY, total * 4 + 64, &d_key));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SP_T1, total * 4 + 64, &d_t1));
  if (total) SHZ_TRY(sp_write(ctx, W, (uint32_t*)d_key, (uint32_t*)d_t1, total));
  if (ms_warp) {
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], st));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->rp_ev[1]));
    SHZ_HIP(ctx, hipEventElapsedTime(ms_warp, ctx->rp_ev[0], ctx->rp_ev[1]));
  }
  // 3) the join of (virtual(a, v), b) at the window of every job
  std::vector<uint32_t> virt_hashes((size_t)n_virt, 0);
  sh_out V = O;
  V.rec_hashes = virt_hashes.data();
  const int32_t rc = sh_core(ctx, who, (const uint32_t*)d_key, (const uint32_t*)d_t1, ho.data(), vrec.data(), n_virt, L.job_virt.data(), J.b,
                             J.n, P, V, ms_pairs, ms_cells, J.lo, J.hi);
  if (rc != SHZ_OK && rc != SHZ_E_CAPACITY) {
    (void)hipStreamSynchronize(st);   // (a refused join may have queued work that reads the columns)
    return rc;
  }
  for (uint32_t r = 0; r < n_recs; ++r) O.rec_hashes[r] = virt_hashes[r];
  for (uint32_t j = 0; j < J.n; ++j) job_hashes[j] = virt_hashes[L.job_virt[j]];
  return rc;
}

// device copies of N >= 1 host peaks for the length of a call (tests / tools)
struct sw_peaks {
  shz_ctx* ctx;
  void *f = nullptr, *t = nullptr;
  explicit sw_peaks(shz_ctx* c) : ctx(c) {}
  int32_t upload(const char* who, const uint16_t* peak_f, const uint32_t* peak_t, uint64_t N) {
    SHZ_HIP(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(&f, N * 2 + 64) != hipSuccess || hipMalloc(&t, N * 4 + 64) != hipSuccess) {
      (void)hipGetLastError();
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(%llu + %llu) failed", who, (unsigned long long)(N * 2), (unsigned long long)(N * 4));
    }
    if (shz_memcpy(ctx, f, peak_f, N * 2, hipMemcpyHostToDevice) != hipSuccess ||
        shz_memcpy(ctx, t, peak_t, N * 4, hipMemcpyHostToDevice) != hipSuccess)
      SHZ_FAIL(ctx, SHZ_E_HIP, "%s: copy of the peaks failed", who);
    return SHZ_OK;
  }
  ~sw_peaks() {
    if (f || t) (void)hipStreamSynchronize(ctx->stream);
    if (f) (void)hipFree(f);
    if (t) (void)hipFree(t);
  }
};

extern "C" int32_t shz_shared_warps_peaks(shz_ctx* ctx, const uint16_t* peak_f, const uint32_t* peak_t, const uint64_t* peak_off,
                                          uint32_t n_clips, const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fan_value,
                                          const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, const uint32_t* job_a,
                                          const uint32_t* job_b, const uint32_t* job_v, const int32_t* job_lag_lo,
                                          const int32_t* job_lag_hi, uint32_t n_jobs, uint32_t max_run, uint32_t cell_shift,
                                          uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                                          uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                                          uint32_t* rec_hashes, uint32_t* job_hashes, uint64_t* job_pairs, uint32_t* job_skipped_keys,
                                          uint64_t* job_skipped_rows, uint64_t cap_cells, uint64_t* count) {
  const char* who = "shz_shared_warps_peaks";
  if (!ctx) return SHZ_E_INVALID;
  const sh_params P{0, 0, max_run, cell_shift, min_cell_pairs};
  const sh_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  const sw_jobs J{job_a, job_b, job_v, job_lag_lo, job_lag_hi, n_jobs, tempo_q16, pitch_q16, n_warps};
  // everything that can be refused is refused before the first launch
  if (flags) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags must be 0", who);
  SHZ_TRY(sw_check(ctx, who, P, O, job_hashes, J, n_recs, fan_value));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  if (!peak_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peak_off is NULL", who);
  if (peak_off[0] != 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peak_off must start at 0 (it starts at %llu)", who, (unsigned long long)peak_off[0]);
  for (uint32_t c = 0; c < n_clips; ++c)
    if (peak_off[c + 1] < peak_off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peak_off decreases at clip %u", who, c);
  const uint64_t N = peak_off[n_clips];
  if (N && (!peak_f || !peak_t)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL peak list", who);
  std::vector<uint64_t> last((size_t)n_clips, 0);
  std::vector<uint8_t> has((size_t)n_clips, 0);
  for (uint32_t c = 0; c < n_clips; ++c)
    for (uint64_t i = peak_off[c]; i < peak_off[c + 1]; ++i) {
      if (peak_t[i] >> RP_T_BITS)
        SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peak %llu has t = %u, times must be below 2^20", who, (unsigned long long)i, peak_t[i]);
      if (peak_f[i] > SP_F_MAX)
        SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peak %llu has f = %u, the spectrogram ends at bin %u", who, (unsigned long long)i, peak_f[i], SP_F_MAX);
      if (i > peak_off[c] && (peak_t[i] < peak_t[i - 1] || (peak_t[i] == peak_t[i - 1] && peak_f[i] < peak_f[i - 1])))
        SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: peaks must be in (time asc, freq asc) order inside a clip; peak %llu breaks it", who,
                 (unsigned long long)i);
      last[c] = peak_t[i];
      has[c] = 1;
    }
  sw_plan L;
  SHZ_TRY(sw_plan_jobs(ctx, who, J, n_recs, &L));
  if (n_recs) SHZ_TRY(sw_check_times(ctx, who, last.data(), has.data(), rec_clip0, J, L));
  if (n_recs == 0 || N == 0) {
    sw_empty(O, job_hashes, n_recs, n_jobs);
    return SHZ_OK;
  }
  sw_peaks C(ctx);
  SHZ_TRY(C.upload(who, peak_f, peak_t, N));
  return sw_core(ctx, who, (const uint16_t*)C.f, (const uint32_t*)C.t, peak_off, n_clips, rec_clip0, n_recs, fan_value, J, L, P, O, job_hashes,
                 nullptr, nullptr, nullptr);
}

extern "C" int32_t shz_shared_warps_batch(shz_ctx* ctx, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                                          const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fs, double amp_min, uint32_t fan_value,
                                          const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, const uint32_t* job_a,
                                          const uint32_t* job_b, const uint32_t* job_v, const int32_t* job_lag_lo,
                                          const int32_t* job_lag_hi, uint32_t n_jobs, uint32_t max_run, uint32_t cell_shift,
                                          uint32_t min_cell_pairs, uint32_t flags, uint64_t* cell_off, uint32_t* cell_lag,
                                          uint32_t* cell_block, uint32_t* cell_pairs, uint32_t* cell_first, uint32_t* cell_last,
                                          uint32_t* rec_hashes, uint32_t* job_hashes, uint64_t* job_pairs, uint32_t* job_skipped_keys,
                                          uint64_t* job_skipped_rows, uint64_t cap_cells, uint64_t* count, float* ms_extract,
                                          float* ms_warp, float* ms_pairs, float* ms_cells) {
  const char* who = "shz_shared_warps_batch";
  if (!ctx) return SHZ_E_INVALID;
  const sh_params P{0, 0, max_run, cell_shift, min_cell_pairs};
  const sh_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  const sw_jobs J{job_a, job_b, job_v, job_lag_lo, job_lag_hi, n_jobs, tempo_q16, pitch_q16, n_warps};
  if (flags & ~SHZ_PCM_DEVICE) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE", who);
  SHZ_TRY(sw_check(ctx, who, P, O, job_hashes, J, n_recs, fan_value));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  if (n_recs) SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  sw_plan L;
  SHZ_TRY(sw_plan_jobs(ctx, who, J, n_recs, &L));
  // the frames of every clip bound its peaks' times: the plain side as it is, the warped side at its tempo
  std::vector<uint64_t> last((size_t)n_clips, 0);
  std::vector<uint8_t> has((size_t)n_clips, 1);
  uint64_t all_frames = 0;
  for (uint32_t c = 0; n_recs && c < n_clips; ++c) {
    const uint64_t fc = shz_frame_count_hop(clip_off[c + 1] - clip_off[c], ctx->hop);
    all_frames += fc;
    last[c] = fc ? fc - 1 : 0;
    if (last[c] >> RP_T_BITS)
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: clip %u has %llu frames, times must be below 2^20", who, c, (unsigned long long)fc);
  }
  if (n_recs) SHZ_TRY(sw_check_times(ctx, who, last.data(), has.data(), rec_clip0, J, L));
  // (nothing is refused behind this line without a launch: the first write)
  rp_times T(ms_extract, ms_pairs, ms_cells);
  if (ms_warp) *ms_warp = 0.f;
  if (n_recs == 0) {
    sw_empty(O, job_hashes, 0, 0);   // (without recordings sw_check let no job through)
    return SHZ_OK;
  }
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const bool timed = T.timed || ms_warp;
  float spare = 0.f;
  if (timed) {
    for (hipEvent_t& e : ctx->rp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], ctx->stream));
  }
  std::vector<uint64_t> peak_off((size_t)n_clips + 1, 0);
  const uint16_t* d_pf = nullptr;
  const uint32_t* d_pt = nullptr;
  SHZ_TRY(sp_peaks_owned(ctx, who, pcm, clip_off, n_clips, all_frames, fs, amp_min, flags & SHZ_PCM_DEVICE, peak_off.data(), &d_pf, &d_pt));
  if (timed) {
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[1], ctx->stream));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->rp_ev[1]));
    if (T.extract) SHZ_HIP(ctx, hipEventElapsedTime(T.extract, ctx->rp_ev[0], ctx->rp_ev[1]));
  }
  for (uint32_t c = n_clips; c > 0; --c) peak_off[c] -= peak_off[0];
  peak_off[0] = 0;
  if (peak_off[n_clips] == 0) {
    sw_empty(O, job_hashes, n_recs, n_jobs);
    return SHZ_OK;
  }
  return sw_core(ctx, who, d_pf, d_pt, peak_off.data(), n_clips, rec_clip0, n_recs, fan_value, J, L, P, O, job_hashes,
                 timed ? (ms_warp ? ms_warp : &spare) : nullptr, timed ? (T.pairs() ? T.pairs() : &spare) : nullptr,
                 timed ? (T.cells() ? T.cells() : &spare) : nullptr);
}

// ---- the fold: cells -> repeats, on the host ----------------------------------------------------------------------------------
// Union-find over cell indices, the smaller index the root.  A cell looks only at the cells in front of it: in every row of
// lags [lag - lag_tol, lag] the blocks [block - max_gap - 1, block + max_gap + 1], found by binary search in the sorted list --
// a row without such a cell costs one search, and every other step is a neighbour
namespace {
struct rp_find {
  std::vector<uint64_t> up;
  explicit rp_find(uint64_t n) : up((size_t)n) { std::iota(up.begin(), up.end(), 0ull); }
  uint64_t root(uint64_t x) {
    while (up[x] != x) {
      up[x] = up[up[x]];
      x = up[x];
    }
    return x;
  }
  void join(uint64_t a, uint64_t b) {
    a = root(a);
    b = root(b);
    if (a < b) up[b] = a; else up[a] = b;
  }
};
struct rp_comp {
  uint64_t pairs = 0, cur_sum = 0, best_sum = 0, root = 0;
  uint32_t first = 0xFFFFFFFFu, last = 0, lag_lo = 0, lag_hi = 0, cur_lag = 0, best_lag = 0, cells = 0;
};
}   // namespace

extern "C" int32_t shz_repeats_fold(const uint64_t* cell_off, uint32_t n_recs, const uint32_t* cell_lag, const uint32_t* cell_block,
                                    const uint32_t* cell_pairs, const uint32_t* cell_first, const uint32_t* cell_last, uint32_t lag_tol,
                                    uint32_t max_gap, uint64_t min_pairs, uint32_t* rep_rec, uint32_t* rep_lag, uint32_t* rep_lag_lo,
                                    uint32_t* rep_lag_hi, uint32_t* rep_first, uint32_t* rep_last, uint64_t* rep_pairs,
                                    uint32_t* rep_cells, uint64_t cap, uint64_t* count) {
  if (!count || !cell_off || cell_off[0] != 0) return SHZ_E_INVALID;
  for (uint32_t r = 0; r < n_recs; ++r)
    if (cell_off[r + 1] < cell_off[r]) return SHZ_E_INVALID;
  const uint64_t n = cell_off[n_recs];
  if (n && (!cell_lag || !cell_block || !cell_pairs || !cell_first || !cell_last)) return SHZ_E_INVALID;
  if (cap && (!rep_rec || !rep_lag || !rep_lag_lo || !rep_lag_hi || !rep_first || !rep_last || !rep_pairs || !rep_cells))
    return SHZ_E_INVALID;
  auto before = [&](uint64_t i, uint64_t lag, uint64_t block) {   // cell i < (lag, block)
    return cell_lag[i] < lag || (cell_lag[i] == lag && cell_block[i] < block);
  };
  for (uint32_t r = 0; r < n_recs; ++r)
    for (uint64_t i = cell_off[r]; i < cell_off[r + 1]; ++i) {
      if (i > cell_off[r] && !before(i - 1, cell_lag[i], cell_block[i])) return SHZ_E_INVALID;
      if (cell_first[i] > cell_last[i]) return SHZ_E_INVALID;
    }
  rp_find uf(n);
  const uint64_t reach = (uint64_t)max_gap + 1;
  for (uint32_t r = 0; r < n_recs; ++r) {
    const uint64_t c0 = cell_off[r];
    for (uint64_t i = c0; i < cell_off[r + 1]; ++i) {
      const uint64_t lag = cell_lag[i], block = cell_block[i];
      const uint64_t lag_lo = lag > lag_tol ? lag - lag_tol : 0, b_lo = block > reach ? block - reach : 0, b_hi = block + reach;
      uint64_t row = lag_lo;
      while (row <= lag) {
        uint64_t p = c0, hi = i;   // first cell in [c0, i) at or behind (row, b_lo)
        while (p < hi) {
          const uint64_t mid = p + ((hi - p) >> 1);
          if (before(mid, row, b_lo)) p = mid + 1; else hi = mid;
        }
        if (p >= i) break;
        if (cell_lag[p] != row) {   // the row holds no such cell: on to the row p lies in (ahead, as the list is sorted)
          row = cell_lag[p];
          continue;
        }
        for (uint64_t q = p; q < i && cell_lag[q] == row && cell_block[q] <= b_hi; ++q) uf.join(q, i);
        ++row;
      }
    }
  }
  // the components in the order of their smallest cell: sums, spans, the lag with the most pairs (cells arrive lag-ascending,
  // so a component's cells of one lag arrive together)
  std::vector<rp_comp> comps;
  std::vector<uint64_t> comp_of((size_t)n, ~0ull);
  std::vector<uint32_t> comp_rec;
  auto close_lag = [](rp_comp& c) {
    if (c.cur_sum > c.best_sum) {
      c.best_sum = c.cur_sum;
      c.best_lag = c.cur_lag;
    }
  };
  for (uint32_t r = 0; r < n_recs; ++r)
    for (uint64_t i = cell_off[r]; i < cell_off[r + 1]; ++i) {
      const uint64_t root = uf.root(i);
      if (root == i) {
        comp_of[i] = comps.size();
        comps.emplace_back();
        comps.back().root = i;
        comps.back().lag_lo = comps.back().cur_lag = comps.back().best_lag = cell_lag[i];
        comp_rec.push_back(r);
      }
      rp_comp& c = comps[comp_of[root]];
      if (cell_lag[i] != c.cur_lag) {
        close_lag(c);
        c.cur_lag = cell_lag[i];
        c.cur_sum = 0;
      }
      c.cur_sum += cell_pairs[i];
      c.pairs += cell_pairs[i];
      c.first = std::min(c.first, cell_first[i]);
      c.last = std::max(c.last, cell_last[i]);
      c.lag_hi = cell_lag[i];
      ++c.cells;
    }
  std::vector<uint64_t> keep;
  for (uint64_t k = 0; k < comps.size(); ++k) {
    close_lag(comps[k]);
    if (comps[k].pairs >= min_pairs) keep.push_back(k);
  }
  std::sort(keep.begin(), keep.end(), [&](uint64_t a, uint64_t b) {
    const rp_comp &x = comps[a], &y = comps[b];
    if (comp_rec[a] != comp_rec[b]) return comp_rec[a] < comp_rec[b];
    if (x.first != y.first) return x.first < y.first;
    if (x.best_lag != y.best_lag) return x.best_lag < y.best_lag;
    return x.root < y.root;
  });
  *count = keep.size();
  for (uint64_t k = 0; k < keep.size() && k < cap; ++k) {
    const rp_comp& c = comps[keep[k]];
    rep_rec[k] = comp_rec[keep[k]];
    rep_lag[k] = c.best_lag;
    rep_lag_lo[k] = c.lag_lo;
    rep_lag_hi[k] = c.lag_hi;
    rep_first[k] = c.first;
    rep_last[k] = c.last;
    rep_pairs[k] = c.pairs;
    rep_cells[k] = c.cells;
  }
  return keep.size() > cap ? SHZ_E_CAPACITY : SHZ_OK;
}
