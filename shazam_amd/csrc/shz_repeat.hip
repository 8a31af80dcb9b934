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
// On the host both joins (rp_core, sh_core) are the same list of stages around their own count and expand launches: the header
// block of the call (rp_header), the elements (rp_elements), the owners' pairs (rp_owner_pairs: scan, pairs in front of every
// recording or job, the one read-back) and the slices with the cells and the outputs (rp_slices, rp_cells), all timed on one
// clock (rp_clock).  The searches of the kernels are rp_last_le and rp_bound.
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
// the outputs of every call of the family.  The OWNERS of pairs and cells are the recordings (shz_repeats_*) or the jobs
// (shz_shared_*): cell_off and the owner_* arrays run over them, rec_hashes over the recordings
struct rp_out {
  uint64_t* cell_off;
  uint32_t *cell_lag, *cell_block, *cell_pairs, *cell_first, *cell_last, *rec_hashes, *owner_skipped_keys;
  uint64_t *owner_pairs, *owner_skipped_rows, cap_cells, *count;
};

static inline unsigned rp_grid(uint64_t n, uint32_t bs) { return (unsigned)((n + bs - 1) / bs); }
static inline int rp_bits(uint32_t v) {   // bits that hold the values 0 .. v
  int b = 0;
  while (v >> b) ++b;
  return b;
}

// ---- kernels ------------------------------------------------------------------------------------------------------------
// the last index i of [l, h) with a[i] <= v, in an ascending a with a[l] <= v (l when h - l < 2)
template <class T>
__device__ __forceinline__ uint32_t rp_last_le(const T* __restrict__ a, uint32_t l, uint32_t h, T v) {
  while (h - l > 1) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (a[mid] <= v) l = mid; else h = mid;
  }
  return l;
}
// the first index i of [l, r) with key(i) >= v -- past: with key(i) > v -- where key ascends over [l, r); r when there is none
template <bool past, class V, class K>
__device__ __forceinline__ uint32_t rp_bound(uint32_t l, uint32_t r, V v, K key) {
  while (l < r) {
    const uint32_t mid = l + ((r - l) >> 1);
    if (past ? key(mid) <= v : key(mid) < v) l = mid + 1; else r = mid;
  }
  return l;
}
// rec_off[n_recs + 1]: first hash of every recording; entry i belongs to the last r with rec_off[r] <= i
__global__ __launch_bounds__(RP_THREADS) void rp_compose_kernel(const uint32_t* __restrict__ key32, const uint32_t* __restrict__ t1,
                                                                const uint64_t* __restrict__ rec_off, uint32_t n_recs, uint64_t n,
                                                                uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t lo = rp_last_le(rec_off, 0u, n_recs, i);
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
  rec_start[r] = rp_bound<false>(r == n_recs ? n : 0u, n, r, [&](uint32_t x) { return (uint32_t)(U[x] >> 52); });
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
  const auto t_of = [&](uint32_t x) { return (uint32_t)U[x] & RP_T_MASK; };
  const uint32_t first = rp_bound<false>(i + 1, e, t_lo, t_of);   // first j with t_j >= t_lo
  cnt[i] = rp_bound<true>(first, e, t_hi, t_of) - first;          // behind it: first j with t_j > t_hi
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
struct rp_tile {
  uint64_t base, end;   // the block's positions
  uint32_t xA, xB;      // the owners of its first and last pair
};
__device__ __forceinline__ bool rp_tile_of(const uint64_t* __restrict__ poff, uint32_t e0, uint32_t e1, uint64_t P0, uint64_t np,
                                           uint32_t tile, rp_tile* T) {
  T->base = (uint64_t)blockIdx.x * tile;
  if (T->base >= np) return false;
  T->end = min(T->base + tile, np);
  T->xA = rp_last_le(poff, e0, e1, P0 + T->base);
  T->xB = rp_last_le(poff, T->xA, e1, P0 + T->end - 1);
  return true;
}
// the owner of the block's pair g
__device__ __forceinline__ uint32_t rp_tile_owner(const uint64_t* __restrict__ poff, const rp_tile& T, uint64_t g) {
  return rp_last_le(poff, T.xA, T.xB + 1, g);
}
__global__ __launch_bounds__(RP_THREADS) void rp_expand_kernel(const uint64_t* __restrict__ U, const uint64_t* __restrict__ poff,
                                                               const uint32_t* __restrict__ lo, uint32_t e0, uint32_t e1, uint64_t P0,
                                                               uint64_t np, uint32_t tile, uint32_t r0, uint64_t* __restrict__ out) {
  rp_tile T;
  if (!rp_tile_of(poff, e0, e1, P0, np, tile, &T)) return;
  for (uint64_t p = T.base + threadIdx.x; p < T.end; p += blockDim.x) {
    const uint64_t g = P0 + p;
    const uint32_t l = rp_tile_owner(poff, T, g);
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

// ---- what the entry points refuse before anything is launched --------------------------------------------------------------
static int32_t rp_check_knobs(shz_ctx* ctx, const char* who, uint32_t max_run, uint32_t cell_shift, uint32_t min_cell_pairs) {
  if (max_run < 2 || max_run > 1024) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_run must be in [2, 1024], got %u", who, max_run);
  if (cell_shift > 19) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: cell_shift must be at most 19, got %u", who, cell_shift);
  if (min_cell_pairs == 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: min_cell_pairs must be at least 1", who);
  return SHZ_OK;
}
// the output arrays: `needed` names the ones a call cannot do without ("count, cell_off or a rec_* array"); more_ok: what the
// caller has of them beside rp_out
static int32_t rp_check_out(shz_ctx* ctx, const char* who, const rp_out& O, const char* needed, bool more_ok = true) {
  if (!O.count || !O.cell_off || !O.rec_hashes || !O.owner_skipped_keys || !O.owner_pairs || !O.owner_skipped_rows || !more_ok)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s is NULL", who, needed);
  if (O.cap_cells && (!O.cell_lag || !O.cell_block || !O.cell_pairs || !O.cell_first || !O.cell_last))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL cell array with room for %llu cells", who, (unsigned long long)O.cap_cells);
  return SHZ_OK;
}
static int32_t rp_check(shz_ctx* ctx, const char* who, const rp_params& P, const rp_out& O) {
  SHZ_TRY(rp_check_out(ctx, who, O, "count, cell_off or a rec_* array"));
  if (P.max_lag < P.min_lag) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_lag %u is below min_lag %u", who, P.max_lag, P.min_lag);
  if (P.max_lag >= (1u << RP_T_BITS)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: max_lag must be below 2^20, got %u", who, P.max_lag);
  return rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs);
}
// a host CSR over the clips: off[n_clips + 1] (`name`) from 0 and never decreasing, and with entries the columns there
// (have_columns; `columns`: what they are called)
static int32_t rp_check_csr(shz_ctx* ctx, const char* who, const char* name, const uint64_t* off, uint32_t n_clips, bool have_columns,
                            const char* columns) {
  if (!off) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s is NULL", who, name);
  if (off[0] != 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s must start at 0 (it starts at %llu)", who, name, (unsigned long long)off[0]);
  for (uint32_t c = 0; c < n_clips; ++c)
    if (off[c + 1] < off[c]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: %s decreases at clip %u", who, name, c);
  if (off[n_clips] && !have_columns) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL %s", who, columns);
  return SHZ_OK;
}
// host columns: hash_off a CSR over the clips, fewer than 2^32 hashes, every t1 < 2^20
static int32_t rp_check_columns(shz_ctx* ctx, const char* who, const uint32_t* key32, const uint32_t* t1, const uint64_t* hash_off,
                                uint32_t n_clips) {
  SHZ_TRY(rp_check_csr(ctx, who, "hash_off", hash_off, n_clips, key32 && t1, "column"));
  const uint64_t N = hash_off[n_clips];
  if (N >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu hashes", who, (unsigned long long)N);
  for (uint64_t i = 0; i < N; ++i)
    if (t1[i] >> RP_T_BITS) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: t1[%llu] = %u, times must be below 2^20", who, (unsigned long long)i, t1[i]);
  return SHZ_OK;
}
// device copies of two host columns of N >= 1 entries (`what`: "columns", "peaks") for the length of a call (tests / tools);
// pad: bytes of room behind each
struct rp_upload {
  shz_ctx* ctx;
  void *a = nullptr, *b = nullptr;
  explicit rp_upload(shz_ctx* c) : ctx(c) {}
  int32_t upload(const char* who, const char* what, const void* ha, uint64_t bytes_a, const void* hb, uint64_t bytes_b, uint64_t pad) {
    SHZ_HIP(ctx, hipSetDevice(ctx->device));
    if (hipMalloc(&a, bytes_a + pad) != hipSuccess || hipMalloc(&b, bytes_b + pad) != hipSuccess) {
      (void)hipGetLastError();
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(%llu + %llu) failed", who, (unsigned long long)bytes_a, (unsigned long long)bytes_b);
    }
    if (shz_memcpy(ctx, a, ha, bytes_a, hipMemcpyHostToDevice) != hipSuccess ||
        shz_memcpy(ctx, b, hb, bytes_b, hipMemcpyHostToDevice) != hipSuccess)
      SHZ_FAIL(ctx, SHZ_E_HIP, "%s: copy of the %s failed", who, what);
    return SHZ_OK;
  }
  ~rp_upload() {
    if (a || b) (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
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
// what a call without hashes returns
static void rp_empty(const rp_out& O, uint32_t n_recs, uint32_t n_owners) {
  *O.count = 0;
  for (uint32_t o = 0; o <= n_owners; ++o) O.cell_off[o] = 0;
  for (uint32_t r = 0; r < n_recs; ++r) O.rec_hashes[r] = 0;
  for (uint32_t o = 0; o < n_owners; ++o) {
    O.owner_skipped_keys[o] = 0;
    O.owner_pairs[o] = O.owner_skipped_rows[o] = 0;
  }
}

// ---- the stages both joins share --------------------------------------------------------------------------------------------
// The clock of a call.  It owns ctx->rp_ev (created on first use): start() marks the stream, split(into) marks it again -- the
// interval since the mark before belongs to *into -- and lap(into) is a split that waits for its mark and adds every interval
// since start() to its place.  into may be NULL: that interval is dropped.  A clock that is off does none of this, waiting included
struct rp_clock {
  shz_ctx* ctx;
  bool on;
  int n = 0;   // marks behind start(): rp_ev[1 .. n]
  float* into[2] = {nullptr, nullptr};
  rp_clock(shz_ctx* c, bool on_) : ctx(c), on(on_) {}
  int32_t start() {
    if (!on) return SHZ_OK;
    for (hipEvent_t& e : ctx->rp_ev)
      if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
    n = 0;
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[0], ctx->stream));
    return SHZ_OK;
  }
  int32_t split(float* a) {
    if (!on) return SHZ_OK;
    if (n >= 2) SHZ_FAIL(ctx, SHZ_E_STATE, "rp_clock: three marks behind one start");
    into[n++] = a;
    SHZ_HIP(ctx, hipEventRecord(ctx->rp_ev[n], ctx->stream));
    return SHZ_OK;
  }
  int32_t lap(float* a) {
    if (!on) return SHZ_OK;
    SHZ_TRY(split(a));
    SHZ_HIP(ctx, hipEventSynchronize(ctx->rp_ev[n]));
    for (int k = 0; k < n; ++k) {
      float ms = 0.f;
      SHZ_HIP(ctx, hipEventElapsedTime(&ms, ctx->rp_ev[k], ctx->rp_ev[k + 1]));
      if (into[k]) *into[k] += ms;
    }
    n = 0;
    return SHZ_OK;
  }
};
// the times a fused call returns (each may be NULL), zeroed: the first write of the call.  A call that is asked for any of them
// times every stage: at(p) is p's place, or the one spare float for a time nobody reads
struct rp_times {
  float *extract, *warp, *pairs, *cells, spare = 0.f;
  bool on;
  rp_times(float* e, float* w, float* p, float* c) : extract(e), warp(w), pairs(p), cells(c), on(e || w || p || c) {
    for (float* m : {e, w, p, c})
      if (m) *m = 0.f;
  }
  float* at(float* p) { return on ? (p ? p : &spare) : nullptr; }
};
// what the stages of one join share: the name for messages, the launch shapes (SHZ_DEBUG_REPEAT_SMALL_SLICES), the clock and the
// join's two times.  The join is timed when either time is asked for
struct rp_call {
  shz_ctx* ctx;
  const char* who;
  bool small;
  uint32_t bs, tile;
  rp_clock K;
  float *ms_pairs, *ms_cells, pairs_ms = 0.f, cells_ms = 0.f;   // where the times go at the end (may be NULL) | as they add up
  rp_call(shz_ctx* c, const char* w, float* ms_pairs_, float* ms_cells_)
      : ctx(c), who(w), small((c->debug & SHZ_DEBUG_REPEAT_SMALL_SLICES) != 0), bs(small ? RP_SMALL : RP_THREADS),
        tile(small ? RP_SMALL : RP_TILE), K(c, ms_pairs_ || ms_cells_), ms_pairs(ms_pairs_), ms_cells(ms_cells_) {}
};

// The header block of a join in SHZ_WS_RP_REC, laid out once: a field is a byte offset that holds for the host copy (h) and the
// device copy (d) alike.  The u64 fields come first, then the u32 ones, then what the caller adds before place() (u32, i32).
// The owners (recordings, jobs) own the pairs:
//   u64   tot[4]       unique elements, runs, a slice's cells, its kept cells
//         rec_off      first hash of every recording, n_recs + 1 (goes up)
//         owner_po     pairs in front of every owner, n_owners + 1
//         skip_rows    rows of the runs skipped, per owner
//   u32   rec_start    first unique element of every recording, n_recs + 1
//         skip_keys    keys skipped, per owner
// One upload and one read-back per join (up / down); a single field may travel on its own
template <class T>
struct rp_field {
  uint64_t at;
};
struct rp_header {
  shz_ctx* ctx;
  uint32_t n_recs, n_owners;
  uint64_t bytes = 0;
  std::vector<uint64_t> host;
  char* dev = nullptr;
  rp_field<uint64_t> tot, rec_off, owner_po, skip_rows;
  rp_field<uint32_t> rec_start, skip_keys;
  template <class T>
  rp_field<T> add(uint64_t n) {
    const rp_field<T> f{bytes};
    bytes += n * sizeof(T);
    return f;
  }
  rp_header(shz_ctx* c, uint32_t n_recs_, uint32_t n_owners_) : ctx(c), n_recs(n_recs_), n_owners(n_owners_) {
    tot = add<uint64_t>(4);
    rec_off = add<uint64_t>((uint64_t)n_recs + 1);
    owner_po = add<uint64_t>((uint64_t)n_owners + 1);
    skip_rows = add<uint64_t>(n_owners);
    rec_start = add<uint32_t>((uint64_t)n_recs + 1);
    skip_keys = add<uint32_t>(n_owners);
  }
  template <class T>
  T* h(rp_field<T> f) { return (T*)((char*)host.data() + f.at); }
  template <class T>
  T* d(rp_field<T> f) { return (T*)(dev + f.at); }
  // the host copy, zero but for rec_off, and the room on the device
  int32_t place(const uint64_t* hash_off, const uint32_t* rec_clip0) {
    host.assign((size_t)((bytes + 7) / 8), 0);
    for (uint32_t r = 0; r <= n_recs; ++r) h(rec_off)[r] = hash_off[rec_clip0[r]];
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_REC, host.size() * 8, &p));
    dev = (char*)p;
    return SHZ_OK;
  }
  int32_t up() {
    SHZ_HIP(ctx, shz_memcpy(ctx, dev, host.data(), host.size() * 8, hipMemcpyHostToDevice));
    return SHZ_OK;
  }
  int32_t down() {
    SHZ_HIP(ctx, shz_memcpy(ctx, host.data(), dev, host.size() * 8, hipMemcpyDeviceToHost));
    return SHZ_OK;
  }
  template <class T>
  int32_t up(rp_field<T> f, uint64_t n) {
    SHZ_HIP(ctx, shz_memcpy(ctx, d(f), h(f), n * sizeof(T), hipMemcpyHostToDevice));
    return SHZ_OK;
  }
  template <class T>
  int32_t down(rp_field<T> f, uint64_t n) {
    SHZ_HIP(ctx, shz_memcpy(ctx, h(f), d(f), n * sizeof(T), hipMemcpyDeviceToHost));
    return SHZ_OK;
  }
};

struct rp_elems {
  const uint64_t* U;                        // the unique composed hashes, sorted
  uint32_t nu;
  const uint32_t *head, *pos, *run_start;   // run heads and their scan (SHZ_WS_RP_FLAG / _SCAN), first element of every run
};
// compose, sort + unique, the recordings' borders, the runs of the N >= 1 hashes.  The header (uploaded) holds rec_off; its
// tot[0] / tot[1] get the unique elements / the runs, its rec_start the borders in U.  One host read-back (the unique count);
// the stream is busy with the runs on return
static int32_t rp_elements(rp_call& X, const uint32_t* d_key32, const uint32_t* d_t1, uint64_t N, rp_header& H, rp_elems* E) {
  shz_ctx* ctx = X.ctx;
  const char* who = X.who;
  const uint32_t bs = X.bs, n_recs = H.n_recs;
  const uint64_t* d_rec_off = H.d(H.rec_off);
  uint64_t* d_tot = H.d(H.tot);
  uint32_t* d_rec_start = H.d(H.rec_start);
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
// lie in ka (the expand, queued behind the clock's start(), wrote them); slice() sorts them on the bits from cell_shift up,
// reduces the cells and gathers the kept ones on the host, copy_out() hands them to the caller
struct rp_cells {
  rp_call& X;
  shz_ctx* ctx;
  const char *who, *what;   // the entry point, and what owns cells ("recording", "job"), for messages
  uint32_t n_owners, bs;
  uint64_t cap;
  uint64_t *ka = nullptr, *kb = nullptr;
  uint32_t *flag = nullptr, *scan = nullptr;
  std::vector<uint32_t> c_lag, c_block, c_pairs, c_first, c_last, blockbuf;
  std::vector<uint64_t> cell_off;
  uint64_t n_cells_all = 0;
  rp_cells(rp_call& x, const char* what_, uint32_t n, uint64_t cap_)
      : X(x), ctx(x.ctx), who(x.who), what(what_), n_owners(n), bs(x.bs), cap(cap_), cell_off((size_t)n + 1, 0) {}
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
  // d_tot[2] / d_tot[3]: the slice's cells / kept cells.  The owners [r0, r1) are in the slice.  The time of the expand goes to
  // the join's pairs, that of the cell stage to its cells
  int32_t slice(uint64_t* d_tot, uint32_t np, uint32_t cell_shift, uint32_t min_cell_pairs, int lag_bits, uint32_t r0, uint32_t r1) {
    hipStream_t st = ctx->stream;
    SHZ_TRY(X.K.split(&X.pairs_ms));
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
    SHZ_TRY(X.K.lap(&X.cells_ms));
    SHZ_HIP(ctx, hipStreamSynchronize(st));
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
  int32_t copy_out(const rp_out& O) {
    for (uint32_t r = 0; r < n_owners; ++r) cell_off[r + 1] += cell_off[r];
    memcpy(O.cell_off, cell_off.data(), ((size_t)n_owners + 1) * 8);
    *O.count = n_cells_all;
    const size_t nw = c_lag.size();
    if (nw) {
      memcpy(O.cell_lag, c_lag.data(), nw * 4);
      memcpy(O.cell_block, c_block.data(), nw * 4);
      memcpy(O.cell_pairs, c_pairs.data(), nw * 4);
      memcpy(O.cell_first, c_first.data(), nw * 4);
      memcpy(O.cell_last, c_last.data(), nw * 4);
    }
    if (n_cells_all > cap)
      SHZ_FAIL(ctx, SHZ_E_CAPACITY, "%s: %llu cells, room for %llu", who, (unsigned long long)n_cells_all, (unsigned long long)cap);
    return SHZ_OK;
  }
};

// the recordings' borders in U as they came back: they span the nu unique hashes and never decrease
static int32_t rp_check_borders(rp_call& X, const uint32_t* rec_start, uint32_t n_recs, uint32_t nu) {
  if (rec_start[0] != 0 || rec_start[n_recs] != nu)
    SHZ_FAIL(X.ctx, SHZ_E_STATE, "%s: the recordings' borders do not span the %u unique hashes", X.who, nu);
  for (uint32_t r = 0; r < n_recs; ++r)
    if (rec_start[r + 1] < rec_start[r]) SHZ_FAIL(X.ctx, SHZ_E_STATE, "%s: the borders of recording %u decrease", X.who, r);
  return SHZ_OK;
}

// what a count kernel writes about the n things it counts for (elements, items): the partners of i are lo[i] .. lo[i] + cnt[i];
// poff[n + 1]: the scan of cnt.  Slots SHZ_WS_RP_LO / _CNT / _POFF
struct rp_counts {
  uint32_t* lo = nullptr;
  uint64_t *cnt = nullptr, *poff = nullptr;
  int32_t reserve(shz_ctx* ctx, uint64_t n) {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_LO, n * 4, &p));
    lo = (uint32_t*)p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_CNT, n * 8, &p));
    cnt = (uint64_t*)p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RP_POFF, (n + 1) * 8, &p));
    poff = (uint64_t*)p;
    return SHZ_OK;
  }
};
// The owners' pairs.  The count kernel is queued; d_first[n_owners + 1] (device): the first of the n counted things of every
// owner.  Scan, the pairs in front of every owner, the header back in one copy; the interval since the clock's start() is the
// join's pairs time, and the stream is idle on return.  Nothing counted: nothing runs and no owner has pairs.  The offsets must
// start at 0 and never decrease
static int32_t rp_owner_pairs(rp_call& X, rp_header& H, const char* noun, const rp_counts& C, uint32_t n, const uint32_t* d_first) {
  shz_ctx* ctx = X.ctx;
  hipStream_t st = ctx->stream;
  if (n) {
    SHZ_TRY(shz_scan_u64(ctx, (const uint64_t*)C.cnt, C.poff, n, C.poff + n));
    hipLaunchKernelGGL(rp_rec_pairs_kernel, dim3(rp_grid((uint64_t)H.n_owners + 1, X.bs)), dim3(X.bs), 0, st, (const uint64_t*)C.poff,
                       d_first, H.n_owners, H.d(H.owner_po));
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(H.down());
  }
  SHZ_TRY(X.K.lap(&X.pairs_ms));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  const uint64_t* po = H.h(H.owner_po);
  if (po[0] != 0) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: %llu pairs in front of the first %s", X.who, (unsigned long long)po[0], noun);
  for (uint32_t o = 0; o < H.n_owners; ++o)
    if (po[o + 1] < po[o]) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: the pairs in front of %s %u decrease", X.who, noun, o);
  return SHZ_OK;
}

// The slices, the cells and the outputs of a join whose header is back.  Slices: consecutive whole owners whose two pair buffers
// fit 1/8 of the workspace limit.  refuse(o, pairs, max_pairs) words the refusal of an owner that has more pairs than a slice
// holds -- it names the knobs of its join -- and expand(o0, o1, P0, np, out) queues the one launch that writes the np pairs of the
// owners [o0, o1), which begin at pair P0, to out; the cell stage works on a lag field of lag_bits.  Then, and only then, the
// outputs are written: rec_hashes from the borders, the owners' numbers, the join's times, and the cells there is room for
template <class Refuse, class Expand>
static int32_t rp_slices(rp_call& X, rp_header& H, const char* noun, uint32_t cell_shift, uint32_t min_cell_pairs, int lag_bits,
                         const rp_out& O, Refuse refuse, Expand expand) {
  shz_ctx* ctx = X.ctx;
  const uint32_t n = H.n_owners;
  const uint64_t* po = H.h(H.owner_po);
  const uint64_t max_pairs = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 8 / 16, 1), 1ull << 31);
  for (uint32_t o = 0; o < n; ++o)
    if (po[o + 1] - po[o] > max_pairs) return refuse(o, po[o + 1] - po[o], max_pairs);
  uint64_t np_max = 0;
  const std::vector<uint32_t> slices = rp_cut_slices(po, n, max_pairs, X.small, &np_max);
  rp_cells C(X, noun, n, O.cap_cells);
  SHZ_TRY(C.reserve(np_max));
  for (size_t s = 0; s + 1 < slices.size(); ++s) {
    const uint32_t o0 = slices[s], o1 = slices[s + 1];
    const uint64_t P0 = po[o0], np64 = po[o1] - P0;
    if (np64 == 0) continue;
    SHZ_TRY(X.K.start());
    expand(o0, o1, P0, np64, C.ka);
    SHZ_HIP(ctx, hipGetLastError());
    SHZ_TRY(C.slice(H.d(H.tot), (uint32_t)np64 /* <= 2^31 */, cell_shift, min_cell_pairs, lag_bits, o0, o1));
  }
  const uint32_t *rec_start = H.h(H.rec_start), *skip_keys = H.h(H.skip_keys);
  const uint64_t* skip_rows = H.h(H.skip_rows);
  for (uint32_t r = 0; r < H.n_recs; ++r) O.rec_hashes[r] = rec_start[r + 1] - rec_start[r];
  for (uint32_t o = 0; o < n; ++o) {
    O.owner_pairs[o] = po[o + 1] - po[o];
    O.owner_skipped_keys[o] = skip_keys[o];
    O.owner_skipped_rows[o] = skip_rows[o];
  }
  if (X.ms_pairs) *X.ms_pairs = X.pairs_ms;
  if (X.ms_cells) *X.ms_cells = X.cells_ms;
  return C.copy_out(O);
}

// ---- the core on device columns -------------------------------------------------------------------------------------------
// d_key32 / d_t1: device columns of hash_off[n_clips] < 2^32 entries with t1 < 2^20, hash_off (host) their CSR over the clips;
// everything else is checked (rp_check, rp_check_recs; n_recs >= 1).  The outputs are written when the call ends with SHZ_OK
// or SHZ_E_CAPACITY; the stream is idle then.  ms_pairs / ms_cells (may be NULL) get the stages' hipEvent times
static int32_t rp_core(shz_ctx* ctx, const char* who, const uint32_t* d_key32, const uint32_t* d_t1, const uint64_t* hash_off,
                       const uint32_t* rec_clip0, uint32_t n_recs, const rp_params& P, const rp_out& O, float* ms_pairs,
                       float* ms_cells) {
  const uint64_t N = hash_off[rec_clip0[n_recs]];
  if (N == 0) {
    rp_empty(O, n_recs, n_recs);
    return SHZ_OK;
  }
  hipStream_t st = ctx->stream;
  rp_call X(ctx, who, ms_pairs, ms_cells);
  SHZ_TRY(X.K.start());
  // the header: the recordings own the pairs.  rec_off goes up, the rest comes back in one copy
  rp_header H(ctx, n_recs, n_recs);
  SHZ_TRY(H.place(hash_off, rec_clip0));
  SHZ_TRY(H.up());
  // 1) compose, 2) sort + unique, 3) runs
  rp_elems E;
  SHZ_TRY(rp_elements(X, d_key32, d_t1, N, H, &E));
  // 4) count, scan, the recordings' numbers
  rp_counts C;
  SHZ_TRY(C.reserve(ctx, E.nu));
  hipLaunchKernelGGL(rp_count_kernel, dim3(rp_grid(E.nu, X.bs)), dim3(X.bs), 0, st, E.U, E.head, E.pos, E.run_start, E.nu, P, C.cnt, C.lo,
                     H.d(H.skip_keys), (unsigned long long*)H.d(H.skip_rows));
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(rp_owner_pairs(X, H, "recording", C, E.nu, H.d(H.rec_start)));
  const uint32_t* rec_start = H.h(H.rec_start);
  SHZ_TRY(rp_check_borders(X, rec_start, n_recs, E.nu));
  // 5) slice by slice: expand, sort, cells; 6) the outputs
  auto refuse = [&](uint32_t r, uint64_t pairs, uint64_t max_pairs) -> int32_t {
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED,
             "%s: recording %u has %llu pairs, a slice holds %llu (workspace limit): raise min_lag (%u) or lower max_run (%u)", who, r,
             (unsigned long long)pairs, (unsigned long long)max_pairs, P.min_lag, P.max_run);
  };
  auto expand = [&](uint32_t r0, uint32_t r1, uint64_t P0, uint64_t np, uint64_t* out) {
    hipLaunchKernelGGL(rp_expand_kernel, dim3(rp_grid(np, X.tile)), dim3(X.bs), 0, st, E.U, (const uint64_t*)C.poff, (const uint32_t*)C.lo,
                       rec_start[r0], rec_start[r1], P0, np, X.tile, r0, out);
  };
  return rp_slices(X, H, "recording", P.cell_shift, P.min_cell_pairs, RP_T_BITS, O, refuse, expand);
}

// ---- the extraction of the fused calls ----------------------------------------------------------------------------------------
// extract() -- shz_extract_owned, sp_peaks_owned -- on the clock of the call: its stream interval is the call's extraction time
template <class F>
static int32_t rp_timed_extract(shz_ctx* ctx, rp_times& T, F extract) {
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  rp_clock K(ctx, T.on);
  SHZ_TRY(K.start());
  SHZ_TRY(extract());
  return K.lap(T.extract);
}
// the clips fingerprinted into the library's own columns (shz_extract_owned), timed; fewer than 2^32 hashes
static int32_t rp_extract(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips, uint32_t fs,
                          double amp_min, uint32_t fan_value, uint32_t flags, rp_times& T, uint64_t* hash_off, const uint32_t** d_key,
                          const uint32_t** d_t1) {
  SHZ_TRY(rp_timed_extract(ctx, T, [&] {
    return shz_extract_owned(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags & SHZ_PCM_DEVICE, hash_off, d_key, d_t1);
  }));
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
    rp_empty(O, n_recs, n_recs);
    return SHZ_OK;
  }
  rp_upload C(ctx);
  SHZ_TRY(C.upload(who, "columns", key32, N * 4, t1, N * 4, 0));
  return rp_core(ctx, who, (const uint32_t*)C.a, (const uint32_t*)C.b, hash_off, rec_clip0, n_recs, P, O, nullptr, nullptr);
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
  rp_times T(ms_extract, nullptr, ms_pairs, ms_cells);
  if (n_recs == 0) {
    rp_empty(O, 0, 0);
    return SHZ_OK;
  }
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(rp_extract(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags, T, hash_off.data(), &d_key, &d_t1));
  return rp_core(ctx, who, d_key, d_t1, hash_off.data(), rec_clip0, n_recs, P, O, T.at(T.pairs), T.at(T.cells));
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
  const uint32_t j = rp_last_le(item_off, 0u, n_jobs, i);
  const uint32_t b = job_b[j], el = rec_start[job_a[j]] + (i - item_off[j]);
  const uint64_t key = U[el];
  const uint64_t want = ((uint64_t)b << 32) | (uint32_t)(key >> RP_T_BITS);
  const uint32_t b1 = rec_start[b + 1];
  const auto key_of = [&](uint32_t x) { return U[x] >> RP_T_BITS; };
  const uint32_t rb = rp_bound<false>(rec_start[b], b1, want, key_of);   // first x of b with U[x] >> 20 >= want
  const uint32_t re = rp_bound<true>(rb, b1, want, key_of), m_b = re - rb;   // behind it: first x with U[x] >> 20 > want
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
        const auto t_of = [&](uint32_t x) { return (uint32_t)U[x] & RP_T_MASK; };
        first = rp_bound<false>(rb, re, (uint32_t)t_lo, t_of);        // first x with t_x >= t_lo
        n = rp_bound<true>(first, re, (uint32_t)t_hi, t_of) - first;   // behind it: first x with t_x > t_hi
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
  rp_tile T;
  if (!rp_tile_of(poff, x0, x1, P0, np, tile, &T)) return;
  const uint32_t jA = rp_last_le(item_off, j0, j1, T.xA), jB = rp_last_le(item_off, jA, j1, T.xB);
  for (uint64_t p = T.base + threadIdx.x; p < T.end; p += blockDim.x) {
    const uint64_t g = P0 + p;
    const uint32_t l = rp_tile_owner(poff, T, g), j = rp_last_le(item_off, jA, jB + 1, l);
    const uint32_t ta = (uint32_t)U[el[l]] & RP_T_MASK, tb = (uint32_t)U[lo[l] + (uint32_t)(g - poff[l])] & RP_T_MASK;
    out[p] = ((uint64_t)(j - j0) << (RP_T_BITS + SH_LAG_BITS)) | ((uint64_t)(tb + SHZ_SHARED_LAG_BIAS - ta) << RP_T_BITS) | ta;
  }
}

// job j names two recordings of the call
static int32_t sh_check_names(shz_ctx* ctx, const char* who, uint32_t j, uint32_t a, uint32_t b, uint32_t n_recs) {
  if (a >= n_recs || b >= n_recs) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u names the recordings %u and %u of %u", who, j, a, b, n_recs);
  return SHZ_OK;
}
// what the plain calls refuse about the outputs, the one window, the knobs and the jobs: the job count before the jobs.  (The
// warped calls look at their jobs first, word the window per job and let a recording meet itself: sw_check)
static int32_t sh_check(shz_ctx* ctx, const char* who, const sh_params& P, const rp_out& O, const uint32_t* job_a, const uint32_t* job_b,
                        uint32_t n_jobs, uint32_t n_recs) {
  SHZ_TRY(rp_check_out(ctx, who, O, "count, cell_off, rec_hashes or a job_* array"));
  const int32_t most = (int32_t)RP_T_MASK;
  if (P.lag_lo < -most || P.lag_hi > most)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: the lag window [%d, %d] must lie in [-(2^20 - 1), 2^20 - 1]", who, P.lag_lo, P.lag_hi);
  if (P.lag_hi < P.lag_lo) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: lag_hi %d is below lag_lo %d", who, P.lag_hi, P.lag_lo);
  SHZ_TRY(rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs));
  if (n_jobs > SH_MAX_JOBS) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %u jobs in one call, at most %u", who, n_jobs, SH_MAX_JOBS);
  if (n_jobs && (!job_a || !job_b)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL job list with %u jobs", who, n_jobs);
  for (uint32_t j = 0; j < n_jobs; ++j) {
    SHZ_TRY(sh_check_names(ctx, who, j, job_a[j], job_b[j], n_recs));
    if (job_a[j] == job_b[j])
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u joins recording %u with itself (that is shz_repeats_*)", who, j, job_a[j]);
  }
  return SHZ_OK;
}

// The core on device columns, as rp_core: everything is checked (sh_check, rp_check_recs), the outputs are written when the call
// ends with SHZ_OK or SHZ_E_CAPACITY.  job_lag_lo / job_lag_hi (host, both or neither; NULL: P's window for every job): the
// window of every job, checked by the caller
static int32_t sh_core(shz_ctx* ctx, const char* who, const uint32_t* d_key32, const uint32_t* d_t1, const uint64_t* hash_off,
                       const uint32_t* rec_clip0, uint32_t n_recs, const uint32_t* job_a, const uint32_t* job_b, uint32_t n_jobs,
                       const sh_params& P, const rp_out& O, float* ms_pairs, float* ms_cells, const int32_t* job_lag_lo = nullptr,
                       const int32_t* job_lag_hi = nullptr) {
  const uint64_t N = n_recs ? hash_off[rec_clip0[n_recs]] : 0;
  if (N == 0) {
    rp_empty(O, n_recs, n_jobs);
    return SHZ_OK;
  }
  hipStream_t st = ctx->stream;
  rp_call X(ctx, who, ms_pairs, ms_cells);
  SHZ_TRY(X.K.start());
  // the header: the jobs own the pairs, and behind its fields lie item_off | job_a | job_b (u32) | with a window per job: lag_lo |
  // lag_hi (i32).  rec_off and the jobs go up, item_off follows once the borders are known, the rest comes back in one copy
  const bool windows = job_lag_lo && job_lag_hi;
  const uint64_t nj1 = (uint64_t)n_jobs + 1;
  rp_header H(ctx, n_recs, n_jobs);
  const rp_field<uint32_t> f_item = H.add<uint32_t>(nj1), f_a = H.add<uint32_t>(n_jobs), f_b = H.add<uint32_t>(n_jobs);
  const rp_field<int32_t> f_lo = H.add<int32_t>(windows ? n_jobs : 0), f_hi = H.add<int32_t>(windows ? n_jobs : 0);
  SHZ_TRY(H.place(hash_off, rec_clip0));
  std::copy_n(job_a, n_jobs, H.h(f_a));
  std::copy_n(job_b, n_jobs, H.h(f_b));
  if (windows) {
    std::copy_n(job_lag_lo, n_jobs, H.h(f_lo));
    std::copy_n(job_lag_hi, n_jobs, H.h(f_hi));
  }
  SHZ_TRY(H.up());
  // 1) .. 3) the elements, as the self-join's
  rp_elems E;
  SHZ_TRY(rp_elements(X, d_key32, d_t1, N, H, &E));
  // 4) the items: the borders come back (the count kernel's grid needs their total on the host anyway), item_off goes up
  SHZ_TRY(H.down(H.rec_start, (uint64_t)n_recs + 1));
  SHZ_HIP(ctx, hipStreamSynchronize(st));
  const uint32_t* rec_start = H.h(H.rec_start);
  SHZ_TRY(rp_check_borders(X, rec_start, n_recs, E.nu));
  uint32_t* item_off = H.h(f_item);
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
  rp_counts C;
  void* d_el = nullptr;
  if (ni) {
    SHZ_TRY(H.up(f_item, nj1));
    SHZ_TRY(C.reserve(ctx, ni));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SH_EL, (uint64_t)ni * 4, &d_el));
    hipLaunchKernelGGL(sh_count_kernel, dim3(rp_grid(ni, X.bs)), dim3(X.bs), 0, st, E.U, E.head, E.pos, E.run_start,
                       (const uint32_t*)H.d(H.rec_start), (const uint32_t*)H.d(f_item), (const uint32_t*)H.d(f_a), (const uint32_t*)H.d(f_b),
                       windows ? (const int32_t*)H.d(f_lo) : nullptr, windows ? (const int32_t*)H.d(f_hi) : nullptr, n_jobs, ni, P, C.cnt,
                       C.lo, (uint32_t*)d_el, H.d(H.skip_keys), (unsigned long long*)H.d(H.skip_rows));
    SHZ_HIP(ctx, hipGetLastError());
  }
  SHZ_TRY(rp_owner_pairs(X, H, "job", C, ni, H.d(f_item)));
  // 6) slice by slice: expand, then the self-join's cell stage on a lag field of 21 bits; 7) the outputs
  auto refuse = [&](uint32_t j, uint64_t pairs, uint64_t max_pairs) -> int32_t {
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED,
             "%s: job %u (recordings %u and %u) has %llu pairs, a slice holds %llu (workspace limit): narrow the lag window [%d, %d] or "
             "lower max_run (%u)",
             who, j, job_a[j], job_b[j], (unsigned long long)pairs, (unsigned long long)max_pairs, windows ? job_lag_lo[j] : P.lag_lo,
             windows ? job_lag_hi[j] : P.lag_hi, P.max_run);
  };
  auto expand = [&](uint32_t j0, uint32_t j1, uint64_t P0, uint64_t np, uint64_t* out) {
    hipLaunchKernelGGL(sh_expand_kernel, dim3(rp_grid(np, X.tile)), dim3(X.bs), 0, st, E.U, (const uint64_t*)C.poff, (const uint32_t*)C.lo,
                       (const uint32_t*)d_el, (const uint32_t*)H.d(f_item), item_off[j0], item_off[j1], P0, np, X.tile, j0, j1, out);
  };
  return rp_slices(X, H, "job", P.cell_shift, P.min_cell_pairs, SH_LAG_BITS, O, refuse, expand);
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
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  if (flags) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags must be 0", who);
  SHZ_TRY(sh_check(ctx, who, P, O, job_a, job_b, n_jobs, n_recs));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  SHZ_TRY(rp_check_columns(ctx, who, key32, t1, hash_off, n_clips));
  const uint64_t N = hash_off[n_clips];
  if (n_recs == 0 || N == 0) {
    rp_empty(O, n_recs, n_jobs);
    return SHZ_OK;
  }
  rp_upload C(ctx);
  SHZ_TRY(C.upload(who, "columns", key32, N * 4, t1, N * 4, 0));
  return sh_core(ctx, who, (const uint32_t*)C.a, (const uint32_t*)C.b, hash_off, rec_clip0, n_recs, job_a, job_b, n_jobs, P, O, nullptr,
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
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  if (flags & ~SHZ_PCM_DEVICE) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags may hold SHZ_PCM_DEVICE", who);
  SHZ_TRY(sh_check(ctx, who, P, O, job_a, job_b, n_jobs, n_recs));
  if (fan_value < 1 || fan_value > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "fan_value must be in [1,64]");
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  if (n_recs) SHZ_TRY(shz_check_clip_off(ctx, clip_off, n_clips));
  // (nothing is refused behind this line without a launch: the first write)
  rp_times T(ms_extract, nullptr, ms_pairs, ms_cells);
  if (n_recs == 0) {
    rp_empty(O, 0, 0);   // (without recordings sh_check let no job through)
    return SHZ_OK;
  }
  std::vector<uint64_t> hash_off((size_t)n_clips + 1, 0);
  const uint32_t *d_key = nullptr, *d_t1 = nullptr;
  SHZ_TRY(rp_extract(ctx, who, pcm, clip_off, n_clips, fs, amp_min, fan_value, flags, T, hash_off.data(), &d_key, &d_t1));
  return sh_core(ctx, who, d_key, d_t1, hash_off.data(), rec_clip0, n_recs, job_a, job_b, n_jobs, P, O, T.at(T.pairs), T.at(T.cells));
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
static int32_t sw_check(shz_ctx* ctx, const char* who, const sh_params& P, const rp_out& O, const uint32_t* job_hashes, const sw_jobs& J,
                        uint32_t n_recs, uint32_t fan_value) {
  SHZ_TRY(rp_check_out(ctx, who, O, "count, cell_off, rec_hashes or a job_* array", job_hashes != nullptr));
  SHZ_TRY(rp_check_knobs(ctx, who, P.max_run, P.cell_shift, P.min_cell_pairs));
  SHZ_TRY(sp_check_ladder(ctx, who, "n_warps", "tempo", J.tempo, "pitch", J.pitch, J.n_warps, fan_value));
  if (J.n && (!J.a || !J.b || !J.v || !J.lo || !J.hi)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL job array with %u jobs", who, J.n);
  const int32_t most = (int32_t)RP_T_MASK;
  for (uint32_t j = 0; j < J.n && j < SH_MAX_JOBS; ++j) {
    SHZ_TRY(sh_check_names(ctx, who, j, J.a[j], J.b[j], n_recs));
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

static void sw_empty(const rp_out& O, uint32_t* job_hashes, uint32_t n_recs, uint32_t n_jobs) {
  rp_empty(O, n_recs, n_jobs);
  for (uint32_t j = 0; j < n_jobs; ++j) job_hashes[j] = 0;
}

// The core on device peak lists (d_pf / d_pt, peak_off their host CSR from 0 over the clips, at least one peak): everything is
// checked.  ms_warp (may be NULL) gets the warp pass's stream interval (a lap of the clock, the read-backs of the job ranges and
// of the CSR inside it)
static int32_t sw_core(shz_ctx* ctx, const char* who, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* peak_off, uint32_t n_clips,
                       const uint32_t* rec_clip0, uint32_t n_recs, uint32_t fan_value, const sw_jobs& J, const sw_plan& L, const sh_params& P,
                       const rp_out& O, uint32_t* job_hashes, float* ms_warp, float* ms_pairs, float* ms_cells) {
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
  rp_clock K(ctx, ms_warp != nullptr);
  SHZ_TRY(K.start());
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
  SHZ_TRY(K.lap(ms_warp));
  // 3) the join of (virtual(a, v), b) at the window of every job
  std::vector<uint32_t> virt_hashes((size_t)n_virt, 0);
  rp_out V = O;
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
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
                 job_skipped_rows, cap_cells, count};
  const sw_jobs J{job_a, job_b, job_v, job_lag_lo, job_lag_hi, n_jobs, tempo_q16, pitch_q16, n_warps};
  // everything that can be refused is refused before the first launch
  if (flags) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: flags must be 0", who);
  SHZ_TRY(sw_check(ctx, who, P, O, job_hashes, J, n_recs, fan_value));
  SHZ_TRY(rp_check_recs(ctx, who, n_clips, rec_clip0, n_recs));
  SHZ_TRY(rp_check_csr(ctx, who, "peak_off", peak_off, n_clips, peak_f && peak_t, "peak list"));
  const uint64_t N = peak_off[n_clips];
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
  rp_upload C(ctx);
  SHZ_TRY(C.upload(who, "peaks", peak_f, N * 2, peak_t, N * 4, 64));
  return sw_core(ctx, who, (const uint16_t*)C.a, (const uint32_t*)C.b, peak_off, n_clips, rec_clip0, n_recs, fan_value, J, L, P, O, job_hashes,
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
  const rp_out O{cell_off, cell_lag, cell_block, cell_pairs, cell_first, cell_last, rec_hashes, job_skipped_keys, job_pairs,
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
  rp_times T(ms_extract, ms_warp, ms_pairs, ms_cells);
  if (n_recs == 0) {
    sw_empty(O, job_hashes, 0, 0);   // (without recordings sw_check let no job through)
    return SHZ_OK;
  }
  std::vector<uint64_t> peak_off((size_t)n_clips + 1, 0);
  const uint16_t* d_pf = nullptr;
  const uint32_t* d_pt = nullptr;
  SHZ_TRY(rp_timed_extract(ctx, T, [&] {
    return sp_peaks_owned(ctx, who, pcm, clip_off, n_clips, all_frames, fs, amp_min, flags & SHZ_PCM_DEVICE, peak_off.data(), &d_pf, &d_pt);
  }));
  for (uint32_t c = n_clips; c > 0; --c) peak_off[c] -= peak_off[0];
  peak_off[0] = 0;
  if (peak_off[n_clips] == 0) {
    sw_empty(O, job_hashes, n_recs, n_jobs);
    return SHZ_OK;
  }
  return sw_core(ctx, who, d_pf, d_pt, peak_off.data(), n_clips, rec_clip0, n_recs, fan_value, J, L, P, O, job_hashes,
                 T.at(T.warp), T.at(T.pairs), T.at(T.cells));
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
