// Internal declarations shared by the libshz.so translation units (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/shz.h"

#define SHZ_FAIL(ctx, code, ...)                                   \
  do {                                                             \
    char _b[512];                                                  \
    snprintf(_b, sizeof(_b), __VA_ARGS__);                         \
    (ctx)->err = _b;                                               \
    return (code);                                                 \
  } while (0)

#define SHZ_HIP(ctx, call)                                                                       \
  do {                                                                                           \
    hipError_t _e = (call);                                                                      \
    if (_e != hipSuccess) SHZ_FAIL(ctx, SHZ_E_HIP, "%s failed: %s (%s:%d)", #call,                \
                                   hipGetErrorString(_e), __FILE__, __LINE__);                   \
  } while (0)

#define SHZ_TRY(expr)                  \
  do {                                 \
    int32_t _s = (expr);               \
    if (_s != SHZ_OK) return _s;       \
  } while (0)

static inline double now_seconds() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

struct shz_prof_rec;
// a growable device buffer owned by the ctx (scratch arena slot)
struct shz_buf {
  void* p = nullptr;
  uint64_t cap = 0;
};

enum {
  SHZ_WS_DB = 0,     // dB spectrogram [frames][row_stride] f64
  SHZ_WS_MASK,       // peak bit masks
  SHZ_WS_SCAN,       // scan outputs
  SHZ_WS_SCAN_TMP,   // scan block sums
  SHZ_WS_PEAK_F,
  SHZ_WS_PEAK_T,
  SHZ_WS_PEAK_CLIP,
  SHZ_WS_HCNT,
  SHZ_WS_HOFF,
  SHZ_WS_META,       // per-clip metadata (frame offsets, sample offsets)
  SHZ_WS_META2,
  SHZ_WS_PCM,        // staged host PCM
  SHZ_WS_KEY,
  SHZ_WS_T1,
  SHZ_WS_MISC0,
  SHZ_WS_MISC1,
  SHZ_WS_MISC2,
  SHZ_WS_MISC3,
  SHZ_WS_SORT_A,
  SHZ_WS_SORT_B,
  SHZ_WS_SORT_C,
  SHZ_WS_SORT_D,
  SHZ_WS_SORT_H,
  SHZ_WS_PCM_B,      // second PCM buffer of the chunked host upload (extract_streamed)
  SHZ_WS_CTL,        // device control block of the extraction pass (xctl)
  SHZ_WS_OFFS,       // per-clip output offsets (u64)
  SHZ_WS_UND,        // undecided cells of fp32 peak picking
  SHZ_WS_M0, SHZ_WS_M1, SHZ_WS_M2, SHZ_WS_M3, SHZ_WS_M4, SHZ_WS_M5, SHZ_WS_M6, SHZ_WS_M7,
  SHZ_WS_M8, SHZ_WS_M9,      // top-n candidates of the vote fold (M3 / M4 hold the probe's group tables until the last vote pass)
  SHZ_WS_VT0, SHZ_WS_VT1, SHZ_WS_VT2, SHZ_WS_VT3,   // vote tiles: tile starts, candidate records
  SHZ_WS_VT4,        // table of the vote passes
  SHZ_WS_VT5,        // sub-group of every expand chunk's first vote (expand by sort blocks)
  SHZ_WS_VT6,        // the bar of every query of a vote pass (vt_stream2_kernel)
  SHZ_WS_RQ_KEY, SHZ_WS_RQ_T1,   // hashes of shz_recognize_batch / shz_scan_batch between their extraction and their match (neither reserves them)
  SHZ_WS_SC_JOBS,    // shz_scan.hip, the window stage of both scans: the descriptors of a slice's recordings (the plain scan: | hash_off
                     // of the clips | its one rung behind them; a scan over warps with a selection: | the slot CSR over the slice's
                     // windows | the rung of every slot)
  SHZ_WS_SC_CTL,     // ... first entry | count | offset of every (window, rung, channel), the total behind the offsets
  SHZ_WS_SC_KEY, SHZ_WS_SC_QO,   // ... the windows of one group: key32 and t1 - window start, window-major (rung-minor)
                     // (shz_scan_extents' zone stage reuses the four SC slots once the window stage is done with them: zone
                     // descriptors | hash_off; first | count | offset of every (zone, channel); key32 and t1 - lo of the zones;
                     // shz_scan_plays, which has no window stage, uses them the same way over the CSR of its jobs)
  SHZ_WS_SP_PF, SHZ_WS_SP_PT,    // shz_speed.hip: the peaks of the clips (the extraction's, or a host list staged)
  SHZ_WS_SP_TAB,     // ... peak_off | time factors | frequency factors of the call
  SHZ_WS_SP_Q,       // ... first item | first clip of every query of a pass (the job form, shz_scan_plays: the job descriptors | the
                     // items of every job | their scan)
  SHZ_WS_SP_A, SHZ_WS_SP_B,      // ... per (peak, speed) item: keep flags, then partner counts | their scans
  SHZ_WS_SP_WF, SHZ_WS_SP_WT,    // ... the warped, compacted peaks in output order
  SHZ_WS_SP_SEG,     // ... first kept peak of every (query, speed, clip) | hash_off | totals
  SHZ_WS_SP_KEY, SHZ_WS_SP_T1,   // ... the hashes of a pass between the warp and the match
  SHZ_WS_CG_LIST,    // shz_catalog.hip: bitmap of the listed song ids | the list sorted | its slots | the list as given
  SHZ_WS_CG_BLK,     // ... hits of every block of SG_ROWS rows, then their scan
  SHZ_WS_CG_CNT,     // ... rows of every song id up to the largest listed | rows of every listed song | largest offset gathered
  SHZ_WS_RW_TAB,     // ... the row warp: CSR of the songs over their rows | time factors | frequency factors of the call (the job
                     // form: CSR of the songs | first item of every job | the jobs' songs | their time | their frequency factors)
  SHZ_WS_RW_BLK,     // ... kept items of every block of RW_ITEMS items of a slice, then their scan
  SHZ_WS_RW_CNT,     // ... kept items of every (song, warp) of a slice
  SHZ_WS_EX_SEGS,    // shz_extent.hip: the segment descriptors
  SHZ_WS_EX_QOFF,    // ... the CSR of the queries over their hashes
  SHZ_WS_EX_CAND,    // ... the candidates of the call: song ids | d_lo | d_hi | used slots of every query
  SHZ_WS_EX_CTL,     // ... control block of a sub-batch | largest offset of every query | its shift
  SHZ_WS_EX_OUT,     // ... count | q_first | q_last | t_first | t_last | histograms of every candidate
  SHZ_WS_EX_LO, SHZ_WS_EX_ROWS, SHZ_WS_EX_PO,   // ... per (element, segment): first row, rows, pairs in front of it
  SHZ_WS_SP_XTAB,    // shz_speed.hip, the extent stage of shz_recognize_warps_extents: first hash of every query's best variant in the
                     // slice's columns | the CSR of the packed queries
  SHZ_WS_SP_XKEY, SHZ_WS_SP_XT1,   // ... the hashes of the best variants of a slice, packed one query behind the other
  SHZ_WS_RP_REC,     // shz_repeat.hip: totals | first hash, first unique element, pairs in front and skip counters of every recording
  SHZ_WS_RP_U,       // ... the unique composed hashes rec << 52 | key32 << 20 | t1, sorted
  SHZ_WS_RP_FLAG, SHZ_WS_RP_SCAN,   // ... head flags and their scan: of the sorted hashes, of the runs, of a slice's sorted pairs
  SHZ_WS_RP_RUN,     // ... first element of every run (one key of one recording), the element count behind the last
  SHZ_WS_RP_LO,      // ... first partner of every element
  SHZ_WS_RP_CNT, SHZ_WS_RP_POFF,    // ... partners of every element | pairs in front of it, the total behind the last
  SHZ_WS_RP_CELL,    // ... a slice's cells: first pair | first | last | keep flag | place among the kept
  SHZ_WS_RP_OUT,     // ... a slice's kept cells: rec | lag | block | pairs | first | last
  SHZ_WS_SH_EL,      // ... the join between two recordings (shz_shared_*; it uses the RP slots with items in the place of elements and
                     // jobs in the place of recordings): the element of every item
  SHZ_WS_FS_BLK,     // shz_table.hip, the song filter (shz_set_song_filter): kept total | kept votes of every block | their scan
  SHZ_WS_FS_MAP,     // ... the set of every query of the sub-batch (shz_match_batch_sets)
  SHZ_WS_COUNT
};

struct shz_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  hipDeviceProp_t prop;
  uint64_t ws_limit = 0;
  shz_buf ws[SHZ_WS_COUNT];
  // constant tables (device)
  double* d_window = nullptr;   // hann(4096)
  double2* d_twiddle = nullptr; // W4096^k, k in [0,1024]
  int16_t* d_sine_lut = nullptr;
  double m_votes_per_hash = 0.0;   // votes per query hash of the last match sub-batch: sizes the next one before it is tried
  double win_sumsq = 0.0;
  // numpy's own tables (shz_numpy_tables): np.hanning(4096), pocketfft's twiddles exp(-2 pi i k / 4096) as its
  // sincos_2pibyn computes them, sum(window ** 2) in numpy's pairwise order -- for the fp64 path that follows numpy's
  // arithmetic operation by operation (stft_np_kernel / peak_verify_kernel)
  double* d_np_window = nullptr;
  double2* d_np_comp = nullptr;
  double np_sumsq = 0.0;
  bool np_unfused = false;       // numpy's complex product on this host has no FMA (shz_set_numpy_product)
  uint32_t hop = SHZ_HOP;          // new samples per frame: NFFT - noverlap (shz_set_overlap; the reference's wratio)
  // timers / profiling
  hipEvent_t tev[16][2];
  bool tev_init = false;
  hipEvent_t rq_ev[3] = {nullptr, nullptr, nullptr};   // shz_recognize_batch: start, extraction done, match done (created on first use)
  hipEvent_t sc_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};   // shz_scan_batch / shz_scan_speeds: start, extraction done (then: a warp begun / done); the window stage: a step begun / done, the match behind it done (created on first use)
  hipEvent_t sp_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // shz_recognize_speeds / shz_match_songs_warps / _warps_extents: start, peaks (rows) done, a slice's warp begun / done, the stage after it done (the match; in the catalogue's job form the extent pass), shz_recognize_speeds' extent pass done (created on first use)
  hipEvent_t rp_ev[3] = {nullptr, nullptr, nullptr};   // shz_repeats_* / shz_shared_*: a stage begun, the pairs done, the cells done (created on first use)
  bool profiling = false;
  float kernel_ms[8] = {0};
  uint32_t kernel_launches[8] = {0};
  std::vector<struct shz_prof_rec> prof_pending;  // recorded, not yet resolved
  std::vector<struct shz_prof_rec> prof_free;
  // match stats
  uint64_t st_rows = 0, st_pairs = 0, st_keys = 0;
  uint64_t st_spec_queued = 0, st_spec_used = 0;   // single small queries whose votes were queued ahead of the count / whose results that gave
  uint64_t st_vt_redo = 0;      // sub-batches whose vote tiles flagged an overflow and were voted again by the full sort
  uint64_t key_cap = 0;         // shz_set_key_cap: a key that holds more table rows votes for nobody (0: off)
  uint64_t st_cap_groups = 0, st_cap_pairs = 0;   // ... the (query, key) groups and the pairs it dropped in the last match call
  uint32_t debug = 0;           // SHZ_DEBUG_* (shz_set_debug): switches that force rare paths, for tests
  uint32_t vote_tol = 0;        // shz_set_vote_tolerance: neighbouring offset bins a song's aligned count sums over (0 .. 31)
  uint32_t vote_floor = 0;      // shz_set_vote_floor: every query handed to the match records a row of two histograms
  std::vector<uint32_t> floor_rows;   // ... the rows not yet taken, in query order: song_hist[32] | bin_hist[32] each (256 bytes)
  // shz_set_song_filter: one bitmap of filter_words words per set, set-major, in a device block of the context's own (not a
  // workspace slot: it outlives every call); NULL and filter_sets == 0 while no filter is set
  uint32_t* d_filter = nullptr;
  uint32_t filter_sets = 0, filter_words = 0, filter_flags = 0;
  uint64_t filter_ids = 0;      // ids listed over all sets, as given (shz_get_song_filter)
  // extraction stats: cells fp32 peak picking left undecided, of those decided on fp64 values, frames recomputed for
  // that, passes repeated with fp64 staging
  uint64_t st_und = 0, st_und_f64 = 0, st_und_ffts = 0, st_fallbacks = 0;
  uint64_t st_f64_clips = 0, st_f64_frames = 0;   // clips re-run one by one with fp64 staging (per-clip fallback), their frames
  bool stage_f64 = false;       // shz_set_stage_f64: stage fp64 power and decide ties in peak_pick (no fp32 pass)
  // pinned bounce buffers of shz_memcpy (two halves, an event each)
  void* pin[2] = {nullptr, nullptr};
  hipEvent_t pin_ev[2] = {nullptr, nullptr};
  bool pin_busy[2] = {false, false};
  hipStream_t stream_up = nullptr; // uploads of host PCM, chunk by chunk beside the kernels of the chunk before (created on first use)
  uint64_t st_up_chunks = 0, st_up_bytes = 0;   // chunks / bytes that went through that pipeline
  double st_up_copy_s = 0.0, st_up_wait_s = 0.0;   // seconds the upload thread spent copying / the main thread waited for a chunk
  shz_ctx* twin = nullptr;         // second pipeline of a dual extraction pass: own stream, own workspace (created on first use)
  hipEvent_t ev_twin = nullptr;
  void* mail = nullptr;         // shz_mailbox
  uint64_t mail_cap = 0;
  // large device blocks (table slabs, run arenas, staging columns) that a destroyed table handed back: kept for the next
  // table instead of going through hipFree + hipMalloc (shz_block_alloc / shz_block_free; shz_release_workspace drops them)
  std::vector<shz_buf> blocks;
  std::mutex blocks_mu;
};

// Copy on ctx->stream.  Host <-> device copies of 16 KB .. 64 MB go through pinned bounce buffers owned by the context
// instead of handing the caller's pages to the driver: HIP registers pageable memory of that size with the kernel
// driver for the DMA, and when the application later frees it the driver evicts and restores every queue of the
// process -- 20-28 ms in the next device call (seen as every other query batch of a stream being 6x slower).  Smaller
// copies use the runtime's own staging, larger ones amortise one such event.  H2D: the source may be reused on return;
// D2H (bounced sizes): the data is there on return.
hipError_t shz_memcpy(shz_ctx* ctx, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind);

// pinned host memory owned by the ctx for small latency-critical transfers (counts, result blocks, query uploads):
// grows to the largest request; contents are the caller's between two calls
void shz_numpy_tables_host(uint32_t n, double* window, double2* comp, double* sumsq);
int32_t shz_mailbox(shz_ctx* ctx, uint64_t bytes, void** out);

// Big blocks with reuse.  A hipFree'd gigabyte comes back from the driver scrubbed at ~40 GB/s on its next use (measured:
// the same 207 GB reservation took 0 s on untouched memory and 5 s after 70 GB had been freed in the process), so blocks
// a table gives up stay with the context.  alloc: the smallest cached block of bytes <= size <= 1.5 x bytes, else
// hipMalloc (cached blocks are dropped first if the device is short); *got = the block's real size.  Thread-safe.
hipError_t shz_block_alloc(shz_ctx* ctx, uint64_t bytes, void** out, uint64_t* got);
void shz_block_free(shz_ctx* ctx, void* p, uint64_t bytes);

// ensure ws slot has >= bytes (grow-only; contents not preserved)
int32_t shz_ws_reserve(shz_ctx* ctx, int slot, uint64_t bytes, void** out);

// profiling helpers: bracket a kernel group with events when ctx->profiling.  Events are only
// recorded here (no host sync inside a timed region); shz_get_kernel_ms drains them.
struct shz_prof_rec { hipEvent_t a, b; int which; };
void shz_prof_begin(shz_ctx* ctx, int which);
void shz_prof_end(shz_ctx* ctx);
struct shz_prof_scope {
  shz_ctx* c;
  shz_prof_scope(shz_ctx* ctx, int w) : c(ctx) { if (c->profiling) shz_prof_begin(c, w); }
  ~shz_prof_scope() { if (c->profiling) shz_prof_end(c); }
};

// ---- device primitives (shz_prims.hip) ------------------------------------------------
// exclusive scan of n u32 values -> u32 (total written to d_total if non-null, as u64).  Contract: every sum is formed in
// 32 bits (lanes, waves, block sums, the total before it is widened), so the caller keeps the grand total at or below
// 2^32 - 1; up to there every prefix and the total are exact, above it they wrap.  d_out may be d_in (the sort's digit
// tables); n = 0 writes *d_total = 0 and nothing else.
int32_t shz_scan_u32(shz_ctx* ctx, const uint32_t* d_in, uint32_t* d_out, uint64_t n, uint64_t* d_total);
// exclusive scan of popcount(mask[i]) for u64 words -> u32; the same contract: the set bits of all n words together
// number at most 2^32 - 1
int32_t shz_scan_popc64(shz_ctx* ctx, const uint64_t* d_in, uint32_t* d_out, uint64_t n, uint64_t* d_total);
// exclusive scan of n u64 values -> u64
int32_t shz_scan_u64(shz_ctx* ctx, const uint64_t* d_in, uint64_t* d_out, uint64_t n, uint64_t* d_total);
// stable LSD radix sort of u64 keys (bits [bit_lo, bit_hi)) with an optional 4- or 8-byte payload.
// keys/vals are ping-ponged between (k0,v0) and (k1,v1); *out_sel tells which pair holds the result.
int32_t shz_sort_u64(shz_ctx* ctx, uint64_t* k0, uint64_t* k1, void* v0, void* v1, int vbytes, uint64_t n,
                     int bit_lo, int bit_hi, int* out_sel);

// stable LSD radix sort of 4-byte keys on bits [bit_lo, bit_hi) (k0 <-> k1 ping-pong); the result is written to out64 as
// 8-byte keys, key + add
// segments of a segmented 4-byte sort (shz_sort_u32_seg): segment i holds the keys [qv[i], qv[i + 1]) and is cut into
// the blocks [bq[i], bq[i + 1]) of <= 4,096 or 8,192 keys (bq is filled in by the sort); no block crosses a segment border
#define SHZ_SEG_MAX 128
struct shz_seg_plan {
  uint32_t nq;
  uint32_t qv[SHZ_SEG_MAX + 1];
  uint32_t bq[SHZ_SEG_MAX + 1];
};
int32_t shz_sort_u32_seg(shz_ctx* ctx, uint32_t* k0, uint32_t* k1, uint64_t n, int bit_lo, int bit_hi, const shz_seg_plan& sp,
                         int* sel, bool hist0 = false);
uint32_t shz_seg_tile(uint64_t n);                          // keys per block the sort of n keys uses
void shz_seg_blocks(shz_seg_plan* sp, uint32_t tile);       // bq from nq, qv
int shz_seg_first_pass(int bit_lo, int bit_hi, uint32_t* dmask);   // digit width (8 or 9) and mask of the first pass
int32_t shz_sort_u32_widen(shz_ctx* ctx, uint32_t* k0, uint32_t* k1, uint64_t* out64, uint64_t n, int bit_lo, int bit_hi,
                           uint64_t add, int* sel);

// ---- match on device columns the library owns (shz_table.hip) ------------------------------
int32_t shz_match_device(shz_ctx* ctx, shz_table* t, const uint32_t* d_key32, const uint32_t* d_q_off, const uint64_t* query_off,
                         uint32_t n_queries, uint32_t topn, uint32_t flags, int64_t bias_bound, uint32_t* out_sid,
                         int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                         uint64_t* out_npairs, const uint32_t* set_of_query = nullptr);   // (host; NULL: set 0 of a song filter)
int32_t shz_match_ready(shz_ctx* ctx, shz_table* t, uint32_t topn);
// the key cap (shz_set_key_cap) on the counts of a probe, before their scan: d_vals[g * nseg + sg] of the groups g < *d_n
// (<= bound) are zeroed where the group's key holds more rows than the cap.  d_gs: first element of every group, one more
// entry behind the last (the values are rows x elements), or NULL (the values are rows).  d_ctr (or NULL): the dropped
// groups and pairs, striped (M_CAP_STRIPES in shz_table.hip).  Launches nothing while no cap is set.
int32_t shz_key_cap_apply(shz_ctx* ctx, uint64_t* d_vals, const uint32_t* d_gs, const unsigned long long* d_n, uint64_t bound,
                          uint32_t nseg, unsigned long long* d_ctr);
// the vote floor (shz_set_vote_floor): n zero rows, for a caller that skips the match because nothing is to be looked up (its
// rows must line up with its result arrays).  Nothing while the floor is off
void shz_floor_zero_rows(shz_ctx* ctx, uint64_t n);

// ---- match extents on device columns the library owns (shz_extent.hip) ------------------------------
struct ex_args {   // what every caller hands over (host arrays but the two query columns)
  uint32_t n_queries, ncand;
  const uint32_t* cand_sid;
  const int32_t *cand_dlo, *cand_dhi;
  const uint32_t* cand_n;
  uint32_t *out_count, *out_q_first, *out_q_last, *out_t_first, *out_t_last, *out_hist, *out_shift;
  // the moments of every candidate's pairs, [n_queries * ncand] each: all four NULL (not computed) or none
  uint64_t *out_sum_q = nullptr, *out_sum_u = nullptr, *out_sum_qq = nullptr, *out_sum_qu = nullptr;
};
#define EX_FIT_MAX_WIDTH 4096   // with the moments, d_hi - d_lo stays below it: q u < 2^32 and no sum but sum_qq can wrap
// what every form refuses before anything is launched: the table's state (ex_state), its offsets (ex_table_limits: a part of
// ex_check, for callers whose candidates do not exist yet when they must refuse), the candidates and outputs (ex_check; n > 0;
// with the moments asked for: all four arrays, and every used candidate narrower than EX_FIT_MAX_WIDTH)
int32_t ex_state(shz_ctx* ctx, shz_table* t, const char* who, uint32_t ncand);
int32_t ex_table_limits(shz_ctx* ctx, shz_table* t, const char* who);
int32_t ex_check(shz_ctx* ctx, shz_table* t, const char* who, const ex_args& A);
// The one path of every entry point: d_key32 / d_q_off are device columns, query_off (host) their CSR, never decreasing; the
// rest of A is checked (ex_check).  Workspace: the slots SHZ_WS_EX_*, SHZ_WS_SORT_A / _B and SHZ_WS_M1 / _M2 -- none of the
// extraction's or the scan's.  The outputs are written only when the whole call succeeded; the stream is idle then.
int32_t ex_device(shz_ctx* ctx, shz_table* t, const char* who, const uint32_t* d_key32, const uint32_t* d_q_off,
                  const uint64_t* query_off, const ex_args& A);

// ---- refusals the fused calls share (shz_recognize.hip) ------------------------------
// clip0 (`name`): the CSR of the clips over n items (`what`) -- not NULL, from 0 to n_clips, never decreasing; clip_off: not
// NULL, never decreasing.  SHZ_E_INVALID with a message otherwise
int32_t shz_check_clip0(shz_ctx* ctx, const char* name, const char* what, const uint32_t* clip0, uint32_t n, uint32_t n_clips);
int32_t shz_check_clip_off(shz_ctx* ctx, const uint64_t* clip_off, uint32_t n_clips);

// ---- extraction into buffers the library owns (shz_recognize.hip) ------------------------------
// shz_fingerprint_batch of the clips into the slots SHZ_WS_RQ_KEY / SHZ_WS_RQ_T1, sized from the frame counts
// (shz_recognize_estimate) and repeated with the room the pass asked for: *d_key / *d_t1 are the columns, hash_off[n_clips + 1]
// (host) their CSR.  flags: SHZ_PCM_DEVICE.  who: the caller's name, for messages.  No clips: nothing runs, hash_off[0] = 0.
int32_t shz_extract_owned(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                          uint32_t fs, double amp_min, uint32_t fan_value, uint32_t flags, uint64_t* hash_off,
                          const uint32_t** d_key, const uint32_t** d_t1);

// ---- the speed warp's stages (shz_speed.hip), shared with the speed-tolerant scan (shz_scan.hip) ----------------------
#define SP_S_MIN 32768u
#define SP_S_ONE 65536u
#define SP_S_MAX 131072u
#define SP_MAX_SPEEDS 1024u
struct sp_job {               // one job of the job form (sp_count_jobs): a range of one clip's peaks at a pair of its own
  uint64_t c_lo, c_hi;        // its peaks [c_lo, c_hi) in the peak lists (host: all peaks of its clip; narrowed on the device)
  uint64_t w_lo, w_end;       // the warped times it keeps: w_lo <= W(t) <= w_end
  uint32_t t16, f16;          // its time and its frequency factor (Q16)
};
struct sp_view {              // what the kernels of one pass read (device pointers)
  const uint16_t* pf;         // peaks of all clips, (clip, t asc, f asc)
  const uint32_t* pt;
  const uint64_t* poff;       // n_clips + 1
  const uint64_t* qbase;      // nq + 1: first item of every query of the pass (query q has peaks(q) x K items)
  const uint32_t* clip0;      // nq + 1: first clip of every query of the pass
  const uint32_t* tempo;      // K: the time factor of every warp
  const uint32_t* pitch;      // K: its frequency factor (the same table for a speed ladder)
  uint32_t nq, K, fan;
  uint64_t n_items;
  const sp_job* jobs = nullptr;   // the job form: nq jobs, qbase their first items, segment e of the CSR is job e; poff, clip0,
                                  // tempo and pitch are not read
};
struct sp_pass {
  sp_view V;
  uint64_t n_seg;
  uint32_t *a, *b;            // flags, then partner counts | places, then hash offsets
  uint16_t* wf;
  uint32_t *wt, *segstart;
  unsigned long long *d_hoff, *d_tot;   // hash_off[n_seg + 1] | kept peaks, hashes
};
#define SP_F_MAX 2048u          // the last bin of the spectrogram (SHZ_NBINS - 1)
__host__ __device__ __forceinline__ uint32_t sp_warp_f(uint32_t f, uint32_t s16) {
  if (f < 16384u) return ((f << 17) + s16) / (2u * s16);   // fits 32 bits: every bin of the spectrogram
  return (uint32_t)((((uint64_t)f << 17) + s16) / (2ull * s16));
}
__host__ __device__ __forceinline__ uint32_t sp_warp_t(uint32_t t, uint32_t s16) {
  const uint64_t x = ((uint64_t)t * s16 + 32768u) >> 16;
  return x > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)x;   // (t < 2^31 is the caller's promise; this keeps the value defined)
}
// items of the queries [q0, q0 + nq) at K speeds (clip0: first clip of every query)
uint64_t sp_items(const uint64_t* peak_off, const uint32_t* clip0, uint32_t q0, uint32_t nq, uint32_t K);
// one warp pass over the queries [q0, q0 + nq) at the K warps (d_tempo[v], d_pitch[v]), v in [0, K): sp_count counts
// (hash_off: n_seg + 1 entries on the host, relative to the pass, segments in the order query, warp, clip; P->d_hoff the same
// on the device; the stream is idle on return), sp_write writes (key32, t1) of the pass to device columns of cap entries.
// d_poff / d_tempo / d_pitch: the call's tables on the device (sp_upload_tables; a speed ladder gives its one table twice).
// A pass without peaks launches nothing and leaves P's pointers unset
int32_t sp_count(shz_ctx* ctx, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* d_poff, const uint64_t* peak_off,
                 const uint32_t* clip0, uint32_t q0, uint32_t nq, const uint32_t* d_tempo, const uint32_t* d_pitch, uint32_t K,
                 uint32_t fan, sp_pass* P, uint64_t* hash_off);
int32_t sp_write(shz_ctx* ctx, const sp_pass& P, uint32_t* d_key, uint32_t* d_t1, uint64_t cap);
// the same pass over a list of jobs (shz_scan_plays): hash_off has n_jobs + 1 entries, *n_items = the peak items warped
int32_t sp_count_jobs(shz_ctx* ctx, const uint16_t* d_pf, const uint32_t* d_pt, const sp_job* jobs, uint32_t n_jobs, uint32_t fan,
                      sp_pass* P, uint64_t* hash_off, uint64_t* n_items);
// steps 2-4 of shz_recognize_warps on peaks that lie on the device -- slices of whole queries (the 2^28-pair budget, 1/8 of the
// workspace limit; SHZ_DEBUG_SPEED_SMALL_SLICES), sp_count / sp_write, shz_match_device on all (query, warp) pairs of a slice,
// sp_best -- shared with the peak-window listeners (shz_stream.hip).  peak_off: host CSR from 0 over n_clips clips; t_max: the
// largest warped time (the match's bias bound); flags: SHZ_MATCH_FULL_SORT; out_nhash / out_profile may be NULL; timed:
// ms_warp / ms_match (may be NULL) get the two stages' hipEvent times
// X (may be NULL: no extent stage): the extent pass of every slice on the hashes of its queries' best variants, which exist
// on the device only until the next slice is warped -- candidate n < nres of query q is (sid, delta - w, delta + w); the
// outputs [n_queries * topn] ([... * 64] for hist, which may be NULL; [n_queries] for shift) are written when the whole call
// succeeded; ms_extent (may be NULL) gets the stage's hipEvent time with `timed`
struct sp_extent {
  uint32_t w;
  uint32_t *count, *q_first, *q_last, *t_first, *t_last;
  uint64_t *sum_q, *sum_u, *sum_qq, *sum_qu;
  uint32_t *hist, *shift;
  float* ms_extent;
};
int32_t sp_match_fold(shz_ctx* ctx, shz_table* t, const uint16_t* d_pf, const uint32_t* d_pt, const uint64_t* peak_off,
                      uint32_t n_clips, const uint32_t* query_clip0, uint32_t n_queries, uint32_t fan_value, uint32_t topn,
                      const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t K, uint32_t flags, uint64_t t_max,
                      uint32_t* out_best, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                      uint32_t* out_nres, uint32_t* out_nhash, uint32_t* out_profile, bool timed, float* ms_warp, float* ms_match,
                      const sp_extent* X = nullptr);
// what every entry point with a ladder refuses about it.  n_name: the count's argument ("n_speeds"); t_name / f_name: what a
// factor of either table is called ("speed", or "tempo" and "pitch"; the table's argument is <name>_q16).  pitch_q16 ==
// tempo_q16 is one ladder: it is checked, and named, once
int32_t sp_check_ladder(shz_ctx* ctx, const char* who, const char* n_name, const char* t_name, const uint32_t* tempo_q16,
                        const char* f_name, const uint32_t* pitch_q16, uint32_t n, uint32_t fan_value);
// peak_off | tempo | pitch on the device (one block of the call); pitch_q16 == tempo_q16: one table, *d_pitch = *d_tempo
int32_t sp_upload_tables(shz_ctx* ctx, const uint64_t* peak_off, uint32_t n_clips, const uint32_t* tempo_q16,
                         const uint32_t* pitch_q16, uint32_t K, const uint64_t** d_poff, const uint32_t** d_tempo,
                         const uint32_t** d_pitch);
uint32_t sp_best(const uint32_t* top1, const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t K);
// shz_peaks of the clips into SHZ_WS_SP_PF / SHZ_WS_SP_PT (frames: of all clips together; flags: SHZ_PCM_DEVICE)
int32_t sp_peaks_owned(shz_ctx* ctx, const char* who, const int16_t* pcm, const uint64_t* clip_off, uint32_t n_clips,
                       uint64_t frames, uint32_t fs, double amp_min, uint32_t flags, uint64_t* peak_off, const uint16_t** d_pf,
                       const uint32_t** d_pt);

// ---- RCCL helpers (shz_comm.hip) ----------------------------------------------------------
int32_t shz_comm_info(shz_comm* c, int* rank, int* nranks);
shz_ctx* shz_comm_ctx(shz_comm* c);
int32_t shz_comm_allgather_bytes(shz_comm* c, const void* d_send, void* d_recv, uint64_t bytes);
int32_t shz_comm_alltoallv_bytes(shz_comm* c, const void* d_send, const uint64_t* scount, const uint64_t* sdispl,
                                 void* d_recv, const uint64_t* rcount, const uint64_t* rdispl);
int32_t shz_comm_allgatherv_bytes(shz_comm* c, const void* d_send, void* d_recv, const uint64_t* counts,
                                  const uint64_t* displ);
// the gathered build's transport: a second stream owned by the communicator, a blocking all-gather of small host
// blocks on it, and the all-gather of lists of device buffers (see shz_comm.hip)
struct shz_xfer { void* p; uint64_t bytes; };
int32_t shz_comm_exchange_stream(shz_comm* c, hipStream_t* out);
int32_t shz_comm_allgather_bytes_on(shz_comm* c, hipStream_t s, const void* d_send, void* d_recv, uint64_t bytes);
int32_t shz_comm_allgather_host(shz_comm* c, const void* h_mine, void* h_all, uint64_t bytes);
int32_t shz_comm_allgather_lists_on(shz_comm* c, hipStream_t s, const std::vector<shz_xfer>& send,
                                    const std::vector<std::vector<shz_xfer>>& recv);
