// The catalogue's own questions: the rows of listed songs read back out of the table (SELECT hash, offset FROM fingerprints
// WHERE song_id IN (...)), and those songs matched against the rest of the table (which of my tracks are the same recording?).
//
// The gather streams the song-id column of every segment twice, 4 bytes a row each time, in blocks of SG_ROWS rows (one
// wave a block, 16 loads of 64 consecutive ids): pass 1 tests every id against a bitmap of the listed ids (128 KB for 2^20
// ids: it stays in L2), ballots the hits, writes one hit count per block and adds every hit to its song's row count; the
// block counts are scanned; pass 2 repeats the test and writes every hit in table order as a packed (slot, key32, offset),
// reading the key and offset columns only where a row hits.  The hits are then radix-sorted (stable) into (slot, key32,
// offset) order -- on the slot bits alone where the table is one segment, whose order already is (key32, offset).  The
// places come from the scan alone -- no atomic decides where a row lands, so the output is ordered and repeatable; the one
// atomic of the gather is the integer add of the per-song row counts, whose result no order changes.
// Scratch: 4 bytes per SG_ROWS rows, 8 bytes per song id up to the largest listed, and per HIT 16 bytes (32 where slot, key
// and offset do not fit one 64-bit word) that belong to the call -- the match that may follow uses the workspace.
#include "shz_table_int.h"

#define SG_ROWS 1024u   // rows of a block
#define SG_LOADS 16     // SG_ROWS / 64
#define SG_WAVES 4      // blocks (waves) of a workgroup

__device__ __forceinline__ bool sg_listed(uint32_t s, const uint32_t* __restrict__ bitmap, uint32_t last) {
  return s <= last && ((bitmap[s >> 5] >> (s & 31)) & 1u);   // tbl_sid_keep_kernel's test, the sense turned
}

// pass 1: hits of every block, rows of every listed song
__global__ __launch_bounds__(64 * SG_WAVES) void sg_count_kernel(const uint32_t* __restrict__ sid, uint64_t n,
                                                                  const uint32_t* __restrict__ bitmap, uint32_t last,
                                                                  uint32_t* __restrict__ blk_cnt,
                                                                  unsigned long long* __restrict__ song_cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  const uint64_t r0 = blk * SG_ROWS;
  if (r0 >= n) return;   // uniform in the wave
  uint32_t s[SG_LOADS];
#pragma unroll
  for (int j = 0; j < SG_LOADS; ++j) {
    const uint64_t i = r0 + (uint64_t)j * 64 + lane;
    s[j] = i < n ? sid[i] : 0u;
  }
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < SG_LOADS; ++j) {
    const uint64_t i = r0 + (uint64_t)j * 64 + lane;
    const bool hit = i < n && sg_listed(s[j], bitmap, last);
    if (hit) atomicAdd(song_cnt + s[j], 1ull);
    c += (uint32_t)__popcll(__ballot(hit));
  }
  if (lane == 0) blk_cnt[blk] = c;
}

// rows of the listed songs in list order (an id above `last` has no rows)
__global__ void sg_pick_kernel(const uint32_t* __restrict__ list, uint32_t n_ids, uint32_t last,
                               const unsigned long long* __restrict__ song_cnt, unsigned long long* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_ids) out[i] = list[i] <= last ? song_cnt[list[i]] : 0ull;
}

// pass 2: every hit, in table order, at the place the scan of the block counts gives.  PACKED: a[] = slot | key32 | offset in
// one word; else a[] = key32 | offset and b[] = slot.  ob: bits of the offset field; total: the hits of the call (no store
// beyond it)
template <bool PACKED>
__global__ __launch_bounds__(64 * SG_WAVES) void sg_write_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ sid,
                                                                  const uint32_t* __restrict__ off, uint64_t n,
                                                                  const uint32_t* __restrict__ bitmap, uint32_t last,
                                                                  const uint32_t* __restrict__ blk_pos,
                                                                  const uint32_t* __restrict__ ids, const uint32_t* __restrict__ slot_of,
                                                                  uint32_t n_ids, int ob, uint64_t total,
                                                                  uint64_t* __restrict__ a, uint64_t* __restrict__ b) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  const uint64_t r0 = blk * SG_ROWS;
  if (r0 >= n) return;   // uniform in the wave
  uint32_t s[SG_LOADS];
#pragma unroll
  for (int j = 0; j < SG_LOADS; ++j) {
    const uint64_t i = r0 + (uint64_t)j * 64 + lane;
    s[j] = i < n ? sid[i] : 0u;
  }
  uint64_t base = blk_pos[blk];
#pragma unroll
  for (int j = 0; j < SG_LOADS; ++j) {
    const uint64_t i = r0 + (uint64_t)j * 64 + lane;
    const bool hit = i < n && sg_listed(s[j], bitmap, last);
    const uint64_t m = __ballot(hit);
    if (hit) {
      const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
      uint32_t lo = 0, hi = n_ids;   // the id is in the list: the last entry <= s
      while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (ids[mid] <= s[j]) lo = mid; else hi = mid;
      }
      const uint64_t slot = slot_of[lo];
      const uint64_t ko = ((uint64_t)key[i] << ob) | off[i];
      if (pos < total) {
        if (PACKED) a[pos] = (slot << (32 + ob)) | ko;
        else { a[pos] = ko; b[pos] = slot; }
      }
    }
    base += (uint64_t)__popcll(m);
  }
}

// the sorted hits as columns; PACKED: w[] = slot | key32 | offset; else w[] = key32 | offset (the slots were the sort's keys).
// max_off (may be NULL): the largest offset written
__global__ void sg_unpack_kernel(const uint64_t* __restrict__ w, uint64_t total, int ob, uint32_t* __restrict__ key32,
                                 uint32_t* __restrict__ off, uint32_t* __restrict__ max_off) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t o = 0;
  if (i < total) {
    const uint64_t x = w[i];
    o = (uint32_t)(x & ((1ull << ob) - 1ull));
    key32[i] = (uint32_t)(x >> ob);   // (a slot above the key falls off the 32 bits)
    off[i] = o;
  }
  if (!max_off) return;
  for (int d = 32; d >= 1; d >>= 1) o = max(o, (uint32_t)__shfl_xor((int)o, d, 64));
  if ((threadIdx.x & 63) == 0 && o) atomicMax(max_off, o);
}

namespace {

// device allocations of one call, freed when it ends
struct sg_bufs {
  std::vector<void*> p;
  ~sg_bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  void* get(uint64_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<uint64_t>(bytes, 256)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    p.push_back(q);
    return q;
  }
};

struct song_gather {
  shz_table* t = nullptr;
  uint32_t n_ids = 0, last = 0;
  std::vector<shz_seg> segs;
  std::vector<uint64_t> blk0;     // first block of every segment
  uint64_t n_blk = 0, total = 0;  // blocks of all segments, hits
  uint32_t *d_bitmap = nullptr, *d_ids = nullptr, *d_slot = nullptr, *d_blk = nullptr;
};

static inline uint64_t sg_blocks(uint64_t n) { return (n + SG_ROWS - 1) / SG_ROWS; }
static inline unsigned sg_grid(uint64_t n) { return (unsigned)((sg_blocks(n) + SG_WAVES - 1) / SG_WAVES); }

// What both entry points refuse about the list, then pass 1: row_off[n_sids + 1] on the host, G ready for sg_fill.  The
// stream is idle on return.
int32_t sg_prepare(shz_table* t, const char* who, const uint32_t* sids, uint32_t n_sids, uint64_t* row_off, song_gather* G) {
  shz_ctx* ctx = t->ctx;
  if (!row_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: row_off is NULL", who);
  if (n_sids && !sids) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: sids is NULL", who);
  if (t->broken) SHZ_FAIL(ctx, SHZ_E_STATE, "table lost rows in a failed finalize");
  if (pending_rows(t)) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: table has staged rows; call shz_table_finalize first", who);
  std::vector<std::pair<uint32_t, uint32_t>> byid(n_sids);   // (id, slot)
  for (uint32_t i = 0; i < n_sids; ++i) byid[i] = {sids[i], i};
  std::sort(byid.begin(), byid.end());
  for (uint32_t i = 1; i < n_sids; ++i)
    if (byid[i].first == byid[i - 1].first) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: song id %u is listed twice", who, byid[i].first);
  G->t = t;
  G->n_ids = n_sids;
  G->total = 0;
  for (uint32_t i = 0; i <= n_sids; ++i) row_off[i] = 0;
  if (n_sids == 0 || total_rows(t) == 0 || byid[0].first > t->max_sid) return SHZ_OK;   // no listed song has a row
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  // ids above the table's largest have no rows: the bitmap ends at the largest listed id that may have some
  uint32_t last = 0;
  for (uint32_t i = 0; i < n_sids && byid[i].first <= t->max_sid; ++i) last = byid[i].first;
  G->last = last;
  const uint64_t words = (uint64_t)last / 32 + 1;
  std::vector<uint32_t> host(words + 3ull * n_sids, 0u);   // bitmap | ids sorted | their slots | the list as given
  for (uint32_t i = 0; i < n_sids; ++i) {
    const uint32_t s = byid[i].first;
    if (s <= last) host[s >> 5] |= 1u << (s & 31);
    host[words + i] = s;
    host[words + n_sids + i] = byid[i].second;
    host[words + 2ull * n_sids + i] = sids[i];
  }
  void *d_list, *d_blk, *d_cnt;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_CG_LIST, host.size() * 4, &d_list));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_list, host.data(), host.size() * 4, hipMemcpyHostToDevice));
  G->d_bitmap = (uint32_t*)d_list;
  G->d_ids = G->d_bitmap + words;
  G->d_slot = G->d_ids + n_sids;
  const uint32_t* d_given = G->d_slot + n_sids;
  G->segs = all_segs(t);
  G->blk0.clear();
  G->n_blk = 0;
  for (const shz_seg& g : G->segs) { G->blk0.push_back(G->n_blk); G->n_blk += sg_blocks(g.n); }
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_CG_BLK, G->n_blk * 4, &d_blk));
  G->d_blk = (uint32_t*)d_blk;
  const uint64_t cnt_bytes = ((uint64_t)last + 1) * 8;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_CG_CNT, cnt_bytes + (uint64_t)n_sids * 8 + 8, &d_cnt));
  unsigned long long* song_cnt = (unsigned long long*)d_cnt;
  unsigned long long* picked = song_cnt + (uint64_t)last + 1;
  SHZ_HIP(ctx, hipMemsetAsync(song_cnt, 0, cnt_bytes, ctx->stream));
  for (size_t g = 0; g < G->segs.size(); ++g)
    hipLaunchKernelGGL(sg_count_kernel, dim3(sg_grid(G->segs[g].n)), dim3(64 * SG_WAVES), 0, ctx->stream,
                       (const uint32_t*)G->segs[g].sid, G->segs[g].n, (const uint32_t*)G->d_bitmap, last, G->d_blk + G->blk0[g],
                       song_cnt);
  hipLaunchKernelGGL(sg_pick_kernel, dim3(nblk(n_sids)), dim3(256), 0, ctx->stream, d_given, n_sids, last,
                     (const unsigned long long*)song_cnt, picked);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, shz_memcpy(ctx, row_off + 1, picked, (uint64_t)n_sids * 8, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t run = 0;
  for (uint32_t i = 1; i <= n_sids; ++i) { run += row_off[i]; row_off[i] = run; }   // counts -> CSR
  G->total = run;
  return SHZ_OK;
}

// scan, pass 2, sort: the G->total hits as device columns of at least that many entries, song after song in list order,
// (key32, offset) ascending inside a song.  d_max_off (may be NULL): a zeroed device word that receives the largest offset.
// The stream is idle on return.
int32_t sg_fill(const song_gather& G, const char* who, uint32_t* d_key, uint32_t* d_off, uint32_t* d_max_off) {
  shz_table* t = G.t;
  shz_ctx* ctx = t->ctx;
  const uint64_t total = G.total;
  if (total == 0) return SHZ_OK;
  if (total >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu rows in one call (limit 2^32 - 1); list fewer songs", who, (unsigned long long)total);
  const int ob = bits_for(t->max_off), sb = bits_for((uint64_t)G.n_ids - 1);
  const bool packed = sb + 32 + ob <= 64;
  sg_bufs own;
  uint64_t* a[2] = {(uint64_t*)own.get(total * 8), (uint64_t*)own.get(total * 8)};
  uint64_t* b[2] = {nullptr, nullptr};
  if (!packed) { b[0] = (uint64_t*)own.get(total * 8); b[1] = (uint64_t*)own.get(total * 8); }
  if (!a[0] || !a[1] || (!packed && (!b[0] || !b[1])))
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(%d x %llu) for the gathered rows failed", who, packed ? 2 : 4, (unsigned long long)(total * 8));
  SHZ_TRY(shz_scan_u32(ctx, G.d_blk, G.d_blk, G.n_blk, nullptr));
  for (size_t g = 0; g < G.segs.size(); ++g) {
    const shz_seg& s = G.segs[g];
    if (packed)
      hipLaunchKernelGGL(sg_write_kernel<true>, dim3(sg_grid(s.n)), dim3(64 * SG_WAVES), 0, ctx->stream, (const uint32_t*)s.key,
                         (const uint32_t*)s.sid, (const uint32_t*)s.off, s.n, (const uint32_t*)G.d_bitmap, G.last,
                         (const uint32_t*)(G.d_blk + G.blk0[g]), (const uint32_t*)G.d_ids, (const uint32_t*)G.d_slot, G.n_ids, ob,
                         total, a[0], b[0]);
    else
      hipLaunchKernelGGL(sg_write_kernel<false>, dim3(sg_grid(s.n)), dim3(64 * SG_WAVES), 0, ctx->stream, (const uint32_t*)s.key,
                         (const uint32_t*)s.sid, (const uint32_t*)s.off, s.n, (const uint32_t*)G.d_bitmap, G.last,
                         (const uint32_t*)(G.d_blk + G.blk0[g]), (const uint32_t*)G.d_ids, (const uint32_t*)G.d_slot, G.n_ids, ob,
                         total, a[0], b[0]);
  }
  SHZ_HIP(ctx, hipGetLastError());
  // A segment's rows are sorted by (key32, song, offset), and pass 2 keeps their order: the hits of ONE segment are in
  // (key32, offset) order inside every song already, and the stable sort by slot alone finishes the job.  Several segments
  // are several such runs: the whole word is sorted.
  const bool one_seg = G.segs.size() == 1;
  const uint64_t* sorted;
  int sel = 0;
  if (packed) {
    SHZ_TRY(shz_sort_u64(ctx, a[0], a[1], nullptr, nullptr, 0, total, one_seg ? 32 + ob : 0, sb + 32 + ob, &sel));
    sorted = a[sel];
  } else {   // by (key32, offset) with the slot as payload, then (stable) by slot with (key32, offset) as payload
    if (!one_seg) SHZ_TRY(shz_sort_u64(ctx, a[0], a[1], b[0], b[1], 8, total, 0, 32 + ob, &sel));
    int sel2 = 0;
    SHZ_TRY(shz_sort_u64(ctx, b[sel], b[sel ^ 1], a[sel], a[sel ^ 1], 8, total, 0, sb, &sel2));
    sorted = a[sel ^ sel2];
  }
  hipLaunchKernelGGL(sg_unpack_kernel, dim3(nblk(total)), dim3(256), 0, ctx->stream, sorted, total, ob, d_key, d_off, d_max_off);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));   // (the call's buffers are freed on return)
  return SHZ_OK;
}

}  // namespace

extern "C" int32_t shz_table_song_hashes(shz_table* t, const uint32_t* sids, uint32_t n_sids, uint64_t* row_off, uint32_t* key32,
                                         uint32_t* off, uint64_t cap, uint32_t flags) {
  if (!t) return SHZ_E_INVALID;
  shz_ctx* ctx = t->ctx;
  if (flags & ~SHZ_SONGS_DEVICE_OUT) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_table_song_hashes: flags may hold SHZ_SONGS_DEVICE_OUT");
  if ((key32 == nullptr) != (off == nullptr))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_table_song_hashes: key32 and off are both NULL (counts only) or both given");
  song_gather G;
  SHZ_TRY(sg_prepare(t, "shz_table_song_hashes", sids, n_sids, row_off, &G));
  if (!key32 || G.total == 0) return SHZ_OK;
  if (G.total > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_table_song_hashes: need %llu rows", (unsigned long long)G.total);
  if (flags & SHZ_SONGS_DEVICE_OUT) return sg_fill(G, "shz_table_song_hashes", key32, off, nullptr);
  sg_bufs own;
  uint32_t *d_key = (uint32_t*)own.get(G.total * 4), *d_off = (uint32_t*)own.get(G.total * 4);
  if (!d_key || !d_off) SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_table_song_hashes: hipMalloc(2 x %llu) failed", (unsigned long long)(G.total * 4));
  SHZ_TRY(sg_fill(G, "shz_table_song_hashes", d_key, d_off, nullptr));
  SHZ_HIP(ctx, shz_memcpy(ctx, key32, d_key, G.total * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, off, d_off, G.total * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_match_songs(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t topn, uint32_t flags,
                                   uint64_t* out_rows, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                   uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "table belongs to another ctx");
  if (topn < 1 || topn > 63) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs: topn must be in [1,63]");
  if (flags & ~SHZ_MATCH_FULL_SORT) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs: flags may hold SHZ_MATCH_FULL_SORT");
  if (n_sids == 0) return SHZ_OK;
  if (!out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs: NULL buffer");
  SHZ_TRY(shz_match_ready(ctx, t, topn + 1));
  song_gather G;
  std::vector<uint64_t> row_off((uint64_t)n_sids + 1);
  SHZ_TRY(sg_prepare(t, "shz_match_songs", sids, n_sids, row_off.data(), &G));
  if (G.total >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_songs: %llu rows in one call (limit 2^32 - 1); list fewer songs", (unsigned long long)G.total);
  // the query columns belong to this call: the match uses the workspace
  sg_bufs own;
  uint32_t *d_key = (uint32_t*)own.get(G.total * 4), *d_off = (uint32_t*)own.get(G.total * 4), *d_max = (uint32_t*)own.get(4);
  if (!d_key || !d_off || !d_max) SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_match_songs: hipMalloc(2 x %llu) failed", (unsigned long long)(G.total * 4));
  uint32_t max_off = 0;
  if (G.total) {
    SHZ_HIP(ctx, hipMemsetAsync(d_max, 0, 4, ctx->stream));
    SHZ_TRY(sg_fill(G, "shz_match_songs", d_key, d_off, d_max));
    SHZ_HIP(ctx, shz_memcpy(ctx, &max_off, d_max, 4, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (max_off >= (1u << 20))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_songs: a listed song holds offset %u; its offsets are query offsets here and must be < 2^20", max_off);
  const uint32_t w = topn + 1;
  const uint64_t cells = (uint64_t)n_sids * w;
  std::vector<uint32_t> r_sid(cells), r_aligned(cells), r_dedup(cells), r_nres(n_sids), r_nhash(n_sids);
  std::vector<int32_t> r_delta(cells);
  std::vector<uint64_t> r_npairs(n_sids);
  int32_t rc = SHZ_OK;
  if (G.total)   // (no listed song has a row: nothing to look up, every count stays zero)
    rc = shz_match_device(ctx, t, d_key, d_off, row_off.data(), n_sids, w, flags, (int64_t)t->max_off, r_sid.data(),
                          r_delta.data(), r_aligned.data(), r_dedup.data(), r_nres.data(), r_nhash.data(), r_npairs.data());
  (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
  if (rc != SHZ_OK) return rc;
  // the song itself leaves its own list: what stays are the first topn of every other song (see shz.h)
  for (uint32_t q = 0; q < n_sids; ++q) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < std::min(r_nres[q], w) && k < topn; ++i) {
      const uint64_t src = (uint64_t)q * w + i, dst = (uint64_t)q * topn + k;
      if (r_sid[src] == sids[q]) continue;
      out_sid[dst] = r_sid[src];
      out_delta[dst] = r_delta[src];
      out_aligned[dst] = r_aligned[src];
      out_dedup[dst] = r_dedup[src];
      ++k;
    }
    out_nres[q] = k;
    for (; k < topn; ++k) {
      const uint64_t dst = (uint64_t)q * topn + k;
      out_sid[dst] = 0; out_delta[dst] = 0; out_aligned[dst] = 0; out_dedup[dst] = 0;
    }
    if (out_rows) out_rows[q] = row_off[q + 1] - row_off[q];
    if (out_nhash) out_nhash[q] = r_nhash[q];
    if (out_npairs) out_npairs[q] = r_npairs[q];
  }
  return SHZ_OK;
}
