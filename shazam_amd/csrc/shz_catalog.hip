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

namespace {

// The rows of the listed songs as columns that belong to the call (`own`; the match that follows uses the workspace):
// row_off[n_sids + 1] on the host, *d_key / *d_off of G->total rows (NULL where no listed song has a row) and, where max_off
// is given, the largest offset among them.  The stream is idle on return.
int32_t sg_columns(shz_table* t, const char* who, const uint32_t* sids, uint32_t n_sids, uint64_t* row_off, song_gather* G,
                   sg_bufs* own, uint32_t** d_key, uint32_t** d_off, uint32_t* max_off) {
  shz_ctx* ctx = t->ctx;
  *d_key = *d_off = nullptr;
  if (max_off) *max_off = 0;
  SHZ_TRY(sg_prepare(t, who, sids, n_sids, row_off, G));
  if (G->total >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu rows in one call (limit 2^32 - 1); list fewer songs", who, (unsigned long long)G->total);
  if (G->total == 0) return SHZ_OK;
  *d_key = (uint32_t*)own->get(G->total * 4);
  *d_off = (uint32_t*)own->get(G->total * 4);
  uint32_t* d_max = max_off ? (uint32_t*)own->get(4) : nullptr;
  if (!*d_key || !*d_off || (max_off && !d_max)) SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(2 x %llu) failed", who, (unsigned long long)(G->total * 4));
  if (d_max) SHZ_HIP(ctx, hipMemsetAsync(d_max, 0, 4, ctx->stream));
  SHZ_TRY(sg_fill(*G, who, *d_key, *d_off, d_max));
  if (d_max) {
    SHZ_HIP(ctx, shz_memcpy(ctx, max_off, d_max, 4, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  return SHZ_OK;
}

// The song itself leaves its own list (see shz.h).  r_*: the top w = topn + 1 of n queries, query i being a form of the song
// sids[i / per]; out_*: the first topn of every OTHER song, the rest of a row zeroed, and their number
void sg_drop_self(const uint32_t* sids, uint32_t per, uint64_t n, uint32_t topn, const uint32_t* r_sid, const int32_t* r_delta,
                  const uint32_t* r_aligned, const uint32_t* r_dedup, const uint32_t* r_nres, uint32_t* out_sid, int32_t* out_delta,
                  uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres) {
  const uint32_t w = topn + 1;
  for (uint64_t q = 0; q < n; ++q) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < std::min(r_nres[q], w) && k < topn; ++i) {
      const uint64_t src = q * w + i, dst = q * topn + k;
      if (r_sid[src] == sids[q / per]) continue;
      out_sid[dst] = r_sid[src];
      out_delta[dst] = r_delta[src];
      out_aligned[dst] = r_aligned[src];
      out_dedup[dst] = r_dedup[src];
      ++k;
    }
    out_nres[q] = k;
    for (; k < topn; ++k) {
      const uint64_t dst = q * topn + k;
      out_sid[dst] = 0; out_delta[dst] = 0; out_aligned[dst] = 0; out_dedup[dst] = 0;
    }
  }
}

}  // namespace

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
  sg_bufs own;
  std::vector<uint64_t> row_off((uint64_t)n_sids + 1);
  uint32_t *d_key, *d_off, max_off;
  SHZ_TRY(sg_columns(t, "shz_match_songs", sids, n_sids, row_off.data(), &G, &own, &d_key, &d_off, &max_off));
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
  else
    shz_floor_zero_rows(ctx, n_sids);   // (the vote floor's rows line up with the result arrays)
  (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
  if (rc != SHZ_OK) return rc;
  sg_drop_self(sids, 1, n_sids, topn, r_sid.data(), r_delta.data(), r_aligned.data(), r_dedup.data(), r_nres.data(), out_sid,
               out_delta, out_aligned, out_dedup, out_nres);
  for (uint32_t q = 0; q < n_sids; ++q) {
    if (out_rows) out_rows[q] = row_off[q + 1] - row_off[q];
    if (out_nhash) out_nhash[q] = r_nhash[q];
    if (out_npairs) out_npairs[q] = r_npairs[q];
  }
  return SHZ_OK;
}

// ---- the row warp: sped-up and pitch-shifted copies inside the table -----------------------------
// The table holds no peaks, but a row IS two peaks: key32 = f1 << 20 | f2 << 8 | dt at offset t1 is (f1, t1) and (f2, t1 + dt).
// Both are moved by the integer maps of shz_warp_pair_hash_tf (sp_warp_f, and the time map in 64 bits) and the key is formed
// again; a row leaves where a frequency leaves the spectrogram or dt' passes 200.  Elementwise: no sort, no fan_value.
//
// Work is laid out over items, and a LAYOUT says which row of which song an item is, which segment of the output it counts
// into and which factor pair warps it.  There are two:
//   product (3.7h)  every listed song at every warp: (song q, warp v, row r) items, song-major, then warp-major, then the
//                   song's rows (sp_decode's layout); segment q K + v is one contiguous query of the match;
//   jobs (3.7o)     a list of (song, t16, f16) in which a song may stand several times: (job j, row r) items, job-major, then
//                   the rows of the job's song; segment j is one contiguous query of the extent pass.
// In both a wave stays at one warp over consecutive rows wherever it lies inside one segment.  The compaction is
// sg_count_kernel / sg_write_kernel's and exists once, as templates on the layout: blocks of RW_ITEMS items, one wave a
// block; pass 1 ballots, writes one count per block and adds the kept items to their segment's count (one add a wave where
// the wave lies inside one segment); the block counts are scanned; pass 2 repeats the map and writes at block base + rank
// inside the ballot.  No atomic decides a place.
#define RW_ITEMS 512u   // items of a block
#define RW_LOADS 8      // RW_ITEMS / 64
#define RW_WAVES 4      // blocks (waves) of a workgroup
#define RW_SMALL_WARPS 2u   // warps of a slice (of one song) under SHZ_DEBUG_CATALOG_SMALL_SLICES
#define RW_SMALL_JOBS 2u    // jobs of a slice under SHZ_DEBUG_CATALOG_SMALL_SLICES

// THE map: row (key32, off) under the warp (t16, f16) -> kept?, and (*okey, *ooff) where kept (off t16 < 2^48 is the
// caller's promise: t1' is stored in 32 bits).  The kernels and shz_warp_row_host both call it
__host__ __device__ __forceinline__ bool rw_warp_row(uint32_t key32, uint32_t off, uint32_t t16, uint32_t f16, uint32_t* okey,
                                                     uint32_t* ooff) {
  const uint32_t f1 = key32 >> 20, f2 = (key32 >> 8) & 0xFFFu, dt = key32 & 0xFFu;
  const uint64_t t1 = ((uint64_t)off * t16 + 32768u) >> 16, t2 = (((uint64_t)off + dt) * t16 + 32768u) >> 16;
  const uint32_t g1 = sp_warp_f(f1, f16), g2 = sp_warp_f(f2, f16), d = (uint32_t)(t2 - t1);
  *okey = (g1 << 20) | (g2 << 8) | d;
  *ooff = (uint32_t)t1;
  return g1 <= SP_F_MAX && g2 <= SP_F_MAX && d <= SHZ_MAX_DT;
}

struct rw_cursor {                 // where an item lies
  uint32_t seg, fac;               // the segment it counts into, the index of its factor pair
  uint32_t r, n;                   // row of the song, rows of the song
  uint64_t row0;                   // the song's first row
};

struct rw_product {                // the slice: songs [q0, q0 + nq) at the warps [v0, v0 + K)
  const uint64_t* roff;            // CSR of the call's songs over the rows, from 0
  uint32_t q0, nq, v0, K;
  // item w -> its song (the last q whose first item is <= w: empty songs share a start), warp and row
  __device__ __forceinline__ void seek(uint64_t w, rw_cursor* c) const {
    const uint64_t r00 = roff[q0];
    uint32_t lo = 0, hi = nq;
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((roff[q0 + mid] - r00) * K <= w) lo = mid; else hi = mid;
    }
    const uint64_t r0 = roff[q0 + lo];
    const uint32_t n = (uint32_t)(roff[q0 + lo + 1] - r0);   // (> 0: w lies inside the song's items)
    const uint32_t rem = (uint32_t)(w - (r0 - r00) * K), v = rem / max(n, 1u), vc = min(v, K - 1);
    c->seg = lo * K + vc;
    c->fac = v0 + vc;
    c->r = min(rem - v * n, max(n, 1u) - 1);   // (the clamps hold for every consistent view; they keep any read inside the columns)
    c->n = n;
    c->row0 = r0;
  }
};

struct rw_jobs {                   // the slice: nj jobs, each one song at one warp
  const uint64_t* roff;            // CSR of the call's distinct songs over the rows, from 0
  const uint32_t* song;            // the job's song (index into roff)
  const uint64_t* base;            // nj + 1: first item of every job (item w of the slice is base[0] + w)
  uint32_t nj;
  // item w -> its job (the last j whose first item is <= w: empty jobs share a start) and row
  __device__ __forceinline__ void seek(uint64_t w, rw_cursor* c) const {
    const uint64_t b0 = base[0];
    uint32_t lo = 0, hi = nj;
    while (lo + 1 < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (base[mid] - b0 <= w) lo = mid; else hi = mid;
    }
    const uint32_t s = song[lo];
    const uint64_t r0 = roff[s];
    const uint32_t n = (uint32_t)(roff[s + 1] - r0);   // (> 0: w lies inside the job's items)
    const uint64_t rem = w - (base[lo] - b0);
    c->seg = c->fac = lo;
    c->r = (uint32_t)min(rem, (uint64_t)(max(n, 1u) - 1));   // (the clamp holds for every consistent view; it keeps any read inside the columns)
    c->n = n;
    c->row0 = r0;
  }
};

template <class L>
struct rw_view {                   // what the kernels of one slice read (device pointers)
  const uint32_t *key, *off;       // the rows of all songs of the call, song after song
  const uint32_t *t16, *f16;       // the factor pairs a cursor's fac indexes: the call's warps, or the slice's jobs
  uint64_t n_items;
  L lay;
};

// the RW_LOADS items of this lane in the block at w0: rows loaded, segment and factor index kept; dead lanes: seg = ~0, fac = 0
template <class L>
__device__ __forceinline__ void rw_load(const rw_view<L>& V, uint64_t w0, uint32_t lane, uint32_t* k, uint32_t* o, uint32_t* seg,
                                        uint32_t* fac) {
  rw_cursor c{0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < RW_LOADS; ++j) {
    const uint64_t w = w0 + (uint64_t)j * 64 + lane;
    seg[j] = 0xFFFFFFFFu;
    k[j] = o[j] = fac[j] = 0;
    if (w >= V.n_items) continue;
    if (j == 0 || c.r + 64 >= c.n) V.lay.seek(w, &c);   // (64 items on: still inside this segment's rows?)
    else c.r += 64;
    if (c.n == 0) continue;
    k[j] = V.key[c.row0 + c.r];
    o[j] = V.off[c.row0 + c.r];
    seg[j] = c.seg;
    fac[j] = c.fac;
  }
}

// pass 1: kept items of every block, kept items of every segment
template <class L>
__global__ __launch_bounds__(64 * RW_WAVES) void rw_count_kernel(rw_view<L> V, uint32_t* __restrict__ blk_cnt,
                                                                  uint32_t* __restrict__ seg_cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * RW_WAVES + (threadIdx.x >> 6);
  const uint64_t w0 = blk * RW_ITEMS;
  if (w0 >= V.n_items) return;   // uniform in the wave
  uint32_t k[RW_LOADS], o[RW_LOADS], seg[RW_LOADS], fac[RW_LOADS];
  rw_load(V, w0, lane, k, o, seg, fac);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < RW_LOADS; ++j) {
    const bool live = seg[j] != 0xFFFFFFFFu;   // (a dead lane maps nothing; its factor index 0 lies inside the arrays)
    uint32_t a, b;
    const bool keep = live && rw_warp_row(k[j], o[j], V.t16[fac[j]], V.f16[fac[j]], &a, &b);
    const uint64_t m = __ballot(keep);
    const uint32_t first = (uint32_t)__shfl((int)seg[j], 0, 64);   // (live lanes are a prefix of the wave)
    if (__ballot(live && seg[j] != first) == 0) {   // the wave inside one segment: one add
      if (lane == 0 && m) atomicAdd(seg_cnt + first, (uint32_t)__popcll(m));
    } else if (keep) {
      atomicAdd(seg_cnt + seg[j], 1u);
    }
    c += (uint32_t)__popcll(m);
  }
  if (lane == 0) blk_cnt[blk] = c;
}

// pass 2: every kept item, in item order, at the place the scan of the block counts gives (no store at or beyond cap)
template <class L>
__global__ __launch_bounds__(64 * RW_WAVES) void rw_write_kernel(rw_view<L> V, const uint32_t* __restrict__ blk_pos,
                                                                  uint32_t* __restrict__ out_key, uint32_t* __restrict__ out_off,
                                                                  uint64_t cap) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t blk = (uint64_t)blockIdx.x * RW_WAVES + (threadIdx.x >> 6);
  const uint64_t w0 = blk * RW_ITEMS;
  if (w0 >= V.n_items) return;   // uniform in the wave
  uint32_t k[RW_LOADS], o[RW_LOADS], seg[RW_LOADS], fac[RW_LOADS];
  rw_load(V, w0, lane, k, o, seg, fac);
  uint64_t base = blk_pos[blk];
#pragma unroll
  for (int j = 0; j < RW_LOADS; ++j) {
    uint32_t a, b;
    const bool keep = seg[j] != 0xFFFFFFFFu && rw_warp_row(k[j], o[j], V.t16[fac[j]], V.f16[fac[j]], &a, &b);
    const uint64_t m = __ballot(keep);
    if (keep) {
      const uint64_t pos = base + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
      if (pos < cap) { out_key[pos] = a; out_off[pos] = b; }
    }
    base += (uint64_t)__popcll(m);
  }
}

// the largest offset of every gathered song (song_max zeroed; a song without rows keeps 0): one atomicMax a wave where the
// wave lies inside one song, whose result no order changes
__global__ __launch_bounds__(256) void rw_song_max_kernel(const uint32_t* __restrict__ off, const uint64_t* __restrict__ roff,
                                                           uint32_t n_songs, uint64_t total, uint32_t* __restrict__ song_max) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < total;
  uint32_t lo = 0, hi = n_songs;   // the last song whose first row is <= i (empty songs share a start)
  while (live && lo + 1 < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (roff[mid] <= i) lo = mid; else hi = mid;
  }
  uint32_t o = live ? off[i] : 0u;
  const uint32_t first = (uint32_t)__shfl((int)lo, 0, 64);   // (live lanes are a prefix of the wave)
  if (__ballot(live && lo != first) == 0) {
    for (int d = 32; d >= 1; d >>= 1) o = max(o, (uint32_t)__shfl_xor((int)o, d, 64));
    if ((threadIdx.x & 63) == 0 && o) atomicMax(song_max + first, o);
  } else if (live && o) {
    atomicMax(song_max + lo, o);
  }
}

namespace {

struct rw_tabs {                   // the call's tables on the device (one block); base and song in the job form only
  const uint64_t *d_roff = nullptr, *d_base = nullptr;
  const uint32_t *d_t16 = nullptr, *d_f16 = nullptr, *d_song = nullptr;
};
template <class L>
struct rw_slice {                  // one slice of a call: its view and the number of its segments
  rw_view<L> V;
  uint64_t n_seg;
};

static inline uint64_t rw_blocks(uint64_t n) { return (n + RW_ITEMS - 1) / RW_ITEMS; }
static inline dim3 rw_grid(uint64_t n_items) { return dim3((unsigned)((rw_blocks(n_items) + RW_WAVES - 1) / RW_WAVES)); }

// roff[n_songs + 1] (from 0) | base[n_fac + 1] | t16[n_fac] | f16[n_fac] | song[n_fac], uploaded once a call; base and song
// may both be NULL (the product form: the factors are the call's warps)
int32_t rw_upload(shz_ctx* ctx, const uint64_t* row_off, uint32_t n_songs, const uint32_t* t16, const uint32_t* f16, uint32_t n_fac,
                  const uint64_t* base, const uint32_t* song, rw_tabs* T) {
  const uint64_t ro_bytes = ((uint64_t)n_songs + 1) * 8, ba_bytes = base ? ((uint64_t)n_fac + 1) * 8 : 0, col = (uint64_t)n_fac * 4;
  const uint64_t bytes = ro_bytes + ba_bytes + (song ? 3 : 2) * col;
  std::vector<char> h(bytes);
  uint64_t* hr = (uint64_t*)h.data();
  for (uint32_t q = 0; q <= n_songs; ++q) hr[q] = row_off[q] - row_off[0];
  if (base) memcpy(h.data() + ro_bytes, base, ba_bytes);
  memcpy(h.data() + ro_bytes + ba_bytes, t16, col);
  memcpy(h.data() + ro_bytes + ba_bytes + col, f16, col);
  if (song) memcpy(h.data() + ro_bytes + ba_bytes + 2 * col, song, col);
  void* d;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RW_TAB, bytes, &d));
  SHZ_HIP(ctx, shz_memcpy(ctx, d, h.data(), bytes, hipMemcpyHostToDevice));
  T->d_roff = (const uint64_t*)d;
  T->d_base = (const uint64_t*)((char*)d + ro_bytes);
  T->d_t16 = (const uint32_t*)((char*)d + ro_bytes + ba_bytes);
  T->d_f16 = T->d_t16 + n_fac;
  T->d_song = T->d_f16 + n_fac;
  return SHZ_OK;
}

// pass 1 and the scan of one slice: seg_off[n_seg + 1] (host) is the exact CSR of the segments' kept rows, relative to the
// slice, and *d_blk the scanned block counts that pass 2 reads.  The stream is idle on return.  A slice without items
// launches nothing
template <class L>
int32_t rw_count(shz_ctx* ctx, const rw_view<L>& V, uint64_t n_seg, uint32_t** d_blk, uint64_t* seg_off) {
  for (uint64_t e = 0; e <= n_seg; ++e) seg_off[e] = 0;
  *d_blk = nullptr;
  if (V.n_items == 0) return SHZ_OK;
  const uint64_t n_blk = rw_blocks(V.n_items);
  void *blk, *d_cnt;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RW_BLK, n_blk * 4, &blk));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_RW_CNT, n_seg * 4, &d_cnt));
  *d_blk = (uint32_t*)blk;
  SHZ_HIP(ctx, hipMemsetAsync(d_cnt, 0, n_seg * 4, ctx->stream));
  hipLaunchKernelGGL(rw_count_kernel<L>, rw_grid(V.n_items), dim3(64 * RW_WAVES), 0, ctx->stream, V, *d_blk, (uint32_t*)d_cnt);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, *d_blk, *d_blk, n_blk, nullptr));
  std::vector<uint32_t> cnt(n_seg);
  SHZ_HIP(ctx, shz_memcpy(ctx, cnt.data(), d_cnt, n_seg * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint64_t e = 0; e < n_seg; ++e) seg_off[e + 1] = seg_off[e] + cnt[e];
  return SHZ_OK;
}

// pass 2 of the slice rw_count counted (d_blk: its block counts, scanned), queued on the stream
template <class L>
int32_t rw_write(shz_ctx* ctx, const rw_view<L>& V, const uint32_t* d_blk, uint32_t* d_okey, uint32_t* d_ooff, uint64_t cap) {
  if (V.n_items == 0) return SHZ_OK;
  hipLaunchKernelGGL(rw_write_kernel<L>, rw_grid(V.n_items), dim3(64 * RW_WAVES), 0, ctx->stream, V, d_blk, d_okey, d_ooff, cap);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// a timed call begins: the ctx's events exist (created on first use) and slot 0 holds the start
int32_t rw_clock_start(shz_ctx* ctx) {
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  for (hipEvent_t& e : ctx->sp_ev)
    if (!e) SHZ_HIP(ctx, hipEventCreate(&e));
  SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[0], ctx->stream));
  return SHZ_OK;
}

// Warp and stage, slice by slice.  Per slice: both passes into d_wkey / d_woff (room for buf_items rows), then
// stage(i, seg_off) on the warped columns and the CSR of the slice's segments over them (seg_off[n_seg] rows; the stage is
// called for a slice whose rows all left too).  Where timed, *warp_ms and *stage_ms gain the slice's two hipEvent intervals
// (slots 2, 3, 4 of sp_ev: neither shz_match_device nor ex_device records an event).
// Nothing returns from inside the loop: a failed pass, stage or event call ends it, and the stream is synchronised before
// the error leaves -- work that a refused call queued may read the columns, which the caller frees next.
template <class L, class Stage>
int32_t rw_run_slices(shz_ctx* ctx, const char* who, const std::vector<rw_slice<L>>& slices, uint32_t* d_wkey, uint32_t* d_woff,
                      uint64_t buf_items, bool timed, Stage stage, float* warp_ms, float* stage_ms) {
  hipEvent_t* ev = ctx->sp_ev;
  const auto mark = [&](int i) { return !timed || hipEventRecord(ev[i], ctx->stream) == hipSuccess; };
  std::vector<uint64_t> seg_off;
  int32_t rc = SHZ_OK;
  bool ev_ok = true;
  for (size_t i = 0; i < slices.size(); ++i) {
    const rw_slice<L>& s = slices[i];
    if (!(ev_ok = mark(2))) break;
    seg_off.assign((size_t)s.n_seg + 1, 0);
    uint32_t* d_blk = nullptr;
    rc = rw_count(ctx, s.V, s.n_seg, &d_blk, seg_off.data());
    if (rc == SHZ_OK && seg_off[s.n_seg]) rc = rw_write(ctx, s.V, d_blk, d_wkey, d_woff, buf_items);
    if (rc != SHZ_OK || !(ev_ok = mark(3))) break;
    rc = stage(i, seg_off.data());
    if (rc != SHZ_OK) break;
    if (timed) {
      float a = 0.f, b = 0.f;
      ev_ok = mark(4) && hipEventSynchronize(ev[4]) == hipSuccess && hipEventElapsedTime(&a, ev[2], ev[3]) == hipSuccess &&
              hipEventElapsedTime(&b, ev[3], ev[4]) == hipSuccess;
      if (!ev_ok) break;
      *warp_ms += a;
      *stage_ms += b;
    }
  }
  (void)hipStreamSynchronize(ctx->stream);
  if (!ev_ok) SHZ_FAIL(ctx, SHZ_E_HIP, "%s: timing a slice failed", who);
  return rc;
}

}  // namespace

extern "C" int32_t shz_warp_row_host(const uint32_t* key32, const uint32_t* off, uint64_t n, uint32_t t16, uint32_t f16,
                                     uint32_t* out_key32, uint32_t* out_off, uint8_t* out_keep) {
  if (t16 < SP_S_MIN || t16 > SP_S_MAX || f16 < SP_S_MIN || f16 > SP_S_MAX) return SHZ_E_INVALID;
  if (n && (!key32 || !off || !out_key32 || !out_off || !out_keep)) return SHZ_E_INVALID;
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t a, b;
    const bool keep = rw_warp_row(key32[i], off[i], t16, f16, &a, &b);
    out_key32[i] = keep ? a : 0u;
    out_off[i] = keep ? b : 0u;
    out_keep[i] = keep ? 1 : 0;
  }
  return SHZ_OK;
}

extern "C" int32_t shz_warp_rows(shz_ctx* ctx, const uint32_t* key32, const uint32_t* off, const uint64_t* row_off, uint32_t n_songs,
                                 const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                                 uint32_t* out_key32, uint32_t* out_off, uint64_t* out_row_off, uint64_t cap, uint64_t* count) {
  if (!ctx) return SHZ_E_INVALID;
  if (count) *count = 0;
  // everything that can be refused is refused before the first launch
  if (flags & ~(SHZ_IN_DEVICE | SHZ_OUT_DEVICE)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_rows: flags may hold SHZ_IN_DEVICE and SHZ_OUT_DEVICE");
  SHZ_TRY(sp_check_ladder(ctx, "shz_warp_rows", "n_warps", "tempo", tempo_q16, "pitch", pitch_q16, n_warps, 1));
  if (!row_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_rows: row_off is NULL");
  for (uint32_t q = 0; q < n_songs; ++q)
    if (row_off[q + 1] < row_off[q]) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_rows: row_off decreases at song %u", q);
  const uint64_t n = row_off[n_songs] - row_off[0], n_seg = (uint64_t)n_songs * n_warps;
  if (n && (!key32 || !off)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_rows: NULL buffer");
  if (cap && (!out_key32 || !out_off)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_warp_rows: NULL buffer");
  if (n >= (1ull << 32) || n * n_warps >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_warp_rows: %llu rows x %u warps in one call (limit 2^32 - 1 items)", (unsigned long long)n, n_warps);
  if (out_row_off) memset(out_row_off, 0, (n_seg + 1) * 8);
  if (n == 0) return SHZ_OK;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  sg_bufs own;
  const uint32_t *d_key = key32 + row_off[0], *d_off = off + row_off[0];
  if (!(flags & SHZ_IN_DEVICE)) {
    uint32_t *a = (uint32_t*)own.get(n * 4), *b = (uint32_t*)own.get(n * 4);
    if (!a || !b) SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_warp_rows: hipMalloc(2 x %llu) failed", (unsigned long long)(n * 4));
    SHZ_HIP(ctx, shz_memcpy(ctx, a, d_key, n * 4, hipMemcpyHostToDevice));
    SHZ_HIP(ctx, shz_memcpy(ctx, b, d_off, n * 4, hipMemcpyHostToDevice));
    d_key = a;
    d_off = b;
  }
  rw_tabs T;
  SHZ_TRY(rw_upload(ctx, row_off, n_songs, tempo_q16, pitch_q16, n_warps, nullptr, nullptr, &T));
  const rw_view<rw_product> V{d_key, d_off, T.d_t16, T.d_f16, n * n_warps, {T.d_roff, 0, n_songs, 0, n_warps}};
  std::vector<uint64_t> so((size_t)n_seg + 1, 0);
  uint32_t* d_blk = nullptr;
  int32_t rc = rw_count(ctx, V, n_seg, &d_blk, so.data());
  if (rc != SHZ_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }   // (queued work may read the staged columns)
  const uint64_t total = so[n_seg];
  if (out_row_off) memcpy(out_row_off, so.data(), (n_seg + 1) * 8);
  if (count) *count = total;
  if (total > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_warp_rows: need %llu rows", (unsigned long long)total);
  if (total == 0) return SHZ_OK;
  uint32_t *d_ok = out_key32, *d_oo = out_off;
  if (!(flags & SHZ_OUT_DEVICE)) {
    d_ok = (uint32_t*)own.get(total * 4);
    d_oo = (uint32_t*)own.get(total * 4);
    if (!d_ok || !d_oo) SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_warp_rows: hipMalloc(2 x %llu) failed", (unsigned long long)(total * 4));
  }
  rc = rw_write(ctx, V, d_blk, d_ok, d_oo, (flags & SHZ_OUT_DEVICE) ? cap : total);
  if (rc == SHZ_OK && !(flags & SHZ_OUT_DEVICE)) {
    if (shz_memcpy(ctx, out_key32, d_ok, total * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        shz_memcpy(ctx, out_off, d_oo, total * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      ctx->err = "shz_warp_rows: copy of the warped rows failed";
      rc = SHZ_E_HIP;
    }
  }
  if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SHZ_OK) { ctx->err = "shz_warp_rows: hipStreamSynchronize failed"; rc = SHZ_E_HIP; }
  return rc;   // (the call's buffers are freed on return: the stream is idle)
}

extern "C" int32_t shz_match_songs_warps(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t topn,
                                         const uint32_t* tempo_q16, const uint32_t* pitch_q16, uint32_t n_warps, uint32_t flags,
                                         uint64_t* out_rows, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                         uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                                         float* ms_gather, float* ms_warp, float* ms_match) {
  if (!ctx || !t) return SHZ_E_INVALID;
  const char* who = "shz_match_songs_warps";
  if (ms_gather) *ms_gather = 0.f;
  if (ms_warp) *ms_warp = 0.f;
  if (ms_match) *ms_match = 0.f;
  if (t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "table belongs to another ctx");
  if (topn < 1 || topn > 63) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs_warps: topn must be in [1,63]");
  if (flags & ~SHZ_MATCH_FULL_SORT) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs_warps: flags may hold SHZ_MATCH_FULL_SORT");
  SHZ_TRY(sp_check_ladder(ctx, who, "n_warps", "tempo", tempo_q16, "pitch", pitch_q16, n_warps, 1));
  if (n_sids == 0) return SHZ_OK;
  if (!out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_songs_warps: NULL buffer");
  SHZ_TRY(shz_match_ready(ctx, t, topn + 1));
  const uint32_t K = n_warps, w = topn + 1;
  const uint32_t t16_max = *std::max_element(tempo_q16, tempo_q16 + K);   // (time alone: the bias bound)
  const bool timed = ms_gather || ms_warp || ms_match;
  if (timed) SHZ_TRY(rw_clock_start(ctx));
  // 1) the rows of the listed songs into columns of this call
  song_gather G;
  sg_bufs own;
  std::vector<uint64_t> row_off((uint64_t)n_sids + 1);
  uint32_t *d_key, *d_off, max_off;
  SHZ_TRY(sg_columns(t, who, sids, n_sids, row_off.data(), &G, &own, &d_key, &d_off, &max_off));
  const uint64_t nv = (uint64_t)n_sids * K;
  for (uint64_t i = 0; i < nv * topn; ++i) { out_sid[i] = 0; out_delta[i] = 0; out_aligned[i] = 0; out_dedup[i] = 0; }
  for (uint64_t i = 0; i < nv; ++i) {
    out_nres[i] = 0;
    if (out_nhash) out_nhash[i] = 0;
    if (out_npairs) out_npairs[i] = 0;
  }
  if (out_rows)
    for (uint32_t q = 0; q < n_sids; ++q) out_rows[q] = row_off[q + 1] - row_off[q];
  if (G.total == 0) {   // (no listed song has a row: nothing to look up, every count stays zero -- and every floor row)
    shz_floor_zero_rows(ctx, nv);
    return SHZ_OK;
  }
  // the largest warped offset: the bias bound of the match
  const uint64_t t_max = ((uint64_t)max_off * t16_max + 32768) >> 16;
  if (t_max >= (1ull << 20))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_songs_warps: a listed song holds offset %u, which the time factor %u / 65536 takes to %llu; warped offsets are query offsets here and must be < 2^20",
             max_off, t16_max, (unsigned long long)t_max);
  rw_tabs T;
  SHZ_TRY(rw_upload(ctx, row_off.data(), n_sids, tempo_q16, pitch_q16, K, nullptr, nullptr, &T));
  // 2) the slices, from the row counts alone: whole songs x a contiguous chunk of warps whose items (8 bytes each in the
  // call's buffers) stay within 1/8 of the workspace limit and the match's 2^28-pair budget, and below 2^32; the ladder is
  // cut only where one song at all warps is beyond that, and a song at one warp is never split.  Either way the segments of
  // a slice are the queries q0 K + v0 onwards of the call, one after the other
  const uint64_t max_items = std::min<uint64_t>(std::max<uint64_t>(ctx->ws_limit / 64, 1), 1ull << 28);
  const uint64_t max_seg = 1ull << 24;
  const bool small = (ctx->debug & SHZ_DEBUG_CATALOG_SMALL_SLICES) != 0;
  std::vector<rw_slice<rw_product>> plan;
  uint64_t buf_items = 0;
  const auto slice = [&](uint32_t q0, uint32_t nq, uint32_t v0, uint32_t kv) {
    const uint64_t n_items = (row_off[q0 + nq] - row_off[q0]) * kv;
    plan.push_back({{d_key, d_off, T.d_t16, T.d_f16, n_items, {T.d_roff, q0, nq, v0, kv}}, (uint64_t)nq * kv});
    buf_items = std::max(buf_items, n_items);
  };
  for (uint32_t q0 = 0; q0 < n_sids;) {
    const uint64_t r0 = row_off[q0 + 1] - row_off[q0];
    if (small || r0 * K > max_items) {   // one song, its warps in chunks
      const uint32_t kv = small ? RW_SMALL_WARPS : (uint32_t)std::max<uint64_t>(max_items / std::max<uint64_t>(r0, 1), 1);
      for (uint32_t v0 = 0; v0 < K; v0 += kv) slice(q0, 1, v0, std::min(kv, K - v0));
      ++q0;
      continue;
    }
    uint32_t nq = 1;
    while (q0 + nq < n_sids && (uint64_t)(nq + 1) * K <= max_seg && (row_off[q0 + nq + 1] - row_off[q0]) * K <= max_items) ++nq;
    slice(q0, nq, 0, K);
    q0 += nq;
  }
  if (buf_items >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_songs_warps: a song of %llu rows (limit 2^32 - 1 warped rows a slice)", (unsigned long long)buf_items);
  // the warped columns of the largest slice, once
  uint32_t *d_wkey = (uint32_t*)own.get(buf_items * 4), *d_woff = (uint32_t*)own.get(buf_items * 4);
  if (!d_wkey || !d_woff)
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_match_songs_warps: hipMalloc(2 x %llu + 2 x %llu) failed", (unsigned long long)(G.total * 4), (unsigned long long)(buf_items * 4));
  if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[1], ctx->stream));
  // 3) warp and match, slice by slice: (song, warp) = one query of the match, its top w at its place among the call's
  std::vector<uint32_t> r_sid(nv * w), r_aligned(nv * w), r_dedup(nv * w), r_nres(nv), r_nhash(nv);
  std::vector<int32_t> r_delta(nv * w);
  std::vector<uint64_t> r_npairs(nv);
  float warp_ms = 0.f, match_ms = 0.f;
  const auto match = [&](size_t i, const uint64_t* seg_off) -> int32_t {
    const rw_slice<rw_product>& s = plan[i];
    const uint64_t e0 = (uint64_t)s.V.lay.q0 * K + s.V.lay.v0;
    if (!seg_off[s.n_seg]) {   // (a slice without a warped row: the vote floor's rows line up with the result arrays)
      shz_floor_zero_rows(ctx, s.n_seg);
      return SHZ_OK;
    }
    return shz_match_device(ctx, t, d_wkey, d_woff, seg_off, (uint32_t)s.n_seg, w, flags, (int64_t)t_max, r_sid.data() + e0 * w,
                            r_delta.data() + e0 * w, r_aligned.data() + e0 * w, r_dedup.data() + e0 * w, r_nres.data() + e0,
                            r_nhash.data() + e0, r_npairs.data() + e0);
  };
  SHZ_TRY(rw_run_slices(ctx, who, plan, d_wkey, d_woff, buf_items, timed, match, &warp_ms, &match_ms));
  // 4) the song itself leaves the list of every one of its warps
  sg_drop_self(sids, K, nv, topn, r_sid.data(), r_delta.data(), r_aligned.data(), r_dedup.data(), r_nres.data(), out_sid, out_delta,
               out_aligned, out_dedup, out_nres);
  if (out_nhash) memcpy(out_nhash, r_nhash.data(), nv * 4);
  if (out_npairs) memcpy(out_npairs, r_npairs.data(), nv * 8);
  if (timed) {
    if (ms_gather) SHZ_HIP(ctx, hipEventElapsedTime(ms_gather, ctx->sp_ev[0], ctx->sp_ev[1]));
    if (ms_warp) *ms_warp = warp_ms;
    if (ms_match) *ms_match = match_ms;
  }
  return SHZ_OK;
}

// ---- the job form: where an altered copy overlaps its original, and at what tempo ------------------------
// The refinement of found pairs has a JOB LIST: job j is one song at the one warp (t16, f16) its pair was found at, and a song
// may stand in several jobs.  The row warp is the one above, under the rw_jobs layout.
extern "C" int32_t shz_match_songs_warps_extents(shz_ctx* ctx, shz_table* t, const uint32_t* job_sid, const uint32_t* job_t16,
                                                 const uint32_t* job_f16, uint32_t n_jobs, uint32_t ncand, const uint32_t* cand_sid,
                                                 const int32_t* cand_dlo, const int32_t* cand_dhi, const uint32_t* cand_n,
                                                 uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last,
                                                 uint32_t* out_t_first, uint32_t* out_t_last, uint32_t* out_hist, uint32_t* out_shift,
                                                 uint64_t* out_sum_q, uint64_t* out_sum_u, uint64_t* out_sum_qq, uint64_t* out_sum_qu,
                                                 uint64_t* out_kept, float* ms_gather, float* ms_warp, float* ms_extent) {
  if (!ctx || !t) return SHZ_E_INVALID;
  const char* who = "shz_match_songs_warps_extents";
  // everything that can be refused from the arguments is refused before the first launch
  SHZ_TRY(ex_state(ctx, t, who, ncand));
  if (n_jobs == 0) return SHZ_OK;
  if (!job_sid || !job_t16 || !job_f16) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL job array", who);
  for (uint32_t j = 0; j < n_jobs; ++j)
    if (job_t16[j] < SP_S_MIN || job_t16[j] > SP_S_MAX || job_f16[j] < SP_S_MIN || job_f16[j] > SP_S_MAX)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: job %u has the factors (%u, %u); factors are Q16 in [%u, %u] (0.5x .. 2x)", who, j, job_t16[j],
               job_f16[j], SP_S_MIN, SP_S_MAX);
  if (!out_sum_q || !out_sum_u || !out_sum_qq || !out_sum_qu) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL sum array", who);
  ex_args A{n_jobs, ncand, cand_sid, cand_dlo, cand_dhi, cand_n, out_count, out_q_first, out_q_last, out_t_first, out_t_last,
            out_hist, out_shift};
  A.out_sum_q = out_sum_q;
  A.out_sum_u = out_sum_u;
  A.out_sum_qq = out_sum_qq;
  A.out_sum_qu = out_sum_qu;
  SHZ_TRY(ex_check(ctx, t, who, A));
  const bool timed = ms_gather || ms_warp || ms_extent;
  if (timed) SHZ_TRY(rw_clock_start(ctx));
  // 1) the distinct songs of the jobs, ascending, each gathered once; job j reads song slot[j] of them
  std::vector<uint32_t> usid(job_sid, job_sid + n_jobs), slot(n_jobs);
  std::sort(usid.begin(), usid.end());
  usid.erase(std::unique(usid.begin(), usid.end()), usid.end());
  const uint32_t n_songs = (uint32_t)usid.size();
  for (uint32_t j = 0; j < n_jobs; ++j) slot[j] = (uint32_t)(std::lower_bound(usid.begin(), usid.end(), job_sid[j]) - usid.begin());
  song_gather G;
  sg_bufs own;
  std::vector<uint64_t> row_off((size_t)n_songs + 1);
  uint32_t *d_key, *d_off;
  SHZ_TRY(sg_columns(t, who, usid.data(), n_songs, row_off.data(), &G, &own, &d_key, &d_off, nullptr));
  std::vector<uint64_t> base((size_t)n_jobs + 1, 0);   // first item of every job
  for (uint32_t j = 0; j < n_jobs; ++j) base[j + 1] = base[j] + (row_off[slot[j] + 1] - row_off[slot[j]]);
  if (base[n_jobs] >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu rows over all jobs in one call (limit 2^32 - 1 items); list fewer jobs", who,
             (unsigned long long)base[n_jobs]);
  // the results of all slices collect here: the caller's arrays are written when the whole call succeeded
  const uint64_t cells = (uint64_t)n_jobs * ncand;
  std::vector<uint32_t> r_u32(cells * 5 + (out_hist ? cells * 64 : 0) + n_jobs, 0u);
  std::vector<uint64_t> r_u64(cells * 4 + n_jobs, 0ull);
  uint32_t *r_hist = out_hist ? r_u32.data() + cells * 5 : nullptr, *r_shift = r_u32.data() + r_u32.size() - n_jobs;
  uint64_t* r_kept = r_u64.data() + cells * 4;
  float gather_ms = 0.f, warp_ms = 0.f, extent_ms = 0.f;
  if (G.total) {   // (no job's song has a row: every query is empty, every output zero)
    rw_tabs T;
    SHZ_TRY(rw_upload(ctx, row_off.data(), n_songs, job_t16, job_f16, n_jobs, base.data(), slot.data(), &T));
    // 2) the slices, from the row counts alone: whole jobs whose items (8 bytes each in the call's warped columns) stay
    // within 1/8 of the workspace limit; a job is never split
    const uint64_t max_items = std::max<uint64_t>(ctx->ws_limit / 64, 1);
    const uint32_t max_jobs = (ctx->debug & SHZ_DEBUG_CATALOG_SMALL_SLICES) ? RW_SMALL_JOBS : (1u << 24);
    std::vector<rw_slice<rw_jobs>> plan;
    std::vector<uint32_t> first;   // the first job of every slice
    uint64_t buf_items = 0;
    for (uint32_t j0 = 0; j0 < n_jobs;) {
      uint32_t nj = 1;
      while (j0 + nj < n_jobs && nj < max_jobs && base[j0 + nj + 1] - base[j0] <= max_items) ++nj;
      const uint64_t n_items = base[j0 + nj] - base[j0];
      plan.push_back({{d_key, d_off, T.d_t16 + j0, T.d_f16 + j0, n_items, {T.d_roff, T.d_song + j0, T.d_base + j0, nj}}, nj});
      first.push_back(j0);
      buf_items = std::max(buf_items, n_items);
      j0 += nj;
    }
    // the songs' largest offsets and the warped columns of the largest slice, once
    uint32_t* d_smax = (uint32_t*)own.get((uint64_t)n_songs * 4);
    uint32_t *d_wkey = (uint32_t*)own.get(buf_items * 4), *d_woff = (uint32_t*)own.get(buf_items * 4);
    if (!d_smax || !d_wkey || !d_woff)
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(2 x %llu + 2 x %llu) failed", who, (unsigned long long)(G.total * 4), (unsigned long long)(buf_items * 4));
    // a warped offset is a query offset of the extent pass: every job's largest must stay below 2^20
    std::vector<uint32_t> smax(n_songs);
    SHZ_HIP(ctx, hipMemsetAsync(d_smax, 0, (uint64_t)n_songs * 4, ctx->stream));
    hipLaunchKernelGGL(rw_song_max_kernel, dim3(nblk(G.total)), dim3(256), 0, ctx->stream, (const uint32_t*)d_off, T.d_roff, n_songs,
                       G.total, d_smax);
    SHZ_HIP(ctx, hipGetLastError());
    const hipError_t e_copy = shz_memcpy(ctx, smax.data(), d_smax, (uint64_t)n_songs * 4, hipMemcpyDeviceToHost);
    const hipError_t e_sync = hipStreamSynchronize(ctx->stream);   // (the call's buffers are freed on return: the stream is idle)
    if (e_copy != hipSuccess || e_sync != hipSuccess) SHZ_FAIL(ctx, SHZ_E_HIP, "%s: reading the songs' largest offsets failed", who);
    for (uint32_t j = 0; j < n_jobs; ++j) {
      const uint64_t img = ((uint64_t)smax[slot[j]] * job_t16[j] + 32768) >> 16;
      if (img >= (1ull << 20))
        SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: song %u of job %u holds offset %u, which the time factor %u / 65536 takes to %llu; warped offsets are query offsets here and must be < 2^20",
                 who, job_sid[j], j, smax[slot[j]], job_t16[j], (unsigned long long)img);
    }
    if (timed) SHZ_HIP(ctx, hipEventRecord(ctx->sp_ev[1], ctx->stream));
    // 3) warp and extent pass, slice by slice: job = one query
    const auto extent = [&](size_t i, const uint64_t* job_off) -> int32_t {
      const uint32_t j0 = first[i], nj = (uint32_t)plan[i].n_seg;
      for (uint32_t e = 0; e < nj; ++e) r_kept[j0 + e] = job_off[e + 1] - job_off[e];
      if (!job_off[nj]) return SHZ_OK;   // (a slice whose rows all left: its queries are empty, its outputs stay zero)
      const uint64_t c0 = (uint64_t)j0 * ncand;
      ex_args S{nj, ncand, cand_sid + c0, cand_dlo + c0, cand_dhi + c0, cand_n + j0, r_u32.data() + c0,
                r_u32.data() + cells + c0, r_u32.data() + 2 * cells + c0, r_u32.data() + 3 * cells + c0,
                r_u32.data() + 4 * cells + c0, r_hist ? r_hist + c0 * 64 : nullptr, r_shift + j0};
      S.out_sum_q = r_u64.data() + c0;
      S.out_sum_u = r_u64.data() + cells + c0;
      S.out_sum_qq = r_u64.data() + 2 * cells + c0;
      S.out_sum_qu = r_u64.data() + 3 * cells + c0;
      return ex_device(ctx, t, who, d_wkey, d_woff, job_off, S);
    };
    SHZ_TRY(rw_run_slices(ctx, who, plan, d_wkey, d_woff, buf_items, timed, extent, &warp_ms, &extent_ms));
    if (timed) SHZ_HIP(ctx, hipEventElapsedTime(&gather_ms, ctx->sp_ev[0], ctx->sp_ev[1]));
  }
  uint32_t* outs[5] = {out_count, out_q_first, out_q_last, out_t_first, out_t_last};
  for (int k = 0; k < 5; ++k) memcpy(outs[k], r_u32.data() + cells * k, cells * 4);
  if (out_hist) memcpy(out_hist, r_hist, cells * 64 * 4);
  memcpy(out_shift, r_shift, (uint64_t)n_jobs * 4);
  uint64_t* sums[4] = {out_sum_q, out_sum_u, out_sum_qq, out_sum_qu};
  for (int k = 0; k < 4; ++k) memcpy(sums[k], r_u64.data() + cells * k, cells * 8);
  if (out_kept) memcpy(out_kept, r_kept, (uint64_t)n_jobs * 8);
  if (ms_gather) *ms_gather = gather_ms;
  if (ms_warp) *ms_warp = warp_ms;
  if (ms_extent) *ms_extent = extent_ms;
  return SHZ_OK;
}
