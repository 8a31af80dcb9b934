// The match / align path on the HBM-resident fingerprint table (storage and build: shz_build.hip).
//   shz_match_batch replaces return_matches + align_matches (recognizer.py:222-338)
#include "shz_table_int.h"

// ======================================================================================== match
#define QOFF_BITS 20
#define QKEY_SHIFT 20
#define QIDX_SHIFT 52
#define MAX_Q_SUB 4096

__global__ void m_compose_kernel(const uint32_t* __restrict__ key32, const uint32_t* __restrict__ q_off,
                                 const uint64_t* __restrict__ query_off /*sub-batch CSR, nq+1*/, uint32_t nq, uint64_t m,
                                 uint32_t nshards, uint32_t shard, uint64_t* __restrict__ c, uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // a shard only looks at the hashes it owns; the others collapse into ONE filler element behind the last query
  // (index nq), which the host drops after the sort.  err[2] != 0: some element is not owned (the filler exists).
  const bool own = i < m && (nshards <= 1 || shard_of(key32[query_off[0] + i], nshards) == shard);
  // (a flag, set by the first wave that sees a foreign element.  A COUNT of the owned elements kept with one atomicAdd per
  // wave -- 41,000 waves on ONE word, and as many atomicMax on the next -- was what this kernel cost: 0.7 ms per 2.6 M
  // elements)
  if (nshards > 1) {
    const bool foreign = i < m && !own;
    if (__ballot(foreign) && (threadIdx.x & 63) == 0 && *(volatile uint32_t*)(err + 2) == 0u) atomicOr(err + 2, 1u);
  }
  // largest query offset (the vote key biases deltas by it) and the "offset too wide" flag: one atomic per wave
  uint32_t o = 0;
  uint64_t h = 0;
  if (own) {
    h = query_off[0] + i;
    o = q_off[h];
  }
  uint32_t omax = o;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) omax = max(omax, (uint32_t)__shfl_xor((int)omax, d, 64));
  // the running maximum only grows: a wave whose own maximum is not above what it reads there has nothing to add (the
  // wave that wrote that value also set the flag if it was too wide)
  if ((threadIdx.x & 63) == 0 && omax > *(volatile uint32_t*)(err + 1)) {
    atomicMax(err + 1, omax);
    if (omax >> QOFF_BITS) atomicOr(err, 1u);
  }
  // the query of an element = the last one whose first hash is not behind it.  A wave's 64 consecutive elements lie in
  // one or two queries: ONE search per wave (scalar loads, for the wave's first element), then each lane walks on from
  // there -- a step or two instead of log2(nq) dependent loads per element (2.9 % of a match at 100k songs before)
  const uint64_t iw = i & ~63ull;   // the wave's first element: the same in every lane, and told so to the compiler
  const uint64_t i0 = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)iw) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(iw >> 32)) << 32);
  if (i0 >= m) return;   // uniform
  const uint64_t h0 = query_off[0] + i0;
  uint32_t w_lo = 0, w_hi = nq;
  while (w_hi - w_lo > 1) {   // uniform
    const uint32_t mid = (w_lo + w_hi) >> 1;
    if (query_off[mid] <= h0) w_lo = mid; else w_hi = mid;
  }
  if (i >= m) return;
  if (!own) { c[i] = (uint64_t)nq << QIDX_SHIFT; return; }
  uint32_t lo = w_lo;
  while (lo + 1 < nq && query_off[lo + 1] <= h) ++lo;
  c[i] = ((uint64_t)lo << QIDX_SHIFT) | ((uint64_t)key32[h] << QKEY_SHIFT) | (o & ((1u << QOFF_BITS) - 1));
}

// Counts that used to travel to the host between the stages (unique elements, groups) stay on the device: kernels
// are launched over a host-known bound and read the count here.  mctl sits in the first 256 bytes of SHZ_WS_MISC0.
struct mctl {
  unsigned long long mu;      // unique (query, key, offset) elements
  unsigned long long ng;      // groups = distinct (query, key)
  unsigned long long rows;    // table rows under the probed keys
  unsigned long long P;       // votes
  unsigned long long G;       // (query, song) groups of the votes
  unsigned long long pad[3];
  unsigned int err[4];        // [0] offset too wide, [1] largest query offset, [2] some hash belongs to another shard
};
// rows under the probed keys: striped over the 8-byte words [16, 16 + M_ROW_STRIPES) of the 256-byte control block
#define M_ROW_STRIPES 16
static_assert(sizeof(mctl) <= 128 && 128 + M_ROW_STRIPES * 8 <= 256, "the stripes sit in the second half of the control block");
// the key cap (shz_set_key_cap): groups dropped in the words [M_CAP_WORD, M_CAP_WORD + M_CAP_STRIPES), their pairs in the
// M_CAP_STRIPES words behind them -- between mctl and the row stripes, zero while no cap is set
#define M_CAP_WORD 10
#define M_CAP_STRIPES 3
static_assert(sizeof(mctl) <= M_CAP_WORD * 8 && (M_CAP_WORD + 2 * M_CAP_STRIPES) * 8 <= 128, "the cap's counters sit behind mctl");
// the filler element that stands for the hashes other shards own sorts last: it is not an element
__global__ void m_fix_mu_kernel(mctl* c, unsigned long long m) {
  if (c->err[2] && c->mu) --c->mu;
}
// flag[i] = 1 where (c[i] >> shift) differs from its predecessor, for i < *n (0 beyond, up to the launch bound)
__global__ void m_head_flag_dn_kernel(const uint64_t* __restrict__ c, const unsigned long long* __restrict__ n,
                                      uint64_t bound, int shift, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= bound) return;
  flag[i] = (i < *n && (i == 0 || (c[i] >> shift) != (c[i - 1] >> shift))) ? 1u : 0u;
}

// ---- head of the match for SMALL query sets (<= MH_MAX hashes, no shard filter) in ONE workgroup: compose, sort,
// unique, group heads.  Replaces m_compose + the radix sort (1 to 21 launches) + 11 flag / scan / compact launches:
// for one 5-10 s query the launches, not the work, were the latency.
#define MH_THREADS 1024
#define MH_ROWS 8
#define MH_MAX (MH_THREADS * MH_ROWS)   // 8,192 elements: two 64 KB key buffers in LDS

// exclusive scan of one value per thread over the 1024-thread workgroup; *total = sum.  tmp: >= 17 entries of LDS.
__device__ __forceinline__ uint32_t mh_block_scan(uint32_t v, uint32_t* total, uint32_t* tmp) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  __syncthreads();   // tmp may still be read from the previous use
  if (lane == 63) tmp[wave] = inc;
  __syncthreads();
  uint32_t woff = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < MH_THREADS / 64; ++w) {
    const uint32_t x = tmp[w];
    if (w < wave) woff += x;
    tot += x;
  }
  *total = tot;
  return woff + inc - v;
}

// Stable LSD radix sort of m <= MH_MAX keys that sit in sk[0], on bits [bit_lo, bit_hi), 8 bits per pass, all in LDS.
// Wave w owns the slice [w * 64 rows, (w + 1) * 64 rows), rows = ceil(m / 1024): every pass ranks a slice's elements among themselves by ballots
// (the scheme of sort_scatter_kernel), prefixes the per-wave digit counts over the waves and the digits, and scatters
// into the other buffer.  Bits on which no two keys differ (`diff` = OR of all keys ^ AND of all keys) are skipped: a
// digit begins at the next differing bit.  Returns the index of the buffer that holds the result.  Ends with a barrier.
__device__ __forceinline__ int mh_lds_sort(uint64_t (*sk)[MH_MAX], uint16_t (*wrun)[256], uint32_t* dbase, uint32_t m,
                                           int bit_lo, int bit_hi, unsigned long long diff) {
  const int rows = (int)((m + MH_THREADS - 1) / MH_THREADS);   // rows of 64 elements per wave: the slices shrink with m
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const unsigned long long lt = (1ull << lane) - 1ull;
  int cur = 0;
  for (int shift = bit_lo; shift < bit_hi; shift += 8) {
    // a digit starts at the next bit on which any two keys differ (not at a multiple of 8): offsets of 8 bits + 32 key bits
    // are five passes wherever the fields sit, not six
    const unsigned long long rest = shift < 64 ? diff >> shift : 0ull;
    if (rest == 0ull) break;                        // uniform
    shift += __ffsll((long long)rest) - 1;
    if (shift >= bit_hi) break;
    const uint32_t dmask = (1u << min(8, bit_hi - shift)) - 1u;
    for (int i = j; i < (MH_THREADS / 64) * 256; i += MH_THREADS) (&wrun[0][0])[i] = 0;
    __syncthreads();
    uint64_t k[MH_ROWS];
    uint32_t rank[MH_ROWS];
#pragma unroll
    for (int r = 0; r < MH_ROWS; ++r) {
      if (r >= rows) break;   // uniform
      const uint32_t li = (uint32_t)wave * (rows * 64) + (uint32_t)r * 64 + lane;
      const bool valid = li < m;
      k[r] = valid ? sk[cur][li] : 0;
      const uint32_t d = (uint32_t)(k[r] >> shift) & dmask;
      unsigned long long peers = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const unsigned long long mm = __ballot((d >> b) & 1u);
        peers &= ((d >> b) & 1u) ? mm : ~mm;
      }
      const uint32_t rk = (uint32_t)__popcll(peers & lt);
      const uint32_t run = wrun[wave][d];
      rank[r] = run + rk;
      if (valid && rk == 0) wrun[wave][d] = (uint16_t)(run + (uint32_t)__popcll(peers));
    }
    __syncthreads();
    if (j < 256) {   // per digit: exclusive prefix over the waves, total of the digit
      uint32_t acc = 0;
#pragma unroll
      for (int w = 0; w < MH_THREADS / 64; ++w) {
        const uint32_t c = wrun[w][j];
        wrun[w][j] = (uint16_t)acc;
        acc += c;
      }
      dbase[j] = acc;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan of the 256 digit totals: 4 per lane
      uint32_t a0 = dbase[4 * lane], a1 = dbase[4 * lane + 1], a2 = dbase[4 * lane + 2], a3 = dbase[4 * lane + 3];
      uint32_t sum = a0 + a1 + a2 + a3, inc = sum;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
      }
      uint32_t ex = inc - sum;
      dbase[4 * lane] = ex; ex += a0;
      dbase[4 * lane + 1] = ex; ex += a1;
      dbase[4 * lane + 2] = ex; ex += a2;
      dbase[4 * lane + 3] = ex;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < MH_ROWS; ++r) {
      if (r >= rows) break;   // uniform
      const uint32_t li = (uint32_t)wave * (rows * 64) + (uint32_t)r * 64 + lane;
      if (li < m) {
        const uint32_t d = (uint32_t)(k[r] >> shift) & dmask;
        sk[cur ^ 1][dbase[d] + wrun[wave][d] + rank[r]] = k[r];
      }
    }
    cur ^= 1;
    __syncthreads();
  }
  return cur;
}

// the votes of a small match (<= MH_MAX of them) sorted in one workgroup instead of 3-4 passes x 3 launches
__global__ __launch_bounds__(MH_THREADS) void m_sort_small_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                                  uint32_t n, int bit_lo, int bit_hi) {
  __shared__ uint64_t sk[2][MH_MAX];
  __shared__ uint16_t wrun[MH_THREADS / 64][256];
  __shared__ uint32_t dbase[256];
  for (uint32_t i = threadIdx.x; i < n; i += MH_THREADS) sk[0][i] = in[i];
  __syncthreads();
  const int cur = mh_lds_sort(sk, wrun, dbase, n, bit_lo, bit_hi, ~0ull);
  for (uint32_t i = threadIdx.x; i < n; i += MH_THREADS) out[i] = sk[cur][i];
}

__global__ __launch_bounds__(MH_THREADS) void m_head_small_kernel(const uint32_t* __restrict__ key32,
                                                                  const uint32_t* __restrict__ q_off,
                                                                  const uint64_t* __restrict__ query_off, uint32_t nq,
                                                                  uint32_t m, int bit_hi, uint64_t* __restrict__ E,
                                                                  uint32_t* __restrict__ gs, mctl* __restrict__ ctl) {
  __shared__ uint64_t sk[2][MH_MAX];
  __shared__ uint16_t wrun[MH_THREADS / 64][256];
  __shared__ uint32_t dbase[256], tmp[20];
  __shared__ unsigned long long s_or, s_and;
  __shared__ uint32_t s_omax;
  const int j = threadIdx.x, lane = j & 63;
  if (j == 0) { s_or = 0; s_and = ~0ull; s_omax = 0; }
  __syncthreads();
  // compose (query, key, offset) elements; wave w owns the slice [w * 512, w * 512 + 512)
  const uint64_t h0 = query_off[0];
  unsigned long long vor = 0, vand = ~0ull;
  uint32_t omax = 0;
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r) {
    const uint32_t li = (uint32_t)r * MH_THREADS + j;   // (any order: the sort follows)
    if (li < m) {
      const uint64_t h = h0 + li;
      const uint32_t o = q_off[h];
      uint32_t lo = 0, hi = nq;
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (query_off[mid] <= h) lo = mid; else hi = mid;
      }
      const uint64_t c = ((uint64_t)lo << QIDX_SHIFT) | ((uint64_t)key32[h] << QKEY_SHIFT) | (o & ((1u << QOFF_BITS) - 1));
      sk[0][li] = c;
      vor |= c;
      vand &= c;
      omax = max(omax, o);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    vor |= __shfl_xor((long long)vor, d, 64);
    vand &= __shfl_xor((long long)vand, d, 64);
    omax = max(omax, (uint32_t)__shfl_xor((int)omax, d, 64));
  }
  if (lane == 0) {
    atomicOr(&s_or, vor);
    atomicAnd(&s_and, vand);
    atomicMax(&s_omax, omax);
  }
  __syncthreads();
  const unsigned long long diff = s_or ^ s_and;   // bits on which the elements differ at all: other digits need no pass
  const int cur = mh_lds_sort(sk, wrun, dbase, m, 0, bit_hi, diff);
  // unique elements: thread j looks at the MH_ROWS consecutive sorted elements [j * 8, j * 8 + 8)
  const uint64_t* S = sk[cur];
  uint64_t* U = sk[cur ^ 1];
  uint32_t f = 0, cnt = 0;
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r) {
    const uint32_t i = (uint32_t)j * MH_ROWS + r;
    if (i < m && (i == 0 || S[i] != S[i - 1])) { f |= 1u << r; ++cnt; }
  }
  uint32_t mu;
  uint32_t pos = mh_block_scan(cnt, &mu, tmp);
  uint64_t mine[MH_ROWS];
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r) mine[r] = S[(uint32_t)j * MH_ROWS + r];
  __syncthreads();   // everybody has read S before U (the other buffer) is written; U != S, but keep the phases apart
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r)
    if ((f >> r) & 1u) { U[pos] = mine[r]; E[pos] = mine[r]; ++pos; }
  __syncthreads();
  // group heads: first element of every distinct (query, key)
  f = 0; cnt = 0;
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r) {
    const uint32_t i = (uint32_t)j * MH_ROWS + r;
    if (i < mu && (i == 0 || (U[i] >> QKEY_SHIFT) != (U[i - 1] >> QKEY_SHIFT))) { f |= 1u << r; ++cnt; }
  }
  uint32_t ng;
  pos = mh_block_scan(cnt, &ng, tmp);
#pragma unroll
  for (int r = 0; r < MH_ROWS; ++r)
    if ((f >> r) & 1u) gs[pos++] = (uint32_t)j * MH_ROWS + r;
  if (j == 0) {
    gs[ng] = mu;
    ctl->mu = mu;
    ctl->ng = ng;
    ctl->err[0] = (s_omax >> QOFF_BITS) ? 1u : 0u;
    ctl->err[1] = s_omax;
    ctl->err[2] = 0;   // (one shard: nothing is foreign)
  }
}

// flag[i] = 1 where (c[i] >> shift) differs from its predecessor
__global__ void m_head_flag_kernel(const uint64_t* __restrict__ c, uint64_t n, int shift, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flag[i] = (i == 0 || (c[i] >> shift) != (c[i - 1] >> shift)) ? 1u : 0u;
}

__global__ void m_compact_vals_kernel(const uint64_t* __restrict__ c, const uint32_t* __restrict__ flag,
                                      const uint32_t* __restrict__ pos, uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[pos[i]] = c[i];
}

// starts[pos[i]] = i for heads; starts[n_heads] = n
__global__ void m_compact_idx_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                     const unsigned long long* __restrict__ n_dev, uint64_t bound,
                                     const unsigned long long* __restrict__ n_heads, uint32_t* __restrict__ starts) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = *n_dev;
  if (i == 0) starts[*n_heads] = (uint32_t)n;
  if (i < bound && i < n && flag[i]) starts[pos[i]] = (uint32_t)i;
}

// probe: rows [lo, lo+rows) of every (query, key) group g in every segment sg, one thread per x = g * nseg + sg.
// g_lo[x] = first row, g_pairs[x] = rows x offsets of the group (the votes it expands to); x = ng * nseg is the
// sentinel that makes the exclusive scan end in the total.
__global__ void m_probe_kernel(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                               const unsigned long long* __restrict__ ng_dev, uint64_t bound,
                               const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ g_lo,
                               uint64_t* __restrict__ g_pairs, unsigned long long* __restrict__ rows_total,
                               uint32_t* __restrict__ rb, uint32_t rb_words) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (uint64_t i = x; i < rb_words; i += (uint64_t)gridDim.x * blockDim.x) rb[i] = 0u;   // the result block (a fill launch otherwise)
  const uint64_t nx = (uint64_t)*ng_dev * nseg;   // <= bound - 1: slots past nx count no pairs
  unsigned long long s = 0;
  if (x < nx) {
    const uint32_t g = (uint32_t)(x / nseg), sg = (uint32_t)(x - (uint64_t)g * nseg);
    const uint32_t e0 = gs[g];
    const uint32_t key = (uint32_t)(E[e0] >> QKEY_SHIFT);
    const uint64_t b = key >> 8;
    const uint32_t* __restrict__ tkey = segs[sg].key;
    uint32_t lo = 0, rows = 0;
    // a segment is asked only for keys inside [its first key, its last bucket]: the segments of one k-way merge hold
    // disjoint key ranges, so one of them answers and the others cost this compare (not a bucket fetch + searches)
    if (b < segs[sg].nbuckets && key >= segs[sg].key_lo && segs[sg].n) {
      uint32_t l = segs[sg].bucket[b], h = segs[sg].bucket[b + 1];
      const uint32_t h0 = h;
      while (l < h) {  // lower_bound(key)
        uint32_t mid = l + ((h - l) >> 1);
        if (tkey[mid] < key) l = mid + 1; else h = mid;
      }
      lo = l;
      h = h0;
      while (l < h) {  // upper_bound(key)
        uint32_t mid = l + ((h - l) >> 1);
        if (tkey[mid] <= key) l = mid + 1; else h = mid;
      }
      rows = l - lo;
    }
    g_lo[x] = lo;
    g_pairs[x] = (uint64_t)rows * (gs[g + 1] - e0);
    s = rows;
  } else if (x < bound) {
    g_pairs[x] = 0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor((long long)s, d, 64);
  // (statistics only.  One word for all waves cost more than the searches: 31,000 atomics on one address per call; the
  // count is kept in M_ROW_STRIPES words of the control block instead and summed on the host)
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(rows_total + (blockIdx.x & (M_ROW_STRIPES - 1)), s);
}

// ---- the key cap (shz_set_key_cap): a key that holds more than `cap` table rows over all segments votes for nobody.  Between
// the probe and the scan of its counts, one thread per group g < *n_dev sums the rows of the group's nseg sub-groups --
// vals[g * nseg + sg] / (elements of the group) -- and zeroes all nseg entries where the sum exceeds the cap: the scan, and
// with it the expand, the tiles, the queued fold, the per-query counts and the sink, then never see the key.  gs == NULL (the
// extent pass, whose slots are (element, segment) and hold rows): one element a group.  ctr (NULL: not counted): dropped
// groups and dropped pairs, reduced over the wave, one atomic a wave and counter into M_CAP_STRIPES striped words each.
__device__ __forceinline__ bool key_cap_drop(uint64_t* __restrict__ vals, uint32_t nseg, uint32_t elems, uint64_t cap,
                                             unsigned long long* pairs) {
  unsigned long long rows = 0, p = 0;
  for (uint32_t sg = 0; sg < nseg; ++sg) {
    const uint64_t v = vals[sg];
    p += v;
    rows += v / elems;
  }
  *pairs = p;
  if (rows <= cap) return false;
  for (uint32_t sg = 0; sg < nseg; ++sg) vals[sg] = 0;
  return true;
}
__global__ void key_cap_kernel(uint64_t* __restrict__ vals, const uint32_t* __restrict__ gs,
                               const unsigned long long* __restrict__ n_dev, uint64_t bound, uint32_t nseg, uint64_t cap,
                               unsigned long long* __restrict__ ctr) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint64_t n = *n_dev < bound ? *n_dev : bound;   // (the launch and the buffers are sized by the bound)
  unsigned long long dg = 0, dp = 0;
  if (g < n) {
    unsigned long long p;
    if (key_cap_drop(vals + g * nseg, nseg, gs ? gs[g + 1] - gs[g] : 1u, cap, &p)) {
      dg = 1;
      dp = p;
    }
  }
  if (!ctr) return;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    dg += __shfl_xor((long long)dg, d, 64);
    dp += __shfl_xor((long long)dp, d, 64);
  }
  if ((threadIdx.x & 63) == 0 && dg) {
    atomicAdd(ctr + blockIdx.x % M_CAP_STRIPES, dg);
    atomicAdd(ctr + M_CAP_STRIPES + blockIdx.x % M_CAP_STRIPES, dp);
  }
}
int32_t shz_key_cap_apply(shz_ctx* ctx, uint64_t* d_vals, const uint32_t* d_gs, const unsigned long long* d_n, uint64_t bound,
                          uint32_t nseg, unsigned long long* d_ctr) {
  if (!ctx->key_cap || bound == 0) return SHZ_OK;
  hipLaunchKernelGGL(key_cap_kernel, dim3(nblk(bound)), dim3(256), 0, ctx->stream, d_vals, d_gs, d_n, bound, nseg, ctx->key_cap,
                     d_ctr);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

__global__ void m_query_stats_kernel(const uint64_t* __restrict__ E, const mctl* __restrict__ ctl,
                                     const uint32_t* __restrict__ gs, const uint64_t* __restrict__ po, uint32_t nseg,
                                     uint32_t nq, uint32_t* __restrict__ nhash, uint64_t* __restrict__ npairs) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nq) return;
  const uint32_t mu = (uint32_t)ctl->mu, ng = (uint32_t)ctl->ng;
  // elements of q: E in [q << 52, (q+1) << 52)
  auto lb_e = [&](uint64_t target) {
    uint32_t l = 0, h = mu;
    while (l < h) { uint32_t mid = l + ((h - l) >> 1); if (E[mid] < target) l = mid + 1; else h = mid; }
    return l;
  };
  auto lb_g = [&](uint64_t target) {
    uint32_t l = 0, h = ng;
    while (l < h) { uint32_t mid = l + ((h - l) >> 1); if (E[gs[mid]] < target) l = mid + 1; else h = mid; }
    return l;
  };
  // (q + 1) << 52 wraps to 0 for query 4,095 of a full sub-batch (MAX_Q_SUB): its elements run to the end of E
  const uint64_t a = (uint64_t)q << QIDX_SHIFT, b = (uint64_t)(q + 1) << QIDX_SHIFT;
  const bool to_end = ((q + 1) >> (64 - QIDX_SHIFT)) != 0;
  nhash[q] = (to_end ? mu : lb_e(b)) - lb_e(a);
  npairs[q] = po[(uint64_t)(to_end ? ng : lb_g(b)) * nseg] - po[(uint64_t)lb_g(a) * nseg];
}

struct m_bits { int sb, dbits, qb; uint32_t bias; };  // bias = max query offset of the sub-batch: delta + bias >= 0

// expand: pair p = (query hash element, table row) of sub-group x = (group g, segment sg), packed as a vote.  A
// workgroup owns M_EXP_TILE consecutive pairs.  m_tile_start_kernel finds the sub-group of every tile's first pair; a
// tile spans a handful of sub-groups (the whole po[] has ~1e6 entries), so the workgroup copies their descriptors to
// LDS once and every pair is resolved from there: the only per-pair global traffic is the table row and the store.
#define M_EXP_PER 8
#define M_EXP_TILE (256 * M_EXP_PER)
#define M_EXP_SUB 512   // sub-groups per tile that fit the LDS tables (more: the same search over global memory)

// tile_x[t] = last x in [0, nx) with po[x] <= min(t * M_EXP_TILE, P - 1), t = 0 .. ntiles
// (votes [v_lo, P) of the sub-batch: a vote pass may cover a range of queries only)
__global__ void m_tile_start_kernel(const uint64_t* __restrict__ po, uint32_t nx, uint64_t v_lo, uint64_t P, uint32_t ntiles,
                                    uint32_t* __restrict__ tile_x) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t > ntiles) return;
  const uint64_t p = min(v_lo + (uint64_t)t * M_EXP_TILE, P - 1);
  uint32_t l = 0, h = nx;
  while (h - l > 1) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (po[mid] <= p) l = mid; else h = mid;
  }
  tile_x[t] = l;
}

// the same for EVERY vote pass of a sub-batch in one launch: pass p covers the votes [pv[2p], pv[2p+1]) and owns the
// entries [toff[p], toff[p+1]) of tile_x (its tiles + 1)
__global__ void m_tile_start_all_kernel(const uint64_t* __restrict__ po, uint32_t nx, const uint64_t* __restrict__ pv,
                                        const uint32_t* __restrict__ toff, uint32_t n_pass, uint32_t* __restrict__ tile_x) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= toff[n_pass]) return;
  uint32_t lo = 0, hi = n_pass;   // last pass with toff[p] <= e
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (toff[mid] <= e) lo = mid; else hi = mid;
  }
  const uint64_t v_lo = pv[2 * lo], P = pv[2 * lo + 1];
  const uint64_t p = min(v_lo + (uint64_t)(e - toff[lo]) * M_EXP_TILE, P - 1);
  uint32_t l = 0, h = nx;
  while (h - l > 1) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (po[mid] <= p) l = mid; else h = mid;
  }
  tile_x[e] = l;
}

#define M_NO_QUERY_BITS INT64_MIN   // q_base of a pass whose votes carry no query index (segmented sort: position says it)
__device__ __forceinline__ uint64_t m_vote(uint64_t e, uint32_t sid, uint32_t off, uint32_t first, m_bits mb, int64_t q_base) {
  const uint64_t q = q_base == M_NO_QUERY_BITS ? 0ull : (uint64_t)((int64_t)(e >> QIDX_SHIFT) + q_base);
  const uint32_t qo = (uint32_t)e & ((1u << QOFF_BITS) - 1);
  const uint64_t dprime = (uint64_t)off + mb.bias - qo;  // delta + bias >= 0
  return ((((q << mb.sb) | sid) << mb.dbits | dprime) << 1) | first;
}

// Votes [v_lo, P) of the sub-batch go to v[0 ..): VT = uint64_t, or uint32_t when a pass's queries, song ids and deltas
// fit 31 bits (q_base then shifts the query index to the pass's first query).
// The votes [base, end) of the sub-batch, whose sub-groups are [xA, xB], go to v[base - v_lo ..).  HIST: the digit
// (vote >> shift) & dmask of every vote is counted in h (LDS, 256 counters of the caller).  May be called in a loop: the
// tables below are rewritten per call, behind a barrier.
template <typename VT, bool HIST>
__device__ __forceinline__ void m_expand_chunk(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                                               const uint64_t* __restrict__ po, const uint32_t* __restrict__ g_lo,
                                               const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint64_t v_lo,
                                               uint64_t base, uint64_t end, uint32_t xA, uint32_t xB, m_bits mb,
                                               int64_t q_base, VT* __restrict__ v, uint32_t* h, int shift, uint32_t dmask) {
  __shared__ uint64_t s_po[M_EXP_SUB], s_e[M_EXP_SUB];
  __shared__ uint32_t s_lo[M_EXP_SUB], s_e0[M_EXP_SUB], s_noff[M_EXP_SUB], s_sg[M_EXP_SUB];
  __shared__ const uint32_t* s_sid[SHZ_MAX_SEGS];
  __shared__ const uint32_t* s_off[SHZ_MAX_SEGS];
  if (HIST) __syncthreads();   // (the previous chunk's tables are still being read)
  const uint64_t last = end - 1;
  const uint32_t cnt = xB - xA + 1;
  int iters = 0;
  while ((1u << iters) < cnt) ++iters;  // uniform
  uint64_t p[M_EXP_PER];
  uint32_t l[M_EXP_PER], hh[M_EXP_PER];
#pragma unroll
  for (int j = 0; j < M_EXP_PER; ++j)
    p[j] = min(base + (uint64_t)j * 256 + threadIdx.x, last);  // clamped: lanes past the end redo the last pair, unstored
  if (threadIdx.x < nseg) { s_sid[threadIdx.x] = segs[threadIdx.x].sid; s_off[threadIdx.x] = segs[threadIdx.x].off; }
  if (cnt <= M_EXP_SUB) {  // uniform
    for (uint32_t i = threadIdx.x; i < cnt; i += 256) {
      const uint32_t x = xA + i, g = x / nseg;
      const uint32_t e0 = gs[g];
      s_po[i] = po[x];
      s_lo[i] = g_lo[x];
      s_e0[i] = e0;
      s_noff[i] = gs[g + 1] - e0;
      s_sg[i] = x - g * nseg;
      s_e[i] = E[e0];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < M_EXP_PER; ++j) { l[j] = 0; hh[j] = cnt; }  // last i in [0, cnt) with s_po[i] <= p
    for (int it = 0; it < iters; ++it) {
#pragma unroll
      for (int j = 0; j < M_EXP_PER; ++j) {
        const uint32_t mid = (l[j] + hh[j]) >> 1;   // == l once h - l <= 1: s_po[l] <= p keeps l
        if (s_po[mid] <= p[j]) l[j] = mid; else hh[j] = mid;
      }
    }
#pragma unroll
    for (int j = 0; j < M_EXP_PER; ++j) {
      const uint32_t i = l[j];
      const uint32_t noff = s_noff[i];
      const uint32_t r = (uint32_t)(p[j] - s_po[i]);  // < P < 2^32
      uint32_t ridx = r, oi = 0;                      // row number inside the sub-group's rows, offset of the hash
      uint64_t e = s_e[i];
      if (noff != 1) { ridx = r / noff; oi = r - ridx * noff; e = E[s_e0[i] + oi]; }
      const uint32_t row = s_lo[i] + ridx, sg = s_sg[i];
      const uint64_t out = m_vote(e, s_sid[sg][row], s_off[sg][row], oi == 0 ? 1u : 0u, mb, q_base);
      const uint64_t pj = base + (uint64_t)j * 256 + threadIdx.x;
      if (pj < end) {
        v[pj - v_lo] = (VT)out;
        if (HIST) atomicAdd(&h[((uint32_t)out >> shift) & dmask], 1u);
      }
    }
    return;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < M_EXP_PER; ++j) { l[j] = xA; hh[j] = xB + 1; }  // last x in [xA, xB] with po[x] <= p
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int j = 0; j < M_EXP_PER; ++j) {
      const uint32_t mid = (l[j] + hh[j]) >> 1;
      if (po[mid] <= p[j]) l[j] = mid; else hh[j] = mid;
    }
  }
#pragma unroll 2
  for (int j = 0; j < M_EXP_PER; ++j) {
    const uint32_t x = l[j], g = x / nseg, sg = x - g * nseg;
    const uint32_t e0 = gs[g], noff = gs[g + 1] - e0;
    const uint32_t r = (uint32_t)(p[j] - po[x]);
    uint32_t ridx = r, oi = 0;
    if (noff != 1) { ridx = r / noff; oi = r - ridx * noff; }
    const uint32_t row = g_lo[x] + ridx;
    const uint64_t out = m_vote(E[e0 + oi], s_sid[sg][row], s_off[sg][row], oi == 0 ? 1u : 0u, mb, q_base);
    const uint64_t pj = base + (uint64_t)j * 256 + threadIdx.x;
    if (pj < end) {
      v[pj - v_lo] = (VT)out;
      if (HIST) atomicAdd(&h[((uint32_t)out >> shift) & dmask], 1u);
    }
  }
}

// one tile of M_EXP_TILE votes per workgroup
template <typename VT>
__device__ __forceinline__ void m_expand_tile(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                                              const uint32_t* __restrict__ tile_x, const uint64_t* __restrict__ po,
                                              const uint32_t* __restrict__ g_lo,
                                              const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint64_t v_lo,
                                              uint64_t P, m_bits mb, int64_t q_base, VT* __restrict__ v) {
  const uint64_t base = v_lo + (uint64_t)blockIdx.x * M_EXP_TILE;
  m_expand_chunk<VT, false>(E, gs, po, g_lo, segs, nseg, v_lo, base, min(base + M_EXP_TILE, P), tile_x[blockIdx.x],
                            tile_x[blockIdx.x + 1], mb, q_base, v, nullptr, 0, 0u);
}

template <typename VT>
__global__ __launch_bounds__(256) void m_expand_kernel(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                                                       const uint32_t* __restrict__ tile_x, const uint64_t* __restrict__ po,
                                                       const uint32_t* __restrict__ g_lo,
                                                       const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint64_t v_lo,
                                                       uint64_t P, m_bits mb, int64_t q_base, VT* __restrict__ v) {
  m_expand_tile<VT>(E, gs, tile_x, po, g_lo, segs, nseg, v_lo, P, mb, q_base, v);
}

// ---- expand by the BLOCKS of the segmented vote sort (shz_sort_u32_seg): workgroup b produces the votes of sort block b
// (<= 4,096 or 8,192 votes of one query, M_EXP_TILE at a time) and counts their first-pass digits on the way, in the
// sort's table layout -- the sort's first counting kernel (a pass over all votes at 3.4 TB/s, 5 % of a match at 1M songs)
// is not run.  cx[b * (cpb + 1) + c], c = 0 .. cpb: the sub-group of the first vote of chunk c of block b (cpb chunks of
// M_EXP_TILE votes per block; positions past the block's end name its end).
__device__ __forceinline__ void m_block_range(const shz_seg_plan& sp, uint32_t tile, uint32_t b, uint32_t& seg, uint32_t& bl,
                                              uint32_t& bs, uint32_t& be) {
  uint32_t i = 0, hi = sp.nq;                        // last segment with bq[i] <= b (empty segments have no blocks)
  while (hi - i > 1) {
    const uint32_t mid = (i + hi) >> 1;
    if (sp.bq[mid] <= b) i = mid; else hi = mid;
  }
  seg = i;
  bl = b - sp.bq[i];
  bs = sp.qv[i] + bl * tile;
  be = min(bs + tile, sp.qv[i + 1]);
}

__global__ void m_chunk_start_kernel(const uint64_t* __restrict__ po, uint32_t nx, shz_seg_plan sp, uint32_t tile, uint64_t v_lo,
                                     uint64_t v_hi, uint32_t* __restrict__ cx) {
  const uint32_t cpb = tile / M_EXP_TILE, nb = sp.bq[sp.nq];
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nb * (cpb + 1)) return;
  const uint32_t b = e / (cpb + 1), c = e - b * (cpb + 1);
  uint32_t seg, bl, bs, be;
  m_block_range(sp, tile, b, seg, bl, bs, be);
  const uint64_t p = min(v_lo + min(bs + c * M_EXP_TILE, be), v_hi - 1);
  uint32_t l = 0, h = nx;
  while (h - l > 1) {
    const uint32_t mid = l + ((h - l) >> 1);
    if (po[mid] <= p) l = mid; else h = mid;
  }
  cx[e] = l;
}

__global__ __launch_bounds__(256, 8) void m_expand_blocks_kernel(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                                                              const uint32_t* __restrict__ cx, const uint64_t* __restrict__ po,
                                                              const uint32_t* __restrict__ g_lo,
                                                              const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint64_t v_lo,
                                                              shz_seg_plan sp, uint32_t tile, m_bits mb, int shift, uint32_t dmask,
                                                              uint32_t* __restrict__ v, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;   // (every chunk starts with a barrier)
  const uint32_t cpb = tile / M_EXP_TILE;
  uint32_t seg, bl, bs, be;
  m_block_range(sp, tile, blockIdx.x, seg, bl, bs, be);
  const uint32_t* cxb = cx + (uint64_t)blockIdx.x * (cpb + 1);
  for (uint32_t c = 0; c < cpb; ++c) {   // uniform
    const uint32_t cb = bs + c * M_EXP_TILE;
    if (cb >= be) break;
    m_expand_chunk<uint32_t, true>(E, gs, po, g_lo, segs, nseg, v_lo, v_lo + cb, v_lo + min(cb + (uint32_t)M_EXP_TILE, be), cxb[c],
                                   cxb[c + 1], mb, M_NO_QUERY_BITS, v, h, shift, dmask);
  }
  __syncthreads();
  const uint32_t nbs = sp.bq[seg + 1] - sp.bq[seg];
  hist[((uint64_t)sp.bq[seg] << 8) + bl + (uint64_t)threadIdx.x * nbs] = h[threadIdx.x];
}

// ---- one small query, votes queued BEFORE their number is known on the host
// A single query against a small or medium table has a few thousand votes, and its match is a chain of short launches: the
// read-back of the vote count in the middle of it (a stream sync, ~30 us) is a sixth of the whole call.  For one query
// whose hashes went through m_head_small_kernel the host therefore queues the one-workgroup vote path behind the probe
// at once, sized for VT_ONE_WG_MAX votes; these kernels read the vote count from the control block and do nothing when it
// is larger -- the host then sees that count in the one read-back and continues as if nothing had been queued.
//
// m_spec_plan_kernel: tile_x of the expand tiles (as m_tile_start_kernel) + the single vote range (as vt_one_range_kernel)
// + the zeroed result block
__global__ void m_spec_plan_kernel(const uint64_t* __restrict__ po, const mctl* __restrict__ ctl, uint32_t nseg, uint64_t cap,
                                   uint32_t* __restrict__ tile_x, uint32_t* __restrict__ n_heavy, uint2* __restrict__ heavy,
                                   uint32_t* __restrict__ heavy_q, uint32_t* __restrict__ rb, uint32_t rb_words) {
  for (uint32_t i = threadIdx.x; i < rb_words; i += blockDim.x) rb[i] = 0u;   // the result block (the host's fill otherwise)
  const uint64_t P = ctl->P;
  const bool ok = P > 0 && P <= cap;
  if (threadIdx.x == 0) {
    *n_heavy = ok ? 1u : 0u;
    heavy[0] = make_uint2(0u, ok ? (uint32_t)P : 0u);
    heavy_q[0] = 0u;
  }
  if (!ok) return;
  const uint32_t nx = (uint32_t)ctl->ng * nseg, ntiles = (uint32_t)((P + M_EXP_TILE - 1) / M_EXP_TILE);
  for (uint32_t t = threadIdx.x; t <= ntiles; t += blockDim.x) {
    const uint64_t p = min((uint64_t)t * M_EXP_TILE, P - 1);
    uint32_t l = 0, h = nx;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (po[mid] <= p) l = mid; else h = mid;
    }
    tile_x[t] = l;
  }
}

__global__ __launch_bounds__(256) void m_expand_spec_kernel(const uint64_t* __restrict__ E, const uint32_t* __restrict__ gs,
                                                            const uint32_t* __restrict__ tile_x, const uint64_t* __restrict__ po,
                                                            const uint32_t* __restrict__ g_lo,
                                                            const shz_seg_dev* __restrict__ segs, uint32_t nseg,
                                                            const mctl* __restrict__ ctl, uint64_t cap, m_bits mb,
                                                            uint32_t* __restrict__ v) {
  const uint64_t P = ctl->P;
  if (P == 0 || P > cap || (uint64_t)blockIdx.x * M_EXP_TILE >= P) return;   // uniform, before any barrier
  m_expand_tile<uint32_t>(E, gs, tile_x, po, g_lo, segs, nseg, 0ull, P, mb, (int64_t)0, v);
}

// ---- fold of the sorted votes into one record per (query, sid) group
// The votes are sorted by (query, sid, delta, flag).  A thread owns RG_PER consecutive votes and every group whose FIRST
// vote lies among them; it follows such a group past its own votes to the group's end (groups average a few votes, the
// true match a few hundred).  Record = (best count of one delta, smallest delta reaching it, votes with the
// first-offset flag = rows matched).  Records are written densely in group order: m_gcount_kernel counts the heads
// per wave, a scan of those counts gives every wave its first slot.
#define RG_PER 8
#define RG_LONG_ITERS 16   // loads of RG_PER votes a thread follows a group before handing it over
#define RG_LONG_CAP 16384  // long groups per vote pass that get a workgroup of their own

__device__ __forceinline__ int rg_load(const uint64_t* __restrict__ v, uint64_t i0, uint64_t P, uint64_t (&e)[RG_PER]) {
  if (i0 + RG_PER <= P) {
    const ulonglong2* p2 = (const ulonglong2*)(v + i0);
#pragma unroll
    for (int j = 0; j < RG_PER / 2; ++j) { const ulonglong2 x = p2[j]; e[2 * j] = x.x; e[2 * j + 1] = x.y; }
    return RG_PER;
  }
  const int n = i0 < P ? (int)(P - i0) : 0;
#pragma unroll
  for (int j = 0; j < RG_PER; ++j) e[j] = j < n ? v[i0 + j] : 0;
  return n;
}

// the vote before a thread's first one: the neighbour lane's last vote, or memory for lane 0 (0 = "none" for i0 == 0)
__device__ __forceinline__ uint64_t rg_prev(const uint64_t* __restrict__ v, uint64_t i0, uint64_t P, uint64_t e_last) {
  uint64_t prev = (uint64_t)__shfl_up((long long)e_last, 1, 64);
  if ((threadIdx.x & 63) == 0) prev = (i0 > 0 && i0 <= P) ? v[i0 - 1] : 0;
  return prev;
}

__global__ __launch_bounds__(256) void m_gcount_kernel(const uint64_t* __restrict__ v, uint64_t P, int gshift,
                                                       uint32_t* __restrict__ wcnt) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i0 = t * RG_PER;
  uint64_t e[RG_PER];
  const int n = rg_load(v, i0, P, e);
  uint64_t prev = rg_prev(v, i0, P, e[RG_PER - 1]);
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < RG_PER; ++j) {
    if (j < n && (i0 + j == 0 || (e[j] >> gshift) != (prev >> gshift))) ++c;
    prev = e[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor((int)c, d, 64);
  if ((threadIdx.x & 63) == 0) wcnt[t >> 6] = c;
}

struct rg_state {
  uint64_t grp, curd;
  uint32_t best, bestd, cur, dedup;
};

__device__ __forceinline__ void rg_add(rg_state& s, uint64_t val, uint64_t dmask) {
  const uint64_t d = (val >> 1) & dmask;
  if (d != s.curd) {
    if (s.cur > s.best) { s.best = s.cur; s.bestd = (uint32_t)s.curd; }
    s.curd = d;
    s.cur = 0;
  }
  ++s.cur;
  s.dedup += (uint32_t)(val & 1);
}

__global__ __launch_bounds__(256) void m_reduce_kernel(const uint64_t* __restrict__ v, uint64_t P, m_bits mb,
                                                       const uint32_t* __restrict__ wbase, uint64_t* __restrict__ g_pack,
                                                       uint32_t* __restrict__ g_delta, uint32_t* __restrict__ g_dedup,
                                                       uint32_t* __restrict__ qstart, uint32_t* __restrict__ long_cnt,
                                                       uint2* __restrict__ long_list) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t i0 = t * RG_PER;
  const int gshift = mb.dbits + 1, qshift = mb.sb + mb.dbits + 1;
  const uint64_t dmask = (1ull << mb.dbits) - 1, smask = (1ull << mb.sb) - 1;
  uint64_t e[RG_PER];
  const int n = rg_load(v, i0, P, e);
  const uint64_t before = rg_prev(v, i0, P, e[RG_PER - 1]);
  uint32_t hm = 0;  // bit j: vote j opens a group
  {
    uint64_t prev = before;
#pragma unroll
    for (int j = 0; j < RG_PER; ++j) {
      if (j < n && (i0 + j == 0 || (e[j] >> gshift) != (prev >> gshift))) hm |= 1u << j;
      prev = e[j];
    }
  }
  const uint32_t hc = (uint32_t)__popc(hm);
  uint32_t incl = hc;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
    if ((int)(threadIdx.x & 63) >= d) incl += o;
  }
  if (hm == 0) return;
  uint32_t slot = wbase[t >> 6] + incl - hc;
  rg_state s;
  bool owning = false;
  auto emit = [&]() {
    if (s.cur > s.best) { s.best = s.cur; s.bestd = (uint32_t)s.curd; }
    g_pack[slot] = ((uint64_t)s.best << 32) | (0xFFFFFFFFu - (uint32_t)(s.grp & smask));   // rank: count desc, then sid asc
    g_delta[slot] = s.bestd;
    g_dedup[slot] = s.dedup;
    ++slot;
  };
  {
    uint64_t prev = before;
#pragma unroll
    for (int j = 0; j < RG_PER; ++j) {
      if (j < n) {
        if ((hm >> j) & 1u) {
          if (owning) emit();
          owning = true;
          s.grp = e[j] >> gshift;
          s.curd = ~0ull;
          s.best = s.bestd = s.cur = s.dedup = 0;
          if (i0 + j == 0 || (e[j] >> qshift) != (prev >> qshift)) qstart[e[j] >> qshift] = slot;  // first group of a query
        }
        if (owning) rg_add(s, e[j], dmask);
      }
      prev = e[j];
    }
  }
  // the last group may run on past this thread's votes.  A group still open after RG_LONG_ITERS more loads (a clean
  // query puts thousands of votes on its own song) goes to m_reduce_long_kernel, a workgroup per group, instead of
  // being walked by this one thread; the list is bounded, a group that does not get a place is walked here after all.
  bool open = n == RG_PER;
  int iters = 0;
  for (uint64_t i = i0 + RG_PER; open && i < P; i += RG_PER) {
    if (++iters == RG_LONG_ITERS + 1) {
      const uint32_t idx = atomicAdd(long_cnt, 1u);
      if (idx < RG_LONG_CAP) {
        long_list[idx] = make_uint2(slot, (uint32_t)(i0 + (31 - __clz((int)hm))));   // record slot, first vote of the group
        return;
      }
    }
    uint64_t x[RG_PER];
    const int m = rg_load(v, i, P, x);
#pragma unroll
    for (int j = 0; j < RG_PER; ++j) {
      if (open && j < m) {
        if ((x[j] >> gshift) != s.grp) open = false; else rg_add(s, x[j], dmask);
      }
    }
    if (m < RG_PER) open = false;
  }
  emit();
}

// One workgroup per long group handed over by m_reduce_kernel: wave 0 finds the group's end (64-ary search, the votes
// are sorted), every thread folds a contiguous piece into (first run, last run, best run between them), thread 0 joins
// the pieces in order -- runs of one delta that cross piece borders are added up, ties keep the smaller delta.
struct rg_part {
  uint64_t hd, td;   // delta of the first / last run of the piece
  uint32_t hl, tl;   // their lengths (hl == 0: empty piece)
  uint32_t best, bestd, dedup, single;   // best run strictly between them; flag votes; single: the piece is one run
};

__global__ __launch_bounds__(256) void m_reduce_long_kernel(const uint64_t* __restrict__ v, uint64_t P, m_bits mb,
                                                            const uint32_t* __restrict__ long_cnt,
                                                            const uint2* __restrict__ long_list,
                                                            uint64_t* __restrict__ g_pack, uint32_t* __restrict__ g_delta,
                                                            uint32_t* __restrict__ g_dedup) {
  __shared__ rg_part parts[256];
  __shared__ uint64_t s_end;
  const int gshift = mb.dbits + 1;
  const uint64_t dmask = (1ull << mb.dbits) - 1, smask = (1ull << mb.sb) - 1;
  const uint32_t nl = min(*long_cnt, (uint32_t)RG_LONG_CAP);
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t L = blockIdx.x; L < nl; L += gridDim.x) {
    const uint32_t slot = long_list[L].x;
    const uint64_t h0 = long_list[L].y;
    const uint64_t grp = v[h0] >> gshift;
    if (threadIdx.x < 64) {  // last index of the group in [h0, P)
      uint64_t lo = h0, n = P - h0;
      while (n > 1) {
        const uint64_t step = (n + 63) / 64;
        const uint64_t idx = lo + lane * step;
        const bool ok = lane * step < n && (v[idx] >> gshift) == grp;   // a prefix of the lanes (lane 0 always)
        const unsigned long long b = __ballot(ok);
        const uint32_t last = 63u - (uint32_t)__clzll(b);
        n = min(step, n - last * step);
        lo += last * step;
      }
      if (lane == 0) s_end = lo + 1;
    }
    __syncthreads();
    const uint64_t end = s_end;
    const uint64_t per = (end - h0 + 255) / 256;
    const uint64_t a = min(h0 + threadIdx.x * per, end), b = min(a + per, end);
    rg_part p;
    p.hd = p.td = 0;
    p.hl = p.tl = p.best = p.bestd = p.dedup = 0;
    p.single = 1;
    uint64_t curd = ~0ull;
    uint32_t cur = 0, nruns = 0;
    for (uint64_t i = a; i < b; ++i) {
      const uint64_t val = v[i];
      const uint64_t d = (val >> 1) & dmask;
      if (d != curd) {
        if (cur) {  // a run ended inside the piece
          if (nruns == 0) { p.hd = curd; p.hl = cur; }
          else if (cur > p.best) { p.best = cur; p.bestd = (uint32_t)curd; }
          ++nruns;
        }
        curd = d;
        cur = 0;
      }
      ++cur;
      p.dedup += (uint32_t)(val & 1);
    }
    if (cur) {
      if (nruns == 0) { p.hd = curd; p.hl = cur; }          // the piece is one run
      else { p.td = curd; p.tl = cur; p.single = 0; }      // last run of several
    }
    parts[threadIdx.x] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t best = 0, bestd = 0, run = 0, dedup = 0;
      uint64_t rd = ~0ull;
      for (int k = 0; k < 256; ++k) {
        const rg_part& q = parts[k];
        if (q.hl == 0) continue;
        dedup += q.dedup;
        if (q.hd == rd) run += q.hl;
        else {
          if (run > best) { best = run; bestd = (uint32_t)rd; }
          rd = q.hd;
          run = q.hl;
        }
        if (!q.single) {
          if (run > best) { best = run; bestd = (uint32_t)rd; }
          if (q.best > best) { best = q.best; bestd = q.bestd; }
          rd = q.td;
          run = q.tl;
        }
      }
      if (run > best) { best = run; bestd = (uint32_t)rd; }
      g_pack[slot] = ((uint64_t)best << 32) | (0xFFFFFFFFu - (uint32_t)(grp & smask));
      g_delta[slot] = bestd;
      g_dedup[slot] = dedup;
    }
    __syncthreads();
  }
}

// group records [r0, r1) of query q: qstart[] holds the first record of every query that has any (0xFFFFFFFF = none)
__device__ __forceinline__ void m_query_groups(const uint32_t* __restrict__ qstart, uint32_t nq,
                                               const unsigned long long* __restrict__ G, uint32_t q, uint32_t& r0,
                                               uint32_t& r1) {
  r0 = qstart[q];
  if (r0 == 0xFFFFFFFFu) { r0 = r1 = 0; return; }
  r1 = (uint32_t)*G;
  for (uint32_t k = q + 1; k < nq; ++k) {
    const uint32_t x = qstart[k];
    if (x != 0xFFFFFFFFu) { r1 = x; break; }
  }
}

// qstart[0..nq) = "no group yet", the counter of long groups behind it = 0
__global__ void m_tail_init_kernel(uint32_t* __restrict__ qstart, uint32_t nq) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nq) qstart[i] = 0xFFFFFFFFu;
  else if (i == nq) qstart[nq] = 0u;
}

// one workgroup per query: top-n groups by (count desc, sid asc) over the packed group summaries
__global__ __launch_bounds__(256) void m_topn_kernel(const uint32_t* __restrict__ qstart,
                                                     const unsigned long long* __restrict__ G, m_bits mb,
                                                     const uint64_t* __restrict__ g_pack,
                                                     const uint32_t* __restrict__ g_delta,
                                                     const uint32_t* __restrict__ g_dedup, uint32_t nq, uint32_t topn,
                                                     uint32_t* __restrict__ out_sid, int32_t* __restrict__ out_delta,
                                                     uint32_t* __restrict__ out_aligned, uint32_t* __restrict__ out_dedup,
                                                     uint32_t* __restrict__ out_nres) {
  __shared__ uint64_t s_best[4];
  __shared__ uint32_t s_r[4];
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t r0, r1;
  m_query_groups(qstart, nq, G, q, r0, r1);
  uint64_t prev = ~0ull;  // packed rank of the previous winner; candidates must rank strictly below it
  uint32_t found = 0;
  for (uint32_t n = 0; n < topn; ++n) {
    uint64_t best = 0;
    uint32_t bestr = 0xFFFFFFFFu;
    for (uint32_t r = r0 + threadIdx.x; r < r1; r += 256) {
      const uint64_t packed = g_pack[r];
      if (packed < prev && packed > best) { best = packed; bestr = r; }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      const uint64_t ob = (uint64_t)__shfl_xor((long long)best, d, 64);
      const uint32_t orr = (uint32_t)__shfl_xor((int)bestr, d, 64);
      if (ob > best) { best = ob; bestr = orr; }
    }
    if (lane == 0) { s_best[wave] = best; s_r[wave] = bestr; }
    __syncthreads();
    best = s_best[0]; bestr = s_r[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (s_best[w] > best) { best = s_best[w]; bestr = s_r[w]; }
    __syncthreads();
    if (best == 0) break;  // uniform
    if (threadIdx.x == 0) {
      const uint64_t o = (uint64_t)q * topn + n;
      out_sid[o] = 0xFFFFFFFFu - (uint32_t)best;
      out_aligned[o] = (uint32_t)(best >> 32);
      out_delta[o] = (int32_t)((int64_t)g_delta[bestr] - (int64_t)mb.bias);
      out_dedup[o] = g_dedup[bestr];
    }
    prev = best;
    ++found;
  }
  if (threadIdx.x == 0) out_nres[q] = found;
}

// Two-level form of m_topn_kernel for queries with millions of (query, song) groups (a 1M-song table yields ~9M per
// 10 s query, and only a few dozen queries fit one vote pass): with one workgroup per query the scan of g_pack ran on
// a few dozen workgroups.  Level 1: workgroup (c, q) finds the top-n of slice c of query q's groups; level 2: one
// workgroup per query ranks the C x topn candidates.  g_pack is unique per group, so "strictly below the previous
// winner" selects the same groups as the single-level kernel.
__device__ __forceinline__ void topn_block_max(uint64_t& best, uint32_t& bestr, uint64_t* s_best, uint32_t* s_r) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const uint64_t ob = (uint64_t)__shfl_xor((long long)best, d, 64);
    const uint32_t orr = (uint32_t)__shfl_xor((int)bestr, d, 64);
    if (ob > best) { best = ob; bestr = orr; }
  }
  if (lane == 0) { s_best[wave] = best; s_r[wave] = bestr; }
  __syncthreads();
  best = s_best[0]; bestr = s_r[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (s_best[w] > best) { best = s_best[w]; bestr = s_r[w]; }
  __syncthreads();
}

__global__ __launch_bounds__(256) void m_topn_partial_kernel(const uint32_t* __restrict__ qstart,
                                                             const unsigned long long* __restrict__ G, uint32_t nq,
                                                             const uint64_t* __restrict__ g_pack, uint32_t topn, uint64_t* __restrict__ part_pack,
                                                             uint32_t* __restrict__ part_r) {
  __shared__ uint64_t s_best[4];
  __shared__ uint32_t s_r[4];
  const uint32_t q = blockIdx.y, c = blockIdx.x, C = gridDim.x;
  uint32_t r0, r1;
  m_query_groups(qstart, nq, G, q, r0, r1);
  const uint32_t S = (r1 - r0 + C - 1) / C;
  const uint32_t a = r0 + (uint32_t)min((uint64_t)c * S, (uint64_t)(r1 - r0));
  const uint32_t b = (uint32_t)min((uint64_t)a + S, (uint64_t)r1);
  uint64_t prev = ~0ull;
  const uint64_t o = ((uint64_t)q * C + c) * topn;
  for (uint32_t n = 0; n < topn; ++n) {
    uint64_t best = 0;
    uint32_t bestr = 0xFFFFFFFFu;
    if (prev) {
      for (uint32_t r = a + threadIdx.x; r < b; r += 256) {
        const uint64_t packed = g_pack[r];
        if (packed < prev && packed > best) { best = packed; bestr = r; }
      }
    }
    topn_block_max(best, bestr, s_best, s_r);
    if (threadIdx.x == 0) { part_pack[o + n] = best; part_r[o + n] = bestr; }
    prev = best;  // 0 once the slice is exhausted: the remaining slots are written as 0
  }
}

__global__ __launch_bounds__(256) void m_topn_final_kernel(const uint64_t* __restrict__ part_pack,
                                                           const uint32_t* __restrict__ part_r, uint32_t ncand, m_bits mb,
                                                           const uint32_t* __restrict__ g_delta,
                                                           const uint32_t* __restrict__ g_dedup, uint32_t nq, uint32_t topn,
                                                           uint32_t* __restrict__ out_sid, int32_t* __restrict__ out_delta,
                                                           uint32_t* __restrict__ out_aligned, uint32_t* __restrict__ out_dedup,
                                                           uint32_t* __restrict__ out_nres) {
  __shared__ uint64_t s_best[4];
  __shared__ uint32_t s_r[4];
  const uint32_t q = blockIdx.x;
  if (q >= nq) return;
  const uint64_t* pp = part_pack + (uint64_t)q * ncand;
  const uint32_t* pr = part_r + (uint64_t)q * ncand;
  uint64_t prev = ~0ull;
  uint32_t found = 0;
  for (uint32_t n = 0; n < topn; ++n) {
    uint64_t best = 0;
    uint32_t bestr = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < ncand; i += 256) {
      const uint64_t packed = pp[i];
      if (packed < prev && packed > best) { best = packed; bestr = pr[i]; }
    }
    topn_block_max(best, bestr, s_best, s_r);
    if (best == 0) break;  // uniform
    if (threadIdx.x == 0) {
      const uint64_t o = (uint64_t)q * topn + n;
      out_sid[o] = 0xFFFFFFFFu - (uint32_t)best;
      out_aligned[o] = (uint32_t)(best >> 32);
      out_delta[o] = (int32_t)((int64_t)g_delta[bestr] - (int64_t)mb.bias);
      out_dedup[o] = g_dedup[bestr];
    }
    prev = best;
    ++found;
  }
  if (threadIdx.x == 0) out_nres[q] = found;
}

// ---- tolerant fold of the sorted votes (shz_set_vote_tolerance): a song's count is the sum over tol + 1 neighbouring
// offset bins.  The votes are sorted by (query, sid, delta, flag), so a RUN -- the votes of one (query, sid, delta) -- is a
// range of indices and a window of bins a range of runs: its sum is an index difference.
//   mt_flag_kernel    per vote: run heads (scanned into run indices; R runs)
//   mt_runs_kernel    per vote: first vote of every run, which runs open a (query, sid) group (scanned into record slots;
//                     G groups), flag votes of every run
//   mt_groups_kernel  per run:  the records of the groups start empty; first record of every query
//   mt_window_kernel  per run:  the window that starts at the run -- at most tol + 1 runs of its own group ahead, no bin
//                     beyond delta + tol or the delta field -- into its group's record: atomicMax of (sum << 32 | ~run), so
//                     the first window in run order wins among equal sums; the flag votes are added up beside it.  A wave
//                     joins the runs of one group before it goes to memory: a group of any size, spread over any number
//                     of workgroups, costs its waves one atomic each.
//   mt_record_kernel  per group: the winning window once more for its strongest bin (the first of equal ones: the smaller
//                     delta), the record in the form m_reduce_kernel writes: g_pack = sum << 32 | ~sid, g_delta, g_dedup.
// With tol = 0 a window is one run: the record is m_reduce_kernel's.  rfirst has R + 1 entries (rfirst[R] = P); counts
// that the host does not know (R, G) are read on the device, the launches are sized by their bound P.
__global__ void mt_flag_kernel(const uint64_t* __restrict__ v, uint64_t P, uint32_t* __restrict__ fl, uint32_t* __restrict__ gfl,
                               uint32_t* __restrict__ rdd) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P) return;
  fl[i] = (i == 0 || (v[i] >> 1) != (v[i - 1] >> 1)) ? 1u : 0u;
  gfl[i] = 0u;   // (per run, and R <= P: the scan over P entries ends in G)
  rdd[i] = 0u;
}

__global__ __launch_bounds__(256) void mt_runs_kernel(const uint64_t* __restrict__ v, uint64_t P, int gshift,
                                                      const uint32_t* __restrict__ fl, const uint32_t* __restrict__ ps,
                                                      const unsigned long long* __restrict__ R_dev, uint32_t* __restrict__ rfirst,
                                                      uint32_t* __restrict__ gfl, uint32_t* __restrict__ rdd) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = i < P;
  const uint64_t x = in ? v[i] : 0ull;
  const bool head = in && fl[i] != 0u;
  const uint32_t r = in ? (head ? ps[i] : ps[i] - 1u) : 0u;   // (vote 0 is a head: ps[i] >= 1 for every other vote)
  if (head) {
    rfirst[r] = (uint32_t)i;
    gfl[r] = (i == 0 || (x >> gshift) != (v[i - 1] >> gshift)) ? 1u : 0u;
  }
  if (i == 0) rfirst[*R_dev] = (uint32_t)P;
  // flag votes per run: the wave's lanes of one run are adjacent; the first of them adds their number up
  const unsigned long long bits = __ballot(in && (x & 1ull)), heads = __ballot(head);
  const uint32_t lane = threadIdx.x & 63u;
  if (in && (head || lane == 0)) {
    const unsigned long long above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t span = above ? (uint32_t)__ffsll((long long)above) : 64u - lane;   // lanes [lane, lane + span)
    const unsigned long long mask = (span == 64u ? ~0ull : (1ull << span) - 1ull) << lane;
    const uint32_t c = (uint32_t)__popcll(bits & mask);
    if (c) atomicAdd(&rdd[r], c);
  }
}

__global__ void mt_groups_kernel(const uint64_t* __restrict__ v, const unsigned long long* __restrict__ R_dev, uint64_t bound,
                                 int qshift, const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ gfl,
                                 const uint32_t* __restrict__ gps, uint64_t* __restrict__ g_pack, uint32_t* __restrict__ g_dedup,
                                 uint32_t* __restrict__ qstart) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= bound || r >= *R_dev || !gfl[r]) return;
  const uint32_t slot = gps[r], i = rfirst[r];
  g_pack[slot] = 0ull;
  g_dedup[slot] = 0u;
  if (i == 0 || (v[i] >> qshift) != (v[i - 1] >> qshift)) qstart[v[i] >> qshift] = slot;   // first group of a query
}

// the window that starts at run r: sum of its votes; count and (biased) delta of its strongest bin
__device__ __forceinline__ void mt_window(const uint64_t* __restrict__ v, const uint32_t* __restrict__ rfirst, uint64_t R,
                                          uint64_t r, const m_bits& mb, uint32_t tol, uint32_t& sum, uint32_t& bestd) {
  const int gshift = mb.dbits + 1;
  const uint64_t dmask = (1ull << mb.dbits) - 1;
  const uint32_t i0 = rfirst[r];
  const uint64_t x0 = v[i0], grp = x0 >> gshift, d0 = (x0 >> 1) & dmask;
  const uint64_t dend = min(d0 + tol, dmask);          // the window ends inside the delta field ...
  const uint64_t kmax = min(r + tol + 1ull, R);        // ... and after tol + 1 runs at the most
  uint32_t nxt = rfirst[r + 1];
  uint32_t best = nxt - i0;
  bestd = (uint32_t)d0;
  uint64_t k = r + 1;
  for (; k < kmax; ++k) {
    const uint64_t x = v[nxt];                         // first vote of run k
    const uint64_t d = (x >> 1) & dmask;
    if ((x >> gshift) != grp || d > dend) break;       // ... and inside its (query, song) group
    const uint32_t after = rfirst[k + 1], len = after - nxt;
    if (len > best) { best = len; bestd = (uint32_t)d; }
    nxt = after;
  }
  sum = nxt - i0;
}

__global__ __launch_bounds__(256) void mt_window_kernel(const uint64_t* __restrict__ v,
                                                        const unsigned long long* __restrict__ R_dev, m_bits mb, uint32_t tol,
                                                        const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ gfl,
                                                        const uint32_t* __restrict__ gps, const uint32_t* __restrict__ rdd,
                                                        unsigned long long* __restrict__ g_pack, uint32_t* __restrict__ g_dedup) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x, R = *R_dev;
  const bool in = r < R;
  uint32_t slot = 0xFFFFFFFFu, dd = 0;   // (slots number below P < 2^32 - 1)
  unsigned long long best = 0;
  if (in) {
    uint32_t sum, bd;
    mt_window(v, rfirst, R, r, mb, tol, sum, bd);
    slot = gps[r] + gfl[r] - 1u;
    best = ((unsigned long long)sum << 32) | (0xFFFFFFFFu - (uint32_t)r);
    dd = rdd[r];
  }
  // the lanes of one group are adjacent: each ends up with what the lanes of its group from itself upwards hold
  const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long ob = (unsigned long long)__shfl_down((long long)best, d, 64);
    const uint32_t od = (uint32_t)__shfl_down((int)dd, d, 64), os = (uint32_t)__shfl_down((int)slot, d, 64);
    if (lane + d < 64u && os == slot) { best = max(best, ob); dd += od; }
  }
  const uint32_t below = (uint32_t)__shfl_up((int)slot, 1, 64);
  if (in && (lane == 0 || below != slot)) {
    atomicMax(&g_pack[slot], best);
    if (dd) atomicAdd(&g_dedup[slot], dd);
  }
}

__global__ void mt_record_kernel(const uint64_t* __restrict__ v, const unsigned long long* __restrict__ R_dev, uint64_t bound,
                                 m_bits mb, uint32_t tol, const uint32_t* __restrict__ rfirst, const uint32_t* __restrict__ gfl,
                                 const uint32_t* __restrict__ gps, uint64_t* __restrict__ g_pack, uint32_t* __restrict__ g_delta) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, R = *R_dev;
  if (r >= bound || r >= R || !gfl[r]) return;
  const uint32_t slot = gps[r];
  const uint64_t w = g_pack[slot];
  uint32_t sum, bd;
  mt_window(v, rfirst, R, 0xFFFFFFFFu - (uint32_t)w, mb, tol, sum, bd);   // (sum == w >> 32)
  const uint64_t sid = (v[rfirst[r]] >> (mb.dbits + 1)) & ((1ull << mb.sb) - 1);
  g_pack[slot] = ((uint64_t)sum << 32) | (0xFFFFFFFFu - (uint32_t)sid);   // rank: count desc, then sid asc
  g_delta[slot] = bd;
}

// ---- the vote floor (shz_set_vote_floor): per query, how many single bins and how many songs reached which count -- the
// evidence the top-n throws away.  A count c >= 1 falls into one of FH_BUCKETS buckets: c - 1 up to 16 (exact counts), then
// by powers of two, floor(log2 c) + 12 (17..31 -> 16, 32..63 -> 17, ...), everything from 2^19 up into the last one.  The
// kernel and shz_vote_bucket share the function.
#define FH_BUCKETS 32
#define FH_ROW (2 * FH_BUCKETS)   // the row of a query: song_hist[FH_BUCKETS] | bin_hist[FH_BUCKETS]
#define FH_LDS_Q 32               // queries of a workgroup's span that its LDS table holds (SHZ_DEBUG_FLOOR_SMALL: 2)
#define FH_SMALL_Q 3              // queries of a match sub-batch under SHZ_DEBUG_FLOOR_SMALL
__host__ __device__ __forceinline__ uint32_t vote_bucket(uint32_t c) {   // c >= 1
  if (c <= 16u) return c - 1u;
  const uint32_t b = (31u - (uint32_t)__builtin_clz(c)) + 12u;
  return b < (uint32_t)FH_BUCKETS - 1u ? b : (uint32_t)FH_BUCKETS - 1u;
}

// Both histogram stages run behind the tolerant fold's records, over its RUNS (rfirst, R: a run is the votes of one (query,
// song, delta), its length a difference of two first indices -- no thread walks a run of 40,000 votes):
//   fh_hist_kernel<false>  every run: the bucket of its length            -> bin_hist  (single bins, whatever the tolerance)
//   fh_hist_kernel<true>   every run that opens a (query, song) group: the bucket of the group's record, the count the
//                          fold reports as `aligned` for that song        -> song_hist
// The votes are sorted by query, so the 256 runs of a workgroup span a contiguous range of queries that starts at the query
// of its first run: the first lq <= FH_LDS_Q queries of the span are counted in an LDS table and flushed with one global add
// per non-zero cell, the queries behind them (a span that does not fit) go to global memory one add a run.  Integer adds:
// exact, and independent of the order.  hist: the rows of the pass's first query (zeroed by the caller).
template <bool SONGS>
__global__ __launch_bounds__(256) void fh_hist_kernel(const uint64_t* __restrict__ v, const unsigned long long* __restrict__ R_dev,
                                                      int qshift, const uint32_t* __restrict__ rfirst,
                                                      const uint32_t* __restrict__ gfl, const uint32_t* __restrict__ gps,
                                                      const uint64_t* __restrict__ g_pack, uint32_t lq, uint32_t nq,
                                                      uint32_t* __restrict__ hist) {
  __shared__ uint32_t tab[FH_LDS_Q * FH_BUCKETS];
  const uint64_t R = *R_dev, r0 = (uint64_t)blockIdx.x * 256;
  if (r0 >= R) return;   // uniform
  const uint32_t col = SONGS ? 0u : (uint32_t)FH_BUCKETS;
  for (uint32_t i = threadIdx.x; i < lq * FH_BUCKETS; i += 256) tab[i] = 0u;
  const uint32_t q0 = qshift < 64 ? (uint32_t)(v[rfirst[r0]] >> qshift) : 0u;
  __syncthreads();
  const uint64_t r = r0 + threadIdx.x;
  if (r < R && (!SONGS || gfl[r] != 0u)) {
    const uint32_t i = rfirst[r];
    const uint32_t q = qshift < 64 ? (uint32_t)(v[i] >> qshift) : 0u;
    const uint32_t c = SONGS ? (uint32_t)(g_pack[gps[r]] >> 32) : rfirst[r + 1] - i;
    if (c != 0u && q < nq) {   // (always: a run has a vote, a vote's query is one of the pass)
      const uint32_t b = vote_bucket(c);
      if (q - q0 < lq) atomicAdd(&tab[(q - q0) * FH_BUCKETS + b], 1u);
      else atomicAdd(&hist[(uint64_t)q * FH_ROW + col + b], 1u);
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < lq * FH_BUCKETS; i += 256) {
    const uint32_t n = tab[i];
    if (n) atomicAdd(&hist[(uint64_t)(q0 + i / FH_BUCKETS) * FH_ROW + col + (i % FH_BUCKETS)], n);
  }
}


// ---------------------------------------------------------------------------------------------------------------
// Vote tiles: the fold of 4-byte votes without sorting them all the way.
// A record (best count of one delta, smallest delta reaching it, rows matched) is a function of the MULTISET of a
// (query, song) group's votes, and the top-n of a query is a function of its records, so the full order the radix
// sort produced (four passes + run lengths + scans + dense records) is not needed.  Two radix passes order the votes
// by their upper 16 bits only (query | upper song-id bits); the array is then cut into tiles of ~VT_TILE votes at
// places where those bits change, never inside a (query, song) group and never across queries; one workgroup per
// tile counts (song, delta) in an LDS hash table, reduces that to one entry per song in a second table (atomicMax of
// count << 32 | ~delta, atomicAdd of the flags) and picks the tile's top-n; a last kernel ranks the tiles' candidates
// of every query.  g_pack (count << 32 | ~sid) is the rank of align_matches as in m_reduce_kernel: count descending,
// song id ascending, and the delta of a record is the smallest one reaching the count (recognizer.py:305-322 as
// restated in oracle/cpu_ref.py: vote / align_matches).
#define VT_THREADS 1024
#define VT_SLOTS 8192          // per LDS table (4 arrays of 4 bytes x VT_SLOTS = 128 KB)
#define VT_TILE 2048           // votes per tile before the cut is moved to the next group border
#define VT_LIMIT 6144          // distinct keys a table may hold: VT_TILE + 2^12 deltas of one song always fit one sweep
#define VT_MAXQ SHZ_SEG_MAX     // queries per vote pass (their votes stay apart as segments of the sort: shz_sort_u32_seg)
#define VT_MAXTOPN 8
#define VT_MAX_DBITS 12
#define VT_MAX_DSPLIT 8        // delta bits above those a sweep may split by (vt_fold_kernel): tracks of up to 2^20 frames
#define VT_EMPTY 0xFFFFFFFFu
#define VT_ORDERED_BITS 16     // upper bits of a vote the radix passes order (two passes of 8)
#define VT_ONE_WG_MAX 32768     // votes of a single query that one workgroup folds without any radix pass

struct vt_plan {
  uint32_t nq;                 // queries of the pass
  uint32_t qv[VT_MAXQ + 1];    // first vote of every query in the ordered pass (prefix sums of the per-query counts)
  uint32_t tb[VT_MAXQ + 1];    // first tile of every query; tb[nq] = number of tiles
  int g_lo;                    // lowest bit the radix passes ordered: tiles are cut where bits >= g_lo change
  int dbits, sb;               // layout of a vote: flag | delta (dbits) | song id (sb) | query
  uint32_t tile;               // nominal votes per tile
  uint32_t flush;              // votes a batch of vt_stream2_kernel holds before it may end at a group border
};

__device__ __forceinline__ uint32_t vt_query_of_tile(const vt_plan& pl, uint32_t g) {
  uint32_t i = 0, hi = pl.nq;                        // last query with tb[i] <= g (queries without votes have no tiles)
  while (hi - i > 1) {
    const uint32_t mid = (i + hi) >> 1;
    if (pl.tb[mid] <= g) i = mid; else hi = mid;
  }
  return i;
}

// tile_start[g], g = 0 .. ntiles: the first tile of a query starts at the query's first vote, the others at the first
// group border at or behind their nominal start.  One WAVE per tile: the border is a few dozen votes away as a rule (a
// group is 2^slb songs), so the wave looks at the next 63 votes at once, then at three more rows, and only a group longer
// than that is searched by halving (the votes are ordered by the bits >= g_lo) -- one or two dependent loads instead of the
// ~23 of a binary search over the whole query, which was 10 us of a single query's 300.
__global__ __launch_bounds__(256) void vt_bounds_kernel(const uint32_t* __restrict__ k, vt_plan pl, uint32_t* __restrict__ tile_start,
                                                        uint32_t* __restrict__ n_heavy, unsigned long long* __restrict__ qbar) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, nt = pl.tb[pl.nq];
  if (qbar && t <= VT_MAXQ) qbar[t] = 0ull;          // the queries' bars start at nothing (vt_stream2_kernel)
  const uint32_t g = t >> 6, lane = t & 63u;
  if (g > nt) return;
  if (g == nt) { if (lane == 0) { tile_start[g] = pl.qv[pl.nq]; *n_heavy = 0; } return; }
  const uint32_t i = vt_query_of_tile(pl, g), l = g - pl.tb[i];
  const uint32_t a = pl.qv[i], b = pl.qv[i + 1];
  if (l == 0) { if (lane == 0) tile_start[g] = a; return; }
  const uint32_t p = a + l * pl.tile;   // < b: the query has ceil((b - a) / tile) tiles
  uint32_t pos = p - 1, found = b;      // lane 0 of the first row holds the vote in front of the nominal start
  uint32_t h = 0;
  bool done = false;
  for (int r = 0; r < 4 && pos < b; ++r) {           // uniform
    const uint32_t j = pos + lane;
    const uint32_t v = j < b ? k[j] >> pl.g_lo : 0u;
    if (r == 0) h = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    const unsigned long long m = __ballot(j < b && v > h);   // (lane 0 of the first row is the vote itself: not above itself)
    if (m) { found = pos + (uint32_t)__ffsll((long long)m) - 1; done = true; break; }
    pos += 64;
  }
  if (!done && pos < b) {
    uint32_t lo = pos, hi = b;          // first position in [pos, b) whose upper bits exceed h
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if ((k[mid] >> pl.g_lo) > h) hi = mid; else lo = mid + 1;
    }
    found = lo;
  }
  if (lane == 0) tile_start[g] = found;
}

#define VT_SLOTS2 4096         // table 2 (one entry per song)
#define VT_LIMIT2 3000         // songs a sweep may hold: VT_LIMIT2 + one row of new ones stays below VT_SLOTS2
static_assert(VT_SLOTS == 1 << 13 && VT_SLOTS2 == 1 << 12, "vt_hash<13> / vt_hash<12>");
static_assert(VT_LIMIT + VT_THREADS < VT_SLOTS && VT_LIMIT2 + VT_THREADS < VT_SLOTS2, "a probe must find a free slot");
static_assert(VT_TILE + (1 << VT_MAX_DBITS) <= VT_LIMIT && VT_TILE < VT_LIMIT2, "the finest sweep always fits");

template <int BITS>
__device__ __forceinline__ uint32_t vt_hash(uint32_t x) { return (x * 2654435761u) >> (32 - BITS); }

// Slots of N (song | delta) keys in table 1 and of their N songs in table 2, open addressing, inserted if absent.
// All compare-and-swaps of a round are in flight together: a round costs one LDS round trip, not 2 N.
// A probe sequence is BOUNDED by `probe_limit` rounds (the table size: after that many steps every slot has been seen; a
// debug switch lowers it).  The fill limits of the callers keep a free slot within reach, so the bound is never met -- but
// if a table ever is full (a caller's limit broken, a zero-trip clear: the hang of round 2) the lanes give up, *err is
// set, the pass's results are void and the host repeats the pass through the full sort.
template <int N, int B1, int B2>
__device__ __forceinline__ void vt_slots(uint32_t* key1, uint32_t* key2, const uint32_t (&x1)[N], const uint32_t (&x2)[N],
                                         const bool (&valid)[N], uint32_t (&s1)[N], uint32_t (&s2)[N], bool (&fresh1)[N],
                                         bool (&fresh2)[N], uint32_t probe_limit, uint32_t* __restrict__ err) {
  bool p1[N], p2[N];
#pragma unroll
  for (int r = 0; r < N; ++r) {
    s1[r] = vt_hash<B1>(x1[r]);
    s2[r] = vt_hash<B2>(x2[r]);
    p1[r] = p2[r] = valid[r];
    fresh1[r] = fresh2[r] = false;
  }
  auto round = [&]() {
    uint32_t o1[N], o2[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
      o1[r] = p1[r] ? atomicCAS(&key1[s1[r]], VT_EMPTY, x1[r]) : 0u;
      o2[r] = p2[r] ? atomicCAS(&key2[s2[r]], VT_EMPTY, x2[r]) : 0u;
    }
#pragma unroll
    for (int r = 0; r < N; ++r) {
      const bool e1 = p1[r] && o1[r] == VT_EMPTY, e2 = p2[r] && o2[r] == VT_EMPTY;
      fresh1[r] = fresh1[r] || e1;
      fresh2[r] = fresh2[r] || e2;
      p1[r] = p1[r] && !e1 && o1[r] != x1[r];
      p2[r] = p2[r] && !e2 && o2[r] != x2[r];
      if (p1[r]) s1[r] = (s1[r] + 1) & ((1u << B1) - 1u);
      if (p2[r]) s2[r] = (s2[r] + 1) & ((1u << B2) - 1u);
    }
  };
  auto pending = [&]() {
    bool any = false;
#pragma unroll
    for (int r = 0; r < N; ++r) any |= p1[r] | p2[r];
    return __ballot(any) != 0ull;   // uniform
  };
  // The first rounds are straight-line code: at the fill levels the callers keep, two or three rounds settle a row, and
  // outside a loop the lanes' states (pending, fresh) stay lane masks in scalar registers -- as loop-carried values of a
  // divergent loop they were re-materialised per round (35 VALU instructions per round; round 3's fold was bound by VALU
  // issue).  Whatever is still pending goes round a wave-uniform loop.
  constexpr uint32_t STRAIGHT = 3;
  round();                                   // (probe_limit >= 1)
  if (probe_limit > 1) round();
  if (probe_limit > 2) round();
  for (uint32_t done = probe_limit < STRAIGHT ? probe_limit : STRAIGHT; pending(); ++done) {
    if (done >= probe_limit) { atomicOr(err, 1u); break; }   // (the slots of the lanes that gave up are valid indices of the wrong entries)
    round();
  }
}

// N votes of a lane: count of (song, delta) in table 1; the song's entry of table 2 keeps the largest count seen and,
// among equal counts, the smallest delta (counts only grow, so the maximum over all increments is the maximum of the
// final counts), and the number of flagged votes.  Songs entered for the first time are appended to lst (length *n2),
// one LDS atomic per wave; *n1 counts table 1's entries when `count1`.  Called by whole waves.
template <int N>
__device__ __forceinline__ void vt_votes(uint32_t* key1, uint32_t* cnt, uint32_t* key2, unsigned long long* best,
                                         uint32_t* ded, uint16_t* lst, uint32_t* n1, uint32_t* n2, bool count1,
                                         const uint32_t (&v)[N], const bool (&valid)[N], int dbits, uint32_t dmask,
                                         uint32_t probe_limit, uint32_t* __restrict__ err) {
  uint32_t x1[N], x2[N], s1[N], s2[N];
  bool f1[N], f2[N];
#pragma unroll
  for (int r = 0; r < N; ++r) { x1[r] = v[r] >> 1; x2[r] = x1[r] >> dbits; }
  vt_slots<N, 13, 12>(key1, key2, x1, x2, valid, s1, s2, f1, f2, probe_limit, err);
  uint32_t c[N];
#pragma unroll
  for (int r = 0; r < N; ++r) c[r] = valid[r] ? atomicAdd(&cnt[s1[r]], 1u) : 0u;
#pragma unroll
  for (int r = 0; r < N; ++r)
    if (valid[r]) {
      atomicMax(&best[s2[r]], ((unsigned long long)(c[r] + 1u) << 32) | (dmask - (x1[r] & dmask)));
      if (v[r] & 1u) atomicAdd(&ded[s2[r]], 1u);
    }
  const int lane = threadIdx.x & 63;
  const unsigned long long lt = (1ull << lane) - 1ull;
  unsigned long long fb[N];
  uint32_t tot = 0, tot1 = 0;
#pragma unroll
  for (int r = 0; r < N; ++r) {
    fb[r] = __ballot(f2[r]);
    tot += (uint32_t)__popcll(fb[r]);
    if (count1) tot1 += (uint32_t)__popcll(__ballot(f1[r]));
  }
  if (count1 && tot1 && lane == 0) atomicAdd(n1, tot1);
  if (tot == 0) return;   // uniform
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(n2, tot);
  base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
  for (int r = 0; r < N; ++r) {
    if (f2[r]) lst[base + (uint32_t)__popcll(fb[r] & lt)] = (uint16_t)s2[r];
    base += (uint32_t)__popcll(fb[r]);
  }
}

// maximum of v over the wave (all lanes get it): DPP inside the rows of 16 lanes, then the four row results
__device__ __forceinline__ uint32_t vt_wave_max(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1 /* quad_perm [1,0,3,2] */, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E /* quad_perm [2,3,0,1] */, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141 /* row_half_mirror */, 0xF, 0xF, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140 /* row_mirror */, 0xF, 0xF, true));
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  return max(max(r0, r1), max(r2, r3));
}


// Persistent workgroups, tile g = blockIdx.x, + gridDim.x, ...  Per tile (and per sweep of an over-full tile):
//   A  every vote: vt_votes (both tables at once)
//   C  wave 0: top-n of the listed songs (+ the candidates of earlier sweeps)
//   D  both tables cleared for the next tile
// The first VT_ROWS rows of the NEXT tile's votes are requested after A, so that they arrive during C and D.
#define VT_ROWS 3

__global__ __launch_bounds__(VT_THREADS) void vt_fold_kernel(const uint32_t* __restrict__ k,
                                                             const uint2* __restrict__ ranges,
                                                             const uint32_t* __restrict__ n_ranges, uint32_t cap, vt_plan pl,
                                                             uint32_t topn, uint64_t* __restrict__ c_pack,
                                                             uint32_t* __restrict__ c_delta, uint32_t* __restrict__ c_dedup,
                                                             uint32_t probe_limit, uint32_t* __restrict__ err) {
  __shared__ uint4 t1[VT_SLOTS / 2];                  // table 1: key1[VT_SLOTS] | cnt[VT_SLOTS]
  __shared__ uint32_t key2[VT_SLOTS2];
  __shared__ unsigned long long best[VT_SLOTS2];     // count << 32 | dmask - delta
  __shared__ uint32_t ded[VT_SLOTS2];
  __shared__ uint16_t lst[VT_SLOTS2];
  __shared__ uint64_t s_cpack[2][VT_MAXTOPN];
  __shared__ uint32_t s_cdelta[2][VT_MAXTOPN], s_cdedup[2][VT_MAXTOPN];
  __shared__ uint32_t s_n1, s_n2;
  uint32_t* const key1 = (uint32_t*)t1;
  uint32_t* const cnt = key1 + VT_SLOTS;
  const uint32_t j = threadIdx.x, lane = j & 63, nt = min(*n_ranges, cap);
  if (blockIdx.x >= nt) return;   // the usual case: nothing was handed over
  const uint32_t dmask = (1u << pl.dbits) - 1u, smask = (pl.sb >= 32 ? ~0u : (1u << pl.sb) - 1u);
  const int slb = pl.g_lo - 1 - pl.dbits;           // song-id bits below the ordered ones: what sweeps may split by
  // ... and behind them the delta bits above the low VT_MAX_DBITS: one song of a long track (> 2^12 frames) may vote for
  // more distinct deltas than table 1 holds; its delta range is then swept in parts.  The song's entry of table 2 lives
  // through all parts of its deltas (counts of one (song, delta) pair are complete inside one part, so the maximum over
  // the parts is the maximum over all deltas; ties keep the smallest delta; the flagged votes add up).
  const int dsb = pl.dbits > VT_MAX_DBITS ? pl.dbits - VT_MAX_DBITS : 0;
  auto clear1 = [&]() {
    for (uint32_t i = j; i < VT_SLOTS / 4; i += VT_THREADS) t1[i] = make_uint4(VT_EMPTY, VT_EMPTY, VT_EMPTY, VT_EMPTY);
    for (uint32_t i = VT_SLOTS / 4 + j; i < VT_SLOTS / 2; i += VT_THREADS) t1[i] = make_uint4(0, 0, 0, 0);
  };
  clear1();
  for (uint32_t i = j; i < VT_SLOTS2; i += VT_THREADS) { key2[i] = VT_EMPTY; best[i] = 0; ded[i] = 0; }
  if (j == 0) { s_n1 = 0; s_n2 = 0; }
  uint32_t g = blockIdx.x;
  uint32_t a = 0, b = 0, pre[VT_ROWS];
  if (g < nt) { a = ranges[g].x; b = ranges[g].y; }
#pragma unroll
  for (int r = 0; r < VT_ROWS; ++r) { const uint32_t i = a + r * VT_THREADS + j; pre[r] = i < b ? k[i] : 0u; }
  __syncthreads();
  for (; g < nt; g += gridDim.x) {
    const uint32_t gn = g + gridDim.x;
    uint32_t na = 0, nb = 0;                         // (both 0 behind the last tile: nothing is loaded)
    if (gn < nt) { na = ranges[gn].x; nb = ranges[gn].y; }
    const bool checked = b - a > VT_LIMIT2;         // fewer votes than either table may hold: no sweep can overflow
    int cl = 0, ns = 0, nd = 0;                      // candidate list in use; song bits / delta bits the sweeps split by
    // more votes than table 1 holds keys (a single query's unsorted votes, mostly one per (song, delta)): start with
    // the sweeps that many distinct pairs need, instead of finding out at the end of a first sweep over everything
    if (b - a > VT_LIMIT)
      while (ns < slb && ((uint32_t)VT_LIMIT << ns) < b - a) ++ns;
    bool prefetched = false;
    for (bool done = (a >= b); !done;) {             // until a sweep count is found under which every sweep fits
      bool over = false;
      uint32_t over_songs = 0;                         // songs in table 2 when a sweep overflowed
      cl = 0;
      const int nsl = ns + nd;
      for (uint32_t sw = 0; sw < (1u << nsl) && !over; ++sw) {
        const uint32_t song_part = sw >> nd, delta_part = sw & ((1u << nd) - 1u);
        const bool last_of_song = delta_part == (1u << nd) - 1u;
        // ---- A
        if (!checked && nsl == 0 && b - a <= VT_ROWS * VT_THREADS) {   // the usual tile: its rows are in registers
          bool ok[VT_ROWS];
#pragma unroll
          for (int r = 0; r < VT_ROWS; ++r) ok[r] = a + r * VT_THREADS + j < b;
          vt_votes<VT_ROWS>(key1, cnt, key2, best, ded, lst, &s_n1, &s_n2, false, pre, ok, pl.dbits, dmask, probe_limit, err);
        } else {
          for (uint32_t row = 0, base = a; base < b; base += VT_THREADS, ++row) {
            const uint32_t i = base + j;
            uint32_t v[1] = {0};
            if (row < VT_ROWS && nsl == 0) v[0] = row == 0 ? pre[0] : row == 1 ? pre[1] : pre[2];
            else if (i < b) v[0] = k[i];
            const uint32_t x = v[0] >> 1;
            const bool ok[1] = {i < b && (ns == 0 || (((x >> pl.dbits) & ((1u << slb) - 1u)) >> (slb - ns)) == song_part) &&
                                (nd == 0 || ((x & dmask) >> (pl.dbits - nd)) == delta_part)};
            vt_votes<1>(key1, cnt, key2, best, ded, lst, &s_n1, &s_n2, true, v, ok, pl.dbits, dmask, probe_limit, err);
            if (checked) {
              __syncthreads();
              over = s_n1 > VT_LIMIT || s_n2 > VT_LIMIT2;      // uniform: read between two barriers
              over_songs = s_n2;
              __syncthreads();
              if (over) break;
            }
          }
        }
        static_assert(VT_ROWS == 3, "the row select above names pre[0..2]");
        __syncthreads();
        const uint32_t n2 = s_n2;
        if (!prefetched) {               // the next tile's first rows: in flight during C and D
          prefetched = true;
#pragma unroll
          for (int r = 0; r < VT_ROWS; ++r) { const uint32_t i = na + r * VT_THREADS + j; pre[r] = i < nb ? k[i] : 0u; }
        }
        // ---- C: rank = (count descending, song id ascending); the smallest delta reaching the count is in best
        if (j < 64 && !over && last_of_song) {
          constexpr int CE = 12;                     // songs per lane whose rank stays in registers (n2 <= 768: the usual tile)
          uint64_t cpk[CE];
          const bool cached = n2 <= 64 * CE;         // uniform
          if (cached) {
            uint32_t cs[CE];
#pragma unroll
            for (int u = 0; u < CE; ++u) { const uint32_t e = lane + 64 * u; cs[u] = e < n2 ? lst[e] : 0xFFFFFFFFu; }
#pragma unroll
            for (int u = 0; u < CE; ++u)
              cpk[u] = cs[u] == 0xFFFFFFFFu ? 0ull : ((best[cs[u]] >> 32) << 32) | (0xFFFFFFFFu - (key2[cs[u]] & smask));
          }
          uint64_t prev = ~0ull;
          const uint64_t old = (song_part > 0 && lane < topn) ? s_cpack[cl][lane] : 0ull;
          for (uint32_t n = 0; n < topn; ++n) {
            uint64_t m = old < prev ? old : 0ull;
            uint32_t ms = 0xFFFFFFFFu;               // slot of m (0xFFFFFFFF: the old candidate), index of the entry if cached
            if (cached) {
#pragma unroll
              for (int u = 0; u < CE; ++u)
                if (cpk[u] < prev && cpk[u] > m) { m = cpk[u]; ms = lane + 64 * u; }
            } else {
              for (uint32_t e = lane; e < n2; e += 64) {
                const uint32_t s = lst[e];
                const uint64_t pk = ((best[s] >> 32) << 32) | (0xFFFFFFFFu - (key2[s] & smask));
                if (pk < prev && pk > m) { m = pk; ms = s; }
              }
            }
            const uint32_t cmax = vt_wave_max((uint32_t)(m >> 32));
            const uint32_t lo = vt_wave_max((uint32_t)(m >> 32) == cmax ? (uint32_t)m : 0u);
            const uint64_t w = ((uint64_t)cmax << 32) | lo;     // the wave's best below prev (0: none left)
            if (w != 0 && m == w) {                              // one lane: packs are unique
              if (cached && ms != 0xFFFFFFFFu) ms = lst[ms];
              s_cpack[cl ^ 1][n] = w;
              s_cdelta[cl ^ 1][n] = ms == 0xFFFFFFFFu ? s_cdelta[cl][lane] : dmask - ((uint32_t)best[ms] & dmask);
              s_cdedup[cl ^ 1][n] = ms == 0xFFFFFFFFu ? s_cdedup[cl][lane] : ded[ms];
            }
            if (w == 0 && lane == 0) { s_cpack[cl ^ 1][n] = 0; s_cdelta[cl ^ 1][n] = 0; s_cdedup[cl ^ 1][n] = 0; }
            prev = w;   // 0 once exhausted: nothing ranks below it
          }
        }
        __syncthreads();
        // ---- D (also what an overflowing sweep leaves behind)
        clear1();
        if (last_of_song || over) {                  // table 2 lives through the parts of a song's delta range
          for (uint32_t e = j; e < n2; e += VT_THREADS) { const uint32_t s = lst[e]; key2[s] = VT_EMPTY; best[s] = 0; ded[s] = 0; }
          if (j == 0) s_n2 = 0;
        }
        if (j == 0) s_n1 = 0;
        if (!over && last_of_song) cl ^= 1;
        __syncthreads();
      }
      if (!over) { done = true; break; }
      // at nsl == slb + dsb a sweep is 2^VT_MAX_DBITS deltas of one song of the last group + less than VT_TILE other
      // votes, which fits.  Should it not (a broken invariant), the range is given up and the pass flagged: the host
      // repeats it through the full sort.
      if (nsl >= slb + dsb) {
        if (j < VT_MAXTOPN) s_cpack[0][j] = 0;
        if (j == 0) atomicOr(err, 2u);
        cl = 0;
        done = true;
      }
      // split by song ids while many songs share the sweep; a sweep of a handful of songs that still overflows holds one
      // long track's deltas: split those (a query against a stationary 10-minute track would otherwise walk through
      // every song-id level, each a full pass over the range, before the first delta split)
      if (ns < slb && (over_songs > 8 || nd >= dsb)) ++ns;
      else if (nd < dsb) ++nd;
      else ++ns;
      __syncthreads();
    }
    if (!prefetched) {   // an empty tile, or one given up
#pragma unroll
      for (int r = 0; r < VT_ROWS; ++r) { const uint32_t i = na + r * VT_THREADS + j; pre[r] = i < nb ? k[i] : 0u; }
    }
    if (j < topn) {
      const uint64_t o = (uint64_t)g * topn + j;
      const bool any = a < b;
      c_pack[o] = any ? s_cpack[cl][j] : 0ull;
      c_delta[o] = any ? s_cdelta[cl][j] : 0u;
      c_dedup[o] = any ? s_cdedup[cl][j] : 0u;
    }
    __syncthreads();   // the candidate lists are rewritten by the next tile
    a = na;
    b = nb;
  }
}

// ---- the usual path: one WAVE per tile of ~VW_CHUNK votes, streaming through it with wave-private tables.
// No barriers, no LDS counters: a CU runs nine such waves side by side, each hiding the others' LDS round trips.
// The wave adds whole groups (votes that share the ordered bits) to its tables until VW_FLUSH votes are in, and at
// the next group border merges the songs of that batch into its running top-n (lane n holds candidate n) and clears
// the tables.  A batch whose distinct (song, delta) pairs or songs outgrow the tables -- one group with hundreds of
// pairs: copies of one recording, stationary tones -- is handed to vt_fold_kernel as the range [batch start, next
// group border): at most VW_FLUSH + 64 votes in front of its last group, so that kernel's bound holds for it too.
#define VW_B1 9
#define VW_S1 (1 << VW_B1)     // (song | delta) entries of a batch
#define VW_LIMIT1 384
#define VW_FLUSH 64
#define VW_CHUNK 2048
// songs of a batch: 2^B2 slots, B2 = 7 (2 KB, 26 waves per CU) where a batch is expected to hold few songs, else 8
#define VW_HEAVY_PER_TILE 40   // a range handed over has more than 2^7 - 68 votes: at most 34 inside the nominal tile + the one around its last group
static_assert(VW_LIMIT1 + 64 < VW_S1, "a probe must find a free slot");
static_assert(VW_FLUSH + 64 <= VT_TILE, "a range handed to vt_fold_kernel has less than VT_TILE votes before its last group");

// ---- filter first (round 4).  What decides a query's top-n are the (song, delta) pairs that many votes
// agree on; of the ~140 votes of a batch (a group of 16 songs against 1M songs: ~9 votes a song over ~1,000 deltas) nearly
// all are alone with their pair or share it with one other.  Round 3's fold (vt_stream_kernel, since removed) paid two
// compare-and-swap probe chains, a 64-bit maximum and a table scan for every one of them, and was bound by instruction
// issue (171 vector + 211 scalar instructions per row of 64 votes, both ports ~70 % busy: profiles/r03f_pmc_match.json).
// Here a batch first goes through a KEYLESS COUNTING FILTER: table 1's 4 KB as 4,096 eight-bit counters, one ds_add_rtn
// per vote on the counter its (song | delta) hashes to.  A counter is an upper bound of the count of every pair that maps to it -- never below -- so
// "no counter of the batch reached the bar" proves that no pair of the batch did: the batch is finished, with no probe
// loop, no key compare, no per-lane state (the test is one compare per row, OR-ed into a scalar mask).
// The bar is the larger of the tile's own n-th candidate and the QUERY's bar: every tile publishes its n-th candidate
// (atomicMax on a word per query), and the n-th best of any subset of a query's songs is a lower bound of the n-th best of
// all of them -- a song below it is not in the query's top-n whatever its tile's list holds.  So a tile does not climb from
// zero: after a query's first tiles the bar stands at the noise ceiling.  A batch that MAY reach it (no bar yet; a counter
// got there -- by a real pair or by pairs sharing a counter; the filter says nothing about ties, so "reached" includes
// "equalled") is read again and folded by the exact code of round 3's fold: every candidate's count, smallest delta
// and row sum come from there, so the results are the same arrays (which tile reports a song, and whether a tile reports
// songs that end below the final top-n, depends on timing; the ranking of vt_rank_kernel does not).
__device__ __forceinline__ uint64_t vt_wave_max64(uint64_t v) {
  const uint32_t h = vt_wave_max((uint32_t)(v >> 32));
  const uint32_t l = vt_wave_max((uint32_t)(v >> 32) == h ? (uint32_t)v : 0u);
  return ((uint64_t)h << 32) | l;
}
// counter of a (song | delta) key, 12 bits: the multiply is 24-bit (full rate); the bits above 24 are folded in first
#define VW_SEED_TILES 64u      // tiles at the head of a query that fold undecided batches on the spot (vt_stream2_kernel)
#define VW_FILTER_MAX 200u     // a counter that gets here sends its batch to the exact fold whatever the bar (8 bits wrap at 256)
__device__ __forceinline__ uint32_t vw_hash_filter(uint32_t x) { return (__umul24((x ^ (x >> 13)) & 0xFFFFFFu, 0x9E3779u) >> 11) & 4095u; }
static_assert(VW_S1 * 8 == 4096, "table 1 (keys + counts) is 4 KB: 4,096 eight-bit counters");

template <int VW_B2>
__global__ __launch_bounds__(64) void vt_stream2_kernel(const uint32_t* __restrict__ k, const uint32_t* __restrict__ tile_start,
                                                        vt_plan pl, uint32_t topn, uint64_t* __restrict__ c_pack,
                                                        uint32_t* __restrict__ c_delta, uint32_t* __restrict__ c_dedup,
                                                        uint32_t* __restrict__ n_heavy, uint2* __restrict__ heavy,
                                                        uint32_t* __restrict__ heavy_q, uint32_t heavy_cap,
                                                        uint32_t probe_limit, unsigned long long* __restrict__ qbar,
                                                        uint32_t* __restrict__ err, unsigned long long* __restrict__ stats) {
  constexpr int VW_S2 = 1 << VW_B2;
  constexpr uint32_t VW_LIMIT2 = VW_S2 - 68;        // + one row of new songs stays below VW_S2
  static_assert(VW_LIMIT2 + 64 < (uint32_t)VW_S2 && VW_LIMIT1 + 64 < VW_S1, "a probe must find a free slot in either table");
  uint32_t st_b = 0, st_seed = 0, st_beat = 0, st_votes_redo = 0;   // SHZ_VT_STATS
  __shared__ uint4 t1[VW_S1 / 2];                    // key1[VW_S1] | cnt[VW_S1]
  __shared__ uint4 t2[VW_S2];                        // key2[VW_S2] | ded[VW_S2] | best[VW_S2] (8 bytes each)
  uint32_t* const key1 = (uint32_t*)t1;
  uint32_t* const cnt = key1 + VW_S1;
  uint32_t* const key2 = (uint32_t*)t2;
  uint32_t* const ded = key2 + VW_S2;
  unsigned long long* const best = (unsigned long long*)(ded + VW_S2);
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t a = tile_start[g], b = tile_start[g + 1];
  const uint32_t dmask = (1u << pl.dbits) - 1u, smask = (pl.sb >= 32 ? ~0u : (1u << pl.sb) - 1u);
  uint64_t cp = 0;                                   // lane n < topn: candidate n of this tile
  uint32_t cdl = 0, cdd = 0;
  auto clear1 = [&]() {                              // table 1
#pragma unroll
    for (int i = 0; i < VW_S1 / 4 / 64; ++i) t1[lane + 64 * i] = make_uint4(VT_EMPTY, VT_EMPTY, VT_EMPTY, VT_EMPTY);
#pragma unroll
    for (int i = 0; i < VW_S1 / 4 / 64; ++i) t1[VW_S1 / 4 + lane + 64 * i] = make_uint4(0, 0, 0, 0);
  };
  auto clear2 = [&]() {
#pragma unroll
    for (int i = 0; i < (VW_S2 + 63) / 64; ++i) {     // key2 (VW_S2 / 4 vectors of EMPTY), then ded and best (zero)
      const uint32_t e = lane + 64 * i;
      if (e < VW_S2) t2[e] = e < VW_S2 / 4 ? make_uint4(VT_EMPTY, VT_EMPTY, VT_EMPTY, VT_EMPTY) : make_uint4(0, 0, 0, 0);
    }
  };
  auto clear_filter = [&]() {                        // table 1 as the filter's counters
#pragma unroll
    for (int i = 0; i < VW_S1 / 2 / 64; ++i) t1[lane + 64 * i] = make_uint4(0, 0, 0, 0);
  };
  uint32_t* const filt = (uint32_t*)t1;
  if (a < b) {
    const uint32_t qi = vt_query_of_tile(pl, g);
    unsigned long long bar_q = qbar[qi];             // the query's bar as this tile last saw it (it only rises)
    clear_filter();
    clear2();                                        // (table 2 is left empty by whoever used it)
    uint32_t n1 = 0, n2 = 0;                         // wave-uniform (exact fold only)
    // ---------------- the exact fold of one batch [s, e): round 3's, on a range that is known
    auto insert = [&](bool act, uint32_t v) {        // whole wave
      const uint32_t x1[1] = {v >> 1}, x2[1] = {(v >> 1) >> pl.dbits};
      uint32_t s1[1], s2[1];
      bool f1[1], f2[1];
      const bool ok[1] = {act};
      vt_slots<1, VW_B1, VW_B2>(key1, key2, x1, x2, ok, s1, s2, f1, f2, probe_limit, err);
      if (act) {
        const uint32_t c = atomicAdd(&cnt[s1[0]], 1u);
        atomicMax(&best[s2[0]], ((unsigned long long)(c + 1u) << 32) | (dmask - (x1[0] & dmask)));
        if (v & 1u) atomicAdd(&ded[s2[0]], 1u);
      }
      n2 += (uint32_t)__popcll(__ballot(f2[0]));
      n1 += (uint32_t)__popcll(__ballot(f1[0]));
    };
    auto merge = [&]() {                             // the batch's songs into the running top-n
      if (n2 == 0) return;
      constexpr int CE = VW_S2 / 64;                 // every slot of table 2: CE per lane
      uint64_t pk[CE];
#pragma unroll
      for (int u = 0; u < CE; ++u) {
        const uint32_t s = lane + 64 * u, kk = key2[s];
        pk[u] = kk == VT_EMPTY ? 0ull : ((best[s] >> 32) << 32) | (0xFFFFFFFFu - (kk & smask));
      }
      uint64_t prev = ~0ull, ncp = 0;
      uint32_t ncdl = 0, ncdd = 0;
      for (uint32_t n = 0; n < topn; ++n) {
        uint64_t m = cp < prev ? cp : 0ull;          // (lanes >= topn hold 0)
        int mu = -1;                                 // entry of m, -1: the old candidate
#pragma unroll
        for (int u = 0; u < CE; ++u)
          if (pk[u] < prev && pk[u] > m) { m = pk[u]; mu = u; }
        const uint64_t w = vt_wave_max64(m);
        if (w == 0) break;                           // uniform: nothing ranks below prev
        const int win = __ffsll((long long)__ballot(m == w)) - 1;   // one lane: packs are unique
        uint32_t wdl = cdl, wdd = cdd;
        if ((int)lane == win && mu >= 0) { const uint32_t s = lane + 64 * mu; wdl = dmask - ((uint32_t)best[s] & dmask); wdd = ded[s]; }
        wdl = (uint32_t)__shfl((int)wdl, win, 64);
        wdd = (uint32_t)__shfl((int)wdd, win, 64);
        if (lane == n) { ncp = w; ncdl = wdl; ncdd = wdd; }
        prev = w;
      }
      cp = ncp; cdl = ncdl; cdd = ncdd;
    };
    auto hand_over = [&](uint32_t s, uint32_t e) {   // [s, e) to vt_fold_kernel
      if (lane == 0) {
        const uint32_t idx = atomicAdd(n_heavy, 1u);
        if (idx < heavy_cap) { heavy[idx] = make_uint2(s, e); heavy_q[idx] = qi; }
        else atomicOr(err, 4u);                      // no room in the list: the range's votes would be lost -> the pass is repeated
      }
    };
    auto nth_own = [&]() -> uint64_t {
      const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(cp >> 32), (int)topn - 1);
      const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)cp, (int)topn - 1);
      return ((uint64_t)h << 32) | l;
    };
    auto exact_batch = [&](uint32_t s, uint32_t e) { // table 2 empty on entry and on return; table 1 is handed back as the filter
      clear1();
      n1 = n2 = 0;
      bool over = false;
      for (uint32_t base = s; base < e && !over; base += 64) {
        const uint32_t i = base + lane;
        const bool act = i < e;
        insert(act, act ? k[i] : 0u);
        over = n1 > VW_LIMIT1 || n2 > VW_LIMIT2;
      }
      if (over) hand_over(s, e); else merge();
      clear_filter();
      clear2();
      // the tile's n-th candidate raises the query's bar for every tile still running; and this tile looks at the bar again
      const uint64_t mine = nth_own();
      if (mine > bar_q) {
        unsigned long long seen = 0;
        if (lane == 0) seen = atomicMax(&qbar[qi], (unsigned long long)mine);
        seen = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(seen >> 32)) << 32) |
               (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)seen);
        bar_q = seen > mine ? seen : mine;
      }
    };
    // ---------------- the stream
    uint32_t batch_start = a, batch_votes = 0, last_hi = 0xFFFFFFFFu;   // wave-uniform
    unsigned long long hit = 0;                      // wave-uniform: lanes whose counter reached the bar in this batch
    uint32_t cm = 0;                                 // per lane: the largest counter value it saw in this batch
    uint32_t cur_hi = 0;                             // the ordered bits of the batch's first vote
    uint32_t thr = 2u;                               // a counter at or above this marks the batch (`hit`)
    uint32_t thr1 = 0u;                              // the count a pair of the batch needs to get past the bar (0: anything does)
    uint64_t own = 0;                                // the tile's n-th candidate (0: the list is not full)
    const int slb = pl.g_lo - 1 - pl.dbits;          // bits of a song id below the ordered ones: song id >= (hi << slb)
    // the smallest count that lets a pair of a batch whose lowest possible id is first_hi << slb past `bar`
    auto thr_of = [&](uint64_t bar, uint32_t first_hi) -> uint32_t {
      uint32_t barc = (uint32_t)(bar >> 32);
      // a pair that only EQUALS the bar's count wins on the smaller song id: never, when every id of the batch (ids ascend
      // along a tile, and tile after tile) lies above the bar's song -- then a counter must EXCEED the bar's count
      const uint32_t bar_sid = 0xFFFFFFFFu - (uint32_t)bar;
      if (barc != 0u && ((uint64_t)first_hi << slb) > (uint64_t)bar_sid) ++barc;
      return barc;
    };
    auto set_thr = [&](uint32_t first_hi) {          // first_hi: the ordered bits of the batch's first vote
      cur_hi = first_hi;
      own = nth_own();
      thr1 = thr_of(own > bar_q ? own : bar_q, first_hi);
      thr = thr1 < 2u ? 2u : (thr1 > VW_FILTER_MAX ? VW_FILTER_MAX : thr1);   // (count 1 is not the filter's business: thr1 < 2 is)
    };
    auto refresh_bar = [&]() {                       // the query's bar as it stands now
      unsigned long long now = 0;
      if (lane == 0) now = __hip_atomic_load(&qbar[qi], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      now = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(now >> 32)) << 32) |
            (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)now);
      if (now > bar_q) bar_q = now;
    };
    // does a batch whose largest counter was cmax (>= 1: every vote is a pair of count 1) still need the exact fold, with
    // the tile's list and the query's bar as they are NOW?  (Exact batches of a tile run in ascending order of ids, so the
    // tile's own candidates come from lower ids than the batch's.)
    auto needed = [&](uint32_t cmax, uint32_t first_hi) -> bool {
      own = nth_own();
      return cmax >= VW_FILTER_MAX || cmax >= thr_of(own > bar_q ? own : bar_q, first_hi);
    };
    // DEFERRED batches.  All tiles of a query start together with no bar at all, and a bar worth having (count 2 at a low
    // id, which makes every later batch need count 3) only exists once a few tiles have folded a few batches exactly; a tile
    // that decided every batch on the spot paid one exact fold for its first batch (no bar) and more for the counter
    // collisions of the next ones (count-1 bar) -- 60 % of the time of a single query's fold (measured with the bar left
    // over from the previous call: 0.345 -> 0.283 ms a query at 1M songs).  So only the query's first VW_SEED_TILES tiles
    // (the lowest ids: their bars are the ones that bind everybody else) decide on the spot; the others note an undecided
    // batch -- its range, first ordered bits and largest counter, in the registers of lane i for note i -- and decide
    // when the tile's stream has ended (or 64 notes are there), in order, against the bar of that moment.
    // (a sixteenth of the query's tiles, between 4 and VW_SEED_TILES: 100k songs, ~110 tiles a query: 9.95 us a query with 64
    // seeds -- nearly every tile folding on the spot --, 9.25 with 8; 1M songs, 1,100-4,400 tiles: 4 / 16 / 64 within 2 %)
    const uint32_t q_tiles = pl.tb[qi + 1] - pl.tb[qi];
    const uint32_t n_seed = min(max(q_tiles >> 4, 4u), VW_SEED_TILES);
    const bool seed_tile = g - pl.tb[qi] < n_seed;
    uint32_t npend = 0;                              // wave-uniform
    uint32_t pd_s = 0, pd_e = 0, pd_hi = 0, pd_c = 0;   // lane i: note i
    auto run_pending = [&]() {
      if (npend == 0) return;
      refresh_bar();
      for (uint32_t i = 0; i < npend; ++i) {         // uniform
        const uint32_t ps = (uint32_t)__builtin_amdgcn_readlane((int)pd_s, (int)i), pe = (uint32_t)__builtin_amdgcn_readlane((int)pd_e, (int)i);
        const uint32_t ph = (uint32_t)__builtin_amdgcn_readlane((int)pd_hi, (int)i), pc = (uint32_t)__builtin_amdgcn_readlane((int)pd_c, (int)i);
        if (needed(pc, ph)) { ++st_beat; st_votes_redo += pe - ps; exact_batch(ps, pe); }   // (which looks at the bar again)
      }
      npend = 0;
    };
    // ONE place ends a batch (the row loop below) and ONE place folds exactly (run_pending): the exact fold is a long piece
    // of code -- probe loops, the top-n merge -- and the seven inlined copies it had made a 16,000-instruction kernel.
    auto end_batch = [&](uint32_t e, uint32_t next_hi, bool last) {   // next_hi: the ordered bits of the vote at e (the next batch's first)
      ++st_b;
      bool noted = false;
      if (hit != 0ull || thr1 < 2u) {                // a counter reached the batch's threshold, or songs of count 1 may still enter
        const uint32_t w = vt_wave_max(cm), cmax = w < 1u ? 1u : w;
        ++st_seed;
        if (lane == npend) { pd_s = batch_start; pd_e = e; pd_hi = cur_hi; pd_c = cmax; }
        ++npend;
        noted = true;
      }
      clear_filter();
      // decide now: a seed tile's note (on the spot), 64 notes, the end of the tile.  Otherwise a tile that keeps noting batches
      // has a stale bar (none, if it started with its query): it looks again now and then -- with a bar worth having, notes
      // become rare and so do these loads
      if (npend != 0u && (seed_tile || npend == 64u || last)) run_pending();
      else if (noted && (npend & 7u) == 0u) refresh_bar();
      set_thr(next_hi);
      hit = 0ull;
      cm = 0;
      batch_start = e;
      batch_votes = 0;
    };
    // one row's votes of the lanes `act` through the filter: +1 on the counter of (song | delta); lanes outside add nothing
    auto fast_insert = [&](bool act, uint32_t v) {
      const uint32_t h = vw_hash_filter(v >> 1), sh = (h & 3u) << 3;
      const uint32_t old = atomicAdd(&filt[h >> 2], act ? 1u << sh : 0u);
      const uint32_t c = act ? ((old >> sh) & 0xFFu) + 1u : 0u;
      cm = c > cm ? c : cm;
      hit |= __ballot(c >= thr);
    };
    // the same in two halves: a whole row's update is ISSUED, and its counter values are looked at one row later -- after
    // the next row's update has been issued -- so that an LDS round trip is always in flight beside the next row's work
    uint32_t p_old = 0, p_sh = 0;
    bool p_any = false;                              // wave-uniform: a row's values are still to be looked at
    auto consume = [&]() {
      if (!p_any) return;
      const uint32_t c = ((p_old >> p_sh) & 0xFFu) + 1u;   // (only whole rows are deferred: every lane took part)
      cm = c > cm ? c : cm;
      hit |= __ballot(c >= thr);
      p_any = false;
    };
    // the next VW_AHEAD rows of votes: loads in flight.  The wave waits for memory, not for issue slots (SQ counters: 90 % of
    // its cycles) -- 26 waves a CU with 4 rows each in flight are 6.8 MB on the whole chip, what ~3 us of loaded latency
    // turn into ~2 TB/s at best
    constexpr int VW_AHEAD = 8;
    uint32_t rr[VW_AHEAD];
#pragma unroll
    for (int j = 0; j < VW_AHEAD; ++j) { const uint32_t i = a + lane + 64u * j; rr[j] = i < b ? k[i] : 0u; }
    for (uint32_t base = a;; base += 64) {
      // behind the last vote comes a pseudo-row with a border at lane 0: it ends the last batch where every batch ends
      const bool tail = base >= b;
      uint32_t v = 0, hi = 0;
      unsigned long long mg = 1ull;
      bool valid = false;
      if (!tail) {
        v = rr[0];
#pragma unroll
        for (int j = 0; j + 1 < VW_AHEAD; ++j) rr[j] = rr[j + 1];
        { const uint32_t i = base + 64u * VW_AHEAD + lane; rr[VW_AHEAD - 1] = i < b ? k[i] : 0u; }
        valid = base + lane < b;
        hi = v >> pl.g_lo;
        const uint32_t hp = (uint32_t)__builtin_amdgcn_update_dpp((int)last_hi, (int)hi, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
        mg = __ballot(valid && hi != hp);                            // lanes that open a group
        last_hi = (uint32_t)__builtin_amdgcn_readlane((int)hi, 63);  // (the last row is the only partial one)
        if (base == a) set_thr((uint32_t)__builtin_amdgcn_readfirstlane((int)hi));
        if (mg == 0ull || batch_votes < pl.flush) {                  // no border in the row, or none that may end the batch (it is
          // still below its flush size when the row begins: the whole row joins it, as in round 3's fold): one piece
          if (base + 64u <= b) {                                     // a whole row: issued now, looked at with the next row
            const uint32_t h = vw_hash_filter(v >> 1), sh = (h & 3u) << 3;
            const uint32_t old = atomicAdd(&filt[h >> 2], 1u << sh);
            consume();
            p_old = old; p_sh = sh; p_any = true;
            batch_votes += 64u;
          } else {
            consume();
            fast_insert(valid, v);
            batch_votes += b - base;
          }
          continue;
        }
      }
      consume();
      uint32_t lo = 0;                               // first lane of the row not dealt with yet
      while (lo < 64) {                              // uniform
        const unsigned long long rest = mg & ~((1ull << lo) - 1ull);
        uint32_t cut = 64;                           // the batch may end at the next group border once it is large enough
        if ((batch_votes >= pl.flush || tail) && rest) cut = (uint32_t)__ffsll((long long)rest) - 1;
        if (cut == lo) {
          end_batch(tail ? b : base + lo, tail ? 0xFFFFFFFFu : (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)lo), tail);
          if (tail) break;
          continue;
        }
        const bool act = valid && lane >= lo && lane < cut;
        fast_insert(act, v);
        batch_votes += (uint32_t)__popcll(__ballot(act));
        lo = cut;                                    // (a border at `cut` ends the batch at the top of this loop)
      }
      if (tail) break;
    }
    if (stats && lane == 0) {
      atomicAdd(stats + 0, (unsigned long long)st_b);
      atomicAdd(stats + 2, (unsigned long long)st_seed); atomicAdd(stats + 3, (unsigned long long)st_beat);
      atomicAdd(stats + 6, (unsigned long long)st_votes_redo); atomicAdd(stats + 7, (unsigned long long)(b - a));
    }
  }
  if (lane < topn) {
    const uint64_t o = (uint64_t)g * topn + lane;
    c_pack[o] = cp;
    c_delta[o] = cdl;
    c_dedup[o] = cdd;
  }
}

// one query whose votes one workgroup can fold as they come out of the expand (no radix pass at all): the whole pass is
// the one range handed to vt_fold_kernel
__global__ void vt_one_range_kernel(uint32_t* __restrict__ n_heavy, uint2* __restrict__ heavy, uint32_t* __restrict__ heavy_q,
                                    uint32_t n_votes) {
  *n_heavy = 1u;
  heavy[0] = make_uint2(0u, n_votes);
  heavy_q[0] = 0u;
}

// one workgroup per query of the pass: top-n of its tiles' candidates
#define VR_THREADS 1024
#define VR_CACHE 12            // candidates a thread keeps in registers: 12,288 per query before it re-reads them

__global__ __launch_bounds__(VR_THREADS) void vt_rank_kernel(vt_plan pl, uint32_t topn, m_bits mb, const uint64_t* __restrict__ c_pack,
                                                             const uint32_t* __restrict__ c_delta,
                                                             const uint32_t* __restrict__ c_dedup,
                                                             const uint32_t* __restrict__ n_heavy,
                                                             const uint32_t* __restrict__ heavy_q, uint32_t heavy_cap,
                                                             uint32_t* __restrict__ out_sid,
                                                             int32_t* __restrict__ out_delta, uint32_t* __restrict__ out_aligned,
                                                             uint32_t* __restrict__ out_dedup, uint32_t* __restrict__ out_nres) {
  __shared__ uint64_t s_best[2][VR_THREADS / 64];
  const uint32_t q = blockIdx.x, j = threadIdx.x;
  const uint32_t c0 = pl.tb[q] * topn, nc = (pl.tb[q + 1] - pl.tb[q]) * topn;
  const uint32_t nt = pl.tb[pl.nq], nh = min(*n_heavy, heavy_cap) * topn;   // candidates of range r: slots (nt + r) * topn ...
  const bool cached = nc <= VR_CACHE * VR_THREADS;   // uniform
  uint64_t ck[VR_CACHE];
  if (cached) {
#pragma unroll
    for (int u = 0; u < VR_CACHE; ++u) { const uint32_t i = j + u * VR_THREADS; ck[u] = i < nc ? c_pack[c0 + i] : 0ull; }
  }
  uint64_t prev = ~0ull;
  uint32_t found = 0;
  for (uint32_t n = 0; n < topn; ++n) {
    uint64_t best = 0;
    uint32_t bestr = 0xFFFFFFFFu;
    if (cached) {
#pragma unroll
      for (int u = 0; u < VR_CACHE; ++u)
        if (ck[u] < prev && ck[u] > best) { best = ck[u]; bestr = c0 + j + u * VR_THREADS; }
    } else {
      for (uint32_t i = j; i < nc; i += VR_THREADS) {
        const uint64_t packed = c_pack[c0 + i];
        if (packed < prev && packed > best) { best = packed; bestr = c0 + i; }
      }
    }
    for (uint32_t i = j; i < nh; i += VR_THREADS) {    // (usually none)
      if (heavy_q[i / topn] != q) continue;
      const uint64_t packed = c_pack[(uint64_t)nt * topn + i];
      if (packed < prev && packed > best) { best = packed; bestr = nt * topn + i; }
    }
    // the block's best: count first, then the low word, inside the waves; the 16 wave results through LDS
    const uint32_t cmax = vt_wave_max((uint32_t)(best >> 32));
    const uint32_t lo = vt_wave_max((uint32_t)(best >> 32) == cmax ? (uint32_t)best : 0u);
    if ((j & 63) == 0) s_best[n & 1][j >> 6] = ((uint64_t)cmax << 32) | lo;
    __syncthreads();
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < VR_THREADS / 64; ++i) w = s_best[n & 1][i] > w ? s_best[n & 1][i] : w;
    if (w == 0) break;  // uniform
    if (best == w) {    // one thread: packs are unique
      const uint64_t o = (uint64_t)q * topn + n;
      out_sid[o] = 0xFFFFFFFFu - (uint32_t)w;
      out_aligned[o] = (uint32_t)(w >> 32);
      out_delta[o] = (int32_t)((int64_t)c_delta[bestr] - (int64_t)mb.bias);
      out_dedup[o] = c_dedup[bestr];
    }
    prev = w;
    ++found;
  }
  if (j == 0) out_nres[q] = found;
}

// shz_match_pairs: the packed votes themselves leave match_core (device buffer of `cap` entries), in a key layout
// the caller chose for ALL shards: ((q << sb | sid) << dbits | delta + bias) << 1 | first-offset flag, q global
struct pair_sink {
  uint64_t* d_pairs;
  uint64_t cap, count;
  m_bits lay;
  uint32_t shard, nshards;  // nshards > 1: only the query hashes this shard owns are looked up
};

// ---- switches: each is read once per process (the tests run every mode in a child process of its own)
static int env_int(const char* name, int unset) {
  const char* e = getenv(name);
  return e ? atoi(e) : unset;
}
struct vote_switches {
  int tiles;    // SHZ_VOTE_TILES: 0 never (neither the vote tiles nor the one-workgroup fold)
  int vote32;   // SHZ_VOTE32: 0 never, 1 whenever it fits
};
static const vote_switches& vote_env() { static const vote_switches sw{env_int("SHZ_VOTE_TILES", -1), env_int("SHZ_VOTE32", -1)}; return sw; }
static bool vt_stats_env() { static const bool on = env_int("SHZ_VT_STATS", 0) != 0; return on; }
static bool trace_match_env() { static const bool on = env_int("SHZ_TRACE_MATCH", 0) != 0; return on; }
// rounds a probe of an LDS table of `slots` entries may take (debug: it gives up after one)
static uint32_t vt_probe_limit(const shz_ctx* ctx, uint32_t slots) { return (ctx->debug & SHZ_DEBUG_VT_PROBE1) ? 1u : slots; }

// ---- the results and per-query counters of a sub-batch live in ONE block, on the device (zeroed by the probe) and in
// the host copy of it:  npairs[nq] u64 | sid, delta, aligned, dedup [nres = nq * topn] u32 each | nres[nq] | nhash[nq] |
// vt_err (and a pad word).  Callers with arrays of their own (shz_pairs_vote) fill the same views by hand.
struct res_block {
  uint64_t* npairs;
  uint32_t* sid;
  int32_t* delta;
  uint32_t *aligned, *dedup, *nres, *nhash;
  uint32_t* vt_err;   // set by a vote-tile kernel whose LDS table or range list overflowed: the votes go through the full sort again
  uint32_t* hist = nullptr;   // the vote floor's rows [nq][FH_ROW] behind the block (shz_set_vote_floor), NULL while it is off
};
static uint64_t res_block_bytes(uint32_t nq, uint64_t nres) { return (uint64_t)nq * 8 + nres * 16 + (uint64_t)nq * 8 + 8; }
static res_block res_block_at(void* base, uint32_t nq, uint64_t nres) {
  uint32_t* w = (uint32_t*)((uint64_t*)base + nq);
  return res_block{(uint64_t*)base, w, (int32_t*)(w + nres), w + 2 * nres, w + 3 * nres, w + 4 * nres, w + 4 * nres + nq,
                   w + 4 * nres + 2 * (uint64_t)nq};
}
// the rows of query qa and those behind it (what a vote pass over [qa, qb) writes)
static res_block res_rows(res_block r, uint32_t qa, uint32_t topn) {
  const uint64_t o = (uint64_t)qa * topn;
  r.sid += o; r.delta += o; r.aligned += o; r.dedup += o;
  r.nres += qa;
  if (r.hist) r.hist += (uint64_t)qa * FH_ROW;
  return r;
}

// the records of a vote pass -> top-n per query, into the device rows r
static int32_t vote_rank(shz_ctx* ctx, uint64_t P, uint32_t nq, m_bits mb, uint32_t topn, const uint32_t* qstart,
                         const unsigned long long* d_G, const uint64_t* gh, const uint32_t* gd, const uint32_t* gdd,
                         const res_block& r) {
  // groups per query decide the shape: one workgroup per query, or C slices per query and a final ranking.  The bound
  // votes / queries stands in for groups / queries (more slices than needed cost a few idle workgroups).
  const uint32_t C = (uint32_t)std::min<uint64_t>(512, (P / nq + 16383) / 16384);
  if (C <= 1) {
    hipLaunchKernelGGL(m_topn_kernel, dim3(nq), dim3(256), 0, ctx->stream, qstart, d_G, mb, gh, gd, gdd, nq, topn, r.sid, r.delta,
                       r.aligned, r.dedup, r.nres);
  } else {
    void *pp, *pr;
    const uint64_t ncand = (uint64_t)C * topn;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M8, (uint64_t)nq * ncand * 8, &pp));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M9, (uint64_t)nq * ncand * 4, &pr));
    hipLaunchKernelGGL(m_topn_partial_kernel, dim3(C, nq), dim3(256), 0, ctx->stream, qstart, d_G, nq, gh, topn, (uint64_t*)pp,
                       (uint32_t*)pr);
    hipLaunchKernelGGL(m_topn_final_kernel, dim3(nq), dim3(256), 0, ctx->stream, (const uint64_t*)pp, (const uint32_t*)pr,
                       (uint32_t)ncand, mb, gd, gdd, nq, topn, r.sid, r.delta, r.aligned, r.dedup, r.nres);
  }
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// sorted votes -> one record per (query, song) group -> top-n per query, into the device rows r (zeroed by the caller)
static int32_t vote_fold(shz_ctx* ctx, const uint64_t* vs, uint64_t P, uint32_t nq, m_bits mb, uint32_t topn, uint64_t* d_tot,
                         const res_block& r) {
  // group heads per wave -> first record slot of every wave -> one record per (query, sid) group
  const uint32_t nb = nblk((P + RG_PER - 1) / RG_PER), nw = nb * 4;
  void *wc, *gh, *gd, *gdd;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M1, ((uint64_t)nw * 2 + nq + 2) * 4 + (uint64_t)RG_LONG_CAP * 8, &wc));
  uint32_t *wcnt = (uint32_t*)wc, *wbase = wcnt + nw, *qstart = wbase + nw;
  uint32_t* long_cnt = qstart + nq;
  uint2* long_list = (uint2*)(long_cnt + 1 + ((nw * 2 + nq + 1) & 1));   // 8-byte aligned behind the counter
  hipLaunchKernelGGL(m_gcount_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, P, mb.dbits + 1, wcnt);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, wcnt, wbase, nw, d_tot));   // *d_tot = G, the number of (query, song) groups: stays on the device
  hipLaunchKernelGGL(m_tail_init_kernel, dim3(nblk((uint64_t)nq + 1)), dim3(256), 0, ctx->stream, qstart, nq);   // qstart = none, long_cnt = 0
  // G <= P, and a group needs a vote per song: the record arrays are sized by that bound instead of a read-back of G
  const uint64_t Gb = P;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M2, Gb * 8, &gh));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M5, Gb * 4, &gd));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M6, Gb * 4, &gdd));
  const unsigned long long* d_G = (const unsigned long long*)d_tot;
  hipLaunchKernelGGL(m_reduce_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, P, mb, (const uint32_t*)wbase, (uint64_t*)gh,
                     (uint32_t*)gd, (uint32_t*)gdd, qstart, long_cnt, long_list);
  hipLaunchKernelGGL(m_reduce_long_kernel, dim3(std::min<uint32_t>(1024, nb)), dim3(256), 0, ctx->stream, vs, P, mb,
                     (const uint32_t*)long_cnt, (const uint2*)long_list, (uint64_t*)gh, (uint32_t*)gd, (uint32_t*)gdd);
  return vote_rank(ctx, P, nq, mb, topn, qstart, d_G, (const uint64_t*)gh, (const uint32_t*)gd, (const uint32_t*)gdd, r);
}

// ... with a tolerance (shz_set_vote_tolerance): the mt_* kernels in place of m_reduce_kernel / m_reduce_long_kernel, the same
// records, the same ranking.  d_tot[0] = G as in vote_fold; d_tot[1] = R, the number of runs (both stay on the device).
static int32_t vote_fold_tol(shz_ctx* ctx, const uint64_t* vs, uint64_t P, uint32_t nq, m_bits mb, uint32_t topn, uint32_t tol,
                             uint64_t* d_tot, const res_block& r) {
  void *a, *b, *gh, *gd, *gdd;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M1, (P * 3 + 1 + nq + 2) * 4, &a));   // fl | ps | rfirst (R + 1 <= P + 1) | qstart
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M3, P * 3 * 4, &b));                  // gfl | gps | rdd (per run)
  uint32_t *fl = (uint32_t*)a, *ps = fl + P, *rfirst = ps + P, *qstart = rfirst + P + 1;
  uint32_t *gfl = (uint32_t*)b, *gps = gfl + P, *rdd = gps + P;
  const unsigned long long *d_G = (const unsigned long long*)d_tot, *d_R = d_G + 1;
  const int gshift = mb.dbits + 1, qshift = mb.sb + mb.dbits + 1;
  const uint32_t nb = nblk(P);
  hipLaunchKernelGGL(mt_flag_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, P, fl, gfl, rdd);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, fl, ps, P, d_tot + 1));
  hipLaunchKernelGGL(mt_runs_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, P, gshift, (const uint32_t*)fl, (const uint32_t*)ps,
                     d_R, rfirst, gfl, rdd);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, gfl, gps, P, d_tot));
  hipLaunchKernelGGL(m_tail_init_kernel, dim3(nblk((uint64_t)nq + 1)), dim3(256), 0, ctx->stream, qstart, nq);
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M2, P * 8, &gh));   // G <= P records, as in vote_fold
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M5, P * 4, &gd));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M6, P * 4, &gdd));
  hipLaunchKernelGGL(mt_groups_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, d_R, P, qshift, (const uint32_t*)rfirst,
                     (const uint32_t*)gfl, (const uint32_t*)gps, (uint64_t*)gh, (uint32_t*)gdd, qstart);
  hipLaunchKernelGGL(mt_window_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, d_R, mb, tol, (const uint32_t*)rfirst,
                     (const uint32_t*)gfl, (const uint32_t*)gps, (const uint32_t*)rdd, (unsigned long long*)gh, (uint32_t*)gdd);
  hipLaunchKernelGGL(mt_record_kernel, dim3(nb), dim3(256), 0, ctx->stream, vs, d_R, P, mb, tol, (const uint32_t*)rfirst,
                     (const uint32_t*)gfl, (const uint32_t*)gps, (uint64_t*)gh, (uint32_t*)gd);
  if (r.hist) {   // the vote floor: the runs' lengths and the groups' records, before the ranking throws them away
    const uint32_t lq = (ctx->debug & SHZ_DEBUG_FLOOR_SMALL) ? 2u : (uint32_t)FH_LDS_Q;
    hipLaunchKernelGGL(fh_hist_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, vs, d_R, qshift, (const uint32_t*)rfirst,
                       (const uint32_t*)gfl, (const uint32_t*)gps, (const uint64_t*)gh, lq, nq, r.hist);
    hipLaunchKernelGGL(fh_hist_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, vs, d_R, qshift, (const uint32_t*)rfirst,
                       (const uint32_t*)gfl, (const uint32_t*)gps, (const uint64_t*)gh, lq, nq, r.hist);
  }
  SHZ_HIP(ctx, hipGetLastError());
  return vote_rank(ctx, P, nq, mb, topn, qstart, d_G, (const uint64_t*)gh, (const uint32_t*)gd, (const uint32_t*)gdd, r);
}

// ---- the song filter (shz_set_song_filter): between the expand and the sort of the one 8-byte pass, the votes of the songs
// outside their query's set are dropped by a stable compaction -- kept votes of every block (fs_count_kernel), their scan,
// the kept votes in order (fs_write_kernel).  A block holds FS_BLOCK votes, a wave a quarter of them in FS_ROUNDS rounds of
// 64 lanes x 2 votes (one 16-byte load a lane); ranks inside a round come from two 64-bit ballots, the waves' bases from LDS.
// A vote costs its 8 bytes read twice and one bitmap word (L2: 128 KB a set at 1M songs), a kept vote 8 bytes written.
#define FS_BLOCK 2048u
#define FS_SMALL_BLOCK 64u   // SHZ_DEBUG_FILTER_SMALL
#define FS_SMALL_Q 3u        // queries of a match sub-batch under SHZ_DEBUG_FILTER_SMALL
#define FS_ROUNDS 4          // = FS_BLOCK / 4 waves / 128 votes
struct fs_view {
  const uint64_t* v;         // the P expanded votes, query-major (16-byte aligned)
  uint64_t P;
  const uint32_t* bm;        // [n_sets][words] bitmaps
  const uint32_t* set_of;    // the set of every query of the sub-batch, NULL: set 0
  uint32_t words, exclude, nq, bv;   // bv: votes of a block
  int sshift, qshift;        // dbits + 1; sb + dbits + 1
  uint64_t smask;            // mask(sb)
};
// does the vote stay?  *q = its query (a query index the layout cannot hold keeps nothing and counts nowhere)
__device__ __forceinline__ bool fs_keep(const fs_view& F, uint64_t v, uint32_t* q) {
  const uint32_t qq = (uint32_t)(v >> F.qshift);
  *q = qq;
  if (qq >= F.nq) return false;
  const uint32_t sid = (uint32_t)((v >> F.sshift) & F.smask), w = sid >> 5;
  uint32_t bit = 0;   // an id beyond the bitmap is not listed
  if (w < F.words) bit = (F.bm[(uint64_t)(F.set_of ? F.set_of[qq] : 0u) * F.words + w] >> (sid & 31)) & 1u;
  return bit != F.exclude;
}
// round r of a wave: lane l holds the votes i, i + 1 with i = w0 + 128 r + 2 l, dead beyond `end`
__device__ __forceinline__ void fs_load(const fs_view& F, uint64_t i, uint64_t end, uint64_t* a, uint64_t* b, bool* la, bool* lb) {
  *la = i < end;
  *lb = i + 1 < end;
  *a = *b = 0;
  if (*lb) {
    const ulonglong2 x = *(const ulonglong2*)(F.v + i);
    *a = x.x;
    *b = x.y;
  } else if (*la) {
    *a = F.v[i];
  }
}
// the kept votes of a round that spans several queries: one add per query present
__device__ __forceinline__ void fs_add_runs(uint32_t q, bool keep, uint32_t lane, unsigned long long* __restrict__ npairs) {
  uint64_t todo = __ballot(keep);
  while (todo) {
    const int l = __ffsll((unsigned long long)todo) - 1;
    const uint32_t qq = (uint32_t)__shfl((int)q, l, 64);
    const uint64_t m = __ballot(keep && q == qq);
    if ((int)lane == l) atomicAdd(npairs + qq, (unsigned long long)__popcll(m));
    todo &= ~m;
  }
}
__global__ __launch_bounds__(256) void fs_count_kernel(fs_view F, uint32_t* __restrict__ blk_cnt,
                                                       unsigned long long* __restrict__ npairs /*zeroed*/) {
  __shared__ uint32_t s_w[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wc = F.bv >> 2;
  const uint64_t w0 = (uint64_t)blockIdx.x * F.bv + (uint64_t)wave * wc;
  const uint64_t end = w0 + wc < F.P ? w0 + wc : F.P;
  uint32_t c = 0, acc_q = 0, acc_n = 0;   // acc: kept votes of the run of query acc_q not yet added (uniform in the wave)
#pragma unroll
  for (int r = 0; r < FS_ROUNDS; ++r) {
    uint64_t a, b;
    bool la, lb;
    uint32_t qa = 0, qb = 0;
    fs_load(F, w0 + 128ull * r + 2ull * lane, end, &a, &b, &la, &lb);
    const bool ka = la && fs_keep(F, a, &qa), kb = lb && fs_keep(F, b, &qb);
    const uint64_t ma = __ballot(ka), mb = __ballot(kb);
    const uint32_t n = (uint32_t)(__popcll(ma) + __popcll(mb));
    if (n) {   // uniform
      const uint32_t qf = ma ? (uint32_t)__shfl((int)qa, __ffsll((unsigned long long)ma) - 1, 64)
                             : (uint32_t)__shfl((int)qb, __ffsll((unsigned long long)mb) - 1, 64);
      if ((__ballot(ka && qa != qf) | __ballot(kb && qb != qf)) == 0) {   // one query: the run goes on
        if (qf != acc_q) {
          if (lane == 0 && acc_n) atomicAdd(npairs + acc_q, (unsigned long long)acc_n);
          acc_q = qf;
          acc_n = 0;
        }
        acc_n += n;
      } else {
        if (lane == 0 && acc_n) atomicAdd(npairs + acc_q, (unsigned long long)acc_n);
        acc_n = 0;
        fs_add_runs(qa, ka, lane, npairs);
        fs_add_runs(qb, kb, lane, npairs);
      }
    }
    c += n;
  }
  if (lane == 0 && acc_n) atomicAdd(npairs + acc_q, (unsigned long long)acc_n);
  if (lane == 0) s_w[wave] = c;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ __launch_bounds__(256) void fs_write_kernel(fs_view F, const uint32_t* __restrict__ blk_pos, uint64_t* __restrict__ out) {
  __shared__ uint32_t s_w[4];
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wc = F.bv >> 2;
  const uint64_t w0 = (uint64_t)blockIdx.x * F.bv + (uint64_t)wave * wc;
  const uint64_t end = w0 + wc < F.P ? w0 + wc : F.P;
  const uint64_t below = (1ull << lane) - 1ull;
  uint64_t a[FS_ROUNDS], b[FS_ROUNDS];
  uint32_t keep = 0, c = 0;   // keep: bit 2 r = the round's first vote stays, bit 2 r + 1 = its second
#pragma unroll
  for (int r = 0; r < FS_ROUNDS; ++r) {
    bool la, lb;
    uint32_t q = 0;
    fs_load(F, w0 + 128ull * r + 2ull * lane, end, &a[r], &b[r], &la, &lb);
    const bool ka = la && fs_keep(F, a[r], &q), kb = lb && fs_keep(F, b[r], &q);
    keep |= (ka ? 1u : 0u) << (2 * r) | (kb ? 2u : 0u) << (2 * r);
    c += (uint32_t)(__popcll(__ballot(ka)) + __popcll(__ballot(kb)));
  }
  if (lane == 0) s_w[wave] = c;
  __syncthreads();
  uint64_t base = blk_pos[blockIdx.x];
  for (uint32_t w = 0; w < wave; ++w) base += s_w[w];
#pragma unroll
  for (int r = 0; r < FS_ROUNDS; ++r) {
    const bool ka = (keep >> (2 * r)) & 1u, kb = (keep >> (2 * r + 1)) & 1u;
    const uint64_t ma = __ballot(ka), mb = __ballot(kb);
    const uint64_t pos = base + (uint64_t)(__popcll(ma & below) + __popcll(mb & below));   // lane order, a before b
    if (ka && pos < F.P) out[pos] = a[r];
    if (kb && pos + (ka ? 1u : 0u) < F.P) out[pos + (ka ? 1u : 0u)] = b[r];
    base += (uint64_t)(__popcll(ma) + __popcll(mb));
  }
}

// the tolerance of this context's votes, or -1 for the plain fold of one bin (SHZ_DEBUG_VOTE_TOLERANT_ROUTE: the tolerant
// fold at 0 bins too; the vote floor: its histograms are taken from the tolerant fold's runs and records, at the tolerance
// in force -- at 0 bins that fold computes the plain fold's results; a song filter, shz_set_song_filter: the one 8-byte pass
// is where its compaction sits)
static int vote_tol_of(const shz_ctx* ctx) {
  return (ctx->vote_tol > 0 || ctx->vote_floor || ctx->filter_sets || (ctx->debug & SHZ_DEBUG_VOTE_TOLERANT_ROUTE))
             ? (int)ctx->vote_tol
             : -1;
}

// the full sort: sort the packed 8-byte votes, then vote_fold (tol < 0) or vote_fold_tol.  v0 holds the P votes, v1 is
// scratch of the same size.
static int32_t vote_tail(shz_ctx* ctx, uint64_t* v0, uint64_t* v1, uint64_t P, uint32_t nq, m_bits mb, uint32_t topn, int tol,
                         uint64_t* d_tot, const res_block& r) {
  int sel = 0;
  // bit 0 (the first-offset flag) is only counted by the fold, never compared: it stays out of the sort
  if (P <= MH_MAX) {
    hipLaunchKernelGGL(m_sort_small_kernel, dim3(1), dim3(MH_THREADS), 0, ctx->stream, (const uint64_t*)v0, v1, (uint32_t)P, 1,
                       mb.qb + mb.sb + mb.dbits + 1);
    SHZ_HIP(ctx, hipGetLastError());
    sel = 1;
  } else {
    SHZ_TRY(shz_sort_u64(ctx, v0, v1, nullptr, nullptr, 0, P, 1, mb.qb + mb.sb + mb.dbits + 1, &sel));
  }
  if (tol >= 0) return vote_fold_tol(ctx, sel ? v1 : v0, P, nq, mb, topn, (uint32_t)tol, d_tot, r);
  return vote_fold(ctx, sel ? v1 : v0, P, nq, mb, topn, d_tot, r);
}

// ---- one vote-tile pass, in two steps so that the producer of the votes may use the plan (m_expand_blocks_kernel counts the
// first radix pass by the sort's blocks)
// plan from the votes per query of the pass: vote and tile offsets per query, the bits the radix passes order
static void vt_make_plan(const uint64_t* counts, uint32_t nqp, const m_bits& mbp, vt_plan& pl, shz_seg_plan& sp) {
  const int Bt = mbp.sb + mbp.dbits + 1;   // the votes of a tile pass carry no query bits
  pl.nq = sp.nq = nqp;
  pl.dbits = mbp.dbits;
  pl.sb = mbp.sb;
  pl.g_lo = std::max(1 + mbp.dbits, Bt - VT_ORDERED_BITS);
  // votes per tile: a tile pays a fixed price (its place in the plan, the query's bar, the first loads' latency, its
  // candidates' way through vt_rank_kernel) that 2,048 votes do not amortise -- 1M songs, batches of 200: 0.147 ms a query at
  // 2,048, 0.141 at 4,096, 0.138 at 8,192, 0.136 at 16,384 -- but the chip wants ~2 rounds of tiles (256 CUs x 26 waves).
  // (Those were the fold of mid round 4; with deferred batches and batches of 128: 0.1365 at 2,048, 0.1348 at 4,096, 0.132 at
  // 8,192, 0.1348 at 16,384, 0.1418 at 32,768: the cap is 8,192.)
  uint64_t all_votes = 0;
  for (uint32_t i = 0; i < nqp; ++i) all_votes += counts[i];
  uint32_t chunk = VW_CHUNK;
  while (chunk < 8192u && all_votes / (2ull * chunk) >= 13312ull) chunk *= 2;
  // (one query of 8.9 M votes, fewer tiles than wave slots: 1,024 votes a tile 0.379 ms, 2,048: 0.354, 4,096: 0.349 -- smaller tiles
  // do not shorten the pass, every tile pays its start)
  pl.tile = chunk;
  // votes a batch holds before it may end at a group border: 64 where tiles are small (one query: more, smaller batches let
  // the bar settle sooner: 0.281 ms against 0.300 with 128), 128 in the large passes of a batch of queries (fewer batch ends
  // to pay for: 0.1365 -> 0.1339 ms a query at 1M songs; 192: the same)
  pl.flush = chunk >= 8192 ? 2 * VW_FLUSH : VW_FLUSH;
  pl.qv[0] = pl.tb[0] = sp.qv[0] = sp.bq[0] = 0;
  for (uint32_t i = 0; i < nqp; ++i) {
    const uint64_t c = counts[i];
    pl.qv[i + 1] = sp.qv[i + 1] = pl.qv[i] + (uint32_t)c;
    pl.tb[i + 1] = pl.tb[i] + (uint32_t)((c + chunk - 1) / chunk);
    sp.bq[i + 1] = sp.bq[i] + (uint32_t)((c + 4095) / 4096);   // (the sort fills in its own block size)
  }
  for (uint32_t i = nqp; i < VT_MAXQ; ++i) {
    pl.qv[i + 1] = sp.qv[i + 1] = pl.qv[nqp];
    pl.tb[i + 1] = pl.tb[nqp];
    sp.bq[i + 1] = sp.bq[nqp];
  }
}

// the pass itself: the pp votes in k32 (4 bytes each, no query bits, query by query as the plan says; k32_alt = the second
// buffer of the sort) -> two radix passes (the first one already counted: hist0) -> tiles -> per-query top-n in the rows r
// (those of the pass's first query).  *r.vt_err is set when a tile gave up (the caller repeats the votes through the full
// sort).
static int32_t vt_run_pass(shz_ctx* ctx, uint32_t* k32, uint32_t* k32_alt, uint64_t pp, const vt_plan& pl, const shz_seg_plan& sp,
                           const m_bits& mbp, uint32_t topn, bool hist0, uint32_t max_sid, const res_block& r) {
  const uint32_t nqp = pl.nq;
  const int Bt = mbp.sb + mbp.dbits + 1;
  const uint32_t nt = pl.tb[nqp], hcap = (ctx->debug & SHZ_DEBUG_VT_TINY_HEAVY) ? 1u : nt * (VW_HEAVY_PER_TILE * ((pl.tile + VW_CHUNK - 1) / VW_CHUNK));
  int sel = 0;
  SHZ_TRY(shz_sort_u32_seg(ctx, k32, k32_alt, pp, pl.g_lo, Bt, sp, &sel, hist0));
  const uint32_t* ks = sel ? k32_alt : k32;
  // tile starts | counter of handed-over ranges | the ranges | their queries; candidates of tiles, then of ranges
  void *ts, *cp, *cd, *cdd;
  const uint64_t ncand = ((uint64_t)nt + hcap) * topn;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT0, ((uint64_t)nt + 4 + (uint64_t)hcap * 3) * 4, &ts));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT1, ncand * 8, &cp));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT2, ncand * 4, &cd));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT3, ncand * 4, &cdd));
  uint32_t* tile_start = (uint32_t*)ts;
  uint32_t* n_heavy = tile_start + nt + 1;
  uint2* heavy = (uint2*)(tile_start + ((nt + 2 + 1) & ~1u));   // 8-byte aligned
  uint32_t* heavy_q = (uint32_t*)(heavy + hcap);
  void* qb;   // the bar of every query of the pass (its tiles' n-th candidates, atomicMax); zeroed by vt_bounds_kernel
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT6, 8ull * (VT_MAXQ + 1), &qb));
  unsigned long long* d_qbar = (unsigned long long*)qb;
  hipLaunchKernelGGL(vt_bounds_kernel, dim3(nblk(std::max<uint64_t>(((uint64_t)nt + 1) * 64, (uint64_t)VT_MAXQ + 1))), dim3(256), 0, ctx->stream, ks, pl, tile_start,
                     n_heavy, d_qbar);
  // songs a batch is expected to hold: the 2^slb ids of a group + the ids that fill 64 votes
  const int slb_ = pl.g_lo - 1 - mbp.dbits;
  const double per_song = std::max(1.0, (double)pp / nqp / std::max<uint32_t>(max_sid, 1u));
  const bool few_songs = (double)(1u << slb_) + (double)pl.flush / per_song <= 40.0;
  const uint32_t plim = vt_probe_limit(ctx, VW_S1);
  unsigned long long* d_stats = nullptr;
  if (vt_stats_env()) {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC3, 64, &p));
    d_stats = (unsigned long long*)p;
    SHZ_HIP(ctx, hipMemsetAsync(d_stats, 0, 64, ctx->stream));
  }
  if (few_songs)
    hipLaunchKernelGGL(vt_stream2_kernel<7>, dim3(nt), dim3(64), 0, ctx->stream, ks, (const uint32_t*)tile_start, pl, topn,
                       (uint64_t*)cp, (uint32_t*)cd, (uint32_t*)cdd, n_heavy, heavy, heavy_q, hcap, plim, d_qbar, r.vt_err, d_stats);
  else
    hipLaunchKernelGGL(vt_stream2_kernel<8>, dim3(nt), dim3(64), 0, ctx->stream, ks, (const uint32_t*)tile_start, pl, topn,
                       (uint64_t*)cp, (uint32_t*)cd, (uint32_t*)cdd, n_heavy, heavy, heavy_q, hcap, plim, d_qbar, r.vt_err, d_stats);
  if (d_stats) {
    unsigned long long h[8];
    SHZ_HIP(ctx, hipMemcpyAsync(h, d_stats, 64, hipMemcpyDeviceToHost, ctx->stream));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    fprintf(stderr, "[vt_stats] tiles %u few_songs %d batches %llu count1 %llu beat %llu votes_redone %llu votes %llu\n",
            nt, (int)few_songs, h[0], h[2], h[3], h[6], h[7]);
  }
  hipLaunchKernelGGL(vt_fold_kernel, dim3(std::min<uint32_t>(hcap, 64u)),
                     dim3(VT_THREADS), 0, ctx->stream, ks, (const uint2*)heavy, (const uint32_t*)n_heavy, hcap, pl, topn,
                     (uint64_t*)cp + (uint64_t)nt * topn, (uint32_t*)cd + (uint64_t)nt * topn,
                     (uint32_t*)cdd + (uint64_t)nt * topn, vt_probe_limit(ctx, VT_SLOTS), r.vt_err);
  hipLaunchKernelGGL(vt_rank_kernel, dim3(nqp), dim3(VR_THREADS), 0, ctx->stream, pl, topn, mbp, (const uint64_t*)cp,
                     (const uint32_t*)cd, (const uint32_t*)cdd, (const uint32_t*)n_heavy, (const uint32_t*)heavy_q, hcap,
                     r.sid, r.delta, r.aligned, r.dedup, r.nres);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// ---- ONE workgroup folds the unordered 4-byte votes of ONE query without any radix pass: vt_fold_kernel over a single
// range (no tiles), then vt_rank_kernel.  The caller expands the votes and sends the range's end to the device between
// the two steps below: from the host once the count is known (vt_one_range_kernel), or on the device before it is
// (m_spec_plan_kernel, the queued fold).
struct one_wg_fold {
  vt_plan pl;
  uint32_t* n_heavy;   // 1 range ...
  uint2* heavy;        // ... [0, end) ...
  uint32_t* heavy_q;   // ... of query 0
  uint64_t* c_pack;    // the range's candidates
  uint32_t *c_al, *c_dd;
};
// pp: the votes of the range where the host knows them (else 0: its end is heavy[0] alone)
static int32_t one_wg_prepare(shz_ctx* ctx, const m_bits& mb, uint32_t topn, uint32_t pp, one_wg_fold* w) {
  void *ts, *cp, *cd, *cdd;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT0, 64, &ts));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT1, (uint64_t)topn * 8, &cp));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT2, (uint64_t)topn * 4, &cd));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT3, (uint64_t)topn * 4, &cdd));
  w->n_heavy = (uint32_t*)ts;
  w->heavy = (uint2*)(w->n_heavy + 2);
  w->heavy_q = w->n_heavy + 4;
  w->c_pack = (uint64_t*)cp;
  w->c_al = (uint32_t*)cd;
  w->c_dd = (uint32_t*)cdd;
  vt_plan& pl = w->pl;
  pl.nq = 1;
  pl.dbits = mb.dbits;
  pl.sb = mb.sb;
  pl.g_lo = mb.sb + mb.dbits + 1;   // no bit is ordered: a sweep may split by any song-id bit
  pl.tile = VW_CHUNK;
  pl.flush = VW_FLUSH;
  for (uint32_t i = 0; i <= VT_MAXQ; ++i) { pl.qv[i] = i ? pp : 0u; pl.tb[i] = 0; }   // no tiles, one range
  return SHZ_OK;
}
static int32_t one_wg_run(shz_ctx* ctx, const one_wg_fold& w, const uint32_t* k32, const m_bits& mb, uint32_t topn,
                          const res_block& r) {
  hipLaunchKernelGGL(vt_fold_kernel, dim3(1), dim3(VT_THREADS), 0, ctx->stream, k32, (const uint2*)w.heavy,
                     (const uint32_t*)w.n_heavy, 1u, w.pl, topn, w.c_pack, w.c_al, w.c_dd, vt_probe_limit(ctx, VT_SLOTS), r.vt_err);
  hipLaunchKernelGGL(vt_rank_kernel, dim3(1), dim3(VR_THREADS), 0, ctx->stream, w.pl, topn, mb, (const uint64_t*)w.c_pack,
                     (const uint32_t*)w.c_al, (const uint32_t*)w.c_dd, (const uint32_t*)w.n_heavy, (const uint32_t*)w.heavy_q, 1u,
                     r.sid, r.delta, r.aligned, r.dedup, r.nres);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// ---- which way the votes of a sub-batch go: decided HERE, from numbers alone
enum vote_route {
  ROUTE_NONE,          // no votes: the zeroed result block is the answer
  ROUTE_QUEUED,        // ONE small host-fed query: folded by one workgroup, queued before its vote count was known
  ROUTE_SINK,          // shz_match_pairs: 8-byte votes in the caller's layout, into the caller's buffer
  ROUTE_ONE_WG,        // ONE query with few votes: expand, one workgroup folds the unordered 4-byte votes
  ROUTE_TILES_FUSED,   // 4-byte votes through the vote tiles; the expand runs by the sort's blocks and counts its first pass
  ROUTE_TILES,         // 4-byte votes through the vote tiles, expand and sort apart
  ROUTE_WIDEN,         // 4-byte votes (query bits inside), sorted and widened into the full sort's fold
  ROUTE_SORT64,        // 8-byte votes through the full sort, one pass over all queries
  ROUTE_TOLERANT,      // shz_set_vote_tolerance: the same votes and sort, then the fold over neighbouring offset bins
};
struct vote_pass { uint32_t qa, qb; uint64_t v_lo, v_hi; };   // queries [qa, qb), their votes [v_lo, v_hi) of the sub-batch
struct vote_plan {
  vote_route route = ROUTE_NONE;
  uint32_t fuse_dmask = 0;          // ROUTE_TILES_FUSED: digit mask of the sort's first pass
  std::vector<vote_pass> passes;
};
struct vote_case {
  uint32_t nq;             // queries of the sub-batch
  uint64_t P;              // its votes ...
  const uint64_t* votes;   // ... per query
  m_bits mb;
  uint32_t topn;
  bool full_sort;          // SHZ_MATCH_FULL_SORT, or the tiles gave up on these queries: once more, through the full sort
  bool sink;               // the votes leave as they are (shz_match_pairs)
  bool queued_held;        // the fold queued ahead of the count ran on the right layout
  int tol;                 // >= 0: the vote's tolerance in bins (vote_tol_of), every fold but the tolerant one is out
  vote_switches sw;
};

static const uint64_t VOTE_PASS_MAX = 1ull << 28;   // votes of one vote pass (its buffers: 2 x 4 or 8 bytes per vote)

// song id, biased delta and the flag bit of a vote in vote_bits bits (the query bits not counted)
static bool vote_fits_bits(const m_bits& mb, int vote_bits) { return mb.sb + mb.dbits + 1 <= vote_bits; }
// what the LDS folds (vt_fold_kernel: the vote tiles, the one-workgroup fold) take: a 4-byte vote, top-n and delta bits
// within their tables' reach.  vote_bits: 32 where the expand writes the votes; 31 for the gathered votes of a sharded
// match, which have always kept one bit in hand (shz_pairs_vote chooses as it did before it shared this rule).
static bool vt_layout_fits(const m_bits& mb, uint32_t topn, const vote_switches& sw, int vote_bits = 32) {
  return vote_fits_bits(mb, vote_bits) && topn <= VT_MAXTOPN && mb.dbits <= VT_MAX_DBITS + VT_MAX_DSPLIT && sw.tiles != 0;
}
// ... and of them the one-workgroup fold: a single query, unless the full sort is asked for.  (Its vote limit,
// VT_ONE_WG_MAX, is the caller's to check: the queued fold decides before the count exists.)
static bool one_wg_fits(uint32_t nq, const m_bits& mb, uint32_t topn, bool full_sort, const vote_switches& sw) {
  return nq == 1 && !full_sort && vt_layout_fits(mb, topn, sw);
}

// the next vote pass behind *vp (first call: all zero): as many queries as q_max and VOTE_PASS_MAX votes allow, one query
// at the least.  The rule of every route that votes in passes; a pass may come out without votes.  false: no query is left.
static bool next_vote_pass(const uint64_t* votes, uint32_t nq, uint32_t q_max, vote_pass* vp) {
  if (vp->qb >= nq) return false;
  vp->qa = vp->qb;
  vp->v_lo = vp->v_hi;
  do vp->v_hi += votes[vp->qb++];
  while (vp->qb < nq && vp->qb - vp->qa < q_max && vp->v_hi - vp->v_lo + votes[vp->qb] <= VOTE_PASS_MAX);
  return true;
}

static void vote_plan_make(const vote_case& c, vote_plan* plan) {
  plan->passes.clear();
  plan->fuse_dmask = 0;
  if (c.queued_held) { plan->route = ROUTE_QUEUED; return; }
  if (c.P == 0) { plan->route = ROUTE_NONE; return; }
  if (c.sink) { plan->route = ROUTE_SINK; return; }
  // a sum over neighbouring bins needs the votes in order: one 8-byte pass, whatever their number.  The vote floor goes this
  // way too, at the tolerance in force (vote_tol_of): its histograms are taken from the sorted runs and the fold's records
  if (c.tol >= 0) {
    plan->passes.push_back(vote_pass{0, c.nq, 0, c.P});
    plan->route = ROUTE_TOLERANT;
    return;
  }
  // expand -> sort -> groups -> top-n, in vote passes over ranges of queries.  4-BYTE votes when a pass's query
  // index, the song id and the biased delta fit 31 bits (1M songs x 10 s queries: 1 + 20 + 10): half the bytes
  // through expand and the sort passes, whose last pass widens to the 64-bit layout the fold reads.  Worth it only
  // while a pass still has millions of votes; else one 8-byte pass over all queries.
  const int qbits32 = 31 - c.mb.sb - c.mb.dbits;
  bool use32 = vote_fits_bits(c.mb, 32) && c.P > MH_MAX && c.sw.vote32 != 0 && !c.full_sort;
  // vote tiles (vt_fold_kernel): two radix passes + an LDS fold per tile instead of four passes + the record chain
  const bool tiles = use32 && vt_layout_fits(c.mb, c.topn, c.sw);
  if (use32) {
    const uint32_t q_max = tiles ? (uint32_t)VT_MAXQ : (1u << std::min(qbits32, 30));   // tiles: no query bits in the vote
    vote_pass vp{0, 0, 0, 0};
    while (next_vote_pass(c.votes, c.nq, q_max, &vp))
      if (vp.v_hi > vp.v_lo) plan->passes.push_back(vp);
    if (c.sw.vote32 != 1 && c.P / std::max<size_t>(plan->passes.size(), 1) < (1ull << 22)) use32 = false;   // small passes: launch-bound
  }
  if (!use32) {
    plan->passes.clear();
    plan->passes.push_back(vote_pass{0, c.nq, 0, c.P});
    // ONE query with few votes (a 5-10 s query against thousands of songs): expand, then one workgroup folds the
    // unordered votes (vt_fold_kernel over the single range [0, P)) -- 5 launches instead of the 9 of sort + fold,
    // and the launches are what such a match costs
    const bool one_wg = c.P <= VT_ONE_WG_MAX && one_wg_fits(c.nq, c.mb, c.topn, c.full_sort, c.sw);
    plan->route = one_wg ? ROUTE_ONE_WG : ROUTE_SORT64;
    return;
  }
  if (!tiles) { plan->route = ROUTE_WIDEN; return; }
  // vote tiles: where the sort's first pass takes 8 bits, the expand runs by the blocks of the segmented sort and counts
  // that pass's digits (no tile starts then: m_chunk_start_kernel per pass)
  const int Bt = c.mb.sb + c.mb.dbits + 1, g_lo = std::max(1 + c.mb.dbits, Bt - VT_ORDERED_BITS);
  plan->route = shz_seg_first_pass(g_lo, Bt, &plan->fuse_dmask) == 8 ? ROUTE_TILES_FUSED : ROUTE_TILES;
}

// ---- a match call, and what one of its sub-batches carries from stage to stage
struct match_call {
  shz_ctx* ctx;
  shz_table* t;
  const uint32_t *key32, *q_off;   // host or device (SHZ_IN_DEVICE)
  const uint64_t* query_off;       // host
  uint32_t n_queries, topn, flags;
  uint32_t* out_sid;
  int32_t* out_delta;
  uint32_t *out_aligned, *out_dedup, *out_nres, *out_nhash;
  uint64_t* out_npairs;
  pair_sink* sink;
  // the query set on the device (match_upload)
  const uint32_t *d_key, *d_qo;
  const shz_seg_dev* d_segs;
  uint32_t nseg;
  const uint64_t* d_qoff_all;   // query_off[0 .. n_queries] on the device, when it went with the packed upload
  mctl* d_ctl_packed;           // ... and a zeroed control block for the first sub-batch
  uint64_t sub_budget;          // votes of one sub-batch
  // device input handed over inside the library (shz_match_device: the fused recognise call, the listeners)
  bool has_bias_bound;          // the caller knows a bound of the query offsets without looking at them ...
  uint32_t bias_bound;          // ... every q_off <= bias_bound: the queued fold may take it for its bias
  bool pack_small;              // segment descriptors | query offsets | control block travel as one pinned copy
  // the vote floor (shz_set_vote_floor; never with a sink): the rows of the queries committed so far, FH_ROW words each, in
  // query order -- handed to the context's store when the whole call succeeded
  bool floor;
  std::vector<uint32_t> floor_rows;
  // the song filter (shz_set_song_filter; refused with a sink): on for this call, and the set of every query (host,
  // shz_match_batch_sets), NULL: set 0
  bool filter = false;
  const uint32_t* set_of = nullptr;
};
enum sub_next {
  SUB_GO,          // on to the next stage
  SUB_EMPTY,       // no hash of these queries is looked up here: their counters are zero, on to the next queries
  SUB_FEWER,       // too much for one sub-batch: the same queries' first half
  SUB_FULL_SORT,   // the LDS fold gave up (its results are void): the same queries again, through the full sort
  SUB_DONE,        // results and counters are with the caller
};
struct match_sub {
  uint32_t q0, nq;
  uint64_t m;                // hashes of the queries [q0, q0 + nq)
  bool redo, full_sort;      // second visit after SUB_FULL_SORT; ... or the caller asked for the full sort
  m_bits mb;                 // sb from the table, qb from nq; bias and dbits once the counts are back
  // head
  const uint64_t* d_qoff;
  mctl* d_ctl;
  uint64_t nx_bound;         // sub-groups (group x segment) + sentinel, from the bound groups <= m
  uint64_t* E;               // unique (query, key, offset) elements
  uint32_t *gs, *glo;        // first element of every group; first row of every sub-group
  uint64_t* po;              // votes in front of every sub-group
  void* rb;                  // the result block ...
  uint64_t nres, rb_bytes;
  res_block r;               // ... and its views
  int tol;                   // the ctx's vote tolerance for this visit (vote_tol_of)
  bool queued;               // one-workgroup fold queued ahead of the count ...
  uint32_t queued_bias;      // ... on this bias
  // counts (sub_read_counts)
  void* mail;                // control block | votes per query | result block of a queued fold
  uint64_t mu, P, nx, rows_total;
  uint64_t kept;             // the votes that were folded: P, or what the song filter left of them
  uint64_t cap_groups, cap_pairs;   // what the key cap dropped at the probe (shz_set_key_cap; P counts the pairs it left)
  uint32_t ng;
  std::vector<uint64_t> votes;   // per query
  double tr[4];              // SHZ_TRACE_MATCH: start, head queued, counts back, votes queued
};

// The query set on the device, once.  Host input of moderate size travels as ONE copy from pinned memory:
// segment descriptors | query offsets | keys | offsets | a zeroed mctl (every separate small copy costs ~20 us of latency)
static int32_t match_upload(match_call& mc) {
  shz_ctx* ctx = mc.ctx;
  // segment descriptors for the kernels (an empty table probes one empty segment)
  std::vector<shz_seg_dev> hsegs;
  for (const shz_seg& g : all_segs(mc.t)) hsegs.push_back(seg_dev_of(g));
  if (hsegs.empty()) hsegs.push_back(shz_seg_dev{nullptr, nullptr, nullptr, mc.t->bucket, 0u, 0u, 0ull});
  const uint32_t nseg = mc.nseg = (uint32_t)hsegs.size();
  const bool host_in = !(mc.flags & SHZ_IN_DEVICE);
  const uint64_t h1 = mc.query_off[mc.n_queries];
  mc.d_key = mc.key32;
  mc.d_qo = mc.q_off;
  mc.d_qoff_all = nullptr;
  mc.d_ctl_packed = nullptr;
  const uint64_t seg_bytes = (sizeof(shz_seg_dev) * (uint64_t)nseg + 255) & ~255ull;
  const uint64_t qoff_bytes = (((uint64_t)mc.n_queries + 1) * 8 + 255) & ~255ull;
  const uint64_t col_bytes = host_in ? (h1 * 4 + 255) & ~255ull : 0;   // (device input: the columns stay where they are)
  const uint64_t pk_bytes = seg_bytes + qoff_bytes + col_bytes * 2 + 256;
  void* d_segs;
  if ((host_in || mc.pack_small) && pk_bytes <= (4ull << 20)) {
    void *hm, *dm;
    SHZ_TRY(shz_mailbox(ctx, pk_bytes, &hm));
    SHZ_TRY(shz_ws_reserve(ctx, host_in ? SHZ_WS_KEY : SHZ_WS_META, pk_bytes, &dm));
    char* hp = (char*)hm;
    memcpy(hp, hsegs.data(), sizeof(shz_seg_dev) * nseg);
    memcpy(hp + seg_bytes, mc.query_off, ((uint64_t)mc.n_queries + 1) * 8);
    const uint64_t ko = seg_bytes + qoff_bytes, oo = ko + col_bytes;
    if (h1 && host_in) {
      memcpy(hp + ko, mc.key32, h1 * 4);
      memcpy(hp + oo, mc.q_off, h1 * 4);
    }
    memset(hp + pk_bytes - 256, 0, 256);
    SHZ_HIP(ctx, hipMemcpyAsync(dm, hm, pk_bytes, hipMemcpyHostToDevice, ctx->stream));
    d_segs = dm;
    mc.d_qoff_all = (const uint64_t*)((char*)dm + seg_bytes);
    if (host_in) {
      mc.d_key = (const uint32_t*)((char*)dm + ko);
      mc.d_qo = (const uint32_t*)((char*)dm + oo);
    }
    mc.d_ctl_packed = (mctl*)((char*)dm + pk_bytes - 256);
  } else {
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_META, sizeof(shz_seg_dev) * SHZ_MAX_SEGS, &d_segs));
    SHZ_HIP(ctx, shz_memcpy(ctx, d_segs, hsegs.data(), sizeof(shz_seg_dev) * nseg, hipMemcpyHostToDevice));
    if (host_in && h1 > 0) {
      void *a, *b;
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_KEY, h1 * 4, &a));
      SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_T1, h1 * 4, &b));
      SHZ_HIP(ctx, shz_memcpy(ctx, a, mc.key32, h1 * 4, hipMemcpyHostToDevice));
      SHZ_HIP(ctx, shz_memcpy(ctx, b, mc.q_off, h1 * 4, hipMemcpyHostToDevice));
      mc.d_key = (const uint32_t*)a;
      mc.d_qo = (const uint32_t*)b;
    }
  }
  mc.d_segs = (const shz_seg_dev*)d_segs;
  return SHZ_OK;
}

// queries of the next sub-batch: at most `step`, fewer where the votes or the hashes would be too many
static uint32_t sub_queries(const match_call& mc, uint32_t q0, uint32_t step) {
  const uint64_t* query_off = mc.query_off;
  uint32_t nq = std::min<uint32_t>(step, mc.n_queries - q0);
  // the vote budget: sized from what a hash yielded in the last sub-batch, so that the head (compose, sort, probe: a
  // round trip) is not run on 200 queries, then 100, then 50 to find that 25 fit
  if (mc.ctx->m_votes_per_hash > 0.0 && nq > 1) {
    const double hashes = (double)mc.sub_budget / (1.05 * mc.ctx->m_votes_per_hash);
    uint32_t lo = 1, hi = nq;   // largest count whose hashes stay under the estimate
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if ((double)(query_off[q0 + mid] - query_off[q0]) <= hashes) lo = mid; else hi = mid - 1;
    }
    nq = lo;
  }
  // shrink so the element count stays sortable
  while (nq > 1 && query_off[q0 + nq] - query_off[q0] >= (1ull << 31)) nq /= 2;
  return nq;
}

// many hashes: compose (query, key, offset) elements, sort, unique -> E (mu of them); groups = distinct (query, key) -> gs
// (ng of them) -- queued without a host round trip in between: every launch is sized by the bound m, the counts are read
// on the device (mctl)
static int32_t head_sorted(const match_call& mc, match_sub& s, void* c0, void* c1) {
  shz_ctx* ctx = mc.ctx;
  const uint64_t m = s.m;
  const uint32_t f_nsh = mc.sink ? mc.sink->nshards : 1u, f_sh = mc.sink ? mc.sink->shard : 0u;
  uint64_t* tot = (uint64_t*)s.d_ctl;   // tot[0..1] = mu, ng
  void *fl, *ps;
  hipLaunchKernelGGL(m_compose_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, mc.d_key, mc.d_qo, s.d_qoff, s.nq, m, f_nsh,
                     f_sh, (uint64_t*)c0, s.d_ctl->err);
  SHZ_HIP(ctx, hipGetLastError());
  int sel = 0;
  SHZ_TRY(shz_sort_u64(ctx, (uint64_t*)c0, (uint64_t*)c1, nullptr, nullptr, 0, m, 0,
                       QIDX_SHIFT + (f_nsh > 1 ? bits_for(s.nq) : s.mb.qb), &sel));
  const uint64_t* cs = sel ? (uint64_t*)c1 : (uint64_t*)c0;   // sorted
  uint64_t* E = s.E = sel ? (uint64_t*)c0 : (uint64_t*)c1;    // unique elements go to the other buffer
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M1, m * 4, &fl));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M2, m * 4, &ps));
  hipLaunchKernelGGL(m_head_flag_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, cs, m, 0, (uint32_t*)fl);
  SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)fl, (uint32_t*)ps, m, tot));
  hipLaunchKernelGGL(m_compact_vals_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, cs, (const uint32_t*)fl,
                     (const uint32_t*)ps, m, E);
  hipLaunchKernelGGL(m_fix_mu_kernel, dim3(1), dim3(1), 0, ctx->stream, s.d_ctl, (unsigned long long)m);
  hipLaunchKernelGGL(m_head_flag_dn_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, (const uint64_t*)E, &s.d_ctl->mu, m,
                     QKEY_SHIFT, (uint32_t*)fl);
  SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)fl, (uint32_t*)ps, m, tot + 1));
  hipLaunchKernelGGL(m_compact_idx_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, (const uint32_t*)fl, (const uint32_t*)ps,
                     &s.d_ctl->mu, m, &s.d_ctl->ng, s.gs);
  return SHZ_OK;
}

// head of a sub-batch: its query offsets and a zeroed control block; elements and groups (head_sorted, or
// m_head_small_kernel in one launch); the probe, which also zeroes the result block; the scan of the votes per sub-group
static int32_t sub_head(match_call& mc, match_sub& s, sub_next* next) {
  shz_ctx* ctx = mc.ctx;
  const uint32_t q0 = s.q0, nq = s.nq;
  const uint64_t m = s.m;
  if (mc.d_qoff_all) {
    s.d_qoff = mc.d_qoff_all + q0;
  } else {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M0, (uint64_t)(nq + 1) * 8, &p));
    SHZ_HIP(ctx, shz_memcpy(ctx, p, mc.query_off + q0, (uint64_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    s.d_qoff = (const uint64_t*)p;
  }
  if (mc.d_ctl_packed && q0 == 0) {
    s.d_ctl = mc.d_ctl_packed;          // arrived zeroed with the upload
    mc.d_ctl_packed = nullptr;          // (a retry with fewer queries, or a later sub-batch, zeroes its own)
  } else {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC0, 256, &p));
    SHZ_HIP(ctx, hipMemsetAsync(p, 0, 256, ctx->stream));
    s.d_ctl = (mctl*)p;
  }
  if (m == 0) { *next = SUB_EMPTY; return SHZ_OK; }
  s.nx_bound = m * (uint64_t)mc.nseg + 1;
  if (s.nx_bound >= (1ull << 32)) {
    if (nq > 1) { *next = SUB_FEWER; return SHZ_OK; }
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "query %u: %llu hashes x %u segments", q0, (unsigned long long)m, mc.nseg);
  }
  void *c0, *c1, *gs, *glo, *gpairs, *po;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_A, m * 8, &c0));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_B, m * 8, &c1));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M3, (m + 1) * 4, &gs));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M4, s.nx_bound * 4, &glo));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M6, s.nx_bound * 8, &gpairs));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M7, s.nx_bound * 8, &po));
  s.gs = (uint32_t*)gs;
  s.glo = (uint32_t*)glo;
  s.po = (uint64_t*)po;
  if (!(mc.sink && mc.sink->nshards > 1) && m <= MH_MAX) {
    s.E = (uint64_t*)c1;
    hipLaunchKernelGGL(m_head_small_kernel, dim3(1), dim3(MH_THREADS), 0, ctx->stream, mc.d_key, mc.d_qo, s.d_qoff, nq,
                       (uint32_t)m, QIDX_SHIFT + s.mb.qb, s.E, s.gs, s.d_ctl);
    SHZ_HIP(ctx, hipGetLastError());
  } else {
    SHZ_TRY(head_sorted(mc, s, c0, c1));
  }
  s.nres = (uint64_t)nq * (mc.sink ? 0 : mc.topn);
  // (the vote floor's rows lie behind the block: zeroed by the probe with it, read back with it)
  s.rb_bytes = res_block_bytes(nq, s.nres) + (mc.floor ? (uint64_t)nq * FH_ROW * 4 : 0);
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_PEAK_F, s.rb_bytes + 64, &s.rb));
  s.r = res_block_at(s.rb, nq, s.nres);
  if (mc.floor) s.r.hist = (uint32_t*)((char*)s.rb + res_block_bytes(nq, s.nres));
  hipLaunchKernelGGL(m_probe_kernel, dim3(nblk(s.nx_bound)), dim3(256), 0, ctx->stream, (const uint64_t*)s.E,
                     (const uint32_t*)s.gs, &s.d_ctl->ng, s.nx_bound, mc.d_segs, mc.nseg, s.glo, (uint64_t*)gpairs,
                     (unsigned long long*)s.d_ctl + 16, (uint32_t*)s.rb, (uint32_t)((s.rb_bytes + 3) / 4));
  SHZ_HIP(ctx, hipGetLastError());
  if (ctx->key_cap)   // groups <= m; the sentinel behind the last sub-group stays 0
    SHZ_TRY(shz_key_cap_apply(ctx, (uint64_t*)gpairs, (const uint32_t*)s.gs, &s.d_ctl->ng, m, mc.nseg,
                              (unsigned long long*)s.d_ctl + M_CAP_WORD));
  SHZ_TRY(shz_scan_u64(ctx, (const uint64_t*)gpairs, s.po, s.nx_bound, (uint64_t*)&s.d_ctl->P));
  return SHZ_OK;
}

// ONE small query from host memory: its votes are queued now, before their number is known (m_spec_plan_kernel puts the
// range's end where the one-workgroup fold reads it, and voids the fold where the votes exceed VT_ONE_WG_MAX), under the
// conditions of ROUTE_ONE_WG.  What differs from that route is what the host cannot know yet: the vote count (the table's
// last match stands in for it), and the bias, which it has to take from the query itself -- so host input, or device
// input whose caller hands a bound of the offsets over (match_call::bias_bound: any bias >= the largest offset is a valid
// layout, include/shz.h at shz_match_pairs).
static int32_t sub_queue_fold(const match_call& mc, match_sub& s) {
  shz_ctx* ctx = mc.ctx;
  const vote_switches& sw = vote_env();
  s.queued = false;
  s.queued_bias = 0;
  // (vote32 == 1 would send P > MH_MAX votes through a 4-byte pass instead; the layout test with the bias still 0 is the
  // least it can need: it saves the walk over the offsets)
  const bool dev_in = (mc.flags & SHZ_IN_DEVICE) != 0;
  if (mc.sink || s.tol >= 0 || (dev_in && !mc.has_bias_bound) || s.m > MH_MAX || sw.vote32 == 1 ||
      !one_wg_fits(s.nq, s.mb, mc.topn, s.full_sort, sw) ||
      (double)s.m * mc.t->votes_per_hash > 2.0 * VT_ONE_WG_MAX)   // (a table whose last query had far more votes: not worth queueing)
    return SHZ_OK;
  bool wide = false;
  if (dev_in) {
    s.queued_bias = mc.bias_bound;
    wide = mc.bias_bound >= (1u << QOFF_BITS);
  } else {
    for (uint64_t i = mc.query_off[s.q0]; i < mc.query_off[s.q0 + 1]; ++i) {
      s.queued_bias = std::max(s.queued_bias, mc.q_off[i]);
      wide |= mc.q_off[i] >= (1u << QOFF_BITS);
    }
  }
  m_bits ms = s.mb;
  ms.qb = 0;
  ms.bias = s.queued_bias;
  ms.dbits = bits_for((uint64_t)mc.t->max_off + ms.bias);
  if (wide || !one_wg_fits(s.nq, ms, mc.topn, s.full_sort, sw)) return SHZ_OK;
  s.queued = true;
  ++ctx->st_spec_queued;
  const uint64_t cap = VT_ONE_WG_MAX;
  const uint32_t cap_tiles = (uint32_t)((cap + M_EXP_TILE - 1) / M_EXP_TILE);
  void *tx, *k32;
  one_wg_fold w;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_HCNT, ((uint64_t)cap_tiles + 1) * 4, &tx));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_C, cap * 8 + 16, &k32));
  SHZ_TRY(one_wg_prepare(ctx, ms, mc.topn, 0u, &w));
  hipLaunchKernelGGL(m_spec_plan_kernel, dim3(1), dim3(64), 0, ctx->stream, (const uint64_t*)s.po, (const mctl*)s.d_ctl, mc.nseg,
                     cap, (uint32_t*)tx, w.n_heavy, w.heavy, w.heavy_q, (uint32_t*)s.rb, (uint32_t)(s.rb_bytes / 4));
  hipLaunchKernelGGL(m_expand_spec_kernel, dim3(cap_tiles), dim3(256), 0, ctx->stream, (const uint64_t*)s.E, (const uint32_t*)s.gs,
                     (const uint32_t*)tx, (const uint64_t*)s.po, (const uint32_t*)s.glo, mc.d_segs, mc.nseg, (const mctl*)s.d_ctl,
                     cap, ms, (uint32_t*)k32);
  return one_wg_run(ctx, w, (const uint32_t*)k32, ms, mc.topn, s.r);
}

// the one read-back before the votes: their number sizes the vote buffers and the sort, their number per query
// plans the vote passes (behind a queued small query: its results come along)
static int32_t sub_read_counts(const match_call& mc, match_sub& s, sub_next* next) {
  shz_ctx* ctx = mc.ctx;
  const uint32_t nq = s.nq;
  if (nq > 1) {   // one query: its counts are the totals
    hipLaunchKernelGGL(m_query_stats_kernel, dim3(nblk(nq)), dim3(256), 0, ctx->stream, (const uint64_t*)s.E, (const mctl*)s.d_ctl,
                       (const uint32_t*)s.gs, (const uint64_t*)s.po, mc.nseg, nq, s.r.nhash, s.r.npairs);
    SHZ_HIP(ctx, hipGetLastError());
  }
  SHZ_TRY(shz_mailbox(ctx, 256 + (uint64_t)nq * 8 + (s.queued ? s.rb_bytes : 0), &s.mail));
  char* mail = (char*)s.mail;
  SHZ_HIP(ctx, hipMemcpyAsync(mail, s.d_ctl, 256, hipMemcpyDeviceToHost, ctx->stream));
  if (nq > 1) SHZ_HIP(ctx, hipMemcpyAsync(mail + 256, s.r.npairs, (uint64_t)nq * 8, hipMemcpyDeviceToHost, ctx->stream));
  if (s.queued) SHZ_HIP(ctx, hipMemcpyAsync(mail + 256 + 8, s.rb, s.rb_bytes, hipMemcpyDeviceToHost, ctx->stream));
  if (trace_match_env()) s.tr[1] = now_s();
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (trace_match_env()) s.tr[2] = now_s();
  const mctl h = *(const mctl*)mail;
  if (h.err[0]) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "query offsets must be < 2^%d frames", QOFF_BITS);
  s.mu = h.mu;
  if (s.mu == 0) { *next = SUB_EMPTY; return SHZ_OK; }   // nothing of this sub-batch belongs to this shard
  s.mb.bias = h.err[1];
  s.mb.dbits = bits_for((uint64_t)mc.t->max_off + s.mb.bias);
  if (mc.sink) {  // the caller's layout must hold this table's ids and offsets and these queries' offsets
    const m_bits& L = mc.sink->lay;
    if (h.err[1] > L.bias || bits_for(mc.t->max_sid) > L.sb || bits_for((uint64_t)mc.t->max_off + L.bias) > L.dbits)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_pairs: layout (sid_bits %d, delta_bits %d, bias %u) too small for this table / these queries", L.sb, L.dbits, L.bias);
  } else if (s.mb.qb + s.mb.sb + s.mb.dbits + 1 > 64) {
    if (nq > 1) { *next = SUB_FEWER; return SHZ_OK; }
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "song id / offset range too wide for the packed vote key");
  }
  s.ng = (uint32_t)h.ng;
  s.nx = (uint64_t)s.ng * mc.nseg;   // sub-groups: (query, key) group x segment
  s.P = s.kept = h.P;
  s.rows_total = 0;
  for (int i = 0; i < M_ROW_STRIPES; ++i) s.rows_total += ((const uint64_t*)mail)[16 + i];
  s.cap_groups = s.cap_pairs = 0;
  for (int i = 0; i < M_CAP_STRIPES; ++i) {
    s.cap_groups += ((const uint64_t*)mail)[M_CAP_WORD + i];
    s.cap_pairs += ((const uint64_t*)mail)[M_CAP_WORD + M_CAP_STRIPES + i];
  }
  ctx->m_votes_per_hash = mc.t->votes_per_hash = (double)s.P / (double)s.mu;
  if (s.P > mc.sub_budget && nq > 1) { *next = SUB_FEWER; return SHZ_OK; }   // too many votes for one sub-batch
  if (s.P >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "query %u alone produces %llu matches (limit 2^32)", s.q0, (unsigned long long)s.P);
  s.votes.assign(nq, s.P);
  if (nq > 1) memcpy(s.votes.data(), mail + 256, (uint64_t)nq * 8);
  return SHZ_OK;
}

// the votes [v_lo, v_hi) of a sub-batch, packed by the layout mb with the query index + q_base on top, into `out`
// (tile_x: the sub-group of every M_EXP_TILE-th vote's first pair, from m_tile_start_kernel)
template <typename VT>
static int32_t expand_votes(const match_call& mc, const match_sub& s, const uint32_t* tile_x, uint64_t v_lo, uint64_t v_hi,
                            const m_bits& mb, int64_t q_base, VT* out) {
  const uint32_t ntiles = (uint32_t)((v_hi - v_lo + M_EXP_TILE - 1) / M_EXP_TILE);
  hipLaunchKernelGGL(m_expand_kernel<VT>, dim3(ntiles), dim3(256), 0, mc.ctx->stream, (const uint64_t*)s.E, (const uint32_t*)s.gs,
                     tile_x, (const uint64_t*)s.po, (const uint32_t*)s.glo, mc.d_segs, mc.nseg, v_lo, v_hi, mb, q_base, out);
  SHZ_HIP(mc.ctx, hipGetLastError());
  return SHZ_OK;
}

// ROUTE_SINK: hand the votes over -- expand straight into the caller's buffer, in the shared layout, with global query
// indices
static int32_t vote_to_sink(const match_call& mc, const match_sub& s) {
  pair_sink* sink = mc.sink;
  if (sink->count + s.P <= sink->cap) {
    const uint32_t ntiles = (uint32_t)((s.P + M_EXP_TILE - 1) / M_EXP_TILE);
    void* tile_x;
    SHZ_TRY(shz_ws_reserve(mc.ctx, SHZ_WS_HCNT, ((uint64_t)ntiles + 1) * 4, &tile_x));
    hipLaunchKernelGGL(m_tile_start_kernel, dim3(nblk((uint64_t)ntiles + 1)), dim3(256), 0, mc.ctx->stream, (const uint64_t*)s.po,
                       (uint32_t)s.nx, (uint64_t)0, s.P, ntiles, (uint32_t*)tile_x);
    SHZ_TRY(expand_votes<uint64_t>(mc, s, (const uint32_t*)tile_x, 0, s.P, sink->lay, (int64_t)s.q0, sink->d_pairs + sink->count));
  }
  sink->count += s.P;  // keeps counting past cap: the caller learns the size it needs
  return SHZ_OK;
}

// the vote buffers of the passes of a plan: v0 | (4-byte votes: a second buffer at v0 + pmax4 entries), v1
struct vote_bufs { void *v0, *v1; uint64_t pmax4; };

// the song filter on the pp expanded votes in v_in (the one 8-byte pass: all queries of the sub-batch, query index from 0):
// the kept votes, in order, into v_out; the kept pairs of every query into the sub-batch's npairs words; *kept = their
// total, read back -- the second small round trip of this route (the sort and the fold are sized by it)
static int32_t vote_filter(const match_call& mc, const match_sub& s, const uint64_t* v_in, uint64_t* v_out, uint64_t pp,
                           uint64_t* kept) {
  shz_ctx* ctx = mc.ctx;
  const uint32_t bv = (ctx->debug & SHZ_DEBUG_FILTER_SMALL) ? FS_SMALL_BLOCK : FS_BLOCK;
  const uint64_t nb = (pp + bv - 1) / bv;
  void *blk, *mail;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_FS_BLK, 8 + nb * 8, &blk));
  uint64_t* d_kept = (uint64_t*)blk;
  uint32_t *cnt = (uint32_t*)(d_kept + 1), *pos = cnt + nb;
  const uint32_t* d_map = nullptr;
  if (mc.set_of) {
    void* p;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_FS_MAP, (uint64_t)s.nq * 4, &p));
    SHZ_HIP(ctx, shz_memcpy(ctx, p, mc.set_of + s.q0, (uint64_t)s.nq * 4, hipMemcpyHostToDevice));
    d_map = (const uint32_t*)p;
  }
  const fs_view F{v_in, pp, ctx->d_filter, d_map, ctx->filter_words, (ctx->filter_flags & SHZ_FILTER_EXCLUDE) ? 1u : 0u, s.nq, bv,
                  s.mb.dbits + 1, s.mb.sb + s.mb.dbits + 1, (1ull << s.mb.sb) - 1ull};
  SHZ_HIP(ctx, hipMemsetAsync(s.r.npairs, 0, (uint64_t)s.nq * 8, ctx->stream));
  hipLaunchKernelGGL(fs_count_kernel, dim3((uint32_t)nb), dim3(256), 0, ctx->stream, F, cnt, (unsigned long long*)s.r.npairs);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_scan_u32(ctx, cnt, pos, nb, d_kept));
  hipLaunchKernelGGL(fs_write_kernel, dim3((uint32_t)nb), dim3(256), 0, ctx->stream, F, (const uint32_t*)pos, v_out);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_TRY(shz_mailbox(ctx, 8, &mail));
  SHZ_HIP(ctx, hipMemcpyAsync(mail, d_kept, 8, hipMemcpyDeviceToHost, ctx->stream));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  *kept = *(const uint64_t*)mail;
  if (*kept > pp) SHZ_FAIL(ctx, SHZ_E_HIP, "song filter: %llu of %llu votes kept", (unsigned long long)*kept, (unsigned long long)pp);
  return SHZ_OK;
}

// one pass of the plan: expand its votes, then sort / fold / rank as the route says, into the rows of its first query
static int32_t vote_run_pass(const match_call& mc, match_sub& s, const vote_plan& plan, const vote_pass& vp,
                             const uint32_t* tile_x, const vote_bufs& b) {
  shz_ctx* ctx = mc.ctx;
  const uint32_t topn = mc.topn, nqp = vp.qb - vp.qa;
  const uint64_t pp = vp.v_hi - vp.v_lo;
  const res_block r = res_rows(s.r, vp.qa, topn);
  uint64_t* d_G = (uint64_t*)&s.d_ctl->G;
  m_bits mbp = s.mb;
  uint32_t* k32 = (uint32_t*)b.v0;   // 4-byte votes: two buffers in SORT_C (the widened result in SORT_D)
  switch (plan.route) {
    case ROUTE_ONE_WG: {
      one_wg_fold w;
      SHZ_TRY(expand_votes<uint32_t>(mc, s, tile_x, vp.v_lo, vp.v_hi, mbp, (int64_t)0, k32));
      SHZ_TRY(one_wg_prepare(ctx, mbp, topn, (uint32_t)pp, &w));
      hipLaunchKernelGGL(vt_one_range_kernel, dim3(1), dim3(1), 0, ctx->stream, w.n_heavy, w.heavy, w.heavy_q, (uint32_t)pp);
      return one_wg_run(ctx, w, k32, mbp, topn, r);
    }
    case ROUTE_TILES_FUSED:
    case ROUTE_TILES: {
      mbp.qb = 0;   // the votes of a tile pass carry no query bits: their place in the pass says it
      vt_plan pl;
      shz_seg_plan sp;
      vt_make_plan(s.votes.data() + vp.qa, nqp, mbp, pl, sp);
      if (plan.route == ROUTE_TILES) {
        SHZ_TRY(expand_votes<uint32_t>(mc, s, tile_x, vp.v_lo, vp.v_hi, mbp, M_NO_QUERY_BITS, k32));
      } else {
        const uint32_t stile = shz_seg_tile(pp), cpb = stile / M_EXP_TILE;
        shz_seg_blocks(&sp, stile);
        const uint32_t nsb = sp.bq[nqp];
        void *cxp, *hist;
        SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT5, (uint64_t)nsb * (cpb + 1) * 4, &cxp));
        SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_H, ((uint64_t)nsb << 8) * 4, &hist));   // (the sort asks for the same)
        hipLaunchKernelGGL(m_chunk_start_kernel, dim3(nblk((uint64_t)nsb * (cpb + 1))), dim3(256), 0, ctx->stream,
                           (const uint64_t*)s.po, (uint32_t)s.nx, sp, stile, vp.v_lo, vp.v_hi, (uint32_t*)cxp);
        hipLaunchKernelGGL(m_expand_blocks_kernel, dim3(nsb), dim3(256), 0, ctx->stream, (const uint64_t*)s.E,
                           (const uint32_t*)s.gs, (const uint32_t*)cxp, (const uint64_t*)s.po, (const uint32_t*)s.glo, mc.d_segs,
                           mc.nseg, vp.v_lo, sp, stile, mbp, pl.g_lo, plan.fuse_dmask, k32, (uint32_t*)hist);
        SHZ_HIP(ctx, hipGetLastError());
      }
      return vt_run_pass(ctx, k32, k32 + b.pmax4, pp, pl, sp, mbp, topn, plan.route == ROUTE_TILES_FUSED, mc.t->max_sid, r);
    }
    case ROUTE_WIDEN:
      mbp.qb = nqp > 1 ? bits_for(nqp - 1) : 0;   // the query index inside the pass
      SHZ_TRY(expand_votes<uint32_t>(mc, s, tile_x, vp.v_lo, vp.v_hi, mbp, -(int64_t)vp.qa, k32));
      SHZ_TRY(shz_sort_u32_widen(ctx, k32, k32 + b.pmax4, (uint64_t*)b.v1, pp, 1, mbp.qb + mbp.sb + mbp.dbits + 1, 0, nullptr));
      return vote_fold(ctx, (const uint64_t*)b.v1, pp, nqp, mbp, topn, d_G, r);
    case ROUTE_SORT64:
    case ROUTE_TOLERANT:
      SHZ_TRY(expand_votes<uint64_t>(mc, s, tile_x, vp.v_lo, vp.v_hi, mbp, (int64_t)0, (uint64_t*)b.v0));
      if (mc.filter) {   // (always ROUTE_TOLERANT, vote_tol_of: the one pass over the sub-batch)
        SHZ_TRY(vote_filter(mc, s, (const uint64_t*)b.v0, (uint64_t*)b.v1, pp, &s.kept));
        if (s.kept == 0) return SHZ_OK;   // the probe zeroed the result rows, and a floor row stays zero
        return vote_tail(ctx, (uint64_t*)b.v1, (uint64_t*)b.v0, s.kept, nqp, mbp, topn, s.tol, d_G, r);
      }
      return vote_tail(ctx, (uint64_t*)b.v0, (uint64_t*)b.v1, pp, nqp, mbp, topn, plan.route == ROUTE_TOLERANT ? s.tol : -1, d_G,
                       r);
    default:
      return SHZ_OK;   // (the routes without passes)
  }
}

// the votes of a sub-batch, by the plan's route: vote buffers, the expand tiles' starts for all passes, then pass by pass
static int32_t sub_vote(const match_call& mc, match_sub& s, const vote_plan& plan) {
  shz_ctx* ctx = mc.ctx;
  if (plan.route == ROUTE_SINK) return vote_to_sink(mc, s);
  const std::vector<vote_pass>& passes = plan.passes;
  if (passes.empty()) return SHZ_OK;   // ROUTE_NONE, ROUTE_QUEUED
  uint64_t pmax = 0;
  for (const vote_pass& vp : passes) pmax = std::max(pmax, vp.v_hi - vp.v_lo);
  vote_bufs b;   // E lives in one of SORT_A/B; the vote buffers use SORT_C/D
  b.pmax4 = (pmax + 3) & ~3ull;   // second 4-byte vote buffer of a pass: 16-byte aligned behind the first
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_C, pmax * 8 + 16, &b.v0));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_D, pmax * 8, &b.v1));
  // the sub-group of every expand tile's first pair, for all passes in one launch: pass table (votes, first entry)
  // up, one kernel
  std::vector<uint32_t> toff(passes.size() + 1, 0);
  std::vector<uint64_t> ptab(passes.size() * 2 + (passes.size() + 2) / 2);   // pv[2 n_pass] | toff[n_pass + 1] (u32)
  for (size_t i = 0; i < passes.size(); ++i) {
    ptab[2 * i] = passes[i].v_lo;
    ptab[2 * i + 1] = passes[i].v_hi;
    toff[i + 1] = toff[i] + (uint32_t)((passes[i].v_hi - passes[i].v_lo + M_EXP_TILE - 1) / M_EXP_TILE) + 1;
  }
  memcpy(ptab.data() + passes.size() * 2, toff.data(), toff.size() * 4);
  void* tile_starts;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_HCNT, (uint64_t)toff.back() * 4, &tile_starts));   // (M5 belongs to the fold)
  const bool by_blocks = plan.route == ROUTE_TILES_FUSED;   // its expand goes by the sort's blocks: m_chunk_start_kernel per pass
  if (!by_blocks && passes.size() == 1) {   // no table to send up
    hipLaunchKernelGGL(m_tile_start_kernel, dim3(nblk(toff.back())), dim3(256), 0, ctx->stream, (const uint64_t*)s.po, (uint32_t)s.nx,
                       passes[0].v_lo, passes[0].v_hi, toff.back() - 1, (uint32_t*)tile_starts);
  } else if (!by_blocks) {
    void* d_ptab;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_VT4, ptab.size() * 8, &d_ptab));
    SHZ_HIP(ctx, shz_memcpy(ctx, d_ptab, ptab.data(), ptab.size() * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(m_tile_start_all_kernel, dim3(nblk(toff.back())), dim3(256), 0, ctx->stream, (const uint64_t*)s.po, (uint32_t)s.nx,
                       (const uint64_t*)d_ptab, (const uint32_t*)((const uint64_t*)d_ptab + passes.size() * 2),
                       (uint32_t)passes.size(), (uint32_t*)tile_starts);
  }
  SHZ_HIP(ctx, hipGetLastError());
  for (size_t i = 0; i < passes.size(); ++i)
    SHZ_TRY(vote_run_pass(mc, s, plan, passes[i], (const uint32_t*)tile_starts + toff[i], b));
  return SHZ_OK;
}

// no hash of the queries is looked up here (none given, or all of them another shard's): zero counters, no results
static void sub_commit_empty(match_call& mc, const match_sub& s) {
  if (mc.floor) mc.floor_rows.resize(mc.floor_rows.size() + (size_t)s.nq * FH_ROW, 0u);   // zero rows
  for (uint32_t q = s.q0; q < s.q0 + s.nq; ++q) {
    if (mc.out_nres) mc.out_nres[q] = 0;
    if (mc.out_nhash) mc.out_nhash[q] = 0;
    if (mc.out_npairs) mc.out_npairs[q] = 0;
  }
}

// the result block back (with the counts already, where the queued fold held) and out to the caller -- unless the LDS fold
// flagged an overflow: then nothing is committed and the queries go round again
static int32_t sub_commit(match_call& mc, const match_sub& s, vote_route route, sub_next* next) {
  shz_ctx* ctx = mc.ctx;
  const uint32_t q0 = s.q0, nq = s.nq;
  void* hb;
  double tr3 = 0.0;
  if (route == ROUTE_QUEUED) {
    ++ctx->st_spec_used;
    hb = (char*)s.mail + 256 + 8;   // came with the first read-back
    if (trace_match_env()) tr3 = now_s();
  } else {
    SHZ_TRY(shz_mailbox(ctx, s.rb_bytes, &hb));
    SHZ_HIP(ctx, hipMemcpyAsync(hb, s.rb, s.rb_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (trace_match_env()) tr3 = now_s();
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (trace_match_env())
    fprintf(stderr, "match trace: head enqueue %.1f us, wait %.1f us, tail enqueue %.1f us, wait %.1f us (P %llu)\n",
            (s.tr[1] - s.tr[0]) * 1e6, (s.tr[2] - s.tr[1]) * 1e6, (tr3 - s.tr[2]) * 1e6, (now_s() - tr3) * 1e6, (unsigned long long)s.P);
  const res_block h = res_block_at(hb, nq, s.nres);
  if (*h.vt_err != 0 && !s.redo) {
    ++ctx->st_vt_redo;
    *next = SUB_FULL_SORT;
    return SHZ_OK;
  }
  ctx->st_rows += s.rows_total;
  ctx->st_pairs += s.P;
  ctx->st_keys += s.ng;
  ctx->st_cap_groups += s.cap_groups;
  ctx->st_cap_pairs += s.cap_pairs;
  if (nq == 1) {
    if (mc.out_npairs) mc.out_npairs[q0] = s.kept;   // (P but under a song filter)
    if (mc.out_nhash) mc.out_nhash[q0] = (uint32_t)s.mu;
  } else {
    if (mc.out_npairs) memcpy(mc.out_npairs + q0, h.npairs, (uint64_t)nq * 8);
    if (mc.out_nhash) memcpy(mc.out_nhash + q0, h.nhash, (uint64_t)nq * 4);
  }
  if (!mc.sink) {
    const uint64_t o0 = (uint64_t)q0 * mc.topn;
    memcpy(mc.out_sid + o0, h.sid, s.nres * 4);
    memcpy(mc.out_delta + o0, h.delta, s.nres * 4);
    memcpy(mc.out_aligned + o0, h.aligned, s.nres * 4);
    memcpy(mc.out_dedup + o0, h.dedup, s.nres * 4);
    memcpy(mc.out_nres + q0, h.nres, (uint64_t)nq * 4);
  }
  if (mc.floor) {   // (a sub-batch that goes round again never gets here: its queries record once)
    const uint32_t* rows = (const uint32_t*)((const char*)hb + res_block_bytes(nq, s.nres));
    mc.floor_rows.insert(mc.floor_rows.end(), rows, rows + (size_t)nq * FH_ROW);
  }
  *next = SUB_DONE;
  return SHZ_OK;
}

// one visit of the sub-batch s: head -> (queued fold) -> counts -> route -> votes -> results
static int32_t match_sub_run(match_call& mc, match_sub& s, sub_next* next) {
  *next = SUB_GO;
  if (trace_match_env()) s.tr[0] = now_s();
  SHZ_TRY(sub_head(mc, s, next));
  if (*next != SUB_GO) return SHZ_OK;
  SHZ_TRY(sub_queue_fold(mc, s));
  SHZ_TRY(sub_read_counts(mc, s, next));
  if (*next != SUB_GO) return SHZ_OK;
  // the queued small query ran when its votes fit and the bias was the query's own -- or, for device input, the caller's
  // bound and no offset above it (else its kernels did nothing, or their results are overwritten, and the passes run as ever)
  const bool bias_held = (mc.flags & SHZ_IN_DEVICE) ? s.mb.bias <= s.queued_bias : s.mb.bias == s.queued_bias;
  vote_case c{s.nq, s.P, s.votes.data(), s.mb, mc.topn, s.full_sort, mc.sink != nullptr,
              s.queued && s.P <= VT_ONE_WG_MAX && bias_held, s.tol, vote_env()};
  vote_plan plan;
  vote_plan_make(c, &plan);
  SHZ_TRY(sub_vote(mc, s, plan));
  return sub_commit(mc, s, plan.route, next);
}

static int32_t match_core(match_call& mc) {
  shz_ctx* ctx = mc.ctx;
  shz_table* t = mc.t;
  if (!ctx || !t) return SHZ_E_INVALID;
  if (t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "table belongs to another ctx");
  if (pending_rows(t) || (!t->bucket && t->done.empty())) SHZ_FAIL(ctx, SHZ_E_STATE, "table not finalized");
  if (mc.n_queries == 0) return SHZ_OK;
  // offsets < 2^31: every delta fits out_delta's int32_t and, biased by a query offset < 2^20, 32 bits
  if (t->max_off >= (1u << 31))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "match: the table holds offset %u; offsets must be < 2^31", t->max_off);
  if (!mc.query_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "match: query_off is NULL");
  if (!mc.sink && (!mc.out_sid || !mc.out_delta || !mc.out_aligned || !mc.out_dedup || !mc.out_nres))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_batch: NULL buffer");
  if (!mc.sink && (mc.topn < 1 || mc.topn > 64)) SHZ_FAIL(ctx, SHZ_E_INVALID, "topn must be in [1,64]");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  ctx->st_rows = ctx->st_pairs = ctx->st_keys = ctx->st_cap_groups = ctx->st_cap_pairs = 0;
  // votes of one sub-batch of queries (one head: compose, sort, probe, one round trip): up to 2^30 where the device has
  // the memory for it (a sub-batch that ends up on the 8-byte path needs ~32 bytes per vote of workspace)
  mc.sub_budget = VOTE_PASS_MAX;
  if (mc.n_queries > 32) {
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) == hipSuccess)
      mc.sub_budget = std::min<uint64_t>(1ull << 30, std::max<uint64_t>(VOTE_PASS_MAX, (uint64_t)mem_free / 64));
  }
  SHZ_TRY(match_upload(mc));
  // a shard's compose marks hashes it does not own with the query index nq (sorted behind all queries): nq << 52 must
  // not wrap, so its sub-batches stay below MAX_Q_SUB
  uint32_t step = std::min<uint32_t>(mc.n_queries, (mc.sink && mc.sink->nshards > 1) ? MAX_Q_SUB - 1 : MAX_Q_SUB);
  mc.floor = ctx->vote_floor && !mc.sink;   // (shz_match_pairs votes nothing: its votes' rows are shz_pairs_vote's)
  mc.floor_rows.clear();
  if (mc.floor && (ctx->debug & SHZ_DEBUG_FLOOR_SMALL)) step = std::min<uint32_t>(step, FH_SMALL_Q);
  mc.filter = ctx->filter_sets != 0 && !mc.sink;   // (shz_match_pairs refuses a filter before it gets here)
  if (mc.filter && (ctx->debug & SHZ_DEBUG_FILTER_SMALL)) step = std::min<uint32_t>(step, FS_SMALL_Q);
  bool redo = false;
  for (uint32_t q0 = 0; q0 < mc.n_queries;) {
    match_sub s{};
    s.q0 = q0;
    s.nq = sub_queries(mc, q0, step);
    s.m = mc.query_off[q0 + s.nq] - mc.query_off[q0];
    if (s.m >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "query %u has too many hashes", q0);
    s.redo = redo;
    s.full_sort = redo || (mc.flags & SHZ_MATCH_FULL_SORT);
    s.tol = mc.sink ? -1 : vote_tol_of(ctx);
    s.mb = m_bits{bits_for(t->max_sid), 0, bits_for(s.nq - 1), 0};
    sub_next next;
    SHZ_TRY(match_sub_run(mc, s, &next));
    switch (next) {
      case SUB_FEWER: step = s.nq / 2; break;
      case SUB_FULL_SORT: redo = true; break;
      case SUB_EMPTY: sub_commit_empty(mc, s); q0 += s.nq; break;
      default: redo = false; q0 += s.nq; break;   // SUB_DONE
    }
  }
  if (mc.floor) ctx->floor_rows.insert(ctx->floor_rows.end(), mc.floor_rows.begin(), mc.floor_rows.end());
  return SHZ_OK;
}

extern "C" int32_t shz_match_batch(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                   const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                                   uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                                   uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs) {
  match_call mc{ctx, t, key32, q_off, query_off, n_queries, topn, flags, out_sid, out_delta, out_aligned, out_dedup,
                out_nres, out_nhash, out_npairs, nullptr};
  return match_core(mc);
}

// what shz_match_batch_sets / shz_match_device_host_sets refuse before anything is launched
static int32_t match_sets_check(shz_ctx* ctx, const char* who, uint32_t n_queries, const uint32_t* set_of_query) {
  if (!ctx->filter_sets) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: no song filter is set (shz_set_song_filter)", who);
  if (n_queries && !set_of_query) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: set_of_query is NULL", who);
  for (uint32_t q = 0; q < n_queries; ++q)
    if (set_of_query[q] >= ctx->filter_sets)
      SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: query %u asks for set %u of %u", who, q, set_of_query[q], ctx->filter_sets);
  return SHZ_OK;
}

extern "C" int32_t shz_match_batch_sets(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                        const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                                        uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                                        uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                                        const uint32_t* set_of_query) {
  if (!ctx || !t) return SHZ_E_INVALID;
  SHZ_TRY(match_sets_check(ctx, "shz_match_batch_sets", n_queries, set_of_query));
  match_call mc{ctx, t, key32, q_off, query_off, n_queries, topn, flags, out_sid, out_delta, out_aligned, out_dedup,
                out_nres, out_nhash, out_npairs, nullptr};
  mc.set_of = set_of_query;
  return match_core(mc);
}

// match_core on query columns that are already on the device and belong to the library (the fused recognise call, the
// listeners): query_off is the host's; bias_bound >= every q_off, or < 0 where the caller knows none
int32_t shz_match_device(shz_ctx* ctx, shz_table* t, const uint32_t* d_key32, const uint32_t* d_q_off, const uint64_t* query_off,
                         uint32_t n_queries, uint32_t topn, uint32_t flags, int64_t bias_bound, uint32_t* out_sid,
                         int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash,
                         uint64_t* out_npairs, const uint32_t* set_of_query) {
  match_call mc{ctx, t, d_key32, d_q_off, query_off, n_queries, topn, (flags & SHZ_MATCH_FULL_SORT) | SHZ_IN_DEVICE, out_sid,
                out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, nullptr};
  mc.has_bias_bound = bias_bound >= 0 && bias_bound < (int64_t)1 << 32;
  mc.bias_bound = mc.has_bias_bound ? (uint32_t)bias_bound : 0u;
  mc.pack_small = true;
  mc.set_of = set_of_query;   // (host; NULL from every caller inside the library: set 0)
  return match_core(mc);
}

// tests / tools: shz_match_device on HOST columns -- copied into device buffers of this call's own (not the workspace, which
// the match uses), handed to shz_match_device as its callers hand theirs, freed afterwards.  Nothing else is added: the
// bound, the flags and the outputs go through as they are.
static int32_t match_device_host(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                 const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags, int64_t bias_bound,
                                 uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned, uint32_t* out_dedup,
                                 uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs, const uint32_t* set_of_query) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (flags & ~SHZ_MATCH_FULL_SORT) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_device_host: flags may hold SHZ_MATCH_FULL_SORT");
  if (n_queries && !query_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_device_host: query_off is NULL");
  const uint64_t h1 = n_queries ? query_off[n_queries] : 0;
  if (h1 && (!key32 || !q_off)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_device_host: NULL column");
  if (h1 >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_device_host: %llu hashes", (unsigned long long)h1);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void *d_key = nullptr, *d_qo = nullptr;
  if (hipMalloc(&d_key, std::max<uint64_t>(h1, 1) * 4) != hipSuccess || hipMalloc(&d_qo, std::max<uint64_t>(h1, 1) * 4) != hipSuccess) {
    (void)hipGetLastError();
    if (d_key) (void)hipFree(d_key);
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_match_device_host: hipMalloc(2 x %llu) failed", (unsigned long long)(h1 * 4));
  }
  int32_t rc = SHZ_OK;
  if (h1 && (shz_memcpy(ctx, d_key, key32, h1 * 4, hipMemcpyHostToDevice) != hipSuccess ||
             shz_memcpy(ctx, d_qo, q_off, h1 * 4, hipMemcpyHostToDevice) != hipSuccess)) {
    ctx->err = "shz_match_device_host: copy of the columns failed";
    rc = SHZ_E_HIP;
  }
  if (rc == SHZ_OK)
    rc = shz_match_device(ctx, t, (const uint32_t*)d_key, (const uint32_t*)d_qo, query_off, n_queries, topn, flags, bias_bound,
                          out_sid, out_delta, out_aligned, out_dedup, out_nres, out_nhash, out_npairs, set_of_query);
  (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
  (void)hipFree(d_key);
  (void)hipFree(d_qo);
  return rc;
}
extern "C" int32_t shz_match_device_host(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                         const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                                         int64_t bias_bound, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                         uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs) {
  return match_device_host(ctx, t, key32, q_off, query_off, n_queries, topn, flags, bias_bound, out_sid, out_delta, out_aligned,
                           out_dedup, out_nres, out_nhash, out_npairs, nullptr);
}
// ... with the set of every query, as shz_match_batch_sets takes it (and refuses it)
extern "C" int32_t shz_match_device_host_sets(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                              const uint64_t* query_off, uint32_t n_queries, uint32_t topn, uint32_t flags,
                                              int64_t bias_bound, uint32_t* out_sid, int32_t* out_delta, uint32_t* out_aligned,
                                              uint32_t* out_dedup, uint32_t* out_nres, uint32_t* out_nhash, uint64_t* out_npairs,
                                              const uint32_t* set_of_query) {
  if (!ctx || !t) return SHZ_E_INVALID;
  SHZ_TRY(match_sets_check(ctx, "shz_match_device_host_sets", n_queries, set_of_query));
  return match_device_host(ctx, t, key32, q_off, query_off, n_queries, topn, flags, bias_bound, out_sid, out_delta, out_aligned,
                           out_dedup, out_nres, out_nhash, out_npairs, set_of_query);
}

// what match_core refuses before it launches anything, for callers that must know before they change state of their own
int32_t shz_match_ready(shz_ctx* ctx, shz_table* t, uint32_t topn) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "table belongs to another ctx");
  if (topn < 1 || topn > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "topn must be in [1,64]");
  if (pending_rows(t) || (!t->bucket && t->done.empty())) SHZ_FAIL(ctx, SHZ_E_STATE, "table not finalized");
  if (t->max_off >= (1u << 31))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "match: the table holds offset %u; offsets must be < 2^31", t->max_off);
  return SHZ_OK;
}

extern "C" int32_t shz_table_maxima(shz_table* t, uint32_t* max_sid, uint32_t* max_off) {
  if (!t) return SHZ_E_INVALID;
  if (max_sid) *max_sid = t->max_sid;
  if (max_off) *max_off = t->max_off;
  return SHZ_OK;
}

extern "C" int32_t shz_match_pairs(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                   const uint64_t* query_off, uint32_t n_queries, uint32_t flags, uint32_t shard,
                                   uint32_t nshards, uint32_t sid_bits, uint32_t delta_bits, uint32_t bias,
                                   uint64_t* d_pairs, uint64_t cap, uint64_t* count, uint32_t* out_nhash,
                                   uint64_t* out_npairs) {
  if (!ctx || !count) return SHZ_E_INVALID;
  if (ctx->filter_sets) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_pairs: a song filter is set (shz_set_song_filter): the sharded match does not apply it");
  if (cap && !d_pairs) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_pairs: NULL buffer");
  if (nshards == 0 || shard >= nshards) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_pairs: shard %u of %u", shard, nshards);
  if (sid_bits < 1 || delta_bits < 1 || delta_bits > 32 ||
      bits_for(n_queries ? n_queries - 1 : 0) + sid_bits + delta_bits + 1 > 64)
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_match_pairs: %u queries x %u sid bits x %u delta bits do not fit 64 bits", n_queries, sid_bits, delta_bits);
  pair_sink sink{d_pairs, cap, 0, m_bits{(int)sid_bits, (int)delta_bits, 0, bias}, shard, nshards};
  match_call mc{ctx, t, key32, q_off, query_off, n_queries, 1, flags, nullptr, nullptr, nullptr, nullptr, nullptr,
                out_nhash, out_npairs, &sink};
  SHZ_TRY(match_core(mc));
  *count = sink.count;
  if (sink.count > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_match_pairs: %llu votes, capacity %llu", (unsigned long long)sink.count, (unsigned long long)cap);
  return SHZ_OK;
}

extern "C" int32_t shz_set_debug(shz_ctx* ctx, uint32_t flags) {
  if (!ctx) return SHZ_E_INVALID;
  ctx->debug = flags;
  return SHZ_OK;
}
extern "C" int32_t shz_set_vote_tolerance(shz_ctx* ctx, uint32_t bins) {
  if (!ctx) return SHZ_E_INVALID;
  if (bins > 31) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_vote_tolerance: %u bins (at most 31)", bins);
  ctx->vote_tol = bins;
  return SHZ_OK;
}
extern "C" int32_t shz_get_vote_tolerance(shz_ctx* ctx, uint32_t* bins) {
  if (!ctx || !bins) return SHZ_E_INVALID;
  *bins = ctx->vote_tol;
  return SHZ_OK;
}
// the key cap: a setting of the context; the yield of a hash depends on it, so the estimate that sizes the next sub-batch
// (m_votes_per_hash) is forgotten when it changes
extern "C" int32_t shz_set_key_cap(shz_ctx* ctx, uint64_t rows) {
  if (!ctx) return SHZ_E_INVALID;
  if (rows != ctx->key_cap) ctx->m_votes_per_hash = 0.0;
  ctx->key_cap = rows;
  return SHZ_OK;
}
extern "C" int32_t shz_get_key_cap(shz_ctx* ctx, uint64_t* rows) {
  if (!ctx || !rows) return SHZ_E_INVALID;
  *rows = ctx->key_cap;
  return SHZ_OK;
}
extern "C" int32_t shz_key_cap_stats(shz_ctx* ctx, uint64_t* groups_dropped, uint64_t* pairs_dropped) {
  if (!ctx) return SHZ_E_INVALID;
  if (groups_dropped) *groups_dropped = ctx->st_cap_groups;
  if (pairs_dropped) *pairs_dropped = ctx->st_cap_pairs;
  return SHZ_OK;
}
extern "C" int32_t shz_set_vote_floor(shz_ctx* ctx, uint32_t on) {
  if (!ctx) return SHZ_E_INVALID;
  ctx->vote_floor = on ? 1u : 0u;
  if (!on) std::vector<uint32_t>().swap(ctx->floor_rows);   // off: the rows not taken are dropped
  return SHZ_OK;
}
// the song filter: one bitmap per set, built on the host, in a device block of the context's own.  Every refusal leaves the
// previous setting in force: the new block replaces the old one only when it is complete
extern "C" int32_t shz_set_song_filter(shz_ctx* ctx, const uint32_t* sids, const uint64_t* set_off, uint32_t n_sets, uint32_t flags) {
  if (!ctx) return SHZ_E_INVALID;
  if (flags & ~SHZ_FILTER_EXCLUDE) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_song_filter: flags may hold SHZ_FILTER_EXCLUDE");
  uint64_t n_ids = 0, words = 0;
  if (n_sets) {
    if (!set_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_song_filter: set_off is NULL");
    if (set_off[0] != 0) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_song_filter: set_off[0] is %llu, not 0", (unsigned long long)set_off[0]);
    for (uint32_t i = 0; i < n_sets; ++i)
      if (set_off[i + 1] < set_off[i]) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_song_filter: set_off decreases at set %u", i);
    n_ids = set_off[n_sets];
    if (n_ids && !sids) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_set_song_filter: sids is NULL");
    uint32_t top = 0;
    for (uint64_t i = 0; i < n_ids; ++i) top = std::max(top, sids[i]);
    words = n_ids ? (uint64_t)top / 32 + 1 : 0;
    if (words * n_sets * 4 > (1ull << 31))
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_set_song_filter: %u bitmaps of %llu words exceed 2^31 bytes", n_sets, (unsigned long long)words);
  }
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void* d_new = nullptr;
  if (n_sets) {
    std::vector<uint32_t> bm;
    try {
      bm.assign(std::max<uint64_t>(words * n_sets, 1), 0u);
    } catch (const std::bad_alloc&) {
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_set_song_filter: no host memory for %llu bitmap words", (unsigned long long)(words * n_sets));
    }
    for (uint32_t s = 0; s < n_sets; ++s)
      for (uint64_t i = set_off[s]; i < set_off[s + 1]; ++i) bm[(uint64_t)s * words + sids[i] / 32] |= 1u << (sids[i] & 31);
    if (hipMalloc(&d_new, bm.size() * 4) != hipSuccess) {
      (void)hipGetLastError();
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_set_song_filter: hipMalloc(%llu) failed", (unsigned long long)(bm.size() * 4));
    }
    if (shz_memcpy(ctx, d_new, bm.data(), bm.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) {
      (void)hipGetLastError();
      (void)hipFree(d_new);
      SHZ_FAIL(ctx, SHZ_E_HIP, "shz_set_song_filter: upload of the bitmaps failed");
    }
  }
  if (ctx->d_filter) {
    (void)hipStreamSynchronize(ctx->stream);   // (nothing queued reads the old block any more)
    (void)hipFree(ctx->d_filter);
  }
  ctx->d_filter = (uint32_t*)d_new;
  ctx->filter_sets = n_sets;
  ctx->filter_words = (uint32_t)words;
  ctx->filter_flags = n_sets ? flags : 0u;
  ctx->filter_ids = n_ids;
  return SHZ_OK;
}
extern "C" int32_t shz_get_song_filter(shz_ctx* ctx, uint32_t* n_sets, uint32_t* flags, uint64_t* n_ids) {
  if (!ctx) return SHZ_E_INVALID;
  if (n_sets) *n_sets = ctx->filter_sets;
  if (flags) *flags = ctx->filter_flags;
  if (n_ids) *n_ids = ctx->filter_ids;
  return SHZ_OK;
}
extern "C" int32_t shz_get_vote_floor(shz_ctx* ctx, uint32_t* on) {
  if (!ctx || !on) return SHZ_E_INVALID;
  *on = ctx->vote_floor;
  return SHZ_OK;
}
extern "C" int32_t shz_vote_floor_rows(shz_ctx* ctx, uint64_t* n) {
  if (!ctx || !n) return SHZ_E_INVALID;
  *n = ctx->floor_rows.size() / FH_ROW;
  return SHZ_OK;
}
extern "C" int32_t shz_vote_floor_take(shz_ctx* ctx, uint32_t* song_hist, uint32_t* bin_hist, uint64_t cap, uint64_t* n) {
  if (!ctx || !n) return SHZ_E_INVALID;
  const uint64_t rows = ctx->floor_rows.size() / FH_ROW;
  *n = rows;
  if (rows > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_vote_floor_take: %llu rows, capacity %llu", (unsigned long long)rows, (unsigned long long)cap);
  if (rows && (!song_hist || !bin_hist)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_vote_floor_take: NULL buffer");
  for (uint64_t q = 0; q < rows; ++q) {
    memcpy(song_hist + q * FH_BUCKETS, ctx->floor_rows.data() + q * FH_ROW, FH_BUCKETS * 4);
    memcpy(bin_hist + q * FH_BUCKETS, ctx->floor_rows.data() + q * FH_ROW + FH_BUCKETS, FH_BUCKETS * 4);
  }
  ctx->floor_rows.clear();
  return SHZ_OK;
}
extern "C" int32_t shz_vote_bucket(uint32_t count, uint32_t* bucket) {
  if (!bucket || count == 0) return SHZ_E_INVALID;
  *bucket = vote_bucket(count);
  return SHZ_OK;
}
void shz_floor_zero_rows(shz_ctx* ctx, uint64_t n) {
  if (ctx->vote_floor) ctx->floor_rows.resize(ctx->floor_rows.size() + n * FH_ROW, 0u);
}
extern "C" int32_t shz_match_vt_redo(shz_ctx* ctx, uint64_t* count) {
  if (!ctx || !count) return SHZ_E_INVALID;
  *count = ctx->st_vt_redo;
  return SHZ_OK;
}

extern "C" int32_t shz_match_spec_stats(shz_ctx* ctx, uint64_t* queued, uint64_t* used) {
  if (!ctx || !queued || !used) return SHZ_E_INVALID;
  *queued = ctx->st_spec_queued;
  *used = ctx->st_spec_used;
  return SHZ_OK;
}

extern "C" int32_t shz_match_stats(shz_ctx* ctx, uint64_t* rows_scanned, uint64_t* pairs, uint64_t* distinct_keys) {
  if (!ctx) return SHZ_E_INVALID;
  if (rows_scanned) *rows_scanned = ctx->st_rows;
  if (pairs) *pairs = ctx->st_pairs;
  if (distinct_keys) *distinct_keys = ctx->st_keys;
  return SHZ_OK;
}

// ---- the key sizes of a table (shz_table_key_hist): how many rows its keys hold.  One launch per segment s over its sorted
// key column, a workgroup owns KH_CHUNK consecutive rows (KH_PER rounds of 256 coalesced loads; the predecessor comes from the
// same cache lines).  A run head (key[i] != key[i - 1]) finds the end of its run in its bucket of the directory, then asks
// every other segment the way the probe does (range test, bucket, lower and upper bound); a key that a lower-numbered segment
// holds is that segment's to count.  Buckets: shz_vote_bucket's.  A wave adds the heads of an exact bucket (1 .. 16 rows: the
// rows follow from the count) with one LDS atomic pair per bucket present, the rare larger keys one by one; the workgroup's
// 64-bit LDS table goes to the global one once, in the words keys[32] | rows[32] | largest key | keys.
#define KH_PER 16
#define KH_CHUNK (256 * KH_PER)
#define KH_WORDS (2 * FH_BUCKETS + 2)
__device__ __forceinline__ uint32_t kh_rows_in(const shz_seg_dev& g, uint32_t key) {
  const uint64_t b = key >> 8;
  if (!(b < g.nbuckets && key >= g.key_lo && g.n)) return 0;
  uint32_t l = g.bucket[b], h = g.bucket[b + 1];
  const uint32_t h0 = h;
  while (l < h) {   // lower_bound(key)
    const uint32_t mid = l + ((h - l) >> 1);
    if (g.key[mid] < key) l = mid + 1; else h = mid;
  }
  const uint32_t lo = l;
  h = h0;
  while (l < h) {   // upper_bound(key)
    const uint32_t mid = l + ((h - l) >> 1);
    if (g.key[mid] <= key) l = mid + 1; else h = mid;
  }
  return l - lo;
}
__global__ __launch_bounds__(256) void key_hist_kernel(const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint32_t s,
                                                       unsigned long long* __restrict__ out /*[KH_WORDS]*/) {
  __shared__ unsigned long long sh[KH_WORDS];
  if (threadIdx.x < KH_WORDS) sh[threadIdx.x] = 0;
  __syncthreads();
  const shz_seg_dev me = segs[s];
  const uint32_t* __restrict__ key = me.key;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t base = (uint64_t)blockIdx.x * KH_CHUNK;
  unsigned long long top = 0;
  for (int r = 0; r < KH_PER; ++r) {
    const uint64_t i = base + (uint64_t)r * 256 + threadIdx.x;
    if (base + (uint64_t)r * 256 >= me.n) break;   // uniform
    bool head = false;
    uint32_t b = 0;
    unsigned long long rows = 0;
    if (i < me.n) {
      const uint32_t k = key[i];
      if (i == 0 || key[i - 1] != k) {
        uint32_t l = (uint32_t)i + 1, h = me.bucket[(k >> 8) + 1];   // upper_bound(k) behind the head, inside its bucket
        while (l < h) {
          const uint32_t mid = l + ((h - l) >> 1);
          if (key[mid] <= k) l = mid + 1; else h = mid;
        }
        rows = l - (uint32_t)i;
        head = true;
        for (uint32_t o = 0; o < nseg; ++o) {
          if (o == s) continue;
          const uint32_t ro = kh_rows_in(segs[o], k);
          if (ro && o < s) { head = false; break; }   // counted at the lowest segment that holds the key
          rows += ro;
        }
        if (head) b = rows >> 19 ? (uint32_t)FH_BUCKETS - 1u : vote_bucket((uint32_t)rows);
      }
    }
    const uint64_t heads = __ballot(head);
    if (heads == 0) continue;   // uniform
    if (lane == 0) atomicAdd(&sh[2 * FH_BUCKETS + 1], (unsigned long long)__popcll(heads));
    if (head && rows > top) top = rows;
    uint64_t todo = __ballot(head && b < 16u);
    while (todo) {   // uniform
      const int l = __ffsll((unsigned long long)todo) - 1;
      const uint32_t bb = (uint32_t)__shfl((int)b, l, 64);
      const uint64_t m = __ballot(head && b == bb);
      if ((int)lane == l) {
        atomicAdd(&sh[bb], (unsigned long long)__popcll(m));
        atomicAdd(&sh[FH_BUCKETS + bb], (unsigned long long)__popcll(m) * (bb + 1u));
      }
      todo &= ~m;
    }
    if (head && b >= 16u) {
      atomicAdd(&sh[b], 1ull);
      atomicAdd(&sh[FH_BUCKETS + b], rows);
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const unsigned long long o = (unsigned long long)__shfl_xor((long long)top, d, 64);
    top = o > top ? o : top;
  }
  if (lane == 0 && top) atomicMax(&sh[2 * FH_BUCKETS], top);
  __syncthreads();
  if (threadIdx.x < KH_WORDS && sh[threadIdx.x]) {
    if (threadIdx.x == 2 * FH_BUCKETS) atomicMax(out + threadIdx.x, sh[threadIdx.x]);
    else atomicAdd(out + threadIdx.x, sh[threadIdx.x]);
  }
}
extern "C" int32_t shz_table_key_hist(shz_table* t, uint64_t* keys, uint64_t* rows, uint64_t* max_rows, uint64_t* n_keys) {
  if (!t) return SHZ_E_INVALID;
  shz_ctx* ctx = t->ctx;
  if (!keys || !rows) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_table_key_hist: NULL histogram");
  if (pending_rows(t)) SHZ_FAIL(ctx, SHZ_E_STATE, "table has %llu staged rows; call shz_table_finalize first", (unsigned long long)pending_rows(t));
  uint64_t h[KH_WORDS] = {0};
  const std::vector<shz_seg> segs = all_segs(t);
  if (!segs.empty()) {
    SHZ_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<shz_seg_dev> hsegs;
    for (const shz_seg& g : segs) hsegs.push_back(seg_dev_of(g));
    const uint64_t seg_bytes = (sizeof(shz_seg_dev) * hsegs.size() + 255) & ~255ull;
    void* d;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC1, seg_bytes + KH_WORDS * 8, &d));
    unsigned long long* d_out = (unsigned long long*)((char*)d + seg_bytes);
    SHZ_HIP(ctx, shz_memcpy(ctx, d, hsegs.data(), sizeof(shz_seg_dev) * hsegs.size(), hipMemcpyHostToDevice));
    SHZ_HIP(ctx, hipMemsetAsync(d_out, 0, KH_WORDS * 8, ctx->stream));
    for (uint32_t s = 0; s < hsegs.size(); ++s) {
      if (!hsegs[s].n) continue;
      hipLaunchKernelGGL(key_hist_kernel, dim3((unsigned)(((uint64_t)hsegs[s].n + KH_CHUNK - 1) / KH_CHUNK)), dim3(256), 0,
                         ctx->stream, (const shz_seg_dev*)d, (uint32_t)hsegs.size(), s, d_out);
      SHZ_HIP(ctx, hipGetLastError());
    }
    SHZ_HIP(ctx, shz_memcpy(ctx, h, d_out, KH_WORDS * 8, hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  }
  memcpy(keys, h, FH_BUCKETS * 8);
  memcpy(rows, h + FH_BUCKETS, FH_BUCKETS * 8);
  if (max_rows) *max_rows = h[2 * FH_BUCKETS];
  if (n_keys) *n_keys = h[2 * FH_BUCKETS + 1];
  return SHZ_OK;
}

// ---------------------------------------------------------------------------------------- votes: gather + rank
extern "C" int32_t shz_pairs_allgather(shz_comm* c, uint64_t n_local, const uint64_t* d_pairs, uint64_t* d_all, uint64_t cap,
                                       uint64_t* n_total) {
  if (!c || !n_total) return SHZ_E_INVALID;
  int rank, nranks;
  shz_comm_info(c, &rank, &nranks);
  shz_ctx* ctx = shz_comm_ctx(c);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void* d_cnt;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC2, 8ull * (nranks + 1), &d_cnt));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_cnt, &n_local, 8, hipMemcpyHostToDevice));
  SHZ_TRY(shz_comm_allgather_bytes(c, d_cnt, (uint64_t*)d_cnt + 1, 8));
  std::vector<uint64_t> cnt(nranks), bytes(nranks), displ(nranks);
  SHZ_HIP(ctx, shz_memcpy(ctx, cnt.data(), (uint64_t*)d_cnt + 1, 8ull * nranks, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t total = 0;
  for (int r = 0; r < nranks; ++r) { displ[r] = total * 8; bytes[r] = cnt[r] * 8; total += cnt[r]; }
  *n_total = total;
  if (total > cap) SHZ_FAIL(ctx, SHZ_E_CAPACITY, "shz_pairs_allgather: %llu votes, capacity %llu", (unsigned long long)total, (unsigned long long)cap);
  if (total == 0) return SHZ_OK;
  if (!d_all || (n_local && !d_pairs)) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_pairs_allgather: NULL buffer");
  SHZ_TRY(shz_comm_allgatherv_bytes(c, d_pairs, d_all, bytes.data(), displ.data()));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

// ---- the gathered votes of a sharded match through the vote tiles
// first vote of every query in the pairs ordered by query: qstart[q] = first i with (pairs[i] >> shift) >= q, q = 0 .. nq
__global__ void pv_qstart_kernel(const uint64_t* __restrict__ pairs, uint64_t n, int shift, uint32_t nq,
                                 unsigned long long* __restrict__ qstart) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q > nq) return;
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((pairs[mid] >> shift) < q) lo = mid + 1; else hi = mid;
  }
  qstart[q] = lo;
}
// the 4-byte vote of the tiles: a pair without its query bits
__global__ void pv_narrow_kernel(const uint64_t* __restrict__ pairs, uint64_t n, uint32_t mask, uint32_t* __restrict__ k32) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    k32[i] = (uint32_t)pairs[i] & mask;
}

enum pv_tiles { PV_NOT_TAKEN /* nothing written */, PV_DONE, PV_REDO /* a tile gave up: the rows written are void */ };

// Votes of shz_match_pairs (8 bytes, query index on top) -> results, by the path of the unsharded match: ONE stable sort
// by the query bits (one or two passes over 8 bytes instead of the five of the full key), the query bits dropped, then
// the vote-tile passes over 4-byte votes.  Where it is not taken or gives up, the votes go through the full sort.
// It is ROUTE_TILES with another producer of the votes, and chosen by vote_plan_make's terms for that route: the 4-byte
// switch, the tile layout (one bit tighter: vt_layout_fits), 2^22 votes -- but over the whole call, not per pass: the sort
// by query and the read-back of the counts are paid before the passes are known.
static int32_t pairs_vote_tiles(shz_ctx* ctx, uint64_t* d_pairs, uint64_t* d_alt, uint64_t n, uint32_t nq, const m_bits& mb,
                                uint32_t topn, res_block r, pv_tiles* outcome) {
  *outcome = PV_NOT_TAKEN;
  const vote_switches& sw = vote_env();
  const int Bt = mb.sb + mb.dbits + 1;
  if (sw.vote32 == 0 || !vt_layout_fits(mb, topn, sw, 31)) return SHZ_OK;
  if (sw.vote32 != 1 && n < (1ull << 22)) return SHZ_OK;   // few votes: the passes' launches cost more than the full sort's extra bytes
  // 1. by query (stable: the order inside a query does not matter to the tiles)
  int sel = 0;
  if (mb.qb > 0) SHZ_TRY(shz_sort_u64(ctx, d_pairs, d_alt, nullptr, nullptr, 0, n, Bt, Bt + mb.qb, &sel));
  const uint64_t* sorted = sel ? d_alt : d_pairs;
  // 2. votes per query
  void *qs, *flag;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M0, ((uint64_t)nq + 1) * 8, &qs));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M1, 64, &flag));
  SHZ_HIP(ctx, hipMemsetAsync(flag, 0, 64, ctx->stream));
  r.vt_err = (uint32_t*)flag;   // the tiles' error word: this call has no block to keep it in
  hipLaunchKernelGGL(pv_qstart_kernel, dim3(nblk((uint64_t)nq + 1)), dim3(256), 0, ctx->stream, sorted, n, Bt, nq,
                     (unsigned long long*)qs);
  SHZ_HIP(ctx, hipGetLastError());
  std::vector<uint64_t> votes((size_t)nq + 1);   // first vote of every query, then their numbers
  SHZ_HIP(ctx, shz_memcpy(ctx, votes.data(), qs, ((uint64_t)nq + 1) * 8, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  for (uint32_t q = 0; q < nq; ++q) votes[q] = votes[q + 1] - votes[q];
  // 3. 4-byte votes; the other half of the buffer is the sort's second one
  void* kb;
  const uint64_t n4 = (n + 3) & ~3ull;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_C, (n4 * 2) * 4 + 64, &kb));
  uint32_t* k32 = (uint32_t*)kb;
  hipLaunchKernelGGL(pv_narrow_kernel, dim3((unsigned)std::min<uint64_t>(nblk(n), 65536)), dim3(256), 0, ctx->stream, sorted, n,
                     (uint32_t)((1ull << Bt) - 1ull), k32);
  SHZ_HIP(ctx, hipGetLastError());
  // 4. passes of up to VT_MAXQ queries and 2^28 votes
  m_bits mbp = mb;
  mbp.qb = 0;
  vote_pass vp{0, 0, 0, 0};
  while (next_vote_pass(votes.data(), nq, (uint32_t)VT_MAXQ, &vp)) {
    const uint64_t pp = vp.v_hi - vp.v_lo;
    if (pp >= (1ull << 32)) return SHZ_OK;   // (one query with 2^32 votes: the full sort's error message)
    if (pp == 0) continue;
    vt_plan pl;
    shz_seg_plan sp;
    vt_make_plan(votes.data() + vp.qa, vp.qb - vp.qa, mbp, pl, sp);
    // the pass sorts inside [v_lo, v_lo + pp) of k32 and of the second buffer; both offsets 16-byte aligned by address
    // is not required (the counting kernel aligns by address)
    SHZ_TRY(vt_run_pass(ctx, k32 + vp.v_lo, k32 + n4 + vp.v_lo, pp, pl, sp, mbp, topn, false,
                        mb.sb >= 31 ? 0x7FFFFFFFu : (1u << mb.sb), res_rows(r, vp.qa, topn)));
  }
  uint32_t h_flag = 0;
  SHZ_HIP(ctx, shz_memcpy(ctx, &h_flag, r.vt_err, 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  if (h_flag) ++ctx->st_vt_redo;
  *outcome = h_flag ? PV_REDO : PV_DONE;
  return SHZ_OK;
}

// (five arrays of shz_pairs_vote's own, not match_core's block that the probe zeroes along: the call has no probe)
static int32_t pv_zero_results(shz_ctx* ctx, const res_block& r, uint32_t nq, uint64_t nres) {
  SHZ_HIP(ctx, hipMemsetAsync(r.sid, 0, nres * 4, ctx->stream));
  SHZ_HIP(ctx, hipMemsetAsync(r.delta, 0, nres * 4, ctx->stream));
  SHZ_HIP(ctx, hipMemsetAsync(r.aligned, 0, nres * 4, ctx->stream));
  SHZ_HIP(ctx, hipMemsetAsync(r.dedup, 0, nres * 4, ctx->stream));
  SHZ_HIP(ctx, hipMemsetAsync(r.nres, 0, (uint64_t)nq * 4, ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_pairs_vote(shz_ctx* ctx, uint64_t* d_pairs, uint64_t n, uint32_t n_queries, uint32_t sid_bits,
                                  uint32_t delta_bits, uint32_t bias, uint32_t topn, uint32_t* out_sid, int32_t* out_delta,
                                  uint32_t* out_aligned, uint32_t* out_dedup, uint32_t* out_nres) {
  if (!ctx) return SHZ_E_INVALID;
  if (ctx->filter_sets) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_pairs_vote: a song filter is set (shz_set_song_filter): the sharded match does not apply it");
  if (n_queries == 0) return SHZ_OK;
  if (!out_sid || !out_delta || !out_aligned || !out_dedup || !out_nres) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_pairs_vote: NULL output");
  if (topn < 1 || topn > 64) SHZ_FAIL(ctx, SHZ_E_INVALID, "topn must be in [1,64]");
  if (n >= (1ull << 32)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_pairs_vote: %llu votes (limit 2^32); vote fewer queries per call", (unsigned long long)n);
  m_bits mb{(int)sid_bits, (int)delta_bits, bits_for(n_queries - 1), bias};
  if (sid_bits < 1 || delta_bits < 1 || mb.qb + mb.sb + mb.dbits + 1 > 64) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_pairs_vote: key layout does not fit 64 bits");
  if (delta_bits > 32) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "shz_pairs_vote: %u delta bits (at most 32)", delta_bits);
  const uint64_t nres = (uint64_t)n_queries * topn;
  memset(out_sid, 0, nres * 4); memset(out_delta, 0, nres * 4); memset(out_aligned, 0, nres * 4);
  memset(out_dedup, 0, nres * 4); memset(out_nres, 0, (uint64_t)n_queries * 4);
  if (n == 0) { shz_floor_zero_rows(ctx, n_queries); return SHZ_OK; }
  if (!d_pairs) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_pairs_vote: NULL votes");
  if ((uintptr_t)d_pairs & 15) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_pairs_vote: the vote buffer must be 16-byte aligned");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void *v1, *tot, *r_sid, *r_delta, *r_al, *r_dd, *r_n;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_D, n * 8, &v1));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC0, 64, &tot));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_PEAK_F, nres * 4, &r_sid));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_PEAK_T, nres * 4, &r_delta));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_PEAK_CLIP, nres * 4, &r_al));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC1, nres * 4, &r_dd));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC2, (uint64_t)n_queries * 4, &r_n));
  const res_block r_plain{nullptr, (uint32_t*)r_sid, (int32_t*)r_delta, (uint32_t*)r_al, (uint32_t*)r_dd, (uint32_t*)r_n, nullptr,
                          nullptr};
  res_block r = r_plain;
  const uint64_t floor_bytes = (uint64_t)n_queries * FH_ROW * 4;
  if (ctx->vote_floor) {   // the vote floor: the rows of the gathered votes, as match_core records its own
    void* fh;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC3, floor_bytes, &fh));
    SHZ_HIP(ctx, hipMemsetAsync(fh, 0, floor_bytes, ctx->stream));
    r.hist = (uint32_t*)fh;
  }
  SHZ_TRY(pv_zero_results(ctx, r, n_queries, nres));
  const int tol = vote_tol_of(ctx);   // a tolerance (or the vote floor): the full sort and the tolerant fold, as in the unsharded match
  pv_tiles tiles = PV_NOT_TAKEN;
  if (tol < 0) SHZ_TRY(pairs_vote_tiles(ctx, d_pairs, (uint64_t*)v1, n, n_queries, mb, topn, r, &tiles));
  if (tiles == PV_REDO) SHZ_TRY(pv_zero_results(ctx, r, n_queries, nres));
  // (the full sort orders any permutation of the votes: whatever the sort by query left in d_pairs / v1 is fine for it)
  if (tiles != PV_DONE) SHZ_TRY(vote_tail(ctx, d_pairs, (uint64_t*)v1, n, n_queries, mb, topn, tol, (uint64_t*)tot, r));
  SHZ_HIP(ctx, shz_memcpy(ctx, out_sid, r_sid, nres * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, out_delta, r_delta, nres * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, out_aligned, r_al, nres * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, out_dedup, r_dd, nres * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, out_nres, r_n, (uint64_t)n_queries * 4, hipMemcpyDeviceToHost));
  std::vector<uint32_t> rows;
  if (r.hist) {
    rows.resize((size_t)n_queries * FH_ROW);
    SHZ_HIP(ctx, shz_memcpy(ctx, rows.data(), r.hist, floor_bytes, hipMemcpyDeviceToHost));
  }
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  ctx->floor_rows.insert(ctx->floor_rows.end(), rows.begin(), rows.end());
  return SHZ_OK;
}
