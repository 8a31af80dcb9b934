// Match extents: WHERE in the query and in the song the aligned hashes of known winners lie.
//   shz_match_extents / shz_match_songs_extents -> ex_device, on query columns that are on the device; shz_scan_extents
//   (shz_scan.hip) calls ex_device on the zones it cuts from a scan's own hash lists.
//
// A second, cheap pass over the (query hash, table row) pairs of the match.  The winners are known, so nothing is sorted by
// song: the head composes (query, key32, q_off) elements, sorts them and drops duplicates (the set semantics of the match),
// and finds the row range of every distinct element in every segment (the bucket fetch + lower / upper bound of the match's
// probe, foreign segments skipped by their key range).  An exclusive scan of the rows per (element, segment) numbers the
// pairs; a workgroup of the extent kernel owns a tile of EX_TILE consecutive PAIRS, whatever elements they belong to (one
// key owns thousands of rows at 1M songs), finds its first (element, segment) by search and keeps the descriptors it walks
// in LDS, EX_SUB at a time.  Per pair it loads the row's song id and offset (8 bytes), forms d = off - q_off in 64-bit signed
// arithmetic and tests it against the candidates of the pair's query, which sit in LDS for the first EX_QC queries a chunk
// touches.  Almost every pair misses: load, compare, nothing.  A hit is accumulated with integer atomicAdd / atomicMin /
// atomicMax alone -- in LDS for those queries, flushed once per (chunk, candidate touched) -- so no order changes a result.
// The rows of a key are streamed: nothing here relies on their order inside the key.
//
// The moments of a candidate's pairs (shz_match_extents_fit, and the extent stage of
// shz_recognize_warps_extents): with q = q_off and u = d - d_lo of every pair that belongs, sum q, sum u, sum q^2 and sum q u
// in unsigned 64 bits, accumulated where the count is -- four 64-bit LDS adds a hit into one 32-byte cell of the candidate
// (an LDS atomic costs what a store costs at either width, experiments/lds_ops/README.md), flushed with the count; 64-bit
// global adds for the other queries.  The kernel is a template: without the moments it is the code it was.
#include "shz_table_int.h"

#define EX_QOFF_BITS 20
#define EX_KEY_SHIFT 20
#define EX_QIDX_SHIFT 52
#define EX_MAX_Q_SUB 4096u      // the query index has 12 bits in an element: more queries are cut into sub-batches
#define EX_SMALL_Q_SUB 3u       // ... under SHZ_DEBUG_EXTENT_SMALL_TILES
#define EX_TILE 2048u           // pairs of a workgroup
#define EX_SMALL_TILE 64u
#define EX_SUB 512u             // (element, segment) descriptors of a chunk in LDS
#define EX_SMALL_SUB 4u
#define EX_QC 4u                // queries of a chunk whose candidates and accumulators live in LDS (the others: global memory)
#define EX_MAX_CAND 64u
#define EX_HIST 64u
// EX_DIRECT_ATOMICS (a build switch for the A/B of DESIGN.md 3.7k, never set in the library): every hit goes to global memory

struct exctl {
  unsigned long long mu;   // distinct elements of the sub-batch
  unsigned long long P;    // its pairs
  unsigned int err;        // a query offset >= 2^20
  unsigned int pad;
};

__host__ __device__ __forceinline__ uint32_t ex_shift_of(uint32_t top) {
  uint32_t s = 0;
  while ((top >> s) >= EX_HIST) ++s;
  return s;
}

// element i of the sub-batch: (query, key32, q_off); the largest offset of every query; the "offset too wide" flag.
// A wave's 64 consecutive elements lie in one or two queries: ONE search per wave for its first element, then every lane
// walks on from there (m_compose_kernel's scheme), and ONE atomicMax per wave for the query of its first lane -- the lanes of
// a later query add theirs on their own.  (One atomicMax per element behind a read of the same word was an atomic hot spot:
// 0.79 ms of a 1.45 ms call for 577,000 elements of 200 queries)
__global__ void ex_compose_kernel(const uint32_t* __restrict__ key32, const uint32_t* __restrict__ q_off,
                                  const uint64_t* __restrict__ query_off /* sub-batch CSR, nq + 1 */, uint32_t nq, uint64_t m,
                                  uint64_t* __restrict__ c, uint32_t* __restrict__ qmax /* of the sub-batch */,
                                  uint32_t* __restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t iw = i & ~63ull;   // the wave's first element: the same in every lane, and told so to the compiler
  const uint64_t i0 = (uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)iw) |
                      ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(iw >> 32)) << 32);
  if (i0 >= m) return;   // uniform
  const uint64_t h0 = query_off[0] + i0;
  uint32_t w_lo = 0, w_hi = nq;   // the last query whose first hash is not behind h0 (empty queries share a start)
  while (w_hi - w_lo > 1) {        // uniform
    const uint32_t mid = (w_lo + w_hi) >> 1;
    if (query_off[mid] <= h0) w_lo = mid; else w_hi = mid;
  }
  const bool live = i < m;
  uint32_t q = w_lo, o = 0, key = 0;
  if (live) {
    const uint64_t h = query_off[0] + i;
    while (q + 1 < nq && query_off[q + 1] <= h) ++q;
    o = q_off[h];
    key = key32[h];
  }
  if (__ballot(live && (o >> EX_QOFF_BITS)) && lane == 0) atomicOr(err, 1u);
  uint32_t wmax = (live && q == w_lo) ? o : 0u;   // (lane 0 is live and in query w_lo)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) wmax = max(wmax, (uint32_t)__shfl_xor((int)wmax, d, 64));
  if (lane == 0 && wmax > *(volatile uint32_t*)(qmax + w_lo)) atomicMax(qmax + w_lo, wmax);   // (the maximum only grows)
  if (live && q != w_lo && o > *(volatile uint32_t*)(qmax + q)) atomicMax(qmax + q, o);
  if (live) c[i] = ((uint64_t)q << EX_QIDX_SHIFT) | ((uint64_t)key << EX_KEY_SHIFT) | (o & ((1u << EX_QOFF_BITS) - 1));
}

__global__ void ex_flag_kernel(const uint64_t* __restrict__ c, uint64_t n, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) flag[i] = (i == 0 || c[i] != c[i - 1]) ? 1u : 0u;
}

__global__ void ex_compact_kernel(const uint64_t* __restrict__ c, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                  uint64_t n, uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[pos[i]] = c[i];
}

// rows [lo, lo + rows) of element e in segment sg, one thread per x = e * nseg + sg; slots from mu * nseg up to the bound
// hold no rows, so that the exclusive scan of rows[] ends in the pairs of the sub-batch everywhere behind the last element
__global__ void ex_probe_kernel(const uint64_t* __restrict__ E, const unsigned long long* __restrict__ mu_dev, uint64_t bound,
                                const shz_seg_dev* __restrict__ segs, uint32_t nseg, uint32_t* __restrict__ g_lo,
                                uint64_t* __restrict__ g_rows) {
  const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= bound) return;
  const uint64_t nx = (uint64_t)*mu_dev * nseg;   // <= bound - 1
  uint32_t lo = 0, rows = 0;
  if (x < nx) {
    const uint32_t e = (uint32_t)(x / nseg), sg = (uint32_t)(x - (uint64_t)e * nseg);
    const uint32_t key = (uint32_t)(E[e] >> EX_KEY_SHIFT);
    const uint64_t b = key >> 8;
    const uint32_t* __restrict__ tkey = segs[sg].key;
    // a segment is asked only for keys inside [its first key, its last bucket] (the match's probe)
    if (b < segs[sg].nbuckets && key >= segs[sg].key_lo && segs[sg].n) {
      uint32_t l = segs[sg].bucket[b], h = segs[sg].bucket[b + 1];
      const uint32_t h0 = h;
      while (l < h) {   // lower_bound(key)
        const uint32_t mid = l + ((h - l) >> 1);
        if (tkey[mid] < key) l = mid + 1; else h = mid;
      }
      lo = l;
      h = h0;
      while (l < h) {   // upper_bound(key)
        const uint32_t mid = l + ((h - l) >> 1);
        if (tkey[mid] <= key) l = mid + 1; else h = mid;
      }
      rows = l - lo;
    }
  }
  g_lo[x] = lo;
  g_rows[x] = rows;
}

struct ex_cands {                 // the call's candidates and outputs on the device, [n_queries * ncand] each
  const uint32_t* sid;
  const int32_t *dlo, *dhi;
  const uint32_t* n;              // [n_queries]
  const uint32_t* qmax;           // [n_queries]: the largest offset of every query (complete for the sub-batch at hand)
  uint32_t *count, *q_first, *q_last, *t_first, *t_last;
  uint32_t* hist;                 // [n_queries * ncand * 64], or NULL
  uint32_t ncand;
  unsigned long long* fit;        // [n_queries * ncand][4]: sum q, sum u, sum q^2, sum q u of every candidate, or NULL
};

// one hit of candidate cell (query * ncand + slot), straight to global memory
__device__ __forceinline__ void ex_hit_global(const ex_cands& C, uint64_t cell, uint32_t qo, uint32_t off) {
  atomicAdd(C.count + cell, 1u);
  atomicMin(C.q_first + cell, qo);
  atomicMax(C.q_last + cell, qo);
  atomicMin(C.t_first + cell, off);
  atomicMax(C.t_last + cell, off);
}
// the four moments of one hit, q = q_off and u = d - d_lo < EX_FIT_MAX_WIDTH (so q u < 2^32), added to a cell's four words
__device__ __forceinline__ void ex_hit_fit(unsigned long long* __restrict__ f, uint32_t qo, uint32_t u) {
  atomicAdd(f + 0, (unsigned long long)qo);
  atomicAdd(f + 1, (unsigned long long)u);
  atomicAdd(f + 2, (unsigned long long)qo * qo);
  atomicAdd(f + 3, (unsigned long long)qo * u);
}

// tile = pairs [blockIdx.x * tile, ... + tile) of the sub-batch's P; po[x] = pairs in front of x = (element, segment), nx + 1
// entries at least (po[nx] = P); q0 = the sub-batch's first query in the call.  FIT: the moments too (C.fit is not NULL)
template <bool FIT>
__global__ __launch_bounds__(256) void ex_pairs_kernel(const uint64_t* __restrict__ E, const uint64_t* __restrict__ po,
                                                        const uint32_t* __restrict__ g_lo, uint32_t nx, uint32_t nseg,
                                                        const shz_seg_dev* __restrict__ segs, uint64_t P, uint32_t tile,
                                                        uint32_t sub_cap, uint32_t q0, ex_cands C) {
  __shared__ uint64_t s_e[EX_SUB];
  __shared__ uint64_t s_po[EX_SUB + 1];
  __shared__ uint32_t s_lo[EX_SUB];
  __shared__ uint16_t s_sg[EX_SUB];
  __shared__ uint32_t s_csid[EX_QC * EX_MAX_CAND];
  __shared__ int32_t s_clo[EX_QC * EX_MAX_CAND], s_chi[EX_QC * EX_MAX_CAND];
  __shared__ uint32_t s_cnt[EX_QC * EX_MAX_CAND], s_qmin[EX_QC * EX_MAX_CAND], s_qmaxv[EX_QC * EX_MAX_CAND],
      s_tmin[EX_QC * EX_MAX_CAND], s_tmax[EX_QC * EX_MAX_CAND];
  __shared__ uint32_t s_cn[EX_QC], s_shift[EX_QC];
  __shared__ uint32_t s_x[2];
  __shared__ unsigned long long s_fit[FIT ? EX_QC * EX_MAX_CAND * 4 : 1];   // 8 KB: a candidate's four sums side by side
#ifdef EX_DIRECT_ATOMICS
  const bool lds_acc = false;
#else
  const bool lds_acc = true;
#endif
  const uint32_t tid = threadIdx.x, ncand = C.ncand;
  const uint64_t p0 = (uint64_t)blockIdx.x * tile, p1 = min(p0 + tile, P);
  if (p0 >= P) return;   // uniform
  if (tid < 2) {         // the last x with po[x] <= the tile's first / last pair: it has rows, and the pair is one of them
    const uint64_t p = tid == 0 ? p0 : p1 - 1;
    uint32_t l = 0, h = nx;
    while (h - l > 1) {
      const uint32_t mid = l + ((h - l) >> 1);
      if (po[mid] <= p) l = mid; else h = mid;
    }
    s_x[tid] = l;
  }
  __syncthreads();
  const uint32_t x0 = s_x[0], x1 = s_x[1];
  for (uint32_t xc = x0; xc <= x1; xc += sub_cap) {
    const uint32_t nsub = min(sub_cap, x1 - xc + 1);
    for (uint32_t i = tid; i <= nsub; i += 256) {
      const uint32_t x = xc + i;   // (<= nx: po has that entry)
      s_po[i] = po[x];
      if (i < nsub) {
        const uint32_t e = x / nseg;
        s_e[i] = E[e];
        s_sg[i] = (uint16_t)(x - e * nseg);
        s_lo[i] = g_lo[x];
      }
    }
    const uint32_t qa = (uint32_t)(E[xc / nseg] >> EX_QIDX_SHIFT);   // the chunk's first query (uniform)
    if (lds_acc) {
      for (uint32_t i = tid; i < EX_QC * EX_MAX_CAND; i += 256) {
        s_cnt[i] = 0; s_qmin[i] = 0xFFFFFFFFu; s_qmaxv[i] = 0; s_tmin[i] = 0xFFFFFFFFu; s_tmax[i] = 0;
      }
      if (tid < EX_QC) s_cn[tid] = 0;
      if (FIT)
        for (uint32_t i = tid; i < EX_QC * EX_MAX_CAND * 4; i += 256) s_fit[i] = 0;
    }
    __syncthreads();
    if (lds_acc) {
      // the queries qa .. qa + EX_QC - 1 that some element of the chunk belongs to, found through the elements: no query
      // index beyond the sub-batch is formed, and a query without pairs here keeps s_cn = 0
      for (uint32_t i = tid; i < nsub; i += 256) {
        const uint32_t q = (uint32_t)(s_e[i] >> EX_QIDX_SHIFT), j = q - qa;
        const bool head = i == 0 || (uint32_t)(s_e[i - 1] >> EX_QIDX_SHIFT) != q;
        if (head && j < EX_QC) {
          s_cn[j] = min(C.n[q0 + q], ncand);
          s_shift[j] = ex_shift_of(C.qmax[q0 + q]);
        }
      }
      __syncthreads();
      for (uint32_t i = tid; i < EX_QC * EX_MAX_CAND; i += 256) {
        const uint32_t j = i / EX_MAX_CAND, c = i - j * EX_MAX_CAND;
        if (c < s_cn[j]) {
          const uint64_t cell = ((uint64_t)q0 + qa + j) * ncand + c;
          s_csid[i] = C.sid[cell];
          s_clo[i] = C.dlo[cell];
          s_chi[i] = C.dhi[cell];
        }
      }
      __syncthreads();
    }
    const uint64_t a = max(s_po[0], p0), b = min(s_po[nsub], p1);
    for (uint64_t p = a + tid; p < b; p += 256) {
      uint32_t l = 0, h = nsub;   // the last descriptor with po <= p
      while (h - l > 1) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (s_po[mid] <= p) l = mid; else h = mid;
      }
      const uint64_t e = s_e[l];
      const uint32_t q = (uint32_t)(e >> EX_QIDX_SHIFT), qo = (uint32_t)e & ((1u << EX_QOFF_BITS) - 1);
      const uint32_t row = s_lo[l] + (uint32_t)(p - s_po[l]);
      const shz_seg_dev& g = segs[s_sg[l]];
      const uint32_t sid = g.sid[row], off = g.off[row];
      const int64_t d = (int64_t)off - (int64_t)qo;
      const uint32_t j = q - qa;
      if (lds_acc && j < EX_QC) {
        const uint32_t n = s_cn[j];
        for (uint32_t c = 0; c < n; ++c) {
          const uint32_t k = j * EX_MAX_CAND + c;
          if (s_csid[k] == sid && d >= (int64_t)s_clo[k] && d <= (int64_t)s_chi[k]) {
            atomicAdd(s_cnt + k, 1u);
            atomicMin(s_qmin + k, qo);
            atomicMax(s_qmaxv + k, qo);
            atomicMin(s_tmin + k, off);
            atomicMax(s_tmax + k, off);
            if (FIT) ex_hit_fit(s_fit + 4 * k, qo, (uint32_t)(d - (int64_t)s_clo[k]));
            if (C.hist) atomicAdd(C.hist + ((((uint64_t)q0 + q) * ncand + c) << 6) + (qo >> s_shift[j]), 1u);
          }
        }
      } else {
        const uint64_t gq = (uint64_t)q0 + q;
        const uint32_t n = C.n[gq];
        for (uint32_t c = 0; c < n; ++c) {
          const uint64_t cell = gq * ncand + c;
          if (C.sid[cell] == sid && d >= (int64_t)C.dlo[cell] && d <= (int64_t)C.dhi[cell]) {
            ex_hit_global(C, cell, qo, off);
            if (FIT) ex_hit_fit(C.fit + 4 * cell, qo, (uint32_t)(d - (int64_t)C.dlo[cell]));
            if (C.hist) atomicAdd(C.hist + (cell << 6) + (qo >> ex_shift_of(C.qmax[gq])), 1u);
          }
        }
      }
    }
    __syncthreads();
    if (lds_acc) {   // one flush per (chunk, candidate touched)
      for (uint32_t i = tid; i < EX_QC * EX_MAX_CAND; i += 256) {
        if (s_cnt[i] == 0) continue;
        const uint32_t j = i / EX_MAX_CAND, c = i - j * EX_MAX_CAND;
        const uint64_t cell = ((uint64_t)q0 + qa + j) * ncand + c;
        atomicAdd(C.count + cell, s_cnt[i]);
        atomicMin(C.q_first + cell, s_qmin[i]);
        atomicMax(C.q_last + cell, s_qmaxv[i]);
        atomicMin(C.t_first + cell, s_tmin[i]);
        atomicMax(C.t_last + cell, s_tmax[i]);
        if (FIT)
          for (uint32_t k = 0; k < 4; ++k) atomicAdd(C.fit + 4 * cell + k, s_fit[4 * i + k]);
      }
      __syncthreads();
    }
  }
}

// before the pairs: the minima start at the top
__global__ void ex_init_kernel(uint32_t* __restrict__ q_first, uint32_t* __restrict__ t_first, uint64_t cells) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells) { q_first[i] = 0xFFFFFFFFu; t_first[i] = 0xFFFFFFFFu; }
}
// after them: a candidate nothing belongs to is all zeros; the shift of every query
__global__ void ex_tail_kernel(const uint32_t* __restrict__ count, uint32_t* __restrict__ q_first, uint32_t* __restrict__ t_first,
                               uint64_t cells, const uint32_t* __restrict__ qmax, uint32_t nq, uint32_t* __restrict__ shift) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells && count[i] == 0) { q_first[i] = 0; t_first[i] = 0; }
  if (i < nq) shift[i] = ex_shift_of(qmax[i]);
}

namespace {

struct own_bufs {   // device allocations of one call, freed when it ends
  std::vector<void*> p;
  ~own_bufs() {
    for (void* q : p) (void)hipFree(q);
  }
  void* get(uint64_t bytes) {
    void* q = nullptr;
    if (hipMalloc(&q, std::max<uint64_t>(bytes, 256)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    p.push_back(q);
    return q;
  }
};

}  // namespace

// (ex_args, and the declarations of what follows: shz_internal.h -- the scan calls them on its own device columns)
int32_t ex_table_limits(shz_ctx* ctx, shz_table* t, const char* who) {
  if (t->max_off >= (1u << 31))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: the table holds offset %u; offsets must be < 2^31", who, t->max_off);
  return SHZ_OK;
}

// what every form refuses about the table and the candidates before anything is launched (n > 0)
int32_t ex_check(shz_ctx* ctx, shz_table* t, const char* who, const ex_args& A) {
  if (!A.cand_sid || !A.cand_dlo || !A.cand_dhi || !A.cand_n) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL candidate array", who);
  if (!A.out_count || !A.out_q_first || !A.out_q_last || !A.out_t_first || !A.out_t_last || !A.out_shift)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL output array", who);
  const int nfit = !!A.out_sum_q + !!A.out_sum_u + !!A.out_sum_qq + !!A.out_sum_qu;
  if (nfit != 0 && nfit != 4) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL sum array (all four, or none)", who);
  for (uint32_t q = 0; q < A.n_queries; ++q) {
    if (A.cand_n[q] > A.ncand) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: cand_n[%u] = %u is above ncand = %u", who, q, A.cand_n[q], A.ncand);
    for (uint32_t c = 0; c < A.cand_n[q]; ++c) {
      const uint64_t i = (uint64_t)q * A.ncand + c;
      if (A.cand_dlo[i] > A.cand_dhi[i])
        SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: candidate %u of query %u has d_lo = %d above d_hi = %d", who, c, q, A.cand_dlo[i], A.cand_dhi[i]);
      if (nfit && (int64_t)A.cand_dhi[i] - A.cand_dlo[i] >= EX_FIT_MAX_WIDTH)
        SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: candidate %u of query %u spans d_lo = %d .. d_hi = %d; with the sums d_hi - d_lo must be < %d",
                 who, c, q, A.cand_dlo[i], A.cand_dhi[i], EX_FIT_MAX_WIDTH);
    }
  }
  return ex_table_limits(ctx, t, who);
}

int32_t ex_state(shz_ctx* ctx, shz_table* t, const char* who, uint32_t ncand) {
  if (t->ctx != ctx) SHZ_FAIL(ctx, SHZ_E_INVALID, "table belongs to another ctx");
  if (ncand < 1 || ncand > EX_MAX_CAND) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: ncand must be in [1,64]", who);
  if (t->broken) SHZ_FAIL(ctx, SHZ_E_STATE, "table lost rows in a failed finalize");
  if (pending_rows(t) || (!t->bucket && t->done.empty())) SHZ_FAIL(ctx, SHZ_E_STATE, "%s: table not finalized", who);
  return SHZ_OK;
}

// The one path of every entry point (the two below, and shz_scan_extents on the zones of a scan; whoever holds query columns
// on the device later -- the listeners -- calls it the same way): d_key32 / d_q_off are device columns, query_off (host)
// their CSR, never decreasing; the rest of A is checked (ex_check).  The outputs are written only when the whole call
// succeeded.
int32_t ex_device(shz_ctx* ctx, shz_table* t, const char* who, const uint32_t* d_key32, const uint32_t* d_q_off,
                  const uint64_t* query_off, const ex_args& A) {
  const uint32_t nq_all = A.n_queries, ncand = A.ncand;
  const uint64_t cells = (uint64_t)nq_all * ncand;
  const bool small = (ctx->debug & SHZ_DEBUG_EXTENT_SMALL_TILES) != 0;
  const uint32_t tile = small ? EX_SMALL_TILE : EX_TILE, sub_cap = small ? EX_SMALL_SUB : EX_SUB;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  // segment descriptors (an empty table probes one empty segment)
  std::vector<shz_seg_dev> hsegs;
  for (const shz_seg& g : all_segs(t)) hsegs.push_back(seg_dev_of(g));
  if (hsegs.empty()) hsegs.push_back(shz_seg_dev{nullptr, nullptr, nullptr, t->bucket, 0u, 0u, 0ull});
  const uint32_t nseg = (uint32_t)hsegs.size();
  void *d_segs, *d_qoff, *d_cand, *d_ctl, *d_out;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_SEGS, sizeof(shz_seg_dev) * SHZ_MAX_SEGS, &d_segs));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_QOFF, ((uint64_t)nq_all + 1) * 8, &d_qoff));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_CAND, cells * 12 + (uint64_t)nq_all * 4, &d_cand));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_CTL, 256 + (uint64_t)nq_all * 8, &d_ctl));   // exctl | qmax | shift
  const uint64_t hist_words = A.out_hist ? cells * EX_HIST : 0;
  const bool fit = A.out_sum_q != nullptr;
  const uint64_t fit_at = ((cells * 5 + hist_words) * 4 + 7) & ~7ull, out_bytes = fit_at + (fit ? cells * 32 : 0);   // ... | the sums
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_OUT, out_bytes, &d_out));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_segs, hsegs.data(), sizeof(shz_seg_dev) * nseg, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, d_qoff, query_off, ((uint64_t)nq_all + 1) * 8, hipMemcpyHostToDevice));
  uint32_t* dc = (uint32_t*)d_cand;
  SHZ_HIP(ctx, shz_memcpy(ctx, dc, A.cand_sid, cells * 4, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, dc + cells, A.cand_dlo, cells * 4, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, dc + 2 * cells, A.cand_dhi, cells * 4, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, shz_memcpy(ctx, dc + 3 * cells, A.cand_n, (uint64_t)nq_all * 4, hipMemcpyHostToDevice));
  exctl* ctl = (exctl*)d_ctl;
  uint32_t* d_qmax = (uint32_t*)((char*)d_ctl + 256);
  uint32_t* d_shift = d_qmax + nq_all;
  uint32_t* o = (uint32_t*)d_out;
  ex_cands C{dc, (const int32_t*)(dc + cells), (const int32_t*)(dc + 2 * cells), dc + 3 * cells, d_qmax,
             o, o + cells, o + 2 * cells, o + 3 * cells, o + 4 * cells, A.out_hist ? o + 5 * cells : nullptr, ncand,
             fit ? (unsigned long long*)((char*)d_out + fit_at) : nullptr};
  SHZ_HIP(ctx, hipMemsetAsync(d_out, 0, out_bytes, ctx->stream));
  SHZ_HIP(ctx, hipMemsetAsync(d_qmax, 0, (uint64_t)nq_all * 4, ctx->stream));
  hipLaunchKernelGGL(ex_init_kernel, dim3(nblk(cells)), dim3(256), 0, ctx->stream, C.q_first, C.t_first, cells);
  SHZ_HIP(ctx, hipGetLastError());
  uint32_t step = small ? EX_SMALL_Q_SUB : EX_MAX_Q_SUB;
  for (uint32_t q0 = 0; q0 < nq_all;) {
    uint32_t nq = std::min(step, nq_all - q0);
    // the elements stay sortable, and their (element, segment) slots countable in 32 bits
    while (nq > 1 && ((query_off[q0 + nq] - query_off[q0]) >= (1ull << 31) ||
                      (query_off[q0 + nq] - query_off[q0]) * nseg + 1 >= (1ull << 32)))
      nq /= 2;
    const uint64_t m = query_off[q0 + nq] - query_off[q0];
    if (m >= (1ull << 31) || m * nseg + 1 >= (1ull << 32))
      SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: query %u: %llu hashes x %u segments", who, q0, (unsigned long long)m, nseg);
    if (m == 0) { q0 += nq; continue; }
    const uint64_t bound = m * nseg + 1;
    void *c0, *c1, *fl, *ps, *lo, *rows, *po;
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_A, m * 8, &c0));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_SORT_B, m * 8, &c1));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M1, m * 4, &fl));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_M2, m * 4, &ps));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_LO, bound * 4, &lo));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_ROWS, bound * 8, &rows));
    SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_EX_PO, bound * 8, &po));
    SHZ_HIP(ctx, hipMemsetAsync(ctl, 0, sizeof(exctl), ctx->stream));
    hipLaunchKernelGGL(ex_compose_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, d_key32, d_q_off, (const uint64_t*)d_qoff + q0,
                       nq, m, (uint64_t*)c0, d_qmax + q0, &ctl->err);
    SHZ_HIP(ctx, hipGetLastError());
    int sel = 0;
    SHZ_TRY(shz_sort_u64(ctx, (uint64_t*)c0, (uint64_t*)c1, nullptr, nullptr, 0, m, 0, EX_QIDX_SHIFT + bits_for(nq - 1), &sel));
    const uint64_t* cs = sel ? (uint64_t*)c1 : (uint64_t*)c0;   // sorted
    uint64_t* E = sel ? (uint64_t*)c0 : (uint64_t*)c1;          // the distinct elements go to the other buffer
    hipLaunchKernelGGL(ex_flag_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, cs, m, (uint32_t*)fl);
    SHZ_TRY(shz_scan_u32(ctx, (const uint32_t*)fl, (uint32_t*)ps, m, (uint64_t*)&ctl->mu));
    hipLaunchKernelGGL(ex_compact_kernel, dim3(nblk(m)), dim3(256), 0, ctx->stream, cs, (const uint32_t*)fl, (const uint32_t*)ps, m, E);
    hipLaunchKernelGGL(ex_probe_kernel, dim3(nblk(bound)), dim3(256), 0, ctx->stream, (const uint64_t*)E, &ctl->mu, bound,
                       (const shz_seg_dev*)d_segs, nseg, (uint32_t*)lo, (uint64_t*)rows);
    SHZ_HIP(ctx, hipGetLastError());
    if (ctx->key_cap)   // (shz_set_key_cap: an element is a group of its own here, its slots hold rows)
      SHZ_TRY(shz_key_cap_apply(ctx, (uint64_t*)rows, nullptr, (const unsigned long long*)&ctl->mu, m, nseg, nullptr));
    SHZ_TRY(shz_scan_u64(ctx, (const uint64_t*)rows, (uint64_t*)po, bound, (uint64_t*)&ctl->P));
    exctl h;
    SHZ_HIP(ctx, shz_memcpy(ctx, &h, ctl, sizeof(exctl), hipMemcpyDeviceToHost));
    SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h.err) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: a query offset is >= 2^20", who);
    if (h.mu > m) SHZ_FAIL(ctx, SHZ_E_HIP, "%s: %llu distinct of %llu elements", who, h.mu, (unsigned long long)m);
    const uint64_t ntiles = (h.P + tile - 1) / tile;
    if (ntiles >= (1ull << 31)) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu pairs in one sub-batch", who, h.P);
    if (ntiles) {
      hipLaunchKernelGGL(fit ? ex_pairs_kernel<true> : ex_pairs_kernel<false>, dim3((unsigned)ntiles), dim3(256), 0, ctx->stream,
                         (const uint64_t*)E, (const uint64_t*)po, (const uint32_t*)lo, (uint32_t)(h.mu * nseg), nseg,
                         (const shz_seg_dev*)d_segs, (uint64_t)h.P, tile, sub_cap, q0, C);
      SHZ_HIP(ctx, hipGetLastError());
    }
    q0 += nq;
  }
  hipLaunchKernelGGL(ex_tail_kernel, dim3(nblk(std::max<uint64_t>(cells, nq_all))), dim3(256), 0, ctx->stream,
                     (const uint32_t*)C.count, C.q_first, C.t_first, cells, (const uint32_t*)d_qmax, nq_all, d_shift);
  SHZ_HIP(ctx, hipGetLastError());
  // the results travel to a block of this call first: a failed copy leaves the caller's arrays as they were
  std::vector<uint32_t> hres(cells * 5 + hist_words + nq_all);
  SHZ_HIP(ctx, shz_memcpy(ctx, hres.data(), d_out, (cells * 5 + hist_words) * 4, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, shz_memcpy(ctx, hres.data() + cells * 5 + hist_words, d_shift, (uint64_t)nq_all * 4, hipMemcpyDeviceToHost));
  std::vector<uint64_t> hfit(fit ? cells * 4 : 0);
  if (fit && cells) SHZ_HIP(ctx, shz_memcpy(ctx, hfit.data(), C.fit, cells * 32, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint32_t* outs[5] = {A.out_count, A.out_q_first, A.out_q_last, A.out_t_first, A.out_t_last};
  for (int k = 0; k < 5; ++k) memcpy(outs[k], hres.data() + cells * k, cells * 4);
  if (A.out_hist) memcpy(A.out_hist, hres.data() + cells * 5, hist_words * 4);
  memcpy(A.out_shift, hres.data() + cells * 5 + hist_words, (uint64_t)nq_all * 4);
  for (uint64_t i = 0; fit && i < cells; ++i) {
    A.out_sum_q[i] = hfit[4 * i];
    A.out_sum_u[i] = hfit[4 * i + 1];
    A.out_sum_qq[i] = hfit[4 * i + 2];
    A.out_sum_qu[i] = hfit[4 * i + 3];
  }
  return SHZ_OK;
}

// the host-array form, with the sums (shz_match_extents_fit) or without: A holds everything but the queries
static int32_t ex_host(shz_ctx* ctx, shz_table* t, const char* who, const uint32_t* key32, const uint32_t* q_off,
                       const uint64_t* query_off, const ex_args& A) {
  const uint32_t n_queries = A.n_queries;
  SHZ_TRY(ex_state(ctx, t, who, A.ncand));
  if (n_queries == 0) return SHZ_OK;
  if (!query_off) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: query_off is NULL", who);
  for (uint32_t q = 0; q < n_queries; ++q)
    if (query_off[q + 1] < query_off[q]) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: query_off decreases at query %u", who, q);
  const uint64_t h0 = query_off[0], h1 = query_off[n_queries];
  if (h1 > h0 && (!key32 || !q_off)) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: NULL column", who);
  SHZ_TRY(ex_check(ctx, t, who, A));
  for (uint64_t i = h0; i < h1; ++i)
    if (q_off[i] >> EX_QOFF_BITS) SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: query offset %u; offsets must be < 2^20", who, q_off[i]);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  // the columns of the queries, from their first hash on (the CSR moves with them)
  void *d_key, *d_qo;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_KEY, (h1 - h0) * 4, &d_key));
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_T1, (h1 - h0) * 4, &d_qo));
  if (h1 > h0) {
    SHZ_HIP(ctx, shz_memcpy(ctx, d_key, key32 + h0, (h1 - h0) * 4, hipMemcpyHostToDevice));
    SHZ_HIP(ctx, shz_memcpy(ctx, d_qo, q_off + h0, (h1 - h0) * 4, hipMemcpyHostToDevice));
  }
  std::vector<uint64_t> rel((size_t)n_queries + 1);
  for (uint32_t q = 0; q <= n_queries; ++q) rel[q] = query_off[q] - h0;
  const int32_t rc = ex_device(ctx, t, who, (const uint32_t*)d_key, (const uint32_t*)d_qo, rel.data(), A);
  if (rc != SHZ_OK) (void)hipStreamSynchronize(ctx->stream);
  return rc;
}

extern "C" int32_t shz_match_extents(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                     const uint64_t* query_off, uint32_t n_queries, uint32_t ncand, const uint32_t* cand_sid,
                                     const int32_t* cand_dlo, const int32_t* cand_dhi, const uint32_t* cand_n, uint32_t* out_count,
                                     uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first, uint32_t* out_t_last,
                                     uint32_t* out_hist, uint32_t* out_shift) {
  if (!ctx || !t) return SHZ_E_INVALID;
  const ex_args A{n_queries, ncand, cand_sid, cand_dlo, cand_dhi, cand_n, out_count, out_q_first, out_q_last, out_t_first,
                  out_t_last, out_hist, out_shift};
  return ex_host(ctx, t, "shz_match_extents", key32, q_off, query_off, A);
}

extern "C" int32_t shz_match_extents_fit(shz_ctx* ctx, shz_table* t, const uint32_t* key32, const uint32_t* q_off,
                                         const uint64_t* query_off, uint32_t n_queries, uint32_t ncand, const uint32_t* cand_sid,
                                         const int32_t* cand_dlo, const int32_t* cand_dhi, const uint32_t* cand_n,
                                         uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last, uint32_t* out_t_first,
                                         uint32_t* out_t_last, uint32_t* out_hist, uint32_t* out_shift, uint64_t* out_sum_q,
                                         uint64_t* out_sum_u, uint64_t* out_sum_qq, uint64_t* out_sum_qu) {
  if (!ctx || !t) return SHZ_E_INVALID;
  if (n_queries && (!out_sum_q || !out_sum_u || !out_sum_qq || !out_sum_qu))
    SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_match_extents_fit: NULL sum array");
  ex_args A{n_queries, ncand, cand_sid, cand_dlo, cand_dhi, cand_n, out_count, out_q_first, out_q_last, out_t_first,
            out_t_last, out_hist, out_shift};
  A.out_sum_q = out_sum_q;
  A.out_sum_u = out_sum_u;
  A.out_sum_qq = out_sum_qq;
  A.out_sum_qu = out_sum_qu;
  return ex_host(ctx, t, "shz_match_extents_fit", key32, q_off, query_off, A);
}

extern "C" int32_t shz_match_songs_extents(shz_ctx* ctx, shz_table* t, const uint32_t* sids, uint32_t n_sids, uint32_t ncand,
                                           const uint32_t* cand_sid, const int32_t* cand_dlo, const int32_t* cand_dhi,
                                           const uint32_t* cand_n, uint32_t* out_count, uint32_t* out_q_first, uint32_t* out_q_last,
                                           uint32_t* out_t_first, uint32_t* out_t_last, uint32_t* out_hist, uint32_t* out_shift) {
  if (!ctx || !t) return SHZ_E_INVALID;
  const char* who = "shz_match_songs_extents";
  SHZ_TRY(ex_state(ctx, t, who, ncand));
  if (n_sids == 0) return SHZ_OK;
  if (!sids) SHZ_FAIL(ctx, SHZ_E_INVALID, "%s: sids is NULL", who);
  const ex_args A{n_sids, ncand, cand_sid, cand_dlo, cand_dhi, cand_n, out_count, out_q_first, out_q_last, out_t_first,
                  out_t_last, out_hist, out_shift};
  SHZ_TRY(ex_check(ctx, t, who, A));
  // the listed songs' rows are the queries: counted, then gathered into columns of this call on the device (a song id listed
  // twice is refused by the count)
  std::vector<uint64_t> row_off((size_t)n_sids + 1);
  SHZ_TRY(shz_table_song_hashes(t, sids, n_sids, row_off.data(), nullptr, nullptr, 0, 0));
  const uint64_t total = row_off[n_sids];
  if (total >= (1ull << 32))
    SHZ_FAIL(ctx, SHZ_E_UNSUPPORTED, "%s: %llu rows in one call (limit 2^32 - 1); list fewer songs", who, (unsigned long long)total);
  own_bufs own;
  uint32_t *d_key = (uint32_t*)own.get(total * 4), *d_off = (uint32_t*)own.get(total * 4);
  if (!d_key || !d_off) SHZ_FAIL(ctx, SHZ_E_NOMEM, "%s: hipMalloc(2 x %llu) failed", who, (unsigned long long)(total * 4));
  if (total) SHZ_TRY(shz_table_song_hashes(t, sids, n_sids, row_off.data(), d_key, d_off, total, SHZ_SONGS_DEVICE_OUT));
  const int32_t rc = ex_device(ctx, t, who, d_key, d_off, row_off.data(), A);
  (void)hipStreamSynchronize(ctx->stream);   // (a refused call may have queued work that reads the columns)
  return rc;
}
