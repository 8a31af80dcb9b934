// fp32 peak picking + the fp64 verification of what fp32 cannot decide.  Included by shz_extract.hip.
//
// The reference's rule (__init__.py:143,161 on the array of :241): cell c is a peak <=> dB(P[c]) == dB(M) and
// dB(P[c]) > amp_min, M = the fp64 power maximum of the 21x21 window clipped to the clip.  Facts used, with
// key(x) = the bits of fp32(x) read as an integer (monotone in x for x >= 0):
//   (a) a dB tie needs P[c] within ~40 fp64 ulp of M, so key(P[c]) >= key(M) - 1;
//   (b) a cell whose key exceeds every other key of its window by more than 2 is M itself;
//   (c) key(M) is the maximum key of the window.
// peak_pick32 therefore emits (mask) the cells that hold the window's maximum key ALONE -- no other cell within 2 steps --
// and clear the threshold by a margin, and appends to a list every other cell whose key is within 1-2 steps of the
// maximum key.  peak_verify_kernel re-reads the window of a listed cell, and if more than one cell is within 2 steps of
// the maximum (or the threshold is close) recomputes those cells' fp64 power with stft_frame and applies the exact rule.
// Windows with more than PV_MAX_NEAR near-maximum cells (plateaus, flat spectra: ties across frames AND bins) mark
// their CLIP in a bitmap and raise XF_FALLBACK_CLIP: the host re-runs just those clips with the fp64 kernels
// (peak_pick_kernel<true>) and splices their entries into the batch's; every other clip of the batch is settled here.
// XF_FALLBACK (more undecided cells than the list holds) still sends the whole pass to fp64 staging.

#define P32_BH 7   // rows of a time block = rows of a load group; divides the segment lengths 42, 252 and 672
#define P32_OW 44  // output columns of a wave: its 64 columns less the 10 halo columns on either side
// predicate codes of the compare builtins that return the lane mask (__builtin_amdgcn_uicmp / sicmp / fcmpf)
enum { P32_OGE = 3, P32_UGE = 35, P32_SGE = 39 };

enum : uint32_t {
  XF_FALLBACK = 1u,   // fp32 staging cannot decide this input cheaply: rerun with fp64 staging
  XF_PEAK_CAP = 2u,   // a sub-batch had more peaks than its list holds
  XF_UND_CAP = 4u,    // more undecided cells than the list holds
  XF_FALLBACK_CLIP = 8u,  // some clips (bitmap behind the control block) need fp64 staging; the rest of the pass stands
};

// per-call control block on the device: everything the host used to read back between stages
struct xctl {
  unsigned long long peak_base;    // peaks written by earlier sub-batches
  unsigned long long hash_base;    // hashes written by earlier sub-batches
  unsigned long long sub_peaks;    // this sub-batch: scan total of the mask popcounts
  unsigned long long sub_hashes;   // this sub-batch: scan total of the partner counts
  unsigned long long max_sub_peaks;
  unsigned int und_count;          // undecided cells listed by peak_pick32 in this sub-batch
  unsigned int flags;              // XF_*
  unsigned long long und_total;    // statistics: undecided cells, cells that needed fp64, FFT frames recomputed
  unsigned long long und_f64;
  unsigned long long und_ffts;
};

// how mask words map to bins: word = (frame * n_slabs + slab) * nw + wave, bit = lane;
// bin = slab * sw + lane_stride * wave + lane - 10
struct mask_geom {
  uint32_t n_slabs, nw, lane_stride, sw;
};

__device__ __forceinline__ bool key_near(float p, float m, int d) { return __float_as_int(p) >= __float_as_int(m) - d; }

struct p32_args {
  const float* A;            // [frame][P32_STRIDE]
  const peak_seg* segs;
  uint32_t n_slabs, n_segs;
  float p_lo, p_hi;          // fp32 powers safely below / above the amp_min threshold
  uint64_t* mask;
  uint64_t* und_list;        // (frame << 12) | bin
  xctl* ctl;
  uint32_t und_cap;
  uint32_t* frame_cnt;       // peaks per frame (zeroed by the host): what the scan in front of peak_expand needs
};

// Block rule of non-maximum suppression (Neubeck and Van Gool 2006): the 21x21 window of a cell contains every cell at most
// 10 rows and 10 columns away, so a cell that is not within two key steps of the maximum of ANY set of such cells is neither
// a peak nor listed (both need key(cell) >= key(window maximum) - 2, see `hot` below).  Only the few cells that pass such a
// test get the window test; the others cost a select and a maximum.
// Workgroup = one wave = (clip segment, slab of P32_OW = 44 bins); lane l holds slab column l - 10, lanes 10..53 are the
// output columns.  Waves share nothing: no LDS memory, no barrier; the 20 halo columns are re-read (through L2).
// Blocks: P32_BH = 7 rows (the load group; divides 42, 252, 672, and blocks start at the segment's first frame) by a
// SLIDING 21 columns centred on the lane, not an aligned 8 or 16: the window of a cell in rows 7k..7k+6 holds those 7 rows
// of its 21 columns whole, and so does it hold block k-1 for the block's rows 0..3 and block k+1 for rows 3..6.  So
//   bm = the lane's column maximum over a block (3 max3), hm = the maximum of bm over lanes l-10..l+10 (once per block:
//   doubling, 7 lane permutes + 5 max), and a cell of block k goes on only if its key >= key(max(hm[k], hm[k-+1])) - 2:
// one compare per stored row, taken as a lane mask, a wave-uniform branch.  That is a test against 14 x 21 = 294 cells; about
// one row in seven has a lane that passes (0.85 rows a block on noise), where aligned 7 x 8 blocks would pass eight cells
// per seven rows.
// A row that goes on is decided once block k+2 is complete (its window reaches row 7k+16), from the rows of blocks
// k-2..k+2, which stay in registers (5 x 7; the five blocks rotate through five unrolled phases, so nothing is moved):
// mx = the row maximum without the centre (20 neighbouring lanes), co = the lane's column maximum over the window's other
// 20 rows (10 max3), t2 = the maximum of co over the 21 lanes = the largest of the other rows' maxima, t1 = max(mx, centre,
// t2) = the window maximum; then the tests of the rule above, as before: alone at the top by more than 2 steps and > p_hi:
// mask bit and frame_cnt; within a step of the maximum and >= p_lo but not alone: undecided list.
// Lane permutes are ds_bpermute_b32: they use the LDS crossbar but no LDS memory, and only once per block and per row
// that goes on, never per row.
// The mask buffer is zeroed by the host; only non-zero words are written.
// The loads of the next group of P32_BH rows are in flight while a group is worked on: every group issues exactly P32_BH
// loads, without a branch (a row outside the segment and its halo is a re-read of the nearest row inside, a column outside
// the spectrum a re-read of column 0; the value is replaced by -inf where the group is CONSUMED), so the wait in front of a
// group's rows is vmcnt(P32_BH), the loads just issued staying in flight.  (With each load behind its own `if (tn < hi)`
// the count was unknown to the compiler and the wait was vmcnt(0) right behind the loads: DESIGN.md 3.2.)
template <int PH> struct p32_phase { static constexpr int value = PH; };

template <int NW, int OCC>
__global__ __launch_bounds__(64 * NW, OCC) void peak_pick32_kernel(p32_args a) {
  static_assert(NW == 1, "waves share nothing: one wave per workgroup, one mask word per slab");
  constexpr int BH = P32_BH, SW = P32_OW;
  // XCD-aware work map (a speed choice only): workgroups b, b+8, b+16, ... share an XCD and its L2 (round-robin
  // dispatch), so the n_slabs slabs of one segment are given to consecutive workgroups of ONE XCD: the 20 halo columns
  // neighbouring slabs share are then read from HBM once, not once per XCD.
  const uint32_t b = blockIdx.x, per_xcd = (a.n_segs + 7) >> 3;
  const uint32_t seg_i = (b >> 3) / a.n_slabs * 8 + (b & 7);
  const uint32_t slab = (b >> 3) % a.n_slabs;
  if ((b >> 3) / a.n_slabs >= per_xcd || seg_i >= a.n_segs) return;   // uniform: before any barrier
  const peak_seg sg = a.segs[seg_i];
  const int lane = threadIdx.x;
  const float NEG = -__builtin_inff();
  const int col = (int)slab * SW - 10 + lane;
  const bool loads = col >= 0 && col < SHZ_NBINS;
  const bool is_out = lane >= 10 && lane < 10 + SW && col < SHZ_NBINS;  // window = lanes lane-10 .. lane+10
  const uint64_t out_m = __builtin_amdgcn_ballot_w64(is_out);     // the wave's output lanes as a scalar mask
  const int t0 = (int)sg.t0, t1 = (int)sg.t1;
  const int lo = t0 - 10 > 0 ? t0 - 10 : 0;
  const int hi = (int)(sg.t1 + 10 < sg.nframes ? sg.t1 + 10 : sg.nframes);
  const uint32_t boff = loads ? (uint32_t)col * 4u : 0u;         // byte offset in a row (a lane outside the spectrum: column 0)
  const float* base = a.A + (uint64_t)sg.gframe0 * P32_STRIDE;   // uniform; rows are added as uniform offsets
  // the value of lane + d (mod 64) by ds_bpermute_b32: the byte address of the source lane's register
  auto lane_at = [&](int d) { return ((lane + d) & 63) << 2; };
  const int a1 = lane_at(1), a2 = lane_at(2), a4 = lane_at(4), a6 = lane_at(6), a8 = lane_at(8), a9 = lane_at(9),
            a10 = lane_at(10), am2 = lane_at(-2), am10 = lane_at(-10);
  auto from = [](int addr, float v) { return __int_as_float(__builtin_amdgcn_ds_bpermute(addr, __float_as_int(v))); };
  // maximum over lanes l-10 .. l+10 (true for lanes 10..53, whose 21 lanes exist): x[l-10..l+5], x[l+6..l+9], x[l+10]
  auto max21 = [&](float x) {
    const float w2 = fmaxf(x, from(a1, x)), w4 = fmaxf(w2, from(a2, w2)), w8 = fmaxf(w4, from(a4, w4));
    const float w16 = fmaxf(w8, from(a8, w8));
    return fmaxf(fmaxf(from(am10, w16), from(a6, w4)), from(a10, x));
  };
  // the same without lane l itself: x[l-10..l-3], x[l-2..l-1] | x[l+1..l+8], x[l+9..l+10]
  auto max20 = [&](float x) {
    const float w2 = fmaxf(x, from(a1, x)), w4 = fmaxf(w2, from(a2, w2)), w8 = fmaxf(w4, from(a4, w4));
    return fmaxf(fmaxf(from(am10, w8), from(am2, w2)), fmaxf(from(a1, w8), from(a9, w2)));
  };

  // R[b]: the rows of a block; five blocks rotate through the five slots.  hm[b]: see the header
  float R[5][BH], hm[5], pre[BH];
#pragma unroll
  for (int b5 = 0; b5 < 5; ++b5) {
    hm[b5] = NEG;
#pragma unroll
    for (int i = 0; i < BH; ++i) R[b5][i] = NEG;
  }
  // row t of the segment's clip, clamped to the rows the segment reads (hi > lo >= 0): the segment's first row as the uniform
  // base, and one 32-bit offset per lane = the lane's byte offset in a row + the row's distance from that base (a segment
  // and its halo: at most PK_SEG_LONG + 20 rows of 8,256 bytes, asserted where the segments are cut).  The load is the
  // scalar-base form, global_load_dword v, v_off, s[base]; a row costs min, subtract, multiply (scalar) and one 32-bit add
  // (the compiler's own address was a 64-bit multiply-add per row and lane)
  typedef __attribute__((address_space(1))) const char gchar;
  typedef __attribute__((address_space(1))) const float gfloat;
  gchar* const row0 = (gchar*)(base + (uint64_t)(uint32_t)lo * P32_STRIDE);
  auto row_load = [&](int t) {
    const uint32_t roff = (uint32_t)(min(max(t, lo), hi - 1) - lo) * (uint32_t)(P32_STRIDE * sizeof(float));
    return *(gfloat*)(row0 + (boff + roff));
  };
  // Blocks are counted from the segment's first frame: block k = rows t0 + 7k .. t0 + 7k + 6, k = -2 (its rows t0-10..t0-8
  // are the first a window reaches) .. n_blk + 1.  Step s consumes block s - 2 and decides the rows of block s - 4.
  const int n_blk = (t1 - t0 + BH - 1) / BH, n_steps = n_blk + 4;
#pragma unroll
  for (int p = 0; p < BH; ++p) pre[p] = row_load(t0 - 2 * BH + p);

  // one step; PH = s mod 5 at compile time, so that block s - d lives in slot (PH - d) mod 5 and no row is ever moved
  auto step = [&](auto ph, const int s) {
    constexpr int PH = decltype(ph)::value;
    constexpr int S0 = PH, S1 = (PH + 4) % 5, S2 = (PH + 3) % 5, S3 = (PH + 2) % 5, S4 = (PH + 1) % 5;  // blocks s, s-1, .. s-4
    const int tb = t0 + (s - 2) * BH;   // first row of the block consumed
    // the rows one group ahead: exactly BH loads, no branch, nothing done with the values in this step
    float nxt[BH];
#pragma unroll
    for (int i = 0; i < BH; ++i) nxt[i] = row_load(tb + BH + i);
    __builtin_amdgcn_sched_barrier(0);  // issued BEFORE the wait for this block's rows: that wait is then vmcnt(BH)
    // the block's rows as loaded one step ago; what the segment does not read (row outside [lo, hi), column outside the
    // spectrum) becomes -inf here, where the value is first needed, by one select on a lane mask made of scalars.
    // Which rows exist: one scalar word per block, one bit test per row
    const int v_lo = max(lo - tb, 0), v_hi = min(hi - tb, BH);
    const uint32_t row_bits = v_hi > v_lo ? ((1u << (v_hi - v_lo)) - 1u) << v_lo : 0u;
#pragma unroll
    for (int i = 0; i < BH; ++i) {
      R[S0][i] = (loads && ((row_bits >> i) & 1u)) ? pre[i] : NEG;
      pre[i] = nxt[i];
    }
    const float bm = fmaxf(fmaxf(fmaxf(R[S0][0], R[S0][1]), fmaxf(R[S0][2], R[S0][3])),
                           fmaxf(fmaxf(R[S0][4], R[S0][5]), R[S0][6]));
    static_assert(BH == 7, "the block maximum and the thresholds below are written for 7 rows");
    hm[S0] = max21(bm);
    if (s < 4) return;   // uniform
    // block k = s - 4 in slot S2, k-1 in S3 (whole inside the window of rows 0..3), k+1 in S1 (rows 3..6)
    const int tk = t0 + (s - 4) * BH;
    const uint32_t seg_bits = (1u << min(t1 - tk, BH)) - 1u;   // rows of the block inside the segment (t1 > tk: s < n_steps)
    const int k_lo = __float_as_int(fmaxf(hm[S2], hm[S3])) - 2, k_hi = __float_as_int(fmaxf(hm[S2], hm[S1])) - 2;
    const int k_mid = max(k_lo, k_hi);
#pragma unroll
    for (int i = 0; i < BH; ++i) {
      const float c = R[S2][i];
      const uint64_t cand = !((seg_bits >> i) & 1u)
                                ? 0ull
                                : out_m & __builtin_amdgcn_sicmp(__float_as_int(c), i < 3 ? k_lo : i > 3 ? k_hi : k_mid, P32_SGE);
      if (!cand) continue;   // wave-uniform: no lane of this row is within two steps of its 14 x 21 cells' maximum
      const int tc = tk + i;
      // the centre in its row: e >= 5 alone at the top, >= 2 holds the row maximum, >= 1 within one step of it
      const float mx = max20(c), c1 = fmaxf(mx, c);
      int e = __float_as_int(c) - __float_as_int(mx) + 2;
      const uint32_t q = (uint32_t)min(max(e, 0), 5);
      // the lane's column over the window's other rows tc-10 .. tc+10: rows i+d of block k, which are row (i+d) mod 7 of a
      // neighbouring block where i+d leaves 0..6
      float co = NEG;
#pragma unroll
      for (int d = -10; d <= 10; ++d) {
        if (d == 0) continue;
        const int r = i + d + 2 * BH, bq = r / BH, br = r % BH;   // bq: 0 = block k-2 .. 4 = block k+2
        co = fmaxf(co, bq == 0 ? R[S4][br] : bq == 1 ? R[S3][br] : bq == 2 ? R[S2][br] : bq == 3 ? R[S1][br] : R[S0][br]);
      }
      const float t2 = max21(co);          // largest row maximum of the window's other rows
      const float w1 = fmaxf(c1, t2);      // the window's maximum
      // hot <=> in_seg && is_out && q >= 1 && key_near(c1, w1, 1) && w1 >= p_lo, kept as the lane MASK the compares
      // deliver (a ballot of a bool made of several compares goes through a 0/1 register and a compare with zero)
      const uint64_t hot = out_m & __builtin_amdgcn_uicmp(q, 1u, P32_UGE) &
                           __builtin_amdgcn_sicmp(__float_as_int(c1), __float_as_int(w1) - 1, P32_SGE) &
                           __builtin_amdgcn_fcmpf(w1, a.p_lo, P32_OGE);
      if (hot) {  // wave-uniform: some lane's centre is within one step of its window maximum
        const bool exact = q >= 2u && c1 == w1;
        const bool uniq = q == 5u && !key_near(t2, w1, 2);
        const bool hot_l = (hot >> lane) & 1ull;
        const bool pk = hot_l && exact && uniq && w1 > a.p_hi;
        const bool und = hot_l && !pk;
        const unsigned long long bal = __builtin_amdgcn_ballot_w64(pk);
        if (bal && lane == 0) {
          a.mask[(uint64_t)(sg.gframe0 + tc) * a.n_slabs + slab] = bal;
          atomicAdd(&a.frame_cnt[sg.gframe0 + tc], (uint32_t)__popcll(bal));
        }
        if (und) {
          const uint32_t idx = atomicAdd(&a.ctl->und_count, 1u);
          if (idx < a.und_cap) a.und_list[idx] = ((uint64_t)(sg.gframe0 + tc) << 12) | (uint32_t)col;
        }
      }
    }
  };
  for (int s = 0; s < n_steps; s += 5) {
    step(p32_phase<0>{}, s);
    if (s + 1 < n_steps) step(p32_phase<1>{}, s + 1);
    if (s + 2 < n_steps) step(p32_phase<2>{}, s + 2);
    if (s + 3 < n_steps) step(p32_phase<3>{}, s + 3);
    if (s + 4 < n_steps) step(p32_phase<4>{}, s + 4);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// peak_verify: one workgroup (256 threads) per listed cell, grid-stride over the list.
#define PV_MAX_NEAR 32

struct verify_args {
  stft_args st;              // PCM + clip tables + FFT constants (out unused)
  const float* A;            // fp32 staged power
  uint64_t* mask;
  uint32_t* frame_cnt;       // peaks per frame, kept in step with the mask
  mask_geom mg;
  const uint64_t* und_list;
  xctl* ctl;
  uint32_t und_cap;
  float p_hi32;              // fp32 power safely above the threshold
  double p_lo, p_hi, amp_min;  // fp64 threshold band and the exact threshold
  uint32_t* fb_clips;        // bitmap over the CALL's clips: clips whose windows hold too many tied cells for this kernel
  uint32_t clip0;            // the call's index of this sub-batch's clip 0
};

__global__ __launch_bounds__(256, 2) void peak_verify_kernel(verify_args a) {
  __shared__ cplx lds[SHZ_NFFT];   // one frame's transform, numpy's arithmetic (np_fft4096)
  __shared__ int s_max[4], s_cnt, s_cell[PV_MAX_NEAR];
  __shared__ double s_p[PV_MAX_NEAR];
  __shared__ uint32_t s_clip, s_stop, s_skip;
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const uint32_t n = min(a.ctl->und_count, a.und_cap);
  if (blockIdx.x >= n) return;
  double2 ww[8];
#pragma unroll
  for (int t = 0; t < 8; ++t) ww[t] = *reinterpret_cast<const double2*>(a.st.np_window + 2 * (j + 256 * t));
  // The workgroup's entries (blockIdx.x, + gridDim.x, ...) are looked at 256 at a time: every thread reads one entry, finds
  // its clip and tests the clip's bit; entries of clips already marked for the fp64 re-run are dropped here, 256 per
  // round trip, instead of one per barrier pair below (a click-per-hop clip lists ~500,000 cells: 3.9 ms -> see DESIGN 3.2).
  __shared__ uint64_t s_ent[256];
  __shared__ uint32_t s_eclip[256], s_keep[256];
  bool stop = false;
  for (uint32_t k0 = 0; !stop && blockIdx.x + (uint64_t)k0 * gridDim.x < n; k0 += 256) {
    {
      const uint64_t e = blockIdx.x + (uint64_t)(k0 + j) * gridDim.x;
      uint32_t keep = 0;
      if (e < n) {
        const uint64_t ent = a.und_list[e];
        const uint32_t g = (uint32_t)(ent >> 12);
        uint32_t lo = 0, hi = a.st.n_clips;
        while (hi - lo > 1) {
          uint32_t mid = (lo + hi) >> 1;
          if (a.st.clip_foff[mid] <= g) lo = mid; else hi = mid;
        }
        const uint32_t gc = a.clip0 + lo;
        keep = ((__hip_atomic_load(&a.fb_clips[gc >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (gc & 31)) & 1u) ^ 1u;
        s_ent[j] = ent;
        s_eclip[j] = lo;
      }
      s_keep[j] = keep;
    }
    __syncthreads();
  for (int te = 0; te < 256; ++te) {
    if (!s_keep[te]) continue;   // uniform
    const uint64_t ent = s_ent[te];
    const uint32_t g = (uint32_t)(ent >> 12);
    const int bin = (int)(ent & 0xFFF);
    if (j == 0) {
      const uint32_t lo = s_eclip[te];
      s_clip = lo;
      s_cnt = 0;
      // the pass is going to be repeated with fp64 staging anyway: stop (read by one thread, so that the whole
      // workgroup takes the same branch around the barriers below)
      s_stop = __hip_atomic_load(&a.ctl->flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & XF_FALLBACK;
      // a clip that is going to be redone with fp64 staging: its cells need no answer here
      const uint32_t gc = a.clip0 + lo;
      s_skip = (__hip_atomic_load(&a.fb_clips[gc >> 5], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (gc & 31)) & 1u;
    }
    __syncthreads();
    if (s_stop) { stop = true; break; }
    if (s_skip) { __syncthreads(); continue; }
    const uint32_t clip = s_clip;
    const int f0 = (int)a.st.clip_foff[clip], F = (int)a.st.clip_foff[clip + 1] - f0, t = (int)g - f0;
    // the 441 cells of the window: cell id = (dt + 10) * 21 + (df + 10); threads 0..220 take two cells
    int key[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int id = j + 256 * h;
      const int dt = id / 21 - 10, df = id % 21 - 10;
      const bool valid = id < 441 && t + dt >= 0 && t + dt < F && bin + df >= 0 && bin + df < SHZ_NBINS;
      key[h] = valid ? __float_as_int(a.A[(uint64_t)(g + dt) * P32_STRIDE + bin + df]) : INT32_MIN;
    }
    int mk = max(key[0], key[1]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mk = max(mk, __shfl_xor(mk, d, 64));
    if (lane == 0) s_max[wave] = mk;
    __syncthreads();
    mk = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
#pragma unroll
    for (int h = 0; h < 2; ++h)
      if (key[h] >= mk - 2) {
        const int q = atomicAdd(&s_cnt, 1);
        if (q < PV_MAX_NEAR) s_cell[q] = j + 256 * h;
      }
    __syncthreads();
    const int n_near = s_cnt;
    const int key_c = __float_as_int(a.A[(uint64_t)g * P32_STRIDE + bin]);
    bool decided = false, pk = false;
    if (key_c < mk - 2) decided = true;                                              // cannot tie with M in dB
    else if (n_near == 1 && __int_as_float(mk) > a.p_hi32) { decided = true; pk = true; }  // alone at the top, clear of the threshold
    else if (n_near > PV_MAX_NEAR) {
      decided = true;
      if (j == 0) {
        const uint32_t gc = a.clip0 + clip;
        atomicOr(&a.fb_clips[gc >> 5], 1u << (gc & 31));
        atomicOr(&a.ctl->flags, XF_FALLBACK_CLIP);
      }
    }
    if (!decided) {
      // fp64 power of the near-maximum cells, by the arithmetic of the REFERENCE (numpy's transform, np_fft4096): one FFT
      // per FRAME that holds any of them (a stationary partial ties across the 21 frames of the window in one bin: 21
      // cells, 21 frames)
      uint32_t n_ffts = 0;
      for (int dt = -10; dt <= 10; ++dt) {
        bool any = false;   // uniform: s_cell is shared
        for (int q = 0; q < n_near; ++q) any |= (s_cell[q] / 21 - 10) == dt;
        if (!any) continue;
        ++n_ffts;
        int pw[8];
        stft_load_frame(a.st, clip, g + dt, j, pw);
        np_stage_frame(lds, pw, ww, j);
        __syncthreads();
        np_fft4096(lds, a.st.np_comp, j);
        if (j < n_near && s_cell[j] / 21 - 10 == dt) {
          const int k = bin + s_cell[j] % 21 - 10;
          s_p[j] = stage_value<double>(np_power(lds[k], k, a.st.r_fs, a.st.r_s, a.st.np_unfused));
        }
        __syncthreads();   // lds is rewritten by the next frame
      }
      if (j == 0) atomicAdd(&a.ctl->und_ffts, (unsigned long long)n_ffts);
      __syncthreads();
      if (j == 0) {
        double M = s_p[0], pc = 0.0;
        for (int q = 0; q < n_near; ++q) {
          M = fmax(M, s_p[q]);
          if (s_cell[q] == 220) pc = s_p[q];  // the centre (dt = df = 0)
        }
        pk = (pc == M || db_equal(pc, M)) && (M > a.p_hi || (M > a.p_lo && db_above(M, a.amp_min)));
        atomicAdd(&a.ctl->und_f64, 1ull);
      }
    }
    if (j == 0) {
      if (pk) {
        const uint32_t slab = (uint32_t)bin / a.mg.sw;
        const uint32_t lic = (uint32_t)bin - slab * a.mg.sw + 10;
        // the wave that OWNS the column (a wave's lanes reach past lane_stride where the next wave or slab takes over)
        const uint32_t wv = min(lic / a.mg.lane_stride, a.mg.nw - 1u), ln = lic - wv * a.mg.lane_stride;
        const unsigned long long was = atomicOr((unsigned long long*)&a.mask[((uint64_t)g * a.mg.n_slabs + slab) * a.mg.nw + wv], 1ull << ln);
        if (!((was >> ln) & 1ull)) atomicAdd(&a.frame_cnt[g], 1u);
      }
      atomicAdd(&a.ctl->und_total, 1ull);
    }
    __syncthreads();  // s_* are rewritten by the next entry
  }
    __syncthreads();  // s_ent / s_keep are rewritten by the next round
  }
}
