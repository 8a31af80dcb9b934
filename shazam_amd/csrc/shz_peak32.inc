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

#define P32_PF 7  // frames per barrier group (3 groups = one van Herk block of 21)
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
__device__ __forceinline__ float f_wave_shl1(float v) {  // value of lane + 1 (lane 63: unspecified)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130 /* wave_shl:1 */, 0xF, 0xF, false));
}

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

// Workgroup = NW waves = (clip segment, slab of SW = 61 NW - 17 bins); wave w, lane l holds slab column 61 w + l
// (lanes 61..63 repeat lanes 0..2 of the next wave, so pair and quad maxima come from DPP wave shifts).
// Frequency direction through LDS: rows of pair maxima r2[i] = max(x[i], x[i+1]) and quad maxima r4[i] = max(x[i..i+3]);
// the 20 neighbours of column c in its row are r4[c-10], r4[c-6], r2[c-2] | r2[c+1], r4[c+3], r4[c+7]: six 4-byte reads
// give the row maximum WITHOUT the centre (mx), and e = key(centre) - key(mx) classifies the centre in its row:
// e >= 3 alone at the top, e >= 0 holds the maximum, e >= -1 within one step of it (3 bits per row, packed).
// Time direction: van Herk / Gil-Werman on blocks of 21 frames (prefix maximum R1 of the current block, suffix maxima S1
// of the previous one: 2 max per frame); the row maxima of both blocks stay in registers (cur, prev), so a wave that
// finds a lane whose centre is within one step of its window maximum -- one wave-row in eight -- can work out there and
// then whether that lane is alone (second-largest row maximum of the window, 20 max) or has to be listed.
// The mask buffer is zeroed by the host; only non-zero words are written.
// The loads of the next group of P32_PF rows are in flight while a group is worked on: every group issues exactly P32_PF
// loads, without a branch (a row past the segment's last is a re-read of the last, a column outside the spectrum a re-read
// of column 0; the value is replaced by -inf where the group is CONSUMED), so the wait in front of a group's rows is
// vmcnt(P32_PF), the loads just issued staying in flight.  (With each load behind its own `if (tn < hi)` the count was
// unknown to the compiler and the wait was vmcnt(0) right behind the loads in two groups of three: DESIGN.md 3.2.)
// Two groups ahead (14 rows in flight per lane) was measured in round 4 on 644,000 frames, with those vmcnt(0) waits:
// 2.13 ms -> 2.38 at 4 waves per SIMD (the 7 extra registers spill) and 2.41 at 3.
template <int NW, int OCC>
__global__ __launch_bounds__(64 * NW, OCC) void peak_pick32_kernel(p32_args a) {
  constexpr int TH = 64 * NW, SW = 61 * NW - 17;
  // lanes 61..63 of a wave hold no column of their own (their pair / quad maxima are the next wave's): they store into a
  // dump column behind the row instead of being masked off row by row
  constexpr int TW = TH + 64;
  __shared__ float r2[P32_PF][TW];
  __shared__ float r4[P32_PF][TW];
  // XCD-aware work map (a speed choice only): workgroups b, b+8, b+16, ... share an XCD and its L2 (round-robin
  // dispatch), so the n_slabs slabs of one segment are given to consecutive workgroups of ONE XCD: the 20 halo columns
  // neighbouring slabs share are then read from HBM once, not once per XCD.
  const uint32_t b = blockIdx.x, per_xcd = (a.n_segs + 7) >> 3;
  const uint32_t seg_i = (b >> 3) / a.n_slabs * 8 + (b & 7);
  const uint32_t slab = (b >> 3) % a.n_slabs;
  if ((b >> 3) / a.n_slabs >= per_xcd || seg_i >= a.n_segs) return;   // uniform: before any barrier
  const peak_seg sg = a.segs[seg_i];
  const int j = threadIdx.x, lane = j & 63, wave = j >> 6;
  const float NEG = -__builtin_inff();
  const int li = 61 * wave + lane;                               // LDS column = bin - (slab*SW - 10)
  const int col = (int)slab * SW - 10 + li;
  const bool loads = col >= 0 && col < SHZ_NBINS;
  const bool owns = lane < 61 && li >= 10 && li <= 61 * NW - 8;  // output column li (window = LDS columns li-10 .. li+10)
  const bool is_out = owns && col < SHZ_NBINS;
  const uint64_t out_m = __builtin_amdgcn_ballot_w64(is_out);     // the wave's output lanes as a scalar mask
  const int lo = (int)sg.t0 - 10 > 0 ? (int)sg.t0 - 10 : 0;
  const int hi = (int)(sg.t1 + 10 < sg.nframes ? sg.t1 + 10 : sg.nframes);
  const int end = (int)sg.t1 + 10;  // last iteration decides frame t1-1
  const uint32_t boff = loads ? (uint32_t)col * 4u : 0u;         // byte offset in a row (a lane outside the spectrum: column 0)
  const float* base = a.A + (uint64_t)sg.gframe0 * P32_STRIDE;   // uniform; rows are added as uniform offsets
  const int o = owns ? li - 10 : 0;                              // other lanes read columns 0..17: valid, ignored
  const int wcol = lane < 61 ? li : TH + lane;                   // where this lane stores its row values

  float S1[21], cur[21], prev[21], pre[P32_PF];
  uint32_t qc[3] = {0, 0, 0}, qp[3] = {0, 0, 0};  // 3-bit row classes of the current / previous block, 7 rows per word
  float R1 = NEG;
#pragma unroll
  for (int u = 0; u < 21; ++u) { S1[u] = NEG; prev[u] = NEG; cur[u] = NEG; }
  // row t of the segment's clip, clamped to the last row that exists (hi > lo >= 0): the segment's first row as the uniform
  // base, and one 32-bit offset per lane = the lane's byte offset in a row + the row's distance from that base (a segment
  // and its halo: at most PK_SEG_LONG + 20 rows of 8,256 bytes, asserted where the segments are cut).  The load is the
  // scalar-base form, global_load_dword v, v_off, s[base]; a row costs min, subtract, multiply (scalar) and one 32-bit add
  // (the compiler's own address was a 64-bit multiply-add per row and lane)
  typedef __attribute__((address_space(1))) const char gchar;
  typedef __attribute__((address_space(1))) const float gfloat;
  gchar* const row0 = (gchar*)(base + (uint64_t)(uint32_t)lo * P32_STRIDE);
  auto row_load = [&](int t) {
    const uint32_t roff = (uint32_t)(min(t, hi - 1) - lo) * (uint32_t)(P32_STRIDE * sizeof(float));
    return *(gfloat*)(row0 + (boff + roff));
  };
#pragma unroll
  for (int p = 0; p < P32_PF; ++p) pre[p] = row_load(lo + p);
  for (int tb = lo; tb < end; tb += 21) {
    // which of the block's 21 centre frames tb - 10 + u lie inside the segment: one scalar word per block, one bit test per
    // row (the two compares and the mask logic per row were a third of the scalar instructions of this loop)
    const int c_lo = max((int)sg.t0 - (tb - 10), 0), c_hi = min((int)sg.t1 - (tb - 10), 21);
    const uint32_t seg_bits = c_hi > c_lo ? ((1u << (c_hi - c_lo)) - 1u) << c_lo : 0u;
#pragma unroll
    for (int g3 = 0; g3 < 21 / P32_PF; ++g3) {
      float v[P32_PF], mx[P32_PF];
      // the frames one group ahead: exactly P32_PF loads, no branch, nothing done with the values in this group
      float nxt[P32_PF];
#pragma unroll
      for (int i = 0; i < P32_PF; ++i) nxt[i] = row_load(tb + P32_PF * (g3 + 1) + i);
      __builtin_amdgcn_sched_barrier(0);  // issued BEFORE the wait for this group's rows: that wait is then vmcnt(P32_PF)
      // the group's rows as loaded one group ago; what does not exist (row past the segment, column outside the spectrum)
      // becomes -inf here, where the value is first needed, by one select on a lane mask made of scalars
#pragma unroll
      for (int i = 0; i < P32_PF; ++i) {
        v[i] = (loads && tb + P32_PF * g3 + i < hi) ? pre[i] : NEG;
        pre[i] = nxt[i];
      }
      __syncthreads();  // every wave is done reading the previous group's rows
#pragma unroll
      for (int i = 0; i < P32_PF; ++i) {
        const float p2 = fmaxf(v[i], f_wave_shl1(v[i]));                 // columns li, li+1     (valid: lane < 63)
        const float p4 = fmaxf(p2, f_wave_shl1(f_wave_shl1(p2)));        // columns li .. li+3   (valid: lane < 61)
        r2[i][wcol] = p2; r4[i][wcol] = p4;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < P32_PF; ++i) {
        const float l = fmaxf(fmaxf(r4[i][o], r4[i][o + 4]), r2[i][o + 8]);
        const float r = fmaxf(fmaxf(r4[i][o + 13], r4[i][o + 17]), r2[i][o + 11]);
        mx[i] = fmaxf(l, r);
      }
      uint32_t qw = 0;
      // time direction (registers only)
#pragma unroll
      for (int i = 0; i < P32_PF; ++i) {
        const int u = P32_PF * g3 + i;
        const int t = tb + u;
        const float m = fmaxf(mx[i], v[i]);
        int e = __float_as_int(v[i]) - __float_as_int(mx[i]) + 2;   // >= 5 alone, >= 2 holds the row maximum, >= 1 near it
        e = min(max(e, 0), 5);
        qw |= (uint32_t)e << (3 * i);
        if (i == P32_PF - 1) qc[g3] = qw;
        R1 = (u == 0) ? m : fmaxf(R1, m);
        cur[u] = m;
        const float t1 = (u < 20) ? fmaxf(S1[(u + 1) % 21], R1) : R1;
        // centre frame t - 10: position u-10 of the current block or u+11 of the previous one
        const int kc = (u + 11) % 21;
        const float c1 = (u >= 10) ? cur[kc] : prev[kc];
        // class word of the centre row (the current group's word is still being assembled in qw)
        const uint32_t cw = (u >= 10) ? ((kc / P32_PF == g3) ? qw : qc[kc / P32_PF]) : qp[kc / P32_PF];
        const uint32_t q = (cw >> (3 * (kc % P32_PF))) & 7u;
        const int tc = t - 10;
        const bool in_seg = (seg_bits >> u) & 1u;
        // hot <=> in_seg && is_out && q >= 1 && key_near(c1, t1, 1) && t1 >= p_lo, kept as the lane MASK the compares
        // deliver (a ballot of a bool made of several compares goes through a 0/1 register and a compare with zero)
        const int kt1 = __float_as_int(t1);
        const uint64_t hot = !in_seg ? 0ull
                                     : out_m & __builtin_amdgcn_uicmp(q, 1u, P32_UGE) &
                                           __builtin_amdgcn_sicmp(__float_as_int(c1), kt1 - 1, P32_SGE) &
                                           __builtin_amdgcn_fcmpf(t1, a.p_lo, P32_OGE);
        if (hot) {  // wave-uniform: some lane's centre is within one step of its window maximum
          float t2 = NEG;     // largest row maximum of the window's other rows
#pragma unroll
          for (int k = 0; k < 21; ++k) {
            if (k == kc) continue;
            const bool in_cur = k <= u;  // window rows: cur[0..u] and prev[u+1..20]
            t2 = fmaxf(t2, in_cur ? cur[k] : prev[k]);
          }
          const bool exact = q >= 2u && c1 == t1;
          const bool uniq = q == 5u && !key_near(t2, t1, 2);
          const bool hot_l = (hot >> lane) & 1ull;
          const bool pk = hot_l && exact && uniq && t1 > a.p_hi;
          const bool und = hot_l && !pk;
          const unsigned long long bal = __builtin_amdgcn_ballot_w64(pk);
          if (bal && lane == 0) {
            a.mask[((uint64_t)(sg.gframe0 + tc) * a.n_slabs + slab) * NW + wave] = bal;
            atomicAdd(&a.frame_cnt[sg.gframe0 + tc], (uint32_t)__popcll(bal));
          }
          if (und) {
            const uint32_t idx = atomicAdd(&a.ctl->und_count, 1u);
            if (idx < a.und_cap) a.und_list[idx] = ((uint64_t)(sg.gframe0 + tc) << 12) | (uint32_t)col;
          }
        }
        if (u == 20) {  // block complete: it becomes the previous one; suffix maxima
          qp[0] = qc[0]; qp[1] = qc[1]; qp[2] = qc[2];
#pragma unroll
          for (int k = 0; k < 21; ++k) prev[k] = cur[k];
          S1[20] = cur[20];
#pragma unroll
          for (int k = 19; k >= 0; --k) S1[k] = fmaxf(cur[k], S1[k + 1]);
        }
      }
    }
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
        const uint32_t wv = lic / a.mg.lane_stride, ln = lic % a.mg.lane_stride;
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
