// Context, device memory, timers and the synthetic-PCM generator of libshz.so.
#include <math.h>

#include <algorithm>

#include <time.h>
#include <stdlib.h>

#include "shz_internal.h"

extern "C" const char* shz_version(void) { return "shz 0.2 (gfx950)"; }

int32_t shz_ws_reserve(shz_ctx* ctx, int slot, uint64_t bytes, void** out) {
  shz_buf& b = ctx->ws[slot];
  if (bytes == 0) bytes = 256;
  if (b.cap < bytes) {
    const bool regrow = b.p != nullptr;
    if (b.p) {
      SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
      SHZ_HIP(ctx, hipFree(b.p));
      b.p = nullptr;
      b.cap = 0;
    }
    // slack against regrowth: 12.5 %, 25 % for a slot that has grown before (its size varies from call to call; a
    // hipFree + hipMalloc pair costs milliseconds to tens of milliseconds and showed as slow match batches in a stream)
    uint64_t want = (bytes + (bytes >> (regrow ? 2 : 3)) + 4095) & ~uint64_t(4095);
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
      want = (bytes + 4095) & ~uint64_t(4095);
      e = hipMalloc(&b.p, want);
    }
    if (e != hipSuccess) SHZ_FAIL(ctx, SHZ_E_NOMEM, "hipMalloc(%llu) for workspace slot %d failed: %s",
                                  (unsigned long long)want, slot, hipGetErrorString(e));
    b.cap = want;
  }
  *out = b.p;
  return SHZ_OK;
}

hipError_t shz_block_alloc(shz_ctx* ctx, uint64_t bytes, void** out, uint64_t* got) {
  *out = nullptr;
  if (bytes == 0) bytes = 256;
  {
    std::lock_guard<std::mutex> lk(ctx->blocks_mu);
    int best = -1;
    for (int i = 0; i < (int)ctx->blocks.size(); ++i) {
      const uint64_t c = ctx->blocks[i].cap;
      if (c >= bytes && c <= bytes + bytes / 2 && (best < 0 || c < ctx->blocks[best].cap)) best = i;
    }
    if (best >= 0) {
      *out = ctx->blocks[best].p;
      if (got) *got = ctx->blocks[best].cap;
      ctx->blocks.erase(ctx->blocks.begin() + best);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(out, bytes);
  if (e != hipSuccess) {   // short of memory: what the cache holds goes back first
    (void)hipGetLastError();
    std::vector<shz_buf> drop;
    {
      std::lock_guard<std::mutex> lk(ctx->blocks_mu);
      drop.swap(ctx->blocks);
    }
    for (shz_buf& b : drop) (void)hipFree(b.p);
    e = hipMalloc(out, bytes);
  }
  if (e == hipSuccess && got) *got = bytes;
  return e;
}

void shz_block_free(shz_ctx* ctx, void* p, uint64_t bytes) {
  if (!p) return;
  if (bytes < (256ull << 20)) { (void)hipFree(p); return; }   // small blocks are cheap either way
  std::lock_guard<std::mutex> lk(ctx->blocks_mu);
  ctx->blocks.push_back(shz_buf{p, bytes});
}

int32_t shz_mailbox(shz_ctx* ctx, uint64_t bytes, void** out) {
  if (ctx->mail_cap < bytes) {
    if (ctx->mail) {
      SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
      SHZ_HIP(ctx, hipHostFree(ctx->mail));
      ctx->mail = nullptr;
      ctx->mail_cap = 0;
    }
    const uint64_t want = std::max<uint64_t>(bytes + bytes / 2, 1ull << 16);
    if (hipHostMalloc(&ctx->mail, want, hipHostMallocDefault) != hipSuccess)
      SHZ_FAIL(ctx, SHZ_E_NOMEM, "hipHostMalloc(%llu) failed", (unsigned long long)want);
    ctx->mail_cap = want;
  }
  *out = ctx->mail;
  return SHZ_OK;
}

#define SHZ_PIN_CHUNK (8ull << 20)

hipError_t shz_memcpy(shz_ctx* ctx, void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind) {
  if (bytes == 0) return hipSuccess;
  const bool h2d = kind == hipMemcpyHostToDevice, d2h = kind == hipMemcpyDeviceToHost;
  if ((!h2d && !d2h) || bytes < (16u << 10) || bytes > (64ull << 20)) return hipMemcpyAsync(dst, src, bytes, kind, ctx->stream);
  hipError_t e;
  for (int i = 0; i < 2; ++i)
    if (!ctx->pin[i]) {
      if ((e = hipHostMalloc(&ctx->pin[i], SHZ_PIN_CHUNK, hipHostMallocDefault)) != hipSuccess) return e;
      if ((e = hipEventCreateWithFlags(&ctx->pin_ev[i], hipEventDisableTiming)) != hipSuccess) return e;
    }
  auto wait_free = [&](int i) -> hipError_t {
    if (!ctx->pin_busy[i]) return hipSuccess;
    ctx->pin_busy[i] = false;
    return hipEventSynchronize(ctx->pin_ev[i]);
  };
  // (cutting a copy of a few hundred KB -- one query's PCM -- into four pieces so that the host copy of one overlaps the
  // DMA of the previous one made it slower, 0.178 -> 0.207 ms per fingerprint call: the extra API calls cost more)
  const uint64_t piece = SHZ_PIN_CHUNK;
  const uint64_t nch = (bytes + piece - 1) / piece;
  if (h2d) {
    for (uint64_t k = 0; k < nch; ++k) {
      const int i = (int)(k & 1);
      const uint64_t off = k * piece, n = std::min<uint64_t>(piece, bytes - off);
      if ((e = wait_free(i)) != hipSuccess) return e;
      memcpy(ctx->pin[i], (const char*)src + off, n);
      if ((e = hipMemcpyAsync((char*)dst + off, ctx->pin[i], n, hipMemcpyHostToDevice, ctx->stream)) != hipSuccess) return e;
      if ((e = hipEventRecord(ctx->pin_ev[i], ctx->stream)) != hipSuccess) return e;
      ctx->pin_busy[i] = true;
    }
    return hipSuccess;
  }
  auto issue = [&](uint64_t k) -> hipError_t {
    const int i = (int)(k & 1);
    const uint64_t off = k * piece, n = std::min<uint64_t>(piece, bytes - off);
    hipError_t r = wait_free(i);
    if (r != hipSuccess) return r;
    if ((r = hipMemcpyAsync(ctx->pin[i], (const char*)src + off, n, hipMemcpyDeviceToHost, ctx->stream)) != hipSuccess) return r;
    if ((r = hipEventRecord(ctx->pin_ev[i], ctx->stream)) != hipSuccess) return r;
    ctx->pin_busy[i] = true;
    return hipSuccess;
  };
  if ((e = issue(0)) != hipSuccess) return e;
  for (uint64_t k = 0; k < nch; ++k) {
    if (k + 1 < nch && (e = issue(k + 1)) != hipSuccess) return e;
    const int i = (int)(k & 1);
    const uint64_t off = k * piece, n = std::min<uint64_t>(piece, bytes - off);
    if ((e = wait_free(i)) != hipSuccess) return e;
    memcpy((char*)dst + off, ctx->pin[i], n);
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------------------
// numpy's tables, for the fp64 path that follows the reference's arithmetic operation by operation (mlab._spectral_helper
// -> np.fft.fft, the call of __init__.py:232-237).  Nothing of this is in /root/reference: numpy (2.x) computes a complex
// FFT with the C++ pocketfft, whose plan for n = 4096 is four radix-8 passes with twiddles from `sincos_2pibyn`: two short
// tables of cos / sin (libm, double) whose entries are multiplied -- restated here from the published algorithm and pinned
// by tests/test_numpy_tables.py, which compares the tables and a transform built on them with numpy's own bits.
//   window   np.hanning(n): 0.5 + 0.5 cos(pi k / (n - 1)), k = 1 - n, 3 - n, ...        (mlab.window_hanning)
//   comp[i]  exp(-2 pi i / n) ... the value pocketfft's comp[i] holds (cos, +sin of 2 pi i / n; the passes conjugate)
//   sumsq    (window ** 2).sum() in numpy's pairwise order (8 running sums per block of <= 128, halves above)
static void np_sc_calc(size_t x, size_t n, double ang, double* re, double* im) {
  x <<= 3;
  if (x < 4 * n) {
    if (x < 2 * n) {
      if (x < n) { *re = cos((double)x * ang); *im = sin((double)x * ang); return; }
      *re = sin((double)(2 * n - x) * ang); *im = cos((double)(2 * n - x) * ang); return;
    }
    x -= 2 * n;
    if (x < n) { *re = -sin((double)x * ang); *im = cos((double)x * ang); return; }
    *re = -cos((double)(2 * n - x) * ang); *im = sin((double)(2 * n - x) * ang); return;
  }
  x = 8 * n - x;
  if (x < 2 * n) {
    if (x < n) { *re = cos((double)x * ang); *im = -sin((double)x * ang); return; }
    *re = sin((double)(2 * n - x) * ang); *im = -cos((double)(2 * n - x) * ang); return;
  }
  x -= 2 * n;
  if (x < n) { *re = -sin((double)x * ang); *im = -cos((double)x * ang); return; }
  *re = -cos((double)(2 * n - x) * ang); *im = -sin((double)(2 * n - x) * ang);
}

static double np_pairwise_sum(const double* a, size_t n) {
  if (n < 8) {
    double r = 0.0;
    for (size_t i = 0; i < n; ++i) r += a[i];
    return r;
  }
  if (n <= 128) {
    double r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    size_t i = 8;
    for (; i < n - (n % 8); i += 8)
      for (int j = 0; j < 8; ++j) r[j] += a[i + j];
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += a[i];
    return res;
  }
  size_t n2 = n / 2;
  n2 -= n2 % 8;
  return np_pairwise_sum(a, n2) + np_pairwise_sum(a + n2, n - n2);
}

void shz_numpy_tables_host(uint32_t n, double* window, double2* comp, double* sumsq) {
  if (window) {
    std::vector<double> sq(n);
    for (uint32_t i = 0; i < n; ++i) {
      const double k = (double)(1 - (long)n + 2 * (long)i);
      window[i] = n > 1 ? 0.5 + 0.5 * cos(M_PI * k / (double)(n - 1)) : 1.0;
      sq[i] = window[i] * window[i];
    }
    if (sumsq) *sumsq = np_pairwise_sum(sq.data(), n);
  }
  if (comp) {
    const long double pi = 3.141592653589793238462643383279502884197L;
    const double ang = (double)(0.25L * pi / (long double)n);
    const size_t nval = ((size_t)n + 2) / 2;
    size_t shift = 1;
    while (((size_t)1 << shift) * ((size_t)1 << shift) < nval) ++shift;
    const size_t mask = ((size_t)1 << shift) - 1;
    std::vector<double2> v1(mask + 1), v2((nval + mask) / (mask + 1));
    v1[0] = double2{1.0, 0.0};
    for (size_t i = 1; i < v1.size(); ++i) np_sc_calc(i, n, ang, &v1[i].x, &v1[i].y);
    v2[0] = double2{1.0, 0.0};
    for (size_t i = 1; i < v2.size(); ++i) np_sc_calc(i * (mask + 1), n, ang, &v2[i].x, &v2[i].y);
    for (size_t idx = 0; idx < n; ++idx) {
      if (2 * idx <= n) {
        const double2 x1 = v1[idx & mask], x2 = v2[idx >> shift];
        comp[idx] = double2{x1.x * x2.x - x1.y * x2.y, x1.x * x2.y + x1.y * x2.x};
      } else {
        const size_t m = n - idx;
        const double2 x1 = v1[m & mask], x2 = v2[m >> shift];
        comp[idx] = double2{x1.x * x2.x - x1.y * x2.y, -(x1.x * x2.y + x1.y * x2.x)};
      }
    }
  }
}

// the window of the fp64 path as THE HOST'S numpy forms it (np.hanning(4096) and (window ** 2).sum()): the Python layer hands
// both over when it creates a context, so that the window is numpy's by construction and not by the agreement of two cosine
// routines (numpy may use a vendor routine where this library uses libm; on the hosts seen so far they agree on all 4,096
// arguments).  A C caller that sets nothing gets the libm form of shz_numpy_tables.
extern "C" int32_t shz_set_numpy_window(shz_ctx* ctx, const double* window, double sumsq) {
  if (!ctx) return SHZ_E_INVALID;
  if (!window) SHZ_FAIL(ctx, SHZ_E_INVALID, "window is NULL");
  // (tested on the bits: this file is compiled with -fno-honor-nans)
  auto finite_below = [](double v, double lim) {
    uint64_t b;
    memcpy(&b, &v, 8);
    return ((b >> 52) & 0x7FFu) != 0x7FFu && (b & 0x7FFFFFFFFFFFFFFFull) <= [&] { uint64_t l; memcpy(&l, &lim, 8); return l; }();
  };
  if (!finite_below(sumsq, 1e300) || !(sumsq > 0.0)) SHZ_FAIL(ctx, SHZ_E_INVALID, "sum of the squared window must be positive and finite");
  for (int i = 0; i < SHZ_NFFT; ++i)
    if (!finite_below(window[i], 2.0)) SHZ_FAIL(ctx, SHZ_E_INVALID, "window[%d] is not a window value", i);
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SHZ_HIP(ctx, hipMemcpy(ctx->d_np_window, window, sizeof(double) * SHZ_NFFT, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, hipMemcpy(ctx->d_window, window, sizeof(double) * SHZ_NFFT, hipMemcpyHostToDevice));   // the fast kernel's copy
  ctx->np_sumsq = sumsq;
  ctx->win_sumsq = sumsq;
  if (ctx->twin) return shz_set_numpy_window(ctx->twin, window, sumsq);
  return SHZ_OK;
}

// how the host's numpy multiplies complex numbers: `np.conj(result) * result` of mlab._spectral_helper yields
// fma(re, re, im * im) where numpy's SIMD product has FMA3 (x86-64 AVX2 / AVX-512, the hosts of the fixtures), re*re + im*im
// where it has not.  The Python layer probes its numpy and says which (fused = 1 is the default).
extern "C" int32_t shz_set_numpy_product(shz_ctx* ctx, int32_t fused) {
  if (!ctx) return SHZ_E_INVALID;
  ctx->np_unfused = fused == 0;
  if (ctx->twin) ctx->twin->np_unfused = ctx->np_unfused;
  return SHZ_OK;
}

extern "C" int32_t shz_numpy_tables(uint32_t nfft, double* window, double* twiddles, double* sumsq) {
  if (nfft < 2 || nfft > (1u << 20)) return SHZ_E_INVALID;
  shz_numpy_tables_host(nfft, window, (double2*)twiddles, sumsq);
  return SHZ_OK;
}

extern "C" int32_t shz_ctx_create(int32_t device_id, shz_ctx** out) {
  if (!out) return SHZ_E_INVALID;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device_id < 0 || device_id >= n) return SHZ_E_HIP;
  if (hipSetDevice(device_id) != hipSuccess) return SHZ_E_HIP;
  shz_ctx* ctx = new shz_ctx();
  ctx->device = device_id;
  if (hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
    delete ctx;
    return SHZ_E_HIP;
  }
  ctx->ws_limit = ctx->prop.totalGlobalMem / 4;
  // constant tables.  The window of the fast STFT kernel is numpy's np.hanning(4096), the one the reference multiplies with
  // (npw below; shz_set_numpy_window replaces both copies).  It used to be the correctly rounded Hann window (evaluated in
  // long double): 2,254 of the 4,096 values differ from numpy's, by 2^-52 at most -- nothing against a frame's maximum,
  // but 4e-11 of w[1] and 1e-13 of w[32], so a frame whose only samples sit in the window's first or last few dozen came
  // out that far from the reference's spectrogram (tests/test_gpu_stft_stage.py: clips of 2, 3 and 33-37 samples).
  const long double pi = 3.14159265358979323846264338327950288L;
  // twiddles of the 2048-point FFT (layout: stft_tables in shz_extract.hip): W^k for k <= 512 (the other octants by
  // symmetry), then W_64^(k t) for pass 2 ([t-1][k], k < 8) and W_512^(k t) for pass 3 ([t-1][k], k < 64), t = 1..7
  std::vector<double2> tw;
  auto W = [&](long m) {  // W4096^m
    const long double a = -2.0L * pi * (long double)(m % SHZ_NFFT) / (long double)SHZ_NFFT;
    return double2{(double)cosl(a), (double)sinl(a)};
  };
  for (int k = 0; k <= SHZ_NFFT / 8; ++k) tw.push_back(W(k));
  for (int t = 1; t < 8; ++t)
    for (int k = 0; k < 8; ++k) tw.push_back(W(64L * k * t));
  for (int t = 1; t < 8; ++t)
    for (int k = 0; k < 64; ++k) tw.push_back(W(8L * k * t));
  std::vector<int16_t> lut(4096);
  for (int i = 0; i < 4096; ++i) lut[i] = (int16_t)lrint(32767.0 * sin(2.0 * M_PI * (double)i / 4096.0));
  std::vector<double> npw(SHZ_NFFT);
  std::vector<double2> npc(SHZ_NFFT);
  shz_numpy_tables_host(SHZ_NFFT, npw.data(), npc.data(), &ctx->np_sumsq);
  const std::vector<double>& win = npw;
  ctx->win_sumsq = ctx->np_sumsq;
  {  // the twiddles in the order the passes read them (pocketfft's own per-pass tables: [c - 1][i] = comp[c l1 i]): copies,
     // no arithmetic -- neighbouring lanes then read neighbouring entries instead of 64 cache lines a load
    std::vector<double2> tw(SHZ_NFFT, double2{0.0, 0.0});
    size_t base = 0;
    for (uint32_t l1 = 1; l1 < SHZ_NFFT; l1 *= 8) {
      const uint32_t ido = SHZ_NFFT / (8 * l1);
      for (uint32_t c = 1; c < 8; ++c)
        for (uint32_t i = 0; i < ido; ++i) tw[base + (size_t)(c - 1) * ido + i] = npc[(size_t)c * l1 * i];
      base += (size_t)7 * ido;
    }
    npc.swap(tw);
  }
  bool ok = hipMalloc(&ctx->d_np_window, sizeof(double) * SHZ_NFFT) == hipSuccess &&
            hipMalloc(&ctx->d_np_comp, sizeof(double2) * SHZ_NFFT) == hipSuccess &&
            hipMemcpy(ctx->d_np_window, npw.data(), sizeof(double) * SHZ_NFFT, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(ctx->d_np_comp, npc.data(), sizeof(double2) * SHZ_NFFT, hipMemcpyHostToDevice) == hipSuccess &&
            hipMalloc(&ctx->d_window, sizeof(double) * SHZ_NFFT) == hipSuccess &&
            hipMalloc(&ctx->d_twiddle, sizeof(double2) * tw.size()) == hipSuccess &&
            hipMalloc(&ctx->d_sine_lut, sizeof(int16_t) * 4096) == hipSuccess &&
            hipMemcpy(ctx->d_window, win.data(), sizeof(double) * SHZ_NFFT, hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(ctx->d_twiddle, tw.data(), sizeof(double2) * tw.size(), hipMemcpyHostToDevice) == hipSuccess &&
            hipMemcpy(ctx->d_sine_lut, lut.data(), sizeof(int16_t) * 4096, hipMemcpyHostToDevice) == hipSuccess;
  if (!ok) {
    shz_ctx_destroy(ctx);
    return SHZ_E_HIP;
  }
  *out = ctx;
  return SHZ_OK;
}

extern "C" int32_t shz_ctx_destroy(shz_ctx* ctx) {
  if (!ctx) return SHZ_E_INVALID;
  (void)hipSetDevice(ctx->device);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  for (auto& b : ctx->ws)
    if (b.p) (void)hipFree(b.p);
  for (auto& b : ctx->blocks)
    if (b.p) (void)hipFree(b.p);
  ctx->blocks.clear();
  if (ctx->d_window) (void)hipFree(ctx->d_window);
  if (ctx->d_np_window) (void)hipFree(ctx->d_np_window);
  if (ctx->d_np_comp) (void)hipFree(ctx->d_np_comp);
  if (ctx->d_twiddle) (void)hipFree(ctx->d_twiddle);
  if (ctx->d_sine_lut) (void)hipFree(ctx->d_sine_lut);
  if (ctx->d_filter) (void)hipFree(ctx->d_filter);   // shz_set_song_filter
  if (ctx->twin) { (void)shz_ctx_destroy(ctx->twin); ctx->twin = nullptr; }
  if (ctx->ev_twin) (void)hipEventDestroy(ctx->ev_twin);
  if (ctx->mail) (void)hipHostFree(ctx->mail);
  for (int i = 0; i < 2; ++i) {
    if (ctx->pin[i]) (void)hipHostFree(ctx->pin[i]);
    if (ctx->pin_ev[i]) (void)hipEventDestroy(ctx->pin_ev[i]);
  }
  for (hipEvent_t e : ctx->rq_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->sc_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->sp_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->rp_ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->tev_init)
    for (auto& e : ctx->tev) {
      (void)hipEventDestroy(e[0]);
      (void)hipEventDestroy(e[1]);
    }
  for (auto* v : {&ctx->prof_pending, &ctx->prof_free})
    for (auto& r : *v) {
      (void)hipEventDestroy(r.a);
      (void)hipEventDestroy(r.b);
    }
  if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
  delete ctx;
  return SHZ_OK;
}

extern "C" const char* shz_last_error(shz_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

extern "C" int32_t shz_device_info(shz_ctx* ctx, char* name, uint64_t name_cap, uint64_t* hbm_bytes,
                                   int32_t* compute_units, int32_t* clock_khz) {
  if (!ctx) return SHZ_E_INVALID;
  if (name && name_cap) {
    snprintf(name, name_cap, "%s (%s)", ctx->prop.name, ctx->prop.gcnArchName);
  }
  if (hbm_bytes) *hbm_bytes = ctx->prop.totalGlobalMem;
  if (compute_units) *compute_units = ctx->prop.multiProcessorCount;
  if (clock_khz) *clock_khz = ctx->prop.clockRate;
  return SHZ_OK;
}

extern "C" int32_t shz_mem_info(shz_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes) {
  if (!ctx) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  size_t f = 0, t = 0;
  SHZ_HIP(ctx, hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return SHZ_OK;
}

extern "C" int32_t shz_dev_alloc(shz_ctx* ctx, uint64_t bytes, void** dptr) {
  if (!ctx || !dptr) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  hipError_t e = hipMalloc(dptr, bytes ? bytes : 256);
  if (e != hipSuccess) SHZ_FAIL(ctx, SHZ_E_NOMEM, "hipMalloc(%llu) failed: %s", (unsigned long long)bytes, hipGetErrorString(e));
  return SHZ_OK;
}

extern "C" int32_t shz_dev_free(shz_ctx* ctx, void* dptr) {
  if (!ctx) return SHZ_E_INVALID;
  if (!dptr) return SHZ_OK;
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  SHZ_HIP(ctx, hipFree(dptr));
  return SHZ_OK;
}

extern "C" int32_t shz_copy_h2d(shz_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return SHZ_E_INVALID;
  if (!bytes) return SHZ_OK;
  SHZ_HIP(ctx, shz_memcpy(ctx, dst, src, bytes, hipMemcpyHostToDevice));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_copy_d2h(shz_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
  if (!ctx || (bytes && (!dst || !src))) return SHZ_E_INVALID;
  if (!bytes) return SHZ_OK;
  SHZ_HIP(ctx, shz_memcpy(ctx, dst, src, bytes, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_sync(shz_ctx* ctx) {
  if (!ctx) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_set_workspace_limit(shz_ctx* ctx, uint64_t bytes) {
  if (!ctx) return SHZ_E_INVALID;
  ctx->ws_limit = bytes ? bytes : ctx->prop.totalGlobalMem / 4;
  return SHZ_OK;
}

extern "C" int32_t shz_release_workspace(shz_ctx* ctx, uint64_t* freed_bytes) {
  if (!ctx) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  uint64_t freed = 0;
  for (auto& b : ctx->ws)
    if (b.p) {
      SHZ_HIP(ctx, hipFree(b.p));
      freed += b.cap;
      b.p = nullptr;
      b.cap = 0;
    }
  {
    std::lock_guard<std::mutex> lk(ctx->blocks_mu);
    for (shz_buf& b : ctx->blocks) {
      (void)hipFree(b.p);
      freed += b.cap;
    }
    ctx->blocks.clear();
  }
  if (freed_bytes) *freed_bytes = freed;
  return SHZ_OK;
}

extern "C" int32_t shz_timer_start(shz_ctx* ctx, int32_t slot) {
  if (!ctx || slot < 0 || slot >= 16) return SHZ_E_INVALID;
  if (!ctx->tev_init) {
    for (auto& e : ctx->tev) {
      SHZ_HIP(ctx, hipEventCreate(&e[0]));
      SHZ_HIP(ctx, hipEventCreate(&e[1]));
    }
    ctx->tev_init = true;
  }
  SHZ_HIP(ctx, hipEventRecord(ctx->tev[slot][0], ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_timer_stop(shz_ctx* ctx, int32_t slot, float* ms) {
  if (!ctx || slot < 0 || slot >= 16 || !ctx->tev_init) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipEventRecord(ctx->tev[slot][1], ctx->stream));
  SHZ_HIP(ctx, hipEventSynchronize(ctx->tev[slot][1]));
  float v = 0;
  SHZ_HIP(ctx, hipEventElapsedTime(&v, ctx->tev[slot][0], ctx->tev[slot][1]));
  if (ms) *ms = v;
  return SHZ_OK;
}

void shz_prof_begin(shz_ctx* ctx, int which) {
  shz_prof_rec r;
  if (!ctx->prof_free.empty()) {
    r = ctx->prof_free.back();
    ctx->prof_free.pop_back();
  } else if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) {
    return;
  }
  r.which = which;
  (void)hipEventRecord(r.a, ctx->stream);
  ctx->prof_pending.push_back(r);
}

void shz_prof_end(shz_ctx* ctx) {
  if (!ctx->prof_pending.empty()) (void)hipEventRecord(ctx->prof_pending.back().b, ctx->stream);
}

static void prof_drain(shz_ctx* ctx) {
  if (ctx->prof_pending.empty()) return;
  (void)hipStreamSynchronize(ctx->stream);
  for (auto& r : ctx->prof_pending) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
      ctx->kernel_ms[r.which] += ms;
      ctx->kernel_launches[r.which] += 1;
    }
    ctx->prof_free.push_back(r);
  }
  ctx->prof_pending.clear();
}

extern "C" int32_t shz_set_profiling(shz_ctx* ctx, int32_t enabled) {
  if (!ctx) return SHZ_E_INVALID;
  prof_drain(ctx);
  ctx->profiling = enabled != 0;
  for (int i = 0; i < 8; ++i) {
    ctx->kernel_ms[i] = 0;
    ctx->kernel_launches[i] = 0;
  }
  if (ctx->twin) (void)shz_set_profiling(ctx->twin, enabled);
  return SHZ_OK;
}

extern "C" int32_t shz_get_kernel_ms(shz_ctx* ctx, int32_t which, float* total_ms, uint32_t* launches) {
  if (!ctx || which < 0 || which >= 8) return SHZ_E_INVALID;
  prof_drain(ctx);
  float ms = ctx->kernel_ms[which];
  uint32_t n = ctx->kernel_launches[which];
  if (ctx->twin) {   // the second pipeline of dual extraction passes
    prof_drain(ctx->twin);
    ms += ctx->twin->kernel_ms[which];
    n += ctx->twin->kernel_launches[which];
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = n;
  return SHZ_OK;
}

// ---------------------------------------------------------------------------------------
// Synthetic PCM: integer-only generator, bit-identical numpy twin in oracle/synth.py.
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  uint64_t z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

#define SYN_NOTE_SHIFT 14
#define SYN_NPART 6
#define SYN_OM_MIN 10713046u
#define SYN_OM_MAX 428521855u

// one thread = 8 consecutive samples (one 16-byte store); grid.y = clip.  The six partials of a note (2^14 samples) are drawn
// once per thread when its eight samples lie in one note (they do unless `start` is odd against the note grid), phases advance
// in 32-bit arithmetic (only the low word of r + m * om is used), and the sine table sits in LDS: 1M x 30 s tracks took 6.9 s
// with the per-sample form below (seven splitmix64 and six cached global gathers a sample), which was longer than
// fingerprinting them.  Same values, bit for bit (tests/test_gpu_synth.py against oracle/synth.py).
__device__ __forceinline__ long long synth_tone_sample(uint64_t key, uint64_t n, const int16_t* lut) {
  const uint64_t seg = n >> SYN_NOTE_SHIFT, m = n & ((1u << SYN_NOTE_SHIFT) - 1);
  long long s = 0;
#pragma unroll
  for (int k = 0; k < SYN_NPART; ++k) {
    uint64_t r = splitmix64(~key + seg * 8 + (uint64_t)k);
    uint64_t om = (uint64_t)SYN_OM_MIN + (((r >> 32) * (uint64_t)(SYN_OM_MAX - SYN_OM_MIN)) >> 32);
    uint32_t ph = (uint32_t)(r + m * om);
    s += lut[ph >> 20];
  }
  return s;
}

__global__ __launch_bounds__(256) void synth_pcm_kernel(int16_t* __restrict__ out, uint64_t seed, uint64_t clip0,
                                                        uint64_t n_samples, uint64_t start, int tone_amp,
                                                        int noise_amp, const int16_t* __restrict__ lut) {
  __shared__ int16_t s_lut[4096];
  if (tone_amp > 0) {
    for (int i = threadIdx.x; i < 4096 / 8; i += 256)
      reinterpret_cast<uint4*>(s_lut)[i] = reinterpret_cast<const uint4*>(lut)[i];
    __syncthreads();
  }
  const uint64_t clip = blockIdx.y;
  const uint64_t key = splitmix64(seed * 0xD6E8FEB86659FD93ull + clip0 + clip);
  int16_t* dst = out + clip * n_samples;
  for (uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; base < n_samples;
       base += (uint64_t)gridDim.x * blockDim.x * 8) {
    const uint64_t n0 = start + base;
    int tone[8];
    if (tone_amp > 0) {
      if (((n0 + 7) >> SYN_NOTE_SHIFT) == (n0 >> SYN_NOTE_SHIFT)) {
        const uint64_t seg = n0 >> SYN_NOTE_SHIFT;
        const uint32_t m0 = (uint32_t)(n0 & ((1u << SYN_NOTE_SHIFT) - 1));
        int s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < SYN_NPART; ++k) {
          const uint64_t r = splitmix64(~key + seg * 8 + (uint64_t)k);
          const uint32_t om = SYN_OM_MIN + (uint32_t)(((r >> 32) * (uint64_t)(SYN_OM_MAX - SYN_OM_MIN)) >> 32);
          uint32_t ph = (uint32_t)r + m0 * om;
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            s[i] += s_lut[ph >> 20];
            ph += om;
          }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) tone[i] = (int)(((long long)s[i] * tone_amp) >> 17);
      } else {
#pragma unroll 1
        for (int i = 0; i < 8; ++i) tone[i] = (int)((synth_tone_sample(key, n0 + i, s_lut) * tone_amp) >> 17);
      }
    }
    int16_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      int acc = 0;
      if (noise_amp > 0) {
        const uint32_t u = (uint32_t)(splitmix64(key + n0 + i) >> 32);
        acc += (int)(((uint64_t)u * (uint32_t)(2 * noise_amp)) >> 32) - noise_amp;
      }
      if (tone_amp > 0) acc += tone[i];
      acc = acc < -32768 ? -32768 : (acc > 32767 ? 32767 : acc);
      v[i] = (int16_t)acc;
    }
    if (base + 8 <= n_samples && ((clip * n_samples + base) & 7) == 0) {
      *reinterpret_cast<uint4*>(dst + base) = *reinterpret_cast<const uint4*>(v);
    } else {
      for (int i = 0; i < 8 && base + i < n_samples; ++i) dst[base + i] = v[i];
    }
  }
}

extern "C" int32_t shz_synth_pcm(shz_ctx* ctx, uint64_t seed, uint64_t clip0, uint32_t n_clips, uint64_t n_samples,
                                 int32_t tone_amp, int32_t noise_amp, uint64_t start_sample, int16_t* dev_out) {
  if (!ctx || !dev_out) return SHZ_E_INVALID;
  if (n_clips == 0 || n_samples == 0) return SHZ_OK;
  if (n_clips > 65535) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_synth_pcm: at most 65535 clips per call (got %u)", n_clips);
  if (tone_amp < 0 || noise_amp < 0 || tone_amp > 10000 || noise_amp > 32768)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_synth_pcm: tone_amp in [0,10000], noise_amp in [0,32768]");
  uint64_t per = (n_samples + 8 * 256 - 1) / (8 * 256);
  per = tone_amp > 0 ? (per + 3) / 4 : per;   // (four strides a workgroup: the table is loaded into LDS once for them)
  dim3 grid((unsigned)(per > 4096 ? 4096 : per), n_clips);
  hipLaunchKernelGGL(synth_pcm_kernel, grid, dim3(256), 0, ctx->stream, dev_out, seed, clip0, n_samples, start_sample,
                     tone_amp, noise_amp, ctx->d_sine_lut);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// ---------------------------------------------------------------------------------------
// Music-like corpus and traffic-like noise (numpy twins: oracle/synth.music_clip / traffic_noise, bit for bit).
// Stand-ins for what the reference's accuracy was measured on (real music under low-passed street noise,
// recognizer_test.py:39-40, 542-558); integer-only and random-access like synth_pcm_kernel.
#define MUS_VOICES 4
#define MUS_NHARM 8
#define MUS_BURST_LEN 2048
__constant__ uint32_t c_mus_omega[48] = {
    10713070u, 11350103u, 12025015u, 12740059u, 13497623u, 14300233u, 15150569u, 16051469u, 17005939u, 18017165u, 19088521u,
    20223584u, 21426141u, 22700205u, 24050030u, 25480119u, 26995246u, 28600467u, 30301139u, 32102938u, 34011878u, 36034330u,
    38177043u, 40447168u, 42852281u, 45400411u, 48100060u, 50960238u, 53990491u, 57200933u, 60602278u, 64205876u, 68023757u,
    72068660u, 76354085u, 80894335u, 85704563u, 90800821u, 96200119u, 101920476u, 107980983u, 114401866u, 121204555u,
    128411753u, 136047513u, 144137319u, 152708170u, 161788671u};
__constant__ int c_mus_shift[MUS_VOICES] = {14, 15, 13, 12};
__constant__ int c_mus_octave[MUS_VOICES] = {1, 1, 1, 2};
__constant__ int c_mus_harm[MUS_NHARM] = {256, 200, 150, 120, 100, 80, 64, 50};

template <int KIND>   // 1: music (amp, bed, burst), 2: traffic noise (amp)
__global__ __launch_bounds__(256) void synth_corpus_kernel(int16_t* __restrict__ out, uint64_t seed, uint64_t clip0,
                                                           uint64_t n_samples, uint64_t start, int amp, int bed, int burst,
                                                           const int16_t* __restrict__ lut) {
  const uint64_t clip = blockIdx.y;
  const uint64_t key = splitmix64(seed * 0xD6E8FEB86659FD93ull + clip0 + clip);
  int16_t* dst = out + clip * n_samples;
  for (uint64_t base = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 8; base < n_samples;
       base += (uint64_t)gridDim.x * blockDim.x * 8) {
    int16_t v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t n = start + base + i;
      long long acc = 0;
      if (KIND == 1) {
        if (bed > 0) {
          const uint64_t u = splitmix64(key + n) >> 32;
          acc += (long long)((u * (uint64_t)(2 * bed)) >> 32) - bed;
        }
#pragma unroll
        for (int vc = 0; vc < MUS_VOICES; ++vc) {
          const int sh = c_mus_shift[vc];
          const uint64_t k = n >> sh, m = n & ((1ull << sh) - 1);
          const uint64_t r = splitmix64(~key + ((uint64_t)vc << 40) + k);
          if ((r >> 60) == 0) continue;
          const uint64_t om = ((uint64_t)c_mus_omega[(r >> 8) % 48] * (uint64_t)c_mus_octave[vc] * (63488ull + ((r >> 24) & 0xFFFull))) >> 16;   // +-3 % detune per note
          const long long env = (long long)((1ull << sh) - m);
          long long s = 0;
#pragma unroll
          for (int h = 1; h <= MUS_NHARM; ++h) {
            const uint32_t ph = (uint32_t)((r >> 16) * (uint64_t)h + m * om * (uint64_t)h);
            s += (long long)lut[ph >> 20] * c_mus_harm[h - 1];
          }
          acc += (((s * env) >> (sh + 8)) * amp) >> 15;
          if (vc == 0 && burst > 0) {
            const uint64_t ub = splitmix64(r + m) >> 32;
            const long long nb = (long long)((ub * (uint64_t)(2 * burst)) >> 32) - burst;
            const long long e2 = (long long)MUS_BURST_LEN - (long long)m;
            if (e2 > 0) acc += (nb * e2) >> 11;
          }
        }
      } else {
#pragma unroll
        for (int t = 0; t < 16; ++t) {
          const uint64_t u = splitmix64(key + n + (uint64_t)t) >> 32;
          acc += (long long)((u * (uint64_t)(2 * amp)) >> 32) - amp;
        }
        acc >>= 2;
      }
      acc = acc < -32768 ? -32768 : (acc > 32767 ? 32767 : acc);
      v[i] = (int16_t)acc;
    }
    if (base + 8 <= n_samples && ((clip * n_samples + base) & 7) == 0) {
      *reinterpret_cast<uint4*>(dst + base) = *reinterpret_cast<const uint4*>(v);
    } else {
      for (int i = 0; i < 8 && base + i < n_samples; ++i) dst[base + i] = v[i];
    }
  }
}

extern "C" int32_t shz_synth_corpus(shz_ctx* ctx, uint32_t kind, uint64_t seed, uint64_t clip0, uint32_t n_clips,
                                    uint64_t n_samples, int32_t amp, int32_t bed, int32_t burst, uint64_t start_sample,
                                    int16_t* dev_out) {
  if (!ctx || !dev_out) return SHZ_E_INVALID;
  if (n_clips == 0 || n_samples == 0) return SHZ_OK;
  if (kind != SHZ_CORPUS_MUSIC && kind != SHZ_CORPUS_TRAFFIC) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_synth_corpus: kind %u", kind);
  if (n_clips > 65535) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_synth_corpus: at most 65535 clips per call (got %u)", n_clips);
  if (amp < 0 || bed < 0 || burst < 0 || amp > 8000 || bed > 32768 || burst > 32768)
    SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_synth_corpus: amp in [0,8000], bed and burst in [0,32768]");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  const uint64_t per = (n_samples + 8 * 256 - 1) / (8 * 256);
  dim3 grid((unsigned)(per > 4096 ? 4096 : per), n_clips);
  if (kind == SHZ_CORPUS_MUSIC)
    hipLaunchKernelGGL(synth_corpus_kernel<1>, grid, dim3(256), 0, ctx->stream, dev_out, seed, clip0, n_samples, start_sample, amp,
                       bed, burst, ctx->d_sine_lut);
  else
    hipLaunchKernelGGL(synth_corpus_kernel<2>, grid, dim3(256), 0, ctx->stream, dev_out, seed, clip0, n_samples, start_sample, amp,
                       bed, burst, ctx->d_sine_lut);
  SHZ_HIP(ctx, hipGetLastError());
  return SHZ_OK;
}

// ---------------------------------------------------------------------------------------
// Query preparation on the device (bench / tests): exact integer sum of squares per clip and
// signal + scale * noise re-quantised to int16 -- the digital form of the reference's noise
// mixing (recognizer_test.py:426-435, 557).  The scale itself is computed on the host from the
// exact sums with the reference's formula, so the numpy twin (oracle/synth.mix_query) and this
// path agree bit for bit.
__global__ __launch_bounds__(256) void sumsq_i16_kernel(const int16_t* __restrict__ x, uint64_t n_samples,
                                                        unsigned long long* __restrict__ out) {
  const int16_t* src = x + (uint64_t)blockIdx.y * n_samples;
  unsigned long long s = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_samples; i += (uint64_t)gridDim.x * blockDim.x) {
    const long long v = src[i];
    s += (unsigned long long)(v * v);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor((long long)s, d, 64);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(out + blockIdx.y, s);
}

__global__ __launch_bounds__(256) void mix_i16_kernel(const int16_t* __restrict__ sig, const int16_t* __restrict__ noise,
                                                      uint64_t n_samples, const double* __restrict__ scale,
                                                      int16_t* __restrict__ out) {
  const uint64_t base = (uint64_t)blockIdx.y * n_samples;
  const double sc = scale[blockIdx.y];
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_samples; i += (uint64_t)gridDim.x * blockDim.x) {
    double v = rint((double)sig[base + i] + (double)noise[base + i] * sc);
    v = v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v);
    out[base + i] = (int16_t)v;
  }
}

extern "C" int32_t shz_sumsq_i16(shz_ctx* ctx, const int16_t* dev_pcm, uint32_t n_clips, uint64_t n_samples,
                                 uint64_t* out_host) {
  if (!ctx || !dev_pcm || !out_host) return SHZ_E_INVALID;
  if (n_clips == 0) return SHZ_OK;
  if (n_clips > 65535) SHZ_FAIL(ctx, SHZ_E_INVALID, "at most 65535 clips per call");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void* d;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC3, 8ull * n_clips, &d));
  SHZ_HIP(ctx, hipMemsetAsync(d, 0, 8ull * n_clips, ctx->stream));
  uint64_t per = (n_samples + 255) / 256;
  dim3 grid((unsigned)(per > 64 ? 64 : (per ? per : 1)), n_clips);
  hipLaunchKernelGGL(sumsq_i16_kernel, grid, dim3(256), 0, ctx->stream, dev_pcm, n_samples, (unsigned long long*)d);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, shz_memcpy(ctx, out_host, d, 8ull * n_clips, hipMemcpyDeviceToHost));
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

extern "C" int32_t shz_mix_i16(shz_ctx* ctx, const int16_t* dev_sig, const int16_t* dev_noise, uint32_t n_clips,
                               uint64_t n_samples, const double* scale_host, int16_t* dev_out) {
  if (!ctx || !dev_sig || !dev_noise || !scale_host || !dev_out) return SHZ_E_INVALID;
  if (n_clips == 0 || n_samples == 0) return SHZ_OK;
  if (n_clips > 65535) SHZ_FAIL(ctx, SHZ_E_INVALID, "at most 65535 clips per call");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  void* d;
  SHZ_TRY(shz_ws_reserve(ctx, SHZ_WS_MISC3, 8ull * n_clips, &d));
  SHZ_HIP(ctx, shz_memcpy(ctx, d, scale_host, 8ull * n_clips, hipMemcpyHostToDevice));
  uint64_t per = (n_samples + 255) / 256;
  dim3 grid((unsigned)(per > 64 ? 64 : per), n_clips);
  hipLaunchKernelGGL(mix_i16_kernel, grid, dim3(256), 0, ctx->stream, dev_sig, dev_noise, n_samples, (const double*)d, dev_out);
  SHZ_HIP(ctx, hipGetLastError());
  SHZ_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SHZ_OK;
}

// ---------------------------------------------------------------------------------------- HBM bandwidth probe
// "confirm on the box with a stream-copy microbench and use the measured copy bandwidth as the
// practical ceiling".  16 bytes per lane, grid-stride, buffers far larger than L2 + Infinity Cache.
__global__ __launch_bounds__(256) void membw_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n16,
                                                    int mode, uint32_t* __restrict__ sink) {
  uint4 acc = make_uint4(0, 0, 0, 0);
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (uint64_t)gridDim.x * blockDim.x) {
    if (mode == 2) {
      dst[i] = make_uint4((uint32_t)i, 1u, 2u, 3u);
    } else {
      const uint4 v = src[i];
      if (mode == 0) dst[i] = v;
      else { acc.x ^= v.x; acc.y ^= v.y; acc.z ^= v.z; acc.w ^= v.w; }
    }
  }
  if (mode == 1 && (acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x9E3779B9u) *sink = 1;  // keeps the loads alive
}

// Pinned host memory for the caller's PCM: a decoder that writes its samples here hands shz_fingerprint_batch a buffer the
// DMA engines read directly (no staging copy, no page registration per call).
extern "C" int32_t shz_host_alloc(shz_ctx* ctx, uint64_t bytes, void** out) {
  if (!ctx || !out) return SHZ_E_INVALID;
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  *out = nullptr;
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_host_alloc: hipHostMalloc(%llu) failed", (unsigned long long)bytes);
  }
  return SHZ_OK;
}
extern "C" int32_t shz_host_free(shz_ctx* ctx, void* p) {   // ctx may be NULL (a buffer may outlive its context)
  if (!p) return SHZ_OK;
  if (hipHostFree(p) != hipSuccess) {
    (void)hipGetLastError();
    if (ctx) SHZ_FAIL(ctx, SHZ_E_HIP, "shz_host_free: hipHostFree failed");
    return SHZ_E_HIP;
  }
  return SHZ_OK;
}

extern "C" int32_t shz_membw(shz_ctx* ctx, int32_t mode, uint64_t bytes, uint32_t iters, float* gb_per_s) {
  if (!ctx || !gb_per_s) return SHZ_E_INVALID;
  if (mode < 0 || mode > 5 || bytes < (1ull << 20) || iters < 1) SHZ_FAIL(ctx, SHZ_E_INVALID, "shz_membw: mode 0..5, >= 1 MiB, >= 1 iteration");
  SHZ_HIP(ctx, hipSetDevice(ctx->device));
  if (mode >= 3) {   // the host link: 3 pinned host -> device, 4 pageable host -> device, 5 device -> pinned host (host clock)
    void *d = nullptr, *h = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_membw: hipMalloc(%llu) failed", (unsigned long long)bytes);
    if (mode == 4) h = malloc(bytes);
    else if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess) h = nullptr;
    if (!h) { (void)hipFree(d); SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_membw: host allocation of %llu bytes failed", (unsigned long long)bytes); }
    memset(h, 0x5A, bytes);
    const hipMemcpyKind kd = mode == 5 ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    void *dst = mode == 5 ? h : d, *src = mode == 5 ? d : h;
    hipError_t err = hipMemcpyAsync(dst, src, bytes, kd, ctx->stream);   // warm-up (page faults, first-touch of the staging)
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    const double t0 = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }();
    for (uint32_t it = 0; it < iters && err == hipSuccess; ++it) err = hipMemcpyAsync(dst, src, bytes, kd, ctx->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(ctx->stream);
    const double t1 = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec + 1e-9 * ts.tv_nsec; }();
    (void)hipFree(d);
    if (mode == 4) free(h); else (void)hipHostFree(h);
    SHZ_HIP(ctx, err);
    *gb_per_s = (float)((double)bytes * iters / (t1 - t0) / 1e9);
    return SHZ_OK;
  }
  const uint64_t n16 = bytes / 16;
  void *a = nullptr, *b = nullptr, *sink = nullptr;
  if (hipMalloc(&a, n16 * 16) != hipSuccess || hipMalloc(&b, n16 * 16) != hipSuccess || hipMalloc(&sink, 64) != hipSuccess) {
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
    if (sink) (void)hipFree(sink);
    SHZ_FAIL(ctx, SHZ_E_NOMEM, "shz_membw: hipMalloc(2 x %llu) failed", (unsigned long long)(n16 * 16));
  }
  (void)hipMemsetAsync(a, 0x5A, n16 * 16, ctx->stream);
  (void)hipMemsetAsync(b, 0, n16 * 16, ctx->stream);
  const unsigned grid = (unsigned)ctx->prop.multiProcessorCount * 16;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  hipLaunchKernelGGL(membw_kernel, dim3(grid), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16, mode, (uint32_t*)sink);  // warm-up
  (void)hipEventRecord(e0, ctx->stream);
  for (uint32_t it = 0; it < iters; ++it)
    hipLaunchKernelGGL(membw_kernel, dim3(grid), dim3(256), 0, ctx->stream, (const uint4*)a, (uint4*)b, n16, mode, (uint32_t*)sink);
  (void)hipEventRecord(e1, ctx->stream);
  hipError_t err = hipEventSynchronize(e1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(a);
  (void)hipFree(b);
  (void)hipFree(sink);
  SHZ_HIP(ctx, err);
  const double moved = (double)(n16 * 16) * iters * (mode == 0 ? 2.0 : 1.0);  // copy = one read + one write
  *gb_per_s = ms > 0.f ? (float)(moved / (ms * 1e-3) / 1e9) : 0.f;
  return SHZ_OK;
}
