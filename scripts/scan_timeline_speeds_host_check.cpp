// Stand-alone host check of the scan's host-only functions (no GPU is touched): shz_scan_window_count, shz_scan_timeline,
// shz_scan_timeline_speeds and shz_scan_timeline_warps on hand-built arrays, meant to be built with the host sanitizers and run on a CPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -c shazam_amd/csrc/shz_scan.hip -o shz_scan.san.o      (shz_speed.hip likewise)
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -c scripts/scan_timeline_speeds_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined main.o shz_scan.san.o shz_speed.san.o \
//         <the library's other objects from shazam_amd/csrc> -ldl -o host_check && ./host_check
// Exit status 0 and "host check OK" mean every expectation held and the sanitizers reported nothing.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/shz.h"

#define EXPECT(c)                                                      \
  do {                                                                 \
    if (!(c)) {                                                        \
      fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                         \
    }                                                                  \
  } while (0)

struct segs {
  std::vector<uint32_t> rec, sid, first, last, hits, best, rung;
  std::vector<int32_t> p0, p1;
  explicit segs(size_t n) : rec(n), sid(n), first(n), last(n), hits(n), best(n), rung(n), p0(n), p1(n) {}
};

int main() {
  const uint32_t ladder[9] = {63512, 63604, 63696, 65444, 65536, 65628, 67376, 67468, 67560};
  const int32_t fast[10] = {-23, 0, 22, 45, 68, 90, 113, 136, 158, 181}, slow[10] = {-58, -36, -15, 6, 27, 49, 70, 91, 112, 134};
  const uint32_t topn = 2, n = 20;
  // exactly sized heap arrays: a read or write past an end is the sanitizer's to report
  std::vector<uint32_t> sid(n * topn, 99), aligned(n * topn, 1), nres(n, 1), best(n);
  std::vector<int32_t> delta(n * topn, 0);
  for (uint32_t w = 0; w < n; ++w) {
    sid[w * topn] = w < 10 ? 2 : 4;
    delta[w * topn] = w < 10 ? fast[w] : slow[w - 10];
    aligned[w * topn] = 54 + 3 * w;
    best[w] = w < 10 ? 7 : w % 2;
  }
  const uint64_t win_off[2] = {0, n};
  uint64_t count = 0;
  // cap = 0: counting, NULL outputs
  int32_t rc = shz_scan_timeline_speeds(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder,
                                        9, 40, 1, 1, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                        0, &count);
  EXPECT(rc == SHZ_E_CAPACITY && count == 2);
  for (uint64_t cap = 1; cap <= 3; ++cap) {
    segs s(cap);
    rc = shz_scan_timeline_speeds(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder, 9,
                                  40, 1, 1, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                  s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), cap, &count);
    EXPECT(count == 2 && rc == (cap < 2 ? SHZ_E_CAPACITY : SHZ_OK));
    EXPECT(s.sid[0] == 2 && s.first[0] == 0 && s.last[0] == 9 && s.hits[0] == 10 && s.p0[0] == -23 && s.p1[0] == 181 && s.rung[0] == 7);
    if (cap >= 2) EXPECT(s.sid[1] == 4 && s.first[1] == 10 && s.last[1] == 19 && s.p0[1] == -58 && s.p1[1] == 134 && s.rung[1] == 1);
  }
  // every tolerance at 0 and a one-rung ladder at the range's ends; a rung index beyond the ladder is refused
  for (uint32_t s16 : {32768u, 131072u}) {
    std::vector<uint32_t> b0(n, 0);
    segs s(n);
    rc = shz_scan_timeline_speeds(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), b0.data(), topn, 0xFFFFFFFFu, &s16,
                                  1, 0, 0, 0, 0, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                  s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), n, &count);
    EXPECT(rc == SHZ_OK && count == n);
  }
  rc = shz_scan_timeline_speeds(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder, 7, 40,
                                1, 1, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &count);
  EXPECT(rc == SHZ_E_INVALID);
  // several recordings, one of them without windows
  const uint64_t wo3[4] = {0, 4, 4, n};
  segs s3(8);
  rc = shz_scan_timeline_speeds(wo3, 3, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder, 9, 40, 1, 1,
                                2, s3.rec.data(), s3.sid.data(), s3.first.data(), s3.last.data(), s3.hits.data(), s3.best.data(),
                                s3.p0.data(), s3.p1.data(), s3.rung.data(), 8, &count);
  EXPECT(rc == SHZ_OK && count >= 3 && s3.rec[0] == 0 && s3.rec[1] == 2);
  // the warps' timeline with the diagonal ladder as both tables: neighbouring rungs (92 apart) are in tolerance, so the same two
  // segments come out
  for (uint64_t cap = 0; cap <= 3; ++cap) {
    segs s(cap);
    rc = shz_scan_timeline_warps(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder, ladder,
                                 9, 40, 1, 92, 92, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                 s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), cap, &count);
    EXPECT(count == 2 && rc == (cap < 2 ? SHZ_E_CAPACITY : SHZ_OK));
    if (cap >= 1) EXPECT(s.sid[0] == 2 && s.first[0] == 0 && s.last[0] == 9 && s.hits[0] == 10 && s.p0[0] == -23 && s.p1[0] == 181 && s.rung[0] == 7);
    if (cap >= 2) EXPECT(s.sid[1] == 4 && s.first[1] == 10 && s.last[1] == 19 && s.p0[1] == -58 && s.p1[1] == 134 && s.rung[1] == 1);
  }
  // one rung apart is 92: at a tolerance of 91 every change of rung opens a segment
  {
    segs s(n);
    rc = shz_scan_timeline_warps(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), best.data(), topn, 22, ladder, ladder,
                                 9, 40, 1, 91, 92, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                 s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), n, &count);
    EXPECT(rc == SHZ_OK && count == 11 && s.hits[0] == 10 && s.hits[1] == 1 && s.rung[1] == 0 && s.rung[2] == 1);
  }
  // SHZ_SCAN_NO_WARP on a window that is no hit: the warps' timeline reads best for hits only and bridges the gap, the speeds'
  // checks every window
  {
    std::vector<uint32_t> nres1(nres), best1(best);
    nres1[5] = 0;
    best1[5] = SHZ_SCAN_NO_WARP;
    segs s(2);
    rc = shz_scan_timeline_warps(win_off, 1, sid.data(), delta.data(), aligned.data(), nres1.data(), best1.data(), topn, 22, ladder,
                                 ladder, 9, 40, 1, 92, 92, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                 s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), 2, &count);
    EXPECT(rc == SHZ_OK && count == 2 && s.first[0] == 0 && s.last[0] == 9 && s.hits[0] == 9 && s.rung[0] == 7 && s.hits[1] == 10);
    rc = shz_scan_timeline_speeds(win_off, 1, sid.data(), delta.data(), aligned.data(), nres1.data(), best1.data(), topn, 22, ladder, 9,
                                  40, 1, 1, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(), s.best.data(),
                                  s.p0.data(), s.p1.data(), s.rung.data(), 2, &count);
    EXPECT(rc == SHZ_E_INVALID);
    nres1[5] = 1;   // a hit: now the entry is refused
    rc = shz_scan_timeline_warps(win_off, 1, sid.data(), delta.data(), aligned.data(), nres1.data(), best1.data(), topn, 22, ladder,
                                 ladder, 9, 40, 1, 92, 92, 2, s.rec.data(), s.sid.data(), s.first.data(), s.last.data(), s.hits.data(),
                                 s.best.data(), s.p0.data(), s.p1.data(), s.rung.data(), 2, &count);
    EXPECT(rc == SHZ_E_INVALID);
  }
  // the plain timeline and the window count on the same arrays
  std::vector<uint32_t> a(n), b(n), c(n), d(n), e(n);
  std::vector<int64_t> sh(n);
  rc = shz_scan_timeline(win_off, 1, sid.data(), delta.data(), aligned.data(), nres.data(), topn, 22, 40, 1, a.data(), b.data(), sh.data(),
                         c.data(), d.data(), e.data(), a.data(), n, &count);
  EXPECT(rc == SHZ_OK && count > 2);
  EXPECT(shz_scan_window_count(515, 108, 22) == 20 && shz_scan_window_count(0, 108, 22) == 0 && shz_scan_window_count(30, 1, 4) == 9);
  printf("host check OK\n");
  return 0;
}
