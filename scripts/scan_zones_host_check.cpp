// Stand-alone host check of shz_scan_zones (no GPU is touched) on hand-built segment lists, meant to be built with the host
// sanitizers and run on a CPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -c shazam_amd/csrc/shz_scan.hip -o shz_scan.san.o
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -c scripts/scan_zones_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined main.o shz_scan.san.o \
//         <the library's other objects from shazam_amd/csrc> -ldl -o zones_check && ./zones_check
// Exit status 0 and "zones check OK" mean every expectation held and the sanitizers reported nothing.
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

struct seg_list {   // exactly sized heap arrays: a read or write past an end is the sanitizer's to report
  std::vector<uint32_t> rec, sid, first, last, lo, hi;
  std::vector<int64_t> shift;
  void add(uint32_t r, uint32_t s, int64_t h, uint32_t a, uint32_t b) {
    rec.push_back(r); sid.push_back(s); shift.push_back(h); first.push_back(a); last.push_back(b);
  }
  int32_t run(const std::vector<uint64_t>& frames, uint32_t W, uint32_t S, uint32_t M) {
    lo.assign(3 * rec.size(), 77);
    hi.assign(3 * rec.size(), 77);
    lo.shrink_to_fit();
    hi.shrink_to_fit();
    return shz_scan_zones(rec.data(), sid.data(), shift.data(), first.data(), last.data(), rec.size(), frames.data(),
                          (uint32_t)frames.size(), W, S, M, lo.data(), hi.data());
  }
};

int main() {
  {   // two segments of one identity, a gap below the margin: both clamps; another song between them; a second recording
    seg_list L;
    L.add(0, 2, -43, 0, 3);
    L.add(0, 5, 7, 5, 7);
    L.add(0, 2, -43, 9, 12);
    L.add(2, 2, -43, 1, 2);
    EXPECT(L.run({400, 0, 60}, 43, 11, 40) == SHZ_OK);
    EXPECT(L.lo[0] == 0 && L.hi[0] == 99 && L.lo[1] == 0 && L.hi[1] == 43 && L.lo[2] == 33 && L.hi[2] == 99);
    EXPECT(L.lo[3] == 15 && L.hi[3] == 160);
    EXPECT(L.lo[6] == 76 && L.hi[6] == 215 && L.hi[7] == 142 && L.lo[8] == 132);
    EXPECT(L.lo[9] == 0 && L.hi[9] == 60 && L.hi[10] == 54 && L.lo[11] == 22 && L.hi[11] == 60);
  }
  {   // windows behind the end, the largest margin, window numbers and steps at the top of 32 bits
    seg_list L;
    L.add(0, 1, 0, 2, 5);
    L.add(0, 1, 0, 0xFFFFFFF0u, 0xFFFFFFFFu);
    EXPECT(L.run({100}, 10, 30, 0xFFFFFFFFu) == SHZ_OK);
    EXPECT(L.lo[0] == 0 && L.hi[0] == 100 && L.hi[1] == 70 && L.lo[2] == 100 && L.hi[2] == 100);
    EXPECT(L.lo[3] == 100 && L.hi[3] == 100 && L.lo[5] == 100 && L.hi[5] == 100);
    EXPECT(L.run({0xFFFFFFFFull}, 0xFFFFFFFFu, 0xFFFFFFFFu, 0) == SHZ_OK);
    EXPECT(L.lo[0] == 0xFFFFFFFFu && L.hi[0] == 0xFFFFFFFFu);
  }
  {   // refusals write nothing
    seg_list L;
    L.add(0, 1, 0, 4, 3);
    EXPECT(L.run({100}, 10, 30, 0) == SHZ_E_INVALID && L.lo[0] == 77 && L.hi[2] == 77);
    seg_list O;
    O.add(0, 1, 0, 3, 4);
    O.add(0, 2, 0, 4, 6);
    EXPECT(O.run({100}, 10, 30, 0) == SHZ_E_INVALID && O.lo[0] == 77);
    EXPECT(O.run({1ull << 32}, 10, 30, 0) == SHZ_E_INVALID);
    EXPECT(shz_scan_zones(nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 10, 30, 0, nullptr, nullptr) == SHZ_OK);
    EXPECT(shz_scan_zones(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 0, 10, 30, 0, nullptr, nullptr) == SHZ_E_INVALID);
  }
  printf("zones check OK\n");
  return 0;
}
