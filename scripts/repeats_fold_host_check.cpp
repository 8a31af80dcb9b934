// Stand-alone host check of shz_repeats_fold (no GPU is touched) on hand-built cell lists, meant to be built with the host
// sanitizers and run on a CPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -c shazam_amd/csrc/shz_repeat.hip -o shz_repeat.san.o
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -c scripts/repeats_fold_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined main.o shz_repeat.san.o \
//         <the library's other objects from shazam_amd/csrc> -ldl -o repeats_fold_check && ./repeats_fold_check
// Exit status 0 and "repeats fold check OK" mean every expectation held and the sanitizers reported nothing.
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

struct cell_list {   // exactly sized heap arrays: a read or write past an end is the sanitizer's to report
  std::vector<uint64_t> off{0}, pairs_out;
  std::vector<uint32_t> lag, block, pairs, first, last;
  std::vector<uint32_t> rec, rlag, lo, hi, rfirst, rlast, ncells;
  uint64_t count = 0;
  void add(uint32_t l, uint32_t b, uint32_t p, uint32_t f, uint32_t t) {
    lag.push_back(l); block.push_back(b); pairs.push_back(p); first.push_back(f); last.push_back(t);
  }
  void end_recording() { off.push_back(lag.size()); }
  int32_t run(uint32_t lag_tol, uint32_t max_gap, uint64_t min_pairs, uint64_t cap) {
    for (auto* v : {&lag, &block, &pairs, &first, &last}) v->shrink_to_fit();
    off.shrink_to_fit();
    for (auto* v : {&rec, &rlag, &lo, &hi, &rfirst, &rlast, &ncells}) {
      v->assign(cap, 77);
      v->shrink_to_fit();
    }
    pairs_out.assign(cap, 77);
    pairs_out.shrink_to_fit();
    count = 77;
    return shz_repeats_fold(off.data(), (uint32_t)off.size() - 1, lag.data(), block.data(), pairs.data(), first.data(), last.data(),
                            lag_tol, max_gap, min_pairs, rec.data(), rlag.data(), lo.data(), hi.data(), rfirst.data(), rlast.data(),
                            pairs_out.data(), ncells.data(), cap, &count);
  }
};

int main() {
  {   // a repeat split over two lags, a second one on the same lags kept apart by time, a stray cell; a second recording
    cell_list L;
    L.add(258, 2, 60, 65, 95);
    L.add(258, 3, 200, 96, 127);
    L.add(258, 5, 150, 160, 191);    // block distance 2 = max_gap + 1: linked
    L.add(258, 9, 120, 288, 319);    // block distance 4: its own repeat
    L.add(259, 4, 90, 128, 159);
    L.add(700, 0, 99, 3, 9);         // 99 pairs: below min_pairs
    L.end_recording();
    L.end_recording();               // a recording without cells
    L.add(258, 2, 100, 64, 64);
    L.end_recording();
    EXPECT(L.run(1, 1, 100, 8) == SHZ_OK && L.count == 3);
    EXPECT(L.rec[0] == 0 && L.rlag[0] == 258 && L.lo[0] == 258 && L.hi[0] == 259 && L.rfirst[0] == 65 && L.rlast[0] == 191);
    EXPECT(L.pairs_out[0] == 500 && L.ncells[0] == 4);
    EXPECT(L.rec[1] == 0 && L.rfirst[1] == 288 && L.rlast[1] == 319 && L.pairs_out[1] == 120 && L.ncells[1] == 1);
    EXPECT(L.rec[2] == 2 && L.rfirst[2] == 64 && L.rlast[2] == 64 && L.pairs_out[2] == 100 && L.rec[3] == 77);
    // the same with exactly the room, with one too few and with none
    EXPECT(L.run(1, 1, 100, 3) == SHZ_OK && L.count == 3 && L.rec[2] == 2);
    EXPECT(L.run(1, 1, 100, 2) == SHZ_E_CAPACITY && L.count == 3 && L.rec[1] == 0 && L.pairs_out[1] == 120);
    EXPECT(L.run(1, 1, 100, 0) == SHZ_E_CAPACITY && L.count == 3);
    EXPECT(shz_repeats_fold(L.off.data(), 3, L.lag.data(), L.block.data(), L.pairs.data(), L.first.data(), L.last.data(), 1, 1, 100,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &L.count) == SHZ_E_CAPACITY);
    // no tolerance: the lags fall apart; every cell on its own with no gap allowed and blocks two apart
    EXPECT(L.run(0, 1, 0, 8) == SHZ_OK && L.count == 5);
    EXPECT(L.run(0, 0, 0, 8) == SHZ_OK && L.count == 6);
  }
  {   // the widest tolerances, lags and blocks at the top of 32 bits: no sum wraps, no row is walked
    cell_list L;
    L.add(0, 0, 0xFFFFFFFFu, 0, 0);
    L.add(0, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFE0u, 0xFFFFFFFFu);
    L.add(0xFFFFFFFFu, 0, 0xFFFFFFFFu, 1, 2);
    L.add(0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu);
    L.end_recording();
    EXPECT(L.run(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 4) == SHZ_OK && L.count == 1);
    EXPECT(L.pairs_out[0] == 4ull * 0xFFFFFFFFull && L.ncells[0] == 4 && L.rlag[0] == 0 && L.hi[0] == 0xFFFFFFFFu);
    EXPECT(L.rfirst[0] == 0 && L.rlast[0] == 0xFFFFFFFFu);
    EXPECT(L.run(0xFFFFFFFEu, 0xFFFFFFFDu, 0, 4) == SHZ_OK && L.count == 4);
    EXPECT(L.run(0, 0, ~0ull, 4) == SHZ_OK && L.count == 0);
  }
  {   // nothing to fold
    cell_list L;
    EXPECT(L.run(1, 1, 100, 0) == SHZ_OK && L.count == 0);
    L.end_recording();
    EXPECT(L.run(1, 1, 100, 2) == SHZ_OK && L.count == 0 && L.rec[0] == 77);
  }
  {   // refusals write nothing
    cell_list L;
    L.add(10, 2, 5, 64, 70);
    L.add(10, 1, 5, 32, 40);         // blocks of one lag out of order
    L.end_recording();
    EXPECT(L.run(1, 1, 1, 2) == SHZ_E_INVALID && L.count == 77 && L.rec[0] == 77 && L.pairs_out[1] == 77);
    cell_list M;
    M.add(10, 1, 5, 41, 40);         // first > last
    M.end_recording();
    EXPECT(M.run(1, 1, 1, 2) == SHZ_E_INVALID && M.count == 77);
    cell_list O;
    O.add(10, 1, 5, 32, 40);
    O.end_recording();
    O.off[0] = 1;                    // a CSR that does not start at 0
    EXPECT(O.run(1, 1, 1, 2) == SHZ_E_INVALID && O.count == 77);
    O.off[0] = 0;
    EXPECT(shz_repeats_fold(O.off.data(), 1, O.lag.data(), O.block.data(), O.pairs.data(), O.first.data(), O.last.data(), 1, 1, 1,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, &O.count) == SHZ_E_INVALID);
    EXPECT(shz_repeats_fold(O.off.data(), 1, nullptr, O.block.data(), O.pairs.data(), O.first.data(), O.last.data(), 1, 1, 1,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &O.count) == SHZ_E_INVALID);
    EXPECT(shz_repeats_fold(O.off.data(), 1, O.lag.data(), O.block.data(), O.pairs.data(), O.first.data(), O.last.data(), 1, 1, 1,
                            nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) == SHZ_E_INVALID);
    EXPECT(shz_repeats_fold(nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr, 1, 1, 1, nullptr, nullptr, nullptr, nullptr,
                            nullptr, nullptr, nullptr, nullptr, 0, &O.count) == SHZ_E_INVALID);
    EXPECT(O.count == 77);
  }
  printf("repeats fold check OK\n");
  return 0;
}
