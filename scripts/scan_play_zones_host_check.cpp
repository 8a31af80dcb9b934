// Stand-alone host check of shz_scan_play_zones (no GPU is touched) on hand-built segment lists, meant to be built with the
// host sanitizers and run on a CPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-omit-frame-pointer -c shazam_amd/csrc/shz_scan.hip -o shz_scan.san.o
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -c scripts/scan_play_zones_host_check.cpp -o main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined main.o shz_scan.san.o \
//         <the library's other objects from shazam_amd/csrc> -ldl -o play_zones_check && ./play_zones_check
// Exit status 0 and "play zones check OK" mean every expectation held and the sanitizers reported nothing.
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

struct play_list {   // exactly sized heap arrays: a read or write past an end is the sanitizer's to report
  std::vector<uint32_t> rec, sid, first, last, t16, lo, hi, cn;
  std::vector<int32_t> pa, pb, dlo, dhi;
  std::vector<uint64_t> wlo, whi;
  void add(uint32_t r, uint32_t s, uint32_t a, uint32_t b, int32_t p_a, int32_t p_b, uint32_t t) {
    rec.push_back(r); sid.push_back(s); first.push_back(a); last.push_back(b); pa.push_back(p_a); pb.push_back(p_b); t16.push_back(t);
  }
  int32_t run(const std::vector<uint64_t>& frames, uint32_t W, uint32_t S, uint32_t M, uint32_t w) {
    const size_t n = 3 * rec.size();
    lo.assign(n, 77); hi.assign(n, 77); cn.assign(n, 77); dlo.assign(n, 77); dhi.assign(n, 77); wlo.assign(n, 77); whi.assign(n, 77);
    lo.shrink_to_fit(); hi.shrink_to_fit(); cn.shrink_to_fit(); dlo.shrink_to_fit(); dhi.shrink_to_fit(); wlo.shrink_to_fit();
    whi.shrink_to_fit();
    return shz_scan_play_zones(rec.data(), sid.data(), first.data(), last.data(), pa.data(), pb.data(), t16.data(), rec.size(),
                               frames.data(), (uint32_t)frames.size(), W, S, M, w, lo.data(), hi.data(), wlo.data(), whi.data(),
                               dlo.data(), dhi.data(), cn.data());
  }
  bool untouched() const {
    for (size_t i = 0; i < lo.size(); ++i)
      if (lo[i] != 77 || hi[i] != 77 || cn[i] != 77 || dlo[i] != 77 || dhi[i] != 77 || wlo[i] != 77 || whi[i] != 77) return false;
    return true;
  }
};

int main() {
  {   // one song twice in a recording at different positions (the clamp is by (rec, sid)), another between, a second recording
    play_list L;
    L.add(0, 2, 0, 3, -43, -8, 68289);
    L.add(0, 5, 5, 7, 7, 30, 32768);
    L.add(0, 2, 9, 12, 300, 340, 76548);
    L.add(2, 2, 1, 1, 5, 5, 131072);
    EXPECT(L.run({400, 0, 60}, 43, 11, 40, 3) == SHZ_OK);
    EXPECT(L.lo[0] == 0 && L.hi[0] == 99 && L.hi[1] == 43 && L.lo[2] == 33 && L.lo[6] == 76 && L.hi[6] == 215 && L.lo[8] == 132);
    EXPECT(L.wlo[3] == 8 && L.whi[3] == 80);                                  // W(15), W(160) at factor 1/2
    EXPECT(L.wlo[9] == 0 && L.whi[9] == 120 && L.wlo[11] == 22 && L.whi[10] == 108);   // factor 2
    // segment 0: W(33) = 34 at 68289; c_a = -43, c_b = -8 - 34 = -42 on the zones that start at 0; the tail starts at 33
    EXPECT(L.dlo[0] == -46 && L.dhi[0] == -39 && L.dlo[1] == -46 && L.dhi[1] == -40 && L.dlo[2] == -42 + 34 - 3 && L.dhi[2] == -42 + 34 + 3);
    EXPECT(L.cn[0] == 1 && L.cn[11] == 1);
  }
  {   // windows behind the end and at the top of 32 bits; candidates at both ends of int32
    play_list L;
    L.add(0, 1, 2, 5, 10, 100, 70000);
    L.add(0, 1, 0xFFFFFFF0u, 0xFFFFFFFFu, 0, 0, 131072);
    EXPECT(L.run({100}, 10, 30, 0xFFFFFFFFu, 1) == SHZ_OK);
    EXPECT(L.lo[3] == 100 && L.hi[3] == 100 && L.cn[3] == 0 && L.cn[4] == 0 && L.cn[5] == 0 && L.dlo[3] == 0 && L.dhi[5] == 0);
    play_list E;
    E.add(0, 1, 0, 2, INT32_MAX, INT32_MAX - 5, 65536);
    E.add(0, 2, 5, 6, INT32_MIN, INT32_MIN, 32768);
    EXPECT(E.run({0xFFFFFFFFull}, 20, 10, 30, 7) == SHZ_OK);
    EXPECT(E.cn[0] == 1 && E.dhi[0] == INT32_MAX && E.dhi[1] == INT32_MAX && E.dlo[1] == INT32_MAX - 7);
    EXPECT(E.cn[3] == 0 && E.cn[4] == 0 && E.cn[5] == 1 && E.dlo[5] == INT32_MIN && E.dhi[5] == INT32_MIN + 7);
    play_list T;                                                              // a S far above 2^40: saturated, no candidate
    T.add(0, 1, 0xFFFFFFF0u, 0xFFFFFFFFu, INT32_MAX, INT32_MAX, 131072);
    EXPECT(T.run({0xFFFFFFFFull}, 10, 0xFFFFFFFFu, 0, 0xFFFFFFFFu) == SHZ_OK);
    EXPECT(T.cn[0] == 0 && T.cn[1] == 0 && T.cn[2] == 0 && T.lo[0] == 0xFFFFFFFFu && T.hi[2] == 0xFFFFFFFFu && T.wlo[0] == 0x1FFFFFFFEull);
  }
  {   // refusals write nothing
    play_list L;
    L.add(0, 1, 4, 3, 0, 0, 65536);
    EXPECT(L.run({100}, 10, 30, 0, 0) == SHZ_E_INVALID && L.untouched());
    play_list F;
    F.add(0, 1, 0, 1, 0, 0, 65536);
    F.add(0, 2, 2, 3, 0, 0, 131073);
    EXPECT(F.run({100}, 10, 30, 0, 0) == SHZ_E_INVALID && F.untouched());
    F.t16[1] = 32767;
    EXPECT(F.run({100}, 10, 30, 0, 0) == SHZ_E_INVALID && F.untouched());
    play_list Z;
    Z.add(0, 1, 0, 0, 0, 0, 131072);
    EXPECT(Z.run({1u << 19}, 1u << 19, 1, 0, 0) == SHZ_E_UNSUPPORTED && Z.untouched());
    EXPECT(Z.run({(1u << 19) - 1}, 1u << 19, 1, 0, 0) == SHZ_OK && Z.whi[0] == (1u << 20) - 2);
    play_list D;
    D.add(0, 1, 0, 4, 0, 40 + 4096 - 6, 65536);
    EXPECT(D.run({400}, 20, 10, 0, 3) == SHZ_E_UNSUPPORTED && D.untouched());
    D.pb[0] -= 1;
    EXPECT(D.run({400}, 20, 10, 0, 3) == SHZ_OK && D.dhi[0] - D.dlo[0] == 4095);
    EXPECT(D.run({400}, 20, 10, 0, 0xFFFFFFFFu) == SHZ_E_UNSUPPORTED && D.untouched());
    EXPECT(shz_scan_play_zones(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, 10, 30, 0, 0, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr) == SHZ_OK);
    EXPECT(shz_scan_play_zones(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, 0, 10, 30, 0, 0, nullptr, nullptr,
                               nullptr, nullptr, nullptr, nullptr, nullptr) == SHZ_E_INVALID);
  }
  printf("play zones check OK\n");
  return 0;
}
