// lds_layout_check.cpp -- host check of csrc/inr_lds.h (tests/test_lds_layout_host.py builds and runs it; exit status
// 0 = pass).
//   c++ -std=c++17 -I mri-implicit-neural-representations_amd/csrc tools/probes/lds_layout_check.cpp -o lds_layout_check
// Over every shape a kernel is instantiated for and a grid of encoder sizes: the pieces of the dynamic LDS block are
// pairwise disjoint and tile [0, bytes) without a hole or an overhang; every piece the kernel reads 16 bytes at a time or
// fills by LDS-DMA starts on 16 bytes; the narrow MLP's option predicates say "fits" exactly where bytes <= the CU's LDS.
// Prints "bytes <shape> : N" for every launch size of the grid (the test holds them against tests/golden/lds_layout.json)
// and, per narrow-MLP instantiation, "threshold ..." with the first encoder size (multiples of 8) at which the dZ_last
// images, the last-layer fragments and the launch itself no longer fit (-1: none up to 2^16).
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "inr_lds.h"

namespace {

struct Piece {
  std::string name;
  size_t off, bytes;  // from the block's start
  bool vec;           // read 16 bytes at a time, or an LDS-DMA destination
};

int bad = 0;

void fail(const std::string& what, const std::string& why) {
  if (bad++ < 20) std::printf("%s: %s\n", what.c_str(), why.c_str());
}

Piece fl(const char* name, int off, int floats, bool vec) { return {name, (size_t)off * 4, (size_t)floats * 4, vec}; }

// empty pieces (no encoder) are left out; the rest tile [0, total) exactly
void check(const std::string& what, std::vector<Piece> p, size_t total) {
  p.erase(std::remove_if(p.begin(), p.end(), [](const Piece& q) { return q.bytes == 0; }), p.end());
  for (const Piece& q : p)
    if (q.vec && q.off % 16 != 0) fail(what, q.name + " is not 16-byte aligned");
  std::sort(p.begin(), p.end(), [](const Piece& a, const Piece& b) { return a.off < b.off; });
  size_t end = 0;
  for (const Piece& q : p) {
    if (q.off < end) fail(what, q.name + " overlaps the piece before it");
    if (q.off > end) fail(what, "hole before " + q.name);
    end = q.off + q.bytes;
  }
  if (end != total) fail(what, "pieces end at " + std::to_string(end) + ", bytes is " + std::to_string(total));
  std::printf("bytes %s : %zu\n", what.c_str(), total);
}

const int ENC[] = {0, 8, 64, 256, 512, 640, 1024};  // 0: no fused encoder (matrix input)

void check_mlp(int NB, int NW, int LD) {
  char what[96];
  for (int E : ENC)
    for (int opt = 0; opt < 3; ++opt) {  // nothing | ll | ll + dz
      const inr::MlpLds L(NB, NW, E != 0, E, LD);
      const bool ll = opt >= 1, dz = opt == 2;
      std::snprintf(what, sizeof(what), "mlp nb %d nw %d ld %d E %d ll %d dz %d", NB, NW, LD, E, ll, dz);
      std::vector<Piece> p;
      for (int w = 0; w < NW; ++w) p.push_back(fl("image", L.image(w), L.image_floats(), true));
      p.push_back(fl("enc", L.enc(), L.EF, false));
      if (ll) p.push_back(fl("last_frag", L.last_frag(), L.last_frag_floats(), true));
      for (int w = 0; dz && w < NW; ++w) p.push_back(fl("dz_image", L.dz_image(w), L.dz_image_floats(), true));
      check(what, p, L.bytes(ll, dz));
      if (L.ll_fits() != (L.bytes(true, false) <= inr::LDS_BYTES_PER_CU)) fail(what, "ll_fits disagrees with bytes");
      if (L.dz_fits() != (L.bytes(true, true) <= inr::LDS_BYTES_PER_CU)) fail(what, "dz_fits disagrees with bytes");
      if (L.dz_fits() && !L.ll_fits()) fail(what, "dz fits where ll does not");
    }
  int dz_off = -1, ll_off = -1, base_off = -1;
  for (int E = (1 << 16); E >= 8; E -= 8) {
    const inr::MlpLds L(NB, NW, true, E, LD);
    if (!L.dz_fits()) dz_off = E;
    if (!L.ll_fits()) ll_off = E;
    if (L.bytes(false, false) > inr::LDS_BYTES_PER_CU) base_off = E;
  }
  std::printf("threshold mlp nb %d nw %d ld %d : dz_off %d ll_off %d base_off %d\n", NB, NW, LD, dz_off, ll_off, base_off);
}

void check_wide(int NB, int LD) {
  char what[96];
  for (int eager = 0; eager < 2; ++eager)
    for (int E : ENC) {
      const inr::MlpWideLds L(NB, E != 0, E, eager != 0, LD);
      std::snprintf(what, sizeof(what), "wide nb %d ld %d E %d eager %d", NB, LD, E, eager);
      std::vector<Piece> p;
      for (int g = 0; g < L.NG; ++g) p.push_back(fl("image", L.image(g), L.image_floats(), true));
      p.push_back(fl("enc", L.enc(), L.EF, false));
      if (eager) p.push_back(fl("last_frag", L.last_frag(), L.last_frag_floats(), true));
      if (eager) p.push_back(fl("pair_exchange", L.pair_exchange(), L.pair_exchange_floats(), false));
      check(what, p, L.bytes());
    }
}

void check_mfn(int NB, int N, int LD) {
  char what[96];
  for (int E : {0, 8, 13, 64, 256, 512, 640, 1024}) {  // 13: the encoder matrix is the last piece, of any size
    const inr::MfnLds L(NB, N, E != 0, E, LD);
    std::snprintf(what, sizeof(what), "mfn nb %d n %d ld %d E %d", NB, N, LD, E);
    std::vector<Piece> p;
    for (int w = 0; w < N; ++w) p.push_back(fl("image", L.image(w), L.image_floats(), true));
    for (int w = 0; w < N; ++w) p.push_back(fl("head_grad", L.head_grad(w), L.head_grad_floats(), true));
    p.push_back(fl("enc", L.enc(), L.EF, false));
    check(what, p, L.bytes());
  }
}

void check_rs(int MO) {
  char what[96];
  for (int E : ENC) {
    if (E == 0) continue;  // the row-split step always has the fused encoder
    const inr::RsLds L(E, MO);
    std::snprintf(what, sizeof(what), "rs E %d mo %d", E, MO);
    check(what, {fl("image", L.image(), inr::RS_IMG_FLOATS, true), fl("enc", L.enc(), L.EF, false),
                 fl("w_last", L.w_last(), L.w_last_floats(), true), fl("dz_last", L.dz_last(), L.dz_last_floats(), true),
                 fl("red", L.red(), L.red_floats(), false), fl("part", L.part(), L.part_floats(), true)},
          L.bytes());
  }
}

void check_bf16(int D) {
  char what[96];
  for (int E : ENC) {
    if (E == 0) continue;
    const inr::SirenBf16Lds L(D, E);
    std::snprintf(what, sizeof(what), "bf16 D %d E %d", D, E);
    check(what, {{"ring", (size_t)L.ring(), (size_t)L.ring_end(), true},
                 {"bias", (size_t)L.bias(), (size_t)D * 256 * 4, true},
                 {"enc", (size_t)L.enc(), (size_t)E * 16, true},
                 {"red", (size_t)L.red(), (size_t)2 * inr::PN_WAVES * 4, false}},
          L.bytes());
  }
}

void check_dwgb() {
  char what[96];
  for (int E : ENC) {
    const inr::DwGemmBf16Lds L(E);
    std::snprintf(what, sizeof(what), "dwgb E %d", E);
    check(what, {{"stage 0", (size_t)L.stages(), (size_t)L.stage_bytes(), true},
                 {"stage 1", (size_t)L.stages() + L.stage_bytes(), (size_t)L.stage_bytes(), true},
                 {"xs", (size_t)L.xs(), (size_t)L.xs_bytes(), false},
                 {"enc", (size_t)L.enc(), (size_t)E * 12, false}},
          L.bytes());
  }
}

}  // namespace

int main() {
  static_assert(inr::MlpLds(8, 4, true, 256).bytes(true, true) == (4 * 8 * 32 * 36 + 768 + 1028 + 4 * 8 * 36) * 4,
                "everything is constexpr");
  static_assert(inr::SirenBf16Lds::ring_end() == 8 * 16384 && inr::RsLds(512).bytes() <= inr::LDS_BYTES_PER_CU, "");
  for (int NB : {1, 2, 4, 8}) check_mlp(NB, 4, 36);   // inr_mlp_nb*.hip, inr_wire_nb*.hip, inr_wire2d_nb*.hip
  for (int NB : {12, 16}) check_wide(NB, 36);         // inr_wire_nb12.hip; inr_mlp_nb16.hip, inr_wire2d_nb16.hip
  check_mfn(1, 4, 36), check_mfn(4, 4, 36), check_mfn(8, 4, 33), check_mfn(16, 2, 36);  // inr_mfn_nb*.hip
  // every number of output rows the row-split kernel's last layer may compute; a launch reserves RS_MO_MAX of them, the
  // one size the test pins
  for (int MO = 1; MO <= inr::RS_MO_MAX; ++MO) check_rs(MO);
  for (int D = 3; D <= 8; ++D) check_bf16(D);
  check_dwgb();
  std::printf("lds layouts: %s (%d failures)\n", bad ? "FAILED" : "ok", bad);
  return bad ? 1 : 0;
}
