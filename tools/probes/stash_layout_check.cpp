// stash_layout_check.cpp -- host check of csrc/inr_stash.h (tests/test_stash_layout_host.py builds and runs it; exit status
// 0 = pass).
//   c++ -std=c++17 -I mri-implicit-neural-representations_amd/csrc tools/probes/stash_layout_check.cpp -o stash_layout_check
// Over a grid of shapes: every piece of a tile's stash starts inside [0, 2^31) floats (the host keeps offsets as int) at a
// multiple of 16 bytes, the pieces are pairwise disjoint and tile [0, floats_per_tile) without a hole or an overhang; the
// one alias (encoder features / WIRE2D's gradient copy) is the documented one.
// With an argument, a text file of lines "mlp NB TL NS D enc_rows" / "mfn NB TL S enc_rows": prints one line
// "floats_per_tile N" for each, for the test to hold against what the built library answers.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "inr_stash.h"

namespace {

struct Piece {
  std::string name;
  size_t off, floats;
};

int bad = 0;

void fail(const std::string& what, const std::string& why) {
  if (bad++ < 20) std::printf("%s: %s\n", what.c_str(), why.c_str());
}

// the pieces start in int range, 16-byte aligned, and tile [0, total) exactly
void check(const std::string& what, std::vector<Piece> p, size_t total) {
  for (const Piece& q : p) {
    if (q.off >= (size_t)1 << 31) fail(what, q.name + " starts outside [0, 2^31)");
    if ((q.off * sizeof(float)) % 16 != 0) fail(what, q.name + " is not 16-byte aligned");
    if (q.floats == 0) fail(what, q.name + " is empty");
  }
  std::sort(p.begin(), p.end(), [](const Piece& a, const Piece& b) { return a.off < b.off; });
  size_t end = 0;
  for (const Piece& q : p) {
    if (q.off < end) fail(what, q.name + " overlaps the piece before it");
    if (q.off > end) fail(what, "hole before " + q.name);
    end = q.off + q.floats;
  }
  if (total > 0x7fffffff) fail(what, "floats_per_tile does not fit the int the host keeps it in");
  if (end != total) fail(what, "pieces end at " + std::to_string(end) + ", floats_per_tile is " + std::to_string(total));
}

void check_mlp(int NB, int TL, inr::StashFamily fam, int D, int enc_rows) {
  const inr::MlpStash st(NB, TL, fam);
  char what[96];
  std::snprintf(what, sizeof(what), "mlp NB %d TL %d NS %d D %d enc_rows %d", NB, TL, (int)fam, D, enc_rows);
  const size_t T = (size_t)st.tensor_floats();
  std::vector<Piece> p;
  for (int l = 0; l <= D - 2; ++l)
    for (int s = 0; s < st.NS; ++s) p.push_back({"layer " + std::to_string(l) + " slot " + std::to_string(s), st.slot(l, s), T});
  p.push_back({"last_dact", st.last_dact(D), (size_t)4 * TL});
  if (enc_rows != 0) p.push_back({"enc", st.enc(D), (size_t)enc_rows * TL});
  if (fam == inr::STASH_GABOR2D) p.push_back({"grad_copy", st.grad_copy(D), T});
  check(what, p, st.floats_per_tile(D, enc_rows));
  if (st.enc(D) != st.grad_copy(D)) fail(what, "enc and grad_copy differ");  // the documented alias: never both in a plan
  if (st.slot(0, st.H) != 0 || st.slot(0, st.ORTH) != 5 * T || st.slot(1, st.H) != st.NS * T) fail(what, "slots are not NS * l + s tensors in");
  // the named slots exist in the family that uses them
  const int last = fam == inr::STASH_REAL ? st.DACT : (fam == inr::STASH_GABOR ? st.DB : st.Q);
  if (last != st.NS - 1) fail(what, "the family's last named slot is not its last tensor");
}

void check_mfn(int NB, int TL, int S, int enc_rows) {
  const inr::MfnStash st(NB, TL);
  char what[96];
  std::snprintf(what, sizeof(what), "mfn NB %d TL %d S %d enc_rows %d", NB, TL, S, enc_rows);
  const size_t T = (size_t)st.tensor_floats();
  std::vector<Piece> p;
  for (int i = 0; i < S; ++i)
    for (int s : {st.F, st.LCOS, st.HH}) p.push_back({"stage " + std::to_string(i) + " slot " + std::to_string(s), st.slot(i, s), T});
  p.push_back({"enc", st.enc(S), (size_t)enc_rows * TL});
  p.push_back({"x2", st.x2(S, enc_rows), (size_t)TL});  // Gabor filters read it; the plain filters' tiles carry it unused
  check(what, p, st.floats_per_tile(S, enc_rows));
  if (st.slot(0, st.F) != 0 || st.slot(1, st.HH) != 5 * T) fail(what, "slots are not 3 * stage + s tensors in");
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(inr::MlpStash::H == 0 && inr::MlpStash::DACT == 1 && inr::MlpStash::DA == 1 &&
                    inr::MlpStash::DB == 2 && inr::MlpStash::DA2 == 3 && inr::MlpStash::DB2 == 4 &&
                    inr::MlpStash::ORTH == 5 && inr::MlpStash::Q == 6,
                "MlpStash slots");
  static_assert(inr::MfnStash::F == 0 && inr::MfnStash::LCOS == 1 && inr::MfnStash::HH == 2, "MfnStash slots");
  static_assert(inr::MlpStash(8, 128, inr::STASH_REAL).floats_per_tile(5, 512) == 2 * 4 * 32768 + 4 * 128 + 512 * 128,
                "everything is constexpr");
  int cases = 0;
  for (int NB : {1, 2, 4, 8, 12, 16})
    for (int TL : {64, 128}) {
      for (int D : {2, 3, 8}) {
        for (int enc_rows : {0, 32, 512}) check_mlp(NB, TL, inr::STASH_REAL, D, enc_rows), ++cases;  // matrix / gauss input
        check_mlp(NB, TL, inr::STASH_GABOR, D, 0), ++cases;                                         // WIRE: matrix input only
        check_mlp(NB, TL, inr::STASH_GABOR2D, D, 0), ++cases;
      }
      for (int S : {1, 2, 8})
        for (int enc_rows : {32, 512}) check_mfn(NB, TL, S, enc_rows), ++cases;  // (one layout with and without Gabor)
    }
  if (argc == 2) {
    FILE* f = std::fopen(argv[1], "r");
    if (f == nullptr) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
    char kind[8];
    int v[5];
    while (std::fscanf(f, "%7s %d %d %d %d", kind, &v[0], &v[1], &v[2], &v[3]) == 5) {
      if (std::strcmp(kind, "mlp") == 0 && std::fscanf(f, "%d", &v[4]) == 1) {
        // NS names the family: a StashFamily's value is its tensors per layer, and nothing else is one
        if (v[2] != inr::STASH_REAL && v[2] != inr::STASH_GABOR && v[2] != inr::STASH_GABOR2D)
          return std::fprintf(stderr, "NS %d is no stash family\n", v[2]), 2;
        check_mlp(v[0], v[1], (inr::StashFamily)v[2], v[3], v[4]);
        std::printf("floats_per_tile %zu\n", inr::MlpStash(v[0], v[1], (inr::StashFamily)v[2]).floats_per_tile(v[3], v[4]));
      } else if (std::strcmp(kind, "mfn") == 0) {
        check_mfn(v[0], v[1], v[2], v[3]);
        std::printf("floats_per_tile %zu\n", inr::MfnStash(v[0], v[1]).floats_per_tile(v[2], v[3]));
      } else {
        return std::fprintf(stderr, "bad line in %s\n", argv[1]), 2;
      }
    }
    std::fclose(f);
  }
  std::printf("%d grid cases: %s (%d failures)\n", cases, bad ? "FAILED" : "ok", bad);
  return bad ? 1 : 0;
}
