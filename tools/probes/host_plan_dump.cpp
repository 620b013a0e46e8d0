// host_plan_dump.cpp -- dumps what the host layer derives for a list of plan descriptions, one digest per line, so that two
// commits' host layers can be compared line for line: NetDesc, packed size, weight-gradient route, the fp32 GEMM's items
// and, per batch size and INR_RS / INR_OVERLAP setting, every member of the call's CallLayout.  Creating and sizing a plan
// touches no GPU.  Built from the csrc directory, against the split host layer
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I . \
//     ../../tools/probes/host_plan_dump.cpp inr_plan.hip inr_layout.hip inr_dw_gemm.hip \
//     -Wl,--unresolved-symbols=ignore-all -o host_plan_dump
// or against a commit whose host layer is one file, whose internals are then visible by inclusion:
//   ... -DHOST_DUMP_ONE_FILE='"/path/to/that/csrc/inr_api.hip"' -I /path/to/that/csrc host_plan_dump.cpp \
//     /path/to/that/csrc/inr_dw_gemm.hip ...
// usage: host_plan_dump DESCRIPTIONS  -- a text file, one plan per line: the 13 values of tests/layout_table.py DESC_FIELDS,
// then 1 if INR_GEMM_ONE_CLASS is set at creation, else 0 (written by a few lines of Python from layout_table.plans()).
#ifdef HOST_DUMP_ONE_FILE
#include HOST_DUMP_ONE_FILE
#else
#include "inr_host.h"
#endif

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

const long long kB[] = {0, 1, 100, 129, 4133, 19200, 25000, 38400, 65536, 100000, 235520, 3532800};  // layout_table.B_VALUES
const char* const kSwitches[][2] = {{nullptr, nullptr}, {nullptr, "0"}, {"0", nullptr},
                                    {"0", "0"},         {"1", nullptr}, {"1", "0"}};  // (INR_RS, INR_OVERLAP)

struct Digest {  // FNV-1a, 64 bits
  unsigned long long h = 1469598103934665603ull;
  void bytes(const void* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
  }
  template <class T>
  void put(const T& v) {  // scalars only: no padding enters
    static_assert(std::is_arithmetic<T>::value || std::is_pointer<T>::value, "scalar members only");
    bytes(&v, sizeof(v));
  }
};

void put(Digest& d, const inr::SlabSplit& s) {
  d.put(s.lo), d.put(s.hi), d.put(s.n2), d.put(s.mask), d.put(s.lo3), d.put(s.hi3), d.put(s.n3);
}

void put(Digest& d, const inr::DwGemmArgs& g) {
  d.put(g.dbg), d.put(g.dbg_cap), d.put(g.save), d.put(g.slabs), d.put(g.save_floats_per_tile), d.put(g.slab_floats);
  d.put(g.n_tiles), d.put(g.n_chunks), d.put(g.tiles_per_chunk), d.put(g.tile0), d.put(g.TL), d.put(g.WB), d.put(g.WBM);
  d.put(g.n_items), d.put(g.units), d.put(g.blocks_per_chunk), d.put(g.place);
  for (const inr::DwGemmItem& it : g.it) {
    d.put(it.g_off), d.put(it.h_off), d.put(it.gw_off), d.put(it.gb_off), d.put(it.Mblk), d.put(it.Kblk), d.put(it.K);
    d.put(it.mt), d.put(it.nt), d.put(it.unit0);
  }
}

void put(Digest& d, const inr::DwGemmBf16Args& g) {
  d.put(g.dbg), d.put(g.dbg_cap), d.put(g.save), d.put(g.slabs), d.put(g.coords), d.put(g.encB), d.put(g.dz_state);
  d.put(g.dz_count), d.put(g.B), d.put(g.save_floats_per_tile), d.put(g.slab_floats), d.put(g.n_tiles);
  d.put(g.n_enc_units), d.put(g.n_chunks_enc), d.put(g.tiles_per_chunk_enc), d.put(g.n_chunks), d.put(g.tiles_per_chunk);
  d.put(g.TL), d.put(g.E), d.put(g.n_units);
  for (const inr::DwGemmBf16Unit& u : g.unit)
    d.put(u.dz_off), d.put(u.z_off), d.put(u.gw_off), d.put(u.gb_off), d.put(u.M), d.put(u.K), d.put(u.n0);
}

void set_env(const char* name, const char* value) {
  if (value != nullptr)
    setenv(name, value, 1);
  else
    unsetenv(name);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return std::fprintf(stderr, "usage: %s DESCRIPTIONS\n", argv[0]), 2;
  FILE* f = std::fopen(argv[1], "r");
  if (f == nullptr) return std::fprintf(stderr, "cannot read %s\n", argv[1]), 2;
  for (const char* k : {"INR_RS", "INR_OVERLAP", "INR_GEMM_ONE_CLASS", "INR_GEMM_ENC_COST"}) unsetenv(k);
  int n = 0, one_class;
  inr_net_desc d;
  std::memset(&d, 0, sizeof(d));
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %f %f %f %f %d %d", &d.kind, &d.in_features, &d.width, &d.depth,
                     &d.out_features, &d.last_act, &d.input, &d.enc_size, &d.w0, &d.first_omega_0, &d.hidden_omega_0,
                     &d.scale_0, &d.precision, &one_class) == 14) {
    set_env("INR_GEMM_ONE_CLASS", one_class ? "1" : nullptr);
    inr_plan* plan = nullptr;
    const int rc = inr_plan_create(&d, &plan);
    unsetenv("INR_GEMM_ONE_CLASS");
    char msg[512] = "";
    if (rc != INR_OK) inr_last_error(msg, sizeof(msg));
    std::printf("plan %d one_class %d: create %d %s\n", n, one_class, rc, msg);
    ++n;
    if (rc != INR_OK) continue;
    Digest nd;
    nd.bytes(&plan->nd, sizeof(NetDesc));  // (zero-filled before it is built: its padding is comparable)
    Digest gemm;
    put(gemm, plan->gemm), put(gemm, plan->gemm_cover);
    std::printf("  NetDesc %zu bytes %016llx  packed_floats %lld  dw_route %d  gemm %d items %016llx\n", sizeof(NetDesc),
                nd.h, (long long)plan->packed_floats, plan->dw_route, plan->gemm.n_items, gemm.h);
    for (const long long B : kB) {
      for (const auto& sw : kSwitches) {
        set_env("INR_RS", sw[0]), set_env("INR_OVERLAP", sw[1]);
        CallLayout c;
        std::memset(static_cast<void*>(&c), 0, sizeof(c));  // members a route leaves alone compare as zeros
        if (const int brc = begin_call(plan, B, "inr_plan_launch_dims", &c)) {
          inr_last_error(msg, sizeof(msg));
          std::printf("  B %lld INR_RS %s INR_OVERLAP %s: refused %d %s\n", B, sw[0] ? sw[0] : "-", sw[1] ? sw[1] : "-", brc,
                      msg);
          continue;
        }
        Digest l;
        l.put(c.nt), l.put(c.nb), l.put(c.save_slots), l.put(c.n_slabs), l.put(c.rs);
        l.put(c.rsched.grid), l.put(c.rsched.rounds), l.put(c.rsched.ncb), l.put(c.rsched.hi), l.put(c.rsched.lo);
        l.put(c.rsched.x);
        put(l, c.plain), put(l, c.plain_red);
        l.put(c.step.split), l.put(c.step.full), l.put(c.step.rem), l.put(c.step.tA);
        put(l, c.step.gA), put(l, c.step.gB), put(l, c.step.red);
        put(l, c.bf16), put(l, c.bf16_red);
        std::printf("  B %lld INR_RS %s INR_OVERLAP %s: nt %lld nb %lld slots %lld slabs %lld rs %d split %d  %016llx\n", B,
                    sw[0] ? sw[0] : "-", sw[1] ? sw[1] : "-", (long long)c.nt, (long long)c.nb, (long long)c.save_slots,
                    (long long)c.n_slabs, (int)c.rs, (int)c.step.split, l.h);
      }
    }
    unsetenv("INR_RS"), unsetenv("INR_OVERLAP");
    inr_plan_destroy(plan);
  }
  std::fclose(f);
  std::printf("%d plans\n", n);
  return 0;
}
