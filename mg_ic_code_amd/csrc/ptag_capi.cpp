// ptag_capi.cpp -- the C ABI of libmgic_ptag.so (include/mgic_ptag.h) over the
// launcher of ptag.hip.  Fields are reached through libmgic's C ABI alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_ptag.h"
#include "launch_ledger.hpp"
#include "ptag.hpp"

namespace {

using mgic::ptag::Args;
using mgic::ptag::Tile;

thread_local std::string g_err;

struct PtagError : std::runtime_error {
  int code;
  PtagError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const PtagError &e) {
    g_err = e.what();
    return e.code;
  } catch (const std::invalid_argument &e) {
    g_err = e.what();
    return MGIC_EBADARG;
  } catch (const std::exception &e) {
    g_err = e.what();
    return MGIC_EUNKNOWN;
  } catch (...) {
    g_err = "unknown exception";
    return MGIC_EUNKNOWN;
  }
}

void need(const void *p, const char *name) {
  if (!p) throw PtagError(MGIC_EBADARG, std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw PtagError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw PtagError(MGIC_EUNKNOWN, std::string(what) + ": " + hipGetErrorString(e));
}

inline int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// this library's device scratch: the mask and the tile table, grown on demand
// and freed when the library unloads
struct Buf {
  void *p = nullptr;
  size_t n = 0;
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  void *at_least(size_t bytes) {
    if (bytes > n) {
      if (p) hip(hipFree(p), "hipFree");
      p = nullptr;
      n = 0;
      hip(hipMalloc(&p, bytes), "hipMalloc");
      n = bytes;
    }
    return p;
  }
};
Buf g_mask, g_tiles;
// the table on the host: it outlives the asynchronous upload
std::vector<Tile> g_table;

}  // namespace

extern "C" {

MGIC_PTAG_API const char *mgic_ptag_last_error(void) { return g_err.c_str(); }

MGIC_PTAG_API int mgic_ptag_lattice(mgic_comm c, mgic_field cond, double tag_val, int grow,
                                    int spacing, int lat_lo[3], int lat_n[3],
                                    unsigned char *mask_host) {
  return guard([&] {
    need(c, "comm");
    need(cond, "cond");
    need(lat_lo, "lat_lo");
    need(lat_n, "lat_n");
    if (grow < 0 || grow > (1 << 20)) throw PtagError(MGIC_EBADARG, "grow must be >= 0");
    if (spacing < 1) throw PtagError(MGIC_EBADARG, "lattice spacing must be >= 1");
    int domain[6], periodic[3], nbox = 0;
    mg(mgic_field_layout(cond, domain, periodic, nullptr, &nbox, nullptr, nullptr));
    if (nbox < 1) throw PtagError(MGIC_EBADARG, "the level has no boxes");
    // every box of the level (all ranks): the bounding box, and the local
    // ones' tiles
    int blo[3], bhi[3], nz_max = 0;
    g_table.clear();
    for (int i = 0; i < nbox; ++i) {
      int lohi[6], owner = 0, li = -1;
      mg(mgic_field_box(cond, i, lohi, &owner, &li));
      for (int d = 0; d < 3; ++d) {
        blo[d] = i == 0 ? lohi[d] : std::min(blo[d], lohi[d]);
        bhi[d] = i == 0 ? lohi[3 + d] : std::max(bhi[d], lohi[3 + d]);
      }
      if (li < 0 || !mask_host) continue;
      long st[3];
      double *p = nullptr;
      mg(mgic_field_device_ptr(cond, li, &p, st));
      Tile t;
      t.p = p;
      t.sy = st[1];
      t.sz = st[2];
      for (int d = 0; d < 3; ++d) {
        t.glo[d] = lohi[d];
        t.n[d] = lohi[3 + d] - lohi[d] + 1;
      }
      if (t.n[0] <= 0 || t.n[1] <= 0 || t.n[2] <= 0) continue;
      nz_max = std::max(nz_max, t.n[2]);
      for (t.j0 = 0; t.j0 < t.n[1]; t.j0 += mgic::ptag::kTileY)
        for (t.i0 = 0; t.i0 < t.n[0]; t.i0 += mgic::ptag::kTileX) g_table.push_back(t);
    }
    // the lattice: the whole domain in a periodic direction; else the
    // bounding box grown and clipped to the domain, in lattice cells
    Args a;
    long cells = 1;
    for (int d = 0; d < 3; ++d) {
      const int dlo = domain[d], dhi = domain[3 + d];
      if (periodic[d]) {
        if (fdiv(dlo, spacing) * spacing != dlo || fdiv(dhi + 1, spacing) * spacing != dhi + 1)
          throw PtagError(MGIC_EBADARG,
                          "regrid: a level's domain is not a multiple of the lattice spacing");
        lat_lo[d] = fdiv(dlo, spacing);
        lat_n[d] = fdiv(dhi + 1, spacing) - lat_lo[d];
      } else {
        const int lo = std::max(blo[d] - grow, dlo), hi = std::min(bhi[d] + grow, dhi);
        lat_lo[d] = fdiv(lo, spacing);
        lat_n[d] = fdiv(hi, spacing) - lat_lo[d] + 1;
      }
      if (lat_n[d] < 1) throw PtagError(MGIC_EBADARG, "the level has an empty lattice");
      cells *= lat_n[d];
      a.dom_lo[d] = dlo;
      a.dom_hi[d] = dhi;
      a.lat_lo[d] = lat_lo[d];
      a.lat_n[d] = lat_n[d];
      a.periodic[d] = periodic[d] ? 1 : 0;
    }
    a.grow = grow;
    a.c = spacing;
    if (!mask_host) return;  // the size query
    void *s = nullptr;
    mg(mgic_comm_get_stream(c, &s));
    const hipStream_t st = static_cast<hipStream_t>(s);
    unsigned char *d = static_cast<unsigned char *>(g_mask.at_least((size_t)cells));
    hip(hipMemsetAsync(d, 0, (size_t)cells, st), "hipMemsetAsync");
    if (!g_table.empty()) {
      const size_t bytes = g_table.size() * sizeof(Tile);
      Tile *dt = static_cast<Tile *>(g_tiles.at_least(bytes));
      hip(hipMemcpyAsync(dt, g_table.data(), bytes, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
      mgic::ptag::tag_lattice(d, dt, (int)g_table.size(), nz_max, tag_val, a, st);
    }
    hip(hipMemcpyAsync(mask_host, d, (size_t)cells, hipMemcpyDeviceToHost, st), "hipMemcpyAsync");
    hip(hipStreamSynchronize(st), "hipStreamSynchronize");
  });
}

MGIC_PTAG_API int mgic_ptag_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw PtagError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_PTAG_API int mgic_ptag_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
