// khyb_capi.cpp -- the C ABI of libmgic_khyb.so (include/mgic_khyb.h) over the
// launcher of khyb.hip.  Fields are reached through libmgic's C ABI alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_khyb.h"
#include "khyb.hpp"
#include "launch_ledger.hpp"

namespace {

using mgic::khyb::Row;

thread_local std::string g_err;

struct KhybError : std::runtime_error {
  int code;
  KhybError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const KhybError &e) {
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
  if (!p) throw KhybError(MGIC_EBADARG, std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw KhybError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw KhybError(MGIC_EUNKNOWN, std::string(what) + ": " + hipGetErrorString(e));
}

struct LocalBox {
  int index;  // local box index (mgic_field_device_ptr)
  int nx, ny, nz;
  long sy, sz;
};
struct Layout {
  int domain[6], periodic[3], nbox = 0;
  double dx = 0.0;
  std::vector<int> boxes;  // 7 ints per box: lohi, owner
  std::vector<LocalBox> local;
};

Layout layout_of(mgic_field f, const char *name) {
  need(f, name);
  Layout L;
  int rank = 0, size = 1;
  mg(mgic_field_layout(f, L.domain, L.periodic, &L.dx, &L.nbox, &rank, &size));
  for (int i = 0; i < L.nbox; ++i) {
    int lohi[6], owner = 0, li = -1;
    mg(mgic_field_box(f, i, lohi, &owner, &li));
    L.boxes.insert(L.boxes.end(), lohi, lohi + 6);
    L.boxes.push_back(owner);
    if (li < 0)
      throw KhybError(MGIC_EBADARG, std::string("box ") + std::to_string(i) + " of " + name +
                                        " is not local: one rank holds the level");
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    L.local.push_back(LocalBox{li, lohi[3] - lohi[0] + 1, lohi[4] - lohi[1] + 1,
                               lohi[5] - lohi[2] + 1, st[1], st[2]});
  }
  return L;
}

void same_layout(const Layout &a, mgic_field f, const char *name) {
  const Layout b = layout_of(f, name);
  bool ok = a.nbox == b.nbox && a.dx == b.dx && a.boxes == b.boxes &&
            std::equal(a.domain, a.domain + 6, b.domain) &&
            std::equal(a.periodic, a.periodic + 3, b.periodic) && a.local.size() == b.local.size();
  for (size_t i = 0; ok && i < a.local.size(); ++i)
    ok = a.local[i].index == b.local[i].index && a.local[i].sy == b.local[i].sy &&
         a.local[i].sz == b.local[i].sz;
  if (!ok) throw KhybError(MGIC_EBADARG, std::string("layout mismatch: ") + name);
}

double *box_ptr(mgic_field f, int local_index) {
  double *p = nullptr;
  mg(mgic_field_device_ptr(f, local_index, &p, nullptr));
  return p;
}

hipStream_t stream_of(mgic_comm c) {
  need(c, "comm");
  void *s = nullptr;
  mg(mgic_comm_get_stream(c, &s));
  return static_cast<hipStream_t>(s);
}

struct DeviceBuffer {
  void *p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t bytes, const char *what) { hip(hipMalloc(&p, bytes), what); }
};

// the checks of the entry point (nothing is launched before they pass), then
// the box table: one Row per local box
struct Table {
  std::vector<Row> rows;
  long long nblocks = 0;
};

Table table_of(mgic_field phi, mgic_field pi, mgic_field K) {
  need(phi, "phi");
  need(K, "K");
  const Layout L = layout_of(phi, "phi");
  if (pi) same_layout(L, pi, "pi");
  same_layout(L, K, "K");
  if (K == phi || K == pi)
    throw KhybError(MGIC_EBADARG, "aliased argument: K is passed as phi or pi");
  Table T;
  for (const LocalBox &b : L.local) {
    if (b.nx <= 0 || b.ny <= 0 || b.nz <= 0) continue;
    Row r{};
    r.nx = b.nx, r.ny = b.ny, r.nz = b.nz;
    r.sy = b.sy, r.sz = b.sz;
    r.first = T.nblocks;
    T.nblocks += mgic::khyb::blocks_of(r);
    r.phi = box_ptr(phi, b.index);
    r.pi = pi ? box_ptr(pi, b.index) : nullptr;
    r.K = box_ptr(K, b.index);
    T.rows.push_back(r);
  }
  return T;
}

}  // namespace

extern "C" {

MGIC_KHYB_API const char *mgic_khyb_last_error(void) { return g_err.c_str(); }

MGIC_KHYB_API int mgic_khyb_K(mgic_comm c, mgic_field phi, mgic_field pi, const double *pot,
                              double G, mgic_field K, long long *bad_cells) {
  return guard([&] {
    need(c, "comm");
    need(pot, "pot");
    need(bad_cells, "bad_cells");
    const Table T = table_of(phi, pi, K);
    const hipStream_t st = stream_of(c);
    int bad = 0;
    if (!T.rows.empty()) {
      // the table on the device, the launch, and its completion (the host
      // table and the device buffer outlive the launch)
      const size_t bytes = T.rows.size() * sizeof(Row);
      DeviceBuffer buf;
      buf.alloc(bytes + sizeof(int), "hipMalloc(box table)");
      int *d_bad = reinterpret_cast<int *>(static_cast<char *>(buf.p) + bytes);
      hip(hipMemcpyAsync(buf.p, T.rows.data(), bytes, hipMemcpyHostToDevice, st),
          "hipMemcpyAsync(box table)");
      hip(hipMemsetAsync(d_bad, 0, sizeof(int), st), "hipMemsetAsync(counter)");
      mgic::khyb::set_K(static_cast<const Row *>(buf.p), (int)T.rows.size(), T.nblocks,
                        mgic::khyb::Params{pot[0], pot[1], pot[2], G}, d_bad, st);
      hip(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st),
          "hipMemcpyAsync(counter)");
      hip(hipStreamSynchronize(st), "hipStreamSynchronize");
    }
    *bad_cells = bad;
  });
}

MGIC_KHYB_API int mgic_khyb_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw KhybError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_KHYB_API int mgic_khyb_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
