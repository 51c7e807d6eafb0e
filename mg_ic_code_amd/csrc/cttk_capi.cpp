// cttk_capi.cpp -- the C ABI of libmgic_cttk.so (include/mgic_cttk.h) over the
// launchers of cttk.hip.  Fields are reached through libmgic's C ABI alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_cttk.h"
#include "cttk.hpp"
#include "launch_ledger.hpp"

namespace {

using mgic::cttk::Row;

thread_local std::string g_err;

struct CttkError : std::runtime_error {
  int code;
  CttkError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const CttkError &e) {
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
  if (!p) throw CttkError(MGIC_EBADARG, std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw CttkError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw CttkError(MGIC_EUNKNOWN, std::string(what) + ": " + hipGetErrorString(e));
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
      throw CttkError(MGIC_EBADARG, std::string("box ") + std::to_string(i) + " of " + name +
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
  if (!ok) throw CttkError(MGIC_EBADARG, std::string("layout mismatch: ") + name);
}

// fields[first..n) are written: each differs from every other field of the call
void distinct(const mgic_field *fields, int n, int first) {
  for (int a = first; a < n; ++a)
    for (int b = 0; b < a; ++b)
      if (fields[a] == fields[b])
        throw CttkError(MGIC_EBADARG, "aliased argument: a field that is written is passed twice");
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

// the checks of every entry point (nothing is launched before they pass),
// then the box table of the n fields: one Row per local box
struct Table {
  std::vector<Row> rows;
  long long nblocks = 0;
  double h = 0.0;  // 0.5 / dx
};

Table table_of(const mgic_field *fields, const char *const *names, int n, int first_written) {
  for (int i = 0; i < n; ++i) need(fields[i], names[i]);
  const Layout L = layout_of(fields[0], names[0]);
  for (int i = 1; i < n; ++i) same_layout(L, fields[i], names[i]);
  distinct(fields, n, first_written);
  Table T;
  T.h = 0.5 / L.dx;
  for (const LocalBox &b : L.local) {
    if (b.nx <= 0 || b.ny <= 0 || b.nz <= 0) continue;
    Row r{};
    r.nx = b.nx, r.ny = b.ny, r.nz = b.nz;
    r.sy = b.sy, r.sz = b.sz;
    r.first = T.nblocks;
    T.nblocks += mgic::cttk::blocks_of(r);
    for (int i = 0; i < n; ++i) r.p[i] = box_ptr(fields[i], b.index);
    T.rows.push_back(r);
  }
  return T;
}

// the table on the device, the launch, and its completion (the host table
// and the device buffer outlive the launch)
template <class F>
void run(mgic_comm c, const Table &T, size_t extra_bytes, F &&launch) {
  const hipStream_t st = stream_of(c);
  if (T.rows.empty()) return;
  const size_t bytes = T.rows.size() * sizeof(Row);
  DeviceBuffer buf;
  buf.alloc(bytes + extra_bytes, "hipMalloc(box table)");
  hip(hipMemcpyAsync(buf.p, T.rows.data(), bytes, hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(box table)");
  launch(static_cast<const Row *>(buf.p), static_cast<char *>(buf.p) + bytes, st);
  hip(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace

extern "C" {

MGIC_CTTK_API const char *mgic_cttk_last_error(void) { return g_err.c_str(); }

MGIC_CTTK_API int mgic_cttk_K(mgic_comm c, mgic_field integrand, mgic_field K,
                              long long *bad_cells) {
  return guard([&] {
    need(c, "comm");
    need(bad_cells, "bad_cells");
    const mgic_field f[2] = {integrand, K};
    const char *const names[2] = {"integrand", "K"};
    const Table T = table_of(f, names, 2, 1);
    int bad = 0;
    run(c, T, sizeof(int), [&](const Row *rows, char *extra, hipStream_t st) {
      int *d_bad = reinterpret_cast<int *>(extra);
      hip(hipMemsetAsync(d_bad, 0, sizeof(int), st), "hipMemsetAsync(counter)");
      mgic::cttk::set_K(rows, (int)T.rows.size(), T.nblocks, d_bad, st);
      hip(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, st),
          "hipMemcpyAsync(counter)");
    });
    *bad_cells = bad;
  });
}

MGIC_CTTK_API int mgic_cttk_source(mgic_comm c, mgic_field psi, mgic_field K,
                                   const mgic_field *S) {
  return guard([&] {
    need(c, "comm");
    need(S, "S");
    const mgic_field f[5] = {psi, K, S[0], S[1], S[2]};
    const char *const names[5] = {"psi", "K", "S[0]", "S[1]", "S[2]"};
    const Table T = table_of(f, names, 5, 2);
    run(c, T, 0, [&](const Row *rows, char *, hipStream_t st) {
      mgic::cttk::add_source(rows, (int)T.rows.size(), T.nblocks, T.h, st);
    });
  });
}

MGIC_CTTK_API int mgic_cttk_constraints(mgic_comm c, mgic_field K, mgic_field ham,
                                        const mgic_field *mom, mgic_field ham_abs) {
  return guard([&] {
    need(c, "comm");
    need(mom, "mom");
    const mgic_field f[6] = {K, ham, mom[0], mom[1], mom[2], ham_abs};
    const char *const names[6] = {"K", "ham", "mom[0]", "mom[1]", "mom[2]", "ham_abs"};
    const Table T = table_of(f, names, 6, 1);
    run(c, T, 0, [&](const Row *rows, char *, hipStream_t st) {
      mgic::cttk::correct_constraints(rows, (int)T.rows.size(), T.nblocks, T.h, st);
    });
  });
}

MGIC_CTTK_API int mgic_cttk_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw CttkError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_CTTK_API int mgic_cttk_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
