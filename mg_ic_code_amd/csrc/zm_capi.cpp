// zm_capi.cpp -- the C ABI of libmgic_zm.so (include/mgic_zm.h) over the
// launcher of zm.hip.  Fields are reached through libmgic's C ABI alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_zm.h"
#include "launch_ledger.hpp"
#include "zm.hpp"

namespace {

using mgic::zm::BoxGeom;

thread_local std::string g_err;

struct ZmError : std::runtime_error {
  int code;
  ZmError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const ZmError &e) {
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
  if (!p) throw ZmError(MGIC_EBADARG, std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw ZmError(st, m ? m : "libmgic error");
  }
}

struct LocalBox {
  int index;  // local box index (mgic_field_device_ptr)
  BoxGeom g;
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
    if (li < 0) continue;
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    L.local.push_back(LocalBox{
        li, BoxGeom{lohi[3] - lohi[0] + 1, lohi[4] - lohi[1] + 1, lohi[5] - lohi[2] + 1, st[1], st[2]}});
  }
  return L;
}

void same_layout(const Layout &a, mgic_field f, const char *name) {
  const Layout b = layout_of(f, name);
  bool ok = a.nbox == b.nbox && a.dx == b.dx && a.boxes == b.boxes &&
            std::equal(a.domain, a.domain + 6, b.domain) &&
            std::equal(a.periodic, a.periodic + 3, b.periodic) && a.local.size() == b.local.size();
  for (size_t i = 0; ok && i < a.local.size(); ++i)
    ok = a.local[i].index == b.local[i].index && a.local[i].g.sy == b.local[i].g.sy &&
         a.local[i].g.sz == b.local[i].g.sz;
  if (!ok) throw ZmError(MGIC_EBADARG, std::string("layout mismatch: ") + name);
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

}  // namespace

extern "C" {

MGIC_ZM_API const char *mgic_zm_last_error(void) { return g_err.c_str(); }

MGIC_ZM_API int mgic_zm_shift(mgic_comm c, int n, const mgic_field *fields, const double *consts) {
  return guard([&] {
    need(fields, "fields");
    need(consts, "consts");
    if (n != 1 && n != 3) throw ZmError(MGIC_EBADARG, "the number of fields is 1 or 3");
    const Layout L = layout_of(fields[0], "fields[0]");
    for (int i = 1; i < n; ++i) same_layout(L, fields[i], "fields[i]");
    for (int a = 0; a < n; ++a)
      for (int b = 0; b < a; ++b)
        if (fields[a] == fields[b])
          throw ZmError(MGIC_EBADARG, "aliased argument: a field is passed twice");
    const hipStream_t st = stream_of(c);
    for (const LocalBox &b : L.local) {
      double *p[3] = {nullptr, nullptr, nullptr};
      for (int i = 0; i < n; ++i) p[i] = box_ptr(fields[i], b.index);
      mgic::zm::shift(n, p, consts, b.g, st);
    }
  });
}

MGIC_ZM_API int mgic_zm_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw ZmError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_ZM_API int mgic_zm_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
