// ctt_capi.cpp -- the C ABI of libmgic_ctt.so (include/mgic_ctt.h) over the
// launchers of ctt.hip.  Fields are reached through libmgic's C ABI alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_ctt.h"
#include "ctt.hpp"
#include "launch_ledger.hpp"

namespace {

using mgic::ctt::BoxGeom;

thread_local std::string g_err;

struct CttError : std::runtime_error {
  int code;
  CttError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const CttError &e) {
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
  if (!p) throw CttError(MGIC_EBADARG, std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw CttError(st, m ? m : "libmgic error");
  }
}

// the local boxes of one field: geometry, and whether each face is a domain
// face that is not periodic
struct LocalBox {
  int index;  // local box index (mgic_field_device_ptr)
  int lohi[6];
  BoxGeom g;
  bool domain_face[6];
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
    LocalBox b;
    b.index = li;
    std::copy(lohi, lohi + 6, b.lohi);
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    b.g = BoxGeom{lohi[3] - lohi[0] + 1, lohi[4] - lohi[1] + 1, lohi[5] - lohi[2] + 1, st[1], st[2]};
    for (int d = 0; d < 3; ++d) {
      b.domain_face[2 * d] = !L.periodic[d] && lohi[d] == L.domain[d];
      b.domain_face[2 * d + 1] = !L.periodic[d] && lohi[3 + d] == L.domain[3 + d];
    }
    L.local.push_back(b);
  }
  return L;
}

void same_layout(const Layout &a, mgic_field f, const char *name) {
  const Layout b = layout_of(f, name);
  bool ok = a.nbox == b.nbox && a.dx == b.dx && a.boxes == b.boxes &&
            std::equal(a.domain, a.domain + 6, b.domain) &&
            std::equal(a.periodic, a.periodic + 3, b.periodic);
  if (!ok) throw CttError(MGIC_EBADARG, std::string("layout mismatch: ") + name);
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

// every field of `f` distinct (an output that is also an operand would be
// read by a neighbouring thread after it was written)
void distinct(const std::vector<mgic_field> &f) {
  for (size_t a = 0; a < f.size(); ++a)
    for (size_t b = 0; b < a; ++b)
      if (f[a] == f[b]) throw CttError(MGIC_EBADARG, "aliased argument: a field is passed twice");
}

}  // namespace

extern "C" {

MGIC_CTT_API const char *mgic_ctt_last_error(void) { return g_err.c_str(); }

MGIC_CTT_API int mgic_ctt_div_rhs(mgic_comm c, const mgic_field v[3], mgic_field out) {
  return guard([&] {
    need(v, "v");
    const Layout L = layout_of(out, "out");
    for (int d = 0; d < 3; ++d) same_layout(L, v[d], "v[d]");
    distinct({v[0], v[1], v[2], out});
    const hipStream_t st = stream_of(c);
    for (const LocalBox &b : L.local) {
      const double *vp[3] = {box_ptr(v[0], b.index), box_ptr(v[1], b.index), box_ptr(v[2], b.index)};
      mgic::ctt::div_rhs(box_ptr(out, b.index), vp, b.g, L.dx, st);
    }
  });
}

MGIC_CTT_API int mgic_ctt_w(mgic_comm c, const mgic_field v[3], mgic_field u,
                            const mgic_field w[3]) {
  return guard([&] {
    need(v, "v");
    need(w, "w");
    const Layout L = layout_of(u, "u");
    for (int d = 0; d < 3; ++d) {
      same_layout(L, v[d], "v[d]");
      same_layout(L, w[d], "w[d]");
    }
    distinct({v[0], v[1], v[2], u, w[0], w[1], w[2]});
    const hipStream_t st = stream_of(c);
    for (const LocalBox &b : L.local) {
      const double *vp[3] = {box_ptr(v[0], b.index), box_ptr(v[1], b.index), box_ptr(v[2], b.index)};
      double *wp[3] = {box_ptr(w[0], b.index), box_ptr(w[1], b.index), box_ptr(w[2], b.index)};
      mgic::ctt::w(wp, vp, box_ptr(u, b.index), b.g, L.dx, st);
    }
  });
}

MGIC_CTT_API int mgic_ctt_lw(mgic_comm c, const mgic_field w[3], const mgic_field lw[6]) {
  return guard([&] {
    need(w, "w");
    need(lw, "lw");
    const Layout L = layout_of(w[0], "w[0]");
    for (int d = 1; d < 3; ++d) same_layout(L, w[d], "w[d]");
    for (int q = 0; q < 6; ++q) same_layout(L, lw[q], "lw[c]");
    distinct({w[0], w[1], w[2], lw[0], lw[1], lw[2], lw[3], lw[4], lw[5]});
    const hipStream_t st = stream_of(c);
    for (const LocalBox &b : L.local) {
      const double *wp[3] = {box_ptr(w[0], b.index), box_ptr(w[1], b.index), box_ptr(w[2], b.index)};
      double *op[6];
      for (int q = 0; q < 6; ++q) op[q] = box_ptr(lw[q], b.index);
      mgic::ctt::lw(op, wp, b.g, L.dx, st);
    }
  });
}

MGIC_CTT_API int mgic_ctt_extrap(mgic_comm c, mgic_field f) {
  return guard([&] {
    const Layout L = layout_of(f, "f");
    const hipStream_t st = stream_of(c);
    for (const LocalBox &b : L.local)  // checked for every box before the first launch
      for (int face = 0; face < 6; ++face)
        if (b.domain_face[face] && b.lohi[3 + face / 2] - b.lohi[face / 2] < 1)
          throw CttError(MGIC_EBADARG, "a box with a domain face has one cell along its normal");
    for (const LocalBox &b : L.local)
      for (int face = 0; face < 6; ++face)
        if (b.domain_face[face]) mgic::ctt::extrap(box_ptr(f, b.index), b.g, face, st);
  });
}

MGIC_CTT_API int mgic_ctt_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw CttError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_CTT_API int mgic_ctt_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
