// horizon_capi.cpp -- the C ABI of libmgic_horizon.so (include/mgic_horizon.h)
// over the launcher of horizon.hip.  Fields are reached through libmgic's C ABI
// alone.  Everything is checked on the host before the launch; the host only
// uploads the points, the normals and the box table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_horizon.h"
#include "horizon.hpp"
#include "launch_ledger.hpp"

namespace {

using namespace mgic::horizon;

static_assert(kMaxLevels == MGIC_HORIZON_MAX_LEVELS && kMaxPoints == MGIC_HORIZON_MAX_POINTS &&
                  kTerms == MGIC_HORIZON_TERMS,
              "mgic_horizon.h");
static_assert(kMaxPunctures == MGIC_MAX_PUNCTURES, "mgic.h");

thread_local std::string g_err;

struct HorizonError : std::runtime_error {
  int code;
  HorizonError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const HorizonError &e) {
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

[[noreturn]] void bad(const std::string &m) { throw HorizonError(MGIC_EBADARG, m); }

void need(const void *p, const char *name) {
  if (!p) bad(std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw HorizonError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw HorizonError(MGIC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
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

// the table as the *_punct entry points take and complete it
void set_punctures(PunctureTable &t, int n, const double *values) {
  if (n < 1 || n > kMaxPunctures)
    bad("puncture count " + std::to_string(n) + " outside 1.." + std::to_string(kMaxPunctures));
  need(values, "punctures");
  for (int i = 0; i < n * kPunctureDoubles; ++i)
    if (!std::isfinite(values[i]))
      bad("puncture " + std::to_string(i / kPunctureDoubles + 1) + ": entry " +
          std::to_string(i % kPunctureDoubles) + " is not finite");
  t.n = n;
  for (int q = 0; q < kMaxPunctures; ++q)
    for (int c = 0; c < kPunctureDoubles; ++c)
      t.v[q][c] = q < n ? values[q * kPunctureDoubles + c] : 0.0;
  if (n % 2)  // the odd count's partner: nothing at the last puncture's position
    for (int c = 1; c <= 3; ++c) t.v[n][c] = t.v[n - 1][c];
}

// what of a field's layout the box table rests on
struct Layout {
  int domain[6], periodic[3], nbox = 0;
  double dx = 0.0;
  std::vector<int> boxes;    // 8 ints per box: lohi, owner, local index
  std::vector<long> strides; // 2 per local box: sy, sz
  std::vector<double *> ptr; // valid-lo pointer per box
};

Layout layout_of(mgic_field f, const std::string &name) {
  need(f, name.c_str());
  Layout L;
  int rank = 0, size = 1;
  mg(mgic_field_layout(f, L.domain, L.periodic, &L.dx, &L.nbox, &rank, &size));
  for (int i = 0; i < L.nbox; ++i) {
    int lohi[6], owner = 0, li = -1;
    mg(mgic_field_box(f, i, lohi, &owner, &li));
    if (li < 0) bad("every box of " + name + " must be local (one rank)");
    L.boxes.insert(L.boxes.end(), lohi, lohi + 6);
    L.boxes.push_back(owner);
    L.boxes.push_back(li);
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    L.strides.push_back(st[1]);
    L.strides.push_back(st[2]);
    L.ptr.push_back(p);
  }
  return L;
}

bool same_layout(const Layout &a, const Layout &b) {
  return a.nbox == b.nbox && a.dx == b.dx && a.boxes == b.boxes && a.strides == b.strides &&
         std::equal(a.domain, a.domain + 6, b.domain) &&
         std::equal(a.periodic, a.periodic + 3, b.periodic);
}

void run(mgic_comm c, int nlev, const mgic_field *psi, const mgic_field *lw, int npunct,
         const double *table, int npts, const double *xyz, const double *normal,
         const double *divn, double *out, int *level_used, int *order_used) {
  need(psi, "psi");
  need(xyz, "xyz");
  need(normal, "normal");
  need(divn, "divn");
  need(out, "out");
  need(level_used, "level_used");
  need(order_used, "order_used");
  if (nlev < 1 || nlev > kMaxLevels)
    bad("level count " + std::to_string(nlev) + " outside 1.." + std::to_string(kMaxLevels));
  if (npts < 1 || npts > kMaxPoints)
    bad("point count " + std::to_string(npts) + " outside 1.." + std::to_string(kMaxPoints));
  PunctureTable t;
  set_punctures(t, npunct, table);
  if (lw)
    for (int i = 0; i < 6 * nlev; ++i)
      need(lw[i], ("lw[" + std::to_string(i / 6) + "][" + std::to_string(i % 6) + "]").c_str());
  const hipStream_t st = stream_of(c);

  Args a{};
  a.nlev = nlev;
  a.npts = npts;
  std::vector<Box> boxes;
  int prev[6] = {0, 0, 0, 0, 0, 0};
  for (int l = 0; l < nlev; ++l) {
    const std::string name = "psi[" + std::to_string(l) + "]";
    a.box0[l] = (int)boxes.size();
    const Layout L = layout_of(psi[l], name);
    const int *dom = L.domain;
    for (int d = 0; d < 3; ++d)
      if (L.periodic[d]) bad("the expansion is not defined on a periodic domain");
    if (l == 0) {
      for (int d = 0; d < 3; ++d) {
        if (dom[d] != 0) bad("the level-0 domain's low corner must be 0");
        if (dom[3 + d] < 0 || dom[3 + d] >= (1 << 20)) bad("the level-0 domain is empty or too large");
        a.n0[d] = dom[3 + d] + 1;
        a.len[d] = (double)a.n0[d] * L.dx;
        a.half[d] = (double)a.n0[d] * L.dx / 2.0;
      }
    } else {
      for (int d = 0; d < 3; ++d)
        if (dom[d] != 2 * prev[d] || dom[3 + d] != 2 * prev[3 + d] + 1)
          bad("the domain of level " + std::to_string(l) + " is not level " +
              std::to_string(l - 1) + "'s refined by 2");
    }
    if (!(L.dx > 0.0)) bad("the spacing of level " + std::to_string(l) + " is not positive");
    a.dx[l] = L.dx;
    std::vector<Layout> W;
    if (lw)
      for (int k = 0; k < 6; ++k) {
        W.push_back(layout_of(lw[6 * l + k], "lw[" + std::to_string(l) + "][" + std::to_string(k) + "]"));
        if (!same_layout(L, W.back()))
          bad("layout mismatch: lw[" + std::to_string(l) + "][" + std::to_string(k) + "] is not on " + name + "'s layout");
      }
    for (int i = 0; i < L.nbox; ++i) {
      Box b;
      for (int d = 0; d < 3; ++d) {
        b.lo[d] = L.boxes[8 * i + d];
        b.hi[d] = L.boxes[8 * i + 3 + d];
      }
      b.sy = L.strides[2 * i];
      b.sz = L.strides[2 * i + 1];
      b.psi = L.ptr[i];
      for (int k = 0; k < 6; ++k) b.lw[k] = lw ? W[k].ptr[i] : nullptr;
      boxes.push_back(b);
    }
    std::copy(dom, dom + 6, prev);
  }
  for (int l = nlev; l <= kMaxLevels; ++l) a.box0[l] = (int)boxes.size();
  if (boxes.empty()) bad("the fields have no boxes");

  // one device allocation: points, normals, divn, the results (doubles), the box
  // table (8-byte aligned members), then the two int arrays
  const size_t n = (size_t)npts;
  const size_t o_xyz = 0, o_normal = o_xyz + n * 3 * sizeof(double);
  const size_t o_divn = o_normal + n * 3 * sizeof(double);
  const size_t o_out = o_divn + n * sizeof(double);
  const size_t o_boxes = o_out + n * kTerms * sizeof(double);
  const size_t o_level = o_boxes + boxes.size() * sizeof(Box);
  const size_t o_order = o_level + n * sizeof(int);
  DeviceBuffer buf;
  buf.alloc(o_order + n * sizeof(int), "hipMalloc(points, box table, results)");
  char *d = static_cast<char *>(buf.p);
  a.xyz = reinterpret_cast<const double *>(d + o_xyz);
  a.normal = reinterpret_cast<const double *>(d + o_normal);
  a.divn = reinterpret_cast<const double *>(d + o_divn);
  a.out = reinterpret_cast<double *>(d + o_out);
  a.boxes = reinterpret_cast<const Box *>(d + o_boxes);
  a.level = reinterpret_cast<int *>(d + o_level);
  a.order = reinterpret_cast<int *>(d + o_order);
  hip(hipMemcpyAsync(d + o_boxes, boxes.data(), boxes.size() * sizeof(Box), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(box table)");
  hip(hipMemcpyAsync(d + o_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(points)");
  hip(hipMemcpyAsync(d + o_normal, normal, n * 3 * sizeof(double), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(normals)");
  hip(hipMemcpyAsync(d + o_divn, divn, n * sizeof(double), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(divn)");
  expansion(a, t, lw != nullptr, st);
  hip(hipMemcpyAsync(out, d + o_out, n * kTerms * sizeof(double), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(out)");
  hip(hipMemcpyAsync(level_used, d + o_level, n * sizeof(int), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(level)");
  hip(hipMemcpyAsync(order_used, d + o_order, n * sizeof(int), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(order)");
  hip(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace

extern "C" {

MGIC_HORIZON_API const char *mgic_horizon_last_error(void) { return g_err.c_str(); }

MGIC_HORIZON_API int mgic_horizon_expansion(mgic_comm c, int nlev, const mgic_field *psi,
                                            const mgic_field *lw, int npunct, const double *table,
                                            int npts, const double *xyz, const double *normal,
                                            const double *divn, double *out, int *level_used,
                                            int *order_used) {
  return guard([&] {
    run(c, nlev, psi, lw, npunct, table, npts, xyz, normal, divn, out, level_used, order_used);
  });
}

MGIC_HORIZON_API int mgic_horizon_launch_ledger_dump(const char *path) {
  return guard([&] {
    need(path, "path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) bad(std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_HORIZON_API int mgic_horizon_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
