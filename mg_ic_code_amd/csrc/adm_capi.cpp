// adm_capi.cpp -- the C ABI of libmgic_adm.so (include/mgic_adm.h) over the
// launchers of adm.hip.  Fields are reached through libmgic's C ABI alone.
// Everything is checked on the host before the first launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_adm.h"
#include "adm.hpp"
#include "launch_ledger.hpp"

namespace {

using namespace mgic::adm;

static_assert(kMaxSurfaces == MGIC_ADM_MAX_SURFACES && kTerms == MGIC_ADM_TERMS, "mgic_adm.h");
static_assert(kMaxPunctures == MGIC_MAX_PUNCTURES, "mgic.h");

thread_local std::string g_err;

struct AdmError : std::runtime_error {
  int code;
  AdmError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const AdmError &e) {
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

[[noreturn]] void bad(const std::string &m) { throw AdmError(MGIC_EBADARG, m); }

void need(const void *p, const char *name) {
  if (!p) bad(std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw AdmError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess) throw AdmError(MGIC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
}

struct LocalBox {
  int index;  // local box index (mgic_field_device_ptr)
  int lohi[6];
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
    if (li < 0) continue;
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    LocalBox b{li, {lohi[0], lohi[1], lohi[2], lohi[3], lohi[4], lohi[5]}, st[1], st[2]};
    L.local.push_back(b);
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
  if (!ok) bad(std::string("layout mismatch: ") + name);
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

void check_surfaces(int nsurf, const int *half_widths) {
  if (nsurf < 1 || nsurf > kMaxSurfaces)
    bad("surface count " + std::to_string(nsurf) + " outside 1.." + std::to_string(kMaxSurfaces));
  need(half_widths, "half_widths");
  for (int s = 0; s < nsurf; ++s)
    if (half_widths[s] < 1)
      bad("half-width " + std::to_string(half_widths[s]) + " of surface " + std::to_string(s) +
          " is below 1");
}

long long faces_of(int n) { return 6LL * (2LL * n) * (2LL * n); }

struct DeviceBuffer {
  void *p = nullptr;
  ~DeviceBuffer() {
    if (p) (void)hipFree(p);
  }
  void alloc(size_t bytes, const char *what) { hip(hipMalloc(&p, bytes), what); }
};

// terms_out: the per-face terms (host, or device with terms_on_device) or
// nullptr; sums_out: the 7 sums per surface (host) or nullptr
void run(mgic_comm c, mgic_field psi, int nsurf, const int *half_widths, int npunct,
         const double *table, const mgic_field *lw, double *terms_out, int terms_on_device,
         double *sums_out) {
  check_surfaces(nsurf, half_widths);
  PunctureTable t;
  set_punctures(t, npunct, table);
  const Layout L = layout_of(psi, "psi");
  const hipStream_t st = stream_of(c);
  int N[3], half_max = 1 << 30;
  for (int d = 0; d < 3; ++d) {
    if (L.periodic[d]) bad("the charges are not defined on a periodic domain");
    if (L.domain[d] != 0) bad("the domain's low corner must be 0");
    N[d] = L.domain[3 + d] + 1;
    if (N[d] % 2) bad("N = " + std::to_string(N[d]) + " is odd: no cell-aligned cube about the centre");
    half_max = std::min(half_max, N[d] / 2 - 1);
  }
  for (int s = 0; s < nsurf; ++s)
    if (half_widths[s] > half_max)
      bad("half-width " + std::to_string(half_widths[s]) + " of surface " + std::to_string(s) +
          " is above " + std::to_string(half_max) + ": its outer cells would leave the domain");
  if ((int)L.local.size() != L.nbox) bad("every level-0 box must be local (one rank)");
  long long cells = 0;
  for (const LocalBox &b : L.local) {
    for (int d = 0; d < 3; ++d)
      if (b.lohi[d] < 0 || b.lohi[3 + d] > L.domain[3 + d] || b.lohi[d] > b.lohi[3 + d])
        bad("a box leaves the domain");
    cells += (long long)(b.lohi[3] - b.lohi[0] + 1) * (b.lohi[4] - b.lohi[1] + 1) *
             (b.lohi[5] - b.lohi[2] + 1);
  }
  // disjoint boxes inside the domain with its cell count: they tile it
  if (cells != (long long)N[0] * N[1] * N[2])
    bad("the boxes do not tile the domain: psi must be the level-0 field");
  if (lw)
    for (int i = 0; i < 6; ++i) same_layout(L, lw[i], "lw[i]");

  Args a{};
  a.nsurf = nsurf;
  a.nbox = L.nbox;
  a.dx = L.dx;
  for (int d = 0; d < 3; ++d) {
    a.centre[d] = N[d] / 2;
    a.domlen[d] = (double)N[d] * L.dx;
  }
  a.face0[0] = 0;
  a.block0[0] = 0;
  for (int s = 0; s < nsurf; ++s) {
    a.half[s] = half_widths[s];
    const long long f = faces_of(half_widths[s]);
    a.face0[s + 1] = a.face0[s] + (long)f;
    const long long nb = a.block0[s] + (f + kBlock - 1) / kBlock;
    if (nb > 0x7fffffffLL) bad("too many faces for one launch");
    a.block0[s + 1] = (int)nb;
  }
  std::vector<Box> boxes(L.local.size());
  for (size_t i = 0; i < boxes.size(); ++i) {
    const LocalBox &b = L.local[i];
    Box &o = boxes[i];
    for (int d = 0; d < 3; ++d) {
      o.lo[d] = b.lohi[d];
      o.hi[d] = b.lohi[3 + d];
    }
    o.sy = b.sy;
    o.sz = b.sz;
    o.psi = box_ptr(psi, b.index);
    for (int k = 0; k < 6; ++k) o.lw[k] = lw ? box_ptr(lw[k], b.index) : nullptr;
  }

  const size_t nterms = (size_t)a.face0[nsurf] * kTerms;
  DeviceBuffer d_boxes, d_part, d_sums, d_terms;
  d_boxes.alloc(boxes.size() * sizeof(Box), "hipMalloc(box table)");
  d_part.alloc((size_t)a.block0[nsurf] * kTerms * sizeof(double), "hipMalloc(partials)");
  d_sums.alloc((size_t)nsurf * kTerms * sizeof(double), "hipMalloc(sums)");
  if (terms_out && !terms_on_device) d_terms.alloc(nterms * sizeof(double), "hipMalloc(terms)");
  a.boxes = static_cast<const Box *>(d_boxes.p);
  a.partials = static_cast<double *>(d_part.p);
  a.sums = static_cast<double *>(d_sums.p);
  a.terms = !terms_out ? nullptr : terms_on_device ? terms_out : static_cast<double *>(d_terms.p);
  hip(hipMemcpyAsync(d_boxes.p, boxes.data(), boxes.size() * sizeof(Box), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(box table)");
  surface(a, t, lw != nullptr, st);
  if (sums_out) {
    finish(a, st);
    hip(hipMemcpyAsync(sums_out, d_sums.p, (size_t)nsurf * kTerms * sizeof(double),
                       hipMemcpyDeviceToHost, st),
        "hipMemcpyAsync(sums)");
  }
  if (terms_out && !terms_on_device)
    hip(hipMemcpyAsync(terms_out, d_terms.p, nterms * sizeof(double), hipMemcpyDeviceToHost, st),
        "hipMemcpyAsync(terms)");
  hip(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace

extern "C" {

MGIC_ADM_API const char *mgic_adm_last_error(void) { return g_err.c_str(); }

MGIC_ADM_API int mgic_adm_surface_count(int nsurf, const int *half_widths, long long *count) {
  return guard([&] {
    need(count, "count");
    check_surfaces(nsurf, half_widths);
    long long n = 0;
    for (int s = 0; s < nsurf; ++s) n += faces_of(half_widths[s]) * kTerms;
    *count = n;
  });
}

MGIC_ADM_API int mgic_adm_surface_terms(mgic_comm c, mgic_field psi, int nsurf,
                                        const int *half_widths, int npunct, const double *table,
                                        const mgic_field *lw, double *out, int out_on_device) {
  return guard([&] {
    need(out, "out");
    run(c, psi, nsurf, half_widths, npunct, table, lw, out, out_on_device, nullptr);
  });
}

MGIC_ADM_API int mgic_adm_charges(mgic_comm c, mgic_field psi, int nsurf, const int *half_widths,
                                  int npunct, const double *table, const mgic_field *lw,
                                  double *out) {
  return guard([&] {
    need(out, "out");
    run(c, psi, nsurf, half_widths, npunct, table, lw, nullptr, 0, out);
  });
}

MGIC_ADM_API int mgic_adm_launch_ledger_dump(const char *path) {
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

MGIC_ADM_API int mgic_adm_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
