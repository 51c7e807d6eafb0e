// sample_capi.cpp -- the C ABI of libmgic_sample.so (include/mgic_sample.h)
// over the launcher of sample.hip.  Fields are reached through libmgic's C ABI
// alone.  Everything is checked on the host before the launch; the host only
// uploads the points and the box table.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mgic_sample.h"
#include "launch_ledger.hpp"
#include "sample.hpp"

namespace {

using namespace mgic::sample;

static_assert(kMaxLevels == MGIC_SAMPLE_MAX_LEVELS && kMaxPoints == MGIC_SAMPLE_MAX_POINTS,
              "mgic_sample.h");

thread_local std::string g_err;

struct SampleError : std::runtime_error {
  int code;
  SampleError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const SampleError &e) {
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

[[noreturn]] void bad(const std::string &m) { throw SampleError(MGIC_EBADARG, m); }

void need(const void *p, const char *name) {
  if (!p) bad(std::string("null argument: ") + name);
}

// a libmgic call: its status and message become this library's
void mg(int st) {
  if (st < 0) {
    const char *m = mgic_last_error();
    throw SampleError(st, m ? m : "libmgic error");
  }
}

void hip(hipError_t e, const char *what) {
  if (e != hipSuccess)
    throw SampleError(MGIC_EHIP, std::string(what) + ": " + hipGetErrorString(e));
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

// level l's boxes appended to the table; its domain, periodicity and spacing
void add_level(mgic_field f, int l, std::vector<Box> &boxes, int domain[6], int periodic[3],
               double &dx) {
  const std::string name = "fields[" + std::to_string(l) + "]";
  need(f, name.c_str());
  int nbox = 0, rank = 0, size = 1;
  mg(mgic_field_layout(f, domain, periodic, &dx, &nbox, &rank, &size));
  for (int i = 0; i < nbox; ++i) {
    int lohi[6], owner = 0, li = -1;
    mg(mgic_field_box(f, i, lohi, &owner, &li));
    if (li < 0) bad("every box of " + name + " must be local (one rank)");
    long st[3];
    double *p = nullptr;
    mg(mgic_field_device_ptr(f, li, &p, st));
    Box b;
    for (int d = 0; d < 3; ++d) {
      b.lo[d] = lohi[d];
      b.hi[d] = lohi[3 + d];
    }
    b.sy = st[1];
    b.sz = st[2];
    b.u = p;
    boxes.push_back(b);
  }
}

void run(mgic_comm c, int nlev, const mgic_field *fields, int npts, const double *xyz, int order,
         double *values, int *level_used, int *order_used) {
  need(fields, "fields");
  need(xyz, "xyz");
  need(values, "values");
  need(level_used, "level_used");
  need(order_used, "order_used");
  if (nlev < 1 || nlev > kMaxLevels)
    bad("level count " + std::to_string(nlev) + " outside 1.." + std::to_string(kMaxLevels));
  if (npts < 1 || npts > kMaxPoints)
    bad("point count " + std::to_string(npts) + " outside 1.." + std::to_string(kMaxPoints));
  if (order != 1 && order != 2 && order != 4)
    bad("order " + std::to_string(order) + " is not 1, 2 or 4");
  const hipStream_t st = stream_of(c);

  Args a{};
  a.nlev = nlev;
  a.npts = npts;
  std::vector<Box> boxes;
  int prev[6] = {0, 0, 0, 0, 0, 0};
  for (int l = 0; l < nlev; ++l) {
    int dom[6], per[3];
    a.box0[l] = (int)boxes.size();
    add_level(fields[l], l, boxes, dom, per, a.dx[l]);
    if (l == 0) {
      for (int d = 0; d < 3; ++d) {
        if (dom[d] != 0) bad("the level-0 domain's low corner must be 0");
        if (dom[3 + d] < 0 || dom[3 + d] >= (1 << 20)) bad("the level-0 domain is empty or too large");
        a.n0[d] = dom[3 + d] + 1;
        a.periodic[d] = per[d] ? 1 : 0;
        a.len[d] = (double)a.n0[d] * a.dx[0];
        a.half[d] = (double)a.n0[d] * a.dx[0] / 2.0;
      }
    } else {
      for (int d = 0; d < 3; ++d) {
        if (dom[d] != 2 * prev[d] || dom[3 + d] != 2 * prev[3 + d] + 1)
          bad("the domain of level " + std::to_string(l) + " is not level " +
              std::to_string(l - 1) + "'s refined by 2");
        if ((per[d] ? 1 : 0) != a.periodic[d])
          bad("the periodicity of level " + std::to_string(l) + " differs from level 0's");
      }
    }
    if (!(a.dx[l] > 0.0)) bad("the spacing of level " + std::to_string(l) + " is not positive");
    std::copy(dom, dom + 6, prev);
  }
  for (int l = nlev; l <= kMaxLevels; ++l) a.box0[l] = (int)boxes.size();
  if (boxes.empty()) bad("the fields have no boxes");

  // one device allocation: points, values (doubles), the box table (8-byte
  // aligned members), then the two int arrays
  const size_t n = (size_t)npts;
  const size_t o_xyz = 0, o_values = o_xyz + n * 3 * sizeof(double);
  const size_t o_boxes = o_values + n * sizeof(double);
  const size_t o_level = o_boxes + boxes.size() * sizeof(Box);
  const size_t o_order = o_level + n * sizeof(int);
  DeviceBuffer buf;
  buf.alloc(o_order + n * sizeof(int), "hipMalloc(points, box table, results)");
  char *d = static_cast<char *>(buf.p);
  a.xyz = reinterpret_cast<const double *>(d + o_xyz);
  a.values = reinterpret_cast<double *>(d + o_values);
  a.boxes = reinterpret_cast<const Box *>(d + o_boxes);
  a.level = reinterpret_cast<int *>(d + o_level);
  a.order = reinterpret_cast<int *>(d + o_order);
  hip(hipMemcpyAsync(d + o_boxes, boxes.data(), boxes.size() * sizeof(Box), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(box table)");
  hip(hipMemcpyAsync(d + o_xyz, xyz, n * 3 * sizeof(double), hipMemcpyHostToDevice, st),
      "hipMemcpyAsync(points)");
  points(a, order, st);
  hip(hipMemcpyAsync(values, d + o_values, n * sizeof(double), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(values)");
  hip(hipMemcpyAsync(level_used, d + o_level, n * sizeof(int), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(level)");
  hip(hipMemcpyAsync(order_used, d + o_order, n * sizeof(int), hipMemcpyDeviceToHost, st),
      "hipMemcpyAsync(order)");
  hip(hipStreamSynchronize(st), "hipStreamSynchronize");
}

}  // namespace

extern "C" {

MGIC_SAMPLE_API const char *mgic_sample_last_error(void) { return g_err.c_str(); }

MGIC_SAMPLE_API int mgic_sample_points(mgic_comm c, int nlev, const mgic_field *fields, int npts,
                                       const double *xyz, int order, double *values,
                                       int *level_used, int *order_used) {
  return guard([&] { run(c, nlev, fields, npts, xyz, order, values, level_used, order_used); });
}

MGIC_SAMPLE_API int mgic_sample_launch_ledger_dump(const char *path) {
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

MGIC_SAMPLE_API int mgic_sample_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
