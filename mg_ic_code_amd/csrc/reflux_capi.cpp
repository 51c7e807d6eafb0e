// reflux_capi.cpp -- the C ABI of libmgic_reflux.so (include/mgic_reflux.h)
// over the launcher of reflux.hip, and the function table libmgic calls it
// through (mgic_amr_reflux_register).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <stdexcept>
#include <string>

#include "../../include/mgic_reflux.h"
#include "launch_ledger.hpp"
#include "reflux.hpp"

namespace {

thread_local std::string g_err;

struct RefluxError : std::runtime_error {
  int code;
  RefluxError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

template <class F>
int guard(F &&f) {
  try {
    f();
    return MGIC_OK;
  } catch (const RefluxError &e) {
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

const char *last_error() { return g_err.c_str(); }

int table_apply(const mgic_reflux_cell *cells, const mgic_reflux_face *faces, long long ncell,
                double *const *target, double *const *phi_c, double *const *phi_f,
                double *const *b, double coef, double dx_c, double dx_f, int sign, void *stream) {
  return guard([&] {
    const mgic::reflux::Args a{cells, faces, ncell, target, phi_c, phi_f, b, coef, dx_c, dx_f, sign};
    mgic::reflux::apply(a, static_cast<hipStream_t>(stream));
  });
}

const mgic_reflux_table g_table = {1, table_apply, last_error};

}  // namespace

extern "C" {

MGIC_REFLUX_API const char *mgic_reflux_last_error(void) { return g_err.c_str(); }

MGIC_REFLUX_API int mgic_reflux_register(void) {
  return guard([&] {
    const int st = mgic_amr_reflux_register(&g_table);
    if (st < 0) {
      const char *m = mgic_last_error();
      throw RefluxError(st, m ? m : "libmgic error");
    }
  });
}

MGIC_REFLUX_API int mgic_reflux_launch_ledger_dump(const char *path) {
  return guard([&] {
    if (!path) throw RefluxError(MGIC_EBADARG, "null argument: path");
    auto rows = mgic::ledger::snapshot();
    std::sort(rows.begin(), rows.end());
    FILE *f = std::fopen(path, "w");
    if (!f) throw RefluxError(MGIC_EBADARG, std::string("launch ledger: cannot write ") + path);
    for (const auto &r : rows) std::fprintf(f, "%s\t%llu\n", r.first.c_str(), r.second);
    std::fclose(f);
  });
}

MGIC_REFLUX_API int mgic_reflux_launch_ledger_reset(void) {
  return guard([&] { mgic::ledger::reset(); });
}

}  // extern "C"
