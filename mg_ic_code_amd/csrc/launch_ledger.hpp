// launch_ledger.hpp -- every kernel launch of the library goes through
// ledger::launch, which counts launches per kernel instantiation on the host
// (one relaxed atomic increment; nothing changes on the device).
//
// The set of entries comes from the build: Site<K> is a class template keyed
// on the kernel's address whose static Entry links itself into the registry
// when the library loads, so every instantiation the host code CAN launch is
// listed with a count of zero before anything runs.  Its name is the
// compiler's spelling of K (demangled from Tag<K>'s type name): nobody types
// "k_gsrb_tb2<float, 64, 22, 1024, false, true, false, true, false>".
//
// A two-sweep (k_gsrb_tb2) launch also records which tile classes (EM of
// tb2_tile: 0, 3, 12, 15) its grid contains; each class is an entry of its
// own, "<name>#em<EM>".
//
// Read through mgic_launch_ledger_dump / _reset (include/mgic.h) and
// MGIC_LAUNCH_LEDGER (capi.cpp).  This is the one file with a triple-chevron
// launch (tests/test_launch_coverage.py holds the others to that).
#pragma once

#include <cxxabi.h>

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <string>
#include <typeinfo>
#include <utility>
#include <vector>

namespace mgic {
namespace ledger {

constexpr int kTileClasses = 4;
constexpr int kTileClassEM[kTileClasses] = {0, 3, 12, 15};
// bit of a tile class in Entry::classes / launch_tiles' `present`
constexpr unsigned class_bit(int em) { return em == 0 ? 1u : em == 3 ? 2u : em == 12 ? 4u : 8u; }

struct Entry {
  const char *pretty;  // typeid(Tag<K>).name(): mangled, spelled out by entry_name
  unsigned classes;    // tile classes this instantiation compiles (0: not tiled)
  std::atomic<unsigned long long> count{0};
  std::atomic<unsigned long long> tiles[kTileClasses]{};
  Entry *next = nullptr;
  Entry(const char *p, unsigned c);
};

// (constant-initialised: valid before any Entry's constructor runs)
inline std::atomic<Entry *> g_head{nullptr};

inline Entry::Entry(const char *p, unsigned c) : pretty(p), classes(c) {
  next = g_head.load(std::memory_order_relaxed);
  while (!g_head.compare_exchange_weak(next, this, std::memory_order_release,
                                       std::memory_order_relaxed)) {
  }
}

// The name is the mangled name of Tag<K>, which spells the kernel
// specialisation out in full (__PRETTY_FUNCTION__ prints a function-pointer
// template argument without its template arguments).
template <auto K>
struct Tag {};

template <auto K, unsigned CLASSES = 0>
struct Site {
  static inline Entry e{typeid(Tag<K>).name(), CLASSES};
};

// "mgic::ledger::Tag<&(void mgic::kern::(anonymous namespace)::k_blas<3>(double*, ...))>"
// or "mgic::ledger::Tag<&mgic::kern::(anonymous namespace)::k_lambda>" -> "k_blas<3>", "k_lambda"
inline std::string entry_name(const char *mangled) {
  int status = 0;
  char *d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string s(status == 0 && d ? d : mangled);
  std::free(d);
  const size_t t = s.find("Tag<");
  if (t != std::string::npos) s = s.substr(t + 4);
  if (!s.empty() && s.back() == '>') s.pop_back();
  for (const char *p : {"&", "(", "void "})
    if (s.compare(0, std::strlen(p), p) == 0) s.erase(0, std::strlen(p));
  // (no static objects here: this also runs while the library unloads)
  const char *const anon = "(anonymous namespace)";
  for (size_t at; (at = s.find(anon)) != std::string::npos;) s.replace(at, std::strlen(anon), "{anon}");
  // the parameter list: from the first '(' outside the template argument list
  int depth = 0;
  for (size_t i = 0; i < s.size(); ++i) {
    if (s[i] == '<') ++depth;
    else if (s[i] == '>') --depth;
    else if (s[i] == '(' && depth == 0) {
      s.erase(i);
      break;
    }
  }
  // the scope in front of the kernel's own name
  const size_t lt = s.find('<');
  const size_t sc = s.rfind("::", lt == std::string::npos ? s.size() : lt);
  if (sc != std::string::npos) s.erase(0, sc + 2);
  return s;
}

// (name, count) of every entry, tile classes as entries of their own
inline std::vector<std::pair<std::string, unsigned long long>> snapshot() {
  std::vector<std::pair<std::string, unsigned long long>> out;
  for (Entry *e = g_head.load(std::memory_order_acquire); e; e = e->next) {
    const std::string n = entry_name(e->pretty);
    out.emplace_back(n, e->count.load(std::memory_order_relaxed));
    for (int c = 0; c < kTileClasses; ++c)
      if (e->classes & (1u << c))
        out.emplace_back(n + "#em" + std::to_string(kTileClassEM[c]),
                         e->tiles[c].load(std::memory_order_relaxed));
  }
  return out;
}

inline void reset() {
  for (Entry *e = g_head.load(std::memory_order_acquire); e; e = e->next) {
    e->count.store(0, std::memory_order_relaxed);
    for (int c = 0; c < kTileClasses; ++c) e->tiles[c].store(0, std::memory_order_relaxed);
  }
}

#if defined(__HIP__)
template <auto K, class... A>
inline void launch(dim3 grid, dim3 block, size_t shmem, hipStream_t st, A &&...a) {
  Site<K>::e.count.fetch_add(1, std::memory_order_relaxed);
  K<<<grid, block, shmem, st>>>(std::forward<A>(a)...);
}

// a tiled launch: CLASSES the tile classes the instantiation compiles,
// `present` the ones this grid contains (bits of class_bit)
template <auto K, unsigned CLASSES, class... A>
inline void launch_tiles(unsigned present, dim3 grid, dim3 block, size_t shmem, hipStream_t st,
                         A &&...a) {
  Entry &e = Site<K, CLASSES>::e;
  e.count.fetch_add(1, std::memory_order_relaxed);
  for (int c = 0; c < kTileClasses; ++c)
    if (present & CLASSES & (1u << c)) e.tiles[c].fetch_add(1, std::memory_order_relaxed);
  K<<<grid, block, shmem, st>>>(std::forward<A>(a)...);
}
#endif

}  // namespace ledger
}  // namespace mgic
