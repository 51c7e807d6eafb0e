// regrid.cpp -- clustering, nesting and owners of set_grids (regrid.hpp).
#include "regrid.hpp"

#include <algorithm>
#include <cstdlib>

namespace mgic {
namespace regrid {

namespace {

inline int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

struct Mask {
  const unsigned char *m;
  int n[3];
  bool at(int x, int y, int z) const { return m[((long)z * n[1] + y) * n[0] + x] != 0; }
};

inline long volume(const IBox &q) {
  return (long)(q.hi[0] - q.lo[0] + 1) * (q.hi[1] - q.lo[1] + 1) * (q.hi[2] - q.lo[2] + 1);
}

// signatures of Q: set cells per plane of every direction; returns their count
long signatures(const Mask &M, const IBox &q, std::vector<long> S[3]) {
  for (int d = 0; d < 3; ++d) S[d].assign(q.hi[d] - q.lo[d] + 1, 0);
  long n = 0;
  for (int z = q.lo[2]; z <= q.hi[2]; ++z)
    for (int y = q.lo[1]; y <= q.hi[1]; ++y)
      for (int x = q.lo[0]; x <= q.hi[0]; ++x)
        if (M.at(x, y, z)) {
          ++S[0][x - q.lo[0]];
          ++S[1][y - q.lo[1]];
          ++S[2][z - q.lo[2]];
          ++n;
        }
  return n;
}

// pieces of at most maxlen a side, sizes differing by at most 1 (larger
// first), z-major
void split_max(const IBox &q, int maxlen, std::vector<IBox> *out) {
  std::vector<int> cut[3];  // piece boundaries per direction
  for (int d = 0; d < 3; ++d) {
    const int len = q.hi[d] - q.lo[d] + 1;
    const int p = (len + maxlen - 1) / maxlen, base = len / p, rem = len % p;
    int at = q.lo[d];
    for (int i = 0; i < p; ++i) {
      cut[d].push_back(at);
      at += base + (i < rem ? 1 : 0);
    }
    cut[d].push_back(at);
  }
  for (size_t k = 0; k + 1 < cut[2].size(); ++k)
    for (size_t j = 0; j + 1 < cut[1].size(); ++j)
      for (size_t i = 0; i + 1 < cut[0].size(); ++i) {
        IBox b;
        b.lo[0] = cut[0][i];
        b.hi[0] = cut[0][i + 1] - 1;
        b.lo[1] = cut[1][j];
        b.hi[1] = cut[1][j + 1] - 1;
        b.lo[2] = cut[2][k];
        b.hi[2] = cut[2][k + 1] - 1;
        out->push_back(b);
      }
}

void cluster_rec(const Mask &M, IBox q, double fill_ratio, int maxlen, std::vector<IBox> *out,
                 std::vector<IBox> *presplit) {
  std::vector<long> S[3];
  long n = signatures(M, q, S);
  if (n == 0) return;
  // 1. shrink to the bounding box of the set cells
  bool shrunk = false;
  for (int d = 0; d < 3; ++d) {
    int a = 0, b = (int)S[d].size() - 1;
    while (S[d][a] == 0) ++a;
    while (S[d][b] == 0) --b;
    if (a != 0 || b != (int)S[d].size() - 1) shrunk = true;
    const int lo = q.lo[d];
    q.lo[d] = lo + a;
    q.hi[d] = lo + b;
  }
  if (shrunk) n = signatures(M, q, S);
  // 2. full enough (or a single cell): accept
  const long vol = volume(q);
  if ((double)n >= fill_ratio * (double)vol || vol == 1) {
    if (presplit) presplit->push_back(q);
    split_max(q, maxlen, out);
    return;
  }
  int len[3];
  for (int d = 0; d < 3; ++d) len[d] = q.hi[d] - q.lo[d] + 1;
  IBox left = q, right = q;
  // 3a. a hole: the empty interior plane nearest the centre
  int hd = -1, hi_ = 0, hdist = 0;
  for (int d = 0; d < 3; ++d)
    for (int i = 1; i <= len[d] - 2; ++i) {
      if (S[d][i] != 0) continue;
      const int dist = std::abs(2 * i + 1 - len[d]);
      if (hd < 0 || dist < hdist || (dist == hdist && len[d] > len[hd])) {
        hd = d;
        hi_ = i;
        hdist = dist;
      }
    }
  if (hd >= 0) {
    left.hi[hd] = q.lo[hd] + hi_ - 1;
    right.lo[hd] = q.lo[hd] + hi_ + 1;
  } else {
    // 3b. an inflection: the strongest sign change of the signature's Laplacian
    int id = -1, ii = 0, idist = 0;
    long istr = 0;
    for (int d = 0; d < 3; ++d) {
      if (len[d] < 4) continue;
      auto lap = [&](int i) { return S[d][i - 1] - 2 * S[d][i] + S[d][i + 1]; };
      for (int i = 1; i <= len[d] - 3; ++i) {
        const long a = lap(i), b = lap(i + 1);
        if (!((a < 0 && b > 0) || (a > 0 && b < 0))) continue;
        const long str = std::labs(a - b);
        const int dist = std::abs(2 * (i + 1) - len[d]);
        if (id < 0 || str > istr || (str == istr && dist < idist)) {
          id = d;
          ii = i;
          istr = str;
          idist = dist;
        }
      }
    }
    if (id >= 0) {
      left.hi[id] = q.lo[id] + ii;
      right.lo[id] = q.lo[id] + ii + 1;
    } else {
      // 3c. bisect the longest direction
      int bd = 0;
      for (int d = 1; d < 3; ++d)
        if (len[d] > len[bd]) bd = d;
      left.hi[bd] = q.lo[bd] + len[bd] / 2 - 1;
      right.lo[bd] = q.lo[bd] + len[bd] / 2;
    }
  }
  // 4.
  cluster_rec(M, left, fill_ratio, maxlen, out, presplit);
  cluster_rec(M, right, fill_ratio, maxlen, out, presplit);
}

bool box_less(const IBox &a, const IBox &b) {
  for (int d = 2; d >= 0; --d)
    if (a.lo[d] != b.lo[d]) return a.lo[d] < b.lo[d];
  return false;
}

}  // namespace

bool lattice_params(int block_factor, int max_grid_size, int *c, int *maxlen, std::string *err) {
  if (block_factor < 1 || (block_factor & (block_factor - 1)) != 0) {
    if (err) *err = "regrid: block_factor must be a power of two";
    return false;
  }
  if (max_grid_size < 1) {
    if (err) *err = "regrid: max_grid_size must be positive";
    return false;
  }
  *c = std::max(block_factor / 2, 1);
  *maxlen = std::max(max_grid_size / block_factor, 1);
  return true;
}

std::vector<IBox> cluster(const unsigned char *mask, const int n[3], double fill_ratio, int maxlen,
                          std::vector<IBox> *presplit) {
  std::vector<IBox> out;
  if (presplit) presplit->clear();
  if (n[0] <= 0 || n[1] <= 0 || n[2] <= 0) return out;
  Mask M{mask, {n[0], n[1], n[2]}};
  IBox q;
  for (int d = 0; d < 3; ++d) {
    q.lo[d] = 0;
    q.hi[d] = n[d] - 1;
  }
  cluster_rec(M, q, fill_ratio, maxlen < 1 ? 1 : maxlen, &out, presplit);
  std::sort(out.begin(), out.end(), box_less);
  return out;
}

int regrid_levels(const std::vector<LevelTags> &tags, const IBox &domain0, int block_factor,
                  int max_grid_size, double fill_ratio, int nesting_radius,
                  std::vector<std::vector<IBox>> *out, int *new_finest, std::string *err,
                  const int *periodic) {
  int c = 1, maxlen = 1;
  if (!lattice_params(block_factor, max_grid_size, &c, &maxlen, err)) return -1;
  if (!(fill_ratio > 0.0)) {
    if (err) *err = "regrid: fill_ratio must be positive";
    return -1;
  }
  const int nlev = (int)tags.size();
  if (nlev < 1 || nlev > 24) {
    if (err) *err = "regrid: bad number of levels";
    return -1;
  }
  std::vector<IBox> dom(nlev + 1);
  dom[0] = domain0;
  for (int l = 0; l <= nlev; ++l) {
    if (l > 0)
      for (int d = 0; d < 3; ++d) {
        dom[l].lo[d] = dom[l - 1].lo[d] * 2;
        dom[l].hi[d] = dom[l - 1].hi[d] * 2 + 1;
      }
    if (l == nlev) break;
    for (int d = 0; d < 3; ++d) {
      if (dom[l].hi[d] < dom[l].lo[d] || dom[l].hi[d] > (1 << 29) || dom[l].lo[d] < -(1 << 29)) {
        if (err) *err = "regrid: empty or too large domain";
        return -1;
      }
      if (fdiv(dom[l].lo[d], c) * c != dom[l].lo[d] ||
          fdiv(dom[l].hi[d] + 1, c) * c != dom[l].hi[d] + 1) {
        if (err) *err = "regrid: a level's domain is not a multiple of the lattice spacing";
        return -1;
      }
      const LevelTags &t = tags[l];
      if (t.lat_n[d] < 0 || (t.lat_n[d] > 0 && !t.mask) || t.lat_lo[d] * (long)c < dom[l].lo[d] ||
          (t.lat_lo[d] + (long)t.lat_n[d]) * c > (long)dom[l].hi[d] + 1) {
        if (err) *err = "regrid: a tag lattice lies outside its level's domain";
        return -1;
      }
    }
  }
  out->assign(nlev, std::vector<IBox>());
  for (int l = nlev - 1; l >= 0; --l) {
    // nesting: the lattice cells of level l under boxes[l + 2] grown by
    // nesting_radius level-(l+1) cells; clipped to the level-(l+1) domain, or
    // in a periodic direction wrapped round it
    std::vector<IBox> nest;
    if (l + 1 < nlev)
      for (const IBox &f : (*out)[l + 1]) {
        // per direction: the lattice intervals under the grown region; one
        // when it is clipped, up to two when it wraps round a periodic domain
        int nr[3] = {0, 0, 0}, rlo[3][2], rhi[3][2];
        for (int d = 0; d < 3; ++d) {
          const int dlo = dom[l + 1].lo[d], dhi = dom[l + 1].hi[d], n = dhi - dlo + 1;
          int lo = fdiv(f.lo[d], 2) - nesting_radius, hi = fdiv(f.hi[d], 2) + nesting_radius;
          auto add = [&](int a, int z) {
            rlo[d][nr[d]] = fdiv(fdiv(a, 2), c);
            rhi[d][nr[d]] = fdiv(fdiv(z, 2), c);
            ++nr[d];
          };
          if (periodic && periodic[d]) {
            if ((long)hi - lo + 1 >= n) {
              add(dlo, dhi);
            } else {
              auto wrap = [&](int v) { return dlo + (int)((((long)v - dlo) % n + n) % n); };
              lo = wrap(lo);
              hi = wrap(hi);
              if (lo <= hi) {
                add(lo, hi);
              } else {  // through the face: the two ends of the domain
                add(dlo, hi);
                add(lo, dhi);
              }
            }
          } else {
            lo = std::max(lo, dlo);
            hi = std::min(hi, dhi);
            if (hi >= lo) add(lo, hi);
          }
        }
        for (int k = 0; k < nr[2]; ++k)
          for (int j = 0; j < nr[1]; ++j)
            for (int i = 0; i < nr[0]; ++i) {
              IBox b;
              b.lo[0] = rlo[0][i];
              b.hi[0] = rhi[0][i];
              b.lo[1] = rlo[1][j];
              b.hi[1] = rhi[1][j];
              b.lo[2] = rlo[2][k];
              b.hi[2] = rhi[2][k];
              nest.push_back(b);
            }
      }
    // the working lattice: the tag mask's region and the nesting cells
    const LevelTags &t = tags[l];
    const bool have_mask = t.lat_n[0] > 0 && t.lat_n[1] > 0 && t.lat_n[2] > 0;
    if (!have_mask && nest.empty()) continue;
    IBox w;
    bool first = true;
    auto merge = [&](const int *lo, const int *hi) {
      for (int d = 0; d < 3; ++d) {
        w.lo[d] = first ? lo[d] : std::min(w.lo[d], lo[d]);
        w.hi[d] = first ? hi[d] : std::max(w.hi[d], hi[d]);
      }
      first = false;
    };
    if (have_mask) {
      const int hi[3] = {t.lat_lo[0] + t.lat_n[0] - 1, t.lat_lo[1] + t.lat_n[1] - 1,
                         t.lat_lo[2] + t.lat_n[2] - 1};
      merge(t.lat_lo, hi);
    }
    for (const IBox &b : nest) merge(b.lo, b.hi);
    const int wn[3] = {w.hi[0] - w.lo[0] + 1, w.hi[1] - w.lo[1] + 1, w.hi[2] - w.lo[2] + 1};
    std::vector<unsigned char> work((size_t)wn[0] * wn[1] * wn[2], 0);
    auto widx = [&](int x, int y, int z) {
      return ((size_t)(z - w.lo[2]) * wn[1] + (y - w.lo[1])) * wn[0] + (x - w.lo[0]);
    };
    if (have_mask)
      for (int z = 0; z < t.lat_n[2]; ++z)
        for (int y = 0; y < t.lat_n[1]; ++y)
          for (int x = 0; x < t.lat_n[0]; ++x)
            if (t.mask[((size_t)z * t.lat_n[1] + y) * t.lat_n[0] + x])
              work[widx(t.lat_lo[0] + x, t.lat_lo[1] + y, t.lat_lo[2] + z)] = 1;
    for (const IBox &b : nest)
      for (int z = b.lo[2]; z <= b.hi[2]; ++z)
        for (int y = b.lo[1]; y <= b.hi[1]; ++y)
          for (int x = b.lo[0]; x <= b.hi[0]; ++x) work[widx(x, y, z)] = 1;
    std::vector<IBox> lat = cluster(work.data(), wn, fill_ratio, maxlen, nullptr);
    for (IBox &b : lat)  // lattice -> level l cells -> level l + 1 cells
      for (int d = 0; d < 3; ++d) {
        b.lo[d] = (b.lo[d] + w.lo[d]) * c * 2;
        b.hi[d] = (b.hi[d] + w.lo[d] + 1) * c * 2 - 1;
      }
    (*out)[l] = lat;
  }
  *new_finest = 0;
  for (int l = 0; l < nlev; ++l)
    if (!(*out)[l].empty()) *new_finest = l + 1;
  return 0;
}

std::vector<int> owners(const std::vector<IBox> &boxes, int size) {
  std::vector<int> own(boxes.size(), 0);
  if (size < 1) size = 1;
  long long total = 0;
  for (const IBox &b : boxes) total += volume(b);
  if (total <= 0) return own;
  long long prefix = 0;
  for (size_t i = 0; i < boxes.size(); ++i) {
    const long long cells = volume(boxes[i]);
    own[i] = (int)((long long)size * (2 * prefix + cells) / (2 * total));
    prefix += cells;
  }
  return own;
}

}  // namespace regrid
}  // namespace mgic
