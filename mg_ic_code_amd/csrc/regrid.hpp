// regrid.hpp -- host side of set_grids (SetGrids.cpp:31-149): Berger-Rigoutsos
// clustering of a tag lattice into boxes, the top-down pass over the levels
// with proper nesting, and the LoadBalance stand-in.
//
// No HIP in here: integer arithmetic on byte masks, one comparison in double
// (n >= fill_ratio * volume).  The algorithm is the one DESIGN.md 3f writes
// out; it restates Chombo's BRMeshRefine and is not pinned against it.
#pragma once

#include <string>
#include <vector>

namespace mgic {
namespace regrid {

// inclusive integer box, x first
struct IBox {
  int lo[3];
  int hi[3];
};

// lattice spacing in level cells (new boxes of the next level are then
// block_factor-aligned) and the longest box side in lattice cells.  false
// (err set) when block_factor is not a power of two or max_grid_size < 1.
bool lattice_params(int block_factor, int max_grid_size, int *c, int *maxlen, std::string *err);

// cluster the set cells of mask (n[0] fastest) into disjoint boxes in mask
// indices, sorted by (lo_z, lo_y, lo_x).  presplit (may be null) receives the
// boxes as accepted, before split_max cuts them to maxlen.
std::vector<IBox> cluster(const unsigned char *mask, const int n[3], double fill_ratio, int maxlen,
                          std::vector<IBox> *presplit);

// one level's tags: a byte mask over lattice cells [lat_lo, lat_lo + lat_n)
// (lattice indices = level cells / c, floored)
struct LevelTags {
  const unsigned char *mask;
  int lat_lo[3];
  int lat_n[3];
};

// BRMeshRefine::regrid stand-in, top-down: tags[0..top] -> boxes[1..top+1]
// (out[l] = the boxes of level l + 1 in that level's cells; may be empty).
// domain0: the level-0 domain box.  Returns 0 or -1 (err set); *new_finest =
// the highest level with boxes (0: none).  periodic (null: no direction):
// in a direction with periodic[d] != 0 the nesting region of a box is not
// clipped to the domain but wrapped round it; clustering runs
// inside the domain either way, so no box crosses a face.
int regrid_levels(const std::vector<LevelTags> &tags, const IBox &domain0, int block_factor,
                  int max_grid_size, double fill_ratio, int nesting_radius,
                  std::vector<std::vector<IBox>> *out, int *new_finest, std::string *err,
                  const int *periodic = nullptr);

// LoadBalance stand-in: box i of the (sorted) list goes to rank
// floor(size * (prefix_i + cells_i / 2) / total)
std::vector<int> owners(const std::vector<IBox> &boxes, int size);

}  // namespace regrid
}  // namespace mgic
