// ptag.hpp -- host-side launcher of the periodic tagging kernel in ptag.hip
// (libmgic_ptag.so; include/mgic_ptag.h is the C ABI).
//
// The launcher works on ALL local boxes of a level at once: the caller cuts
// every box into tiles of kTileX x kTileY cells in x and y, and one launch
// covers the tiles of all boxes over every z plane.
#pragma once

#include <hip/hip_runtime.h>

namespace mgic {
namespace ptag {

constexpr int kTileX = 64;  // one wavefront along x
constexpr int kTileY = 4;   // 4 waves per block: the row block

// one tile of one box: rows [j0, j0 + kTileY) x cells [i0, i0 + kTileX) of
// every z plane of the box
struct Tile {
  const double *p;  // the box's valid-lo cell (mgic_field_device_ptr)
  long sy, sz;      // strides in doubles, sx = 1
  int glo[3];       // global index of the valid-lo cell
  int n[3];         // extent of the box in cells
  int i0, j0;       // the tile's low corner within the box
};

struct Args {
  int dom_lo[3], dom_hi[3];
  int lat_lo[3], lat_n[3];
  int periodic[3];
  int grow, c;
};

// mask[lattice cell] = 1 wherever a tagged cell (|cond| >= tag_val) of the
// tiles, grown by a.grow, reaches: clipped to the domain in a non-periodic
// direction, wrapped round it in a periodic one.  tiles: ntiles entries on
// the device; nz_max: the largest n[2] among them.  One launch.
void tag_lattice(unsigned char *mask, const Tile *tiles, int ntiles, int nz_max, double tag_val,
                 const Args &a, hipStream_t st);

}  // namespace ptag
}  // namespace mgic
