// orb_grid_bin.h -- Frame::AssignFeaturesToGrid (src/Frame.cc:397-417) with PosInGrid (:726-736) for one keypoint set: a counting
// sort by cell, keypoint order inside a cell.  Host code of the grid upload (osh_orb_upload_grid, orb_device.hip) and of the fuse
// search (osh_orb_fuse_search, orb_fuse_device.hip); plain C++, so the test library bins with the same statements.
#pragma once
#include <cmath>
#include <vector>

namespace osh {

// Cell x * rows + y of a keypoint, or -1 outside the grid.
inline int grid_cell_of(float x, float y, float min_x, float min_y, float winv, float hinv, int cols, int rows) {
  const int posX = (int)std::round((x - min_x) * winv);
  const int posY = (int)std::round((y - min_y) * hinv);
  return (posX < 0 || posX >= cols || posY < 0 || posY >= rows) ? -1 : posX * rows + posY;
}

// off [cols*rows + 1], all zero on entry: the keypoints of cell c are idx[off[c] .. off[c + 1]) on return (idx [n]; a keypoint outside
// the grid is in no cell).  Returns the largest number of keypoints in one cell; more than `max_per_cell` and idx is not filled.
inline int bin_keypoints(const float* xy, int n, float min_x, float min_y, float winv, float hinv, int cols, int rows, int max_per_cell,
                         int* off, int* idx, std::vector<int>& cell_of, std::vector<int>& fill) {
  const int ncell = cols * rows;
  cell_of.resize((size_t)(n > 0 ? n : 1));
  for (int i = 0; i < n; ++i) {
    cell_of[i] = grid_cell_of(xy[2 * i], xy[2 * i + 1], min_x, min_y, winv, hinv, cols, rows);
    if (cell_of[i] >= 0) off[cell_of[i] + 1]++;
  }
  int most = 0;
  for (int k = 0; k < ncell; ++k) {
    if (off[k + 1] > most) most = off[k + 1];
    off[k + 1] += off[k];
  }
  if (most > max_per_cell) return most;
  fill.assign(off, off + ncell);
  for (int i = 0; i < n; ++i) if (cell_of[i] >= 0) idx[fill[cell_of[i]]++] = i;
  return most;
}

}  // namespace osh
