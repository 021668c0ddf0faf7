// bowdb_book.h -- the host-side bookkeeping of osh_bow_db (bowdb_device.hip), with no HIP call: which row a handle names, how many
// arena entries belong to erased rows, when the arena is compacted and to which sizes the buffers grow.  bowdb_device.hip carries
// out on the device what the book decides; hosttest/bowdb_book_check.cpp (`make bowdb-check`) and osh_host_bowdb_book_replay run it
// alone.
//
// Rows sit in add order and a handle only ever grows, so the handles of the row table ascend: a handle is found by bisection, and
// ascending row order is ascending handle order.  An erased row keeps its place (alive = 0) until a compaction drops it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace osh {

constexpr size_t kBowDbMaxRows = (size_t)1 << 20;      // rows of the table, erased ones included; past it OSH_ERR_UNSUPPORTED
constexpr size_t kBowDbMaxEntries = (size_t)1 << 31;   // a row's start is a uint32_t
constexpr size_t kBowDbFirstRowCap = 1024;
constexpr size_t kBowDbFirstEntryCap = (size_t)1 << 18;

// 0 if id[0..n) ascends strictly inside [0, n_words); else 1 (not ascending or a duplicate) or 2 (outside the vocabulary), *at the
// first offender
inline int bowdb_check_words(int64_t n, const int32_t* id, int64_t n_words, int64_t* at) {
  for (int64_t i = 0; i < n; ++i) {
    if (id[i] < 0 || (int64_t)id[i] >= n_words) { *at = i; return 2; }
    if (i > 0 && id[i] <= id[i - 1]) { *at = i; return 1; }
  }
  return 0;
}

struct BowDbRow { uint32_t start; int32_t len; int32_t alive; int32_t pad; };   // as the kernels read it
struct BowDbMove { uint32_t src, dst, len; };                                   // a run of entries that survives a compaction

// What a mutation has the device do before it touches a row (BowDbBook::prepare)
struct BowDbPlan {
  bool fresh_arena = false;       // allocate a pair of arenas of entry_cap entries and fill them from the old pair by `moves`
  std::vector<BowDbMove> moves;
  bool fresh_rows = false;        // allocate a row table of row_cap rows
  bool upload_rows = false;       // then send the whole row table
};

struct BowDbBook {
  std::vector<uint64_t> handle;   // ascending
  std::vector<BowDbRow> row;
  uint64_t next_handle = 1;
  size_t entries = 0, dead_entries = 0, live_rows = 0;   // entries: the used part of the arena
  size_t row_cap = 0, entry_cap = 0;                     // what the device buffers hold
  int64_t compactions = 0, reallocations = 0;

  // the row of a live handle, -1 for one that was erased or never given out
  int find(uint64_t h) const {
    const auto it = std::lower_bound(handle.begin(), handle.end(), h);
    if (it == handle.end() || *it != h) return -1;
    const int r = (int)(it - handle.begin());
    return row[r].alive ? r : -1;
  }
  // dead entries exceed half of the used arena, or only erased rows keep the table at its limit
  bool needs_compaction() const { return dead_entries * 2 > entries || (row.size() >= kBowDbMaxRows && live_rows < row.size()); }
  // Drops the erased rows and moves the others up, order and handles kept; returns the runs of entries to copy from the old arena
  // into a fresh one (neighbouring survivors are one run)
  std::vector<BowDbMove> compact() {
    std::vector<BowDbMove> moves;
    size_t keep = 0, at = 0;
    for (size_t r = 0; r < row.size(); ++r) {
      if (!row[r].alive) continue;
      const BowDbRow old = row[r];
      if (old.len > 0) {
        if (!moves.empty() && moves.back().src + moves.back().len == old.start) moves.back().len += (uint32_t)old.len;
        else moves.push_back({old.start, (uint32_t)at, (uint32_t)old.len});
      }
      handle[keep] = handle[r];
      row[keep] = {(uint32_t)at, old.len, 1, 0};
      at += (size_t)old.len;
      ++keep;
    }
    handle.resize(keep); row.resize(keep);
    entries = at; dead_entries = 0;
    ++compactions;
    return moves;
  }
  // the capacity that holds `extra` more entries (rows): the present one if it does, else doubled until it does
  size_t entry_cap_for(size_t extra) const { return grown(entry_cap, entries + extra, kBowDbFirstEntryCap); }
  size_t row_cap_for(size_t extra) const { return grown(row_cap, row.size() + extra, kBowDbFirstRowCap); }
  static size_t grown(size_t cap, size_t need, size_t first) {
    if (need <= cap) return cap;
    size_t c = std::max(cap, first);
    while (c < need) c *= 2;
    return c;
  }
  // What every add and erase does first: the compaction if one is due, then room for `extra` more entries and `extra_rows` more
  // rows.  The book is as after the plan; the caller carries the plan out
  BowDbPlan prepare(size_t extra, size_t extra_rows) {
    BowDbPlan p;
    if (needs_compaction()) { p.moves = compact(); p.fresh_arena = p.upload_rows = true; }
    const size_t cap = entry_cap_for(extra);
    if (cap != entry_cap) {
      if (!p.fresh_arena && entries) p.moves.push_back({0, 0, (uint32_t)entries});   // growth alone: the used part as it lies
      p.fresh_arena = true;
      entry_cap = cap; ++reallocations;
    }
    const size_t rows = row_cap_for(extra_rows);
    if (rows != row_cap) { row_cap = rows; ++reallocations; p.fresh_rows = p.upload_rows = true; }
    return p;
  }
  // a new last row of n entries; its index
  int append(int32_t n) {
    handle.push_back(next_handle++);
    row.push_back({(uint32_t)entries, n, 1, 0});
    entries += (size_t)n;
    ++live_rows;
    return (int)row.size() - 1;
  }
  void erase(int r) {
    row[r].alive = 0;
    dead_entries += (size_t)row[r].len;
    --live_rows;
  }
  // no row left; handles go on counting and the buffers keep their sizes
  void clear() {
    handle.clear(); row.clear();
    entries = dead_entries = live_rows = 0;
  }
};

}  // namespace osh
