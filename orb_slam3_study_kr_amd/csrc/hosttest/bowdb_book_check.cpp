// bowdb_book_check.cpp -- BowDbBook of csrc/bowdb_book.h on plain host memory, for a run under a sanitizer: scripts of add, erase
// and clear run through the book the way bowdb_device.hip runs them, with malloc'ed stand-ins of the device arenas of exactly the
// book's capacities, next to a plain model (a list of live (handle, words) in add order).  After every step the live rows of the
// book, read through its row table out of the stand-in arena, equal the model.  A program of its own (`make bowdb-check`), in no
// library; it makes no HIP call and needs no device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <utility>

#include "../bowdb_book.h"

using namespace osh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } } while (0)

struct Arena {   // the stand-in of d_ids and d_rows
  uint32_t* ids = nullptr;
  BowDbRow* rows = nullptr;
  ~Arena() { std::free(ids); std::free(rows); }
};

// maintain() of bowdb_device.hip with memcpy in place of the kernel and the device copies
static void maintain(BowDbBook& book, Arena& a, size_t extra, size_t extra_rows) {
  const size_t old_cap = book.entry_cap;
  const BowDbPlan plan = book.prepare(extra, extra_rows);
  if (plan.fresh_arena) {
    uint32_t* ids = static_cast<uint32_t*>(std::malloc(book.entry_cap * sizeof(uint32_t)));
    for (size_t k = 0; k < plan.moves.size(); ++k) {
      const BowDbMove& m = plan.moves[k];
      CHECK(k == 0 ? m.dst == 0 : m.dst == plan.moves[k - 1].dst + plan.moves[k - 1].len);   // the runs tile the fresh arena
      CHECK((size_t)m.src + m.len <= old_cap && (size_t)m.dst + m.len <= book.entry_cap);
      std::memcpy(ids + m.dst, a.ids + m.src, m.len * sizeof(uint32_t));
    }
    std::free(a.ids);
    a.ids = ids;
  }
  if (plan.fresh_rows) {
    std::free(a.rows);
    a.rows = static_cast<BowDbRow*>(std::malloc(book.row_cap * sizeof(BowDbRow)));
  }
  if (plan.upload_rows && !book.row.empty()) std::memcpy(a.rows, book.row.data(), book.row.size() * sizeof(BowDbRow));
}

using Model = std::vector<std::pair<uint64_t, std::vector<uint32_t>>>;

static void compare(const BowDbBook& book, const Arena& a, const Model& model) {
  size_t live = 0, entries = 0, dead = 0;
  for (size_t r = 0; r < book.row.size(); ++r) {
    CHECK(r == 0 || book.handle[r] > book.handle[r - 1]);
    CHECK(std::memcmp(&a.rows[r], &book.row[r], sizeof(BowDbRow)) == 0);
    CHECK(book.row[r].start == entries);                                   // the rows tile the used arena
    entries += (size_t)book.row[r].len;
    if (!book.row[r].alive) { dead += (size_t)book.row[r].len; CHECK(book.find(book.handle[r]) == -1); continue; }
    CHECK(live < model.size());
    if (live >= model.size()) return;
    CHECK(book.handle[r] == model[live].first && book.find(book.handle[r]) == (int)r);
    CHECK((size_t)book.row[r].len == model[live].second.size());
    CHECK(book.row[r].len == 0 || std::memcmp(a.ids + book.row[r].start, model[live].second.data(), (size_t)book.row[r].len * 4) == 0);
    ++live;
  }
  CHECK(live == model.size() && live == book.live_rows);
  CHECK(entries == book.entries && dead == book.dead_entries && entries <= book.entry_cap && book.row.size() <= book.row_cap);
  CHECK(book.find(0) == -1 && book.find(book.next_handle) == -1);
}

static void script(unsigned seed, int steps, int max_len, double p_erase, double p_clear, int min_compactions, int min_reallocations) {
  std::mt19937 rng(seed);
  BowDbBook book;
  Arena a;
  Model model;
  uint32_t word = 0;
  for (int s = 0; s < steps; ++s) {
    const double u = std::uniform_real_distribution<double>(0, 1)(rng);
    if (u < p_clear) {
      book.clear(); model.clear();
    } else if (u < p_clear + p_erase && !model.empty()) {
      const size_t k = rng() % model.size();
      const uint64_t h = model[k].first;
      CHECK(book.find(h) >= 0);
      maintain(book, a, 0, 0);
      const int r = book.find(h);
      book.erase(r);
      a.rows[r] = book.row[r];
      model.erase(model.begin() + (long)k);
    } else {
      const int n = (int)(rng() % (unsigned)(max_len + 1));
      std::vector<uint32_t> w((size_t)n);
      for (auto& x : w) x = word++;
      maintain(book, a, (size_t)n, 1);
      const uint64_t expect = book.next_handle;
      const int r = book.append(n);
      CHECK(book.handle[r] == expect && (size_t)r + 1 == book.row.size());
      if (n) std::memcpy(a.ids + book.row[r].start, w.data(), (size_t)n * 4);
      a.rows[r] = book.row[r];
      model.emplace_back(expect, std::move(w));
    }
    compare(book, a, model);
  }
  std::printf("seed %u: %d steps, %zu live of %zu rows, %zu entries of %zu, %lld compactions, %lld reallocations\n", seed, steps,
              book.live_rows, book.row.size(), book.entries, book.entry_cap, (long long)book.compactions, (long long)book.reallocations);
  CHECK(book.compactions >= min_compactions && book.reallocations >= min_reallocations);
}

int main() {
  script(1, 6000, 700, 0.30, 0.0, 2, 4);      // the arenas outgrow their first capacity twice; erases force compactions
  script(2, 5000, 3, 0.20, 0.0, 0, 4);     // short and empty rows: the row table outgrows its first capacity twice
  script(3, 3000, 2000, 0.60, 0.003, 100, 2);   // mostly erasing, with a clear now and then
  int64_t at = -1;
  const int32_t ok[] = {0, 3, 4, 9}, dup[] = {1, 2, 2}, desc[] = {5, 4}, out[] = {1, 10}, neg[] = {-1, 2};
  CHECK(bowdb_check_words(4, ok, 10, &at) == 0 && bowdb_check_words(0, nullptr, 10, &at) == 0);
  CHECK(bowdb_check_words(3, dup, 10, &at) == 1 && at == 2);
  CHECK(bowdb_check_words(2, desc, 10, &at) == 1 && at == 1);
  CHECK(bowdb_check_words(2, out, 10, &at) == 2 && at == 1);
  CHECK(bowdb_check_words(2, neg, 10, &at) == 2 && at == 0);
  std::printf(failures ? "FAILED: %d checks\n" : "bowdb_book_check ok\n", failures);
  return failures ? 1 : 0;
}
