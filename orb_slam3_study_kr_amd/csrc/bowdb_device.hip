// bowdb_device.hip -- the inverted-file walk and the L1 scores of KeyFrameDatabase::DetectNBestCandidates and
// DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:604-845, Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) on MI355X (gfx950).
//
// The database (osh_bow_db) is an object of its own, resident once per device and mutable: one row per added BowVector in add order,
// the word ids (uint32) and values (double) of all rows one after another in two grow-only arenas, and a row table of start,
// length and alive flag.  bowdb_book.h decides what a handle names, when the arenas are compacted and how they grow; this file
// carries it out.  A query writes nothing into the database: its scratch and outputs live in the arena of the calling osh_orb_ctx,
// on its stream, so any number of contexts query one database at once under a shared lock.  add, erase and clear take the lock
// exclusively and return with their device work complete.
//
// Three kernels per call, every query of the batch in each:
//   k_bowdb_count  blocks of four wavefronts, persistent over the rows of the table; the query's word ids are staged once per
//                  block in LDS.  One wavefront per row: the lanes stride over the row's words, each looks its word up in LDS by
//                  bisection; ballot + popcount is the number of shared words, the first hit (the rows ascend) the smallest shared
//                  word.  The maximum over the rows that are not excluded goes into the query's header by an integer atomicMax.
//   k_bowdb_emit   one block per query: the rows with a shared word, compacted in row order (= ascending handle) by a ballot scan;
//                  min_common = (int)((float)max_common * 0.8f) (:648) and with it which rows are scored.
//   k_bowdb_score  as k_bowdb_count over the compacted list, scored rows only: the lanes compute the terms
//                  (|v - w| - |v|) - |w| of 64 words of the row at once, then the terms of the shared words are added in lane order,
//                  chunk after chunk: one sequential FP64 chain in ascending word order, as the reference's loop.  No product, so
//                  nothing to contract.
// Only the headers and the listed rows travel back.
#include "bowdb_book.h"
#include "common.h"
#include "orb_stage.h"
#include <climits>
#include <cmath>
#include <mutex>
#include <shared_mutex>
#include <vector>

namespace osh {

static_assert(kBowDbMaxRows == OSH_BOW_DB_MAX_ROWS, "the header states the book's row limit");
constexpr int kBowDbThreads = 256;                     // four wavefronts
constexpr int kBowDbWaves = kBowDbThreads / 64;
constexpr size_t kBowDbMaxBatchRows = (size_t)1 << 26; // queries x rows of one call: 32 bytes of scratch each

struct BowDbQueryDev { int n, base, n_ex, ex_base; };  // base, ex_base: offsets in the word and exclusion arrays of the batch
struct BowDbHead { int max_common, min_common, n_listed, pad; };
struct BowDbEntry { double score; int row, common, first_word, scored; };

struct BowDbView {
  const BowDbRow* rows; int n_rows;
  const uint32_t* ids; const double* vals;             // the database's arenas
  const BowDbQueryDev* q;
  const uint32_t* q_word; const double* q_val;
  const int* ex;                                       // per query its excluded rows, ascending
  int* common; int* first;                             // [n_queries * n_rows] work
  BowDbHead* head;                                     // [n_queries] out, zero before k_bowdb_count
  BowDbEntry* entry;                                   // [n_queries * n_rows] work: the first n_listed of a query are its list
};

// the position of w in the ascending sh[0..n), -1 if it is not there
__device__ inline int bowdb_find(const uint32_t* sh, int n, uint32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (sh[mid] < w) lo = mid + 1; else hi = mid;
  }
  return lo < n && sh[lo] == w ? lo : -1;
}

__device__ inline bool bowdb_excluded(const int* ex, int n, int row) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ex[mid] < row) lo = mid + 1; else hi = mid;
  }
  return lo < n && ex[lo] == row;
}

__device__ inline void bowdb_stage_words(uint32_t* sh, const BowDbView& v, const BowDbQueryDev& q) {
  for (int i = threadIdx.x; i < q.n; i += kBowDbThreads) sh[i] = v.q_word[q.base + i];
  __syncthreads();
}

// grid = (blocks, n_queries), block = 256, dynamic LDS = 4 bytes * (the longest query)
__global__ __launch_bounds__(kBowDbThreads) void k_bowdb_count(BowDbView v) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sh_word[];
  const BowDbQueryDev q = v.q[blockIdx.y];
  bowdb_stage_words(sh_word, v, q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t o = (size_t)blockIdx.y * (size_t)v.n_rows;
  int best = 0;
  for (int r = blockIdx.x * kBowDbWaves + wave; r < v.n_rows; r += gridDim.x * kBowDbWaves) {
    const BowDbRow m = v.rows[r];                      // the same address in every lane: the loops below are wavefront-uniform
    int common = 0, first = -1;
    if (m.alive)
      for (int i0 = 0; i0 < m.len; i0 += 64) {
        const int i = i0 + lane;
        uint32_t w = 0;
        bool hit = false;
        if (i < m.len) { w = v.ids[(size_t)m.start + i]; hit = bowdb_find(sh_word, q.n, w) >= 0; }
        const unsigned long long b = __ballot(hit);
        if (b) {
          if (first < 0) first = __shfl((int)w, __ffsll((long long)b) - 1);
          common += __popcll(b);
        }
      }
    if (lane == 0) {
      v.common[o + r] = common; v.first[o + r] = first;
      if (common > best && !bowdb_excluded(v.ex + q.ex_base, q.n_ex, r)) best = common;
    }
  }
  if (lane == 0 && best > 0) atomicMax(&v.head[blockIdx.y].max_common, best);
}

// grid = n_queries, block = 256
__global__ __launch_bounds__(kBowDbThreads) void k_bowdb_emit(BowDbView v) {
  __shared__ int sh_count[kBowDbWaves];
  const BowDbQueryDev q = v.q[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t o = (size_t)blockIdx.x * (size_t)v.n_rows;
  const int max_common = v.head[blockIdx.x].max_common;
  const int min_common = (int)((float)max_common * 0.8f);
  int listed = 0;
  for (int r0 = 0; r0 < v.n_rows; r0 += kBowDbThreads) {
    const int r = r0 + (int)threadIdx.x;
    const int c = r < v.n_rows ? v.common[o + r] : 0;
    const unsigned long long b = __ballot(c > 0);
    if (lane == 0) sh_count[wave] = __popcll(b);
    __syncthreads();
    int before = listed, total = 0;
    for (int w = 0; w < kBowDbWaves; ++w) { if (w < wave) before += sh_count[w]; total += sh_count[w]; }
    if (c > 0) {
      BowDbEntry e;
      e.score = 0.0; e.row = r; e.common = c; e.first_word = v.first[o + r];
      e.scored = c > min_common && !bowdb_excluded(v.ex + q.ex_base, q.n_ex, r);
      v.entry[o + before + __popcll(b & ((1ull << lane) - 1))] = e;
    }
    listed += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) { v.head[blockIdx.x].min_common = min_common; v.head[blockIdx.x].n_listed = listed; }
}

// grid = (blocks, n_queries), block = 256, dynamic LDS as k_bowdb_count
__global__ __launch_bounds__(kBowDbThreads) void k_bowdb_score(BowDbView v) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) uint32_t sh_word[];
  const BowDbQueryDev q = v.q[blockIdx.y];
  bowdb_stage_words(sh_word, v, q);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  BowDbEntry* list = v.entry + (size_t)blockIdx.y * (size_t)v.n_rows;
  const int n_listed = v.head[blockIdx.y].n_listed;
  for (int k = blockIdx.x * kBowDbWaves + wave; k < n_listed; k += gridDim.x * kBowDbWaves) {
    if (!list[k].scored) continue;                     // wavefront-uniform
    const BowDbRow m = v.rows[list[k].row];
    double sum = 0.0;
    for (int i0 = 0; i0 < m.len; i0 += 64) {
      const int i = i0 + lane;
      int p = -1;
      if (i < m.len) p = bowdb_find(sh_word, q.n, v.ids[(size_t)m.start + i]);
      double term = 0.0;
      if (p >= 0) {
        const double vi = v.q_val[q.base + p], wi = v.vals[(size_t)m.start + i];
        term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
      }
      unsigned long long b = __ballot(p >= 0);
      while (b) {                                      // the shared words of the chunk, ascending: every lane adds the same chain
        sum += __shfl(term, __ffsll((long long)b) - 1);
        b &= b - 1;
      }
    }
    if (lane == 0) list[k].score = -sum / 2.0;
  }
}

// grid = min(n_moves, 1024), block = 256: the surviving runs of a compaction, old arenas -> fresh arenas
__global__ __launch_bounds__(kBowDbThreads) void k_bowdb_move(const BowDbMove* moves, int n_moves, const uint32_t* ids, const double* vals,
                                                              uint32_t* new_ids, double* new_vals) {
  for (int k = blockIdx.x; k < n_moves; k += gridDim.x) {
    const BowDbMove m = moves[k];
    for (uint32_t i = threadIdx.x; i < m.len; i += kBowDbThreads) {
      new_ids[(size_t)m.dst + i] = ids[(size_t)m.src + i];
      new_vals[(size_t)m.dst + i] = vals[(size_t)m.src + i];
    }
  }
}

struct BowDbState {
  StagedCall call;
  PinBuf h_entry;
  double ms[4] = {0, 0, 0, 0};
};

// hipMalloc for a buffer of the database, zero-filled under OSH_ZERO_NEW_BUFFERS=1
static int bowdb_alloc(void** p, size_t bytes) {
  OSH_HIP(hipMalloc(p, std::max<size_t>(bytes, 256)));
  return zero_new_device(*p, std::max<size_t>(bytes, 256));
}

}  // namespace osh

using namespace osh;

struct osh_bow_db {
  int device = 0;
  int64_t n_words = 0;
  hipStream_t stream = nullptr;           // the mutations' copies and the compaction kernel
  std::shared_mutex mutex;                // shared: queries; exclusive: add, erase, clear, info's view stays consistent
  BowDbBook book;
  uint32_t* d_ids = nullptr;
  double* d_vals = nullptr;
  BowDbRow* d_rows = nullptr;
  bool broken = false;                    // a device call failed half way through a mutation

  // the row table, rows [first, first + count)
  int upload_rows(size_t first, size_t count) {
    if (count) OSH_HIP(hipMemcpyAsync(d_rows + first, book.row.data() + first, count * sizeof(BowDbRow), hipMemcpyHostToDevice, stream));
    return OSH_OK;
  }
  // What a mutation does first (BowDbBook::prepare): the compaction if one is due, then room for `extra` entries and `extra_rows` rows
  int maintain(size_t extra, size_t extra_rows) {
    const size_t old_entry_cap = book.entry_cap;
    const BowDbPlan plan = book.prepare(extra, extra_rows);
    if (plan.fresh_arena) {
      uint32_t* ids = nullptr; double* vals = nullptr; BowDbMove* d_moves = nullptr;
      int rc = bowdb_alloc((void**)&ids, book.entry_cap * sizeof(uint32_t));
      if (rc == OSH_OK) rc = bowdb_alloc((void**)&vals, book.entry_cap * sizeof(double));
      for (const BowDbMove& m : plan.moves)
        if ((size_t)m.src + m.len > old_entry_cap || (size_t)m.dst + m.len > book.entry_cap) { set_error("bow database: a move outside the arenas"); rc = OSH_ERR_DEVICE; }
      if (rc == OSH_OK && plan.moves.size() == 1) {        // growth, or one surviving run: device-to-device copies
        const BowDbMove m = plan.moves[0];
        if (hipMemcpyAsync(ids + m.dst, d_ids + m.src, (size_t)m.len * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(vals + m.dst, d_vals + m.src, (size_t)m.len * sizeof(double), hipMemcpyDeviceToDevice, stream) != hipSuccess) {
          set_error("bow database: device-to-device copy failed"); rc = OSH_ERR_DEVICE;
        }
      } else if (rc == OSH_OK && plan.moves.size() > 1) {  // the surviving runs of a compaction
        rc = bowdb_alloc((void**)&d_moves, plan.moves.size() * sizeof(BowDbMove));
        if (rc == OSH_OK && hipMemcpyAsync(d_moves, plan.moves.data(), plan.moves.size() * sizeof(BowDbMove), hipMemcpyHostToDevice, stream) != hipSuccess) {
          set_error("bow database: upload of the compaction's moves failed"); rc = OSH_ERR_DEVICE;
        }
        if (rc == OSH_OK) {
          hipLaunchKernelGGL(k_bowdb_move, dim3((unsigned)std::min<size_t>(plan.moves.size(), 1024)), dim3(kBowDbThreads), 0, stream,
                             d_moves, (int)plan.moves.size(), d_ids, d_vals, ids, vals);
          rc = launch_check("bow database compaction");
        }
      }
      if (rc == OSH_OK && hipStreamSynchronize(stream) != hipSuccess) { set_error("bow database: the copy into the fresh arenas did not complete"); rc = OSH_ERR_DEVICE; }
      if (d_moves) (void)hipFree(d_moves);
      if (rc != OSH_OK) { if (ids) (void)hipFree(ids); if (vals) (void)hipFree(vals); return OSH_ERR_DEVICE; }
      if (d_ids) (void)hipFree(d_ids);
      if (d_vals) (void)hipFree(d_vals);
      d_ids = ids; d_vals = vals;
    }
    if (plan.fresh_rows) {                                 // the row table is the book's: a larger one is filled from the host
      BowDbRow* rows = nullptr;
      if (bowdb_alloc((void**)&rows, book.row_cap * sizeof(BowDbRow)) != OSH_OK) return OSH_ERR_DEVICE;
      if (d_rows) (void)hipFree(d_rows);
      d_rows = rows;
    }
    if (plan.upload_rows) OSH_TRY(upload_rows(0, book.row.size()));
    return OSH_OK;
  }
};

// runs `body` under the exclusive lock and returns once the device has completed it
template <class F>
static int bowdb_mutate(osh_bow_db* db, const char* entry, F body) {
  std::unique_lock<std::shared_mutex> lock(db->mutex);
  if (db->broken) { set_error("%s: an earlier device error left the database unusable", entry); return OSH_ERR_DEVICE; }
  OSH_HIP(hipSetDevice(db->device));
  int rc = body();
  if (rc == OSH_OK && hipStreamSynchronize(db->stream) != hipSuccess) { set_error("%s: the device work did not complete", entry); rc = OSH_ERR_DEVICE; }
  if (rc == OSH_ERR_DEVICE) db->broken = true;
  return rc;
}

extern "C" int osh_bow_db_create(int device, int64_t n_words, osh_bow_db** out) {
  if (!out) { set_error("osh_bow_db_create: out is NULL"); return OSH_ERR_INVALID; }
  *out = nullptr;
  if (n_words < 1 || n_words > INT_MAX) { set_error("osh_bow_db_create: a vocabulary of %lld words", (long long)n_words); return OSH_ERR_INVALID; }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_error("no HIP device visible"); return OSH_ERR_NO_DEVICE; }
  if (device < 0 || device >= n_dev) { set_error("device %d out of range (have %d)", device, n_dev); return OSH_ERR_INVALID; }
  OSH_HIP(hipSetDevice(device));
  osh_bow_db* db = new osh_bow_db();
  db->device = device; db->n_words = n_words;
  if (hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking) != hipSuccess) { set_error("osh_bow_db_create: no stream"); delete db; return OSH_ERR_DEVICE; }
  *out = db;
  return OSH_OK;
}

extern "C" void osh_bow_db_destroy(osh_bow_db* db) {
  if (!db) return;
  (void)hipSetDevice(db->device);
  (void)hipDeviceSynchronize();   // no query of any context may still read it
  if (db->d_ids) (void)hipFree(db->d_ids);
  if (db->d_vals) (void)hipFree(db->d_vals);
  if (db->d_rows) (void)hipFree(db->d_rows);
  if (db->stream) (void)hipStreamDestroy(db->stream);
  delete db;
}

// What add and query refuse in a word list
static int bowdb_words_check(const char* entry, const osh_bow_db* db, int64_t n, const int32_t* word_id, const double* value) {
  if (n < 0 || (n && (!word_id || !value))) { set_error("%s: negative word count or NULL arrays", entry); return OSH_ERR_INVALID; }
  if (n > OSH_BOW_MAX_FEATURES) { set_error("%s: %lld words exceed %d", entry, (long long)n, OSH_BOW_MAX_FEATURES); return OSH_ERR_UNSUPPORTED; }
  int64_t at = 0;
  const int bad = bowdb_check_words(n, word_id, db->n_words, &at);
  if (bad == 1) { set_error("%s: word ids must ascend without duplicates (entry %lld)", entry, (long long)at); return OSH_ERR_INVALID; }
  if (bad == 2) { set_error("%s: word id %d outside the vocabulary of %lld words", entry, word_id[at], (long long)db->n_words); return OSH_ERR_INVALID; }
  return OSH_OK;
}

extern "C" int osh_bow_db_add(osh_bow_db* db, int32_t n, const int32_t* word_id, const double* value, uint64_t* handle) {
  if (!db || !handle) { set_error("osh_bow_db_add: bad arguments"); return OSH_ERR_INVALID; }
  OSH_TRY(bowdb_words_check("osh_bow_db_add", db, n, word_id, value));
  return bowdb_mutate(db, "osh_bow_db_add", [&]() -> int {
    BowDbBook& book = db->book;
    if (book.live_rows >= kBowDbMaxRows) { set_error("osh_bow_db_add: the database holds its limit of %zu rows", kBowDbMaxRows); return OSH_ERR_UNSUPPORTED; }
    if (book.entries - (book.needs_compaction() ? book.dead_entries : 0) + (size_t)n > kBowDbMaxEntries) {
      set_error("osh_bow_db_add: more than %zu entries", kBowDbMaxEntries);
      return OSH_ERR_UNSUPPORTED;
    }
    if (!book.needs_compaction() && book.row.size() >= kBowDbMaxRows) { set_error("osh_bow_db_add: row table full"); return OSH_ERR_UNSUPPORTED; }
    OSH_TRY(db->maintain((size_t)n, 1));
    const int r = book.append(n);
    const size_t start = book.row[r].start;
    if (n) {
      static_assert(sizeof(int32_t) == sizeof(uint32_t), "word ids are copied as they are");
      OSH_HIP(hipMemcpyAsync(db->d_ids + start, word_id, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, db->stream));
      OSH_HIP(hipMemcpyAsync(db->d_vals + start, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice, db->stream));
    }
    OSH_TRY(db->upload_rows((size_t)r, 1));
    *handle = book.handle[r];
    return OSH_OK;
  });
}

extern "C" int osh_bow_db_erase(osh_bow_db* db, uint64_t handle) {
  if (!db) { set_error("osh_bow_db_erase: no database"); return OSH_ERR_INVALID; }
  return bowdb_mutate(db, "osh_bow_db_erase", [&]() -> int {
    if (db->book.find(handle) < 0) { set_error("osh_bow_db_erase: handle %llu names no live row", (unsigned long long)handle); return OSH_ERR_INVALID; }
    OSH_TRY(db->maintain(0, 0));
    const int r = db->book.find(handle);   // a compaction moved it
    db->book.erase(r);
    return db->upload_rows((size_t)r, 1);
  });
}

extern "C" int osh_bow_db_clear(osh_bow_db* db) {
  if (!db) { set_error("osh_bow_db_clear: no database"); return OSH_ERR_INVALID; }
  return bowdb_mutate(db, "osh_bow_db_clear", [&]() -> int { db->book.clear(); return OSH_OK; });
}

extern "C" int osh_bow_db_info(osh_bow_db* db, int64_t info[6]) {
  if (!db || !info) { set_error("osh_bow_db_info: bad arguments"); return OSH_ERR_INVALID; }
  std::shared_lock<std::shared_mutex> lock(db->mutex);
  const BowDbBook& b = db->book;
  info[0] = (int64_t)b.live_rows; info[1] = (int64_t)b.row.size(); info[2] = (int64_t)b.entries; info[3] = (int64_t)b.entry_cap;
  info[4] = b.compactions; info[5] = b.reallocations;
  return OSH_OK;
}

extern "C" int osh_orb_bow_db_query(osh_orb_ctx* c, osh_bow_db* db, int32_t n_queries, const osh_bow_db_query* queries,
                                    const osh_bow_db_result* results) {
  if (!c || !db || n_queries < 0 || (n_queries && (!queries || !results))) { set_error("osh_orb_bow_db_query: bad arguments"); return OSH_ERR_INVALID; }
  if (n_queries == 0) return OSH_OK;
  PhaseClock clock;
  std::shared_lock<std::shared_mutex> lock(db->mutex);
  if (db->broken) { set_error("osh_orb_bow_db_query: an earlier device error left the database unusable"); return OSH_ERR_DEVICE; }
  const BowDbBook& book = db->book;
  const size_t n_rows = book.row.size();
  if ((size_t)n_queries * std::max<size_t>(n_rows, 1) > kBowDbMaxBatchRows) {
    set_error("osh_orb_bow_db_query: %d queries x %zu rows exceed %zu; split the batch", n_queries, n_rows, kBowDbMaxBatchRows);
    return OSH_ERR_UNSUPPORTED;
  }
  size_t NT = 0, NE = 0;
  int max_n = 0;
  std::vector<BowDbQueryDev> qd(n_queries);
  std::vector<int> ex;                      // the live excluded rows of every query, ascending inside a query
  for (int k = 0; k < n_queries; ++k) {
    const osh_bow_db_query& q = queries[k];
    OSH_TRY(bowdb_words_check("osh_orb_bow_db_query", db, q.n, q.word_id, q.value));
    if (q.n_excluded < 0 || (q.n_excluded && !q.excluded)) { set_error("query %d: negative exclusion count or NULL list", k); return OSH_ERR_INVALID; }
    const size_t ex_base = ex.size();
    for (int e = 0; e < q.n_excluded; ++e) {
      const int r = book.find(q.excluded[e]);
      if (r >= 0) ex.push_back(r);          // a handle that names no live row excludes nothing
    }
    std::sort(ex.begin() + ex_base, ex.end());
    ex.erase(std::unique(ex.begin() + ex_base, ex.end()), ex.end());
    qd[k] = {q.n, (int)NT, (int)(ex.size() - ex_base), (int)ex_base};
    NT += (size_t)q.n;
    max_n = std::max(max_n, q.n);
    if (NT > (size_t)INT_MAX / 64 || ex.size() > (size_t)INT_MAX / 64) { set_error("osh_orb_bow_db_query: batch too large"); return OSH_ERR_UNSUPPORTED; }
  }
  NE = ex.size();
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  if (db->device != device) { set_error("osh_orb_bow_db_query: the database lives on device %d, the context on device %d", db->device, device); return OSH_ERR_INVALID; }
  BowDbState* st = orb_state<BowDbState>(c, kOrbAttachBowDb);
  clock.profiling = orb_profiling(c);

  const size_t QR = (size_t)n_queries * n_rows;
  Layout in, out, work;
  const auto s_q = in.take<BowDbQueryDev>(n_queries);
  const auto s_word = in.take<uint32_t>(NT);
  const auto s_val = in.take<double>(NT);
  const auto s_ex = in.take<int>(NE);
  const auto o_head = out.take<BowDbHead>(n_queries);
  const auto w_common = work.take<int>(QR); const auto w_first = work.take<int>(QR);
  const auto w_entry = work.take<BowDbEntry>(QR);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  std::memcpy(s_q.in(h), qd.data(), sizeof(BowDbQueryDev) * n_queries);
  for (int k = 0; k < n_queries; ++k)
    if (queries[k].n) {
      std::memcpy(s_word.in(h) + qd[k].base, queries[k].word_id, (size_t)queries[k].n * sizeof(uint32_t));
      std::memcpy(s_val.in(h) + qd[k].base, queries[k].value, (size_t)queries[k].n * sizeof(double));
    }
  if (NE) std::memcpy(s_ex.in(h), ex.data(), NE * sizeof(int));
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_HIP(hipMemsetAsync(st->call.dev_out(), 0, st->call.out_bytes, s));
  OSH_TRY(clock.mark_synced(s));

  BowDbView v{};
  char* di = st->call.dev_in(); char* dw = st->call.dev_work();
  v.rows = db->d_rows; v.n_rows = (int)n_rows; v.ids = db->d_ids; v.vals = db->d_vals;
  v.q = s_q.in(di); v.q_word = s_word.in(di); v.q_val = s_val.in(di); v.ex = s_ex.in(di);
  v.common = w_common.in(dw); v.first = w_first.in(dw); v.entry = w_entry.in(dw);
  v.head = o_head.in(st->call.dev_out());
  if (n_rows > 0) {
    const size_t lds = std::max<size_t>((size_t)max_n * sizeof(uint32_t), 16);
    if (lds > 48 * 1024) OSH_TRY(allow_dynamic_lds(device, OSH_BOW_MAX_FEATURES * (int)sizeof(uint32_t), k_bowdb_count, k_bowdb_score));
    // persistent over the rows: about 2048 blocks in all, so a block's LDS copy of the query serves many rows of a large table
    const unsigned want = (unsigned)((n_rows + kBowDbWaves - 1) / kBowDbWaves);
    const dim3 grid(std::min(want, (unsigned)std::max(1, 2048 / n_queries)), (unsigned)n_queries);
    hipLaunchKernelGGL(k_bowdb_count, grid, dim3(kBowDbThreads), lds, s, v);
    hipLaunchKernelGGL(k_bowdb_emit, dim3((unsigned)n_queries), dim3(kBowDbThreads), 0, s, v);
    hipLaunchKernelGGL(k_bowdb_score, grid, dim3(kBowDbThreads), lds, s, v);
    OSH_TRY(launch_check("bow database query"));
  }
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));            // the headers; they say how much of each list travels

  const BowDbHead* head = o_head.in(st->call.host_out());
  size_t total = 0;
  for (int k = 0; k < n_queries; ++k) {
    if (head[k].n_listed < 0 || (size_t)head[k].n_listed > n_rows) { set_error("osh_orb_bow_db_query: query %d lists %d of %zu rows", k, head[k].n_listed, n_rows); return OSH_ERR_DEVICE; }
    total += (size_t)head[k].n_listed;
  }
  BowDbEntry* he = static_cast<BowDbEntry*>(st->h_entry.reserve(std::max<size_t>(total, 1) * sizeof(BowDbEntry)));
  if (!he) { set_error("osh_orb_bow_db_query: pinned allocation of %zu entries failed", total); return OSH_ERR_DEVICE; }
  size_t at = 0;
  for (int k = 0; k < n_queries; ++k) {
    const size_t n = (size_t)head[k].n_listed;
    if (n) OSH_HIP(hipMemcpyAsync(he + at, v.entry + (size_t)k * n_rows, n * sizeof(BowDbEntry), hipMemcpyDeviceToHost, s));
    at += n;
  }
  OSH_HIP(hipStreamSynchronize(s));

  int rc = OSH_OK;
  at = 0;
  for (int k = 0; k < n_queries; ++k) {
    const osh_bow_db_result& r = results[k];
    const int n = head[k].n_listed;
    if (r.max_common) *r.max_common = head[k].max_common;
    if (r.min_common) *r.min_common = head[k].min_common;
    if (r.n_rows) *r.n_rows = n;
    if (n > r.capacity) {
      if (rc == OSH_OK) set_error("osh_orb_bow_db_query: query %d lists %d rows, its result arrays hold %d", k, n, r.capacity);
      rc = OSH_ERR_INVALID;
    } else {
      for (int j = 0; j < n; ++j) {
        const BowDbEntry& e = he[at + j];
        if (r.handle) r.handle[j] = book.handle[e.row];
        if (r.common) r.common[j] = e.common;
        if (r.first_word) r.first_word[j] = e.first_word;
        if (r.scored) r.scored[j] = (uint8_t)e.scored;
        if (r.score) r.score[j] = e.score;
      }
    }
    at += (size_t)n;
  }
  clock.mark();
  clock.store(st->ms);
  return rc;
}

extern "C" int osh_orb_bow_db_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<BowDbState>("osh_orb_bow_db_get_times", c, kOrbAttachBowDb, ms);
}
