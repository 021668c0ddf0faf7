// ransac_stage_check.cpp -- validate_minimal_sets and RansacBatch of csrc/ransac_stage.h and null_vector of csrc/jacobi_rows.h (with
// tv_null9 of csrc/two_view.h around it) on plain host memory, for a run under a sanitizer: every array is malloc'ed with exactly
// the size the call may read, so a read past the end is caught.  A program of its own (`make ransac-stage-check`), in no library;
// it makes no HIP call and needs no device.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../ransac_stage.h"
#include "../two_view.h"

namespace osh {
static char last_error[512];
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(last_error, sizeof last_error, fmt, ap);
  va_end(ap);
}
}  // namespace osh
using namespace osh;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("%s:%d: %s (%s)\n", __FILE__, __LINE__, #cond, last_error); ++failures; } } while (0)

// n_iterations sets of K indices in an allocation of exactly that size: set s is s, s + 1, .. (mod n), distinct for n >= K
struct Sets {
  int32_t* p;
  int K, n_it;
  Sets(int K_, int n_it_, int n) : K(K_), n_it(n_it_) {
    p = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * (size_t)K * n_it));   // malloc(0) for no iterations: nothing to read
    for (int s = 0; s < n_it; ++s) for (int a = 0; a < K; ++a) p[K * s + a] = (s + a) % n;
  }
  Sets(const Sets&) = delete;
  ~Sets() { std::free(p); }
  int32_t& last(int a) { return p[K * (n_it - 1) + a]; }
};

template <int K>
static int validate(const Sets& s, int n) { last_error[0] = 0; return validate_minimal_sets<K>("entry", 7, s.p, s.n_it, n); }
static bool said(const char* text) { return std::strstr(last_error, text) != nullptr; }

template <int K>
static void check_validator() {
  char want[96];
  // n equal to the set size, 0 and 1 iterations, then several
  for (int n_it : {0, 1, 5}) { Sets s(K, n_it, K); CHECK(validate<K>(s, K) == OSH_OK); }
  // no sets at all
  last_error[0] = 0;
  CHECK(validate_minimal_sets<K>("entry", 7, nullptr, 0, K) == OSH_OK);
  CHECK(validate_minimal_sets<K>("entry", 7, nullptr, 1, K) == OSH_ERR_INVALID && said("entry: problem 7: NULL sets with n_iterations = 1"));
  // one correspondence too few: the sets are not read
  {
    Sets s(K, 2, K);
    std::snprintf(want, sizeof want, "entry: problem 7: %d correspondences cannot fill a minimal set of %d", K - 1, K);
    CHECK(validate<K>(s, K - 1) == OSH_ERR_INVALID && said(want));
    CHECK(validate_minimal_sets<K>("entry", 7, s.p, 2, K - 1, "matches") == OSH_ERR_INVALID && said("matches cannot fill"));
    Sets none(K, 0, K);
    CHECK(validate<K>(none, K - 1) == OSH_OK);   // without iterations nothing has to be filled
  }
  // an index of -1 and of n, at the first and at the last position of the last set
  for (int n_it : {1, 3})
    for (int pos : {0, K - 1})
      for (int bad : {-1, K + 2}) {
        const int n = K + 2;
        Sets s(K, n_it, n);
        CHECK(validate<K>(s, n) == OSH_OK);
        s.last(pos) = bad;
        std::snprintf(want, sizeof want, "entry: problem 7: set %d: index %d outside [0, %d)", n_it - 1, bad, n);
        CHECK(validate<K>(s, n) == OSH_ERR_INVALID && said(want));
      }
  // a repeat between the first and the last position, and between the last two
  for (int n_it : {1, 3})
    for (int first : {0, K - 2}) {
      const int n = K + 2;
      Sets s(K, n_it, n);
      s.last(K - 1) = s.last(first);
      std::snprintf(want, sizeof want, "entry: problem 7: set %d repeats index %d", n_it - 1, s.last(first));
      CHECK(validate<K>(s, n) == OSH_ERR_INVALID && said(want));
    }
}

// Five problems: an empty one in the middle, one with iterations and no mask words
static void check_batch() {
  struct P { int n, n_iterations, words; const int32_t* sets; };
  Sets s0(3, 4, 70), s1(3, 1, 3), s3(3, 2, 130), s4(3, 300, 64);
  const P ps[5] = {{70, 4, ransac_mask_words(70), s0.p}, {3, 1, ransac_mask_words(3), s1.p}, {0, 0, ransac_mask_words(0), nullptr},
                   {130, 2, 0, s3.p}, {64, 300, ransac_mask_words(64), s4.p}};
  CHECK(ransac_mask_words(0) == 0 && ransac_mask_words(1) == 2 && ransac_mask_words(64) == 2 && ransac_mask_words(65) == 4 && ransac_mask_words(70) == 4);
  RansacBatch b;
  for (const P& p : ps) b.add(p.n, p.n_iterations, p.words);
  const size_t want_p[5] = {0, 70, 73, 73, 203}, want_h[5] = {0, 4, 5, 5, 7}, want_w[5] = {0, 16, 18, 18, 18};
  CHECK(b.base.size() == 5);
  for (int k = 0; k < 5; ++k) CHECK(b.base[k].p == want_p[k] && b.base[k].h == want_h[k] && b.base[k].w == want_w[k]);
  CHECK(b.N == 70 + 3 + 0 + 130 + 64 && b.I == 4 + 1 + 0 + 2 + 300 && b.W == 4 * 4 + 1 * 2 + 0 + 0 + 300 * 2 && b.max_iter == 300);
  // the sets of all problems into an allocation of exactly I * 3
  int32_t* staged = static_cast<int32_t*>(std::malloc(sizeof(int32_t) * b.I * 3));
  b.stage_sets<3>(staged, ps);
  for (int k = 0; k < 5; ++k)
    for (int e = 0; e < 3 * ps[k].n_iterations; ++e) CHECK(staged[3 * want_h[k] + e] == ps[k].sets[e]);
  std::free(staged);
  RansacBatch none;
  CHECK(none.N == 0 && none.I == 0 && none.W == 0 && none.max_iter == 0 && none.base.empty());
  none.stage_sets<8>(nullptr, ps);
}

// A 16 x COLS row array whose column `zero` is 0 and whose other columns are independent: the null vector is the unit vector e_zero
template <int COLS>
static void fill_rows(double (*a)[COLS], int zero) {
  for (int i = 0; i < kJacobiRows; ++i)
    for (int j = 0; j < COLS; ++j) a[i][j] = j == zero ? 0.0 : 1.0 / (1.0 + i + j) + (i == j ? 2.0 : 0.0) + 0.25 * ((i * 7 + j * 3) % 5);
}
template <int COLS, int SWEEPS>
static void check_unit(int cols, int zero) {
  auto a = static_cast<double (*)[COLS]>(std::malloc(sizeof(double) * kJacobiRows * COLS));
  double* h = static_cast<double*>(std::malloc(sizeof(double) * COLS));
  fill_rows<COLS>(a, zero);
  null_vector<COLS, SWEEPS>(a, cols, h);
  for (int k = 0; k < COLS; ++k) CHECK(h[k] == (k == zero ? 1.0 : 0.0));   // a zero column is never rotated: gamma == 0
  std::free(h);
  std::free(a);
}

static void check_null_vector() {
  check_unit<9, 10>(9, 0); check_unit<9, 10>(9, 4); check_unit<9, 10>(9, 8);
  check_unit<12, 12>(12, 0); check_unit<12, 12>(12, 11);
  // rank deficient with cols = 9 of 12: rows 9..15 and columns 9..11 zero (the planar case), the zero column among the first 9
  {
    auto a = static_cast<double (*)[12]>(std::malloc(sizeof(double) * kJacobiRows * 12));
    double* h = static_cast<double*>(std::malloc(sizeof(double) * 12));
    fill_rows<12>(a, 5);
    for (int i = 0; i < kJacobiRows; ++i) for (int j = 0; j < 12; ++j) if (i >= 9 || j >= 9) a[i][j] = 0.0;
    null_vector<12, 12>(a, 9, h);
    for (int k = 0; k < 12; ++k) CHECK(h[k] == (k == 5 ? 1.0 : 0.0));   // column 5, not the zero columns 9..11 beyond cols
    std::free(h);
    std::free(a);
  }
  // tv_null9 is the float conversion of null_vector<9, 10> of the widened entries, on a general (full rank) system too
  for (int zero : {3, -1}) {
    auto A = static_cast<float (*)[9]>(std::malloc(sizeof(float) * kTvRows * 9));
    auto a = static_cast<double (*)[9]>(std::malloc(sizeof(double) * kTvRows * 9));
    float* hf = static_cast<float*>(std::malloc(sizeof(float) * 9));
    double* hd = static_cast<double*>(std::malloc(sizeof(double) * 9));
    fill_rows<9>(a, zero);
    for (int i = 0; i < kTvRows; ++i) for (int j = 0; j < 9; ++j) { A[i][j] = (float)a[i][j]; a[i][j] = (double)A[i][j]; }
    tv_null9(A, hf);
    null_vector<9, 10>(a, 9, hd);
    double norm = 0;
    for (int k = 0; k < 9; ++k) {
      const float want = (float)hd[k];
      CHECK(std::memcmp(&hf[k], &want, 4) == 0);
      norm += hd[k] * hd[k];
    }
    CHECK(norm > 1.0 - 1e-12 && norm < 1.0 + 1e-12);
    if (zero >= 0) CHECK(hf[zero] == 1.f);
    std::free(hd); std::free(hf); std::free(a); std::free(A);
  }
}

int main() {
  check_validator<3>(); check_validator<6>(); check_validator<8>();
  check_batch();
  check_null_vector();
  if (failures) { std::printf("ransac_stage_check: %d failures\n", failures); return 1; }
  std::printf("ransac_stage_check ok\n");
  return 0;
}
