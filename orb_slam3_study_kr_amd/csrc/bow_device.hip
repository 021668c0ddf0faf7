// bow_device.hip -- TemplatedVocabulary::transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1259) on MI355X (gfx950) for a
// batch of frames: what Frame::ComputeBoW and KeyFrame::ComputeBoW run.
//
// The vocabulary (osh_bow_vocab) is resident once per device and immutable: the tree laid out again so that the children of a node are
// consecutive positions in the order the loader appended them, 32 bytes of descriptor and one int4 record per position.  Every
// context of the device reads it; a call writes only into its own context's arena.
//
// Two kernels per call, every frame of the batch in each:
//   k_bow_descend<G>  one group of G lanes per feature (G = 16 holds the k <= 16 of ORBvoc's k = 10, four features per wavefront;
//                     G = 32 when some node has 17..20 children), lane j on child j: the Hamming distance (orb_hamming.h), then the
//                     minimum of the key (distance << 8) | j over the group, which is the first smallest child: the reference's test
//                     is a strict `<` (:1244).  The steps of a feature depend on each other, so the kernel is latency bound; the grid
//                     is one wavefront per block over the features of all frames.
//   k_bow_sort        one block per (frame, vector): the 64-bit keys (word << 32) | feature and (node << 32) | feature of the features
//                     that are not stopped, sorted ascending by a bitonic network in LDS.  That is the iteration order of the two
//                     std::maps, with the features of a node ascending.
// The write-back walks the two sorted lists on the host: the FP64 sums of a word's weight (once per feature, in feature order,
// BowVector.cpp:34-46), the division by the number of words or by the sequential L1 norm in ascending word order (:62-84).
#include "common.h"
#include "orb_hamming.h"
#include "orb_stage.h"
#include <climits>
#include <vector>

namespace osh {

using u64 = unsigned long long;
constexpr u64 kBowNoKey = ~0ull;          // a stopped feature: sorts behind every kept one
constexpr int kBowSortThreads = 512;
constexpr int kBowStopped = 1 << 8;       // NodeDev::y: the word's weight is not > 0

// One position of the re-laid-out tree (position 0 is the root; the children of a position are consecutive positions)
//   x first child position, y child count | kBowStopped, z node id in file order, w word id (-1: not a leaf)
using NodeDev = int4;

struct BowFrameDev { int n, base; };      // base: offset of the frame in the feature arrays of the batch

struct BowView {
  const BowFrameDev* frames;
  const uint4* desc;                      // two per feature
  const NodeDev* node;
  const uint4* node_desc;                 // two per position
  int nid_level;                          // L - levelsup
  int* feat_word; int* feat_node; int* feat_dist;
  u64* wkey; u64* nkey;                   // [NT] work: unsorted keys
  u64* sorted_wkey; u64* sorted_nkey;     // [NT] out
  int* kept;                              // [n_frames * 2] out: kept entries of the two sorted lists
};

// grid = (ceil(max n / (64 / G)), n_frames), block = one wavefront.  The loop is wavefront-uniform: a group that has reached its leaf
// (or holds no feature) goes on taking part in the cross-lane minimum until every group of the wavefront is done.
template <int G>
__global__ __launch_bounds__(64) void k_bow_descend(BowView v) {
  constexpr int kPerWave = 64 / G;
  const BowFrameDev f = v.frames[blockIdx.y];
  if ((int)blockIdx.x * kPerWave >= f.n) return;   // block-uniform
  const int j = threadIdx.x & (G - 1);
  const int i = blockIdx.x * kPerWave + threadIdx.x / G;
  const bool valid = i < f.n;
  const size_t g = (size_t)f.base + (valid ? i : 0);
  const uint4 a0 = v.desc[g * 2], a1 = v.desc[g * 2 + 1];
  NodeDev nd = v.node[0];
  int depth = 0, dist = 0, recorded = 0;
  bool is_recorded = v.nid_level <= 0;             // the root (:1227)
  for (;;) {
    const int count = nd.y & 0xFF;
    const bool go = valid && count > 0;
    if (__ballot(go) == 0) break;
    unsigned key = 0xFFFFFFFFu;
    if (go && j < count) {
      const uint4* c = v.node_desc + (size_t)(nd.x + j) * 2;
      key = (hamming256(a0, a1, c[0], c[1]) << 8) | (unsigned)j;
    }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o, G));
    if (go) {
      nd = v.node[nd.x + (int)(key & 0xFF)];       // the same address in every lane of the group
      dist = (int)(key >> 8);
      if (++depth == v.nid_level) { recorded = nd.z; is_recorded = true; }   // :1251-1252
    }
  }
  if (!valid || j != 0) return;
  if (!is_recorded) recorded = nd.z;               // a leaf above depth L - levelsup: itself (the reference leaves nid unset)
  v.feat_word[g] = nd.w; v.feat_node[g] = recorded; v.feat_dist[g] = dist;
  const bool stopped = (nd.y & kBowStopped) != 0;  // :1157
  v.wkey[g] = stopped ? kBowNoKey : ((u64)(unsigned)nd.w << 32) | (unsigned)i;
  v.nkey[g] = stopped ? kBowNoKey : ((u64)(unsigned)recorded << 32) | (unsigned)i;
}

// grid = (n_frames, 2), block = 512, dynamic LDS = 8 bytes * (the power of two that holds the longest frame)
__global__ __launch_bounds__(kBowSortThreads) void k_bow_sort(BowView v) {
  extern __shared__ __attribute__((aligned(16))) u64 sh_key[];
  const BowFrameDev f = v.frames[blockIdx.x];
  const u64* src = (blockIdx.y ? v.nkey : v.wkey) + f.base;
  u64* dst = (blockIdx.y ? v.sorted_nkey : v.sorted_wkey) + f.base;
  const int tid = threadIdx.x;
  int P = 1;
  while (P < f.n) P <<= 1;
  for (int i = tid; i < P; i += kBowSortThreads) sh_key[i] = i < f.n ? src[i] : kBowNoKey;
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1)
    for (int s = k >> 1; s > 0; s >>= 1) {
      for (int i = tid; i < P; i += kBowSortThreads) {
        const int o = i ^ s;
        if (o > i) {
          const u64 a = sh_key[i], b = sh_key[o];
          if ((a > b) == ((i & k) == 0)) { sh_key[i] = b; sh_key[o] = a; }
        }
      }
      __syncthreads();
    }
  int* kept = v.kept + blockIdx.x * 2 + blockIdx.y;
  if (tid == 0 && sh_key[0] == kBowNoKey) *kept = 0;
  for (int i = tid; i < f.n; i += kBowSortThreads) {
    const u64 key = sh_key[i];
    dst[i] = key;
    if (key != kBowNoKey && (i + 1 == P || sh_key[i + 1] == kBowNoKey)) *kept = i + 1;
  }
}

struct BowState {
  StagedCall call;
  double ms[4] = {0, 0, 0, 0};
};

// What osh_bow_tree_check refuses; child_count [n + 1] by node id if wanted
static int bow_tree_check(const osh_bow_tree* t, std::vector<int>* child_count) {
  if (!t) { set_error("osh_bow_tree: NULL"); return OSH_ERR_INVALID; }
  if (t->k < 0 || t->k > OSH_BOW_MAX_K || t->L < 1 || t->L > OSH_BOW_MAX_L) { set_error("osh_bow_tree: k %d or L %d outside the loader's limits", t->k, t->L); return OSH_ERR_INVALID; }
  if (t->weighting < OSH_BOW_TF_IDF || t->weighting > OSH_BOW_BINARY || t->scoring < OSH_BOW_L1_NORM || t->scoring > OSH_BOW_DOT_PRODUCT) {
    set_error("osh_bow_tree: weighting %d or scoring %d is not a DBoW2 type", t->weighting, t->scoring);
    return OSH_ERR_INVALID;
  }
  if (t->n < 1 || t->n > INT_MAX / 64 || !t->parent || !t->is_leaf || !t->desc || !t->weight) { set_error("osh_bow_tree: empty tree, too many nodes or a NULL array"); return OSH_ERR_INVALID; }
  std::vector<int> count((size_t)t->n + 1, 0);
  for (int i = 0; i < t->n; ++i) {
    const int p = t->parent[i];
    if (p < 0 || p > i) { set_error("osh_bow_tree: node %d has parent %d, which is not an earlier node", i + 1, p); return OSH_ERR_INVALID; }
    if (++count[p] > OSH_BOW_MAX_K) { set_error("osh_bow_tree: node %d has more than %d children", p, OSH_BOW_MAX_K); return OSH_ERR_INVALID; }
  }
  for (int i = 0; i < t->n; ++i)
    if ((t->is_leaf[i] != 0) != (count[i + 1] == 0)) {
      set_error("osh_bow_tree: node %d is flagged %s and has %d children", i + 1, t->is_leaf[i] ? "leaf" : "inner", count[i + 1]);
      return OSH_ERR_INVALID;
    }
  if (child_count) child_count->swap(count);
  return OSH_OK;
}

}  // namespace osh

using namespace osh;

struct osh_bow_vocab {
  int device = 0;
  int L = 0, weighting = 0, scoring = 0;
  int group = 16;                     // lanes per feature in k_bow_descend
  DevBuf d_node, d_desc;
  std::vector<double> word_weight;    // by word id, for the sums of the write-back
};

extern "C" int osh_bow_tree_check(const osh_bow_tree* tree) { return bow_tree_check(tree, nullptr); }

extern "C" int osh_bow_vocab_create(int device, const osh_bow_tree* t, osh_bow_vocab** out) {
  if (!out) { set_error("osh_bow_vocab_create: out is NULL"); return OSH_ERR_INVALID; }
  *out = nullptr;
  std::vector<int> count;
  OSH_TRY(bow_tree_check(t, &count));
  if (t->scoring == OSH_BOW_L2_NORM) { set_error("osh_bow_vocab_create: L2_NORM scoring is not supported (the rounding of its square root is not pinned)"); return OSH_ERR_UNSUPPORTED; }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_error("no HIP device visible"); return OSH_ERR_NO_DEVICE; }
  if (device < 0 || device >= n_dev) { set_error("device %d out of range (have %d)", device, n_dev); return OSH_ERR_INVALID; }

  // positions: the children of node 0, 1, 2, .. (file order) one block after another, each block in the order the loader appended them
  const size_t n = (size_t)t->n;
  std::vector<int> first(n + 1, 0), pos(n + 1, 0), filled(n + 1, 0);
  int next = 1, max_children = 0;
  for (size_t id = 0; id <= n; ++id) { first[id] = next; next += count[id]; max_children = std::max(max_children, count[id]); }
  std::vector<NodeDev> node(n + 1);
  std::vector<uint8_t> desc((n + 1) * 32, 0);
  std::vector<double> word_weight;
  node[0] = make_int4(first[0], count[0], 0, -1);
  for (size_t i = 0; i < n; ++i) {
    const int id = (int)i + 1, p = t->parent[i];
    pos[id] = first[p] + filled[p]++;
    int word = -1, flags = 0;
    if (t->is_leaf[i]) {
      word = (int)word_weight.size();
      word_weight.push_back(t->weight[i]);
      if (!(t->weight[i] > 0)) flags = kBowStopped;
    }
    node[pos[id]] = make_int4(first[id], count[id] | flags, id, word);
    std::memcpy(&desc[(size_t)pos[id] * 32], t->desc + i * 32, 32);
  }

  OSH_HIP(hipSetDevice(device));
  osh_bow_vocab* v = new osh_bow_vocab();
  v->device = device; v->L = t->L; v->weighting = t->weighting; v->scoring = t->scoring;
  v->group = max_children <= 16 ? 16 : 32;
  v->word_weight.swap(word_weight);
  int rc = v->d_node.reserve(node.size() * sizeof(NodeDev));
  if (rc == OSH_OK) rc = v->d_desc.reserve(desc.size());
  if (rc == OSH_OK && hipMemcpy(v->d_node.p, node.data(), node.size() * sizeof(NodeDev), hipMemcpyHostToDevice) != hipSuccess) rc = OSH_ERR_DEVICE;
  if (rc == OSH_OK && hipMemcpy(v->d_desc.p, desc.data(), desc.size(), hipMemcpyHostToDevice) != hipSuccess) rc = OSH_ERR_DEVICE;
  if (rc != OSH_OK) {
    if (rc == OSH_ERR_DEVICE && !*get_error()) set_error("osh_bow_vocab_create: upload failed");
    delete v;
    return rc;
  }
  *out = v;
  return OSH_OK;
}

extern "C" void osh_bow_vocab_destroy(osh_bow_vocab* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  (void)hipDeviceSynchronize();   // no transform of any context may still read it
  delete v;
}

namespace osh {

// The BowVector and the FeatureVector of one frame from its two sorted key lists
static void bow_write_back(const osh_bow_vocab& V, int n, const u64* wkey, int kept_w, const u64* nkey, int kept_n, const osh_bow_result& r,
                           std::vector<double>& value) {
#pragma clang fp contract(off)
  const bool sums = V.weighting == OSH_BOW_TF_IDF || V.weighting == OSH_BOW_TF;
  int n_words = 0;
  value.clear();
  for (int t = 0; t < kept_w; ++t) {
    const int word = (int)(wkey[t] >> 32);
    const double w = V.word_weight[word];
    if (t > 0 && (int)(wkey[t - 1] >> 32) == word) {
      if (sums) value.back() += w;                 // addWeight: once per feature, in feature order; addIfNotExist: nothing
    } else {
      if (r.word_id) r.word_id[n_words] = word;
      value.push_back(w);
      ++n_words;
    }
  }
  const bool must = V.scoring != OSH_BOW_DOT_PRODUCT;   // ScoringObject.h:74-89; L2_NORM is refused at creation
  if (sums && n_words > 0 && !must) {
    const double nd = (double)n_words;             // :1164-1170
    for (double& x : value) x /= nd;
  }
  if (must) {                                      // BowVector::normalize(L1)
    double norm = 0.0;
    for (const double x : value) norm += std::fabs(x);
    if (norm > 0.0) for (double& x : value) x /= norm;
  }
  if (r.n_words) *r.n_words = n_words;
  if (r.word_value && n_words) std::memcpy(r.word_value, value.data(), sizeof(double) * (size_t)n_words);

  int n_nodes = 0;
  for (int t = 0; t < kept_n; ++t) {
    const int node = (int)(nkey[t] >> 32);
    if (t == 0 || (int)(nkey[t - 1] >> 32) != node) {
      if (r.node_id) r.node_id[n_nodes] = node;
      if (r.node_start) r.node_start[n_nodes] = t;
      ++n_nodes;
    }
    if (r.node_feat) r.node_feat[t] = (int)(nkey[t] & 0xFFFFFFFFu);
  }
  if (r.node_start) r.node_start[n_nodes] = kept_n;
  if (r.n_nodes) *r.n_nodes = n_nodes;
  (void)n;
}

}  // namespace osh

extern "C" int osh_orb_bow_transform(osh_orb_ctx* c, const osh_bow_vocab* vocab, int32_t levelsup, int32_t n_frames, const osh_bow_frame* frames,
                                     const osh_bow_result* results) {
  if (!c || !vocab || n_frames < 0 || (n_frames && (!frames || !results))) { set_error("osh_orb_bow_transform: bad arguments"); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  PhaseClock clock;
  size_t NT = 0;
  int max_n = 0;
  std::vector<BowFrameDev> fd(n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_bow_frame& f = frames[k];
    if (f.n < 0 || (f.n && !f.desc)) { set_error("frame %d: negative feature count or NULL descriptors", k); return OSH_ERR_INVALID; }
    if (f.n > OSH_BOW_MAX_FEATURES) { set_error("frame %d: %d features exceed %d", k, f.n, OSH_BOW_MAX_FEATURES); return OSH_ERR_UNSUPPORTED; }
    fd[k] = {f.n, (int)NT};
    NT += (size_t)f.n;
    max_n = std::max(max_n, f.n);
    if (NT > (size_t)INT_MAX / 64) { set_error("osh_orb_bow_transform: batch too large"); return OSH_ERR_UNSUPPORTED; }
  }
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  if (vocab->device != device) { set_error("osh_orb_bow_transform: the vocabulary lives on device %d, the context on device %d", vocab->device, device); return OSH_ERR_INVALID; }
  BowState* st = orb_state<BowState>(c, kOrbAttachBow);
  clock.profiling = orb_profiling(c);

  // the three stage arrays travel back only if some frame asks for one of them; otherwise the kernel writes them into the work area
  bool stages = false;
  for (int k = 0; k < n_frames; ++k) stages |= results[k].feat_word || results[k].feat_node || results[k].feat_dist;
  Layout in, out, work;
  Layout& stage_area = stages ? out : work;
  const auto s_frames = in.take<BowFrameDev>(n_frames);
  const auto s_desc = in.take<uint4>(NT * 2);
  const auto o_word = stage_area.take<int>(NT); const auto o_node = stage_area.take<int>(NT); const auto o_dist = stage_area.take<int>(NT);
  const auto o_wkey = out.take<u64>(NT); const auto o_nkey = out.take<u64>(NT);
  const auto o_kept = out.take<int>((size_t)n_frames * 2);
  const auto w_wkey = work.take<u64>(NT); const auto w_nkey = work.take<u64>(NT);
  OSH_TRY(st->call.reserve(in, out, work.bytes));

  char* h = st->call.host_in();
  std::memcpy(s_frames.in(h), fd.data(), sizeof(BowFrameDev) * n_frames);
  for (int k = 0; k < n_frames; ++k)
    if (frames[k].n) std::memcpy(s_desc.in(h) + (size_t)fd[k].base * 2, frames[k].desc, (size_t)frames[k].n * 32);
  clock.mark();
  OSH_TRY(st->call.upload(s));
  OSH_TRY(clock.mark_synced(s));

  BowView v{};
  char* di = st->call.dev_in(); char* dout = st->call.dev_out(); char* dw = st->call.dev_work();
  v.frames = s_frames.in(di); v.desc = s_desc.in(di);
  v.node = vocab->d_node.as<NodeDev>(); v.node_desc = vocab->d_desc.as<uint4>();
  v.nid_level = vocab->L - levelsup;
  char* dstage = stages ? dout : dw;
  v.feat_word = o_word.in(dstage); v.feat_node = o_node.in(dstage); v.feat_dist = o_dist.in(dstage);
  v.sorted_wkey = o_wkey.in(dout); v.sorted_nkey = o_nkey.in(dout); v.kept = o_kept.in(dout);
  v.wkey = w_wkey.in(dw); v.nkey = w_nkey.in(dw);
  if (max_n > 0) {
    const int per_wave = 64 / vocab->group;
    const dim3 grid((unsigned)((max_n + per_wave - 1) / per_wave), (unsigned)n_frames);
    if (vocab->group == 16) hipLaunchKernelGGL(k_bow_descend<16>, grid, dim3(64), 0, s, v);
    else hipLaunchKernelGGL(k_bow_descend<32>, grid, dim3(64), 0, s, v);
  }
  int P = 1;
  while (P < max_n) P <<= 1;
  const size_t lds = (size_t)P * sizeof(u64);
  if (lds > 48 * 1024) OSH_TRY(allow_dynamic_lds(device, OSH_BOW_MAX_FEATURES * (int)sizeof(u64), k_bow_sort));
  hipLaunchKernelGGL(k_bow_sort, dim3((unsigned)n_frames, 2), dim3(kBowSortThreads), lds, s, v);
  OSH_TRY(launch_check("bow transform"));
  OSH_TRY(clock.mark_synced(s));
  OSH_TRY(st->call.download(s));

  const char* ho = st->call.host_out();
  std::vector<double> value;
  for (int k = 0; k < n_frames; ++k) {
    const osh_bow_result& r = results[k];
    const size_t n = (size_t)frames[k].n, b = (size_t)fd[k].base;
    if (stages) { scatter(r.feat_word, o_word, ho, b, n); scatter(r.feat_node, o_node, ho, b, n); scatter(r.feat_dist, o_dist, ho, b, n); }
    const int* kept = o_kept.in(ho) + 2 * k;
    bow_write_back(*vocab, frames[k].n, o_wkey.in(ho) + b, kept[0], o_nkey.in(ho) + b, kept[1], r, value);
  }
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

extern "C" int osh_orb_bow_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<BowState>("osh_orb_bow_get_times", c, kOrbAttachBow, ms);
}
