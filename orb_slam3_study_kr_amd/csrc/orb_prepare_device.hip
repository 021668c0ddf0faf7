// orb_prepare_device.hip -- the image front end on MI355X (gfx950) for a batch of raw camera images: the cv::remap of
// System::TrackStereo (src/System.cc:252-269) or the cv::resize of TrackStereo / TrackRGBD / TrackMonocular, then the cvtColor of
// Tracking::GrabImage* (src/Tracking.cc:1462-1489), giving the grey level-0 image ORBextractor::operator() reads.  The statements are
// those of orb_prepare.h; the tap tables of a resize are input data computed on the host, and apart from the one mx * 32.f of a
// remap and its conversion the kernel is integer only.
//
// osh_rectify_map: the two float maps of a camera, resident once on their device and immutable (rows padded to 16 bytes, so that a
//   thread's four coordinates are one aligned 16-byte load).
// osh_orb_prepare: the raw images are packed into pinned memory and uploaded in one copy, with the jobs and the tables;
//   k_prepare      ONE launch for all frames (grid y: the frame): a thread produces four horizontally adjacent grey pixels of one row
//                  and stores them as one dword when the four exist and their address is a multiple of 4, else byte by byte.  The
//                  source is gathered through the cache: neighbouring lanes read neighbouring lines, nothing is staged in LDS.  Every
//                  tap of a remap is bounds-checked (outside the source it is 0); a resize reads through tables clamped to the source.
//   The prepared images lie one after another, rows packed at `cols` bytes; a frame that asks for its image gets it from one D2H copy.
// osh_orb_extract_raw: osh_orb_extract (extract_from of orb_extract.h) with k_prepare as the producer of level 0: it writes straight
//   into the level-0 slots of the context's resident pyramid on the stream before k_pyr_level; only the raw image goes up.
#include "common.h"
#include "orb_extract.h"
#include "orb_prepare.h"
#include "orb_pyramid_set.h"
#include "orb_stage.h"
#include <map>
#include <tuple>
#include <vector>

namespace osh {

constexpr int kPrepBlockX = 64, kPrepBlockY = 4;   // k_prepare: 64 groups of four pixels by 4 rows

struct PrepJobDev {
  long long src_off;            // first byte of the packed raw image in `raw`
  long long dst_off;            // first pixel of the prepared image in `dst`
  const float* map_x;           // the resident maps, rows map_pitch floats apart (a multiple of 4); nullptr without a map
  const float* map_y;
  int map_pitch;
  int src_rows, src_cols, channels, bgr;
  int dst_rows, dst_cols;
  int mode;                     // kPrepPass, kPrepRemap, kPrepResize, kPrepHalve
  int col_tap, row_tap;         // kPrepResize: first entry of the frame's tables in `taps`
};
struct PrepView {
  const PrepJobDev* jobs;
  const PyrTap* taps;
  const unsigned char* raw;
  unsigned char* dst;
};

__global__ __launch_bounds__(kPrepBlockX * kPrepBlockY) void k_prepare(PrepView v) {
  const PrepJobDev& J = v.jobs[blockIdx.y];
  const int groups = (J.dst_cols + 3) / 4;
  const int tiles_x = (groups + kPrepBlockX - 1) / kPrepBlockX;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y = ty * kPrepBlockY + threadIdx.y, g = tx * kPrepBlockX + threadIdx.x;
  if (y >= J.dst_rows || g >= groups) return;
  const int x0 = 4 * g;
  const int n = fast_min(4, J.dst_cols - x0);   // pixels of the group inside the row: 1 to 4
  const PrepSource S{v.raw + J.src_off, (long long)J.src_cols * J.channels, J.src_rows, J.src_cols, J.channels, J.bgr};
  unsigned px[4] = {0, 0, 0, 0};
  if (J.mode == kPrepRemap) {
    // map_pitch is a multiple of 4 floats and the padding exists (and is 0): the whole 16 bytes are inside the map's buffer
    const float4 ax = *reinterpret_cast<const float4*>(J.map_x + (size_t)y * J.map_pitch + x0);
    const float4 ay = *reinterpret_cast<const float4*>(J.map_y + (size_t)y * J.map_pitch + x0);
    const float mx[4] = {ax.x, ax.y, ax.z, ax.w}, my[4] = {ay.x, ay.y, ay.z, ay.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) px[i] = prep_remap_pixel(S, mx[i], my[i]);
  } else if (J.mode == kPrepResize) {
    const PyrTap ry = v.taps[J.row_tap + y];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) px[i] = prep_resize_pixel(S, ry, v.taps[J.col_tap + x0 + i]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) px[i] = J.mode == kPrepHalve ? prep_halve_pixel(S, y, x0 + i) : prep_pass_pixel(S, y, x0 + i);
  }
  const long long at = J.dst_off + (long long)y * J.dst_cols + x0;   // the buffer itself is 256-byte aligned
  unsigned char* dst = v.dst + at;
  if (n == 4 && (at & 3) == 0) {
    *reinterpret_cast<unsigned*>(dst) = px[0] | (px[1] << 8) | (px[2] << 16) | (px[3] << 24);
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < n) dst[i] = (unsigned char)px[i];
  }
}

struct PrepState {
  StagedCall call;      // [jobs | taps] in
  DevBuf raw, gray;     // the packed raw images of the call; osh_orb_prepare: the prepared images
  PinBuf h_raw, h_gray;
  double ms[4] = {0, 0, 0, 0};
};

// What a call does once its frames passed: the sizes, the jobs (dst_off not yet set) and the tables
struct PrepPlan {
  std::vector<PrepJobDev> jobs;
  std::vector<PyrTap> taps;
  std::vector<size_t> raw_row;   // bytes of a packed raw row of frame k
  size_t raw_bytes = 0, out_bytes = 0;
  unsigned max_tiles = 1;
};

}  // namespace osh

using namespace osh;

struct osh_rectify_map {
  int device = 0;
  int rows = 0, cols = 0, src_rows = 0, src_cols = 0;
  int pitch = 0;         // floats per row on the device: cols rounded up to 4
  DevBuf d_x, d_y;
};

extern "C" int osh_rectify_map_create(int device, const osh_rectify_map_desc* d, osh_rectify_map** out) {
  const char* entry = "osh_rectify_map_create";
  if (!out) { set_error("%s: out is NULL", entry); return OSH_ERR_INVALID; }
  *out = nullptr;
  if (!d || !d->map_x || !d->map_y) { set_error("%s: NULL descriptor or map", entry); return OSH_ERR_INVALID; }
  if (d->rows <= 0 || d->cols <= 0 || d->src_rows <= 0 || d->src_cols <= 0) { set_error("%s: a size is not positive (map %d x %d, source %d x %d)", entry, d->rows, d->cols, d->src_rows, d->src_cols); return OSH_ERR_INVALID; }
  if (d->map_x_stride < 4 * (int64_t)d->cols || d->map_y_stride < 4 * (int64_t)d->cols) { set_error("%s: a map stride is under 4 * cols bytes", entry); return OSH_ERR_INVALID; }
  if (d->rows > OSH_FAST_MAX_SIDE || d->cols > OSH_FAST_MAX_SIDE || d->src_rows > OSH_FAST_MAX_SIDE || d->src_cols > OSH_FAST_MAX_SIDE) {
    set_error("%s: a size exceeds %d pixels in one direction", entry, OSH_FAST_MAX_SIDE); return OSH_ERR_UNSUPPORTED;
  }
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { set_error("no HIP device visible"); return OSH_ERR_NO_DEVICE; }
  if (device < 0 || device >= n_dev) { set_error("device %d out of range (have %d)", device, n_dev); return OSH_ERR_INVALID; }

  const int pitch = (d->cols + 3) & ~3;
  std::vector<float> hx((size_t)d->rows * pitch, 0.f), hy((size_t)d->rows * pitch, 0.f);
  for (int y = 0; y < d->rows; ++y) {
    std::memcpy(&hx[(size_t)y * pitch], reinterpret_cast<const char*>(d->map_x) + (int64_t)y * d->map_x_stride, sizeof(float) * (size_t)d->cols);
    std::memcpy(&hy[(size_t)y * pitch], reinterpret_cast<const char*>(d->map_y) + (int64_t)y * d->map_y_stride, sizeof(float) * (size_t)d->cols);
  }
  OSH_HIP(hipSetDevice(device));
  osh_rectify_map* m = new osh_rectify_map();
  m->device = device; m->rows = d->rows; m->cols = d->cols; m->src_rows = d->src_rows; m->src_cols = d->src_cols; m->pitch = pitch;
  const size_t bytes = hx.size() * sizeof(float);
  int rc = m->d_x.reserve(bytes);
  if (rc == OSH_OK) rc = m->d_y.reserve(bytes);
  if (rc == OSH_OK && hipMemcpy(m->d_x.p, hx.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) rc = OSH_ERR_DEVICE;
  if (rc == OSH_OK && hipMemcpy(m->d_y.p, hy.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) rc = OSH_ERR_DEVICE;
  if (rc != OSH_OK) {
    if (rc == OSH_ERR_DEVICE && !*get_error()) set_error("%s: upload failed", entry);
    delete m;
    return rc;
  }
  *out = m;
  return OSH_OK;
}

extern "C" void osh_rectify_map_destroy(osh_rectify_map* m) {
  if (!m) return;
  (void)hipSetDevice(m->device);
  (void)hipDeviceSynchronize();   // no call of any context may still read it
  delete m;
}

namespace osh {

// Frame k and where its image goes; no context and no device.  rows / cols: the prepared size
static int prepare_validate(const char* entry, int k, const osh_prepare_frame& f, const osh_prepare_result* r, int& rows, int& cols) {
  const osh_prepare_image& im = f.image;
  if (!im.data || im.rows <= 0 || im.cols <= 0) { set_error("%s: frame %d: the image is NULL or empty", entry, k); return OSH_ERR_INVALID; }
  if (im.channels != 1 && im.channels != 3 && im.channels != 4) { set_error("%s: frame %d: %d channels, not 1, 3 or 4", entry, k, im.channels); return OSH_ERR_INVALID; }
  if (im.stride < (int64_t)im.cols * im.channels) { set_error("%s: frame %d: stride < cols * channels", entry, k); return OSH_ERR_INVALID; }
  if (f.order != OSH_PREP_RGB && f.order != OSH_PREP_BGR) { set_error("%s: frame %d: unknown channel order %d", entry, k, f.order); return OSH_ERR_INVALID; }
  if (f.map && (f.map->src_rows != im.rows || f.map->src_cols != im.cols)) {
    set_error("%s: frame %d: the map was made for a %d x %d source, the image is %d x %d", entry, k, f.map->src_rows, f.map->src_cols, im.rows, im.cols); return OSH_ERR_INVALID;
  }
  rows = f.out_rows; cols = f.out_cols;
  if (rows == 0 && cols == 0) { rows = f.map ? f.map->rows : im.rows; cols = f.map ? f.map->cols : im.cols; }
  if (rows <= 0 || cols <= 0) { set_error("%s: frame %d: the output size %d x %d is not positive", entry, k, f.out_rows, f.out_cols); return OSH_ERR_INVALID; }
  if (f.map && (rows != f.map->rows || cols != f.map->cols)) { set_error("%s: frame %d: the output size %d x %d is not the map's %d x %d", entry, k, rows, cols, f.map->rows, f.map->cols); return OSH_ERR_INVALID; }
  if (r && r->gray && r->gray_stride < (int64_t)cols) { set_error("%s: frame %d: gray stride < cols", entry, k); return OSH_ERR_INVALID; }
  if (im.rows > OSH_FAST_MAX_SIDE || im.cols > OSH_FAST_MAX_SIDE || rows > OSH_FAST_MAX_SIDE || cols > OSH_FAST_MAX_SIDE) {
    set_error("%s: frame %d: the input or the output exceeds %d pixels in one direction", entry, k, OSH_FAST_MAX_SIDE); return OSH_ERR_UNSUPPORTED;
  }
  return OSH_OK;
}

static int prepare_plan(const char* entry, int n_frames, const osh_prepare_frame* frames, const osh_prepare_result* results, PrepPlan& P) {
  P.jobs.resize((size_t)n_frames); P.raw_row.resize((size_t)n_frames);
  std::map<std::tuple<int, int, bool>, int> table_at;   // the tables once per geometry, as osh_orb_pyramid_build keeps them
  auto table = [&](int src, int dst, bool rows) {
    const auto key = std::make_tuple(src, dst, rows);
    const auto it = table_at.find(key);
    if (it != table_at.end()) return it->second;
    const int at = (int)P.taps.size();
    P.taps.resize(P.taps.size() + (size_t)dst);
    pyr_axis_table(src, dst, rows, P.taps.data() + at);
    table_at.emplace(key, at);
    return at;
  };
  for (int k = 0; k < n_frames; ++k) {
    const osh_prepare_frame& f = frames[k];
    int rows = 0, cols = 0;
    OSH_TRY(prepare_validate(entry, k, f, results ? &results[k] : nullptr, rows, cols));
    PrepJobDev& J = P.jobs[k];
    J = PrepJobDev{};
    J.src_off = (long long)P.raw_bytes;
    J.src_rows = f.image.rows; J.src_cols = f.image.cols; J.channels = f.image.channels; J.bgr = f.order == OSH_PREP_BGR ? kPrepBGR : kPrepRGB;
    J.dst_rows = rows; J.dst_cols = cols;
    if (f.map) {
      J.mode = kPrepRemap; J.map_x = f.map->d_x.as<const float>(); J.map_y = f.map->d_y.as<const float>(); J.map_pitch = f.map->pitch;
    } else {
      J.mode = prep_mode(J.src_rows, J.src_cols, rows, cols);
      if (J.mode == kPrepResize) { J.col_tap = table(J.src_cols, cols, false); J.row_tap = table(J.src_rows, rows, true); }
    }
    P.raw_row[k] = (size_t)J.src_cols * J.channels;
    P.raw_bytes += (P.raw_row[k] * J.src_rows + 255) & ~(size_t)255;
    P.out_bytes += (size_t)rows * cols;
    const unsigned tiles = (unsigned)((((cols + 3) / 4 + kPrepBlockX - 1) / kPrepBlockX) * ((rows + kPrepBlockY - 1) / kPrepBlockY));
    P.max_tiles = std::max(P.max_tiles, tiles);
    if (P.raw_bytes > (size_t)1 << 31 || P.out_bytes > (size_t)1 << 31) { set_error("%s: batch too large", entry); return OSH_ERR_UNSUPPORTED; }
  }
  return OSH_OK;
}

static int prepare_check_device(const char* entry, int n_frames, const osh_prepare_frame* frames, int device) {
  for (int k = 0; k < n_frames; ++k)
    if (frames[k].map && frames[k].map->device != device) {
      set_error("%s: frame %d: the rectify map lives on device %d, the context on device %d", entry, k, frames[k].map->device, device); return OSH_ERR_INVALID;
    }
  return OSH_OK;
}

// The raw images, the jobs and the tables go up and k_prepare runs on s: frame k to dst + dst_off[k].  clock (may be null): a mark
// when the staging is done and one when the upload is
static int prepare_produce(const char* entry, PrepState* st, hipStream_t s, int n_frames, const osh_prepare_frame* frames, PrepPlan& P, unsigned char* dst,
                           const long long* dst_off, PhaseClock* clock) {
  Layout in, out;
  const auto s_jobs = in.take<PrepJobDev>(P.jobs.size());
  const auto s_taps = in.take<PyrTap>(P.taps.size());
  out.take<int>(1);   // nothing comes back through this staging
  OSH_TRY(st->call.reserve(in, out));
  OSH_TRY(st->raw.reserve(P.raw_bytes));
  unsigned char* hr = static_cast<unsigned char*>(st->h_raw.reserve(P.raw_bytes));
  if (!hr) { set_error("%s: pinned allocation of %zu bytes failed", entry, P.raw_bytes); return OSH_ERR_DEVICE; }
  for (int k = 0; k < n_frames; ++k) {
    P.jobs[k].dst_off = dst_off[k];
    const osh_prepare_image& im = frames[k].image;
    unsigned char* to = hr + P.jobs[k].src_off;
    if ((size_t)im.stride == P.raw_row[k]) std::memcpy(to, im.data, P.raw_row[k] * im.rows);
    else for (int r = 0; r < im.rows; ++r) std::memcpy(to + (size_t)r * P.raw_row[k], im.data + (int64_t)r * im.stride, P.raw_row[k]);
  }
  char* h = st->call.host_in();
  std::memcpy(s_jobs.in(h), P.jobs.data(), sizeof(PrepJobDev) * P.jobs.size());
  if (!P.taps.empty()) std::memcpy(s_taps.in(h), P.taps.data(), sizeof(PyrTap) * P.taps.size());
  if (clock) clock->mark();
  OSH_TRY(st->call.upload(s));
  OSH_HIP(hipMemcpyAsync(st->raw.p, hr, P.raw_bytes, hipMemcpyHostToDevice, s));
  if (clock) OSH_TRY(clock->mark_synced(s));
  PrepView v{};
  char* di = st->call.dev_in();
  v.jobs = s_jobs.in(di); v.taps = s_taps.in(di); v.raw = st->raw.as<const unsigned char>(); v.dst = dst;
  hipLaunchKernelGGL(k_prepare, dim3(P.max_tiles, (unsigned)n_frames), dim3(kPrepBlockX, kPrepBlockY), 0, s, v);
  return launch_check("prepare");
}

// The prepared images (frame k at src + off[k] on the device, rows packed) into the frames' gray pointers through one D2H copy of
// the `bytes` at src; the sizes into every result
static int prepare_collect(const char* entry, PrepState* st, hipStream_t s, int n_frames, const PrepPlan& P, const unsigned char* src, size_t bytes,
                           const long long* off, osh_prepare_result* results) {
  bool any = false;
  for (int k = 0; k < n_frames; ++k) { results[k].rows = P.jobs[k].dst_rows; results[k].cols = P.jobs[k].dst_cols; any |= results[k].gray != nullptr; }
  if (!any) return OSH_OK;
  unsigned char* hg = static_cast<unsigned char*>(st->h_gray.reserve(bytes));
  if (!hg) { set_error("%s: pinned allocation of %zu bytes failed", entry, bytes); return OSH_ERR_DEVICE; }
  OSH_HIP(hipMemcpyAsync(hg, src, bytes, hipMemcpyDeviceToHost, s));
  OSH_HIP(hipStreamSynchronize(s));
  for (int k = 0; k < n_frames; ++k) {
    const osh_prepare_result& r = results[k];
    for (int y = 0; r.gray && y < r.rows; ++y) std::memcpy(r.gray + (int64_t)y * r.gray_stride, hg + off[k] + (size_t)y * r.cols, (size_t)r.cols);
  }
  return OSH_OK;
}

}  // namespace osh

extern "C" int osh_orb_prepare(osh_orb_ctx* c, int32_t n_frames, const osh_prepare_frame* frames, osh_prepare_result* results) {
  PhaseClock clock;
  const char* entry = "osh_orb_prepare";
  if (n_frames < 0 || (n_frames && (!frames || !results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  PrepPlan P;
  OSH_TRY(prepare_plan(entry, n_frames, frames, results, P));   // a refusal needs no context and no device
  if (!c) { set_error("%s: no context", entry); return OSH_ERR_INVALID; }
  if (n_frames == 0) return OSH_OK;
  if (n_frames > 65535) { set_error("%s: more than 65535 frames in one call", entry); return OSH_ERR_UNSUPPORTED; }
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  OSH_TRY(prepare_check_device(entry, n_frames, frames, device));
  PrepState* st = orb_state<PrepState>(c, kOrbAttachPrepare);
  clock.profiling = orb_profiling(c);
  std::vector<long long> off((size_t)n_frames);
  size_t bytes = 0;
  for (int k = 0; k < n_frames; ++k) { off[k] = (long long)bytes; bytes += (size_t)P.jobs[k].dst_rows * P.jobs[k].dst_cols; }
  OSH_TRY(st->gray.reserve(bytes));
  OSH_TRY(prepare_produce(entry, st, s, n_frames, frames, P, st->gray.as<unsigned char>(), off.data(), &clock));
  OSH_HIP(hipStreamSynchronize(s));   // the staging buffers are free again when the call returns
  clock.mark();
  OSH_TRY(prepare_collect(entry, st, s, n_frames, P, st->gray.as<const unsigned char>(), bytes, off.data(), results));
  clock.mark();
  clock.store(st->ms);
  return OSH_OK;
}

namespace osh {

int extract_raw_from(const char* entry, osh_orb_ctx* c, int32_t n_frames, const osh_prepare_frame* prepare_frames, const osh_extract_frame* extract_frames,
                     osh_extract_result* extract_results, osh_prepare_result* prepare_results, const ExtractTail* tail) {
  if (n_frames < 0 || (n_frames && (!prepare_frames || !extract_frames || !extract_results))) { set_error("%s: bad arguments", entry); return OSH_ERR_INVALID; }
  PrepPlan P;
  OSH_TRY(prepare_plan(entry, n_frames, prepare_frames, prepare_results, P));   // a refusal needs no context and no device
  std::vector<osh_extract_frame> ef(extract_frames, extract_frames + n_frames);
  for (int k = 0; k < n_frames; ++k) {
    const osh_stereo_image& im = extract_frames[k].image;
    const int rows = P.jobs[k].dst_rows, cols = P.jobs[k].dst_cols;
    if (im.data) { set_error("%s: frame %d: the extract frame brings image data; level 0 is made from the raw image", entry, k); return OSH_ERR_INVALID; }
    if (!(im.rows == 0 && im.cols == 0) && (im.rows != rows || im.cols != cols)) {
      set_error("%s: frame %d: the extract frame names a %d x %d image, the prepared image is %d x %d", entry, k, im.rows, im.cols, rows, cols); return OSH_ERR_INVALID;
    }
    ef[k].image = {nullptr, rows, cols, cols};
  }
  if (n_frames > 65535) { set_error("%s: more than 65535 frames in one call", entry); return OSH_ERR_UNSUPPORTED; }
  PrepState* st = nullptr;
  Level0Producer producer;
  producer.check = [&](int device) { return prepare_check_device(entry, n_frames, prepare_frames, device); };
  producer.produce = [&](hipStream_t s, unsigned char* images, const std::vector<long long>& level0_off) {
    st = orb_state<PrepState>(c, kOrbAttachPrepare);
    return prepare_produce(entry, st, s, n_frames, prepare_frames, P, images, level0_off.data(), nullptr);
  };
  OSH_TRY(extract_from(entry, c, n_frames, ef.data(), extract_results, &producer, tail));
  if (n_frames == 0 || !prepare_results) return OSH_OK;
  // the prepared images are the level 0 of the frames: they lie one after another at the start of the resident pyramid
  int device = 0;
  hipStream_t s = nullptr;
  OSH_TRY(orb_stream(c, &device, &s));
  const ResidentPyramid& rp = orb_state<FastState>(c, kOrbAttachFast)->pyramid;
  std::vector<long long> off((size_t)n_frames);
  for (int k = 0; k < n_frames; ++k) off[k] = rp.levels[rp.frames[k].level0].img_off;
  return prepare_collect(entry, st, s, n_frames, P, rp.images(), P.out_bytes, off.data(), prepare_results);
}

}  // namespace osh

extern "C" int osh_orb_extract_raw(osh_orb_ctx* c, int32_t n_frames, const osh_prepare_frame* prepare_frames, const osh_extract_frame* extract_frames,
                                   osh_extract_result* extract_results, osh_prepare_result* prepare_results) {
  return extract_raw_from("osh_orb_extract_raw", c, n_frames, prepare_frames, extract_frames, extract_results, prepare_results, nullptr);
}

extern "C" int osh_orb_prepare_get_times(osh_orb_ctx* c, double ms[4]) {
  return copy_times<PrepState>("osh_orb_prepare_get_times", c, kOrbAttachPrepare, ms);
}
