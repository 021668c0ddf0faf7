// sim3opt.cc -- osh_host_pack_sim3 / osh_host_optimize_sim3 (include/orbslam3_hip_host.h): Optimizer::OptimizeSim3 and its pair
// walk on two stand-in keyframes, their map points and a vpMatches1 built from flat arrays.
#include <cstdint>
#include <cstring>
#include <memory>
#include <tuple>
#include <vector>

#include "Optimizer.h"
#include "host_pack.h"
#include "orbslam3_hip.h"
#include "orbslam3_hip_host.h"

using namespace ORB_SLAM3;

namespace {

struct Sim3Scene {
  Map map;
  std::unique_ptr<GeometricCamera> cam1, cam2;
  std::unique_ptr<KeyFrame> kf1, kf2;
  std::vector<std::unique_ptr<MapPoint>> mps;
  std::vector<MapPoint*> matches1;
  g2o::Sim3 S12;
};

std::unique_ptr<GeometricCamera> make_camera(const osh_host_sim3_kf& k) {
  if (k.kb8) return std::unique_ptr<GeometricCamera>(new KannalaBrandt8(std::vector<float>(k.cam, k.cam + 8)));
  return std::unique_ptr<GeometricCamera>(new Pinhole(std::vector<float>(k.cam, k.cam + 4)));
}

void fill_keyframe(KeyFrame& kf, const osh_host_sim3_kf& k, GeometricCamera* cam) {
  kf.mTcw.set_raw(Eigen::Quaternionf(k.pose[3], k.pose[0], k.pose[1], k.pose[2]), Eigen::Vector3f(k.pose[4], k.pose[5], k.pose[6]));
  kf.mpCamera = cam;
  kf.N = k.n_keys;
  kf.mvKeysUn.resize(k.n_keys);
  for (int i = 0; i < k.n_keys; ++i) {
    kf.mvKeysUn[i].pt.x = k.keys_un[2 * i];
    kf.mvKeysUn[i].pt.y = k.keys_un[2 * i + 1];
    kf.mvKeysUn[i].octave = k.octave[i];
  }
  kf.mvInvLevelSigma2.assign(k.inv_level_sigma2, k.inv_level_sigma2 + k.n_levels);
  kf.mvpMapPoints.assign(k.n_keys, nullptr);
}

bool build(const osh_host_sim3_input* in, Sim3Scene& sc) {
  if (!in || in->n_points < 0 || in->n_matches < 0 || in->kf1.n_keys < 0 || in->kf2.n_keys < 0) return false;
  sc.cam1 = make_camera(in->kf1);
  sc.cam2 = make_camera(in->kf2);
  sc.kf1.reset(new KeyFrame(1, &sc.map));
  sc.kf2.reset(new KeyFrame(2, &sc.map));
  fill_keyframe(*sc.kf1, in->kf1, sc.cam1.get());
  fill_keyframe(*sc.kf2, in->kf2, sc.cam2.get());
  for (int p = 0; p < in->n_points; ++p) {
    MapPoint* mp = new MapPoint(p, Eigen::Vector3f(in->mp_pos[3 * p], in->mp_pos[3 * p + 1], in->mp_pos[3 * p + 2]), &sc.map);
    mp->mbBad = in->mp_bad[p] != 0;
    mp->mnTrackScaleLevel = in->mp_track_level[p];
    if (in->mp_index2[p] >= 0) mp->mObservations[sc.kf2.get()] = std::tuple<int, int>(in->mp_index2[p], -1);
    sc.mps.emplace_back(mp);
  }
  for (int i = 0; i < in->kf1.n_keys; ++i) {
    const int p = in->kf1_mp[i];
    if (p >= in->n_points) return false;
    sc.kf1->mvpMapPoints[i] = p >= 0 ? sc.mps[p].get() : nullptr;
  }
  sc.matches1.assign(in->n_matches, nullptr);
  for (int i = 0; i < in->n_matches; ++i) {
    const int p = in->matches1[i];
    if (p >= in->n_points) return false;
    sc.matches1[i] = p >= 0 ? sc.mps[p].get() : nullptr;
  }
  const double* S = in->S12;
  sc.S12 = g2o::Sim3(Eigen::Quaterniond(S[3], S[0], S[1], S[2]), Eigen::Vector3d(S[4], S[5], S[6]), S[7]);
  return true;
}

}  // namespace

extern "C" int osh_host_pack_sim3(const osh_host_sim3_input* in, int32_t max_pairs, osh_sim3_problem* out, int32_t* index, double* X1c,
                                  double* X2c, double* obs1, double* obs2, double* info1, double* info2) {
  Sim3Scene sc;
  if (!out || !build(in, sc)) return -1;
  Sim3OptPack pk;
  if (!PackOptimizeSim3(sc.kf1.get(), sc.kf2.get(), sc.matches1, in->all_points != 0, pk)) return -1;
  const int n = (int)pk.index.size();
  if (n > max_pairs) return -1;
  pk.fill(*out, sc.S12, in->th2, in->fix_scale != 0);
  for (int k = 0; k < n; ++k) index[k] = pk.index[k];
  std::memcpy(X1c, pk.X1c.data(), sizeof(double) * 3 * n);
  std::memcpy(X2c, pk.X2c.data(), sizeof(double) * 3 * n);
  std::memcpy(obs1, pk.obs1.data(), sizeof(double) * 2 * n);
  std::memcpy(obs2, pk.obs2.data(), sizeof(double) * 2 * n);
  std::memcpy(info1, pk.info1.data(), sizeof(double) * n);
  std::memcpy(info2, pk.info2.data(), sizeof(double) * n);
  out->X1c = X1c; out->X2c = X2c; out->obs1 = obs1; out->obs2 = obs2; out->info1 = info1; out->info2 = info2;
  return n;
}

extern "C" int osh_host_optimize_sim3(const osh_host_sim3_input* in, uint8_t* nulled, double* S12, double* hessian) {
  Sim3Scene sc;
  if (!nulled || !S12 || !hessian || !build(in, sc)) return -1;
  Eigen::Matrix<double, 7, 7> H;
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) H(r, c) = hessian[r * 7 + c];
  const std::vector<MapPoint*> before = sc.matches1;
  const int ret = Optimizer::OptimizeSim3(sc.kf1.get(), sc.kf2.get(), sc.matches1, sc.S12, in->th2, in->fix_scale != 0, H, in->all_points != 0);
  for (int i = 0; i < in->n_matches; ++i) nulled[i] = (before[i] && !sc.matches1[i]) ? 1 : 0;
  const Eigen::Quaterniond& q = sc.S12.rotation();
  const Eigen::Vector3d& t = sc.S12.translation();
  const double S[8] = {q.x(), q.y(), q.z(), q.w(), t(0), t(1), t(2), sc.S12.scale()};
  for (int k = 0; k < 8; ++k) S12[k] = S[k];
  for (int r = 0; r < 7; ++r)
    for (int c = 0; c < 7; ++c) hessian[r * 7 + c] = H(r, c);
  return ret;
}
