// C ABI of the device k-means.  qce_kmeans_seed: sklearn's _kmeans_plusplus from pre-drawn uniforms on the kernels of
// qce_kmeans_seed.hip (below).  qce_kmeans_lloyd: sklearn's _kmeans_single_lloyd loop around the kernels of
// qce_kmeans.hip.  The host reads three scalars per iteration (centre shift, changed labels, empty clusters); the
// empty-cluster relocation (_relocate_empty_clusters_dense), a rare path, picks its rows on the host from the per-row
// distances.
#include <math.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "qce_capi.h"
#include "qce_kmeans.h"

#define QCE_KM_MAX_N 256
#define QCE_KM_MAX_K 1024
#define QCE_KM_MAX_TRIALS 16

extern "C" int qce_kmeans_lloyd(const double* X, int64_t B, int N, int K, const double* x_mean,
                                const double* centers_init, int max_iter, double tol_abs, double* centers_out,
                                int64_t* labels_out, double* resp_out, double* info_out, int device, int io,
                                void* stream) {
  if (B < 1 || N < 1 || K < 1 || max_iter < 1 || !X || !centers_init || !centers_out || !labels_out || !info_out)
    return qce_set_error(QCE_EARG, "kmeans_lloyd: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "kmeans_lloyd: bad io");
  if (N > QCE_KM_MAX_N) return qce_set_error(QCE_ENOTIMPL, "kmeans_lloyd: N <= " + std::to_string(QCE_KM_MAX_N));
  if (K > QCE_KM_MAX_K) return qce_set_error(QCE_ENOTIMPL, "kmeans_lloyd: K <= " + std::to_string(QCE_KM_MAX_K));
  if ((int64_t)K > B)
    return qce_set_error(QCE_EARG, "kmeans_lloyd: n_samples=" + std::to_string(B) + " should be >= n_clusters=" +
                                       std::to_string(K) + ".");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const QceKmPlan p = qce_km_plan(B, N, K);
  const int D = p.D, DP = p.DP, KP = p.KP;
  const size_t nC = (size_t)KP * DP, nX = (size_t)B * D;

  // padded host images of the mean and the initial centres
  std::vector<double> hmean(DP, 0.0), hC(nC, 0.0);
  if (x_mean) std::copy(x_mean, x_mean + D, hmean.begin());
  for (int k = 0; k < K; ++k) std::copy(centers_init + (size_t)k * D, centers_init + (size_t)(k + 1) * D, &hC[(size_t)k * DP]);

  DevBuf<double> dX, dmean, dCa, dCb, dcnorm, dpart, dpcount, dsums, dcounts, dstatus, ddist, dresp;
  DevBuf<long long> dlabels, dfar;
  DevBuf<int> dpchanged, dempt;
  const double* x = X;
  long long* labels = (long long*)labels_out;
  double* resp = resp_out;
  if (io == QCE_IO_HOST) {
    HIPCHK(dX.ensure(nX));
    HIPCHK(hipMemcpyAsync(dX.p, X, sizeof(double) * nX, hipMemcpyHostToDevice, st));
    x = dX.p;
    HIPCHK(dlabels.ensure((size_t)B));
    labels = dlabels.p;
    if (resp_out) {
      HIPCHK(dresp.ensure((size_t)B * K));
      resp = dresp.p;
    }
  }
  HIPCHK(dmean.ensure(DP));
  HIPCHK(dCa.ensure(nC));
  HIPCHK(dCb.ensure(nC));
  HIPCHK(dcnorm.ensure(KP));
  HIPCHK(dpart.ensure((size_t)p.C * nC));
  HIPCHK(dpcount.ensure((size_t)p.C * KP));
  HIPCHK(dsums.ensure(nC));
  HIPCHK(dcounts.ensure(KP));
  HIPCHK(dstatus.ensure(4));
  HIPCHK(ddist.ensure((size_t)B));
  HIPCHK(dpchanged.ensure(p.nwg));
  HIPCHK(hipMemcpyAsync(dmean.p, hmean.data(), sizeof(double) * DP, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(dCa.p, hC.data(), sizeof(double) * nC, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(labels, 0xFF, sizeof(long long) * (size_t)B, st));  // every label -1

  double *cur = dCa.p, *nxt = dCb.p;
  double status[3] = {0.0, 0.0, 0.0};
  bool strict = false;
  int n_iter = 0;
  long long relocated = 0;
  for (int it = 0; it < max_iter; ++it) {
    HIPCHK(qce_launch_km_cnorm(p, cur, dcnorm.p, st));
    HIPCHK(qce_launch_km_assign(p, x, dmean.p, cur, dcnorm.p, labels, dpchanged.p, st));
    HIPCHK(qce_launch_km_accum(p, x, dmean.p, labels, dpart.p, dpcount.p, st));
    HIPCHK(qce_launch_km_sums(p, dpart.p, dpcount.p, dsums.p, dcounts.p, st));
    HIPCHK(qce_launch_km_finalize(p, dsums.p, dcounts.p, dpchanged.p, cur, nxt, dstatus.p, st));
    HIPCHK(hipMemcpyAsync(status, dstatus.p, sizeof(status), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const int n_empty = (int)status[2];
    if (n_empty > 0) {
      // the n_empty rows farthest from their (old) centres, in descending distance (equal distances: lower row first),
      // become the empty clusters in ascending index; labels stay as they are
      std::vector<double> hdist((size_t)B), hcounts(KP);
      HIPCHK(qce_launch_km_rowdist(p, x, dmean.p, cur, labels, ddist.p, st));
      HIPCHK(hipMemcpyAsync(hdist.data(), ddist.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(hcounts.data(), dcounts.p, sizeof(double) * KP, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      std::vector<long long> idx((size_t)B);
      std::iota(idx.begin(), idx.end(), 0ll);
      std::partial_sort(idx.begin(), idx.begin() + n_empty, idx.end(), [&](long long a, long long b) {
        return hdist[a] > hdist[b] || (hdist[a] == hdist[b] && a < b);
      });
      std::vector<int> empt;
      for (int k = 0; k < K; ++k)
        if (hcounts[k] == 0.0) empt.push_back(k);
      if ((int)empt.size() != n_empty) return qce_set_error(QCE_ESTATE, "kmeans_lloyd: empty-cluster count mismatch");
      HIPCHK(dfar.ensure(n_empty));
      HIPCHK(dempt.ensure(n_empty));
      HIPCHK(hipMemcpyAsync(dfar.p, idx.data(), sizeof(long long) * n_empty, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(dempt.p, empt.data(), sizeof(int) * n_empty, hipMemcpyHostToDevice, st));
      HIPCHK(qce_launch_km_relocate(p, x, dmean.p, labels, dfar.p, dempt.p, n_empty, dsums.p, dcounts.p, st));
      HIPCHK(qce_launch_km_finalize(p, dsums.p, dcounts.p, dpchanged.p, cur, nxt, dstatus.p, st));
      HIPCHK(hipMemcpyAsync(status, dstatus.p, sizeof(status), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));  // also: idx / empt stay alive until their copies are done
      relocated += n_empty;
    }
    std::swap(cur, nxt);
    n_iter = it + 1;
    if (status[1] == 0.0) {
      strict = true;
      break;
    }
    if (status[0] <= tol_abs) break;
  }
  if (!strict) {  // labels of the final centres
    HIPCHK(qce_launch_km_cnorm(p, cur, dcnorm.p, st));
    HIPCHK(qce_launch_km_assign(p, x, dmean.p, cur, dcnorm.p, labels, dpchanged.p, st));
  }
  HIPCHK(qce_launch_km_rowdist(p, x, dmean.p, cur, labels, ddist.p, st));
  HIPCHK(qce_launch_km_vsum(B, ddist.p, dstatus.p + 3, st));
  if (resp_out) HIPCHK(qce_launch_km_onehot(p, labels, resp, st));
  double inertia = 0.0;
  HIPCHK(hipMemcpyAsync(&inertia, dstatus.p + 3, sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(hC.data(), cur, sizeof(double) * nC, hipMemcpyDeviceToHost, st));
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(labels_out, labels, sizeof(long long) * (size_t)B, hipMemcpyDeviceToHost, st));
    if (resp_out)
      HIPCHK(hipMemcpyAsync(resp_out, resp, sizeof(double) * (size_t)B * K, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // results written; the scratch above is freed on return
  for (int k = 0; k < K; ++k) std::copy(&hC[(size_t)k * DP], &hC[(size_t)k * DP] + D, centers_out + (size_t)k * D);
  info_out[0] = (double)n_iter;
  info_out[1] = inertia;
  info_out[2] = strict ? 1.0 : 0.0;
  info_out[3] = (double)relocated;
  return QCE_OK;
}

// k-means++ seeding from pre-drawn uniforms: every step is enqueued (the uniforms are known), the host waits once at
// the end.  Two launches per further centre: pick + search, then the candidate pass.
extern "C" int qce_kmeans_seed(const double* X, int64_t B, int N, int K, const double* x_mean, int64_t first,
                               const double* u, int n_trials, int64_t* indices_out, double* centers_out,
                               int64_t* cand_out, double* pot_out, int device, int io, void* stream) {
  if (B < 1 || N < 1 || K < 1 || n_trials < 1 || !X || !indices_out || !centers_out || (K > 1 && !u))
    return qce_set_error(QCE_EARG, "kmeans_seed: bad arguments");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "kmeans_seed: bad io");
  if (N > QCE_KM_MAX_N) return qce_set_error(QCE_ENOTIMPL, "kmeans_seed: N <= " + std::to_string(QCE_KM_MAX_N));
  if (K > QCE_KM_MAX_K) return qce_set_error(QCE_ENOTIMPL, "kmeans_seed: K <= " + std::to_string(QCE_KM_MAX_K));
  if (n_trials > QCE_KM_MAX_TRIALS)
    return qce_set_error(QCE_ENOTIMPL, "kmeans_seed: n_trials <= " + std::to_string(QCE_KM_MAX_TRIALS));
  if ((int64_t)K > B)
    return qce_set_error(QCE_EARG, "kmeans_seed: n_samples=" + std::to_string(B) + " should be >= n_clusters=" +
                                       std::to_string(K) + ".");
  if (first < 0 || first >= B)
    return qce_set_error(QCE_EARG, "kmeans_seed: first=" + std::to_string(first) + " is outside [0, n_samples=" +
                                       std::to_string(B) + ")");
  const int T = n_trials;
  const size_t nU = (size_t)(K - 1) * T;
  for (size_t i = 0; i < nU; ++i)
    if (!(u[i] >= 0.0 && u[i] < 1.0)) return qce_set_error(QCE_EARG, "kmeans_seed: u must be in [0, 1)");
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const QceKmSeedPlan p = qce_km_seed_plan(B, N);
  const int D = 2 * N;
  const size_t nX = (size_t)B * D;

  DevBuf<double> dX, dmean, du, dsa, dsb, dpa, dpb, dpot, dcent;
  DevBuf<long long> dcand, didx;
  DevBuf<int> dwin;
  const double* x = X;
  if (io == QCE_IO_HOST) {
    HIPCHK(dX.ensure(nX));
    HIPCHK(hipMemcpyAsync(dX.p, X, sizeof(double) * nX, hipMemcpyHostToDevice, st));
    x = dX.p;
  }
  if (x_mean) {
    HIPCHK(dmean.ensure(D));
    HIPCHK(hipMemcpyAsync(dmean.p, x_mean, sizeof(double) * D, hipMemcpyHostToDevice, st));
  }
  HIPCHK(du.ensure(nU));
  if (nU) HIPCHK(hipMemcpyAsync(du.p, u, sizeof(double) * nU, hipMemcpyHostToDevice, st));
  HIPCHK(dsa.ensure((size_t)T * p.stride));
  HIPCHK(dsb.ensure((size_t)T * p.stride));
  HIPCHK(dpa.ensure((size_t)T * p.C));
  HIPCHK(dpb.ensure((size_t)T * p.C));
  HIPCHK(dpot.ensure(K));
  HIPCHK(didx.ensure(K));
  HIPCHK(dwin.ensure(K));
  HIPCHK(dcand.ensure(1 + nU));  // [0]: the first centre; then (K - 1, T) candidate rows
  HIPCHK(dcent.ensure((size_t)K * D));
  const long long first_ll = first;
  HIPCHK(hipMemcpyAsync(dcand.p, &first_ll, sizeof(long long), hipMemcpyHostToDevice, st));

  double *scur = dsa.p, *snxt = dsb.p, *pcur = dpa.p, *pnxt = dpb.p;
  HIPCHK(qce_launch_km_seed_cand(p, 1, x, dmean.p, dcand.p, nullptr, nullptr, scur, pcur, st));
  const long long* cand_prev = dcand.p;
  int Tprev = 1;
  for (int c = 1; c < K; ++c) {
    long long* cand_c = dcand.p + 1 + (size_t)(c - 1) * T;
    HIPCHK(qce_launch_km_seed_pick(p, Tprev, pcur, scur, cand_prev, du.p + (size_t)(c - 1) * T, T, didx.p + (c - 1),
                                   dpot.p + (c - 1), dwin.p + (c - 1), cand_c, st));
    HIPCHK(qce_launch_km_seed_cand(p, T, x, dmean.p, cand_c, scur, dwin.p + (c - 1), snxt, pnxt, st));
    std::swap(scur, snxt);
    std::swap(pcur, pnxt);
    cand_prev = cand_c;
    Tprev = T;
  }
  HIPCHK(qce_launch_km_seed_pick(p, Tprev, pcur, scur, cand_prev, nullptr, 0, didx.p + (K - 1), dpot.p + (K - 1),
                                 dwin.p + (K - 1), nullptr, st));
  HIPCHK(qce_launch_km_seed_gather(p, K, x, dmean.p, didx.p, dcent.p, st));
  HIPCHK(hipMemcpyAsync(indices_out, didx.p, sizeof(long long) * K, hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(centers_out, dcent.p, sizeof(double) * (size_t)K * D, hipMemcpyDeviceToHost, st));
  if (cand_out && nU)
    HIPCHK(hipMemcpyAsync(cand_out, dcand.p + 1, sizeof(long long) * nU, hipMemcpyDeviceToHost, st));
  if (pot_out) HIPCHK(hipMemcpyAsync(pot_out, dpot.p, sizeof(double) * K, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));  // results written; first_ll and the scratch above live until here
  return QCE_OK;
}
