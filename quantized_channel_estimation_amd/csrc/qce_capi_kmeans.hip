// C ABI of the device k-means (qce_kmeans_lloyd): sklearn's _kmeans_single_lloyd loop around the kernels of
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
