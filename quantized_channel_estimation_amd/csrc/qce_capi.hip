// C ABI of libqce.so (declared in include/qce.h), model side: the error slot, model lifetime, options, info and
// the dense tables.  The other entry points: qce_capi_prepare.hip (per-SNR prepare), qce_capi_estimate.hip (estimate /
// log-prob / partials), qce_capi_hostio.hip (host-I/O pipelines), qce_capi_free.hip (model-free entry points).
#include <math.h>
#include <string.h>

#include <string>
#include <vector>

#include "qce_capi.h"

namespace {
thread_local std::string g_err;
}  // namespace

int qce_set_error(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

// the mixture's parameters: host copies and flags, then the device tables on the model's stream (synchronised)
hipError_t upload_params(qce_model* m, const double* means_cplx, const double* covs_cplx, const double* weights) {
  const int K = m->K, N = m->N;
  m->weights.assign(weights, weights + K);
  std::vector<double> logw(K);
  for (int k = 0; k < K; ++k) logw[k] = log(weights[k]);
  std::vector<double> mz((size_t)2 * K * N, 0.0);
  m->has_mean = 0;
  if (means_cplx) {
    memcpy(mz.data(), means_cplx, sizeof(double) * 2 * (size_t)K * N);
    for (double v : mz)
      if (v != 0.0) {
        m->has_mean = 1;
        break;
      }
  }
  hipError_t e = hipMemcpyAsync(m->means.p, mz.data(), sizeof(double2) * (size_t)K * N, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(m->covs.p, covs_cplx, sizeof(double2) * (size_t)K * N * N, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(m->logw.p, logw.data(), sizeof(double) * K, hipMemcpyHostToDevice, m->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(m->stream);
  return e;
}

}  // namespace

extern "C" {

int qce_version(void) { return 200; }

const char* qce_last_error(void) { return g_err.c_str(); }

int qce_device_count(int* count) {
  if (!count) return qce_set_error(QCE_EARG, "null count");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) n = 0;
  *count = n;
  return QCE_OK;
}

int qce_model_create(int K, int N, const double* means_cplx, const double* covs_cplx, const double* weights,
                     int device, qce_model** out) {
  if (!out || !covs_cplx || !weights) return qce_set_error(QCE_EARG, "null argument");
  *out = nullptr;
  if (K <= 0 || N <= 0) return qce_set_error(QCE_EARG, "K and N must be positive");
  if (N > QCE_BIG_MAX) return qce_set_error(QCE_ENOTIMPL, "N > " + std::to_string(QCE_BIG_MAX) + " is not covered");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return qce_set_error(QCE_EHIP, "no HIP device visible");
  if (device < 0 || device >= ndev) return qce_set_error(QCE_EARG, "device index out of range");
  DeviceGuard g(device);
  qce_model* m = new qce_model();
  m->K = K;
  m->N = N;
  m->device = device;
  if (hipDeviceGetAttribute(&m->cu_count, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
      m->cu_count < 1)
    m->cu_count = 256;
  hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = m->means.ensure((size_t)K * N);
  if (e == hipSuccess) e = m->covs.ensure((size_t)K * N * N);
  if (e == hipSuccess) e = m->logw.ensure(K);
  if (e == hipSuccess) e = upload_params(m, means_cplx, covs_cplx, weights);
  if (e != hipSuccess) {
    qce_model_destroy(m);
    return qce_set_error(QCE_EHIP, std::string("model allocation failed: ") + hipGetErrorString(e));
  }
  if ((e = detect_structure(m)) != hipSuccess) {
    qce_model_destroy(m);
    return qce_set_error(QCE_EHIP, std::string("structure detection failed: ") + hipGetErrorString(e));
  }
  *out = m;
  return QCE_OK;
}

int qce_model_set_params(qce_model* m, const double* means_cplx, const double* covs_cplx, const double* weights) {
  if (!m || !covs_cplx || !weights) return qce_set_error(QCE_EARG, "null argument");
  DeviceGuard g(m->device);
  HIPCHK(hipStreamSynchronize(m->stream));
  HIPCHK(upload_params(m, means_cplx, covs_cplx, weights));
  m->prepared = 0;
  HIPCHK(detect_structure(m));
  return QCE_OK;
}

int qce_model_destroy(qce_model* m) {
  if (!m) return QCE_OK;
  DeviceGuard g(m->device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  if (m->status_host) (void)hipHostFree(m->status_host);
  if (m->status_ev) (void)hipEventDestroy(m->status_ev);
  for (int i = 0; i < 2; ++i) {
    if (m->hp.pin_y[i]) (void)hipHostFree(m->hp.pin_y[i]);
    if (m->hp.pin_h[i]) (void)hipHostFree(m->hp.pin_h[i]);
    for (hipEvent_t ev : {m->hp.ev_in[i], m->hp.ev_c[i], m->hp.ev_out[i]})
      if (ev) (void)hipEventDestroy(ev);
  }
  for (hipStream_t hs : {m->hp.s_in, m->hp.s_out})
    if (hs) {
      (void)hipStreamSynchronize(hs);
      (void)hipStreamDestroy(hs);
    }
  if (m->stream) (void)hipStreamDestroy(m->stream);
  delete m;  // every DevBuf frees its memory here, still under the device guard
  return QCE_OK;
}

int qce_cconst_max(qce_model* m, double* out, int io, void* stream) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (!out) return qce_set_error(QCE_EARG, "null out");
  DeviceGuard g(m->device);
  hipStream_t st = pick_stream(m, stream);
  if ((rc = ensure_dense(m, st))) return rc;
  if (io == QCE_IO_HOST) {
    HIPCHK(m->shift_scr.ensure(1));
    HIPCHK(qce_launch_cconst_max(m->K, m->cconst.p, m->status.p, m->shift_scr.p, st));
    HIPCHK(hipMemcpyAsync(out, m->shift_scr.p, sizeof(double), hipMemcpyDeviceToHost, st));
    HOST_SYNC_CHECK(m, st);
  } else {
    HIPCHK(qce_launch_cconst_max(m->K, m->cconst.p, m->status.p, out, st));
  }
  return QCE_OK;
}

int qce_get_tables(qce_model* m, double* means_y, double* Cy, double* Cr, double* P, double* A_eff, double* W,
                   double* b, double* cconst) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if ((rc = ensure_dense(m))) return rc;
  DeviceGuard g(m->device);
  hipStream_t st = m->stream;
  const int K = m->K, M = m->M, N = m->N;
  HOST_SYNC_CHECK(m, st);
  auto cp = [&](double* dst, const void* src, size_t bytes) -> hipError_t {
    if (!dst) return hipSuccess;
    return hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost);
  };
  HIPCHK(cp(means_y, m->means_y.p, sizeof(double2) * (size_t)K * M));
  HIPCHK(cp(Cy, m->Cy.p, sizeof(double2) * (size_t)K * M * M));
  HIPCHK(cp(Cr, m->Cr.p, sizeof(double2) * (size_t)K * M * M));
  HIPCHK(cp(A_eff, m->Aeff.p, sizeof(double2) * (size_t)K * M * N));
  HIPCHK(cp(W, m->W.p, sizeof(double2) * (size_t)K * N * M));
  HIPCHK(cp(b, m->bvec.p, sizeof(double2) * (size_t)K * N));
  HIPCHK(cp(cconst, m->cconst.p, sizeof(double) * (size_t)K));
  if (P) {
    std::vector<double> li((size_t)2 * K * M * M);
    HIPCHK(hipMemcpy(li.data(), m->Linv.p, sizeof(double2) * (size_t)K * M * M, hipMemcpyDeviceToHost));
    for (int k = 0; k < K; ++k)
      for (int i = 0; i < M; ++i)
        for (int j = 0; j < M; ++j) {
          const size_t src = ((size_t)k * M * M + (size_t)j * M + i) * 2;  // P[i][j] = conj(Linv[j][i])
          const size_t dst = ((size_t)k * M * M + (size_t)i * M + j) * 2;
          P[dst] = li[src];
          P[dst + 1] = (j >= i) ? -li[src + 1] : 0.0;
          if (j < i) P[dst] = 0.0;
        }
  }
  return QCE_OK;
}

int qce_model_info(qce_model* m, int* K, int* N, int* M, int* device) {
  if (!m) return qce_set_error(QCE_EARG, "null model");
  if (K) *K = m->K;
  if (N) *N = m->N;
  if (M) *M = m->prepared ? m->M : 0;
  if (device) *device = m->device;
  return QCE_OK;
}

int qce_model_structure(qce_model* m, int* n1, int* n2, int* fourier_active) {
  if (!m) return qce_set_error(QCE_EARG, "null model");
  if (n1) *n1 = m->fft_n1;
  if (n2) *n2 = m->fft_n2;
  if (fourier_active) *fourier_active = m->prepared && qce_be_fourier(m->backend);
  return QCE_OK;
}

int qce_model_kernel(qce_model* m, int* kind) {
  if (!m || !kind) return qce_set_error(QCE_EARG, "null argument");
  *kind = QCE_KERNEL_NONE;
  if (!m->prepared) return QCE_OK;
  switch (m->backend) {
    case QCE_BE_NONE: break;
    case QCE_BE_FOURIER: *kind = QCE_KERNEL_FOURIER; break;
    case QCE_BE_BIG: *kind = QCE_KERNEL_BIG; break;
    case QCE_BE_F64_4M: *kind = QCE_KERNEL_F64_4M; break;
    case QCE_BE_F64_3M:
    case QCE_BE_F64_3M_128: *kind = QCE_KERNEL_F64_3M; break;
    case QCE_BE_F64_WIDE: *kind = QCE_KERNEL_F64_WIDE; break;
    case QCE_BE_FAST: *kind = QCE_KERNEL_FAST; break;
    case QCE_BE_INT8: *kind = QCE_KERNEL_INT8; break;
    case QCE_BE_FOURIER_PILOTS: *kind = QCE_KERNEL_FOURIER_PILOTS; break;
  }
  return QCE_OK;
}

int qce_model_set_option(qce_model* m, int option, double value) {
  if (!m) return qce_set_error(QCE_EARG, "null model");
  if (option == QCE_OPT_BETA_FIRST) {
    m->beta_first = value != 0.0;
    m->prepared = 0;
    return QCE_OK;
  }
  if (option == QCE_OPT_RESERVE_CUS) {
    if (value < 0.0 || value != floor(value)) return qce_set_error(QCE_EARG, "reserve_cus must be an integer >= 0");
    m->reserve_cus = value > 1e6 ? 1000000 : (int)value;
    m->reserve_set = 1;
    return QCE_OK;
  }
  if (option == QCE_OPT_PRECISION) {
    if (value != QCE_PRECISION_F64 && value != QCE_PRECISION_FAST && value != QCE_PRECISION_INT8)
      return qce_set_error(QCE_EARG, "unknown precision");
    m->precision = (int)value;
    m->prepared = 0;
    return QCE_OK;
  }
  if (option == QCE_OPT_FOURIER_PILOTS) {
    m->fourier_pilots = value != 0.0;
    m->prepared = 0;
    return QCE_OK;
  }
  if (option == QCE_OPT_INT8_SLICES) {
    if (!(value >= 3.0 && value <= 8.0) || value != floor(value))
      return qce_set_error(QCE_EARG, "int8 slices must be an integer in 3..8");
    m->int8_slices = (int)value;
    m->prepared = 0;
    return QCE_OK;
  }
  return qce_set_error(QCE_EARG, "unknown option");
}

int qce_synchronize(qce_model* m) {
  if (!m) return qce_set_error(QCE_EARG, "null model");
  DeviceGuard g(m->device);
  HIPCHK(hipStreamSynchronize(m->stream));
  return check_status(m, true);
}

}  // extern "C"
