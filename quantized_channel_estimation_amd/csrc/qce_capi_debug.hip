// Diagnostic exports: the raw digit-plane sums of the int8 kernel, and in the QCE_STAMPS build (libqce_stamps.so) the
// per-wave segment cycle counters of the Fourier and
// FP64 kernels.
#include "qce_capi.h"

extern "C" int qce_debug_i8_products(qce_model* m, const double* y, int64_t B, int k, double* raw_L, double* raw_W,
                                     int* exps) {
  int rc = check_model(m, true);
  if (rc) return rc;
  if (m->backend != QCE_BE_INT8) return qce_set_error(QCE_ESTATE, "the model is not prepared onto the int8 kernel");
  if (B < 0 || k < 0 || k >= m->K || (B > 0 && !y)) return qce_set_error(QCE_EARG, "bad arguments");
  DeviceGuard g(m->device);
  hipStream_t st = m->stream;
  const size_t RL = 2 * (size_t)m->MP, RW = 2 * (size_t)m->NP;
  if (B > 0 && (raw_L || raw_W)) {
    StreamScratch scr(st);
    double2* dy = nullptr;
    double *dL = nullptr, *dW = nullptr;
    HIPCHK(scr.get(reinterpret_cast<void**>(&dy), sizeof(double2) * (size_t)B * m->M));
    HIPCHK(scr.get(reinterpret_cast<void**>(&dL), sizeof(double) * (size_t)B * RL));
    HIPCHK(scr.get(reinterpret_cast<void**>(&dW), sizeof(double) * (size_t)B * RW));
    HIPCHK(hipMemcpyAsync(dy, y, sizeof(double2) * (size_t)B * m->M, hipMemcpyHostToDevice, st));
    if ((rc = run_i8_debug(m, dy, B, k, dL, dW, st))) return rc;
    if (raw_L) HIPCHK(hipMemcpyAsync(raw_L, dL, sizeof(double) * (size_t)B * RL, hipMemcpyDeviceToHost, st));
    if (raw_W) HIPCHK(hipMemcpyAsync(raw_W, dW, sizeof(double) * (size_t)B * RW, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  if (exps) {
    HIPCHK(hipMemcpyAsync(exps, m->i8_exps.p + (size_t)k * (RL + RW), sizeof(int) * (RL + RW), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return check_status(m, true);
}

#ifdef QCE_STAMPS
unsigned long long* g_f64_stamps = nullptr;  // set by run_f64 (qce_capi_estimate.hip)
long long g_f64_stamp_records = 0;

hipError_t qce_fft_set_stamps(unsigned long long* dev);
// diagnostic build only: stamp buffer of k_fft_wave (n 64-bit words on the device; n = 0 frees it) and
// its readback (8 segment cycle sums per wave of the launches since the last call with n > 0)
extern "C" int qce_debug_fft_stamps(unsigned long long* out, long long n) {
  static unsigned long long* d = nullptr;
  static long long cap = 0;
  if (n <= 0) {
    if (d) (void)hipFree(d);
    d = nullptr;
    cap = 0;
    return qce_fft_set_stamps(nullptr) == hipSuccess ? 0 : QCE_EHIP;
  }
  if (!d) {
    if (hipMalloc(&d, sizeof(unsigned long long) * n) != hipSuccess) return QCE_EHIP;
    cap = n;
    if (hipMemset(d, 0, sizeof(unsigned long long) * n) != hipSuccess) return QCE_EHIP;
    if (qce_fft_set_stamps(d) != hipSuccess) return QCE_EHIP;
    return 0;
  }
  if (n > cap) n = cap;
  if (hipDeviceSynchronize() != hipSuccess) return QCE_EHIP;
  if (hipMemcpy(out, d, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess) return QCE_EHIP;
  return (int)n;
}
// diagnostic build only: per-wave segment cycles (8 per wave) of the last k_est_all_f64 launch
extern "C" int qce_debug_f64_stamps(unsigned long long* out, long long n) {
  if (!g_f64_stamps) return QCE_ESTATE;
  if (n > g_f64_stamp_records * 8) n = g_f64_stamp_records * 8;
  if (hipDeviceSynchronize() != hipSuccess) return QCE_EHIP;
  if (hipMemcpy(out, g_f64_stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost) != hipSuccess) return QCE_EHIP;
  return (int)n;
}
#endif
