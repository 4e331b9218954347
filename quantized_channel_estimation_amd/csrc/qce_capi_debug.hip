// Diagnostic exports of the QCE_STAMPS build (libqce_stamps.so): per-wave segment cycle counters of the Fourier and
// FP64 kernels.  Empty in the normal build.
#include "qce_capi.h"

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
