// Fourier-domain path with pilots, A = kron(x, I_N) (kernels: qce_fft_pilot_kernel.h): shape test and launchers.
#include "qce_fft_pilot_kernel.h"

int qce_fftp_kpad(int K) { return (K + 15) / 16 * 16; }

static long long fftp_lds_bytes(int N, int P, int Kp) {
  return 128LL * 16 + 16LL * P * (N + 1) * 16 + 16LL * (Kp + 1) * 8 + 512 * 8;
}

// 2 <= P <= 4 pilots, N a power of two in 16..256 (whole 16-bin blocks), P N <= 512, and the 16-observation tile
// (spectra of all segments + the lp tile) within the 160 KB of LDS
bool qce_fftp_shape(int N, int P, int K) {
  if (P < 2 || P > 4 || N < 16 || N > 256 || (N & (N - 1)) || P * N > 512 || K < 1) return false;
  return fftp_lds_bytes(N, P, qce_fftp_kpad(K)) <= 160 * 1024;
}

long long qce_fftp_tabl_doubles(int N, int P, int Kp, int has_mean) {
  return (long long)Kp * (P * P + (has_mean ? 2 * P : 0)) * N;
}
long long qce_fftp_tabw_doubles(int N, int P, int Kp, int has_mean) {
  return (long long)Kp * (2 * P + (has_mean ? 2 : 0)) * N;
}

hipError_t qce_launch_fftp_prep(const QceFftpPrepArgs& a, hipStream_t st) {
  switch (a.P) {
    case 2: hipLaunchKernelGGL(k_fftp_prep<2>, dim3(a.Kp), dim3(256), 0, st, a); break;
    case 3: hipLaunchKernelGGL(k_fftp_prep<3>, dim3(a.Kp), dim3(256), 0, st, a); break;
    case 4: hipLaunchKernelGGL(k_fftp_prep<4>, dim3(a.Kp), dim3(256), 0, st, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <int P, bool HM, int OUT>
static hipError_t launch_fftp_t(const QceFftpEstArgs& a, hipStream_t st) {
  static bool attr_set = false;  // raise the dynamic-LDS cap once per instance
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute((const void*)k_fftp_est<P, HM, OUT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       160 * 1024);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const long long lds = fftp_lds_bytes(a.N, P, a.Kp);
  if (lds > 160 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL((k_fftp_est<P, HM, OUT>), dim3((unsigned)((a.B + 15) / 16)), dim3(256), (size_t)lds, st, a);
  return hipGetLastError();
}

template <int P, bool HM>
static hipError_t launch_fftp_out(const QceFftpEstArgs& a, int out, hipStream_t st) {
  switch (out) {
    case 0: return launch_fftp_t<P, HM, 0>(a, st);
    case 1: return launch_fftp_t<P, HM, 1>(a, st);
    case 2: return launch_fftp_t<P, HM, 2>(a, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t qce_launch_fftp_est(const QceFftpEstArgs& a, int out, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  switch (a.P * 2 + (a.has_mean ? 1 : 0)) {
    case 4: return launch_fftp_out<2, false>(a, out, st);
    case 5: return launch_fftp_out<2, true>(a, out, st);
    case 6: return launch_fftp_out<3, false>(a, out, st);
    case 7: return launch_fftp_out<3, true>(a, out, st);
    case 8: return launch_fftp_out<4, false>(a, out, st);
    case 9: return launch_fftp_out<4, true>(a, out, st);
    default: return hipErrorInvalidValue;
  }
}
