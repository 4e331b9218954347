// k_fft_wave instances (N = 16, 32), compiled in parallel with the other MFMA Fourier kernels
#include "qce_fft_wave_kernel.h"

namespace {

template <int N, int OUT>
hipError_t launch_wave_t(const QceFftEstArgs& a, hipStream_t st) {
  if (a.has_mean) return a.n1 == 1 ? launch_wave_c<N, OUT, true, true>(a, st) : launch_wave_c<N, OUT, true, false>(a, st);
  return a.n1 == 1 ? launch_wave_c<N, OUT, false, true>(a, st) : launch_wave_c<N, OUT, false, false>(a, st);
}

template <int N>
hipError_t launch_wave_n(const QceFftEstArgs& a, int out, hipStream_t st) {
  switch (out) {
    case 0: return launch_wave_t<N, 0>(a, st);
    case 3: return launch_wave_t<N, 3>(a, st);
    case 4: return launch_wave_t<N, 4>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t qce_fft_launch_wave(const QceFftEstArgs& a, int out, hipStream_t st) {
  switch (a.N) {
    case 16: return launch_wave_n<16>(a, out, st);
    case 32: return launch_wave_n<32>(a, out, st);
    default: return hipErrorInvalidValue;
  }
}
