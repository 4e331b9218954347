// k_fft_wreg instances (N = 64), compiled in parallel with the other MFMA Fourier kernels
#include "qce_fft_wreg_kernel.h"

hipError_t qce_fft_launch_wreg(const QceFftEstArgs& a, int out, hipStream_t st) {
  switch (out) {
    case 0: return a.has_mean ? launch_wreg<0, true>(a, st) : launch_wreg<0, false>(a, st);
    case 3: return a.has_mean ? launch_wreg<3, true>(a, st) : launch_wreg<3, false>(a, st);
    case 4: return a.has_mean ? launch_wreg<4, true>(a, st) : launch_wreg<4, false>(a, st);
    default: return hipErrorInvalidValue;
  }
}
