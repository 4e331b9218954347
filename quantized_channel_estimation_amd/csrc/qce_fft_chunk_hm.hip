// k_fft_chunk_hm instances (N = 128, 256 with means), compiled in parallel with the other MFMA Fourier kernels
#include "qce_fft_chunk_hm_kernel.h"

namespace {

template <int N>
hipError_t launch_chunk_hm_n(const QceFftEstArgs& a, int out, hipStream_t st) {
  switch (out) {
    case 0: return launch_chunk_hm<N, 0>(a, st);
    case 3: return launch_chunk_hm<N, 3>(a, st);
    case 4: return launch_chunk_hm<N, 4>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t qce_fft_launch_chunk_hm(const QceFftEstArgs& a, int out, hipStream_t st) {
  switch (a.N) {
    case 128: return launch_chunk_hm_n<128>(a, out, st);
    case 256: return launch_chunk_hm_n<256>(a, out, st);
    default: return hipErrorInvalidValue;
  }
}
