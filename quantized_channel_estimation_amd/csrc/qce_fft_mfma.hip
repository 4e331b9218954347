// MFMA Fourier-domain 'all' / K-shard-partial estimate for (block-)circulant mixtures with A = I
// (the per-bin algebra is derived in qce_fft.hip's header).
//
// Per estimate (zero mean): Y = DFT(y); lp_k = c'_k - sum_i |Y_i|^2 rinv_ik; gamma = softmax(lp);
// f_i = sum_k gamma_k w_ki; h = IDFT(Y . f (+ sum_k gamma_k bb_ki)).  The two K x N products are the
// whole of the arithmetic (4 K N flops per estimate) and run here on v_mfma_f64_16x16x4_f64, so the
// result keeps the FP64 accuracy of the reference (gmm_cplx_bussgang.py computes in complex128).
//
// Kernels (dispatch by N in qce_launch_fft_mfma; one *_kernel.h and one unit each, helpers in qce_fft_dev.h):
//   k_fft_wave      N = 16, 32: persistent one-wave tiles, wave-local LDS transform; <HM> means  (qce_fft_wave_kernel.h)
//   k_fft_wreg      N = 64: persistent one-wave tiles, register transform (pass 1 / LDS exchange / pass 2); <HM> means
//                   (qce_fft_wreg_kernel.h)
//   k_fft_chunk     zero-mean N = 128, 256: components split over the waves for lp / softmax, bins for the filter,
//                   two barriers per 128-component chunk; register transform for N = 256  (qce_fft_chunk_kernel.h)
//   k_fft_chunk_hm  N = 128, 256 with means: k_fft_chunk's split, spectra kept in the LDS tile, 3x the MFMAs
//                   (qce_fft_chunk_hm_kernel.h)
// On gfx950 FP64 VALU instructions and FP64 MFMAs share the SIMD's issue budget (tools/probe/f64_pipe_probe.hip),
// so the kernels are organised around few VALU instructions per MFMA.  This unit holds the table pack they share
// (k_fft_pack) and the entry points.
#include "qce_fft_dev.h"

namespace {

// natural-order per-bin tables of k_fft_prep -> the kernels' storage order (bit-reversed per axis), negated rinv,
// components padded to Kp (padding: c' = -inf, zero tables), in the fragment order the kernels load: a lane's
// operands for two consecutive MFMAs are one 16-byte load,
//   lp  table: [cb][t/2][lane][t&1] = -rinv[bin p_lp(t, lane/16)][comp 16cb + lane%16]        t < N/4
//   filter   : [cb][j/2][lane][j&1] = w[comp 16cb + lane/16 + 4r][bin p_f(t, lane%16)]        j = r N/16 + t
// with the storage positions p_lp, p_f of the kernel that serves N (layout below)
__global__ __launch_bounds__(256) void k_fft_pack(int N, int lg1, int lg2, int K, int Kp, int has_mean,
                                                  const double* __restrict__ rinvT, const double2* __restrict__ uT,
                                                  const double* __restrict__ cprime, const double* __restrict__ wT,
                                                  const double2* __restrict__ bT, double* __restrict__ pr,
                                                  double* __restrict__ pur, double* __restrict__ pui,
                                                  double* __restrict__ pc, double* __restrict__ pw,
                                                  double* __restrict__ pbr, double* __restrict__ pbi) {
  const int n2m = (1 << lg2) - 1;
  auto bin_of = [&](int p) { return (brev(p >> lg2, lg1) << lg2) | brev(p & n2m, lg2); };
  const long long total = (long long)N * Kp;
  // table layouts: 1 at N = 256 (k_fft_chunk<256> / k_fft_chunk_hm<256>: lp bins 4 t + k, filter bins chunk256_bin),
  // 2 at N = 64 (k_fft_wreg: lp bins 16 k + t, filter bins chunk256_bin), 0 otherwise (k_fft_wave, the N = 128 chunk
  // kernels: lp bins 4 t + k, filter bins 16 t + row)
  const int layout = (N == 256) ? 1 : (N == 64) ? 2 : 0;
  // e = ((cb Q + i) 64 + lane) 2 + s, Q = N / 8 16-byte loads per block and table
  const int Q = N / 8, NT = N / 16;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (long long)gridDim.x * blockDim.x) {
    const int s = (int)(e & 1), lane = (int)((e >> 1) & 63);
    const long long g = e >> 7;
    const int i = (int)(g % Q), cb = (int)(g / Q);
    const int j = 2 * i + s;
    {  // lp: t = j, bin 4t + lane/16, comp 16cb + lane%16
      const int p = (layout == 2) ? 16 * (lane >> 4) + j : 4 * j + (lane >> 4), k = 16 * cb + (lane & 15);
      const bool ok = k < K;
      const long long src = (long long)bin_of(p) * K + k;
      pr[e] = ok ? -rinvT[src] : 0.0;
      if (has_mean) {
        pur[e] = ok ? 2.0 * uT[src].x : 0.0;
        pui[e] = ok ? 2.0 * uT[src].y : 0.0;
      }
    }
    {  // filter: r = j / NT, t = j % NT; comp 16cb + lane/16 + 4r, bin 16t + lane%16
      const int r = j / NT, t = j % NT;
      const int k = 16 * cb + (lane >> 4) + 4 * r;
      const int p = (layout != 0) ? chunk256_bin(t, lane & 15) : 16 * t + (lane & 15);
      const bool ok = k < K;
      const long long src = (long long)k * N + bin_of(p);
      pw[e] = ok ? wT[src] : 0.0;
      if (has_mean) {
        pbr[e] = ok ? bT[src].x : 0.0;
        pbi[e] = ok ? bT[src].y : 0.0;
      }
    }
    if (e < Kp) pc[e] = e < K ? cprime[e] : -__builtin_inf();
  }
}

}  // namespace

bool qce_fft_mfma_shape(int N) { return N >= 16 && N <= 256 && (N & (N - 1)) == 0; }

int qce_fft_kpad(int K) { return (K + 15) & ~15; }

hipError_t qce_launch_fft_pack(const QceFftEstArgs& a, const double* rinvT, const double2* uT, const double* cprime,
                               const double* wT, const double2* bT, hipStream_t st) {
  const int lg1 = __builtin_ctz(a.n1), lg2 = __builtin_ctz(a.n2);
  const long long total = (long long)a.N * a.Kp;
  const int blocks = (int)((total + 255) / 256);
  hipLaunchKernelGGL(k_fft_pack, dim3(blocks), dim3(256), 0, st, a.N, lg1, lg2, a.K, a.Kp, a.has_mean, rinvT, uT,
                     cprime, wT, bT, const_cast<double*>(a.pr), const_cast<double*>(a.pur),
                     const_cast<double*>(a.pui), const_cast<double*>(a.pc), const_cast<double*>(a.pw),
                     const_cast<double*>(a.pbr), const_cast<double*>(a.pbi));
  return hipGetLastError();
}

hipError_t qce_launch_fft_mfma(const QceFftEstArgs& a, int out, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  switch (a.N) {
    case 16:
    case 32: return qce_fft_launch_wave(a, out, st);
    case 64: return qce_fft_launch_wreg(a, out, st);
    case 128:
    case 256: return a.has_mean ? qce_fft_launch_chunk_hm(a, out, st) : qce_fft_launch_chunk(a, out, st);
    default: return hipErrorInvalidValue;
  }
}

#ifdef QCE_STAMPS
// diagnostic build only: point every stamped kernel unit's buffer at dev (8 x 64-bit per wave; nullptr = off)
hipError_t qce_fft_wave_set_stamps(unsigned long long* dev);
hipError_t qce_fft_wreg_set_stamps(unsigned long long* dev);
hipError_t qce_fft_chunk_set_stamps(unsigned long long* dev);
hipError_t qce_fft_set_stamps(unsigned long long* dev) {
  hipError_t e = qce_fft_wave_set_stamps(dev);
  if (e == hipSuccess) e = qce_fft_wreg_set_stamps(dev);
  if (e == hipSuccess) e = qce_fft_chunk_set_stamps(dev);
  return e;
}
#endif
