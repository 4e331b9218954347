// Training side of the VAE-parameterised Bussgang estimator: the part of a training step between the network's
// layers and around them (reference estimators/vae.py:280-281 reparameterisation, :312-365 vae_loss).
//
//   k_vae_sample      z = mu + exp(s) eps                         enc (B, 2L) = [mu | s], eps supplied or drawn
//   k_vae_sample_bwd  g_mu = g_z, g_s = g_z exp(s) eps            into one (B, 2L) gradient of enc
//   k_vae_elbo        row ELBO l_b (FP64) and, in the same pass, the gradient of the loss -mean_b l_b with respect to
//                     dec (B, N) and its direct (KL) part with respect to enc, both with the factor 1 / B, float32
//
// Row ELBO, with v = dec row b, t = [tr | ti] target row index[b] (or b), a_n = tr_n^2 + ti_n^2:
//   KL part      sum_l s_l - 1/2 sum_l mu_l^2 - 1/2 sum_l exp(2 s_l)
//   mode 0       sum_n v_n - sum_n exp(v_n) a_n                                    ('genie' / 'noisy', :345-349)
//   mode 1       c_n = exp(-v_n) + s2, s2 = 10^(-snr / 10), cbar = mean_n c_n      ('real', :322-342)
//                finite bits: delta = sqrt((1 + s2) / 2) step, m_i = i - 2^(bits - 1),
//                  g = k2 cbar^(-1/2) sum_i exp(-delta^2 m_i^2 / cbar), k2 = float(delta) / sqrt(float(pi)) (the
//                  reference's float32 constant, uniform_quantizer.py:101-111), beta = clamp(g^2, 0, 1),
//                  c'_n = beta c_n + (1 - beta) cbar; no quantiser: c' = c
//                sum_n (-log c'_n - a_n / c'_n)
// Gradient of mode 1, q_n = -1 / c'_n + a_n / c'_n^2:
//   g'     = -g / (2 cbar) + k2 cbar^(-1/2) sum_i exp(-delta^2 m_i^2 / cbar) delta^2 m_i^2 / cbar^2
//   beta'  = 2 g g' where g^2 <= 1, else 0 (torch.clamp passes the gradient at the bound)
//   dl/dc_m = beta q_m + [(1 - beta) sum_n q_n + beta' sum_n q_n (c_n - cbar)] / N
//   dloss/dv_m = dl/dc_m exp(-v_m) / B
//
// Arithmetic: inputs widened to FP64; exp, log, sums and gradients in FP64; one rounding to float32 at the store.
// The row math (elbo_row) and the eps draw live in qce_vae_row_dev.h, which k_vae_step (qce_vae_step.hip) includes too.
//
// Layout of k_vae_elbo: a row lives in a group of G = min(N, 64) lanes of one wave (four rows per wave at N = 16, two
// at N = 32, the whole wave from N = 64), lane j holding the E = N / G consecutive elements j E .. j E + E - 1 in
// registers (E = 2 at N = 128, 4 at N = 256), loaded as one 4 E-byte vector per array (16 bytes at N = 256; below
// that a lane owns fewer than four floats, and a wave's lanes together still read a contiguous span).  The latent
// part walks l = j, j + G, ...; the gain sum's 2^bits - 1 terms are spread over the group's lanes the same way.  All
// row sums are xor butterflies within the group: every lane ends with the same bits, in an order that depends on
// nothing but N, L and the bit count, so equal inputs give equal outputs on every call.  No LDS, no atomics; the mean
// over rows is left to the caller on the FP64 `rows`.
//
// Draws of k_vae_sample: Philox4x32-10 keyed by `seed` in a domain of its own; element (b, l) uses counter
// (row_offset + b) L + l, so rows generated in pieces equal the one-shot rows.  eps = sqrt(-2 log u1) cos(2 pi u2) in
// FP64 from two 53-bit uniforms, rounded to float32; z is formed from that float32 value, which is also what the
// backward reads.
#include "qce_common.h"
#include "qce_kernels.h"
#include "qce_vae_row_dev.h"

namespace {

using namespace qce_vae_row;  // the row math and the eps draw, shared with k_vae_step

constexpr int VT_THREADS = 256;
constexpr int VT_MAX_BLOCKS = 4096;  // the element-wise kernels walk the rest grid-stride

__global__ __launch_bounds__(VT_THREADS) void k_vae_sample(const float* __restrict__ enc, const float* __restrict__ eps_in,
                                                           long long B, int L, unsigned long long seed,
                                                           unsigned long long row_offset, float* __restrict__ z,
                                                           float* __restrict__ eps_out) {
  const long long n = B * L, stride = (long long)gridDim.x * VT_THREADS;
  for (long long i = (long long)blockIdx.x * VT_THREADS + threadIdx.x; i < n; i += stride) {
    const long long b = i / L;
    const int l = (int)(i - b * L);
    const float* er = enc + b * 2 * L;
    const float e = eps_in ? eps_in[i]
                           : (float)eps_draw(seed, (row_offset + (unsigned long long)b) * (unsigned long long)L + (unsigned)l);
    z[i] = (float)((double)er[l] + exp((double)er[L + l]) * (double)e);
    if (eps_out) eps_out[i] = e;
  }
}

__global__ __launch_bounds__(VT_THREADS) void k_vae_sample_bwd(const float* __restrict__ enc, const float* __restrict__ eps,
                                                               const float* __restrict__ gz, long long B, int L,
                                                               float* __restrict__ g_enc) {
  const long long n = B * L, stride = (long long)gridDim.x * VT_THREADS;
  for (long long i = (long long)blockIdx.x * VT_THREADS + threadIdx.x; i < n; i += stride) {
    const long long b = i / L;
    const int l = (int)(i - b * L);
    const float g = gz[i];
    g_enc[b * 2 * L + l] = g;
    g_enc[b * 2 * L + L + l] = (float)((double)g * exp((double)enc[b * 2 * L + L + l]) * (double)eps[i]);
  }
}

// G lanes per row, E elements per lane (N = G E); MODE 0: genie / noisy, 1: real.
template <int G, int E, int MODE>
__global__ __launch_bounds__(VT_THREADS) void k_vae_elbo(QceVaeElboArgs a) {
  constexpr int RPB = VT_THREADS / G;  // rows per workgroup
  constexpr int N = G * E;
  const int tid = threadIdx.x, j = tid & (G - 1);
  const long long row = (long long)blockIdx.x * RPB + tid / G;
  const bool live = row < a.B;
  const long long b = live ? row : a.B - 1;  // lanes past the batch redo the last row and store nothing
  long long tb = b;
  if (a.index) {
    const int ix = a.index[b];  // device-side indices cannot be checked on the host
    tb = ix < 0 ? 0 : (ix >= a.T ? a.T - 1 : ix);
  }
  const int L = a.L;
  const RealConst rc{a.n_bits, a.step, a.sqrt_pi_f};
  const float* t = a.t + tb * 2 * N;
  const double acc = elbo_row<G, E, MODE>(j, live, L, (double)a.B, a.enc + b * 2 * L, a.g_enc + b * 2 * L, a.dec + b * N, t,
                                          t + N, MODE == 1 ? a.snr + tb : nullptr, rc, a.g_dec + b * N);
  if (live && j == 0) a.rows[b] = acc;
}

unsigned ew_grid(long long n) {
  const long long g = (n + VT_THREADS - 1) / VT_THREADS;
  return (unsigned)(g < VT_MAX_BLOCKS ? g : VT_MAX_BLOCKS);
}

template <int G, int E>
void launch_elbo(const QceVaeElboArgs& a, hipStream_t st) {
  const long long rpb = VT_THREADS / G;
  const dim3 grid((unsigned)((a.B + rpb - 1) / rpb)), block(VT_THREADS);
  if (a.mode == 0) hipLaunchKernelGGL((k_vae_elbo<G, E, 0>), grid, block, 0, st, a);
  else hipLaunchKernelGGL((k_vae_elbo<G, E, 1>), grid, block, 0, st, a);
}

}  // namespace

bool qce_vae_train_shape(int N, int L) {
  return (N == 16 || N == 32 || N == 64 || N == 128 || N == 256) && L >= 1 && L <= QCE_VAE_MAX_LATENT;
}

hipError_t qce_launch_vae_sample(const float* enc, const float* eps_in, long long B, int L, unsigned long long seed,
                                 unsigned long long row_offset, float* z, float* eps_out, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vae_sample, dim3(ew_grid(B * L)), dim3(VT_THREADS), 0, st, enc, eps_in, B, L, seed, row_offset,
                     z, eps_out);
  return hipGetLastError();
}

hipError_t qce_launch_vae_sample_bwd(const float* enc, const float* eps, const float* gz, long long B, int L,
                                     float* g_enc, hipStream_t st) {
  if (B <= 0) return hipSuccess;
  if (L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_vae_sample_bwd, dim3(ew_grid(B * L)), dim3(VT_THREADS), 0, st, enc, eps, gz, B, L, g_enc);
  return hipGetLastError();
}

hipError_t qce_launch_vae_elbo(const QceVaeElboArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  if (!qce_vae_train_shape(a.N, a.L) || a.T < 1 || a.n_bits < 0 || a.n_bits > 8) return hipErrorInvalidValue;
  if ((a.B + 3) / 4 > 0x7fffffffLL) return hipErrorInvalidValue;  // grid.x
  switch (a.N) {
    case 16: launch_elbo<16, 1>(a, st); break;
    case 32: launch_elbo<32, 1>(a, st); break;
    case 64: launch_elbo<64, 1>(a, st); break;
    case 128: launch_elbo<64, 2>(a, st); break;
    default: launch_elbo<64, 4>(a, st); break;
  }
  return hipGetLastError();
}
