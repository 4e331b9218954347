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
#include "qce_observe_dev.h"

namespace {

using namespace qce_obs;

constexpr int VT_THREADS = 256;
constexpr int VT_MAX_BLOCKS = 4096;  // the element-wise kernels walk the rest grid-stride

template <int G>
QCE_DEV double group_sum(double v) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, G);
  return v;
}

template <int E>
QCE_DEV void load_vec(const float* p, double (&o)[E]) {
  if constexpr (E == 4) {
    const float4 f = *reinterpret_cast<const float4*>(p);
    o[0] = f.x, o[1] = f.y, o[2] = f.z, o[3] = f.w;
  } else if constexpr (E == 2) {
    const float2 f = *reinterpret_cast<const float2*>(p);
    o[0] = f.x, o[1] = f.y;
  } else {
    o[0] = *p;
  }
}

template <int E>
QCE_DEV void store_vec(float* p, const double (&v)[E]) {
  if constexpr (E == 4) *reinterpret_cast<float4*>(p) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
  else if constexpr (E == 2) *reinterpret_cast<float2*>(p) = make_float2((float)v[0], (float)v[1]);
  else *p = (float)v[0];
}

// One standard normal for element counter e of stream `seed`.
QCE_DEV double eps_draw(unsigned long long seed, unsigned long long e) {
  const uint4 r = philox(make_uint4((uint32_t)e, (uint32_t)(e >> 32), DOMAIN_VAE_EPS, 0u),
                         make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const unsigned long long a = ((unsigned long long)r.x << 32 | r.y) >> 11;  // 53 bits
  const unsigned long long b = ((unsigned long long)r.z << 32 | r.w) >> 11;
  const double u1 = (double)(a + 1) * 0x1.0p-53;  // (0, 1]
  const double u2 = (double)b * 0x1.0p-53;        // [0, 1)
  return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

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
  const double Bd = (double)a.B;

  // latent part
  const float* er = a.enc + b * 2 * L;
  float* ge = a.g_enc + b * 2 * L;
  double acc = 0.0;
  for (int l = j; l < L; l += G) {
    const double mu = er[l], s = er[L + l];
    const double e2 = exp(2.0 * s);
    acc += s - 0.5 * mu * mu - 0.5 * e2;
    if (live) {
      ge[l] = (float)(mu / Bd);
      ge[L + l] = (float)(-(1.0 - e2) / Bd);
    }
  }

  // decoder part
  double v[E], tr[E], ti[E], gv[E];
  load_vec<E>(a.dec + b * N + j * E, v);
  load_vec<E>(a.t + tb * 2 * N + j * E, tr);
  load_vec<E>(a.t + tb * 2 * N + N + j * E, ti);
  if (MODE == 0) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const double an = tr[k] * tr[k] + ti[k] * ti[k];
      const double ea = exp(v[k]) * an;
      acc += v[k] - ea;
      gv[k] = -(1.0 - ea) / Bd;
    }
  } else {
    const double s2 = pow(10.0, -a.snr[tb] / 10.0);
    double c[E], ev[E], csum = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      ev[k] = exp(-v[k]);
      c[k] = ev[k] + s2;
      csum += c[k];
    }
    const double cbar = group_sum<G>(csum) / (double)N;
    double beta = 1.0, dbeta = 0.0;
    if (a.n_bits > 0) {
      const double delta = sqrt((1.0 + s2) / 2.0) * a.step;
      const double k2 = (double)((float)delta / a.sqrt_pi_f);
      const int nterm = (1 << a.n_bits) - 1, half = 1 << (a.n_bits - 1);
      const double d2 = delta * delta;
      double S = 0.0, S2 = 0.0;
      for (int i = 1 + j; i <= nterm; i += G) {
        const double m = (double)(i - half);
        const double w = d2 * m * m / cbar;
        const double e = exp(-w);
        S += e;
        S2 += e * w / cbar;
      }
      S = group_sum<G>(S);
      S2 = group_sum<G>(S2);
      const double rs = k2 / sqrt(cbar);
      const double g = rs * S;
      const double dg = -g / (2.0 * cbar) + rs * S2;
      const double g2 = g * g;
      beta = g2 > 1.0 ? 1.0 : g2;
      dbeta = g2 <= 1.0 ? 2.0 * g * dg : 0.0;
    }
    double q[E], sq = 0.0, sqc = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const double an = tr[k] * tr[k] + ti[k] * ti[k];
      const double cp = a.n_bits > 0 ? beta * c[k] + (1.0 - beta) * cbar : c[k];
      const double ic = 1.0 / cp;
      acc += -log(cp) - an * ic;
      q[k] = -ic + an * ic * ic;
      sq += q[k];
      sqc += q[k] * (c[k] - cbar);
    }
    sq = group_sum<G>(sq);
    sqc = group_sum<G>(sqc);
    const double common = ((1.0 - beta) * sq + dbeta * sqc) / (double)N;
#pragma unroll
    for (int k = 0; k < E; ++k) gv[k] = (beta * q[k] + common) * ev[k] / Bd;
  }
  acc = group_sum<G>(acc);
  if (live) {
    store_vec<E>(a.g_dec + b * N + j * E, gv);
    if (j == 0) a.rows[b] = acc;
  }
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
