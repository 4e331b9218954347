// Row math of the VAE training loss, shared by k_vae_elbo (qce_vae_train.hip) and k_vae_step (qce_vae_step.hip): the
// row ELBO of one sample in FP64 and its analytic gradient (formulas at the head of qce_vae_train.hip), and the Philox
// draw of eps.  A row lives in a group of G lanes of one wave, lane j holding the E consecutive elements
// j E .. j E + E - 1 (N = G E); all row sums are xor butterflies within the group, so every lane ends with the same
// bits in an order that depends on nothing but N, L and the bit count.  The pointers may be global memory or LDS.
#pragma once
#include "qce_common.h"
#include "qce_observe_dev.h"

namespace qce_vae_row {

using namespace qce_obs;

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

// The constants of the 'real' loss (MODE 1): n_bits 1..8 or 0 (no quantiser), the standard uniform step, float32 sqrt(pi)
struct RealConst {
  int n_bits;
  double step;
  float sqrt_pi_f;
};

// The row ELBO of one row, returned in every lane of its group; with `live`, the gradient of -mean_b l_b is stored:
// ge[0 .. 2L) the KL part with respect to the encoder output er = [mu | s], g_dec[0 .. N) with respect to the decoder
// output dec, both times 1 / Bd, rounded to float32 once.  tr / ti: the target row's real and imaginary halves;
// snr: its SNR entry (MODE 1 only).  j: the lane's place in the group.  MODE 0: genie / noisy, 1: real.
template <int G, int E, int MODE>
QCE_DEV double elbo_row(int j, bool live, int L, double Bd, const float* er, float* ge, const float* dec, const float* tr_p,
                        const float* ti_p, const double* snr, const RealConst rc, float* g_dec) {
  constexpr int N = G * E;
  // latent part
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
  load_vec<E>(dec + j * E, v);
  load_vec<E>(tr_p + j * E, tr);
  load_vec<E>(ti_p + j * E, ti);
  if (MODE == 0) {
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const double an = tr[k] * tr[k] + ti[k] * ti[k];
      const double ea = exp(v[k]) * an;
      acc += v[k] - ea;
      gv[k] = -(1.0 - ea) / Bd;
    }
  } else {
    const double s2 = pow(10.0, -*snr / 10.0);
    double c[E], ev[E], csum = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      ev[k] = exp(-v[k]);
      c[k] = ev[k] + s2;
      csum += c[k];
    }
    const double cbar = group_sum<G>(csum) / (double)N;
    double beta = 1.0, dbeta = 0.0;
    if (rc.n_bits > 0) {
      const double delta = sqrt((1.0 + s2) / 2.0) * rc.step;
      const double k2 = (double)((float)delta / rc.sqrt_pi_f);
      const int nterm = (1 << rc.n_bits) - 1, half = 1 << (rc.n_bits - 1);
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
      const double cp = rc.n_bits > 0 ? beta * c[k] + (1.0 - beta) * cbar : c[k];
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
  if (live) store_vec<E>(g_dec + j * E, gv);
  return acc;
}

}  // namespace qce_vae_row
