// Device helpers shared by the observation kernels (qce_observe.hip, qce_observe_rows.hip) and, for the generator,
// the VAE training kernels (qce_vae_train.hip): the counter-based
// generator (Philox4x32-10 + Box-Muller in FP64) and the bit-exact quantiser of utils.py:189-203.
#pragma once
#include "qce_common.h"

namespace qce_obs {

constexpr double QUANT_1BIT = 0x1.6a09e667f3bccp-1;  // 1 / np.sqrt(2) as numpy rounds it (utils.py:191)
constexpr double SQRT_HALF = 0x1.6a09e667f3bcdp-1;   // np.sqrt(0.5) (crandn, utils.py:14)
// third counter word: one domain per kind of draw, so the streams of one seed never share a counter
constexpr uint32_t DOMAIN_NOISE = 0x51ED2701u;      // CN(0, 1) of complex element e
constexpr uint32_t DOMAIN_SNR_INDEX = 0x51ED2702u;  // the SNR index of row b (qce_observe_rows.hip)
constexpr uint32_t DOMAIN_VAE_EPS = 0x51ED2703u;    // N(0, 1) of latent element e (qce_vae_train.hip)

// Philox4x32-10 (Salmon et al., SC'11): counter (c0..c3), key (k0, k1)
QCE_DEV uint4 philox(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
    k.x += 0x9E3779B9u;
    k.y += 0xBB67AE85u;
  }
  return c;
}

// One circular complex normal sqrt(1/2) (n1 + j n2) for complex element index e of stream `seed`.
QCE_DEV double2 cn_draw(unsigned long long seed, unsigned long long e) {
  const uint4 r = philox(make_uint4((uint32_t)e, (uint32_t)(e >> 32), DOMAIN_NOISE, 0u),
                         make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  const unsigned long long a = ((unsigned long long)r.x << 32 | r.y) >> 11;  // 53 bits
  const unsigned long long b = ((unsigned long long)r.z << 32 | r.w) >> 11;
  const double u1 = (double)(a + 1) * 0x1.0p-53;  // (0, 1]
  const double u2 = (double)b * 0x1.0p-53;        // [0, 1)
  const double rad = sqrt(-2.0 * log(u1)) * SQRT_HALF;
  double sn, cs;
  sincospi(2.0 * u2, &sn, &cs);
  return make_double2(rad * cs, rad * sn);
}

// One uniform in [0, 1) (53 bits) for row index b of stream `seed`, in the SNR-index domain.
QCE_DEV double row_uniform(unsigned long long seed, unsigned long long b) {
  const uint4 r = philox(make_uint4((uint32_t)b, (uint32_t)(b >> 32), DOMAIN_SNR_INDEX, 0u),
                         make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
  return (double)(((unsigned long long)r.x << 32 | r.y) >> 11) * 0x1.0p-53;
}

// np.digitize(x, thr) for increasing thr (right=False): the number of thresholds <= x; NaN -> L - 1
QCE_DEV int digitize(double x, const double* thr, int nthr) {
  if (x != x) return nthr;
  int lo = 0, hi = nthr;  // first index with thr[i] > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (thr[mid] <= x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

QCE_DEV double npsign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }

// v = Ah + s * w, then the quantiser; kind 0: 1 bit, 1: multi-bit, 2: none
QCE_DEV double2 observe_one(double2 v, double2 w, double s, int noise, int kind, const double* thr,
                            const double* lab, int nthr) {
#pragma clang fp contract(off)
  if (noise) {
    const double nr = s * w.x - 0.0 * w.y;  // (s + 0j) * w, numpy's complex product
    const double ni = s * w.y + 0.0 * w.x;
    v.x = v.x + nr;
    v.y = v.y + ni;
  }
  if (kind == 0) {
    const double sr = npsign(v.x), si = npsign(v.y);
    return make_double2(QUANT_1BIT * sr - 0.0 * si, QUANT_1BIT * si + 0.0 * sr);
  }
  if (kind == 1) return make_double2(lab[digitize(v.x, thr, nthr)], lab[digitize(v.y, thr, nthr)]);
  return v;
}

QCE_DEV int r_bitrev(int j, int lg) { return (int)(__brev((unsigned)j) >> (32 - lg)); }

// The feature transform of qce_observe_rows.hip and qce_vae_net.hip (one definition: their features agree to the bit).
// In-place radix-2 DIT transform (unnormalised, e^{-}) of every row of the tile; tw[t] = e^{-2 pi i t / N}, t < N / 2.
// Starts from rows complete in LDS behind a barrier and ends with a barrier.
template <int THREADS>
QCE_DEV void r_fft_rows(double2* T, int G, int N, int lgN, const double2* tw) {
  const int RS = N + 1;
  for (int e = threadIdx.x; e < G * N; e += THREADS) {
    const int r = e >> lgN, j = e & (N - 1), rv = r_bitrev(j, lgN);
    if (j < rv) {
      double2* row = T + r * RS;
      const double2 u = row[j];
      row[j] = row[rv];
      row[rv] = u;
    }
  }
  __syncthreads();
  const int hN = N >> 1;
  for (int lgl = 1; lgl <= lgN; ++lgl) {
    const int half = 1 << (lgl - 1), wshift = lgN - lgl;
    for (int e = threadIdx.x; e < G * hN; e += THREADS) {
      const int r = e >> (lgN - 1), q = e & (hN - 1);
      const int blk = q >> (lgl - 1), t = q & (half - 1);
      const int j0 = (blk << lgl) + t;
      double2* row = T + r * RS;
      const double2 u = row[j0], v = cmul(row[j0 + half], tw[t << wshift]);
      row[j0] = cadd(u, v);
      row[j0 + half] = csub(u, v);
    }
    __syncthreads();
  }
}

}  // namespace qce_obs
