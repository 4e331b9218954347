// LDS radix-2 transforms and per-SNR scalar helpers shared by the Fourier-domain units (qce_fft.hip: A = I;
// qce_fft_pilot.hip: A = kron(x, I_N)): twiddles, fft_axis / fft2 over a tile of rows held in LDS, the Bussgang
// gain of one diagonal entry, and the phases of the 2-D DFT.
#pragma once
#include "qce_common.h"

#define QCE_NEG_INF (-__builtin_inf())

namespace {

constexpr double PI_D = 3.14159265358979323846;

QCE_DEV int ilog2(int v) { return 31 - __clz(v); }

QCE_DEV int bitrev(int j, int lg) { return (int)(__brev((unsigned)j) >> (32 - lg)) & ((1 << lg) - 1); }

// e^{-2 pi i t / 256}, t < 128, into LDS (every power-of-two length <= 256 indexes it with a stride)
QCE_DEV void twiddles(double2* tw) {
  for (int t = threadIdx.x; t < 128; t += blockDim.x) {
    double s, c;
    sincospi(-(double)t / 128.0, &s, &c);
    tw[t] = make_double2(c, s);
  }
}

// In-place radix-2 DIT FFT along one axis of every row of a TS x N tile (row stride N): the axis has
// length L and element stride st; the other index ranges over N / L lines.  inv: e^{+}, unnormalised.
// Rows sit RS elements apart in LDS; RS = N + 1 by default (16-B elements: consecutive rows start 4 banks apart,
// so a wave reading one element of 16 different rows is conflict-free).
QCE_DEV void fft_axis(double2* T, int TS, int N, int L, int st, bool inv, const double2* tw, int RS) {
  if (L <= 1) return;
  const int lg = ilog2(L), lgN = ilog2(N);
  const int nthr = blockDim.x;
  auto at = [&](int s, int line, int j) -> int {  // element (line, j) of row s
    return s * RS + (st == 1 ? (line << lg) + j : line + j * st);
  };
  for (int e = threadIdx.x; e < TS * N; e += nthr) {
    const int s = e >> lgN, q = e & (N - 1);
    const int line = q >> lg, j = q & (L - 1);
    const int r = bitrev(j, lg);
    if (j < r) {
      const int a = at(s, line, j), b = at(s, line, r);
      const double2 u = T[a];
      T[a] = T[b];
      T[b] = u;
    }
  }
  __syncthreads();
  const int hN = N >> 1, lgh = lgN - 1;
  for (int len = 2; len <= L; len <<= 1) {
    const int half = len >> 1, lgl = ilog2(len), wstride = 256 >> lgl;
    for (int e = threadIdx.x; e < TS * hN; e += nthr) {
      const int s = e >> lgh, q = e & (hN - 1);
      const int line = q >> (lg - 1), bt = q & ((L >> 1) - 1);
      const int blk = bt >> (lgl - 1), t = bt & (half - 1);
      const int j0 = (blk << lgl) + t;
      const int a = at(s, line, j0), b = at(s, line, j0 + half);
      double2 w = tw[t * wstride];
      if (inv) w.y = -w.y;
      const double2 u = T[a], v = cmul(T[b], w);
      T[a] = cadd(u, v);
      T[b] = csub(u, v);
    }
    __syncthreads();
  }
}

// 2-D DFT over (n1, n2), index i = i1 n2 + i2 (kron(F_n1, F_n2) order); n1 = 1 is the 1-D DFT
QCE_DEV void fft2(double2* T, int TS, int N, int n1, int n2, bool inv, const double2* tw, int RS) {
  fft_axis(T, TS, N, n2, 1, inv, tw, RS);
  fft_axis(T, TS, N, n1, n2, inv, tw, RS);
}
QCE_DEV void fft2(double2* T, int TS, int N, int n1, int n2, bool inv, const double2* tw) {
  fft2(T, TS, N, n1, n2, inv, tw, N + 1);
}

// Bussgang gain of a diagonal entry d (same formulas as k_gain_cr, qce_prepare.hip)
QCE_DEV double bussgang_gain(double d, int kind, int n_bits, int quant_kind, double delta, const double* thr,
                             const double* lab) {
  if (kind == 0) return sqrt(2.0 / PI_D) * (1.0 / sqrt(d));
  if (kind == 2) return 1.0;
  if (quant_kind == 0) {
    const int L = 1 << n_bits;
    double dinv = 1.0 / d, acc = 0.0;
    for (int q = 1; q < L; ++q) {
      const double o = (double)q - (double)L / 2.0;
      acc += exp(-delta * delta * (o * o) * dinv);
    }
    return acc * (delta / sqrt(PI_D) / sqrt(d));
  }
  if (quant_kind == 1) {
    const int L = 1 << n_bits;
    const double dinv = 1.0 / d;
    double acc = -lab[0] * exp(-thr[0] * thr[0] * dinv);
    acc += lab[L - 1] * exp(-thr[L - 2] * thr[L - 2] * dinv);
    for (int q = 1; q < L - 1; ++q) acc += lab[q] * (exp(-thr[q - 1] * thr[q - 1] * dinv) - exp(-thr[q] * thr[q] * dinv));
    return acc / (sqrt(PI_D) * sqrt(d));
  }
  return 0.0;
}

// phase index of the 2-D DFT term e^{-2 pi i <i, m>}: (i1 m1 / n1 + i2 m2 / n2) in units of 1/N
QCE_DEV int dft_phase(int i, int m, int n1, int n2) {
  const int i1 = i / n2, i2 = i % n2, m1 = m / n2, m2 = m % n2;
  const int N = n1 * n2;
  return ((i1 * m1 % n1) * n2 + (i2 * m2 % n2) * n1) % N;  // (i1 m1/n1 + i2 m2/n2) N mod N
}

QCE_DEV double2 unit_root(int p, int N) {  // e^{-2 pi i p / N}
  double s, c;
  sincospi(-2.0 * (double)p / (double)N, &s, &c);
  return make_double2(c, s);
}

}  // namespace
