// VAE-parameterised Bussgang LMMSE in the Fourier domain (reference estimators/vae.py:376-431 convert_dec_outputs
// with zeromean=True, and :368-369 lmmse), FP64.
//
// The decoder's conditional covariance is circulant, Ch = F^H diag(c) F with c = max(exp(-log_var), 1e-12) and F the
// unitary DFT, and the scripts' pilot matrix is A = kron(x, I_N) (P pilots).  Then every N x N block of
// Cy = A Ch A^H + s2 I is circulant: block (p, q) has first column x_p conj(x_q) t (+ s2 at m = 0 when p = q) with
// t = IDFT(c), and the diagonal of block p is the constant d_p = |x_p|^2 mean(c) + s2.  So
//   - the Bussgang gain is one scalar g_p per pilot block, A_eff acts as a_p = g_p x_p on block p;
//   - Cr keeps circulant blocks: 1 bit, the arcsine law entry-wise on the first columns; multi-bit,
//     b^2 Cy + (1 - b^2) diag(Cy) with b = clip(mean_p g_p, 0, 1); inf, Cy;
//   - per DFT bin k the P*N x P*N solve splits into a P x P Hermitian system  Lam_k z = (F y_p)_k,
//     Lam_k[p][q] = DFT of the first column of block (p, q) of Cr, and  (F h)_k = c_k sum_p conj(a_p) z_p.
// Multi-bit and inf need no transform for Lam_k (DFT(t) = c).  One estimate is O(P^2 N log N) instead of the dense
// route's O((P N)^3), and reads 16 P N + 4 N (or 8 N) bytes and writes 16 N.
//
// k_vae<P>: one workgroup (256 threads) per tile of TS samples held in LDS as rows of N complex values
// (row stride N + 1): P observation rows per sample, and for 1 bit P (P + 1) / 2 rows of Cr first columns and one row
// for t.  The transforms are radix-2 in LDS over all rows of the tile at once; the per-bin P x P Cholesky runs in
// registers, one (sample, bin) per thread and pass.  N = 16 puts four samples in a wave, N = 256 gives every thread
// one bin of one sample per pass; the loops are the same.
#include "qce_common.h"
#include "qce_kernels.h"

namespace {

QCE_DEV int v_ilog2(int v) { return 31 - __clz(v); }
QCE_DEV int v_bitrev(int j, int lg) { return (int)(__brev((unsigned)j) >> (32 - lg)); }
QCE_DEV double v_clamp1(double v) { return v > 1.0 ? 1.0 : (v < -1.0 ? -1.0 : v); }

// In-place radix-2 DIT FFT of rows r0 .. r0 + nr - 1 of every sample of the tile (unnormalised; inv: e^{+}).
// tw[t] = e^{-2 pi i t / 256}, t < 128.  Ends with a barrier.
QCE_DEV void v_fft_rows(double2* T, int TS, int NR, int r0, int nr, int N, int lgN, bool inv, const double2* tw) {
  const int RS = N + 1, rows = TS * nr, nthr = blockDim.x;
  for (int e = threadIdx.x; e < rows * N; e += nthr) {
    const int r = e >> lgN, j = e & (N - 1), rv = v_bitrev(j, lgN);
    if (j < rv) {
      double2* row = T + (size_t)((r / nr) * NR + r0 + r % nr) * RS;
      const double2 u = row[j];
      row[j] = row[rv];
      row[rv] = u;
    }
  }
  __syncthreads();
  const int hN = N >> 1;
  for (int len = 2; len <= N; len <<= 1) {
    const int half = len >> 1, lgl = v_ilog2(len), wstride = 256 >> lgl;
    for (int e = threadIdx.x; e < rows * hN; e += nthr) {
      const int r = e >> (lgN - 1), q = e & (hN - 1);
      const int blk = q >> (lgl - 1), t = q & (half - 1);
      const int j0 = (blk << lgl) + t;
      double2* row = T + (size_t)((r / nr) * NR + r0 + r % nr) * RS;
      double2 w = tw[t * wstride];
      if (inv) w.y = -w.y;
      const double2 u = row[j0], v = cmul(row[j0 + half], w);
      row[j0] = cadd(u, v);
      row[j0 + half] = csub(u, v);
    }
    __syncthreads();
  }
}

template <int P>
__global__ __launch_bounds__(256) void k_vae(QceVaeArgs a) {
  extern __shared__ double2 v_smem[];
  constexpr int NPAIR = P * (P + 1) / 2, PRM = 3 * P + 1;
  constexpr double HALF_PI = 1.57079632679489661923;
  constexpr double PIVOT_TOL = 8.0 * 2.220446049250313e-16;
  const int N = a.N, RS = N + 1, lgN = v_ilog2(N), TS = a.TS;
  const bool onebit = a.kind == 0;
  const int NR = P + (onebit ? NPAIR + 1 : 0);
  double2* tw = v_smem;                                       // 128
  double2* T = v_smem + 128;                                  // TS * NR rows
  double* cs = reinterpret_cast<double*>(T + (size_t)TS * NR * RS);  // TS x N spectra
  double* prm = cs + TS * N;                                  // TS x PRM: g_p, 1/sqrt(d_p), d_p, b^2
  const long long b0 = (long long)blockIdx.x * TS;
  const int tid = threadIdx.x, nthr = blockDim.x;

  for (int t = tid; t < 128; t += nthr) {
    double s, c;
    sincospi(-(double)t / 128.0, &s, &c);
    tw[t] = make_double2(c, s);
  }
  // spectrum c = max(exp(-log_var), 1e-12); samples past the batch compute on c = 1, y = 0 and store nothing
  for (int e = tid; e < TS * N; e += nthr) {
    const long long b = b0 + (e >> lgN);
    double v = 1.0;
    if (b < a.B) {
      const size_t idx = (size_t)b * N + (e & (N - 1));
      const double lv = a.lv_f32 ? (double)reinterpret_cast<const float*>(a.lv)[idx]
                                 : reinterpret_cast<const double*>(a.lv)[idx];
      v = exp(-lv);
      if (v < 1e-12) v = 1e-12;
    }
    cs[e] = v;
  }
  __syncthreads();
  // per-sample scalars, 16 lanes per sample: mean(c), d_p, g_p, b^2
  {
    const int grp = tid >> 4, gl = tid & 15;
    for (int s = grp; s < TS; s += nthr >> 4) {
      double acc = 0.0;
      for (int k = gl; k < N; k += 16) acc += cs[s * N + k];
      for (int o = 8; o; o >>= 1) acc += __shfl_xor(acc, o);
      const double mean = acc / (double)N;
      double gsum = 0.0;
      for (int p = 0; p < P; ++p) {
        const double d = (a.x[p].x * a.x[p].x + a.x[p].y * a.x[p].y) * mean + a.s2;
        const double isd = 1.0 / sqrt(d);
        double g = 1.0;
        if (a.kind == 0) g = a.k1 * isd;
        else if (a.kind == 1) {
          const int L = 1 << a.n_bits;
          const double dinv = 1.0 / d, nd2 = -a.delta * a.delta;
          double sum = 0.0;
          for (int i = 1 + gl; i < L; i += 16) {
            const double o = (double)i - (double)L / 2.0;
            sum += exp(nd2 * (o * o) * dinv);
          }
          for (int o = 8; o; o >>= 1) sum += __shfl_xor(sum, o);
          g = sum * (a.k2 / sqrt(d));
        }
        gsum += g;
        if (gl == 0) {
          prm[s * PRM + p] = g;
          prm[s * PRM + P + p] = isd;
          prm[s * PRM + 2 * P + p] = d;
        }
      }
      if (gl == 0) {
        double beta = gsum / (double)P;
        beta = beta < 0.0 ? 0.0 : (beta > 1.0 ? 1.0 : beta);
        prm[s * PRM + 3 * P] = beta * beta;
      }
    }
  }
  if (onebit) {
    for (int e = tid; e < TS * N; e += nthr)
      T[(size_t)((e >> lgN) * NR + P + NPAIR) * RS + (e & (N - 1))] = make_double2(cs[e], 0.0);
    __syncthreads();
    v_fft_rows(T, TS, NR, P + NPAIR, 1, N, lgN, true, tw);  // t = IDFT(c) (times N)
    // first columns of Cr's blocks by the arcsine law
    const double invN = 1.0 / (double)N;
    for (int e = tid; e < TS * N; e += nthr) {
      const int s = e >> lgN, m = e & (N - 1);
      const double2 t = cscale(T[(size_t)(s * NR + P + NPAIR) * RS + m], invN);
      const double* pr = prm + s * PRM;
      int pi = 0;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = p; q < P; ++q, ++pi) {
          double2 r;
          if (p == q && m == 0) {
            r = make_double2(a.k3 * HALF_PI, 0.0);
          } else {
            const double2 v = cmul(cmulc(a.x[p], a.x[q]), t);
            r = make_double2(a.k3 * asin(v_clamp1(v.x * pr[P + p] * pr[P + q])),
                             a.k3 * asin(v_clamp1(v.y * pr[P + p] * pr[P + q])));
          }
          T[(size_t)(s * NR + P + pi) * RS + m] = r;
        }
    }
  }
  // observations, pilot-major: y[b][p N + i]
  for (int e = tid; e < TS * P * N; e += nthr) {
    const int s = e / (P * N), r = e - s * (P * N);
    const long long b = b0 + s;
    T[(size_t)(s * NR + (r >> lgN)) * RS + (r & (N - 1))] =
        b < a.B ? a.y[(size_t)b * P * N + r] : make_double2(0.0, 0.0);
  }
  __syncthreads();
  v_fft_rows(T, TS, NR, 0, P + (onebit ? NPAIR : 0), N, lgN, false, tw);

  // per bin: Lam z = y~, h~ = c sum_p conj(a_p) z_p  (1 / N: the two unitary transforms)
  bool bad = false;
  for (int e = tid; e < TS * N; e += nthr) {
    const int s = e >> lgN, k = e & (N - 1);
    const double c = cs[e];
    const double* pr = prm + s * PRM;
    double2 L[P][P], z[P];
    if (onebit) {
      int pi = 0;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = p; q < P; ++q, ++pi) {
          const double2 v = T[(size_t)(s * NR + P + pi) * RS + k];
          L[q][p] = cconj(v);  // lower triangle: Lam[q][p] = conj(Lam[p][q])
        }
    } else {
      const double b2 = a.kind == 1 ? pr[3 * P] : 1.0;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) {
          double2 v = cscale(cmulc(a.x[p], a.x[q]), c);
          if (p == q) v.x += a.s2;
          v = cscale(v, b2);
          if (p == q) v.x += (1.0 - b2) * pr[2 * P + p];
          L[p][q] = v;
        }
    }
#pragma unroll
    for (int p = 0; p < P; ++p) z[p] = T[(size_t)(s * NR + p) * RS + k];
    // Cholesky Lam = L L^H in place (lower), then the two triangular solves
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double ajj = L[j][j].x;
      double d = ajj;
#pragma unroll
      for (int m = 0; m < j; ++m) d -= L[j][m].x * L[j][m].x + L[j][m].y * L[j][m].y;
      // a pivot within the rounding noise of its own subtraction counts as zero: an exactly singular bin must not
      // pass or fail by the last bit
      if (!(d > PIVOT_TOL * ajj)) bad = bad || (b0 + s < a.B);
      const double inv = 1.0 / sqrt(d);
      L[j][j] = make_double2(inv, 0.0);  // keeps 1 / l_jj
#pragma unroll
      for (int i = j + 1; i < P; ++i) {
        double2 v = L[i][j];
#pragma unroll
        for (int m = 0; m < j; ++m) v = csub(v, cmulc(L[i][m], L[j][m]));
        L[i][j] = cscale(v, inv);
      }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
      double2 v = z[i];
#pragma unroll
      for (int m = 0; m < i; ++m) v = csub(v, cmul(L[i][m], z[m]));
      z[i] = cscale(v, L[i][i].x);
    }
#pragma unroll
    for (int i = P - 1; i >= 0; --i) {
      double2 v = z[i];
#pragma unroll
      for (int m = i + 1; m < P; ++m) v = csub(v, cmul(cconj(L[m][i]), z[m]));
      z[i] = cscale(v, L[i][i].x);
    }
    double2 hk = make_double2(0.0, 0.0);
#pragma unroll
    for (int p = 0; p < P; ++p) hk = cadd(hk, cscale(cmul(cconj(a.x[p]), z[p]), pr[p]));
    T[(size_t)(s * NR) * RS + k] = cscale(hk, c / (double)N);
  }
  if (bad) atomicOr(a.status, 1);
  __syncthreads();
  v_fft_rows(T, TS, NR, 0, 1, N, lgN, true, tw);
  for (int e = tid; e < TS * N; e += nthr) {
    const long long b = b0 + (e >> lgN);
    if (b < a.B) a.h[(size_t)b * N + (e & (N - 1))] = T[(size_t)((e >> lgN) * NR) * RS + (e & (N - 1))];
  }
}

// LDS bytes of a tile of TS samples
size_t vae_lds(int N, int P, int onebit, int TS) {
  const int NR = P + (onebit ? P * (P + 1) / 2 + 1 : 0);
  return sizeof(double2) * (128 + (size_t)TS * NR * (N + 1)) + sizeof(double) * ((size_t)TS * N + (size_t)TS * (3 * P + 1));
}

template <int P>
hipError_t launch_vae_p(const QceVaeArgs& a0, hipStream_t st) {
  QceVaeArgs a = a0;
  const int onebit = a.kind == 0;
  int TS = 16;
  while (TS > 1 && vae_lds(a.N, P, onebit, TS) > QCE_VAE_LDS_BUDGET) TS >>= 1;
  const size_t lds = vae_lds(a.N, P, onebit, TS);
  a.TS = TS;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_vae<P>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const long long grid = (a.B + TS - 1) / TS;
  hipLaunchKernelGGL(k_vae<P>, dim3((unsigned)grid), dim3(256), lds, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t qce_launch_vae(const QceVaeArgs& a, hipStream_t st) {
  if (a.B <= 0) return hipSuccess;
  switch (a.P) {
    case 1: return launch_vae_p<1>(a, st);
    case 2: return launch_vae_p<2>(a, st);
    case 3: return launch_vae_p<3>(a, st);
    case 4: return launch_vae_p<4>(a, st);
  }
  return hipErrorInvalidValue;
}
