// The two weighted statistics the covariance recovery from quantised samples rests on (reference
// cov_est_quant.py:31-88 est_cov_from_quant; gmm_cplx_quant.py:817, :915 call it on d = x - mu_k), formed from the
// resident X, R and mu_k in one device pass, with no transformed copy of the observations:
//   nk[k]             = sum_b r_bk + 10 eps                                   (the M-step's nk, qce_em.hip)
//   corr[k][i][j]     = sum_b r_bk s_i conj(s_j) / nk[k],  s = (sign Re d + j sign Im d) / sqrt 2     (:45-46)
//   probs[k][i][t][0] = sum_b r_bk 1(|Re d_i| < thr_t) / nk[k],  [1]: Im d_i                          (:65-69)
// d = x_b - mu_k is one FP64 subtraction per part, sign(0) = 0 (np.sign) and the indicator is strict, as the
// reference decides them.  Padding (features beyond N, samples beyond the chunk) enters as sign 0 / weight 0: it is
// masked before the subtraction, never formed as 0 - mu.
//
// k_qm_probs (bandwidth-bound, shaped like k_em_stats): thread = (sample group g, feature f); each x is loaded once
// for a block of components and all T thresholds; every (chunk, group) writes its own partial.
// k_qm_corr (FP64 MFMA, shaped like k_em_cov): work split by (component, sample chunk, 64 x 64 output block); A = r s
// and B = s are formed in registers from X, four real products per complex product.  The accumulators hold
// sum r (+-1)(+-1): the 1/2 of the two 1/sqrt 2 and the 1/nk are applied once in the final pass, so unweighted sums
// are exact integers.  Partials are summed in a fixed order: no atomics, bit-reproducible.
//
// Roofline: corr 8 K B N^2 FP64 flops on the MFMA pipe; probs reads X once per component block
// (16 B N ceil(K / KB) bytes) plus R (8 B K), and does 2 K T compares and adds per element.
#include "qce_capi.h"
#include "qce_common.h"

#pragma clang fp contract(off)

namespace {

constexpr double EPS10 = 10.0 * 2.220446049250313e-16;  // 10 * np.finfo(float64).eps, as qce_em.hip
constexpr int QM_CHUNK = 512;                             // samples per k_qm_probs workgroup
constexpr int QM_MAX_T = 15;

struct QmThr {
  double t[QM_MAX_T];
};

// np.sign on finite values: +-1.0 with v's sign bit, 0 for +-0 (one compare and two integer operations)
QCE_DEV double sgn(double v) {
  const int hi = (__double2hiint(v) & (int)0x80000000) | 0x3ff00000;
  return v != 0.0 ? __hiloint2double(hi, 0) : 0.0;
}

// per (block of KB components, sample chunk c, sample group g): sum r and sum r 1(|d| < thr_t) per feature.
// Partial slot = c G + g; pnk (slots, K), pp (slots, K, T, 2, N).
template <int NPAD, int KB, int TMAX>
__global__ __launch_bounds__(256) void k_qm_probs(long long B, int N, int K, int T, QmThr thr,
                                                  const double2* __restrict__ X, const double* __restrict__ R,
                                                  const double2* __restrict__ mean, double* __restrict__ pnk,
                                                  double* __restrict__ pp) {
  constexpr int G = 256 / NPAD;
  const int k0 = blockIdx.x * KB, c = blockIdx.y;
  const int f = threadIdx.x % NPAD, g = threadIdx.x / NPAD;
  const int nkb = K - k0 < KB ? K - k0 : KB;
  const long long b0 = (long long)c * QM_CHUNK;
  const long long b1 = b0 + QM_CHUNK < B ? b0 + QM_CHUNK : B;
  const bool live = f < N;
  double nk[KB], pr[KB][TMAX], pi[KB][TMAX];
  double2 mu[KB];
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    nk[j] = 0.0;
    mu[j] = (mean && live && j < nkb) ? mean[(long long)(k0 + j) * N + f] : make_double2(0.0, 0.0);
#pragma unroll
    for (int t = 0; t < TMAX; ++t) pr[j][t] = pi[j][t] = 0.0;
  }
  // unrolled so that the loads of the next samples are in flight while this one is compared (the adds keep
  // their order)
#pragma clang loop unroll_count(TMAX <= 3 ? 4 : 2)
  for (long long b = b0 + g; b < b1; b += G) {
    const double2 x = live ? X[b * N + f] : make_double2(0.0, 0.0);
#pragma unroll
    for (int j = 0; j < KB; ++j) {
      const double r = j < nkb ? (R ? R[b * K + k0 + j] : 1.0) : 0.0;
      nk[j] += r;
      const double ar = fabs(x.x - mu[j].x), ai = fabs(x.y - mu[j].y);
#pragma unroll
      for (int t = 0; t < TMAX; ++t) {
        if (t < T) {
          pr[j][t] += ar < thr.t[t] ? r : 0.0;
          pi[j][t] += ai < thr.t[t] ? r : 0.0;
        }
      }
    }
  }
  const long long slot = (long long)c * G + g;
#pragma unroll
  for (int j = 0; j < KB; ++j) {
    if (j >= nkb) continue;
    const long long o = slot * K + k0 + j;
    if (f == 0) pnk[o] = nk[j];
    if (!live) continue;
#pragma unroll
    for (int t = 0; t < TMAX; ++t) {
      if (t < T) {
        pp[((o * T + t) * 2 + 0) * N + f] = pr[j][t];
        pp[((o * T + t) * 2 + 1) * N + f] = pi[j][t];
      }
    }
  }
}

// fixed-order reduction over the S partial slots: nk and probs (K, N, T, 2).  Block = 64 elements x 4 strided
// quarters of the slots (slot s goes to quarter s % 4, summed in ascending s), combined as (q0 + q1) + (q2 + q3).
__global__ __launch_bounds__(256) void k_qm_probs_final(int S, int N, int K, int T, const double* __restrict__ pnk,
                                                        const double* __restrict__ pp, double* __restrict__ nk_out,
                                                        double* __restrict__ probs) {
  const int k = blockIdx.x, x = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int n = T * 2 * N;  // (t, part, feature): the partials' order, so the reads coalesce
  const int e = blockIdx.y * 64 + x;
  double a_nk = 0.0, a = 0.0;
#pragma unroll 8
  for (int s = q; s < S; s += 4) a_nk += pnk[(long long)s * K + k];
  if (e < n) {
#pragma unroll 8
    for (int s = q; s < S; s += 4) a += pp[((long long)s * K + k) * n + e];
  }
  __shared__ double red[2][4][64];
  red[0][q][x] = a_nk;
  red[1][q][x] = a;
  __syncthreads();
  if (q != 0) return;
  const double nk = ((red[0][0][x] + red[0][1][x]) + (red[0][2][x] + red[0][3][x])) + EPS10;
  if (blockIdx.y == 0 && x == 0) nk_out[k] = nk;
  if (e < n) {
    const double acc = (red[1][0][x] + red[1][1][x]) + (red[1][2][x] + red[1][3][x]);
    const int f = e % N, tp = e / N;
    probs[((long long)k * N + f) * T * 2 + tp] = acc / nk;
  }
}

// weighted sign-correlation partials on FP64 MFMA.  Block = 4 waves; output block (blockIdx.z) of 4 x 4 tiles of
// 16 x 16; wave w owns row tile 4 rb + w and the four column tiles 4 cb + t (the tiling of k_em_cov).
__global__ __launch_bounds__(256) void k_qm_corr(long long B, int N, int K, int NT, int chunk,
                                                 const double2* __restrict__ X, const double* __restrict__ R,
                                                 const double2* __restrict__ mean, double2* __restrict__ part) {
  const int k = blockIdx.x, c = blockIdx.y;
  const int ncb = (NT + 3) >> 2;
  const int rb = blockIdx.z / ncb, cb = blockIdx.z % ncb;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int rt = rb * 4 + w;
  if (rt >= NT) return;  // no barriers below
  const int i = lane & 15, kk = lane >> 4;
  const int fr = rt * 16 + i;
  int fc[4];
  bool cok[4];
  double2 muc[4];
  const double2* mk = mean ? mean + (long long)k * N : nullptr;
  const double2 mur = (mk && fr < N) ? mk[fr] : make_double2(0.0, 0.0);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    fc[t] = (cb * 4 + t) * 16 + i;
    cok[t] = cb * 4 + t < NT && fc[t] < N;
    muc[t] = (mk && cok[t]) ? mk[fc[t]] : make_double2(0.0, 0.0);
  }
  f64x4 re[4], im[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    re[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    im[t] = f64x4{0.0, 0.0, 0.0, 0.0};
  }
  const long long b0 = (long long)c * chunk;
  const long long b1 = b0 + chunk < B ? b0 + chunk : B;
  for (long long bs = b0; bs < b1; bs += 4) {
    const long long b = bs + kk;
    const bool ok = b < b1;
    const double r = ok ? (R ? R[b * K + k] : 1.0) : 0.0;
    const double2* xb = X + (ok ? b : 0) * N;
    double ar = 0.0, ai = 0.0;  // A = r s (row feature), 0 on padding
    if (ok && fr < N) {
      const double2 x = xb[fr];
      ar = r * sgn(x.x - mur.x);
      ai = r * sgn(x.y - mur.y);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (cb * 4 + t >= NT) continue;  // wave-uniform
      double sr = 0.0, si = 0.0;       // B = s (column feature)
      if (ok && cok[t]) {
        const double2 x = xb[fc[t]];
        sr = sgn(x.x - muc[t].x);
        si = sgn(x.y - muc[t].y);
      }
      re[t] = mfma16x16x4d(ar, sr, re[t]);
      re[t] = mfma16x16x4d(ai, si, re[t]);
      im[t] = mfma16x16x4d(ai, sr, im[t]);
      im[t] = mfma16x16x4d(-ar, si, im[t]);
    }
  }
  double2* pk = part + ((long long)c * K + k) * N * N;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (cb * 4 + t >= NT) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = rt * 16 + kk + 4 * q, col = (cb * 4 + t) * 16 + i;
      if (row < N && col < N) pk[(long long)row * N + col] = make_double2(re[t][q], im[t][q]);
    }
  }
}

// fixed-order reduction over chunks, then the 1/2 of s s^H and the 1/nk
__global__ __launch_bounds__(256) void k_qm_corr_final(int C, int N, int K, const double2* __restrict__ part,
                                                       const double* __restrict__ nk, double2* __restrict__ corr) {
  const long long n = (long long)K * N * N;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
    double2 s = make_double2(0.0, 0.0);
    for (int c = 0; c < C; ++c) s = cadd(s, part[(long long)c * n + e]);
    const double d = nk[e / ((long long)N * N)];
    corr[e] = make_double2(0.5 * s.x / d, 0.5 * s.y / d);
  }
}

template <int NPAD>
void launch_probs(long long B, int N, int K, int T, int C, const QmThr& thr, const double2* X, const double* R,
                  const double2* mean, double* pnk, double* pp, hipStream_t st) {
  // accumulators per thread: KB (1 + 2 TMAX) doubles
  if (T <= 3)
    hipLaunchKernelGGL((k_qm_probs<NPAD, 8, 3>), dim3((K + 7) / 8, C), dim3(256), 0, st, B, N, K, T, thr, X, R, mean,
                       pnk, pp);
  else if (T <= 7)
    hipLaunchKernelGGL((k_qm_probs<NPAD, 8, 7>), dim3((K + 7) / 8, C), dim3(256), 0, st, B, N, K, T, thr, X, R, mean,
                       pnk, pp);
  else
    hipLaunchKernelGGL((k_qm_probs<NPAD, 4, QM_MAX_T>), dim3((K + 3) / 4, C), dim3(256), 0, st, B, N, K, T, thr, X, R,
                       mean, pnk, pp);
}

}  // namespace

extern "C" int qce_quant_moments(const double* X, int64_t B, int N, int K, const double* resp, const double* means,
                                 const double* thresholds, int T, double* nk_out, double* corr_out, double* probs_out,
                                 int device, int io, void* stream) {
  if (B < 1 || N < 1 || K < 1 || T < 0 || !X || !nk_out || !corr_out)
    return qce_set_error(QCE_EARG, "quant_moments: bad arguments");
  if (N > 256) return qce_set_error(QCE_ENOTIMPL, "quant_moments: N <= 256");
  if (T > QM_MAX_T) return qce_set_error(QCE_ENOTIMPL, "quant_moments: at most 15 positive thresholds");
  if (!resp && K != 1) return qce_set_error(QCE_EARG, "quant_moments: resp NULL (unit weights) needs K = 1");
  if (T > 0 && (!thresholds || !probs_out))
    return qce_set_error(QCE_EARG, "quant_moments: T > 0 needs thresholds and probs_out");
  if (io != QCE_IO_HOST && io != QCE_IO_DEVICE) return qce_set_error(QCE_EARG, "quant_moments: bad io");
  QmThr thr{};
  for (int t = 0; t < T; ++t) {
    thr.t[t] = thresholds[t];
    if (!(thr.t[t] > 0.0) || (t > 0 && !(thr.t[t] > thr.t[t - 1])))
      return qce_set_error(QCE_EARG, "quant_moments: thresholds must be positive and ascending");
  }
  DeviceGuard g(device);
  hipStream_t st = (hipStream_t)stream;
  const QceEmPlan p = qce_em_plan(B, N, K, 0);  // the chunking of k_em_cov
  const int NPAD = N <= 64 ? 64 : N <= 128 ? 128 : 256;
  const int C = (int)((B + QM_CHUNK - 1) / QM_CHUNK), S = C * (256 / NPAD);
  const size_t nX = (size_t)B * N, nR = (size_t)B * K, nM = (size_t)K * N, nC = nM * N, nP = nM * T * 2;
  // scratch and host-I/O staging: owned for the length of this call, freed under the device guard
  DevBuf<double> scratch, dR, dnk, dprobs;
  DevBuf<double2> dX, dmu, dcorr;
  HIPCHK(scratch.ensure(2 * p.part_elems + (size_t)S * K + (size_t)S * nP));  // one allocation: part | pnk | pp
  double2* part = reinterpret_cast<double2*>(scratch.p);
  double* pnk = scratch.p + 2 * p.part_elems;
  double* pp = pnk + (size_t)S * K;
  const double2* x = (const double2*)X;
  const double* r = resp;
  const double2* mu = (const double2*)means;
  double *nk = nk_out, *probs = probs_out;
  double2* corr = (double2*)corr_out;
  if (io == QCE_IO_HOST) {
    HIPCHK(dX.ensure(nX));
    HIPCHK(hipMemcpyAsync(dX.p, X, sizeof(double2) * nX, hipMemcpyHostToDevice, st));
    x = dX.p;
    if (resp) {
      HIPCHK(dR.ensure(nR));
      HIPCHK(hipMemcpyAsync(dR.p, resp, sizeof(double) * nR, hipMemcpyHostToDevice, st));
      r = dR.p;
    }
    if (means) {
      HIPCHK(dmu.ensure(nM));
      HIPCHK(hipMemcpyAsync(dmu.p, means, sizeof(double2) * nM, hipMemcpyHostToDevice, st));
      mu = dmu.p;
    }
    HIPCHK(dnk.ensure(K));
    HIPCHK(dcorr.ensure(nC));
    HIPCHK(dprobs.ensure(nP));
    nk = dnk.p;
    corr = dcorr.p;
    probs = dprobs.p;
  }
  if (NPAD == 64) launch_probs<64>(B, N, K, T, C, thr, x, r, mu, pnk, pp, st);
  else if (NPAD == 128) launch_probs<128>(B, N, K, T, C, thr, x, r, mu, pnk, pp, st);
  else launch_probs<256>(B, N, K, T, C, thr, x, r, mu, pnk, pp, st);
  hipLaunchKernelGGL(k_qm_probs_final, dim3(K, T ? (T * 2 * N + 63) / 64 : 1), dim3(256), 0, st, S, N, K, T, pnk, pp,
                     nk, probs);
  hipLaunchKernelGGL(k_qm_corr, dim3(K, p.C2, p.nblk), dim3(256), 0, st, (long long)B, N, K, p.NT, p.chunk, x, r, mu,
                     part);
  long long gf = ((long long)nC + 255) / 256;
  if (gf > 4096) gf = 4096;
  hipLaunchKernelGGL(k_qm_corr_final, dim3((unsigned)gf), dim3(256), 0, st, p.C2, N, K, part, nk, corr);
  HIPCHK(hipGetLastError());
  if (io == QCE_IO_HOST) {
    HIPCHK(hipMemcpyAsync(nk_out, nk, sizeof(double) * K, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(corr_out, corr, sizeof(double2) * nC, hipMemcpyDeviceToHost, st));
    if (T > 0) HIPCHK(hipMemcpyAsync(probs_out, probs, sizeof(double) * nP, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));  // the scratch above is freed on return
  return QCE_OK;
}
