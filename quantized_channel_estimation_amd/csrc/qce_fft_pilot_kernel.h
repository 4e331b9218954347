// Fourier-domain path for (block-)circulant mixtures observed through A = kron(x, I_N), 2 <= P <= 4 pilots
// (QCE_OPT_FOURIER_PILOTS; DESIGN.md "Fourier path with pilots").
//
// With C_k = F^H diag(c_k) F and y seen as P segments y_p of length N (spectra Y_p = F y_p), every covariance of
// _prepare_for_prediction (gmm_cplx_bussgang.py:246-328) decouples per DFT bin i into a P x P Hermitian block:
//   d_kp = |x_p|^2 C_k[0,0] + s2 (diagonal of Cy_k, constant per pilot block), g_kp = gain(d_kp), a_k = g_k . x;
//   inf bits: R(i) = c_i x x^H + s2 I;  multi-bit: R(i) = b^2 (c_i x x^H + s2 I) + (1 - b^2) diag(d_k),
//   b = clip(mean_p g_kp, 0, 1);  1 bit: R(i)[p][q] = DFT2(arcsine law of the first column of block (p, q) of Cy_k)[i];
//   lp_k = -PN log(pi) - sum_i log det R(i) + log w_k - sum_i e_i^H G(i) e_i,  G = R^-1, e_i = Y(i) - a_k mu~_k,i;
//   h = F^H sum_k gamma_k [ mu~_k + c_k . (a_k^H G e) ].
// As tables this is the A = I design (qce_fft.hip) with wider rows.  Per bin the quadratic form is a real product
// over P^2 features of the observation -- |Y_p|^2 and, for p < q, Re / Im of conj(Y_p) Y_q -- against G_pp,
// 2 Re G_pq, -2 Im G_pq, plus 2 P features Re / Im Y_p against -2 u, u = G a mu~, when the model has means.  The
// filter is f_p,i = sum_k gamma_k w_k,p,i with the row w_k(i) = c_i a_k^H G(i), then
// Z_i = sum_p Y_p,i f_p,i + sum_k gamma_k b_k,i,  b_k,i = mu~_k,i (1 - w_k(i) a_k),  h = F^H Z.
// The DFT normalisations are folded into the tables (the LDS transforms are unnormalised).
//
// Tables (FP64, components padded to Kp = 16 ceil(K / 16); padded components hold zeros and c' = -inf):
//   tabL[kb][t][i][16]   lp operand: component block kb, feature type t < TL = P^2 (+ 2 P), bin i, component in block
//   tabW[ib][t][k][16]   filter operand: bin block ib, column type t < TF = 2 P (+ 2), component k, bin in block
// so that one v_mfma_f64_16x16x4_f64 A operand (16 rows x 4 k-steps) is 512 contiguous bytes.
//
// k_fftp_prep<P>: one workgroup per component, one thread per bin factorises R(i) in registers (Cholesky).
// k_fftp_est<P, HM, OUT>: one workgroup (4 waves) per tile of 16 observations, spectra of all P segments in LDS.
#pragma once
#include "qce_common.h"
#include "qce_fft_lds.h"
#include "qce_kernels.h"

namespace {

template <int P>
__global__ __launch_bounds__(256) void k_fftp_prep(QceFftpPrepArgs a) {
  constexpr int NPAIR = P * (P + 1) / 2;
  const int k = blockIdx.x, tid = threadIdx.x;
  const int N = a.N, Kp = a.Kp;
  const int TL = P * P + (a.has_mean ? 2 * P : 0), TF = 2 * P + (a.has_mean ? 2 : 0);
  double* tl = a.tabL + ((long long)(k >> 4) * TL * N) * 16 + (k & 15);  // + (t N + i) 16
  double* tf = a.tabW + (long long)k * 16;                               // + ((ib TF + t) Kp) 16 + ii
  auto tf_at = [&](int t, int i) -> double& { return tf[((long long)((i >> 4) * TF + t) * Kp) * 16 + (i & 15)]; };
  if (k >= a.K) {  // padding of the last component block
    for (int i = tid; i < N; i += 256) {
      for (int t = 0; t < TL; ++t) tl[((long long)t * N + i) * 16] = 0.0;
      for (int t = 0; t < TF; ++t) tf_at(t, i) = 0.0;
    }
    if (tid == 0) a.cprime[k] = QCE_NEG_INF;
    return;
  }
  __shared__ double2 rho[NPAIR * 256];  // 1 bit: arcsine law of the first columns of the blocks (p >= q)
  __shared__ double red[256];
  __shared__ double redm[256];
  __shared__ int s_bad;
  const double* c = a.ceig + (long long)k * N;
  const double2* cc = a.col0 + (long long)k * N;
  const double2* ms = a.mspec + (long long)k * N;
  const double s2 = a.s2;
  double d[P], g[P];
  double2 av[P];
  double gm = 0.0;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    d[p] = (a.x[p].x * a.x[p].x + a.x[p].y * a.x[p].y) * cc[0].x + s2;  // the diagonal of Cy_k in pilot block p
    g[p] = bussgang_gain(d[p], a.kind, a.n_bits, a.quant_kind, a.delta, a.thr, a.lab);
    av[p] = cscale(a.x[p], g[p]);
    gm += g[p];
  }
  gm /= (double)P;
  if (tid == 0) s_bad = 0;
  const double PI2 = 2.0 / PI_D;
  if (a.kind == 0) {
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q <= p; ++q) {
        const double2 xx = cmulc(a.x[p], a.x[q]);
        const double nrm = sqrt(d[p] * d[q]);
        for (int m = tid; m < N; m += 256) {
          double2 v = cmul(xx, cc[m]);
          if (p == q && m == 0) v.x += s2;
          double re = v.x / nrm, im = v.y / nrm;
          re = re > 1.0 ? 1.0 : (re < -1.0 ? -1.0 : re);
          im = im > 1.0 ? 1.0 : (im < -1.0 ? -1.0 : im);
          rho[(p * (p + 1) / 2 + q) * 256 + m] = make_double2(PI2 * asin(re), PI2 * asin(im));
        }
      }
  }
  __syncthreads();
  double beta2 = 0.0;
  if (a.kind == 1) {
    const double bt = gm < 0.0 ? 0.0 : (gm > 1.0 ? 1.0 : gm);
    beta2 = bt * bt;
  }
  const double isq = 1.0 / sqrt((double)N), invN = 1.0 / (double)N;
  double ldet = 0.0, mq = 0.0;
  for (int i = tid; i < N; i += 256) {
    // R(i), lower triangle
    double2 R[P][P];
    if (a.kind == 0) {
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) R[p][q] = make_double2(0.0, 0.0);
      for (int m = 0; m < N; ++m) {
        const double2 w = unit_root(dft_phase(i, m, a.n1, a.n2), N);
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int q = 0; q <= p; ++q) R[p][q] = cfma(rho[(p * (p + 1) / 2 + q) * 256 + m], w, R[p][q]);
      }
    } else {
      const double sc = a.kind == 2 ? 1.0 : beta2;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = 0; q <= p; ++q) {
          double2 v = cscale(cmulc(a.x[p], a.x[q]), c[i]);
          if (p == q) v.x += s2;
          v = cscale(v, sc);
          if (p == q && a.kind == 1) v.x += (1.0 - beta2) * d[p];
          R[p][q] = v;
        }
    }
    // Cholesky R = L L^H in registers; a non-positive pivot: Cr_k is not positive definite
    double2 L[P][P];
    double Ld[P];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      double sum = R[j][j].x;
#pragma unroll
      for (int t = 0; t < j; ++t) sum -= L[j][t].x * L[j][t].x + L[j][t].y * L[j][t].y;
      if (!(sum > 0.0)) bad = true;
      ldet += log(sum);
      Ld[j] = sqrt(sum);
      const double inv = 1.0 / Ld[j];
#pragma unroll
      for (int r = j + 1; r < P; ++r) {
        double2 v = R[r][j];
#pragma unroll
        for (int t = 0; t < j; ++t) v = csub(v, cmulc(L[r][t], L[j][t]));
        L[r][j] = cscale(v, inv);
      }
    }
    if (bad) atomicOr(&s_bad, 1);
    // Li = L^-1 (lower), G = R^-1 = Li^H Li
    double2 Li[P][P];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      Li[j][j] = make_double2(1.0 / Ld[j], 0.0);
#pragma unroll
      for (int r = j + 1; r < P; ++r) {
        double2 v = make_double2(0.0, 0.0);
#pragma unroll
        for (int t = j; t < r; ++t) v = cfma(L[r][t], Li[t][j], v);
        Li[r][j] = cscale(v, -1.0 / Ld[r]);
      }
    }
    double2 G[P][P];
#pragma unroll
    for (int p = 0; p < P; ++p)
#pragma unroll
      for (int q = 0; q < P; ++q) {
        double2 v = make_double2(0.0, 0.0);
#pragma unroll
        for (int t = (p > q ? p : q); t < P; ++t) v = cadd(v, cmulc(Li[t][q], Li[t][p]));  // conj(Li[t][p]) Li[t][q]
        G[p][q] = v;
      }
    // mean terms: t = a mu~, u = G t; filter row w = c_i a^H G; bias b = mu~ (1 - w a)
    const double2 mu = ms[i];
    double2 tv[P], u[P], wv[P];
#pragma unroll
    for (int p = 0; p < P; ++p) tv[p] = cmul(av[p], mu);
    double2 wa = make_double2(0.0, 0.0);
#pragma unroll
    for (int p = 0; p < P; ++p) {
      double2 us = make_double2(0.0, 0.0), ws = make_double2(0.0, 0.0);
#pragma unroll
      for (int q = 0; q < P; ++q) {
        us = cfma(G[p][q], tv[q], us);
        ws = cadd(ws, cmulc(G[q][p], av[q]));  // conj(a_q) G[q][p]
      }
      u[p] = us;
      wv[p] = cscale(ws, c[i]);
      mq += tv[p].x * us.x + tv[p].y * us.y;  // Re conj(t_p) u_p
      wa = cfma(wv[p], av[p], wa);
    }
#pragma unroll
    for (int p = 0; p < P; ++p) {
      tl[((long long)p * N + i) * 16] = G[p][p].x * invN;
      tf_at(2 * p, i) = wv[p].x * invN;
      tf_at(2 * p + 1, i) = wv[p].y * invN;
    }
    {
      int t = P;
#pragma unroll
      for (int p = 0; p < P; ++p)
#pragma unroll
        for (int q = p + 1; q < P; ++q) {
          tl[((long long)t * N + i) * 16] = 2.0 * G[p][q].x * invN;
          tl[((long long)(t + 1) * N + i) * 16] = -2.0 * G[p][q].y * invN;
          t += 2;
        }
    }
    if (a.has_mean) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        tl[((long long)(P * P + 2 * p) * N + i) * 16] = -2.0 * u[p].x * isq;
        tl[((long long)(P * P + 2 * p + 1) * N + i) * 16] = -2.0 * u[p].y * isq;
      }
      const double2 b = cmul(mu, make_double2(1.0 - wa.x, -wa.y));
      tf_at(2 * P, i) = b.x * isq;
      tf_at(2 * P + 1, i) = b.y * isq;
    }
  }
  red[tid] = ldet;
  redm[tid] = mq;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      redm[tid] += redm[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    a.cprime[k] = -((double)(P * N) * log(PI_D)) - red[0] + a.logw[k] - redm[0];
    a.status[k] = s_bad;
  }
}

// OUT: 0 = 'all' estimate h, 1 = lp only (B x K), 2 = weighted estimate with the selection weights wts (B x K, from
// k_select).  HM: the model has means (2 P more lp features per bin, the bias columns of the filter).
// LDS: 128 twiddles | spectra, 16 P rows of N + 1 (row s P + p = segment p of observation s) | lp / weights,
// 16 x (Kp + 1) | 512 doubles of reduction scratch.
template <int P, bool HM, int OUT>
__global__ __launch_bounds__(256) void k_fftp_est(QceFftpEstArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TL = P * P + (HM ? 2 * P : 0), TF = 2 * P + (HM ? 2 : 0);
  const int N = a.N, K = a.K, Kp = a.Kp, KP = Kp + 1, RS = N + 1;
  double2* tw = reinterpret_cast<double2*>(smem);
  double2* T = tw + 128;
  double* Lp = reinterpret_cast<double*>(T + 16 * P * RS);
  double* red = Lp + 16 * KP;
  const int tid = threadIdx.x;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const int s = lane & 15, q = lane >> 4;  // MFMA lane map: column (observation) s, k-step / row group q
  const long long b0 = (long long)blockIdx.x * 16;
  const int rows = (int)((a.B - b0) < 16 ? (a.B - b0) : 16);
  twiddles(tw);
  {  // tile of observations -> LDS: 16 P contiguous rows of N
    const double2* yt = a.y + b0 * P * N;
    for (int e = tid; e < 16 * P * N; e += 256) {
      const int r = e / N;
      T[r * RS + e % N] = (r < rows * P) ? yt[e] : make_double2(0.0, 0.0);
    }
  }
  __syncthreads();
  fft2(T, 16 * P, N, a.n1, a.n2, false, tw, RS);  // Y_p = sqrt(N) F y_p (unnormalised DFT)

  if (OUT != 2) {
    // lp[s][k] = c'_k - sum_f feat[s][f] tabL[f][k]: rows = 16 components of a block, columns = observations,
    // one MFMA k-step = 4 consecutive bins of one feature type; the wave takes every fourth component block
    for (int kb = wv; kb < (Kp >> 4); kb += 4) {
      f64x4 acc = {0.0, 0.0, 0.0, 0.0};
      const double* tb = a.tabL + ((long long)kb * TL * N + q) * 16 + s;
      for (int i0 = 0; i0 < N; i0 += 4) {
        double2 Y[P];
#pragma unroll
        for (int p = 0; p < P; ++p) Y[p] = T[(s * P + p) * RS + i0 + q];
        const double* ti = tb + (long long)i0 * 16;
#pragma unroll
        for (int p = 0; p < P; ++p) acc = mfma16x16x4d(ti[(long long)p * N * 16], Y[p].x * Y[p].x + Y[p].y * Y[p].y, acc);
        int t = P;
#pragma unroll
        for (int p = 0; p < P; ++p)
#pragma unroll
          for (int r = p + 1; r < P; ++r) {  // conj(Y_p) Y_r
            acc = mfma16x16x4d(ti[(long long)t * N * 16], Y[p].x * Y[r].x + Y[p].y * Y[r].y, acc);
            acc = mfma16x16x4d(ti[(long long)(t + 1) * N * 16], Y[p].x * Y[r].y - Y[p].y * Y[r].x, acc);
            t += 2;
          }
        if (HM) {
#pragma unroll
          for (int p = 0; p < P; ++p) {
            acc = mfma16x16x4d(ti[(long long)(P * P + 2 * p) * N * 16], Y[p].x, acc);
            acc = mfma16x16x4d(ti[(long long)(P * P + 2 * p + 1) * N * 16], Y[p].y, acc);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {  // D row = q + 4 r (component in block), column = s
        const int k = kb * 16 + q + 4 * r;
        Lp[s * KP + k] = a.cprime[k] - acc[r];
      }
    }
    __syncthreads();
    if (OUT == 1) {
      for (int e = tid; e < rows * K; e += 256) a.lp[b0 * K + e] = Lp[(e / K) * KP + e % K];
      return;
    }
    // FP64 softmax over k < K, 16 threads per observation (as k_fft_est); padded components get weight 0
    const int so = tid & 15, go = tid >> 4;
    const int kpt = (K + 15) / 16, k0 = go * kpt, k1 = (k0 + kpt < K) ? k0 + kpt : K;
    double mx = QCE_NEG_INF;
    for (int k = k0; k < k1; ++k) mx = fmax(mx, Lp[so * KP + k]);
    red[go * 16 + so] = mx;
    __syncthreads();
    mx = QCE_NEG_INF;
    for (int g = 0; g < 16; ++g) mx = fmax(mx, red[g * 16 + so]);
    double sm = 0.0;
    for (int k = k0; k < k1; ++k) {
      const double lpv = Lp[so * KP + k];
      const double e = (lpv == QCE_NEG_INF) ? 0.0 : exp(lpv - mx);
      Lp[so * KP + k] = e;
      sm += e;
    }
    red[256 + go * 16 + so] = sm;
    __syncthreads();
    sm = 0.0;
    for (int g = 0; g < 16; ++g) sm += red[256 + g * 16 + so];
    const double inv = 1.0 / sm;
    for (int k = k0; k < k1; ++k) Lp[so * KP + k] *= inv;
    for (int e = tid; e < 16 * (Kp - K); e += 256) Lp[(e / (Kp - K)) * KP + K + e % (Kp - K)] = 0.0;
  } else {
    for (int e = tid; e < 16 * Kp; e += 256) {
      const int r = e / Kp, k = e % Kp;
      Lp[r * KP + k] = (r < rows && k < K) ? a.wts[(b0 + r) * K + k] : 0.0;
    }
  }
  __syncthreads();
  // filter: columns c of tabW (rows of D) = 16 bins of one type, k-steps = 4 components; the wave takes every fourth
  // bin block.  Lane (s, q) ends with bins ib 16 + q + 4 r of observation s: Z = sum_p Y_p f_p + bias, into segment 0.
  for (int ib = wv; ib < (N >> 4); ib += 4) {
    f64x4 acc[TF];
#pragma unroll
    for (int t = 0; t < TF; ++t) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* tb = a.tabW + ((long long)ib * TF * Kp + q) * 16 + s;
    for (int k0 = 0; k0 < Kp; k0 += 4) {
      const double gam = Lp[s * KP + k0 + q];
      const double* tk = tb + (long long)k0 * 16;
#pragma unroll
      for (int t = 0; t < TF; ++t) acc[t] = mfma16x16x4d(tk[(long long)t * Kp * 16], gam, acc[t]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int i = ib * 16 + q + 4 * r;
      double2 z = HM ? make_double2(acc[2 * P][r], acc[2 * P + 1][r]) : make_double2(0.0, 0.0);
#pragma unroll
      for (int p = 0; p < P; ++p) z = cfma(T[(s * P + p) * RS + i], make_double2(acc[2 * p][r], acc[2 * p + 1][r]), z);
      T[(s * P) * RS + i] = z;
    }
  }
  __syncthreads();
  fft2(T, 16, N, a.n1, a.n2, true, tw, P * RS);  // h = F^H Z over the segment-0 rows (normalisation in the tables)
  double2* ht = a.h + b0 * N;
  for (int e = tid; e < rows * N; e += 256) ht[e] = T[(e / N) * P * RS + e % N];
}

}  // namespace
